"""
The gap-aware GLS system restated in NumPy / SciPy for test_gap_aware_cpu.py and test_gpu_gap_aware.py.  Nothing
here imports the package under test.

    Q    = N^-1: per block the symmetric banded Toeplitz matrix of its band, zero boundary (scipy.sparse.diags)
    P    = pointing: row t is (1, cos 2phi_t, sin 2phi_t) at pixel pix[t], empty where pix[t] < 0
    E    = nt x ng, a one at (position of the j-th flagged sample, j);  P_e = [P E]
    A_e  = P_e^T Q P_e,   b_e = P_e^T Q d0 (d0 = d on V, 0 on G),   M_e = blockdiag(M_BD, 1 / a_0(block))
    S    = Q_VV - Q_VG Q_GG^-1 Q_GV, the inverse covariance of the valid samples alone

Bands: a positive PSD S_k = sigma^2 (1 + (f_knee / f_k)^1.5) on the rfft grid of length L (S_0 := S_1), c = irfft(1/S),
a_j = (1 - j / lambda) c_j -- the Bartlett taper makes the band's symbol 1/S smoothed by the Fejer kernel, so every
block is symmetric positive definite.
"""
import numpy as np
import scipy.signal as ss
import scipy.sparse as sp

WIN = 8192                                                   # time samples of one permutation window


def bands(lam, specs, L=None):
    """[len(specs), lam]: the band of every block from its (sigma, f_knee)."""
    if L is None:
        L = 256 if lam <= 128 else 8192
    assert lam <= L // 2
    f = np.fft.rfftfreq(L)
    out = []
    for sigma, fknee in specs:
        S = np.empty(f.size)
        S[1:] = sigma ** 2 * (1.0 + (fknee / f[1:]) ** 1.5)
        S[0] = S[1]
        c = np.fft.irfft(1.0 / S, L)[:lam]
        out.append((1.0 - np.arange(lam) / float(lam)) * c)
    return np.array(out)


def noise(sizes, specs, rng):
    """A noise stream of the modelled spectrum: per block, white noise coloured by sqrt(S) on the block's own rfft
    grid.  d = P m + noise(...) is then data of the model the solve assumes, so the gap part of the solution -- the
    conditional mean of that noise in the gaps -- has the noise's own amplitude, not that of a mismatched one."""
    out = []
    for n, (sigma, fknee) in zip(sizes, specs):
        f = np.fft.rfftfreq(n)
        S = np.empty(f.size)
        S[1:] = sigma ** 2 * (1.0 + (fknee / f[1:]) ** 1.5)
        S[0] = S[1]
        out.append(np.fft.irfft(np.sqrt(S) * np.fft.rfft(rng.standard_normal(n)), n))
    return np.concatenate(out)


def q_sparse(bnds, sizes):
    """N^-1 as a sparse matrix."""
    blocks = []
    for a, n in zip(bnds, sizes):
        k = min(len(a), n)
        offs = list(range(-(k - 1), k))
        blocks.append(sp.diags([np.full(n - abs(o), a[abs(o)]) for o in offs], offs, shape=(n, n), format="csr"))
    return sp.block_diag(blocks, format="csr")


def ninv(bnds, sizes, v):
    """N^-1 v without the matrix (any band length): per block the zero-boundary product with the symmetric band."""
    out, o = np.empty_like(v), 0
    for a, n in zip(bnds, sizes):
        out[o:o + n] = ss.fftconvolve(v[o:o + n], np.concatenate([a[:0:-1], a]), "same")
        o += n
    return out


def pointing(pix, phi, npix, pol):
    """P as a sparse nt x (pol npix) matrix, pixel-interleaved columns [I0, Q0, U0, I1, ...]."""
    t = np.flatnonzero(pix >= 0)
    p = pix[t].astype(np.int64)
    if pol == 1:
        rows, cols, vals = t, p, np.ones(t.size)
    else:
        comps = [np.ones(t.size), np.cos(2.0 * phi[t]), np.sin(2.0 * phi[t])][3 - pol:]
        rows = np.concatenate([t] * pol)
        cols = np.concatenate([pol * p + k for k in range(pol)])
        vals = np.concatenate(comps)
    return sp.csr_matrix((vals, (rows, cols)), shape=(pix.size, pol * npix))


def extended(P, pos):
    """P_e = [P E]."""
    nt = P.shape[0]
    E = sp.csr_matrix((np.ones(pos.size), (pos, np.arange(pos.size))), shape=(nt, pos.size))
    return sp.hstack([P, E], format="csr")


def block_of(sizes, t):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.searchsorted(off, t, side="right") - 1


def mbd_dense(P, w, npix, pol):
    """M_BD = per-pixel inverse of P^T diag(w) P (its pol x pol diagonal blocks), as a dense matrix."""
    D = (P.T @ sp.diags(w) @ P).toarray()
    M = np.zeros_like(D)
    for p in range(npix):
        s = slice(pol * p, pol * p + pol)
        M[s, s] = np.linalg.inv(D[s, s])
    return M


def system(bnds, sizes, pix, phi, npix, pol, d):
    """Everything dense about one case: a dict with A (A_e), b (b_e), M (M_e), P, Pe, Q, pos, nmap."""
    nt = pix.size
    pos = np.flatnonzero(pix < 0)
    Q = q_sparse(bnds, sizes)
    P = pointing(pix, phi, npix, pol)
    Pe = extended(P, pos)
    QPe = (Q @ Pe).tocsc()
    A = (Pe.T @ QPe).toarray()
    A = 0.5 * (A + A.T)
    d0 = np.where(pix < 0, 0.0, d)
    b = Pe.T @ (Q @ d0)
    a0 = np.array([a[0] for a in bnds])
    w = a0[block_of(sizes, np.arange(nt))]
    nmap = pol * npix
    M = np.zeros((nmap + pos.size, nmap + pos.size))
    M[:nmap, :nmap] = mbd_dense(P, w, npix, pol)
    M[np.arange(nmap, nmap + pos.size), np.arange(nmap, nmap + pos.size)] = 1.0 / w[pos]
    return dict(A=A, b=b, M=M, P=P, Pe=Pe, Q=Q, pos=pos, nmap=nmap, w=w, d0=d0)


def schur_map(sysd):
    """(P^T S P)^-1 P^T S d_V by eliminating the gap block of the dense A_e, b_e."""
    A, b, n = sysd["A"], sysd["b"], sysd["nmap"]
    if A.shape[0] == n:
        return np.linalg.solve(A, b)
    App, Apg, Agg = A[:n, :n], A[:n, n:], A[n:, n:]
    X = np.linalg.solve(Agg, np.column_stack([Apg.T, b[n:]]))
    return np.linalg.solve(App - Apg @ X[:, :-1], b[:n] - Apg @ X[:, -1])


def schur_dense(Q, pos):
    """S = Q_VV - Q_VG Q_GG^-1 Q_GV as a dense matrix on the valid samples, and their positions."""
    nt = Q.shape[0]
    valid = np.setdiff1d(np.arange(nt), pos)
    Qd = Q.toarray()
    Qvv, Qvg, Qgg = Qd[np.ix_(valid, valid)], Qd[np.ix_(valid, pos)], Qd[np.ix_(pos, pos)]
    return Qvv - Qvg @ np.linalg.solve(Qgg, Qvg.T), valid


def window_table(pos, nt):
    """c_w, w = 0 .. nwin: the number of flagged positions below w * 8192 (lower_bound per window)."""
    nwin = (nt + WIN - 1) // WIN
    return np.searchsorted(pos, np.arange(nwin + 1, dtype=np.int64) * WIN, side="left").astype(np.uint32)


# ------------------------------------------------------------------------------- the layouts ------
NT = 4 * WIN + 1234                                          # five permutation windows, the last one partial
SIZES = [14000, 20002]
SPECS = [(1.0, 0.02), (5.0, 0.05)]                           # (sigma, f_knee) of the two blocks
NT_SMALL, SIZES_SMALL = 5000, [3000, 2000]                   # below one window: the per-sample permutations


def long_run(lam):
    return 2 * lam + 5 if lam <= 128 else 300


def flags(lam, whole_window=False):
    """The flagged samples of the five-window layout, as a bool mask."""
    m = np.zeros(NT, dtype=bool)
    m[0:3] = True                                            # the stream's start
    m[3000:3000 + long_run(lam)] = True                      # longer than the band
    m[5000] = True                                           # isolated
    m[8152:8217] = True                                      # across a window end
    m[13995:14007] = True                                    # across the block boundary
    m[33000:33400:2] = True                                  # alternating
    m[NT - 4:] = True                                        # the stream's end
    if whole_window:
        m[3 * WIN:4 * WIN] = True                            # all of window 3
    assert not m[2 * WIN:3 * WIN].any()                      # nothing in window 2
    return m


def flags_small(lam):
    m = np.zeros(NT_SMALL, dtype=bool)
    m[0:3] = True
    m[1000:1000 + long_run(lam)] = True
    m[2500] = True
    m[2995:3007] = True                                      # across the block boundary
    m[4000:4100:2] = True
    m[NT_SMALL - 4:] = True
    return m


def scan(nt, npix, mask, seed):
    """(pix int32 with -1 where flagged, phi): uniform random pixels and angles."""
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, npix, nt).astype(np.int32)
    phi = rng.uniform(0.0, np.pi, nt)
    pix[mask] = -1
    return pix, phi
