"""
Reference, restatement and error bound for the PCA filter (csrc/cm2_pca.hip, include/cosmomap2.h f2g), and the cases
the CPU and the GPU tests share.  Plain NumPy, no GPU.

  * ``cov_ref``: the covariance of every (chunk, group) unit in np.longdouble, with S_ab = sum_i |x_a,i| |x_b,i|.
    Acceptance: any order of an L-term dot product obeys |err| <= gamma_L S, so the bound is
    (L + 2) 2^-53 S_ab 1.01 with L the chunk length (the rule of _vector_ref.c_gemm_tn: derived, not measured; it
    holds whether or not the MFMA fuses), and exactly 0 where S_ab = 0.
  * apply, fit and status: the library's unit is cm2_cmode.hip's with the modes of the sample's chunk, so the
    restatement is ``_cmode_ref.cmode_f64`` / ``cmode_ref`` called per chunk on that chunk's columns with that
    chunk's modes (imported, not copied).
  * ``select_modes``: ``learn``'s eigenvalue selection and sign rule, restated.
  * ``work_items`` / ``slabs``: the tables of cm2_pca_policy.h by brute-force enumeration.
  * ``quality``: the detection-quality case (24 detectors in 2 groups, 4 x 1024 samples, a rank-2 1/f atmosphere at
    1000 x the white noise, 5 % random flags, K = 2) and the whole pipeline on the host.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _cmode_ref as C
import _vector_ref as V

LD, U53, _ld, bits = V.LD, V.U53, V._ld, V.bits

# cm2_pca_policy.h
THREADS, MAX_K, MFMA, MFMA_K, TILE, WAVE_TILE, STEP, PITCH, SEGMENT = 256, 10, 16, 4, 128, 64, 16, 18, 4096
LDS_BYTES = 2 * TILE * PITCH * 8
FITTED, EMPTY, FEW, PIVOT = C.FITTED, C.EMPTY, C.FEW, C.PIVOT
TAU = C.TAU


# ------------------------------------------------------------------- covariance ----
def cov_ref(d, pix, ndet, gedges, cedges):
    """-> (cov, S): lists [chunk][group] of [n, n] np.longdouble arrays.  pix None: every sample is used."""
    ns = len(d) // ndet
    x = _ld(d).reshape(ndet, ns)
    if pix is not None:
        x = np.where(np.asarray(pix).reshape(ndet, ns) < 0, LD(0), x)       # a flagged sample's value is never read
    cov, S = [], []
    with np.errstate(all="ignore"):
        for c0, c1 in zip(cedges[:-1], cedges[1:]):
            cov.append([])
            S.append([])
            for g0, g1 in zip(gedges[:-1], gedges[1:]):
                xs = np.ascontiguousarray(x[g0:g1, c0:c1])
                cov[-1].append(xs @ xs.T)
                S[-1].append(np.abs(xs) @ np.abs(xs).T)
    return cov, S


def cov_bound(L, S):
    return LD(L + 2) * U53 * _ld(S) * LD(1.01)


def cov_excess(got, ref, S, L):
    """max |got - ref| / bound over a unit; where S = 0 the result must be exactly 0.  NaN anywhere gives inf."""
    got, ref = _ld(got), _ld(ref)
    err, bound = np.abs(got - ref), cov_bound(L, S)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(got == 0, LD(0), LD(np.inf)))
    ratio = np.where(np.isnan(ratio), LD(np.inf), ratio)
    return float(ratio.max())


def cov_offsets(gedges, nchunks):
    """off(c, g) = c sum n^2 + sum_{g' < g} n^2 -> [nchunks][G]"""
    sq = np.concatenate([[0], np.cumsum(np.diff(gedges) ** 2)])
    return [[int(c * sq[-1] + sq[g]) for g in range(len(gedges) - 1)] for c in range(nchunks)]


# ------------------------------------------------------------ policy, brute force ----
def work_items(gedges, cedges):
    """every (unit, row tile, column tile <= row tile, segment) the covariance needs, found by visiting every entry
    (a >= b) of every unit and every sample of every chunk: a dict from
    (unit, row0, col0, first sample) -> [len, rows, cols]"""
    G = len(gedges) - 1
    items = {}
    for c, (c0, c1) in enumerate(zip(cedges[:-1], cedges[1:])):
        firsts = {}
        for i in range(c0, c1):
            f = c0 + (i - c0) // SEGMENT * SEGMENT
            firsts[f] = firsts.get(f, 0) + 1
        for g, (g0, g1) in enumerate(zip(gedges[:-1], gedges[1:])):
            for a in range(g0, g1):
                ra = g0 + (a - g0) // TILE * TILE
                for b in range(g0, a + 1):
                    rb = g0 + (b - g0) // TILE * TILE
                    for f, n in firsts.items():
                        key = (c * G + g, ra, rb, f)
                        if key not in items:
                            items[key] = [n, min(TILE, g1 - ra), min(TILE, g1 - rb)]
    return items


def slabs(cedges):
    """the apply slabs by visiting every sample: a list of (first, len, chunk) in sample order"""
    out = []
    for c, (c0, c1) in enumerate(zip(cedges[:-1], cedges[1:])):
        for i in range(c0, c1):
            if (i - c0) % THREADS == 0:
                out.append([i, 0, c])
            out[-1][1] += 1
    return [tuple(s) for s in out]


def policy_status(ns, ndet, gedges, cedges, K):
    """cm2::pca::check restated: 0 ok, 1 K, 2 sizes, 3 group edges, 4 chunk edges, 5 too large"""
    G, Cn = len(gedges) - 1, len(cedges) - 1
    if K < 1 or K > MAX_K:
        return 1
    if ns < 1 or ndet < 1 or G < 1 or Cn < 1:
        return 2
    if not C.F.edges_ok(gedges, ndet):
        return 3
    if not C.F.edges_ok(cedges, ns):
        return 4
    if ndet >= 1 << 31 or ndet > (1 << 46) // ns or ndet > 1 << 23 or Cn > 1 << 16:
        return 5
    lim = (1 << 31) - 1
    pairs = sum((-(-n // TILE)) * (-(-n // TILE) + 1) // 2 for n in np.diff(gedges).tolist())
    segs = sum(-(-ln // SEGMENT) for ln in np.diff(cedges).tolist())
    sl = sum(-(-ln // THREADS) for ln in np.diff(cedges).tolist())
    cov = Cn * sum(n * n for n in np.diff(gedges).tolist())
    if pairs > lim // segs or G > lim // sl or -(-cov // THREADS) > lim:
        return 5
    return 0


# ------------------------------------------------------ apply, fit, status: per chunk ----
def _per_chunk(fn, pix, ndet, gedges, cedges, modes, v):
    ns = len(pix) // ndet
    pix2, v2 = np.asarray(pix).reshape(ndet, ns), np.asarray(v).reshape(ndet, ns)
    return [fn(np.ascontiguousarray(pix2[:, a:b]).reshape(-1), ndet, gedges, np.asarray(modes)[c],
               np.ascontiguousarray(v2[:, a:b]).reshape(-1)) for c, (a, b) in enumerate(zip(cedges[:-1], cedges[1:]))]


def _join(parts, ndet, names):
    out = SimpleNamespace()
    for nm in names:
        arrs = [np.asarray(getattr(p, nm)) for p in parts]
        if arrs[0].ndim == 1:                                           # [ndet ns_c] -> [ndet ns]
            setattr(out, nm, np.concatenate([a.reshape(ndet, -1) for a in arrs], axis=1).reshape(-1))
        else:                                                           # [..., ns_c]
            setattr(out, nm, np.concatenate(arrs, axis=-1))
    return out


def pca_f64(pix, ndet, gedges, cedges, modes, v):
    """the float64 restatement: out [ndet ns], coeff [G, K, ns], status [G, ns]"""
    return _join(_per_chunk(C.cmode_f64, pix, ndet, gedges, cedges, modes, v), ndet,
                 ("out", "coeff", "status", "ratio", "near"))


def pca_ref(pix, ndet, gedges, cedges, modes, v):
    """the np.longdouble reference with its magnitudes: out, S [ndet ns], coeff, Sc [G, K, ns], status [G, ns]"""
    return _join(_per_chunk(C.cmode_ref, pix, ndet, gedges, cedges, modes, v), ndet,
                 ("out", "S", "coeff", "Sc", "status", "ratio", "near"))


# --------------------------------------------------------------------- the modes ----
def select_modes(cov, K):
    """(modes [n, K], eigenvalues [n] descending): the eigenvectors of the K largest eigenvalues of cov, each with
    the sign that makes its component of largest magnitude (the first on a tie) positive"""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.arange(len(w))[::-1]
    out = np.zeros((len(w), K))
    for j in range(K):
        col = v[:, order[j]]
        top = 0
        for k in range(len(col)):
            if abs(col[k]) > abs(col[top]):
                top = k
        out[:, j] = -col if col[top] < 0 else col
    return out, w[order].copy()


def learn(cov, ndet, gedges, K):
    """modes [nchunks, ndet, K] from the covariances [chunk][group]"""
    modes = np.zeros((len(cov), ndet, K))
    for c, row in enumerate(cov):
        for g, unit in enumerate(row):
            modes[c, gedges[g]:gedges[g + 1]] = select_modes(unit, K)[0]
    return modes


# ------------------------------------------------------------------ linear gap fill ----
def linear_fill(d, ok, ndet, nedge=32):
    """utilities.fill_gaps_linear restated for one block per detector: every run of flagged samples becomes the line
    between the means of the valid samples among the nedge samples on either side"""
    ns = len(d) // ndet
    out = np.array(d, dtype=np.float64).reshape(ndet, ns).copy()
    ok = np.asarray(ok).reshape(ndet, ns)
    for k in range(ndet):
        i = 0
        while i < ns:
            if ok[k, i]:
                i += 1
                continue
            s = i
            while i < ns and not ok[k, i]:
                i += 1
            ln = i - s
            level = []
            for lo, hi in ((max(0, s - nedge), s), (i, min(ns, i + nedge))):
                sel = ok[k, lo:hi]
                level.append(out[k, lo:hi][sel].mean() if sel.any() else None)
            L, R = level
            L = R if L is None else L
            R = L if R is None else R
            if L is None:
                L = R = 0.0
            for j in range(ln):
                out[k, s + j] = L + (R - L) * (j + 1) / (ln + 1)
    return out.reshape(-1)


# ------------------------------------------------------------------- quality case ----
Q_NDET, Q_GEDGES, Q_CHUNK, Q_NCHUNKS, Q_K, Q_SEED = 24, (0, 12, 24), 1024, 4, 2, 20260
Q_FLAG_RATE, Q_ATM = 0.05, 1000.0


def one_over_f(rng, n):
    """a time stream of unit variance whose amplitude spectrum falls as 1/f (power as 1/f^2)"""
    f = np.fft.rfftfreq(n)
    amp = np.zeros_like(f)
    amp[1:] = 1.0 / f[1:]
    x = np.fft.irfft(amp * (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size)), n)
    return x / x.std()


@functools.lru_cache(maxsize=None)
def quality():
    """the data of the quality case: d = noise (unit variance) + a rank-2 atmosphere whose detector pattern (gains
    and a gradient over each group) drifts from chunk to chunk"""
    rng = np.random.default_rng(Q_SEED)
    ndet, ns = Q_NDET, Q_CHUNK * Q_NCHUNKS
    gedges, cedges = np.array(Q_GEDGES, dtype=np.int64), np.arange(Q_NCHUNKS + 1, dtype=np.int64) * Q_CHUNK
    noise = rng.standard_normal((ndet, ns))
    t1, t2 = one_over_f(rng, ns), one_over_f(rng, ns)
    gain, slope = rng.uniform(0.7, 1.3, ndet), rng.uniform(-1.0, 1.0, ndet)
    atm = np.zeros((ndet, ns))
    for c in range(Q_NCHUNKS):
        a, b = cedges[c], cedges[c + 1]
        g_c = gain * (1.0 + 0.05 * c * rng.uniform(-1.0, 1.0, ndet))
        s_c = slope + 0.1 * c * rng.uniform(-1.0, 1.0, ndet)
        atm[:, a:b] = Q_ATM * (np.outer(g_c, t1[a:b]) + 0.5 * np.outer(s_c, t2[a:b]))
    ok = rng.random((ndet, ns)) >= Q_FLAG_RATE
    pix = np.where(ok, rng.integers(0, 500, ok.shape), -1).astype(np.int32).reshape(-1)
    return SimpleNamespace(ndet=ndet, ns=ns, gedges=gedges, cedges=cedges, K=Q_K, noise=noise.reshape(-1),
                           d=(noise + atm).reshape(-1), ok=ok.reshape(-1), pix=pix)


def rms_over_noise(q, filtered):
    """rms of the unflagged samples of `filtered` over the rms of the noise on the same samples"""
    return float(np.sqrt(np.mean(np.asarray(filtered)[q.ok] ** 2)) / np.sqrt(np.mean(q.noise[q.ok] ** 2)))


def cov_f64(d, pix, ndet, gedges, cedges):
    """the covariances in float64 (NumPy's own order): for the host pipeline of the quality case only"""
    ns = len(d) // ndet
    x = np.asarray(d, dtype=np.float64).reshape(ndet, ns)
    if pix is not None:
        x = np.where(np.asarray(pix).reshape(ndet, ns) < 0, 0.0, x)
    return [[x[g0:g1, c0:c1] @ x[g0:g1, c0:c1].T for g0, g1 in zip(gedges[:-1], gedges[1:])]
            for c0, c1 in zip(cedges[:-1], cedges[1:])]


@functools.lru_cache(maxsize=None)
def quality_on_the_host():
    """-> SimpleNamespace(unfiltered, zero_filled, gap_filled): rms over noise of the stream itself and of the stream
    filtered with modes learnt from the zero-filled stream and from the linear gap fill with every sample used"""
    q = quality()
    run = lambda modes: rms_over_noise(q, pca_f64(q.pix, q.ndet, q.gedges, q.cedges, modes, q.d).out)
    zero = learn(cov_f64(q.d, q.pix, q.ndet, q.gedges, q.cedges), q.ndet, q.gedges, q.K)
    filled = linear_fill(q.d, q.ok, q.ndet)
    full = learn(cov_f64(filled, None, q.ndet, q.gedges, q.cedges), q.ndet, q.gedges, q.K)
    return SimpleNamespace(unfiltered=rms_over_noise(q, q.d), zero_filled=run(zero), gap_filled=run(full))
