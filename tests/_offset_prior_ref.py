"""
The offset prior of the destriper (csrc/cm2_offset_prior.hip, cosmomap2_amd/utilities/offset_prior.py) restated in
NumPy for test_offset_prior_cpu.py and test_gpu_offset_prior.py.  Nothing here imports the package under test.

Per block, from one row P_k (k = 0 .. n/2, n = nperseg) of a one-sided PSD, the baseline length L, the band length
lam, the relative floor and optionally the white variance sigma^2:

    1. S_k = P_k fs / m_k (m_k = 1 at k = 0 and n/2, else 2), S_0 := S_1
    2. sigma^2 = (4/n) sum_{k = n/4}^{n/2 - 1} S_k when none is given
    3. R_k = max(S_k - sigma^2, 0)
    4. q_j = (1/n) sum_{k = 0}^{n/2} m_k R_k D_k cos(w_k L j), j < K = floor((n/2 + 1) / L), w_k = 2 pi k / n,
       D_k = sin^2(L w_k / 2) / (L^2 sin^2(w_k / 2)), D_0 = 1
    5. Q_i = q~_0 + 2 sum_{j = 1}^{K-1} q~_j cos(2 pi i j / M), q~_j = (1 - j/K) q_j, i <= M/2, M = next_pow2(2K)
    6. H_i = 1 / max(Q_i, floor sigma^2 / L)
    7. band_i = (1 - i/lam) (1/M) sum_{k = 0}^{M/2} m'_k H_k cos(2 pi i k / M), i < lam <= M/2

``prior(..., dtype=LD)`` is the reference in np.longdouble, ``prior(..., dtype=np.float64)`` the float64 restatement
in the kernels' operation order (sums by cumsum: strictly in increasing index order).  In both the angles are reduced
in integers and the cosines and sines are rounded from np.longdouble, as cospi / sinpi of the reduced angle are on
the GPU.

The forward error bound (``Result.band_err``, ``Result.sigma2_err``), with u = 2^-53, to first order, evaluated on the
reference's values.  A sum of N terms t_k computed in any order from inputs with errors e_k:

    |err| <= (N + C) u sum |t_k| + sum e_k,       C = 8 for the roundings of a term's own factors and the division

and for the stages

    S      eS = 2 u S                                             the product with fs
    sigma  e_sigma = (4/n) ((n/4 + C) u sum S_k + sum eS_k)         0 when sigma^2 is given
    R      eR = eS + e_sigma + u |S - sigma^2|                      max(., 0) does not amplify
    D      relative CD u, CD = 24: two sinpi of at most 2 ulp (4 u) each, squared (9 u each), the product with L^2
           (exact) and sd^2 (u), the division (u), rounded up
    W      W = m R D:  eW = m D (eR + CD u R) + 2 u W
    q      eq_j = ((n/2 + 1 + C) u sum |W_k c_jk| + sum (eW_k |c_jk| + 2 u W_k)) / n     (2 u: the cosine, absolute)
    q~     eqt_j = (1 - j/K) eq_j + 3 u |q~_j|
    Q      eQ_i = (K + C) u (|q~_0| + 2 sum |q~_j c_ij|) + eqt_0 + 2 sum (eqt_j |c_ij| + 2 u |q~_j|)
    floor  f = floor sigma^2 / L:  ef = f (e_sigma / sigma^2 + 3 u)
    H      X = max(Q, f), eX = max(eQ, ef); H = 1 / X:  eH = H^2 eX + u H.  Where Q + eQ <= f - ef the computed Q is
           below the computed floor as well, so eX = ef there: the bound is never wider than H^2 max(eQ, ef) + u H.
    band   eb_i = (1 - i/lam) ((M/2 + 1 + C) u sum |m'_k H_k c_ik| + sum m'_k (eH_k |c_ik| + 2 u H_k)) / M
                  + 3 u |band_i|
"""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
U53 = LD(2) ** -53
C, CD = 8, 24
_PI = 4 * np.arctan(LD(1))


def geometry(n, L):
    """(K, M) of nperseg n and baseline length L."""
    K = (n // 2 + 1) // L
    return K, 1 << (2 * K - 1).bit_length()


def _cos2pi(num, den, dtype):
    """cos(2 pi num / den) for integer arrays 0 <= num < den, den a multiple of 4: the angle folded into [0, pi/2]
    in integers, evaluated in np.longdouble, rounded to dtype."""
    r = np.asarray(num, dtype=np.int64) % den
    r = np.where(r > den // 2, den - r, r)                   # [0, den/2]
    neg = r > den // 4
    r = np.where(neg, den // 2 - r, r)                       # [0, den/4]
    c = np.cos(2 * _PI * r.astype(LD) / LD(den))
    c = np.where(r == den // 4, LD(0), c)
    return np.where(neg, -c, c).astype(dtype)


def _sinpi(num, den, dtype):
    """sin(pi num / den) for integer arrays 0 <= num <= den/2."""
    num = np.asarray(num, dtype=np.int64)
    assert np.all((num >= 0) & (2 * num <= den))
    return np.sin(_PI * num.astype(LD) / LD(den)).astype(dtype)


def _seq_sum(terms):
    """Sum over the last axis, strictly in increasing index order."""
    return np.cumsum(terms, axis=-1)[..., -1]


def prior(P, L, lam, fs=1.0, sigma2=None, floor=1e-6, dtype=LD, bound=False):
    """One block.  -> SimpleNamespace(band [lam], sigma2, K, M, S, R, q (untapered), Q, H and, with bound=True,
    band_err [lam], sigma2_err)."""
    T = dtype
    P = np.asarray(P, dtype=np.float64)
    n = 2 * (P.size - 1)
    nf = n // 2 + 1
    K, M = geometry(n, L)
    assert K >= 2 and 1 <= lam <= M // 2
    m = np.full(nf, 2.0).astype(T)
    m[0] = m[-1] = 1
    S = P.astype(T) * T(fs) / m
    S[0] = S[1]
    assert np.all(np.isfinite(S) & (S > 0))
    given = sigma2 is not None
    hi = S[n // 4:n // 2]
    s2 = T(np.float64(sigma2)) if given else (T(4.0) / T(n)) * _seq_sum(hi)
    dS = S - s2
    R = np.where(dS > 0, dS, T(0))
    k = np.arange(nf, dtype=np.int64)
    a = (k * L) % n
    a = np.where(a > n // 2, n - a, a)
    sn, sd = _sinpi(a, n, T), _sinpi(k, n, T)
    Dk = np.ones(nf, dtype=T)
    Dk[1:] = (sn[1:] * sn[1:]) / ((T(L) * T(L)) * (sd[1:] * sd[1:]))
    W = (m * R) * Dk
    j = np.arange(K, dtype=np.int64)
    cq = _cos2pi((k[None, :] * L * j[:, None]) % n, n, T)                    # [K, nf]
    q = _seq_sum(W[None, :] * cq) / T(n)
    qt = (T(1) - j.astype(T) / T(K)) * q
    i = np.arange(M // 2 + 1, dtype=np.int64)
    cQ = _cos2pi((i[:, None] * j[None, 1:]) % M, M, T)                      # [M/2+1, K-1]
    Q = qt[0] + T(2) * _seq_sum(qt[None, 1:] * cQ)
    f = T(np.float64(floor)) * s2 / T(L)
    X = np.where(Q > f, Q, f)
    H = T(1) / X
    mp = np.full(M // 2 + 1, 2.0).astype(T)
    mp[0] = mp[-1] = 1
    ib = np.arange(lam, dtype=np.int64)
    cb = _cos2pi((ib[:, None] * i[None, :]) % M, M, T)                      # [lam, M/2+1]
    band = (T(1) - ib.astype(T) / T(lam)) * (_seq_sum((mp * H)[None, :] * cb) / T(M))
    out = SimpleNamespace(band=band, sigma2=s2, K=K, M=M, S=S, R=R, q=q, Q=Q, H=H, f=f)
    if bound:
        u = U53
        eS = 2 * u * S
        es = LD(0) if given else (LD(4) / n) * ((n // 4 + C) * u * np.abs(hi).sum() + eS[n // 4:n // 2].sum())
        eR = eS + es + u * np.abs(dS)
        eW = m * Dk * (eR + CD * u * R) + 2 * u * W
        eW[0] = m[0] * eR[0] + 2 * u * W[0]                                   # D_0 = 1 is exact
        acq = np.abs(cq)
        eq = ((nf + C) * u * (W[None, :] * acq).sum(axis=1) + (eW[None, :] * acq).sum(axis=1) + 2 * u * W.sum()) / n
        taper = 1 - j.astype(LD) / K
        eqt = taper * eq + 3 * u * np.abs(qt)
        acQ = np.abs(cQ)
        eQ = (K + C) * u * (abs(qt[0]) + 2 * (np.abs(qt[None, 1:]) * acQ).sum(axis=1)) + eqt[0] + \
            2 * ((eqt[None, 1:] * acQ).sum(axis=1) + 2 * u * np.abs(qt[1:]).sum())
        ef = f * (es / s2 + 3 * u)
        eX = np.where(Q + eQ <= f - ef, ef, np.maximum(eQ, ef))
        eH = H * H * eX + u * H
        acb = np.abs(cb)
        out.band_err = (1 - ib.astype(LD) / lam) * (
            (M // 2 + 1 + C) * u * ((mp * H)[None, :] * acb).sum(axis=1) +
            ((mp * eH)[None, :] * acb).sum(axis=1) + 2 * u * (mp * H).sum()) / M + 3 * u * np.abs(band)
        out.sigma2_err = es + u * s2
        out.floored = int(np.count_nonzero(Q <= f))
    return out


def priors(psd, L, lam, fs=1.0, sigma2=None, floor=1e-6, dtype=LD, bound=False):
    """Every row of psd [nb, n/2+1]; sigma2 None, a number or one per block."""
    psd = np.atleast_2d(psd)
    s = [None] * len(psd) if sigma2 is None else np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (len(psd),))
    return [prior(p, L, lam, fs, s[b], floor, dtype, bound) for b, p in enumerate(psd)]


def q_brute(R, n, L, K):
    """q_j = (1/L^2) sum_{|s| < L} (L - |s|) r_{|jL + s|}, r = irfft(R, n), in np.longdouble by the cosine sum."""
    R = np.asarray(R, dtype=LD)
    nf = n // 2 + 1
    m = np.full(nf, LD(2))
    m[0] = m[-1] = 1
    k = np.arange(nf, dtype=np.int64)
    lag = np.arange(n // 2 + 1, dtype=np.int64)
    r = (_cos2pi((lag[:, None] * k[None, :]) % n, n, LD) * (m * R)[None, :]).sum(axis=1) / n     # r_0 .. r_{n/2}
    q = np.zeros(K, dtype=LD)
    for j in range(K):
        for s in range(-(L - 1), L):
            assert abs(j * L + s) <= n // 2
            q[j] += (L - abs(s)) * r[abs(j * L + s)]
    return q / (LD(L) * L)


def toeplitz(band, size):
    """The dense symmetric banded Toeplitz block of `size` rows with the first row `band` (np.float64)."""
    band = np.asarray(band, dtype=np.float64)
    d = np.abs(np.arange(size)[:, None] - np.arange(size)[None, :])
    return np.where(d < band.size, band[np.minimum(d, band.size - 1)], 0.0)


# ------------------------------------------------------------------------------------ the inputs ------
def one_over_f(rng, nt, sigma=1.0, fknee=0.05, alpha=1.5):
    """Stationary noise of the two-sided PSD sigma^2 (1 + (fknee / f)^alpha) at fs = 1 (circulant, zero mean)."""
    f = np.fft.rfftfreq(nt)
    S = np.zeros_like(f)
    S[1:] = sigma ** 2 * (1.0 + (fknee / f[1:]) ** alpha)
    X = np.sqrt(nt * S) * (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size)) / np.sqrt(2.0)
    X[-1] = np.sqrt(nt * S[-1]) * rng.standard_normal()
    return np.fft.irfft(X, nt)


def welch(x, n, fs=1.0):
    """scipy.signal.welch(x, fs, 'hann', n, n/2, detrend='constant', scaling='density') in NumPy."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    acc = np.zeros(n // 2 + 1)
    nseg = (x.size - n) // (n // 2) + 1
    for s in range(nseg):
        seg = x[s * (n // 2):s * (n // 2) + n]
        acc += np.abs(np.fft.rfft((seg - seg.mean()) * w)) ** 2
    m = np.full(n // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    return acc * m / (nseg * fs * (w * w).sum())


def one_sided(S, fs=1.0):
    """The one-sided PSD row P_k = S_k m_k / fs of a per-sample spectrum S_k, k = 0 .. n/2."""
    m = np.full(S.size, 2.0)
    m[0] = m[-1] = 1.0
    return np.asarray(S, dtype=np.float64) * m / fs


def psd_inputs(n, fs=1.0):
    """The four PSD rows of the tests at nperseg n, as {name: (row, white variance of the construction)}:
    Welch PSDs of seeded 1/f noise (knee 0.05 fs, slope 1.5, unit white noise) and of seeded white noise of variance
    2.5 (32 n samples each), the flat spectrum S = 2.5 (every bin floored: band = L / (floor sigma^2) delta_i), and
    S_k = 1 + 40 / (1 + (16 k / n)^2) below n/8, 1 from there on (R is zero above n/8 once sigma^2 = 1)."""
    rng = np.random.default_rng(1000 + n)
    k = np.arange(n // 2 + 1)
    shaped = np.where(8 * k < n, 1.0 + 40.0 / (1.0 + (16.0 * k / n) ** 2), 1.0)
    return {
        "welch_1f": (welch(one_over_f(rng, 32 * n), n, fs), 1.0),
        "welch_white": (welch(np.sqrt(2.5) * rng.standard_normal(32 * n), n, fs), 2.5),
        "flat": (one_sided(np.full(n // 2 + 1, 2.5), fs), 2.5),
        "band_limited": (one_sided(shaped, fs), 1.0),
    }


# (nperseg, L, lam) of the tests: K = 129, M = 512 / K = 43, M = 128 / K = 3, M = 8 (lam 4 and 1) / K = 2, M = 4 /
# K = 13, M = 32
GEOMETRIES = [(256, 1, 256), (256, 3, 64), (256, 37, 4), (256, 37, 1), (256, 64, 2), (1024, 37, 16)]
