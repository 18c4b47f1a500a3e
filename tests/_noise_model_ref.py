"""
References, restatements and error bounds for the noise-model kernels (csrc/cm2_noise_model.hip): the Welch
PSD per noise block (k_psd_pack, rocFFT, k_psd_accumulate, k_psd_finish) and the PSD -> band step
(k_bands_spectrum<0> | k_bands_spectrum<1> and k_bands_cos_table of csrc/cm2_psd_bands.h, k_bands_lags around that
header's cos_sum).

Plain NumPy, no GPU, nothing of the package.

  * ``welch_ref``: Welch per block in extended precision (np.longdouble): segments of L samples every L/2, the
    segment's mean subtracted for detrend = 'constant', periodic Hann window, a direct L x (L/2+1) DFT whose
    phase j k mod L is reduced in integers before the cosine and sine (the quarter points are exact),
    P_k = m_k sum_s |X_s(k)|^2 / (K_b fs sum w^2).
  * ``psd_bound``: the error scale of a PSD bin.  n_s = ||w . src_s||_2 is the window times the RAW segment
    (before the mean is subtracted: that covers the subtraction and its cancellation), e_s = c 2^-53 n_s,

        E_{b,k} = m_k / (K_b fs sum w^2) sum_s (2 |X_s(k)| e_s + e_s^2).

    A PSD is accepted when |got - ref| <= E_{b,k} for EVERY bin; where E = 0 the result must be exactly 0.
    (The impulses of the `impulses` input sit where the window is 1/2 or more: n_s does not see a mean
    carried by a sample that the window removes.)
  * ``welch_f64``: a float64 restatement of the kernels' formulas (the mean by the kernel's tree, |X|^2 added
    in segment order, the last factor formed as the kernel forms it), np.fft.rfft standing in for rocFFT.
    NOT bit-equal to the GPU.  What it loses against the reference, WORST_PSD below (measured with c = 1),
    times the project's headroom of 8 for an FFT with another radix schedule, rounded up to a power of two,
    is the constant c of the PSD bound (``c_psd``).
  * ``bands_ref``: S_k = P_k fs / m_k, S_0 := S_1, G = 1/S | sqrt(S),
    c_j = (G_0 + (-1)^j G_{L/2} + 2 sum_{k=1}^{L/2-1} G_k cos(2 pi (j k mod L) / L)) / L, a_j = (1 - j/lam) c_j,
    in np.longdouble, with its error scale

        B_j = (1 - j/lam) (|G_0| + |G_{L/2}| + 2 sum_k |G_k|) / L.

    A band is accepted when |got - ref| <= C_LAG(L) 2^-53 B_j for every lag.  The constant is derived, not
    measured.  k_bands_lags adds n = L/2 - 1 products g_k t_k serially in increasing k (cos_sum).  To first order, in
    units of 2^-53 of |G_k| (|t| <= 1): G_k carries 2 (the product with fs and the division | square root;
    the division by m_k is exact), a table entry good to two ulps 4, the product 1, the serial sum at most
    n - 1 (its first term), the addition to G_0 + (-1)^j G_{L/2} 1 (the factor 2 and the division by L are
    exact), the taper 3 (j/lam, 1 - ., the product): n + 10.  The G_0 and Nyquist terms carry less.  With the
    project's 2 for the second-order terms and the reference's own roundings

        C_LAG(L) = (L/2 - 1) + 10 + 2 = L/2 + 11                     (139 at L = 256).

    ``bands_f64``, the float64 restatement with a correctly rounded table, uses WORST_LAG of it (random
    roundings add up like sqrt n, not n).
  * ``batch_geometry``: which segments of which blocks share a rocFFT batch of B segments.
  * ``PSD_MUTATIONS``, ``BAND_MUTATIONS``, ``subtle_psd``, ``subtle_band``: wrong kernels, as ``mut=`` of the
    restatements; tests/test_noise_model_ref_cpu.py shows that each fails the check that
    tests/test_gpu_noise_model_kernels.py applies.  The subtle ones are of the kind a norm cannot see: 1e-8 on
    the bins k >= L/4 of the `red` PSD is 1200 x the per-bin bound and moves rel_l2 over a block by 8e-13 at
    most; 1e-9 on the lags j >= lambda/2 of the `red` band at lambda = 128 is 0.044, 0.48 and 52 x the per-lag
    bound on the blocks with the knee at 0.1, 0.03 and 0.01 fs (with the knee at 0.1 fs the far lags are 1e-7 of
    B_j, and 1e-9 of them lies below the rounding of the sum itself) and moves rel_l2 by 5e-13.
"""
import functools
from collections import namedtuple

import numpy as np

from _vector_ref import LD, U53, bits, assert_bit_equal, pow2_at_least  # noqa: F401

_PI = 4 * np.arctan(LD(1))
K_BLOCK = 256                            # csrc/cm2_common.h: kBlock, the workgroup of every kernel here
K_BATCH_SAMPLES = 1 << 24                # csrc/cm2_noise_model.hip: kBatchSamples


# ------------------------------------------------------------------- geometry ----
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def seg_counts(sizes, L):
    """K_b = (n_b - L) // (L/2) + 1"""
    return [(int(n) - L) // (L // 2) + 1 for n in sizes]


def seg_offsets(sizes, L):
    """cm2_psd_welch: segments are numbered block after block"""
    return offsets(seg_counts(sizes, L))


def tails(sizes, L):
    """samples of every block behind its last segment (ignored)"""
    return [int(n) - (L + (K - 1) * (L // 2)) for n, K in zip(sizes, seg_counts(sizes, L))]


def per_segment_bytes(L):
    """psd_build: a segment's doubles and its transform"""
    return 8 * L + 16 * (L // 2 + 1)


Batch = namedtuple("Batch", "first real pad blocks whole")


def batch_geometry(sizes, L, B):
    """The batches of cm2_psd_welch for B segments per batch: `first` segment, `real` segments and `pad` zero
    segments, `blocks` = [(b, s0, s1)]: the segments [s0, s1) of block b that k_psd_accumulate adds in this
    batch, `whole` = the blocks that lie in it entirely."""
    so = seg_offsets(sizes, L)
    nseg, out = int(so[-1]), []
    for first in range(0, nseg, B):
        last = min(first + B, nseg)
        blocks = [(b, max(int(so[b]), first), min(int(so[b + 1]), last)) for b in range(len(sizes))
                  if so[b] < last and so[b + 1] > first]
        whole = [b for b, s0, s1 in blocks if s0 == so[b] and s1 == so[b + 1]]
        out.append(Batch(first, last - first, first + B - last, blocks, whole))
    return out


def geometry_facts(sizes, L, B):
    """-> what the batch boundaries of B segments do to the blocks"""
    so = seg_offsets(sizes, L)
    geo = batch_geometry(sizes, L, B)
    seen = {}
    for i, bt in enumerate(geo):
        for b, _, _ in bt.blocks:
            seen.setdefault(b, []).append(i)
    return dict(straddle=any(len(v) > 1 for v in seen.values()),
                boundary_on_block=any(bt.first > 0 and bt.first in so[1:-1] for bt in geo),
                two_whole=any(len(bt.whole) >= 2 for bt in geo),
                padded_last=geo[-1].pad > 0)


# --------------------------------------------------------------- tables in LD ----
@functools.lru_cache(maxsize=None)
def cos_table_ld(L):
    """cos(2 pi m / L), m < L, np.longdouble, exact at the quarter points"""
    t = np.cos(2 * _PI * np.arange(L, dtype=LD) / LD(L))
    t[[0, L // 4, L // 2, 3 * L // 4]] = [1, 0, -1, 0]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _dft_ld(L):
    """(cos, -sin)(2 pi (j k mod L) / L) as L x (L/2+1)"""
    t = cos_table_ld(L)
    ph = (np.arange(L, dtype=np.int64)[:, None] * np.arange(L // 2 + 1, dtype=np.int64)[None, :]) % L
    return t[ph], -t[(ph - L // 4) % L]


@functools.lru_cache(maxsize=None)
def hann_ld(L):
    """periodic Hann: 1/2 - 1/2 cos(2 pi j / L)"""
    return LD(0.5) - LD(0.5) * cos_table_ld(L)


def m_of(L):
    m = np.full(L // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    return m


# ------------------------------------------------------------------ PSD cases ----
PSD_SIZES = {
    256: (256, 383, 384, 511, 512, 1400, 256),     # 1, 1, 2, 2, 3, 9, 1 segments; tails 127, 127, 120
    512: (512, 1279, 1280),                        # 1, 3, 4 segments: two samples per thread in the mean
}
PSD_INPUTS = ("white", "red", "tone", "impulses", "offset")
PSD_FS = (1.0, 20.0)
TONE_BIN = {256: 37, 512: 74}
# unit impulses (times the block's scale) per block, counted from the block's start: where the window of
# every segment that holds them is >= 1/2, and in the ignored tails (block 1 of L = 256 has nothing else:
# its PSD is exactly zero)
IMPULSES = {
    256: ((64,), (300,), (192,), (64, 500), (320,), (1088, 1280, 1399), (192,)),
    512: ((128,), (640, 1024, 1278), (1152,)),
}
# (`red`: a draw whose every block has the dynamic range of 1e6 that its case is there for, asserted in
# tests/test_noise_model_ref_cpu.py)
_SEED = {"white": 8101, "red": 8128, "tone": 8135, "impulses": 8152, "offset": 8169}


def block_scale(b):
    return 10.0 ** (3 * (b % 3))


def red_spectrum(f):
    """S(f) = 1 + (0.1 / f)^3.5, f > 0"""
    return 1.0 + (0.1 / f) ** 3.5


@functools.lru_cache(maxsize=None)
def psd_input(L, inp):
    sizes = PSD_SIZES[L]
    off = offsets(sizes)
    nt = int(off[-1])
    rng = np.random.default_rng(_SEED[inp] + L)
    i = np.arange(nt, dtype=np.int64)
    if inp == "white":
        x = rng.standard_normal(nt)
    elif inp == "red":                     # circulant draw with the two-sided spectrum S, zero mean
        f = np.fft.rfftfreq(nt)
        S = np.zeros(f.size)
        S[1:] = red_spectrum(f[1:])
        X = np.sqrt(nt * S / 2.0) * (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size))
        x = np.fft.irfft(X, nt)
    elif inp == "tone":                    # exactly on a bin in every segment, whatever its start
        x = 3.0 * np.cos(2.0 * np.pi * ((TONE_BIN[L] * i) % L) / L + 0.3)
    elif inp == "impulses":
        x = np.zeros(nt)
        for b, places in enumerate(IMPULSES[L]):
            x[off[b] + np.asarray(places)] = block_scale(b)
    else:
        assert inp == "offset"
        x = rng.standard_normal(nt) + 1e6 + 1e-3 * i
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ reference ----
def welch_parts(x, sizes, L, detrend):
    """-> per block (|X_s(k)| [K_b, L/2+1], n_s [K_b]), np.longdouble"""
    C, Sn = _dft_ld(L)
    w = hann_ld(L)
    off, half = offsets(sizes), L // 2
    x = np.asarray(x, dtype=LD)
    parts = []
    for b, K in enumerate(seg_counts(sizes, L)):
        src = np.stack([x[off[b] + s * half:off[b] + s * half + L] for s in range(K)])
        ns = np.sqrt(((w * src) ** 2).sum(axis=1))
        y = (src - src.mean(axis=1, keepdims=True) if detrend else src) * w
        re, im = y @ C, y @ Sn
        parts.append((np.sqrt(re * re + im * im), ns))
    return parts


def _psd_factor(L, K, fs):
    """m_k / (K fs sum w^2), sum w^2 = 3 L / 8"""
    return np.asarray(m_of(L), dtype=LD) / (LD(K) * LD(fs) * (LD(3 * L) / 8))


def welch_ref(parts, L, fs):
    return np.stack([_psd_factor(L, len(ns), fs) * (ax * ax).sum(axis=0) for ax, ns in parts])


def psd_bound(parts, L, fs, c):
    """E_{b,k} (np.longdouble)"""
    out = []
    for ax, ns in parts:
        e = (LD(c) * U53 * ns)[:, None]
        out.append(_psd_factor(L, len(ns), fs) * (2 * ax * e + e * e).sum(axis=0))
    return np.stack(out)


def ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; <= 1 passes.  Where bound = 0 the result must be exact
    (ratio 0 or inf).  NaN anywhere gives inf."""
    got, ref, bound = (np.asarray(a, dtype=LD).reshape(-1) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, LD(0), LD(np.inf)))
    r = np.where(np.isnan(r), LD(np.inf), r)
    return float(r.max())


PsdCase = namedtuple("PsdCase", "L inp detrend fs sizes x parts ref")


@functools.lru_cache(maxsize=None)
def _parts_of(L, inp, detrend):
    return welch_parts(psd_input(L, inp), PSD_SIZES[L], L, detrend)


@functools.lru_cache(maxsize=None)
def psd_case(L, inp, detrend, fs):
    """One shared case, evaluated once; nobody writes to it."""
    parts = _parts_of(L, inp, bool(detrend))
    ref = welch_ref(parts, L, fs)
    ref.setflags(write=False)
    return PsdCase(L, inp, bool(detrend), float(fs), PSD_SIZES[L], psd_input(L, inp), parts, ref)


def psd_keys(L=None, detrend=None):
    return [(l, inp, d, fs) for l in sorted(PSD_SIZES) for d in (True, False) for inp in PSD_INPUTS for fs in PSD_FS
            if (L is None or l == L) and (detrend is None or d == bool(detrend))]


def psd_share(got, cs, c=None):
    """largest |got - ref| / E over the bins of every block"""
    c = c_psd(cs.L, cs.detrend) if c is None else c
    return ratio(got, cs.ref, psd_bound(cs.parts, cs.L, cs.fs, c))


def dynamic_range(cs):
    """max / min over the bins, per block"""
    p = np.asarray(cs.ref, dtype=np.float64)
    return p.max(axis=1) / p.min(axis=1)


# ---------------------------------------------------------- PSD: restatement ----
@functools.lru_cache(maxsize=None)
def _window_f64(L, symmetric=False):
    """psd_build: the window and the serial sum of its squares"""
    j = np.arange(L, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / float(L - 1 if symmetric else L))
    s2 = 0.0
    for v in w:
        s2 += v * v
    return w, s2


def _mean_f64(src):
    """k_psd_pack: thread t adds its samples t, t + 256, ... in order; wave_sum halves 64 lanes five times and
    once more; the four waves are added in order; / L"""
    L = src.size
    v = src.reshape(L // K_BLOCK, K_BLOCK)
    s = np.zeros(K_BLOCK)
    for row in v:
        s = s + row
    s = s.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        s[:, :o] = s[:, :o] + s[:, o:2 * o]
    return (((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0]) / float(L)


PSD_MUTATIONS = {
    # name -> the case on which it must exceed the bound
    "window_symmetric": (256, "white", True, 1.0),
    "nyquist_doubled": (256, "white", True, 20.0),
    "tail_segment_counted": (256, "white", False, 1.0),
    "block_mean": (256, "offset", True, 1.0),
    "hop_off_by_one": (512, "white", True, 1.0),
    "last_segment_into_next": (256, "white", True, 1.0),
    "batch_first_dropped": (256, "red", True, 1.0),
    "k_plus_one": (512, "red", False, 20.0),
}
MUT_BATCH = 3                              # batch_first_dropped: segments per batch


def welch_f64(x, sizes, L, fs, detrend, mut=None):
    """k_psd_pack, R2C transform, k_psd_accumulate, k_psd_finish in float64"""
    assert mut is None or mut in PSD_MUTATIONS, mut
    w, wsum2 = _window_f64(L, symmetric=(mut == "window_symmetric"))
    off, so, half, nfreq = offsets(sizes), seg_offsets(sizes, L), L // 2, L // 2 + 1
    x = np.asarray(x, dtype=np.float64)
    xz = np.concatenate([x, np.zeros(L)])                # (what a mutation reads behind the stream)
    m = m_of(L)
    if mut == "nyquist_doubled":
        m[-1] = 2.0
    psd = np.zeros((len(sizes), nfreq))
    for b, K in enumerate(seg_counts(sizes, L)):
        hop = half - 1 if mut == "hop_off_by_one" else half
        starts = [int(off[b]) + s * hop for s in range(K)]
        if mut == "last_segment_into_next":
            starts[-1] += 1
        acc = np.zeros(nfreq)
        for s, o in enumerate(starts):
            src = xz[o:o + L]
            mean = 0.0
            if detrend:
                mean = float(np.mean(x[off[b]:off[b + 1]])) if mut == "block_mean" else _mean_f64(src)
            if mut == "batch_first_dropped" and (so[b] + s) % MUT_BATCH == 0 and so[b] + s > 0:
                continue
            F = np.fft.rfft((src - mean) * w)
            acc = acc + (F.real * F.real + F.imag * F.imag)
        if mut == "tail_segment_counted" and tails(sizes, L)[b] > 0:
            src = np.zeros(L)
            t = tails(sizes, L)[b]
            src[:half + t] = x[off[b + 1] - half - t:off[b + 1]]
            F = np.fft.rfft((src - (_mean_f64(src) if detrend else 0.0)) * w)
            acc = acc + (F.real * F.real + F.imag * F.imag)
            K += 1
        if mut == "k_plus_one":
            K += 1
        psd[b] = acc * (m / (float(K) * fs * wsum2))
    return psd


def subtle_psd(psd, L):
    """a relative error of 1e-8 on the bins k >= L/4: a copy"""
    out = np.array(psd, dtype=np.float64)
    out[..., L // 4:] *= 1.0 + 1e-8
    return out


SUBTLE_PSD_CASE = (256, "red", True, 1.0)

# Largest |welch_f64 - ref| / E(c = 1) over the PSD cases, per (L, detrend), rounded up to one decimal
# (tests/test_noise_model_ref_cpu.py re-measures them and fails when they are stale)
WORST_PSD = {(256, True): 29.0, (256, False): 18.5, (512, True): 92.8, (512, False): 80.0}


def c_psd(L, detrend):
    return pow2_at_least(8.0 * WORST_PSD[(L, bool(detrend))])


def round_up(v):
    return float(np.ceil(v * 10.0 - 1e-9) / 10.0)


def measure_worst_psd():
    worst = {}
    for key in psd_keys():
        cs = psd_case(*key)
        e = psd_share(welch_f64(cs.x, cs.sizes, cs.L, cs.fs, cs.detrend), cs, c=1)
        worst[(cs.L, cs.detrend)] = max(worst.get((cs.L, cs.detrend), 0.0), e)
    return worst


# ----------------------------------------------------------------- band cases ----
BAND_L, BAND_NB = 256, 3
BAND_LAMS = (1, 2, 7, 128)                 # 3, 6, 21, 384 threads: the last crosses a workgroup
INVERSE, SQRT = 0, 1
MODES = (INVERSE, SQRT)
MODE_NAMES = {INVERSE: "inverse", SQRT: "sqrt"}
ONE_BINS = {"onebin_a": (1, 2, 63), "onebin_b": (64, 127, 128)}
BAND_PSDS = ("red", "rough") + tuple(sorted(ONE_BINS))
BAND_FS = {"red": 1.0, "rough": 20.0, "onebin_a": 1.0, "onebin_b": 1.0}
GARBAGE = (float("nan"), -1.0, float("inf"))     # what bin 0 may hold
RED_KNEES = (0.1, 0.03, 0.01)              # of the three blocks of `red` and `rough`, in units of fs


@functools.lru_cache(maxsize=None)
def band_psd(name, mode):
    """[3, L/2+1] one-sided PSDs.  `red`: m_k / fs (1 + b) (1 + (fk_b / f)^3.5) with a bin 0 of its own (0.3);
    `rough`: red times a random factor per bin; one-bin PSDs: inverse mode 1 at k0 and 1e200 elsewhere,
    sqrt mode 0 elsewhere."""
    L, fs = BAND_L, BAND_FS[name]
    f = np.fft.rfftfreq(L, 1.0 / fs)
    P = np.empty((BAND_NB, L // 2 + 1))
    if name in ONE_BINS:
        P[:] = 1e200 if mode == INVERSE else 0.0
        for b, k0 in enumerate(ONE_BINS[name]):
            P[b, k0] = 1.0
    else:
        for b, fk in enumerate(RED_KNEES):
            P[b, 1:] = m_of(L)[1:] / fs * (1.0 + b) * (1.0 + (fk * fs / f[1:]) ** 3.5)
            P[b, 0] = 0.3
        if name == "rough":
            P *= np.exp(np.random.default_rng(8300).standard_normal(P.shape))
    P.setflags(write=False)
    return P


def with_bin0(P, v):
    out = np.array(P)
    out[:, 0] = v
    return out


def _G_ld(psd, L, fs, mode):
    S = np.asarray(psd, dtype=LD) * LD(fs) / np.asarray(m_of(L), dtype=LD)
    S[:, 0] = S[:, 1]
    return 1 / S if mode == INVERSE else np.sqrt(S)


def bands_ref(psd, lam, fs, mode):
    """-> (a [nb, lam], B [nb, lam]) in np.longdouble; bin 0 of the PSD is never read"""
    psd = np.atleast_2d(psd)
    L = 2 * (psd.shape[1] - 1)
    G = _G_ld(psd, L, fs, mode)
    t = cos_table_ld(L)
    j = np.arange(lam, dtype=np.int64)
    k = np.arange(1, L // 2, dtype=np.int64)
    cosjk = t[(j[:, None] * k[None, :]) % L]                                  # [lam, L/2 - 1]
    sign = np.where(j & 1, LD(-1), LD(1))
    c = (G[:, :1] + sign[None, :] * G[:, -1:] + 2 * (G[:, 1:-1] @ cosjk.T)) / LD(L)
    taper = 1 - j.astype(LD) / LD(lam)
    A1 = (np.abs(G[:, 0]) + np.abs(G[:, -1]) + 2 * np.abs(G[:, 1:-1]).sum(axis=1)) / LD(L)
    return taper[None, :] * c, taper[None, :] * A1[:, None]


def C_LAG(L):
    return L // 2 + 11


BandCase = namedtuple("BandCase", "name mode lam fs psd ref B")


@functools.lru_cache(maxsize=None)
def band_case(name, mode, lam):
    P = band_psd(name, mode)
    ref, B = bands_ref(P, lam, BAND_FS[name], mode)
    for a in (ref, B):
        a.setflags(write=False)
    return BandCase(name, mode, lam, BAND_FS[name], P, ref, B)


def band_keys():
    return [(n, mode, lam) for mode in MODES for n in BAND_PSDS for lam in BAND_LAMS]


def band_share(got, cs):
    """largest |got - ref| / (C_LAG 2^-53 B_j) over every lag of every block"""
    L = 2 * (cs.psd.shape[1] - 1)
    return ratio(got, cs.ref, LD(C_LAG(L)) * U53 * cs.B)


# -------------------------------------------------------- bands: restatement ----
BAND_MUTATIONS = {
    # name -> (psd, mode, lambda) on which it must exceed the bound
    "phase_not_reduced": ("red", INVERSE, 7),
    "nyquist_sign_plus": ("red", SQRT, 2),
    "taper_lam_minus_1": ("rough", INVERSE, 7),
    "bin0_used": ("red", INVERSE, 1),
    "dc_m_one": ("rough", SQRT, 1),
}


@functools.lru_cache(maxsize=None)
def _cos_table_f64(L):
    return np.asarray(cos_table_ld(L), dtype=np.float64)       # correctly rounded; the GPU's is cospi


def bands_f64(psd, lam, fs, mode, mut=None):
    """k_bands_spectrum<0> | k_bands_spectrum<1>, k_bands_cos_table, k_bands_lags in float64 (the sum over k serial and
    increasing, as in the kernel)"""
    assert mut is None or mut in BAND_MUTATIONS, mut
    psd = np.atleast_2d(np.asarray(psd, dtype=np.float64))
    nfreq = psd.shape[1]
    L = 2 * (nfreq - 1)
    kk = np.arange(nfreq)
    kk[0] = 1
    m = np.where(kk == nfreq - 1, 1.0, 2.0)
    with np.errstate(all="ignore"):
        S = psd[:, kk] * fs / m
        if mut == "bin0_used":
            S[:, 0] = psd[:, 0] * fs / 1.0
        if mut == "dc_m_one":
            S[:, 0] = psd[:, 1] * fs / 1.0
        G = 1.0 / S if mode == INVERSE else np.sqrt(S)
        tab = _cos_table_f64(L)
        j = np.arange(lam, dtype=np.int64)
        acc = np.zeros((psd.shape[0], lam))
        for k in range(1, nfreq - 1):
            ph = np.minimum(j * k, L - 1) if mut == "phase_not_reduced" else (j * k) % L
            acc = acc + G[:, k, None] * tab[ph][None, :]
        odd = (j & 1).astype(bool) & (mut != "nyquist_sign_plus")
        nyq = np.where(odd[None, :], -G[:, -1:], G[:, -1:])
        c = (G[:, :1] + nyq + 2.0 * acc) / float(L)
        lam_t = lam - 1 if mut == "taper_lam_minus_1" else lam
        return (1.0 - j.astype(np.float64) / float(lam_t))[None, :] * c


def subtle_band(bands):
    """a relative error of 1e-9 on the lags j >= lam/2: a copy"""
    out = np.array(bands, dtype=np.float64)
    out[:, out.shape[1] // 2:] *= 1.0 + 1e-9
    return out


SUBTLE_BAND_CASE = ("red", INVERSE, 128)

# Largest |bands_f64 - ref| / (C_LAG 2^-53 B_j) over the band cases, per mode, rounded up to two decimals
# (re-measured by tests/test_noise_model_ref_cpu.py)
WORST_LAG = {INVERSE: 0.03, SQRT: 0.05}


def round_up2(v):
    return float(np.ceil(v * 100.0 - 1e-9) / 100.0)


def measure_worst_lag():
    worst = {}
    for key in band_keys():
        cs = band_case(*key)
        e = band_share(bands_f64(cs.psd, cs.lam, cs.fs, cs.mode), cs)
        worst[cs.mode] = max(worst.get(cs.mode, 0.0), e)
    return worst
