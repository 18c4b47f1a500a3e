"""
Reference, restatement and error bounds for the Fourier filter (csrc/cm2_fourier.hip; include/cosmomap2.h, f2j).
The reference project has no counterpart: the definition in the header is the specification, and ``ref_ld`` is that
definition.

Plain NumPy, no GPU, nothing of the package.

  * ``Par``: the parameters of a filter (the arguments of cm2_fourier_create after the block sizes).
  * ``fft_length``: the transform length by brute force.
  * ``response_ld``: H_b at every bin in np.longdouble, with the quantities the bound needs.
  * ``ref_ld``: the definition in np.longdouble: the end means, the trend, the zero padding, a direct DFT whose phase
    (k i) mod L is reduced in integers before the cosine and sine (exact at 0 and L/2, and at the quarter points when 4
    divides L), the product with H, the direct real inverse, Re H(0) times the trend.  Products are summed pairwise.
  * The output error scale of a block, per sample (``error_scale``; ``ref_ld`` returns it too),

        E_i = 2^-53 log2(L) max_k |H_b(f_k)| ||xt||_2 + 2^-53 |H_b(0) l_i|.

    An output is accepted when |got - ref| <= c E_i for every sample.  A bad block must be all quiet NaN.
  * ``apply_f64``: the float64 restatement with np.fft (pocketfft standing in for rocFFT), NOT bit-equal to the GPU.
    WORST[L] is the largest |apply_f64 - ref_ld| / E over the blocks of transform length L of the shared cases
    (measured by tests/test_fourier_cpu.py on a CPU, never on a GPU; kept per length as _noise_model_ref.py keeps its
    own per segment length), and c(L) = pow2_at_least(8 WORST[L]): the project's headroom of 8 for an FFT whose
    factorisation differs from pocketfft's under the same log L law.
  * ``MUTATIONS``: wrong kernels, as ``mut=`` of ``apply_f64`` and ``response_f64``; tests/test_fourier_cpu.py shows
    that each breaks a bound the GPU test applies, on at least one shared case.  ``nyquist_imag`` is seen by the
    response bound only: a real inverse transform ignores the imaginary part of the Nyquist bin by definition, which
    is why the definition sets it to +0.0 instead of leaving it to the library.
  * ``response_bound``: the bound on |got - ref| of either part of H at a bin.  It is counted, not measured, in units
    of 2^-53 S with S = |T| g Rloc (Rloc: twice the largest |R| among the table entries around the bin, 1 without
    a table); |T|, g and R as in the header.
        f = (k fs) / L carries 2 roundings, u = ((2 pi) f) tau 2 more and the constant's own: 5.  mode 0: Im T = u,
        5.  mode 1: den = 1 + u u 12, 1 / den 13, -u / den 18: C_T = 18 when a tau is set.
        Butterworth of order p: the ratio 3, its square 7, the power 7 p + (p - 1), 1 + w one more (w / (1 + w) <= 1):
        8 p; the square root halves it and is allowed 2 ulp, the reciprocal and the product into g one each:
        C_B(p) = 4 p + 4.
        A notch: (pi / 2) a one rounding on the argument (below), the sine 2 ulp twice in the square, the square and the
        product into g one each: 6, relative to g_j.  The argument a = |f - f0| / w is NOT relative: f carries 2
        roundings relative to f, the difference one, the quotient one, the product with pi / 2 one, so
        |da| <= 2^-53 (2 f / w + 3 a) and |dg_j| <= (pi / 2) |sin(pi a)| |da|; this term is added as it is, times
        the other factors of S.
        Re T g, Im T g: 1.  The table: s carries 4 roundings, t = s - floor(s) is exact, R_r + t (R_{r+1} - R_r)
        three more relative to |R_r| + |R_{r+1}|: (4 s + 3) Rloc, added as it is times |T| g (it grows with Rn: a
        fine table is read at a position known to 4 ulp of s); the complex product 3.
        The project's 2 for the second-order terms and the reference's own roundings.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

from _vector_ref import LD, U53, bits  # noqa: F401

_PI = 4 * np.arctan(LD(1))
QUIET_NAN = 0x7FF8000000000000
SEGMENT = 4096                           # csrc/cm2_fourier_policy.h: kSegment
MAX_LENGTH = 1 << 28
BATCH_SAMPLES = 1 << 24


def pow2_at_least(r):
    """the smallest power of two (of either sign of exponent) >= r > 0"""
    return 2.0 ** math.ceil(math.log2(r))


# ------------------------------------------------------------------- lengths ----
def smooth7(v):
    for p in (2, 3, 5, 7):
        while v % p == 0:
            v //= p
    return v == 1


def fft_length(n, pad):
    L = max(2, n + pad)
    while L % 2 or not smooth7(L):
        L += 1
    return L


def row_bytes(L):
    return 8 * L + 16 * (L // 2 + 1)


def first_batch(L, blocks, max_work_bytes):
    batch = BATCH_SAMPLES // L
    if batch * row_bytes(L) > max_work_bytes:
        batch = max_work_bytes // row_bytes(L)
    return max(1, min(batch, blocks))


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


# ---------------------------------------------------------------- parameters ----
class Par(SimpleNamespace):
    """fs; tau: None or one per block; mode 0 deconvolve, 1 convolve; lp, hp: None or (fc, order); notch: [(f0, w)];
    table: None, [Rn] or [nblocks, Rn], real or complex; detrend 0 none, 1 ends; end_mean; pad; conjugate"""

    def __init__(self, fs=100.0, tau=None, mode=0, lp=None, hp=None, notch=(), table=None, detrend=1, end_mean=32,
                 pad=1024, conjugate=0):
        SimpleNamespace.__init__(self, fs=float(fs), tau=None if tau is None else np.asarray(tau, dtype=np.float64),
                                 mode=mode, lp=lp, hp=hp, notch=[tuple(map(float, nw)) for nw in notch],
                                 table=None if table is None else np.asarray(table), detrend=detrend,
                                 end_mean=end_mean, pad=pad, conjugate=conjugate)

    def but(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Par(**d)

    def tau_of(self, b):
        return 0.0 if self.tau is None else float(self.tau[b])

    def row_of(self, b):
        if self.table is None:
            return None
        return self.table if self.table.ndim == 1 else self.table[b]

    @property
    def table_kind(self):
        return 0 if self.table is None else 2 if np.iscomplexobj(self.table) else 1


# ------------------------------------------------------------------ response ----
def response_ld(P, b, L, conjugate=None):
    """-> SimpleNamespace(re, im: H_b at k = 0 .. L/2 in LD; S: the scale of the bound; extra: its absolute terms;
    count: its relative count)"""
    conjugate = P.conjugate if conjugate is None else conjugate
    k = np.arange(L // 2 + 1)
    f = k.astype(LD) * LD(P.fs) / LD(L)
    tau = LD(P.tau_of(b))
    count = LD(1 + 2)
    if tau == 0:
        tre, tim = np.ones_like(f), np.zeros_like(f)
    else:
        u = 2 * _PI * f * tau
        count += 18
        if P.mode == 0:
            tre, tim = np.ones_like(f), u
        else:
            tre, tim = 1 / (1 + u * u), -u / (1 + u * u)
    tabs = np.sqrt(tre * tre + tim * tim)
    factors = []                                                              # (g_j, absolute error of g_j)
    with np.errstate(divide="ignore", over="ignore"):
        if P.lp is not None:
            fc, p = P.lp
            factors.append((1 / np.sqrt(1 + (f / LD(fc)) ** (2 * p)), 0))
            count += 4 * p + 4
        if P.hp is not None:
            fc, q = P.hp
            g = np.zeros_like(f)
            g[1:] = 1 / np.sqrt(1 + (LD(fc) / f[1:]) ** (2 * q))
            factors.append((g, 0))
            count += 4 * q + 4
    for f0, w in P.notch:
        a = np.abs(f - LD(f0)) / LD(w)
        g = np.where(a < 1, np.sin(_PI / 2 * a) ** 2, LD(1))
        da = U53 * (2 * f / LD(w) + 3 * a)
        factors.append((g, np.where(a < 1, _PI / 2 * np.abs(np.sin(_PI * a)) * da, LD(0))))
        count += 6
    g = np.ones_like(f)
    for gj, _ in factors:
        g = g * gj
    extra = np.zeros_like(f)
    for j, (_, dgj) in enumerate(factors):
        others = np.ones_like(f)
        for i, (gi, _) in enumerate(factors):
            if i != j:
                others = others * gi
        extra = extra + others * dgj
    hre, him = tre * g, tim * g
    rloc = np.ones_like(f)
    row = P.row_of(b)
    if row is not None:
        Rn = row.size
        rr, ri = np.real(row).astype(LD), np.imag(row).astype(LD)
        s = f / (LD(P.fs) / 2) * (Rn - 1)
        i0 = np.minimum(np.floor(s).astype(np.int64), Rn - 2)
        t = s - i0
        vre, vim = rr[i0] + t * (rr[i0 + 1] - rr[i0]), ri[i0] + t * (ri[i0 + 1] - ri[i0])
        mag = np.sqrt(rr * rr + ri * ri)
        rloc = 2 * np.max([mag[np.clip(i0 + o, 0, Rn - 1)] for o in (-1, 0, 1, 2)], axis=0)
        table_extra = tabs * g * (4 * s + 3) * rloc * U53
        hre, him = hre * vre - him * vim, hre * vim + him * vre
        count += 3
    else:
        table_extra = 0
    if conjugate:
        him = -him
    him[0] = 0
    if L % 2 == 0:
        him[L // 2] = 0
    return SimpleNamespace(re=hre, im=him, S=tabs * g * rloc, extra=extra * tabs * rloc + table_extra, count=count)


def response_bound(P, b, L):
    """the bound on |got - ref| of Re H and of Im H at every bin (see the module's docstring)"""
    r = response_ld(P, b, L)
    return r.count * U53 * r.S + r.extra


def response_excess(H, P, b, L):
    """max |H - ref| / bound over the bins and both parts; where the bound is 0 the value must be exact"""
    ref, bound = response_ld(P, b, L), response_bound(P, b, L)
    worst = 0.0
    for got, want in ((H.real, ref.re), (H.imag, ref.im)):
        d = np.abs(got.astype(LD) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0))
        worst = max(worst, float(r.max()))
    return worst


def _butter64(ratio, order):
    r = ratio * ratio
    pw = r.copy()
    for _ in range(order - 1):
        pw = pw * r
    return 1.0 / np.sqrt(1.0 + pw)


def response_f64(P, b, L, mut=None, n=None):
    """H_b in float64 in the kernel's operation order (complex128 array); mut: a MUTATION"""
    k = np.arange(L // 2 + 1)
    f = (k * P.fs) / float(n if mut == "grid_n" else L)
    tau = P.tau_of(b)
    tre, tim = np.ones_like(f), np.zeros_like(f)
    if tau != 0.0:
        u = (2.0 * np.pi * f) * tau
        if P.mode == 0:
            tim = u
        else:
            den = 1.0 + u * u
            tre, tim = 1.0 / den, -u / den
    g = np.ones_like(f)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if P.lp is not None:
            g = g * _butter64(f / P.lp[0], P.lp[1])
        if P.hp is not None:
            gh = _butter64(P.hp[0] / f, P.hp[1])
            gh[0] = 0.0
            g = g * gh
    for f0, w in P.notch:
        a = np.abs(f - f0) / w
        s = np.sin((np.pi / 2) * a)
        g = g * np.where(a < 1.0, s * s, 1.0)
    hre, him = tre * g, tim * g
    row = P.row_of(b)
    if row is not None:
        Rn = row.size
        s = (f / (0.5 * P.fs)) * float(Rn - 1)
        i0 = np.minimum(s.astype(np.int64), Rn - 2)
        t = s - i0
        rr, ri = np.real(row).astype(np.float64), np.imag(row).astype(np.float64)
        vre = rr[i0] + t * (rr[i0 + 1] - rr[i0])
        if P.table_kind == 1:
            hre, him = hre * vre, him * vre
        else:
            vim = ri[i0] + t * (ri[i0 + 1] - ri[i0])
            hre, him = hre * vre - him * vim, hre * vim + him * vre
    if P.conjugate and mut != "conjugate_ignored":
        him = -him
    him[0] = 0.0
    if mut != "nyquist_imag":
        him[L // 2] = 0.0
    return hre + 1j * him


# -------------------------------------------------------------------- trend ----
def ends_ld(x, P):
    n = x.size
    if not P.detrend:
        return LD(0), LD(0)
    m = min(P.end_mean, n)
    xl = x.astype(LD)
    return xl[:m].sum() / m, xl[n - m:].sum() / m


def trend(a, b, n, dtype):
    i = np.arange(n).astype(dtype)
    if n == 1:
        return np.full(1, a, dtype=dtype)
    return a + ((b - a) * i) / dtype(n - 1)


# ---------------------------------------------------------------- reference ----
@functools.lru_cache(maxsize=4)
def _phase_tables(L):
    m = np.arange(L, dtype=LD)
    c, s = np.cos(2 * _PI * m / L), np.sin(2 * _PI * m / L)
    c[0], s[0], c[L // 2], s[L // 2] = 1, 0, -1, 0
    if L % 4 == 0:
        c[L // 4], s[L // 4], c[3 * L // 4], s[3 * L // 4] = 0, 1, 0, -1
    return c, s


def _dft_ld(xt, L):
    """X_k = sum_i xt_i e^{-2 pi i i k / L}, k = 0 .. L/2, of the n <= L samples xt"""
    c, s = _phase_tables(L)
    n, nf = xt.size, L // 2 + 1
    i = np.arange(n, dtype=np.int64)
    re, im = np.zeros(nf, dtype=LD), np.zeros(nf, dtype=LD)
    step = max(1, (1 << 20) // max(n, 1))
    for k0 in range(0, nf, step):
        k = np.arange(k0, min(nf, k0 + step), dtype=np.int64)
        ph = (k[:, None] * i[None, :]) % L
        re[k0:k0 + k.size] = (c[ph] * xt[None, :]).sum(axis=1)
        im[k0:k0 + k.size] = -(s[ph] * xt[None, :]).sum(axis=1)
    return re, im


def _idft_ld(yre, yim, L, n):
    """y_i = (1/L) sum_k Y_k e^{2 pi i i k / L} over the Hermitian spectrum given at k = 0 .. L/2, i < n"""
    c, s = _phase_tables(L)
    nf = L // 2 + 1
    k = np.arange(1, nf - 1, dtype=np.int64)
    out = np.zeros(n, dtype=LD)
    step = max(1, (1 << 20) // max(k.size, 1))
    for i0 in range(0, n, step):
        i = np.arange(i0, min(n, i0 + step), dtype=np.int64)
        sign = np.where(i % 2 == 0, LD(1), LD(-1))
        acc = yre[0] + sign * yre[nf - 1]
        if k.size:
            ph = (i[:, None] * k[None, :]) % L
            acc = acc + 2 * (c[ph] * yre[None, 1:nf - 1] - s[ph] * yim[None, 1:nf - 1]).sum(axis=1)
        out[i0:i0 + i.size] = acc / L
    return out


def _block_ld(xb, P, b):
    """the trend, the detrended block and the response of block b, with the block's error scale"""
    n = xb.size
    L = fft_length(n, P.pad)
    a, e = ends_ld(xb, P)
    line = trend(a, e, n, LD) if P.detrend else np.zeros(n, dtype=LD)
    xt = xb.astype(LD) - line
    H = response_ld(P, b, L)
    hmax = np.sqrt(H.re * H.re + H.im * H.im).max()
    E = np.asarray(U53 * (math.log2(L) * hmax * np.sqrt((xt * xt).sum()) + np.abs(H.re[0] * line)), dtype=np.float64)
    return L, line, xt, H, E


def error_scale(x, sizes, P):
    """E of every sample (0 in a bad block), without the transforms"""
    off = offsets(sizes)
    E = np.zeros(off[-1])
    for b, n in enumerate(sizes):
        xb = np.asarray(x[off[b]:off[b + 1]], dtype=np.float64)
        if np.isfinite(xb).all():
            E[off[b]:off[b + 1]] = _block_ld(xb, P, b)[4]
    return E


def ref_ld(x, sizes, P):
    """-> (out LD [nt], E float64 [nt], bad: the list of bad blocks).  A bad block's out is NaN and its E 0."""
    off = offsets(sizes)
    out, E, bad = np.zeros(off[-1], dtype=LD), np.zeros(off[-1]), []
    for b, n in enumerate(sizes):
        xb = np.asarray(x[off[b]:off[b + 1]], dtype=np.float64)
        if not np.isfinite(xb).all():
            out[off[b]:off[b + 1]] = np.nan
            bad.append(b)
            continue
        L, line, xt, H, E[off[b]:off[b + 1]] = _block_ld(xb, P, b)
        xre, xim = _dft_ld(xt, L)
        y = _idft_ld(H.re * xre - H.im * xim, H.re * xim + H.im * xre, L, n)
        out[off[b]:off[b + 1]] = y + H.re[0] * line
    return out, E, bad


# -------------------------------------------------------------- restatement ----
MUTATIONS = ("grid_n", "nyquist_imag", "h0_not_restored", "pad_next", "conjugate_ignored")


def apply_f64(x, sizes, P, mut=None):
    off = offsets(sizes)
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(off[-1])
    for b, n in enumerate(sizes):
        xb = x[off[b]:off[b + 1]]
        if not np.isfinite(xb).all():
            out[off[b]:off[b + 1]] = np.nan
            continue
        L = fft_length(n, P.pad)
        if P.detrend:
            m = min(P.end_mean, n)
            line = trend(xb[:m].sum() / m, xb[n - m:].sum() / m, n, np.float64)
        else:
            line = np.zeros(n)
        row = np.zeros(L)
        row[:n] = xb - line
        if mut == "pad_next":
            nxt = x[off[b + 1]:off[b + 1] + (L - n)]
            row[n:n + nxt.size] = nxt
        H = response_f64(P, b, L, mut, n)
        y = np.fft.irfft(np.fft.rfft(row) * H, L)[:n]
        out[off[b]:off[b + 1]] = y if mut == "h0_not_restored" else y + H[0].real * line
    return out


def ratio(got, ref, E):
    """max |got - ref| / E over the samples with a finite reference; where E = 0 the result must be exact"""
    ok = np.isfinite(np.asarray(ref, dtype=np.float64))
    d = np.abs(np.asarray(got, dtype=LD)[ok] - ref[ok])
    e = np.asarray(E, dtype=LD)[ok]
    if not np.isfinite(np.asarray(got, dtype=np.float64)[ok]).all():
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e > 0, d / e, np.where(d > 0, np.inf, 0))
    return float(r.max()) if r.size else 0.0


# --------------------------------------------------------------- shared cases ----
def walk(seed, n):
    """a random walk: the red stream a time constant and a low-pass are applied to"""
    return np.cumsum(np.random.default_rng(seed).standard_normal(n))


FS = 128.0                               # with L = 1024 every bin is a multiple of 1/8: exact notch positions
LP4 = (20.0, 4)


def _table_real(Rn):
    return 1.0 / np.sqrt(1.0 + (np.arange(Rn) / (0.3 * Rn)) ** 2)


def _table_complex(nb, Rn):
    rng = np.random.default_rng(77)
    return (1.0 + 0.3 * rng.standard_normal((nb, Rn))) * np.exp(1j * 0.5 * rng.standard_normal((nb, Rn)))


def _cases():
    seven = [1000, 3, 1000, 1, 2, 700, 1000]
    c = {}
    # the lengths: one block each; L = 1024 (pad 24), the segment edge, L = n
    c["one_1000"] = ([1000], Par(FS, tau=[5 / FS], lp=LP4, pad=24))
    c["one_1"] = ([1], Par(FS, tau=[5 / FS], lp=LP4, pad=0))
    c["one_2"] = ([2], Par(FS, tau=[5 / FS], lp=LP4, pad=0))
    c["one_3"] = ([3], Par(FS, tau=[5 / FS], lp=LP4, pad=0))
    c["edge_4095_4096_4097"] = ([4095, 4096, 4097], Par(FS, tau=[5 / FS, 0.1 / FS, 10 / FS], lp=LP4, pad=0))
    c["one_5184_nopad"] = ([5184], Par(FS, tau=[5 / FS], lp=LP4, pad=0))
    c["walk_3072"] = ([2048], Par(FS, tau=[5 / FS], lp=LP4, pad=1024))
    # seven blocks, three lengths (1024, 28, 750) in one stream, different tau per block
    c["seven"] = (seven, Par(FS, tau=np.array([0, 0.1, 10, 5, 1, 2, 0.5]) / FS, lp=LP4, pad=24))
    c["seven_convolve"] = (seven, Par(FS, tau=np.array([0, 0.1, 10, 5, 1, 2, 0.5]) / FS, mode=1, pad=24))
    c["seven_conjugate"] = (seven, Par(FS, tau=np.array([0, 0.1, 10, 5, 1, 2, 0.5]) / FS, lp=(20.0, 1), pad=24,
                                       conjugate=1, detrend=0))
    # every stage alone
    for p in (1, 4, 16):
        c["lowpass_%d" % p] = ([1000, 500], Par(FS, lp=(10.0, p), pad=24))
        c["highpass_%d" % p] = ([1000, 500], Par(FS, hp=(2.0, p), pad=24))
    # bins of L = 1024 at fs = 128 are k / 8: a bin exactly at f0 = 12.5, at f0 +- w = 12.5 +- 0.5, one outside
    c["notch"] = ([1000], Par(FS, notch=[(12.5, 0.5)], pad=24))
    c["notch_16"] = ([1000], Par(FS, notch=[(3.0 + 3.5 * j, 0.3 + 0.05 * j) for j in range(16)], pad=24))
    c["table_real"] = ([1000, 700], Par(FS, table=_table_real(33), pad=24))
    c["table_complex"] = ([1000, 700], Par(FS, table=_table_complex(2, 17), pad=24, detrend=0))
    c["table_two"] = ([1000], Par(FS, table=np.array([1.0, 0.25]), pad=24))
    # trend: none, one end sample, more end samples than the block has
    c["detrend_none"] = ([1000, 40], Par(FS, tau=[5 / FS, 5 / FS], lp=LP4, pad=24, detrend=0))
    c["end_mean_1"] = ([1000, 40], Par(FS, tau=[5 / FS, 5 / FS], lp=LP4, pad=24, end_mean=1))
    c["end_mean_over"] = ([1000, 40], Par(FS, tau=[5 / FS, 5 / FS], lp=LP4, pad=24, end_mean=1024))
    # all together
    c["all"] = ([1000, 700, 1000], Par(FS, tau=[5 / FS, 0.0, 1 / FS], mode=0, lp=(30.0, 4), hp=(0.5, 2),
                                       notch=[(12.5, 0.5), (50.0, 1.0)], table=_table_complex(3, 17), pad=24))
    return c


_CASES = _cases()
CASES = list(_CASES)


def case(name):
    sizes, P = _CASES[name]
    seed = sum(ord(ch) for ch in name)
    return SimpleNamespace(name=name, sizes=list(sizes), P=P, x=walk(seed, sum(sizes)))


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    out, E, bad = ref_ld(c.x, c.sizes, c.P)
    out.setflags(write=False)
    E.setflags(write=False)
    return SimpleNamespace(out=out, E=E, bad=bad)


def round_up(v):
    """v rounded up to two significant digits"""
    if v <= 0:
        return 0.0
    e = 10.0 ** (math.floor(math.log10(v)) - 1)
    return round(math.ceil(v / e - 1e-9) * e, 12)


def ratios_by_length(got, want, sizes, pad):
    """{L: the largest |got - ref| / E over the blocks of that transform length}; want: expected(name)"""
    off, out = offsets(sizes), {}
    for b, n in enumerate(sizes):
        sl = slice(off[b], off[b + 1])
        L = fft_length(n, pad)
        out[L] = max(out.get(L, 0.0), ratio(np.asarray(got)[sl], want.out[sl], want.E[sl]))
    return out


def measure_worst(mut=None):
    """{L: the largest ratio of apply_f64 against ref_ld over the shared cases, c = 1}"""
    worst = {}
    for name in CASES:
        c = case(name)
        for L, r in ratios_by_length(apply_f64(c.x, c.sizes, c.P, mut), expected(name), c.sizes, c.P.pad).items():
            worst[L] = max(worst.get(L, 0.0), r)
    return worst


# apply_f64 against ref_ld over the shared cases with c = 1, per transform length, rounded up to two digits
# (tests/test_fourier_cpu.py measures it again, on a CPU).  The short transforms sit near 1: a handful of operations,
# each half an ulp, against an E of a few ulps; from L = 1024 on the roundings average out under the log2 L law.
WORST = {2: 0.17, 4: 0.66, 28: 0.6, 64: 0.24, 540: 0.065, 750: 0.059, 1024: 0.037, 3072: 0.0068, 4096: 0.026,
         4116: 0.0072, 5184: 0.007}


def c_out(L):
    """the constant of the output bound for a block of transform length L"""
    return pow2_at_least(8.0 * WORST[L])


def assert_output(got, name, what=""):
    """every sample of every block within c_out(L) E; a bad block all quiet NaN"""
    c, want = case(name), expected(name)
    return assert_output_of(got, want, c.sizes, c.P.pad, what or name)


def assert_output_of(got, want, sizes, pad, what):
    off, worst = offsets(sizes), 0.0
    got = np.asarray(got, dtype=np.float64)
    for b, n in enumerate(sizes):
        sl = slice(off[b], off[b + 1])
        if b in want.bad:
            assert (bits(got[sl]) == QUIET_NAN).all(), "%s: block %d is bad and not all quiet NaN" % (what, b)
            continue
        L = fft_length(n, pad)
        r = ratio(got[sl], want.out[sl], want.E[sl]) / c_out(L)
        assert r <= 1.0, "%s: block %d (n = %d, L = %d): |got - ref| is %.3g x the bound c E (c = %g)" % (
            what, b, n, L, r, c_out(L))
        worst = max(worst, r)
    return worst
