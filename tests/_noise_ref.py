"""
References, restatements and error bounds for the inverse noise operator N^-1 (csrc/cm2_noise.hip,
csrc/cm2_overlap_save.hip).

Plain NumPy, no GPU.

  * ``toeplitz_ref``: the zero-boundary symmetric band sum of every block in extended precision
    (np.longdouble).
  * ``window_scale``: the error scale of an FFT convolution.  Its error is not proportional to an
    element's own sum |a| |v|: it is spread evenly over the window.  For output i in window w of block b

        B_i = A1_b ||x_w||_2 / sqrt(Lw),    A1_b = |a_0| + 2 sum_{j >= 1} |a_j|,

    x_w the zero-padded window as the kernel loads it (the block's own samples, flagged ones as zeros)
    and Lw its length.  A result is accepted when |got - ref| <= c 2^-53 B_i for EVERY element; where
    B_i = 0 it must be exactly 0.
  * ``direct_f64``, ``diag_f64``: float64 restatements in the kernels' term order (bit-equal to the GPU).
  * ``os_f64``, ``fft_f64``: float64 restatements of the formulas of the two FFT routes, NumPy's FFT
    standing in for the radix passes / rocFFT.  They are NOT bit-equal to the GPU; what they lose against
    the reference, WORST below, times a headroom of 8 (the factor the vector and the filter suites adopted
    for equal formulas in another rounding order), rounded up to a power of two, is the constant c.
  * ``MUTATIONS``: wrong kernels, as ``mut=`` of the restatements; tests/test_noise_ref_cpu.py shows that
    each of them fails the check that tests/test_gpu_noise_kernels.py applies.
"""
import functools
from collections import namedtuple

import numpy as np

from _vector_ref import LD, U53, bits, assert_bit_equal, excess, pow2_at_least  # noqa: F401

# ------------------------------------------------------------------- geometry ----
# csrc/cm2_os_policy.h: kT = 256 threads x kPts = 32 complex points, kHalo, W = 2 N, HOP = W - 2 kHalo,
# RLEN = 512 (kPts - 8) / RR with RR = 2 result rounds
N, W, HALO, HOP, RLEN = 8192, 16384, 2048, 12288, 6144
K_DIR_TILE = 2048                        # csrc/cm2_noise.hip: kDirTile
K_TAB_ROWS, K_T = 8, 256                 # csrc/cm2_os_policy.h: kTabRows, kT
DIRECT, FFT, FUSED, AUTO = 1, 2, 3, 0    # include/cosmomap2.h: CM2_TOEPLITZ_*

Win = namedtuple("Win", "start len lo hi blk")


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def windows(off, hop=HOP):
    """cm2::os::windows: `hop` outputs each, the last of a block what is left"""
    wins = []
    for b in range(len(off) - 1):
        for s0 in range(int(off[b]), int(off[b + 1]), hop):
            wins.append(Win(s0, min(int(off[b + 1]) - s0, hop), int(off[b]), int(off[b + 1]), b))
    return wins


def fft_geometry(lam, sizes, fft_len=None):
    """pick_fft_length and the segment loop of fft_build (cm2_noise.hip) -> L, halo, hop, segments;
    fft_len: the value of CM2_FFT_LEN"""
    halo, max_block = lam - 1, max(int(s) for s in sizes)
    L = None
    if fft_len is not None and fft_len > 2 * halo + 1:
        L = int(fft_len)
    if L is None:
        L = 256
        while L < 8 * halo:
            L <<= 1
        need = 1
        while need < max_block + 2 * halo:
            need <<= 1
        if need < L:
            L = need
        if L < 2 * halo + 2:
            L = 2 * (2 * halo + 2)
    hop = L - 2 * halo
    return L, halo, hop, windows(offsets(sizes), hop)


def dir_tiles(off):
    """dir_build: kDirTile outputs of one block per workgroup -> [(start, len, blk)]"""
    return [(w.start, w.len, w.blk) for w in windows(off, K_DIR_TILE)]


def choose_lists(want, build_sort, ntiles):
    """cm2::os::choose_lists with the tile offsets at hand -> list format 1 plain | 2 run-coded | 3 inverse"""
    want = want if want else (3 if ntiles >= 768 else 2)
    bound = ntiles if 0 < ntiles < N else N
    fits = (bound + 63) // 64 * 64 <= K_TAB_ROWS * K_T
    direct = (not build_sort) and 0 < ntiles <= 4096
    if direct and want == 3 and fits:
        return 3
    return 2 if want >= 2 and fits else 1


LIST_NAMES = {1: "plain", 2: "run-coded", 3: "inverse run-coded"}

# ---------------------------------------------------------------------- cases ----
SIZES = {
    "E1": (1, 2, 6143, 6144, 6145, 12287, 12288, 12289, 2047, 2048, 2049, 24577),
    "E2": (1, 2047, 2048, 2049, 6145, 12289),
    "E3": (5,),
    "E8": (12288,) * 8,
    "E9": (12288,) * 8 + (1,),
    "F1": (1, 1, 1),
    "F2": (500, 400, 124),
    "F33": (191, 192, 193, 385, 50),
    "D1": (1, 5, 300, 9000),
    "G8": (700,) * 8,                     # the diagonal operator with equal sizes
}
_SEED = {name: 7001 + 13 * i for i, name in enumerate(sorted(SIZES))}


def make_bands(lam, nb):
    """(1 + 0.1 b) exp(-k / (lam / 4)) cos(0.3 k); the last tap is large enough to be missed"""
    k = np.arange(lam, dtype=np.float64)
    a = np.exp(-k / (lam / 4.0)) * np.cos(0.3 * k)
    assert abs(a[-1]) >= 1e-3 * abs(a[0]), (lam, a[-1])
    return np.stack([(1.0 + 0.1 * b) * a for b in range(nb)])


def block_scale(b):
    return 10.0 ** (3 * (b % 3))


def make_input(name, kind):
    """`normal`: standard normals; `impulses`: one unit impulse per block, rotating over the first sample, the
    last, HOP - 1, HOP, RLEN - 1, RLEN where they exist.  Block b is scaled by 10^(3 (b mod 3)): what a kernel
    reads across a block boundary is far above the reader's own bound."""
    sizes = SIZES[name]
    off = offsets(sizes)
    if kind == "normal":
        v = np.random.default_rng(_SEED[name]).standard_normal(int(off[-1]))
    else:
        assert kind == "impulses"
        v = np.zeros(int(off[-1]))
    used = [0] * 6                         # rotation: the place used least so far, the rarer one on a tie
    for b, n in enumerate(sizes):
        if kind == "impulses":
            places = (0, n - 1, HOP - 1, HOP, RLEN - 1, RLEN)
            i = min((i for i in range(6) if 0 <= places[i] < n), key=lambda i: (used[i], -i))
            used[i] += 1
            v[off[b] + places[i]] = 1.0
        v[off[b]:off[b + 1]] *= block_scale(b)
    return v


FLAGS = ("none", "random7", "first_last", "window", "block")


def make_flags(name, kind):
    """-> ok (bool per sample), zeroed (unflagged samples whose VALUE is set to zero)"""
    sizes = SIZES[name]
    off = offsets(sizes)
    nt = int(off[-1])
    ok, zeroed = np.ones(nt, dtype=bool), np.zeros(nt, dtype=bool)
    big = max(range(len(sizes)), key=lambda b: (sizes[b], -b))
    if kind == "random7":
        ok = np.random.default_rng(_SEED[name] + 1).random(nt) >= 0.07
    elif kind == "first_last":
        ok[off[:-1]] = False
        ok[off[1:] - 1] = False
    elif kind == "window":
        if sizes[big] > HOP:               # the second window's outputs: its result lists have no valid entry
            ok[off[big] + HOP:min(off[big] + 2 * HOP, off[big + 1])] = False
        else:                              # equal sizes: one window without a sample, one of zeros (B = 0)
            ok[off[3]:off[4]] = False
            zeroed[off[5]:off[6]] = True
    elif kind == "block":
        b = min(2, len(sizes) - 1)
        ok[off[b]:off[b + 1]] = False
    else:
        assert kind == "none"
    return ok, zeroed


def make_pointing(kind, nt, npix, ok, seed=5):
    if kind == "raster":
        pix = (np.arange(nt, dtype=np.int64) // 7) % npix
    elif kind == "random":
        pix = np.random.default_rng(seed).integers(0, npix, nt).astype(np.int64)
    else:
        assert kind == "one_pixel"
        pix = np.zeros(nt, dtype=np.int64)
    pix[~ok] = -1
    return pix


# ------------------------------------------------------------------ reference ----
def toeplitz_ref(sizes, bands, v):
    """y_k = a0 v_k + sum_i a_i (v_{k+i} + v_{k-i}) inside every block, np.longdouble"""
    off = offsets(sizes)
    v = np.asarray(v, dtype=LD)
    out = np.empty(v.size, dtype=LD)
    for b, n in enumerate(sizes):
        a, x = np.asarray(bands[b], dtype=LD), v[off[b]:off[b + 1]]
        y = a[0] * x
        for i in range(1, min(len(a), n)):
            t = a[i] * x
            y[:-i] += t[i:]
            y[i:] += t[:-i]
        out[off[b]:off[b + 1]] = y
    return out


def window_scale(sizes, bands, v, Lw, halo, hop):
    """B_i = A1_b ||x_w||_2 / sqrt(Lw) for every sample (np.longdouble)"""
    off = offsets(sizes)
    v = np.asarray(v, dtype=LD)
    B = np.empty(v.size, dtype=LD)
    for w in windows(off, hop):
        a = np.abs(np.asarray(bands[w.blk], dtype=LD))
        A1 = a[0] + 2 * a[1:].sum()
        x = v[max(w.lo, w.start - halo):min(w.hi, w.start - halo + Lw)]
        B[w.start:w.start + w.len] = A1 * np.sqrt((x * x).sum()) / np.sqrt(LD(Lw))
    return B


Case = namedtuple("Case", "name lam inp flags sizes bands raw v ok ref")


@functools.lru_cache(maxsize=None)
def case(name, lam, inp="normal", flags="none"):
    """One shared case: `raw` is the time stream (values at flagged samples too), `v` the stream with the
    flagged samples as zeros, `ref` the extended-precision N^-1 v.  Evaluated once; nobody writes to it."""
    sizes = SIZES[name]
    bands = make_bands(lam, len(sizes))
    raw = make_input(name, inp)
    ok, zeroed = make_flags(name, flags)
    raw[zeroed] = 0.0
    if inp == "impulses":                  # a flagged sample has a value to leak
        raw[~ok] = 3.0
    v = np.where(ok, raw, 0.0)
    ref = toeplitz_ref(sizes, bands, v)
    for arr in (bands, raw, v, ok, ref):
        arr.setflags(write=False)
    return Case(name, lam, inp, flags, sizes, bands, raw, v, ok, ref)


# --------------------------------------------------------------- restatements ----
def direct_f64(sizes, bands, v, mut=None):
    """k_toeplitz_direct / k_toeplitz_direct_tiled: a0 v_k, then for i = 1 .. lambda - 1  + a_i v_{k+i},
    + a_i v_{k-i} (terms outside the block left out, or added as a_i * 0, which is the same)"""
    off = offsets(sizes)
    v = np.asarray(v, dtype=np.float64)
    out = np.empty(v.size)
    for b, n in enumerate(sizes):
        a, x = np.asarray(bands[b], dtype=np.float64), v[off[b]:off[b + 1]]
        y = a[0] * x
        for i in range(1, min(len(a), n)):
            t = a[i] * x
            if mut == "dir_term_order":
                y[i:] += t[:-i]
                y[:-i] += t[i:]
            else:
                y[:-i] += t[i:]
                y[i:] += t[:-i]
        out[off[b]:off[b + 1]] = y
    if mut == "dir_tile_halo":             # the first staged halo sample of every tile is missing
        lam = len(bands[0])
        for start, _, b in dir_tiles(off):
            if start - (lam - 1) >= off[b]:
                a, acc = bands[b], bands[b][0] * v[start]
                for i in range(1, lam):
                    if start + i < off[b + 1]:
                        acc += a[i] * v[start + i]
                    if i < lam - 1:
                        acc += a[i] * v[start - i]
                out[start] = acc
    return out


def diag_f64(sizes, t, v=None):
    """k_diag_apply: t_b v_k, or t_b (cm2_noise_expand_diag)"""
    w = np.repeat(np.asarray(t, dtype=np.float64), np.asarray(sizes, dtype=np.int64))
    return w if v is None else w * np.asarray(v, dtype=np.float64)


_PI = 4 * np.arctan(LD(1))


def _cospi(num, den):
    """cos(pi num / den) for integer arrays, correctly rounded (the kernels use cospi / sinpi)"""
    return np.cos(_PI * np.asarray(num, dtype=LD) / LD(den)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _os_tables():
    m = np.arange(N + 1)
    return _cospi(m, N), np.sin(_PI * np.arange(N, dtype=LD) / LD(N)).astype(np.float64)


def os_alpha_beta(band, mut=None):
    """k_real_cos_table, k_real_spectrum, k_real_alpha_beta: the band's spectrum H on 2N points, summed from
    j = lambda - 1 down to 1 with the cosines of a table, and the two tables of the pairing"""
    band = np.ascontiguousarray(band, dtype=np.float64)
    return _os_alpha_beta(band.tobytes(), mut if mut in ("last_tap_dropped", "nyquist_dropped") else None)


@functools.lru_cache(maxsize=64)
def _os_alpha_beta(band_bytes, mut):
    band = np.frombuffer(band_bytes, dtype=np.float64)
    ct, st = _os_tables()
    lam = len(band)
    k = np.arange(N + 1, dtype=np.int64)
    acc = np.zeros(N + 1)
    for j in range(lam - 2 if mut == "last_tap_dropped" else lam - 1, 0, -1):
        m = (j * k) & (2 * N - 1)
        acc += band[j] * ct[np.where(m <= N, m, 2 * N - m)]
    H = band[0] + 2.0 * acc
    if mut == "nyquist_dropped":
        H[N] = 0.0
    hk, hp = H[:N], H[N - np.arange(N)]
    S, D = 0.5 * (hk + hp), 0.5 * (hk - hp)
    return (S - D * st) / float(N), (D * ct[:N]) / float(N)


@functools.lru_cache(maxsize=64)
def _fft_spectrum(band_bytes, L, mut):
    """k_spectrum: H[k] = (a0 + 2 sum_{j = lambda - 1 .. 1} a_j cospi(2 (j k mod L) / L)) / L"""
    a = np.frombuffer(band_bytes, dtype=np.float64)
    ct = _cospi(2 * np.arange(L), L)
    k = np.arange(L // 2 + 1, dtype=np.int64)
    acc = np.zeros(L // 2 + 1)
    for j in range(len(a) - 2 if mut == "last_tap_dropped" else len(a) - 1, 0, -1):
        acc += a[j] * ct[(j * k) % L]
    return (a[0] + 2.0 * acc) / float(L)

# ---- the three passes of k_os_real (radix 32 / 16 / 16, N = 32 x 16 x 16) in NumPy float64 -----------------
# z[256 m + 16 j + r] -> Z[k1 + 32 k2 + 512 k3]: the kernel's butterflies in their order, its 32-entry
# cosine / sine table, its twiddles w^m by the recurrence from W[t] = exp(-2 pi i t / N).  No FMA contraction
# (NumPy has none), so this is closer to the kernel than NumPy's FFT but still not bit-equal to it.
_COS32 = _cospi(2 * np.arange(32), 32)
_SIN32 = np.sin(_PI * 2 * np.arange(32, dtype=LD) / LD(32)).astype(np.float64)
_COS32[[8, 24]] = 0.0
_SIN32[[0, 16]] = 0.0


def _brev(m, radix):
    return int(format(m, "0%db" % (radix.bit_length() - 1))[::-1], 2)


_BR32, _BR16 = [_brev(m, 32) for m in range(32)], [_brev(m, 16) for m in range(16)]


@functools.lru_cache(maxsize=None)
def _twiddles():
    """k_real_twiddles: W[t] = (cospi(2 t / N), -sinpi(2 t / N))"""
    t = np.arange(N)
    return _cospi(2 * t, N), -np.sin(_PI * 2 * t.astype(LD) / LD(N)).astype(np.float64)


def _dft_sub(re, im, radix):
    """dft_sub: decimation-in-frequency butterflies over axis 0; output m ends at index brev(m)"""
    h = radix // 2
    while h >= 1:
        for blk in range(0, radix, 2 * h):
            for i in range(h):
                a, b, tw = blk + i, blk + i + h, i * (32 // (2 * h))
                ar, ai, br, bi = re[a].copy(), im[a].copy(), re[b].copy(), im[b].copy()
                re[a], im[a] = ar + br, ai + bi
                dr, di = ar - br, ai - bi
                if tw == 0:
                    re[b], im[b] = dr, di
                elif tw == 8:
                    re[b], im[b] = di, -dr
                else:
                    c, s = _COS32[tw], _SIN32[tw]
                    re[b], im[b] = dr * c + di * s, di * c - dr * s
        h //= 2


def _dit_sub(re, im, radix):
    """dit_sub: decimation in time, input m at index brev(m), output natural"""
    h = 1
    while h <= radix // 2:
        for blk in range(0, radix, 2 * h):
            for i in range(h):
                a, b, tw = blk + i, blk + i + h, i * (32 // (2 * h))
                if tw == 0:
                    tr, ti = re[b].copy(), im[b].copy()
                elif tw == 8:
                    tr, ti = im[b].copy(), -re[b]
                else:
                    c, s = _COS32[tw], _SIN32[tw]
                    tr, ti = re[b] * c + im[b] * s, im[b] * c - re[b] * s
                ar, ai = re[a].copy(), im[a].copy()
                re[a], im[a] = ar + tr, ai + ti
                re[b], im[b] = ar - tr, ai - ti
        h *= 2


def _powers(w1r, w1i, radix):
    """w1^m, m = 0 .. radix - 1, by the recurrence of reg_fwd / reg_inv"""
    cr, ci = [np.ones_like(w1r)], [np.zeros_like(w1r)]
    for _ in range(1, radix):
        cr, ci = cr + [cr[-1] * w1r - ci[-1] * w1i], ci + [cr[-1] * w1i + ci[-1] * w1r]
    return cr, ci


def _reg_fwd(re, im, w1r, w1i, radix, br):
    _dft_sub(re, im, radix)
    cr, ci = _powers(w1r, w1i, radix)
    for m in range(1, radix):
        i = br[m]
        re[i], im[i] = re[i] * cr[m] - im[i] * ci[m], re[i] * ci[m] + im[i] * cr[m]


def _reg_inv(re, im, w1r, w1i, radix):
    cr, ci = _powers(w1r, w1i, radix)
    for m in range(1, radix):
        re[m], im[m] = re[m] * cr[m] + im[m] * ci[m], im[m] * cr[m] - re[m] * ci[m]
    _dft_sub(im, re, radix)


def passes_forward(zr, zi):
    """forward_passes and the last radix-16 butterflies -> the spectrum as [brev k3][k1][k2]"""
    wr, wi = _twiddles()
    r = np.arange(16)
    re, im = zr.reshape(32, 256).copy(), zi.reshape(32, 256).copy()            # [m][t], t = 16 j + r
    _reg_fwd(re, im, wr[:256], wi[:256], 32, _BR32)
    re, im = re[_BR32], im[_BR32]                                              # [k1][t]
    re = np.ascontiguousarray(re.reshape(32, 16, 16).transpose(1, 0, 2))      # [j][k1][r]
    im = np.ascontiguousarray(im.reshape(32, 16, 16).transpose(1, 0, 2))
    _reg_fwd(re, im, wr[32 * r][None, :], wi[32 * r][None, :], 16, _BR16)
    re, im = re[_BR16], im[_BR16]                                              # [k2][k1][r]
    re, im = np.ascontiguousarray(re.transpose(2, 1, 0)), np.ascontiguousarray(im.transpose(2, 1, 0))
    _dft_sub(re, im, 16)                                                       # [brev k3][k1][k2]
    return re, im


def passes_inverse(re, im):
    """the first inverse butterflies and inverse_tail: [brev k3][k1][k2] -> y[256 m + 16 j + r], not normalised"""
    wr, wi = _twiddles()
    r = np.arange(16)
    _dit_sub(im, re, 16)                                                       # [r][k1][k2]
    re, im = np.ascontiguousarray(re.transpose(2, 1, 0)), np.ascontiguousarray(im.transpose(2, 1, 0))
    _reg_inv(re, im, wr[32 * r][None, :], wi[32 * r][None, :], 16)            # [brev j][k1][r]
    re, im = re[_BR16], im[_BR16]
    re = np.ascontiguousarray(re.transpose(1, 0, 2)).reshape(32, 256)          # [k1][t]
    im = np.ascontiguousarray(im.transpose(1, 0, 2)).reshape(32, 256)
    _reg_inv(re, im, wr[:256], wi[:256], 32)                                   # [brev m][t]
    return re[_BR32].reshape(-1), im[_BR32].reshape(-1)


def passes_natural(a):
    """[brev k3][k1][k2] -> natural order k = k1 + 32 k2 + 512 k3"""
    return a[_BR16].transpose(0, 2, 1).reshape(-1)


def passes_layout(a):
    """natural order -> [brev k3][k1][k2]"""
    return np.ascontiguousarray(a.reshape(16, 16, 32).transpose(0, 2, 1))[_BR16]


def _load(v, w0, length, lo, hi):
    x = np.zeros(length)
    a, b = max(lo, w0), min(hi, w0 + length)
    if b > a:
        x[a - w0:b - w0] = v[a:b]
    return x


def os_f64(sizes, bands, v, mut=None, raw=None, passes=False):
    """k_os_real: z[a] = x[2a] + i x[2a+1], Z = FFT_N z, Z'[k] = alpha Z[k] + i beta conj(Z[N-k]), z' = IFFT_N Z',
    outputs [HALO, HALO + len) of each window in two rounds of RLEN.  `raw` (mut = flag_leak): the stream
    with the values of the flagged samples.  `passes`: the kernel's three radix passes with its twiddle
    recurrences instead of NumPy's FFT (the constants c come from NumPy's; tests/test_noise_ref_cpu.py shows
    that this one, which loses four to five times as much, stays inside them)."""
    off = offsets(sizes)
    v = np.asarray(raw if mut == "flag_leak" else v, dtype=np.float64)
    nt = int(off[-1])
    out = np.full(nt, np.nan)
    ab = {}
    wins = windows(off)
    first = {}
    for i, w in enumerate(wins):
        first.setdefault(w.blk, i)
    if mut == "window_skipped":
        wins = wins[:-1]
    partner = (N - np.arange(N)) % N
    for i, w in enumerate(wins):
        blk = w.blk
        if mut == "prev_block_band" and blk > 0 and first[blk] == i:
            blk -= 1
        if blk not in ab:
            ab[blk] = os_alpha_beta(bands[blk], mut)
        alpha, beta = ab[blk]
        if mut == "tables_three_digits":     # (alpha, beta) good to 1000 units of rounding only
            rng = np.random.default_rng(11)
            alpha = alpha * (1.0 + 1000.0 * 2.0 ** -53 * rng.uniform(-1, 1, N))
            beta = beta * (1.0 + 1000.0 * 2.0 ** -53 * rng.uniform(-1, 1, N))
        lo, hi = (0, nt) if mut == "no_zero_boundary" else (w.lo, w.hi)
        x = _load(v, w.start - HALO, W, lo, hi)
        if mut == "halo_short":
            x[0] = x[W - 1] = 0.0
        if passes:
            Z = [passes_natural(a) for a in passes_forward(x[0::2].copy(), x[1::2].copy())]
            Z = Z[0] + 1j * Z[1]
        else:
            Z = np.fft.fft(x[0::2] + 1j * x[1::2])
        P = Z if mut == "partner_same" else Z[partner]
        Zp = alpha * Z + 1j * (beta * np.conj(P))
        if passes:
            z = passes_inverse(passes_layout(Zp.real), passes_layout(Zp.imag))
            z = z[0] + 1j * z[1]
        else:
            z = np.fft.ifft(Zp) * float(N)
        y = np.empty(W)
        y[0::2], y[1::2] = z.real, z.imag
        res = y[HALO:HALO + w.len].copy()
        if mut == "round_seam" and w.len > RLEN:
            res[RLEN] = res[RLEN - 1]
        if mut == "seam_1e11" and w.len > RLEN:
            res[RLEN - 1:RLEN + 1] *= 1.0 + 1e-11
        n = w.len - 1 if mut == "drop_last_output" else w.len
        out[w.start:w.start + n] = res[:n]
    return out


def fft_f64(sizes, bands, v, fft_len=None, mut=None):
    """k_spectrum, k_pack, rocFFT R2C, k_spec_mul, rocFFT C2R (not normalised: 1 / L is folded into H), k_unpack"""
    lam = len(bands[0])
    L, halo, hop, segs = fft_geometry(lam, sizes, fft_len)
    off = offsets(sizes)
    v = np.asarray(v, dtype=np.float64)
    nt = int(off[-1])
    out = np.full(nt, np.nan)
    Hs = {}
    first = {}
    for i, w in enumerate(segs):
        first.setdefault(w.blk, i)
    if mut == "window_skipped":
        segs = segs[:-1]
    for i, w in enumerate(segs):
        blk = w.blk
        if mut == "prev_block_band" and blk > 0 and first[blk] == i:
            blk -= 1
        if blk not in Hs:
            Hs[blk] = _fft_spectrum(np.ascontiguousarray(bands[blk], dtype=np.float64).tobytes(), L,
                                    mut if mut == "last_tap_dropped" else None)
        lo, hi = (0, nt) if mut == "no_zero_boundary" else (w.lo, w.hi)
        x = _load(v, w.start - halo, L, lo, hi)
        y = np.fft.irfft(np.fft.rfft(x) * Hs[blk], L) * float(L)
        n = w.len - 1 if mut == "drop_last_output" else w.len
        out[w.start:w.start + n] = y[halo:halo + n]
    return out


# ------------------------------------------------------------ the shared cases ----
# fused kernel on the time order: (sizes, lambda, input, flags)
TIME_CASES = [(n, lam, inp, "none") for n, lams in (("E1", (1, 2, 33, 300)), ("E2", (2048, 2049)), ("E3", (33,)),
                                                     ("E8", (33,)), ("E9", (33,)))
              for lam in lams for inp in ("normal", "impulses")]

# fused kernel on a tile order: (id, sizes, lambda, input, flags, pointing, tiles of 64 pixels, CM2_OS_LISTS,
# CM2_OS_FLAT, CM2_OS_LIST_BUILD=sort).  Every instantiation <1..3, BUF | flat> on `raster` with 7 % flags and
# on `random` with the `window` flags; the auto choice at 100 (run-coded), 800 (inverse) and 2100 tiles (plain:
# the run table does not fit); the sorted builder once per format it yields; one_pixel, first_last, block once.
TileCase = namedtuple("TileCase", "id name lam inp flags pointing ntiles lists flat sort")
TILE_CASES = [TileCase(*c) for c in (
    [("%s-%s-raster7" % (ls, "flat" if fl else "buf"), "E2", 33, "normal", "random7", "raster", 100, ls, fl, False)
     for ls in ("plain", "rc", "inv") for fl in (False, True)] +
    [("%s-%s-randomwin" % (ls, "flat" if fl else "buf"), "E9", 33, "normal", "window", "random", 800, ls, fl, False)
     for ls in ("plain", "rc", "inv") for fl in (False, True)] + [
        ("auto-100", "E2", 2049, "normal", "random7", "raster", 100, None, False, False),
        ("auto-800", "E2", 2049, "impulses", "window", "random", 800, None, False, False),
        ("auto-2100", "E9", 33, "normal", "none", "random", 2100, None, False, False),
        ("sort-rc", "E2", 33, "normal", "random7", "random", 100, None, False, True),
        ("sort-plain", "E2", 33, "normal", "random7", "random", 2100, None, False, True),
        ("one-pixel", "E2", 33, "normal", "none", "one_pixel", 1, None, False, False),
        ("first-last", "E2", 33, "impulses", "first_last", "raster", 100, None, False, False),
        ("block", "E9", 33, "normal", "block", "raster", 800, None, False, False),
    ])]
# AUTO on a tile order (fused, built lazily)
AUTO_TILE_CASES = [TileCase("auto-method-%d" % lam, "E2", lam, "normal", "random7", "raster", 100, None, False, False)
                   for lam in (2, 32, 33)]

# rocFFT route: (sizes, lambda, input, CM2_FFT_LEN)
FFT_CASES = [("F1", 1, "normal", None), ("F2", 2, "normal", None), ("F33", 33, "normal", None),
             ("F33", 33, "impulses", None), ("E2", 2049, "normal", None), ("E2", 2049, "impulses", None),
             ("F33", 33, "normal", 1024)]

# direct routes: tiled kernel (tiles of 2048 against blocks of 2047, 2048, 2049), plain loop
DIRECT_CASES = [("E1", 2), ("E1", 33), ("E2", 300), ("D1", 8578)]


def fused_keys():
    """every (sizes, lambda, input, flags) a fused kernel sees"""
    keys = list(TIME_CASES)
    keys += [(t.name, t.lam, t.inp, t.flags) for t in TILE_CASES + AUTO_TILE_CASES]
    return sorted(set(keys))


# ------------------------------------------------------------- the constants c ----
# Largest |restatement - ref| / (2^-53 B) over the shared cases, per route and band length, rounded up to one
# decimal (tests/test_noise_ref_cpu.py re-measures them and fails when they are stale).
WORST = {
    "fused": {1: 490.2, 2: 367.5, 32: 17.5, 33: 46.3, 300: 5.5, 2048: 0.9, 2049: 0.9},
    "fft": {1: 1.2, 2: 9.7, 33: 2.7, 2049: 1.4},
}


def c_of(route, lam):
    return pow2_at_least(8.0 * WORST[route][lam])


def measure_worst(route):
    """-> {lambda: largest share of 2^-53 B that the restatement of `route` loses}"""
    worst = {}
    if route == "fused":
        for key in fused_keys():
            cs = case(*key)
            e = excess(os_f64(cs.sizes, cs.bands, cs.v), cs.ref, window_scale(cs.sizes, cs.bands, cs.v, W, HALO, HOP), 1)
            worst[cs.lam] = max(worst.get(cs.lam, 0.0), e)
    else:
        for name, lam, inp, fft_len in FFT_CASES:
            cs = case(name, lam, inp)
            L, halo, hop, _ = fft_geometry(lam, cs.sizes, fft_len)
            e = excess(fft_f64(cs.sizes, cs.bands, cs.v, fft_len), cs.ref,
                       window_scale(cs.sizes, cs.bands, cs.v, L, halo, hop), 1)
            worst[lam] = max(worst.get(lam, 0.0), e)
    return worst


def round_up(x):
    return float(np.ceil(x * 10.0 - 1e-9) / 10.0)


def share(got, cs, route, fft_len=None, only=None):
    """largest |got - ref| / (c 2^-53 B) over all elements (`only`: over the unflagged ones)"""
    if route == "fused":
        B = window_scale(cs.sizes, cs.bands, cs.v, W, HALO, HOP)
    else:
        L, halo, hop, _ = fft_geometry(cs.lam, cs.sizes, fft_len)
        B = window_scale(cs.sizes, cs.bands, cs.v, L, halo, hop)
    got = np.asarray(got, dtype=np.float64)
    if only is not None:
        return excess(got[only], cs.ref[only], B[only], c_of(route, cs.lam))
    return excess(got, cs.ref, B, c_of(route, cs.lam))


# ------------------------------------------------------------------ mutations ----
# name -> (route, case on which it must show, what shows it).  The smallest factor by which each value mutation
# exceeds its bound is measured by tests/test_noise_ref_cpu.py.
MUTATIONS = {
    "halo_short": ("fused", ("E2", 2049, "normal", "none"), "value"),
    "no_zero_boundary": ("fused", ("E1", 33, "normal", "none"), "value"),
    "prev_block_band": ("fused", ("E1", 33, "impulses", "none"), "value"),
    "drop_last_output": ("fused", ("E9", 33, "normal", "none"), "nan"),
    "round_seam": ("fused", ("E1", 2, "normal", "none"), "value"),
    "nyquist_dropped": ("fused", ("E1", 300, "normal", "none"), "value"),
    "partner_same": ("fused", ("E3", 33, "normal", "none"), "value"),
    "last_tap_dropped": ("fused", ("E2", 2048, "impulses", "none"), "value"),
    "flag_leak": ("fused", ("E2", 33, "normal", "random7"), "value"),
    "window_skipped": ("fused", ("E9", 33, "impulses", "none"), "nan"),
    "dir_tile_halo": ("direct", ("E1", 33, "normal", "none"), "value"),
    "dir_term_order": ("direct", ("E2", 300, "normal", "none"), "bits"),
}
# Two more, of the kind a norm over the whole stream cannot see (`subtle`: they must exceed the bound, and
# rel_l2 < 1e-12 over the stream must NOT notice them): a relative error of 1e-11 at the two samples of every
# seam between the result rounds, and (alpha, beta) tables that lost three digits (a loss of two digits stays
# within the bound at lambda = 2049, at 0.7 of it: A1 is far above the band's spectrum there).
SUBTLE = {
    "seam_1e11": ("fused", ("E1", 300, "normal", "none"), "subtle"),
    "tables_three_digits": ("fused", ("E2", 2049, "normal", "none"), "subtle"),
}
