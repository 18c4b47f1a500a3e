"""
The jump corrector restated in NumPy from its definition (include/cosmomap2.h, f2f), rule by rule and without the
kernels' method: a window sum is w additions in ascending sample order (the loop runs over the w terms, NumPy over the
windows: every window still adds its own terms one after the other, each addition rounded once), np.sort per block for
the scale, plain loops for the peaks, the offsets and the classes, and the host's iteration loop.  Also the shared
cases of tests/test_jump_cpu.py and tests/test_gpu_jump.py.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _glitch_ref as G

MAD_TO_SIGMA = 1.4826
CLEAN, AT, NEAR = range(3)
CLASSES = ("clean", "jump", "near")
MAX_W, MAX_RADIUS, MAX_ITER = 256, 256, 8
# the layout constants of cm2_jump_policy.h
TILE, TILE_THREADS, STARTS = 2048, 256, 9
TWO53 = 9007199254740992.0                     # 2^53: TWO53 + 1 == TWO53, and 1 - TWO53 is exact

bits, from_bits, flagged, edges = G.bits, G.from_bits, G.flagged, G.edges


def stat_lds_bytes(w):
    values = STARTS * TILE_THREADS + w
    return values * 8 + STARTS * TILE_THREADS * 8 + ((values + 1) * 2 + 7) // 8 * 8


# ------------------------------------------------------------------------ the restatement ----
def usable(d, flags=None, prev=None):
    """rule 1"""
    u = ~flagged(flags, d.size) & np.isfinite(d)
    if prev is not None:
        u &= np.asarray(prev) == 0
    return u


def window_sums(d, use, b0, b1, w):
    """rule 2 for one block: (S_j, n_j) for the starts j = b0 .. b1 - w (none: empty arrays)"""
    n = b1 - b0 - w + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    masked = np.where(use[b0:b1], d[b0:b1], 0.0)
    S, cnt = np.zeros(n), np.zeros(n, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(w):                             # S_j = (..((+0.0 + m_j) + m_{j+1}) + ..) + m_{j+w-1}
            S = S + masked[k:k + n]
            cnt += use[b0 + k:b0 + k + n]
    return S, cnt


def statistic(d, sizes, w, min_count, flags=None, prev=None):
    """rules 1-3: (t, noeval uint8)"""
    d = np.asarray(d, dtype=np.float64)
    use, e = usable(d, flags, prev), edges(sizes)
    t, noeval = np.zeros(d.size), np.ones(d.size, dtype=np.uint8)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b0, b1 in zip(e[:-1], e[1:]):
            S, cnt = window_sums(d, use, b0, b1, w)
            for i in range(b0 + w, b1 - w + 1):
                L, nL, R, nR = S[i - w - b0], cnt[i - w - b0], S[i - b0], cnt[i - b0]
                if nL >= min_count and nR >= min_count:
                    x = R / np.float64(nR) - L / np.float64(nL)
                    if np.isfinite(x):
                        t[i], noeval[i] = x, 0
    return t, noeval


def scale(t, noeval, sizes):
    """rule 4: (sigma per block, evaluable positions per block)"""
    e = edges(sizes)
    sigma, eb = np.full(len(sizes), np.inf), np.zeros(len(sizes), dtype=np.int64)
    for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
        a = np.sort(np.abs(t[b0:b1][noeval[b0:b1] == 0]))
        eb[b] = a.size
        if a.size >= 3:
            sigma[b] = MAD_TO_SIGMA * a[(a.size - 1) // 2]
    return sigma, eb


def find(t, noeval, sizes, w, sigma, nsigma):
    """rules 5-8 (the chain): (positions int64, heights, offsets, njumps per block)"""
    e = edges(sizes)
    pos, heights, offsets, njumps = [], [], [], np.zeros(len(sizes), dtype=np.int64)
    for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
        thr = np.float64(nsigma) * np.float64(sigma[b])
        s = 0.0
        for p in range(b0, b1):
            if noeval[p] or not abs(t[p]) > thr:
                continue
            jump = True
            for j in range(max(b0, p - w), min(b1, p + w + 1)):
                if j != p and not noeval[j] and (abs(t[j]) > abs(t[p]) or (abs(t[j]) == abs(t[p]) and j < p)):
                    jump = False
            if jump:
                with np.errstate(over="ignore", invalid="ignore"):
                    s = s + t[p]
                pos.append(p)
                heights.append(t[p])
                offsets.append(s)
                njumps[b] += 1
    return np.array(pos, dtype=np.int64), np.array(heights, dtype=np.float64), np.array(offsets, dtype=np.float64), \
        njumps


def correct(d, sizes, pos, offsets, prev=None, radius=4):
    """rules 8 and 9: (d_out, classes uint8, counts [nblocks, 3])"""
    d = np.asarray(d, dtype=np.float64)
    e = edges(sizes)
    out, cls = d.copy(), np.zeros(d.size, dtype=np.uint8)
    counts = np.zeros((len(sizes), 3), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
            mine = [k for k in range(len(pos)) if b0 <= pos[k] < b1]
            at, near = np.zeros(d.size, dtype=bool), np.zeros(d.size, dtype=bool)
            for k in mine:                                 # (a jump within its own radius: AT comes first)
                at[pos[k]] = True
                near[max(b0, pos[k] - radius):min(b1, pos[k] + radius + 1)] = True
            m = 0                                          # jumps of the block at or before i
            for i in range(b0, b1):
                while m < len(mine) and pos[mine[m]] <= i:
                    m += 1
                out[i] = d[i] - (offsets[mine[m - 1]] if m else 0.0)
                if prev is not None and prev[i]:
                    cls[i] = prev[i]
                    continue
                cls[i] = AT if at[i] else NEAR if near[i] else CLEAN
                counts[b, cls[i]] += 1
    return out, cls, counts


def run(d, sizes, w, flags=None, classes=None, min_count=None, nsigma=6.0, radius=4, iterations=3, sigma=None):
    """the host's loop: (d_out, classes, info) like JumpCorrector.run, info["each"] the passes"""
    x = np.array(d, dtype=np.float64)
    mc = (w + 1) // 2 if min_count is None else min_count
    given = None if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(sizes),))
    prev = None if classes is None else np.asarray(classes, dtype=np.uint8)
    passes, positions, heights, found = [], [], [], []
    for k in range(iterations):
        t, noeval = statistic(x, sizes, w, mc, flags, prev)
        sig, eb = scale(t, noeval, sizes)
        if given is not None:
            sig = np.array(given)
        pos, hgt, off, njumps = find(t, noeval, sizes, w, sig, nsigma)
        x, cls, counts = correct(x, sizes, pos, off, prev, radius)
        passes.append(SimpleNamespace(t=t, noeval=noeval, sigma=sig, pos=pos, heights=hgt, offsets=off, njumps=njumps,
                                      d_out=x, cls=cls, counts=counts))
        positions.append(pos)
        heights.append(hgt)
        found.append(np.full(pos.size, k, dtype=np.int64))
        prev = cls
        if pos.size == 0:
            break
    info = dict(positions=np.concatenate(positions), heights=np.concatenate(heights),
                found_in_pass=np.concatenate(found), counts=counts, sigma=[p.sigma for p in passes],
                short_blocks=np.flatnonzero(eb < 3), passes=len(passes), each=passes)
    return x, prev, info


# ------------------------------------------------------------------ stream cases (d given) ----
def _case(name, d, sizes, w, min_count=None, flags=None, prev=None, nsigma=4.0, radius=2, sigma=None):
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert d.size == sum(sizes), name
    return SimpleNamespace(name=name, d=d, sizes=[int(s) for s in sizes], w=w,
                           min_count=(w + 1) // 2 if min_count is None else min_count, flags=flags, prev=prev,
                           nsigma=nsigma, radius=radius, sigma=sigma)


def _random_flags(rng, nt, rate=0.1):
    return np.where(rng.random(nt) < rate, -1, rng.integers(0, 50, nt)).astype(np.int32)


W_EDGES = (1, 2, 64, 256)


def block_sizes(w):
    return [1, 2 * w - 1, 2 * w, 2 * w + 1, TILE - 1, TILE, TILE + 1, TILE + w]


def _steps(rng, sizes, w, height=8.0):
    """white noise with one step in the middle of every block that has room for one"""
    d = rng.standard_normal(sum(sizes))
    e = edges(sizes)
    for b0, b1 in zip(e[:-1], e[1:]):
        if b1 - b0 >= 2 * w + 1:
            d[(b0 + b1) // 2:b1] += height * (1 if (b0 + b1) % 3 else -1)
    return d


def stream_cases():
    out = {}

    def add(c):
        out[c.name] = c

    for w in W_EDGES:
        rng = np.random.default_rng(700 + w)
        sizes = block_sizes(w)
        nt = sum(sizes)
        add(_case("sizes_w%d" % w, _steps(rng, sizes, w), sizes, w, flags=_random_flags(rng, nt, 0.05),
                  radius=0 if w == 1 else 256 if w == 256 else 3))
    # a jump w and w + 1 samples from a block edge, on both sides; no noise: the heights are exact
    w = 8
    sizes = [300, 300, 300, 300, 40]
    d = np.zeros(sum(sizes))
    for b, at in enumerate((w, w + 1, 300 - w, 300 - w - 1)):
        d[300 * b + at:300 * (b + 1)] = 5.0 + b
    d[1200:] = 1.0
    add(_case("edge_jumps", d, sizes, w, sigma=0.5, radius=9))
    # nL = min_count - 1 and nL = min_count by flags: w = 8, min_count = 5, a step at 100 in each of two blocks
    sizes = [200, 200]
    rng = np.random.default_rng(710)
    d = 0.01 * rng.standard_normal(400)
    d[100:200] += 3.0
    d[300:400] += 3.0
    fl = np.zeros(400, dtype=np.int32)
    fl[92:96] = -1                                 # block 0: 4 of the 8 samples before 100 are left
    fl[292:295] = -1                               # block 1: 5 are left
    add(_case("min_count_int32", d, sizes, 8, 5, flags=fl, sigma=0.1))
    add(_case("min_count_bytes", d, sizes, 8, 5, flags=fl < 0, sigma=0.1))
    add(_case("min_count_uint8", d, sizes, 8, 5, flags=np.where(fl < 0, 9, 0).astype(np.uint8), sigma=0.1))
    add(_case("min_count_prev", d, sizes, 8, 5, prev=np.where(fl < 0, 3, 0).astype(np.uint8), sigma=0.1))
    both = np.zeros(400, dtype=np.uint8)
    both[292:295] = 4
    half = fl.copy()
    half[292:295] = 0
    add(_case("min_count_flags_and_prev", d, sizes, 8, 5, flags=half, prev=both, sigma=0.1))
    # values
    sizes = [500, 333]
    nt = sum(sizes)
    rng = np.random.default_rng(720)
    base = _steps(rng, sizes, 16)
    bad = base.copy()
    bad[[0, 499, 500, 832]] = [np.nan, np.inf, -np.inf, np.nan]          # first and last sample of both blocks
    bad[[240, 251, 260]] = [np.inf, np.nan, -np.inf]                     # around the step at 250
    add(_case("nonfinite", bad, sizes, 16, flags=_random_flags(rng, nt, 0.05)))
    huge = base.copy()
    huge[100:102] = 1e308                                                # the sums over them overflow: t not finite
    huge[400:402] = [-1e308, -1e308]
    huge[600:602] = [1e308, -1e308]                                      # this pair cancels exactly
    add(_case("huge_pairs", huge, sizes, 16))
    sub = from_bits(rng.integers(0, 1 << 20, nt).astype(np.uint64)) * np.where(rng.random(nt) < 0.5, -1.0, 1.0)
    sub[250:500] += from_bits(np.array([1 << 30], dtype=np.uint64))[0]
    add(_case("subnormals", sub, sizes, 16, flags=_random_flags(rng, nt, 0.05)))
    add(_case("constant", np.full(nt, 2.5), sizes, 16, flags=_random_flags(rng, nt, 0.05)))
    # the order of a window sum: 2^53, 1, -2^53 add up to 0 in ascending order, to 1 with the last two first
    d = np.zeros(300)
    d[100:103] = [TWO53, 1.0, -TWO53]
    d[200:203] = [-TWO53, TWO53, 1.0]
    add(_case("sum_order", d, [300], 4, sigma=0.1))
    # e_b = 2 and e_b = 3 from the block sizes (2 w + 1 and 2 w + 2), w = 5
    rng = np.random.default_rng(730)
    add(_case("scale_edges", rng.standard_normal(11 + 12 + 13), [11, 12, 13], 5))
    return out


@functools.lru_cache(maxsize=None)
def _stream_cases():
    return stream_cases()


STREAM_CASES = ("sizes_w1", "sizes_w2", "sizes_w64", "sizes_w256", "edge_jumps", "min_count_int32", "min_count_bytes",
                "min_count_uint8", "min_count_prev", "min_count_flags_and_prev", "nonfinite", "huge_pairs",
                "subnormals", "constant", "sum_order", "scale_edges")


def stream_case(name):
    return _stream_cases()[name]


@functools.lru_cache(maxsize=None)
def stream_expected(name):
    """one pass of rules 1-9 on a stream case"""
    c = stream_case(name)
    t, noeval = statistic(c.d, c.sizes, c.w, c.min_count, c.flags, c.prev)
    sigma, eb = scale(t, noeval, c.sizes)
    use = sigma if c.sigma is None else np.full(len(c.sizes), c.sigma)
    pos, heights, offsets, njumps = find(t, noeval, c.sizes, c.w, use, c.nsigma)
    d_out, cls, counts = correct(c.d, c.sizes, pos, offsets, c.prev, c.radius)
    return SimpleNamespace(t=t, noeval=noeval, sigma=sigma, eb=eb, sigma_used=use, pos=pos, heights=heights,
                           offsets=offsets, njumps=njumps, d_out=d_out, cls=cls, counts=counts)


# ------------------------------------------------------ peak cases (t and noeval made up) ----
SIGMA_GIVEN, NSIGMA = 0.7, 5.0
THR = NSIGMA * SIGMA_GIVEN                         # one multiplication, as rule 5 has it


def _peaks(name, sizes, w, spikes, noeval_at=(), radius=2, seed=0, sigma=SIGMA_GIVEN):
    """t = 0 but for the spikes {position: value}; every position evaluable but those of noeval_at; d random"""
    nt = sum(sizes)
    t, noeval = np.zeros(nt), np.zeros(nt, dtype=np.uint8)
    for p, v in spikes.items():
        t[p] = v
    noeval[list(noeval_at)] = 1
    d = np.random.default_rng(800 + seed).standard_normal(nt)
    return SimpleNamespace(name=name, sizes=[int(s) for s in sizes], w=w, t=t, noeval=noeval, d=d, radius=radius,
                           sigma=sigma, nsigma=NSIGMA)


def peak_cases():
    out = {}

    def add(c):
        out[c.name] = c

    up = np.nextafter(THR, np.inf)
    add(_peaks("threshold", [1000], 4, {100: THR, 200: up, 300: -up, 400: -THR}))
    w = 16
    add(_peaks("ties", [3000], w, {100: 9.0, 101: 9.0,                       # distance 1: the first wins
                                    500: -9.0, 500 + w: 9.0,                  # distance w: the first wins
                                    900: 9.0, 900 + w + 1: -9.0,              # distance w + 1: both are jumps
                                    1300: 8.0, 1300 + w: 9.0,                 # a larger one within w, after
                                    1700: 9.0, 1700 + w: 8.0,                 # and before
                                    2100: 9.0, 2104: 9.0, 2108: 9.0}))        # a chain of equals: only the first
    add(_peaks("ties_not_evaluable", [600], w, {100: 9.0, 101: 9.5, 300: 9.0, 299: 9.0}, noeval_at=(101, 299)))
    # peaks at the tile edge, at the first and the last position of a block, and of the stream
    sizes = [5000, 2048, 2049]
    add(_peaks("tile_and_block_edges", sizes, w, {0: 9.0, 2047: -9.0, 2048 + w + 1: 9.0, 4096 - 1: 9.0, 4999: 9.5,
                                                   5000: 9.0, 5000 + 2047: 9.0, 7048: 9.0, 7048 + 2047: 9.0,
                                                   7048 + 2048: -9.25}, radius=3))
    add(_peaks("tile_edge_2048", [5000], w, {2048: 9.0}, radius=3))
    add(_peaks("tile_edge_2049", [5000], w, {2049: 9.0, 2049 - w: 8.0}, radius=3))
    for radius in (0, 256):
        add(_peaks("radius_%d" % radius, [2200, 300, 2048], 4, {2047: 9.0, 2100: 9.0, 2199: 9.0, 2200: 9.0, 2350: 9.0,
                                                                 2500: 9.0, 2500 + 1900: 9.0, 4547: 9.0},
                   radius=radius, seed=radius))
    # the chain of the offsets: 2^53, 1, -2^53 add up to 0 in this order, to 1 with the last two first
    add(_peaks("offsets_order", [400, 400], 4, {100: TWO53, 200: 1.0, 300: -TWO53, 500: 1.0, 600: -TWO53, 700: TWO53},
               sigma=0.1))
    add(_peaks("offsets_overflow", [400], 4, {100: 1.5e308, 200: 1.5e308, 300: -1.5e308}))
    add(_peaks("no_jump", [700, 3], 4, {}))
    # many jumps: every fifth position, w = 2, in 3 blocks (601 + 20 + 400 = ... jumps): the capacity cases
    t = {p: 9.0 + (p % 7) for p in range(0, 5105, 5)}
    add(_peaks("many", [3005, 100, 2000], 2, t))
    return out


@functools.lru_cache(maxsize=None)
def _peak_cases():
    return peak_cases()


PEAK_CASES = ("threshold", "ties", "ties_not_evaluable", "tile_and_block_edges", "tile_edge_2048", "tile_edge_2049",
              "radius_0", "radius_256", "offsets_order", "offsets_overflow", "no_jump", "many")


def peak_case(name):
    return _peak_cases()[name]


@functools.lru_cache(maxsize=None)
def peak_expected(name):
    c = peak_case(name)
    pos, heights, offsets, njumps = find(c.t, c.noeval, c.sizes, c.w, [c.sigma] * len(c.sizes), c.nsigma)
    prev = None
    if name.startswith("radius"):                                  # classes carried where rule 9a applies
        prev = np.zeros(c.d.size, dtype=np.uint8)
        prev[[2046, 2100, 2348, 4000]] = [3, 4, 2, 1]
    d_out, cls, counts = correct(c.d, c.sizes, pos, offsets, prev, c.radius)
    return SimpleNamespace(pos=pos, heights=heights, offsets=offsets, njumps=njumps, prev=prev, d_out=d_out, cls=cls,
                           counts=counts)


# --------------------------------------------------------- scale cases (t and noeval made up) ----
def scale_cases():
    """(t, noeval, sizes): e_b = 0, 2, 3, 4 by the noeval bytes, all |t| equal, zeros, two tiles"""
    rng = np.random.default_rng(900)
    sizes = [10, 10, 10, 10, 10, 10, 5000]
    nt = sum(sizes)
    t, noeval = rng.standard_normal(nt), np.zeros(nt, dtype=np.uint8)
    noeval[0:10] = 1                                   # e = 0
    noeval[10:18] = 1                                  # e = 2
    noeval[20:27] = 1                                  # e = 3
    noeval[30:36] = 1                                  # e = 4
    t[40:50] = -0.75                                   # all equal
    t[50:60] = 0.0                                     # sigma = 0
    noeval[60:][rng.random(5000) < 0.3] = 1
    t[noeval == 1] = 0.0                               # as cm2_jump_stat leaves them
    return t, noeval, sizes


# ------------------------------------------------------------------------------ iteration ----
@functools.lru_cache(maxsize=None)
def iteration_case():
    """Two blocks of 1500 and 700 samples, w = 32: a step of 10 at 700 and one of 5 at 716, white noise of 1.5 (the
    scale of t is about 0.4, the threshold about 2.4).  The first pass sees the large one only (rule 6) and takes part
    of the small one for it, the second finds the small one, the third what the two estimates left over: below the
    threshold.  The first seed for which the restatement does exactly that."""
    sizes, w = [1500, 700], 32
    for seed in range(50):
        rng = np.random.default_rng(1000 + seed)
        d = 1.5 * rng.standard_normal(sum(sizes))
        d[700:1500] += 10.0
        d[716:1500] += 5.0
        out, cls, info = run(d, sizes, w, nsigma=6.0, radius=4, iterations=3)
        if info["passes"] == 3 and info["found_in_pass"].tolist() == [0, 1] and \
                abs(info["positions"][0] - 700) <= 3 and abs(info["positions"][1] - 716) <= 3:
            return SimpleNamespace(d=d, sizes=sizes, w=w, seed=seed, d_out=out, cls=cls, info=info)
    raise AssertionError("no seed gives a second pass that finds the hidden jump and a third that finds none")


# ------------------------------------------------------------------------ detection quality ----
QUALITY_SEED = 0
QUALITY_W, QUALITY_NSIGMA, QUALITY_L = 64, 6.0, 4096


def one_over_f_noise(rng, n, knee=0.01):
    """unit white noise shaped to the spectrum 1 + knee / f (f in cycles per sample; f = 0 left alone)"""
    f = np.fft.rfftfreq(n)
    gain = np.ones(f.size)
    gain[1:] = np.sqrt(1.0 + knee / f[1:])
    return np.fft.irfft(np.fft.rfft(rng.standard_normal(n)) * gain, n)


def low_bin_power(x, sizes, L=QUALITY_L):
    """mean over the blocks of the Welch PSD (hann, L samples, half overlap, means removed) in bins 1-5"""
    win = np.hanning(L + 1)[:-1]                           # the periodic window, as scipy.signal.welch uses it
    e, acc = edges(sizes), []
    for b0, b1 in zip(e[:-1], e[1:]):
        segs = [x[s:s + L] for s in range(b0, b1 - L + 1, L // 2)]
        p = np.mean([np.abs(np.fft.rfft((s - s.mean()) * win)) ** 2 for s in segs], axis=0)
        acc.append(2.0 * p[1:6] / (win ** 2).sum())
    return float(np.mean(acc))


@functools.lru_cache(maxsize=None)
def quality_case(seed=QUALITY_SEED, glitches=0):
    """4 blocks of 10 000 samples of 1 + 0.01 / f noise, 3 % flagged, 6 jumps a block of +-3 / 5 / 8 / 20 sigma at least
    3 w apart and 3 w from the block ends; glitches > 0: that many spikes of +-20 at unflagged samples"""
    rng = np.random.default_rng(seed)
    sizes, w = [10000] * 4, QUALITY_W
    nt = sum(sizes)
    clean = np.concatenate([one_over_f_noise(rng, s) for s in sizes])
    pix = rng.integers(0, 768, nt).astype(np.int32)
    pix[rng.random(nt) < 0.03] = -1
    d, where, heights = clean.copy(), [], []
    for b in range(4):
        slots = np.sort(rng.choice(np.arange(1, (10000 - 6 * w) // (3 * w)), 6, replace=False))
        hs = rng.permutation([3.0, 5.0, 8.0, 20.0, 5.0, 8.0]) * np.where(rng.random(6) < 0.5, -1.0, 1.0)
        for s, h in zip(slots, hs):
            p = 10000 * b + 3 * w * int(s) + int(rng.integers(0, w))
            d[p:10000 * (b + 1)] += h
            where.append(p)
            heights.append(h)
    where, heights = np.array(where), np.array(heights)
    assert (np.diff(where) >= 3 * w).all()
    spikes = np.zeros(0, dtype=np.int64)
    if glitches:
        spikes = np.sort(rng.choice(np.flatnonzero(pix >= 0), glitches, replace=False))
        d[spikes] += np.where(rng.random(glitches) < 0.5, -20.0, 20.0)
    return SimpleNamespace(d=d, clean=clean, sizes=sizes, w=w, pix=pix, where=where, heights=heights, spikes=spikes)


@functools.lru_cache(maxsize=None)
def quality_expected():
    q = quality_case()
    out, cls, info = run(q.d, q.sizes, q.w, flags=q.pix, nsigma=QUALITY_NSIGMA, radius=4, iterations=3)
    return SimpleNamespace(d_out=out, cls=cls, info=info)


@functools.lru_cache(maxsize=None)
def end_to_end_expected():
    """flag_glitches, then correct_jumps with its classes, on the quality stream with 40 glitches"""
    q = quality_case(glitches=40)
    gcls, ginfo = G.flag(q.d, q.sizes, 16, flags=q.pix, nsigma=5.0, grow=2, iterations=3)
    out, cls, info = run(q.d, q.sizes, q.w, flags=q.pix, classes=gcls, nsigma=QUALITY_NSIGMA, radius=4, iterations=3)
    return SimpleNamespace(gcls=gcls, ginfo=ginfo, d_out=out, cls=cls, info=info)
