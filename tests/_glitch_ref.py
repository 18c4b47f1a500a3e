"""
The glitch flagger restated in NumPy from its definition (include/cosmomap2.h, f2e), without the kernels' method:
np.sort per window for the median, np.sort per block for the scale, a direct loop for the classes and the host's
iteration loop.  Also the shared cases of tests/test_glitch_cpu.py and tests/test_gpu_glitch.py.
"""
import functools
from types import SimpleNamespace

import numpy as np

MAD_TO_SIGMA = 1.4826
CLEAN, INPUT, NONFINITE, HIT, NEAR = range(5)
CLASSES = ("clean", "input", "nonfinite", "hit", "near")
MAX_H, MAX_GROW, MAX_ITER = 64, 64, 8
# the layout constants of cm2_glitch_policy.h
RUN, CHUNK, TILE, TILE_THREADS, DIGITS, MAX_BINS = 64, 8, 2048, 256, 6, 2048
TIER_MAX_H = (8, 16, 32, 48, 64)
REGISTER_SLOTS = (17, 33, 65, 97, 96)
TIER_THREADS = (64, 64, 64, 64, 64)
DIGIT_BITS = (8, 11, 11, 11, 11, 11)
DIGIT_SHIFT = (55, 44, 33, 22, 11, 0)


def tier_of(h):
    return next(k for k, top in enumerate(TIER_MAX_H) if h <= top)


def group(h):
    """samples one workgroup of the median kernel covers"""
    return TIER_THREADS[tier_of(h)] * RUN


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def from_bits(k):
    return np.ascontiguousarray(k, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------ the restatement ----
def flagged(flags, nt):
    if flags is None:
        return np.zeros(nt, dtype=bool)
    f = np.asarray(flags)
    return f < 0 if np.issubdtype(f.dtype, np.signedinteger) else f != 0


def usable(d, flags=None, prev=None):
    """definition 1"""
    u = ~flagged(flags, d.size) & np.isfinite(d)
    if prev is not None:
        u &= (prev != HIT) & (prev != NEAR)
    return u


def edges(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def residual(d, sizes, h, flags=None, prev=None):
    """definitions 2 and 3"""
    d = np.asarray(d, dtype=np.float64)
    use, r, e = usable(d, flags, prev), np.zeros(d.size), edges(sizes)
    with np.errstate(over="ignore"):
        for b0, b1 in zip(e[:-1], e[1:]):
            for i in range(b0, b1):
                if not use[i]:
                    continue
                lo, hi = max(b0, i - h), min(b1, i + h + 1)
                v = np.sort(d[lo:hi][use[lo:hi]])
                m = v.size
                med = v[(m - 1) // 2] if m & 1 else 0.5 * v[m // 2 - 1] + 0.5 * v[m // 2]
                r[i] = d[i] - med
    return r


def scale(d, r, sizes, h, flags=None, prev=None):
    """definition 4: (sigma per block, usable samples per block)"""
    use, e, W = usable(np.asarray(d, dtype=np.float64), flags, prev), edges(sizes), 2 * h + 1
    sigma, mb = np.full(len(sizes), np.inf), np.zeros(len(sizes), dtype=np.int64)
    for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
        a = np.sort(np.abs(r[b0:b1][use[b0:b1]]))
        mb[b] = a.size
        if a.size >= W:
            sigma[b] = MAD_TO_SIGMA * a[(a.size - 1) // 2]
    return sigma, mb


def classify(d, r, sizes, sigma, nsigma, grow, flags=None, prev=None):
    """definitions 5-7: (classes uint8, counts [nblocks, 5] int64)"""
    d = np.asarray(d, dtype=np.float64)
    use, fl, e = usable(d, flags, prev), flagged(flags, d.size), edges(sizes)
    cls = np.zeros(d.size, dtype=np.uint8)
    counts = np.zeros((len(sizes), 5), dtype=np.int64)
    for b, (b0, b1) in enumerate(zip(e[:-1], e[1:])):
        thr = np.float64(nsigma) * np.float64(sigma[b])
        hit = use[b0:b1] & (np.abs(r[b0:b1]) > thr)
        for i in range(b0, b1):
            k = i - b0
            if fl[i]:
                c = INPUT
            elif not np.isfinite(d[i]):
                c = NONFINITE
            elif prev is not None and prev[i] in (HIT, NEAR):
                c = prev[i]
            elif hit[k]:
                c = HIT
            else:
                lo, hi = max(0, k - grow), min(b1 - b0, k + grow + 1)
                c = NEAR if hit[lo:k].any() or hit[k + 1:hi].any() else CLEAN
            cls[i] = c
        counts[b] = np.bincount(cls[b0:b1], minlength=5)
    return cls, counts


def flag(d, sizes, h, flags=None, nsigma=5.0, grow=2, iterations=3, sigma=None):
    """definition 8: the host's loop.  (classes, info) like GlitchFlagger.flag"""
    d = np.asarray(d, dtype=np.float64)
    given = None if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(sizes),))
    prev, hits, before, passes = None, [], 0, []
    for _ in range(iterations):
        r = residual(d, sizes, h, flags, prev)
        sig, mb = scale(d, r, sizes, h, flags, prev)
        if given is not None:
            sig = given
        cls, counts = classify(d, r, sizes, sig, nsigma, grow, flags, prev)
        hits.append(int(counts[:, HIT].sum()) - before)
        before, prev = int(counts[:, HIT].sum()), cls
        passes.append(SimpleNamespace(r=r, sigma=np.array(sig), cls=cls, counts=counts))
        if hits[-1] == 0:
            break
    info = dict(counts=counts, sigma=np.array(sig), short_blocks=np.flatnonzero(mb < 2 * h + 1), passes=len(hits),
                hits_per_pass=hits, each=passes)
    return cls, info


# -------------------------------------------------------------------------- median cases ----
def _case(name, d, sizes, h, flags=None, prev=None):
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert d.size == sum(sizes), name
    return SimpleNamespace(name=name, d=d, sizes=[int(s) for s in sizes], h=h, flags=flags, prev=prev)


def _random_flags(rng, nt, rate=0.1):
    return np.where(rng.random(nt) < rate, -1, rng.integers(0, 50, nt)).astype(np.int32)


def block_sizes(h):
    W = 2 * h + 1
    return [1, 2, h, h + 1, W - 1, W, W + 1, RUN - 1, RUN, RUN + 1, 2 * RUN + 3]


H_EDGES = (1, 8, 9, 16, 17, 32, 33, 48, 49, 64)          # both edges of every tier, and h = 1


def median_cases():
    """name -> case: block sizes and half-widths, flag patterns, values"""
    out = {}

    def add(c):
        out[c.name] = c

    for h in H_EDGES:
        rng = np.random.default_rng(100 + h)
        sizes = block_sizes(h)
        nt = sum(sizes)
        add(_case("sizes_h%d" % h, rng.standard_normal(nt), sizes, h, _random_flags(rng, nt)))
    for h in (16, 49):                             # a register tier and the LDS tier: what one workgroup covers
        G = group(h)
        rng = np.random.default_rng(200 + h)
        sizes = [G, G - 1, G + 1, RUN]
        nt = sum(sizes)
        add(_case("group_h%d" % h, rng.standard_normal(nt), sizes, h, _random_flags(rng, nt, 0.03)))
    # flag patterns, h = 4 (W = 9), two blocks
    h, sizes = 4, [200, 77]
    nt = sum(sizes)
    rng = np.random.default_rng(300)
    d = rng.standard_normal(nt)
    alt = np.where(np.arange(nt) % 2, -1, 3).astype(np.int32)
    run = np.zeros(nt, dtype=np.int32)
    run[50:50 + 25] = -1                           # longer than W
    run[80:89] = -1                                # a usable sample alone in its window: 89 between two runs
    run[90:99] = -1
    run[195:205] = -1                              # across the block boundary
    prev = rng.choice(np.array([CLEAN, INPUT, NONFINITE, HIT, NEAR], dtype=np.uint8), nt)
    add(_case("flags_none", d, sizes, h))
    add(_case("flags_all", d, sizes, h, np.full(nt, -1, dtype=np.int32)))
    add(_case("flags_alternating", d, sizes, h, alt))
    add(_case("flags_runs", d, sizes, h, run))
    add(_case("flags_bytes", d, sizes, h, (run < 0) | (rng.random(nt) < 0.2)))
    add(_case("flags_uint8", d, sizes, h, np.where(run < 0, 7, 0).astype(np.uint8)))
    add(_case("prev", d, sizes, h, None, prev))
    add(_case("prev_and_flags", d, sizes, h, run, prev))
    # values
    add(_case("three_integers", rng.integers(-1, 2, nt).astype(np.float64), sizes, h, _random_flags(rng, nt)))
    add(_case("constant", np.full(nt, 2.5), sizes, h, _random_flags(rng, nt)))
    bad = d.copy()
    bad[[0, 199, 200, 276]] = [np.nan, np.inf, -np.inf, np.nan]          # first and last sample of both blocks
    bad[[49, 75]] = [np.inf, np.nan]                                     # next to the flagged run 50..74
    add(_case("nonfinite", bad, sizes, h, run))
    huge = np.where(np.arange(nt) % 2, 1e308, -1e308)                    # every even window: 0.5 a + 0.5 b, a = -b
    huge[100:140] = 1e308                                                # and (1e308 + 1e308) / 2 would overflow
    add(_case("huge_pairs", huge, sizes, h, run))
    sub = from_bits(rng.integers(0, 1 << 20, nt).astype(np.uint64)) * np.where(rng.random(nt) < 0.5, -1.0, 1.0)
    add(_case("subnormals", sub, sizes, h, _random_flags(rng, nt)))
    return out


@functools.lru_cache(maxsize=None)
def _median_cases():
    return median_cases()


MEDIAN_CASES = tuple(median_cases())


def median_case(name):
    return _median_cases()[name]


@functools.lru_cache(maxsize=None)
def median_expected(name):
    c = median_case(name)
    r = residual(c.d, c.sizes, c.h, c.flags, c.prev)
    sigma, mb = scale(c.d, r, c.sizes, c.h, c.flags, c.prev)
    return SimpleNamespace(r=r, sigma=sigma, mb=mb)


# ----------------------------------------------------------------------- selection cases ----
def _rank_edge_keys(first):
    """25 keys whose lower median (rank 12) is the first (last) key of its histogram bin at every digit"""
    K = 0
    for sh in DIGIT_SHIFT:
        K |= 5 << sh
    other, far = [], []
    for p, sh in enumerate(DIGIT_SHIFT):
        step = 1 << sh
        other += [K + step, K + step + (3 if p < 5 else 0)] if first else [K - step, K - step - (3 if p < 5 else 0)]
    top = 1 << DIGIT_SHIFT[0]
    far = [K - 2 * top + 17 * j for j in range(12)] if first else [K + 2 * top + 17 * j for j in range(12)]
    keys = np.array([K] + other + far, dtype=np.uint64)
    assert keys.size == 25 and np.sort(keys)[12] == K
    return keys, K


def selection_cases():
    """name -> case with a made-up residual (d = 0 everywhere: usable = not flagged)"""
    out = {}

    def add(name, r, sizes, h, flags=None):
        r = np.ascontiguousarray(r, dtype=np.float64)
        out[name] = SimpleNamespace(name=name, d=np.zeros(r.size), r=r, sizes=[int(s) for s in sizes], h=h,
                                    flags=flags, prev=None)

    rng = np.random.default_rng(400)
    h, W = 3, 7
    # m_b = W - 1 (short), W, W + 1 by flags; all residuals equal; a wholly flagged block between two others
    sizes = [10, 10, 10, 12, 9, 30]
    nt = sum(sizes)
    f = np.zeros(nt, dtype=np.int32)
    f[0:4] = -1                                    # block 0: 6 usable
    f[10:13] = -1                                  # block 1: 7 usable
    f[20:22] = -1                                  # block 2: 8 usable
    f[42:51] = -1                                  # block 4: wholly flagged
    r = rng.standard_normal(nt)
    r[30:42] = 0.75                                # block 3: all equal
    add("short_and_exact", r, sizes, h, f)
    base = int(bits(np.array([1.5]))[0])
    add("lowest_digit", from_bits(np.uint64(base) + rng.permutation(2048).astype(np.uint64)) *
        np.where(rng.random(2048) < 0.5, -1.0, 1.0), [2048], h)
    add("highest_digit", from_bits(rng.permutation(256).astype(np.uint64) << np.uint64(55)), [256], h)
    for first in (True, False):
        keys, _ = _rank_edge_keys(first)
        add("rank_%s_of_bin" % ("first" if first else "last"), from_bits(rng.permutation(keys)), [25], h)
    sizes = rng.integers(7, 41, 300)
    nt = int(sizes.sum())
    add("many_small_blocks", rng.standard_normal(nt) * 10.0 ** rng.integers(-300, 300, nt), sizes, h,
        _random_flags(rng, nt))
    add("one_long_block", rng.standard_normal(20000) ** 3, [20000], h, _random_flags(rng, 20000))
    add("zeros_and_infinities", rng.choice([0.0, -0.0, np.inf, 1.0, 5e-324], 999), [500, 499], h)
    return out


@functools.lru_cache(maxsize=None)
def _selection_cases():
    return selection_cases()


SELECTION_CASES = ("short_and_exact", "lowest_digit", "highest_digit", "rank_first_of_bin", "rank_last_of_bin",
                   "many_small_blocks", "one_long_block", "zeros_and_infinities")


def selection_case(name):
    return _selection_cases()[name]


# ------------------------------------------------------------------- threshold and grow ----
SIGMA_GIVEN, NSIGMA = 0.7, 5.0
THR = NSIGMA * SIGMA_GIVEN                         # one multiplication, as definition 5 has it


def spike_case():
    """zeros with single spikes, two blocks of 3000 and 3100, h = 4: r = d exactly"""
    sizes = [3000, 3100]
    d = np.zeros(sum(sizes))
    up = np.nextafter(THR, np.inf)
    d[100] = THR                                   # equality: no hit
    d[200] = up
    d[300] = -up
    d[400] = -THR
    d[0] = 9.0                                     # first sample of block 0
    d[2999] = -9.0                                 # last sample of block 0: no NEAR in block 1
    d[3000 + 3099] = 9.0                           # last sample of the stream
    d[TILE - 1] = 9.0                              # both sides of a tile edge
    d[TILE + 30] = -9.0
    d[3000 + TILE] = 9.0                           # first sample of block 1's second tile
    d[1000] = 9.0                                  # its neighbours 999 and 1001 are flagged: INPUT, not NEAR
    d[1500] = np.nan
    flags = np.zeros(d.size, dtype=np.int32)
    flags[[999, 1001, 2500]] = -1
    return SimpleNamespace(d=d, sizes=sizes, h=4, flags=flags)


# ------------------------------------------------------------------------------ iteration ----
@functools.lru_cache(maxsize=None)
def iteration_case():
    """One block of 600 samples, h = 8, grow = 0: 30 % of the samples carry +-30 (they inflate the first pass's
    MAD) and one sample a glitch of 6.5 that only the second pass's smaller sigma reaches; the third pass adds
    nothing.  The first seed for which the restatement does exactly that."""
    n, h = 600, 8
    for seed in range(50):
        rng = np.random.default_rng(500 + seed)
        d = rng.standard_normal(n)
        dirty = rng.random(n) < 0.3
        d[dirty] += np.where(rng.random(n) < 0.5, -30.0, 30.0)[dirty]
        weak = int(np.flatnonzero(~dirty)[len(np.flatnonzero(~dirty)) // 2])
        d[weak] += 6.5
        cls, info = flag(d, [n], h, nsigma=5.0, grow=0, iterations=3)
        if info["passes"] == 3 and info["hits_per_pass"][1] >= 1 and info["hits_per_pass"][2] == 0 \
                and info["each"][0].cls[weak] == CLEAN and cls[weak] == HIT:
            return SimpleNamespace(d=d, sizes=[n], h=h, seed=seed, weak=weak, cls=cls, info=info)
    raise AssertionError("no seed gives a second pass that adds a hit and a third that adds none")


# ----------------------------------------------------------------------------- end to end ----
E2E_SEED = 0


@functools.lru_cache(maxsize=None)
def end_to_end(seed=E2E_SEED):
    """four blocks of 10 000 samples: unit white noise + 3 sin(2 pi t / 4000), 3 % flagged at random, 40 glitches of
    +-20 at unflagged positions"""
    rng = np.random.default_rng(seed)
    sizes = [10000] * 4
    nt = sum(sizes)
    t = np.arange(nt)
    clean = rng.standard_normal(nt) + 3.0 * np.sin(2.0 * np.pi * t / 4000.0)
    npix = 12 * 8 * 8
    pix = rng.integers(0, npix, nt).astype(np.int32)
    pix[rng.random(nt) < 0.03] = -1
    where = rng.choice(np.flatnonzero(pix >= 0), 40, replace=False)
    d = clean.copy()
    d[where] += np.where(rng.random(40) < 0.5, -20.0, 20.0)
    cls, info = flag(d, sizes, 16, flags=pix, nsigma=5.0, grow=2, iterations=3)
    return SimpleNamespace(d=d, clean=clean, sizes=sizes, pix=pix, npix=npix, where=np.sort(where), h=16, cls=cls,
                           info=info)
