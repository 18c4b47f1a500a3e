"""
Restatements of the gap kernels (csrc/cm2_gaps.hip) in NumPy float64, their case layouts and a table of wrong
restatements.  Plain NumPy, no GPU; nothing here imports the package under test.

Every function is written from the comment above its kernel: what the kernel promises, not how it computes it.
The kernels state their sum order and the library is built with -ffp-contract=off; NumPy's elementwise loops do
not fuse either, so every restatement is equal to the GPU bit for bit.

  * ``flagged``, ``index``, ``jacobi``, ``masked_diff``, ``finish``, ``linear`` (vectorised over the runs, each
    run's edge sums in time order), ``linear_scalar`` (one run at a time), ``window_table``, ``to_time``,
    ``to_tiles``.
  * ``case(name)``: the layouts E (edges), Ew (E with nothing flagged in its last window), M (257 blocks),
    Mall (M wholly flagged), S1 / S3 (grid-stride sizes), W0 / W1 (nine permutation windows, the last one of one
    sample, valid / flagged), P8191 and P8192 (below one window, exactly one); flags in several encodings and
    data, all from fixed seeds.
  * ``MUTATIONS``: wrong kernels, as ``mut=`` of the restatements; tests/test_gaps_ref_cpu.py shows that each of
    them changes at least one element of ``outputs`` on at least one case.
"""
import functools
from collections import namedtuple

import numpy as np

from _vector_ref import bits, assert_bit_equal  # noqa: F401

WIN = 8192                                 # csrc/cm2_tiles.h: kPermWin, time samples of one permutation window
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GRID_THREADS = 524288                      # 2048 workgroups of 256 threads: beyond it a grid-stride loop iterates
EDGE_THREADS = 131072                      # k_gap_edges launches 64-thread groups

MUTATIONS = {
    "k_for_k_plus_1": "sample s + k gets L + (R - L) k / (len + 1)",
    "len_for_len_plus_1": "sample s + k gets L + (R - L) (k + 1) / len",
    "edge_window_plus_one": "the edge windows hold nedge + 1 samples",
    "edge_not_clipped": "the edge windows reach across the block boundary",
    "fallback_swapped": "a side without a valid sample hands its 0 to the other side",
    "runs_not_cut": "a run that crosses a block boundary stays one run",
    "flagged_is_minus_one": "an int32 flag counts only when it is -1",
    "flagged_is_one": "a byte flag counts only when it is 1",
    "minus_d": "u = -d for u = 0.0 - d when there is no n",
    "finish_ignores_n": "the flagged samples get y_j where they should get n + y_j",
    "window_lower_bound_le": "c_w counts the positions <= w kPermWin",
    "jacobi_previous_block": "the first sample of a block gets 1 / a_0 of the block before",
}


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


# --------------------------------------------------------------- restatements ----
def flagged(flags, mut=None):
    """is_flagged: an int32 flag when negative, a byte (bool, uint8) when non-zero -> bool mask"""
    flags = np.asarray(flags)
    if flags.dtype == np.int32:
        return flags == -1 if mut == "flagged_is_minus_one" else flags < 0
    assert flags.dtype in (np.bool_, np.uint8), flags.dtype
    b = flags.view(np.uint8)
    return b == 1 if mut == "flagged_is_one" else b != 0


Index = namedtuple("Index", "pos runs j0 longest")


def index(mask, sizes, mut=None):
    """The handle's index: pos = ascending positions of the flagged samples (uint32); runs = rows (start, length,
    block) of the runs of consecutive flagged samples, a run ending where its block ends; j0[r] = index into pos
    of run r's first sample, j0[nruns] = ng; longest = the longest run."""
    off = offsets(sizes)
    pos = np.flatnonzero(mask).astype(np.int64)
    ng = pos.size
    if ng == 0:
        return Index(pos.astype(np.uint32), np.zeros((0, 3), dtype=np.int64), np.zeros(1, dtype=np.int64), 0)
    starts = np.ones(ng, dtype=bool)
    starts[1:] = pos[1:] != pos[:-1] + 1
    if mut != "runs_not_cut":
        starts |= np.isin(pos, off[:-1])
    j0 = np.concatenate([np.flatnonzero(starts), [ng]]).astype(np.int64)
    s = pos[j0[:-1]]
    runs = np.stack([s, np.diff(j0), np.searchsorted(off, s, side="right") - 1], axis=1).astype(np.int64)
    return Index(pos.astype(np.uint32), runs, j0, int(runs[:, 1].max()))


def jacobi(pos, sizes, a0, mut=None):
    """jac[j] = 1 / a_0(block of the j-th flagged sample)"""
    off = offsets(sizes)
    p = np.asarray(pos, dtype=np.int64)
    blk = np.searchsorted(off, p, side="right") - 1
    if mut == "jacobi_previous_block":
        blk = np.where((off[blk] == p) & (blk > 0), blk - 1, blk)
    return (1.0 / np.asarray(a0, dtype=np.float64))[blk]


def masked_diff(mask, n, d, mut=None):
    """u_i = +0.0 where flagged, n_i - d_i elsewhere, 0.0 - d_i when there is no n: a select, so whatever d or n
    hold at a flagged sample is dropped"""
    with np.errstate(all="ignore"):
        if n is None:
            diff = -d if mut == "minus_d" else 0.0 - d
        else:
            diff = n - d
    return np.where(mask, 0.0, diff)


def finish(mask, d, n, y, mut=None):
    """out = d on the valid samples, bit for bit; n + y_j (y_j when there is no n) at the j-th flagged one"""
    out = np.array(d, dtype=np.float64)
    pos = np.flatnonzero(mask)
    if pos.size:
        out[pos] = y if (n is None or mut == "finish_ignores_n") else n[pos] + y
    return out


def _edge_levels(d, mask, off, runs, nedge, nt, mut):
    """(L, R) of every run: sums in time order over the valid samples of the edge windows, loop over the offset
    inside the window, vectorised across the runs"""
    s, ln, b = runs[:, 0], runs[:, 1], runs[:, 2]
    e = s + ln
    ne = min(int(nedge), nt) + (1 if mut == "edge_window_plus_one" else 0)
    b0, b1 = (np.zeros_like(s), np.full_like(s, nt)) if mut == "edge_not_clipped" else (off[b], off[b + 1])
    levels = []
    for first, last in ((np.maximum(s - ne, b0), s), (e, np.minimum(e + ne, b1))):
        tot, cnt = np.zeros(s.size), np.zeros(s.size, dtype=np.int64)
        live = np.flatnonzero(last > first)
        k = 0
        while live.size:
            i = first[live] + k
            ok = ~mask[i]
            with np.errstate(all="ignore"):
                tot[live] = np.where(ok, tot[live] + d[i], tot[live])
            cnt[live] += ok
            k += 1
            live = live[first[live] + k < last[live]]
        with np.errstate(all="ignore"):
            levels.append((np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0), cnt))
    (L, nl), (R, nr) = levels
    if mut == "fallback_swapped":
        R = np.where(nl == 0, L, R)
        L = np.where(nr == 0, R, L)
    else:
        L = np.where(nl == 0, R, L)
        R = np.where(nr == 0, L, R)
    return L, R


def linear(d, mask, sizes, nedge, mut=None):
    """The linear fill.  For the run [s, s + len) of a block: L = (sum in time order of the valid samples among the
    nedge before s inside the block) / their number, R the same after the run; a side without a valid sample takes
    the other side's level, 0 when both have none; sample s + k becomes L + ((R - L) (k + 1)) / (len + 1).  Valid
    samples are copied bit for bit."""
    d = np.asarray(d, dtype=np.float64)
    out = d.copy()
    ix = index(mask, sizes, mut)
    if not ix.pos.size:
        return out
    L, R = _edge_levels(d, mask, offsets(sizes), ix.runs, nedge, d.size, mut)
    ln = ix.runs[:, 1]
    r = np.repeat(np.arange(ln.size), ln)
    k = np.arange(ix.pos.size, dtype=np.int64) - ix.j0[:-1][r]
    k1 = (k if mut == "k_for_k_plus_1" else k + 1).astype(np.float64)
    len1 = (ln if mut == "len_for_len_plus_1" else ln + 1).astype(np.float64)[r]
    with np.errstate(all="ignore"):          # a mutation of the flags lets a NaN or an Inf in
        out[ix.pos] = L[r] + ((R[r] - L[r]) * k1) / len1
    return out


def linear_scalar(d, mask, sizes, nedge):
    """`linear` one run and one sample at a time"""
    out = np.array(d, dtype=np.float64)
    off = offsets(sizes)
    for s, ln, b in index(mask, sizes).runs.tolist():
        e = s + ln
        sl = sr = 0.0
        nl = nr = 0
        for i in range(max(int(off[b]), s - nedge), s):
            if not mask[i]:
                sl, nl = sl + d[i], nl + 1
        for i in range(e, min(int(off[b + 1]), e + nedge)):
            if not mask[i]:
                sr, nr = sr + d[i], nr + 1
        L = sl / float(nl) if nl else 0.0
        R = sr / float(nr) if nr else 0.0
        if not nl:
            L = R
        if not nr:
            R = L
        for k in range(ln):
            out[s + k] = L + ((R - L) * float(k + 1)) / float(ln + 1)
    return out


def window_table(pos, nt, mut=None):
    """c_w, w = 0 .. nwin: the number of flagged positions below w kPermWin; None below one window"""
    if nt < WIN:
        return None
    nwin = (nt + WIN - 1) // WIN
    side = "right" if mut == "window_lower_bound_le" else "left"
    return np.searchsorted(np.asarray(pos, dtype=np.int64), np.arange(nwin + 1, dtype=np.int64) * WIN,
                           side=side).astype(np.uint32)


def to_time(src, tb, comp, pos, nt):
    """tile order -> time order with the flagged samples merged in: src[k] is the time sample held at tile-order
    position k; out[src[k]] = tb[k], out[pos[c]] = comp[c]; a sample that is neither stays NaN"""
    out = np.full(nt, np.nan)
    out[np.asarray(src, dtype=np.int64)] = tb
    out[np.asarray(pos, dtype=np.int64)] = comp
    return out


def to_tiles(src, time, pos):
    """time order -> (tile order, compact): tb[k] = time[src[k]], comp[c] = time[pos[c]]"""
    return time[np.asarray(src, dtype=np.int64)], time[np.asarray(pos, dtype=np.int64)]


# ---------------------------------------------------------------------- cases ----
E_SIZES = (1, 8191, 1, 4000, 4268)
E_NT = 2 * WIN + 77
E_NEDGES = (1, 5, 32, E_NT, E_NT + 5)
M_SIZES = tuple((1, 2, 3, 37, 64)[b % 5] for b in range(257))
S_NT = 1100000
W_NT = 8 * WIN + 1
W_COUNTS = (0, 1, 255, 256, 257, WIN, WIN - 1)       # flagged samples of windows 0 .. 6


def _mask_e(last_window=True):
    m = np.zeros(E_NT, dtype=bool)
    m[0] = True                            # a wholly flagged block of one sample
    m[3:7] = True                          # two valid samples to its left inside the block
    m[100] = True                          # isolated
    m[200:205] = True                      # two runs one valid sample apart
    m[206:210] = True
    m[300:350] = True                      # longer than nedge = 32
    m[1000:1700:2] = True                  # alternating: 350 runs
    m[8185:8196] = True                    # three runs in three blocks, across the window end at 8192
    m[12193:12200] = True                  # starts its block
    m[12150:12193] = True                  # ends its block, right against the run that starts the next
    if last_window:
        m[E_NT - 11:] = True               # ends its block and the stream
    return m


def _mask_w(last):
    rng = np.random.default_rng(4242)
    m = np.zeros(W_NT, dtype=bool)
    m[WIN + 4000] = True
    for w in (2, 3, 4):
        m[w * WIN + rng.choice(WIN, W_COUNTS[w], replace=False)] = True
    m[5 * WIN:6 * WIN] = True              # a whole window
    m[6 * WIN + 1:7 * WIN + 10] = True     # all of window 6 but its first sample, and on across the window end
    m[8 * WIN] = last
    return m


_LAYOUTS = {
    "E": lambda: (E_SIZES, _mask_e()),
    "Ew": lambda: (E_SIZES, _mask_e(False)),
    "M": lambda: (M_SIZES, np.random.default_rng(77).random(sum(M_SIZES)) < 1.0 / 3.0),
    "Mall": lambda: (M_SIZES, np.ones(sum(M_SIZES), dtype=bool)),
    "S1": lambda: ((S_NT,), _mask_s()),
    "S3": lambda: ((400001, 679999, 20000), _mask_s()),
    "W0": lambda: ((3 * WIN, W_NT - 3 * WIN), _mask_w(False)),
    "W1": lambda: ((3 * WIN, W_NT - 3 * WIN), _mask_w(True)),
    "P8191": lambda: ((5000, 3191), _mask_p(8191)),
    "P8192": lambda: ((5000, 3192), _mask_p(8192)),
}
SMALL = ("E", "Ew", "M", "Mall", "W0", "W1", "P8191", "P8192")


def _mask_s():
    m = np.zeros(S_NT, dtype=bool)
    m[0:1060000:2] = True                  # 530 000 runs of one sample
    m[1070000:1090000] = True              # one run of 20 000 (S3 cuts it at 1 080 000)
    return m


def _mask_p(nt):
    m = np.random.default_rng(nt).random(nt) < 0.05
    m[0] = m[nt - 1] = True
    m[4990:5010] = True
    return m


Case = namedtuple("Case", "name nt sizes mask i32 u8 d n y a0")


@functools.lru_cache(maxsize=None)
def case(name):
    """One shared layout with its flags in three encodings and its data.  Evaluated once; nobody writes to it.
    i32: flagged from {-1, -7, INT32_MIN}, valid from {0, 5, INT32_MAX}; u8: flagged from {1, 2, 0x80, 0xFF}; the
    mask itself is the bool encoding.  d: normals plus a slow drift, +0.0, -0.0 and a denormal among the valid
    samples, NaN / +Inf / 1e300 at the flagged ones; n: normals; y: ng normals; a0: one positive value per block."""
    sizes, mask = _LAYOUTS[name]()
    nt = int(mask.size)
    assert sum(sizes) == nt, (name, sum(sizes), nt)
    seed = 9100 + 17 * sorted(_LAYOUTS).index(name)
    rng = np.random.default_rng(seed)
    i32 = np.where(mask, rng.choice(np.array([-1, -7, INT32_MIN], dtype=np.int64), nt),
                   rng.choice(np.array([0, 5, INT32_MAX], dtype=np.int64), nt)).astype(np.int32)
    u8 = np.where(mask, rng.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), nt), 0).astype(np.uint8)
    d = rng.standard_normal(nt) + 3.0 * np.sin(np.arange(nt) / 700.0)
    valid = np.flatnonzero(~mask)
    if valid.size >= 3:
        d[valid[[valid.size // 7, valid.size // 3, valid.size // 2]]] = [-0.0, 5e-324, 0.0]
    if name in ("E", "Ew"):
        d[[205, 1001, 7]] = [0.0, -0.0, 5e-324]          # inside edge windows
    d[mask] = np.resize([np.nan, np.inf, 1e300], int(mask.sum()))
    n = rng.standard_normal(nt)
    y = rng.standard_normal(int(mask.sum()))
    a0 = 0.5 + 0.37 * np.arange(len(sizes))
    for arr in (mask, i32, u8, d, n, y, a0):
        arr.setflags(write=False)
    return Case(name, nt, tuple(sizes), mask, i32, u8, d, n, y, a0)


def nedges(cs):
    return E_NEDGES if cs.name in ("E", "Ew") else ((2,) if cs.name.startswith("S") else (32,))


@functools.lru_cache(maxsize=None)
def linear_of(name, nedge):
    out = linear(case(name).d, case(name).mask, case(name).sizes, nedge)
    out.setflags(write=False)
    return out


def outputs(cs, mut=None):
    """Every restated result of a case as a dict of arrays: what a mutation has to change somewhere"""
    mask = flagged(cs.i32, mut)
    ix = index(mask, cs.sizes, mut)
    y = cs.y if ix.pos.size == cs.y.size else np.resize(np.append(cs.y, 1.0), ix.pos.size)
    out = {"mask_i32": mask, "mask_u8": flagged(cs.u8, mut), "pos": ix.pos, "runs": ix.runs,
           "jacobi": jacobi(ix.pos, cs.sizes, cs.a0, mut),
           "masked_diff": masked_diff(mask, cs.n, cs.d, mut), "masked_diff_no_n": masked_diff(mask, None, cs.d, mut),
           "finish": finish(mask, cs.d, cs.n, y, mut), "finish_no_n": finish(mask, cs.d, None, y, mut)}
    table = window_table(ix.pos, cs.nt, mut)
    if table is not None:
        out["window_table"] = table
    for nedge in nedges(cs):
        out["linear_%d" % nedge] = linear(cs.d, mask, cs.sizes, nedge, mut)
    return out


def differing(a, b):
    """number of elements of two result dicts that differ in their bits (a changed shape counts whole)"""
    count = 0
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape:
            count += max(x.size, y.size)
        elif x.dtype == np.float64:
            count += int((bits(x) != bits(y)).sum())
        else:
            count += int((x != y).sum())
    return count
