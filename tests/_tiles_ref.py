"""
Float64 references of the tile-order pointing kernels (csrc/cm2_tiles.hip, csrc/cm2_tiles_fixed.hip,
csrc/cm2_fx_lists.hip) in plain NumPy: the tile ("TB") order, the half-angle storage, P, and P^T with the
summation order of each of its three modes restated term for term.  The kernels are compiled without FMA
contraction and every order is fixed by the plan, so these restatements give the kernels' bits.  No GPU and
no import of the project: a plan is described by what the public API reports -- nt, npix, pol, the pixel,
cos and sin arrays, the tile boundaries (pixel_range(b, b + 1) of every tile), the slice length S
(fixed_order_info()[0]), the mode and the forced part target -- and everything else is derived here.

The default P^T order (mode 1), in the words DESIGN.md uses:
  * every pixel has one accumulator that starts at +0.0; the samples of its tile are walked slice by slice
    (S consecutive samples of the tile's bucket), and inside a slice the pixel's samples (its RUN) are added
    to the accumulator in time order;
  * a run of more than 256 entries inside one slice is cut into chunks of 32 consecutive entries: each chunk
    is summed in time order from 0.0, the chunk sums are added in order starting from the first chunk's sum,
    and that total is added to the accumulator once;
  * a tile with k > 1 parts: part j sums the tile's slices [ns j // k, ns (j + 1) // k) into a copy of the
    tile that starts at 0.0, and the pixel is copy_0 + copy_1 + ...; k = parts_of(load, ns, target);
  * a one-pixel tile of >= 32768 samples ("hot") is cut into ranges of 16384 samples; lane vt of 1024 adds
    the range's positions vt, vt + 1024, ... from 0.0, the lanes are halved (red[t] += red[t + h], h = 512
    ... 1), and the range sums are added in order from 0.0.
Mode 2 (exact) is the serial loop: every term in time order from +0.0.  Mode 0 (atomics) adds the same
terms in an order that is not fixed: it is held to |got - serial| <= gamma_n sum|terms| per element
(gamma_n = n u / (1 - n u), u = 2^-53, n the pixel's hits) and to exact +0.0 where n = 0.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _noise_ref import LD, assert_bit_equal, bits  # noqa: E402,F401

# ---------------------------------------------------------------- restated constants ----
K_CHUNK = 32                # kFxChunk (cm2_tiles_fixed.hip): entries per chunk of a chunked run
K_CHUNK_MIN = 256           # kFxChunkMinDefault: a run LONGER than this inside one slice is chunked
K_HOT_CHUNK = 16384         # kHotChunk: samples per range of a hot tile
K_HOT_T = 1024              # kHotT: lanes of a range
K_FX_T = 512                # policy::kFxThreads: groups of a slice handled in one round (= kHotT / 2: first stride)
K_PERM_WIN = 8192           # kPermWin (cm2_tiles.h): time samples per window of the windowed permutations
K_HOT_TILE_MIN = 32768      # policy::kHotTileMin: samples that make a one-pixel tile hot
K_GROUP_RUN_MAX = 60        # 4 (kFxMaxLevel + 1): the longest run kept in the groups of four
K_STAGE = 256               # ranges staged per round when a hot tile's range sums are added
CIRCLE_TOL = 1e-14          # k_unit_circle: |c^2 + s^2 - 1| <= this for every sample, else both arrays are kept
U = LD(2.0) ** -53


def parts_of(load, nslices, target):
    """policy::parts_of: more than 1.1 x target -> ceil(load / target) parts, never more parts than slices"""
    if load * 10 <= target * 11 or nslices <= 1:
        return 1
    return min((load + target - 1) // target, nslices)


def part_slice(nslices, j, k, ceil=False):
    """policy::part_slice: first slice of part j of k (ceil=True: the deliberately wrong variant)"""
    return -(-nslices * j // k) if ceil else nslices * j // k


def is_hot_tile(pixels, samples):
    """policy::is_hot_tile"""
    return pixels == 1 and samples >= K_HOT_TILE_MIN


def expected_tile_p0(pix, npix, tp, balance_parts):
    """The tile boundaries the plan should report: policy::uniform_tiles, and with CM2_TILE_BALANCE=parts
    policy::choose_tiling's hot_min with policy::hot_pixel_tiles (a pixel with >= hot_min hits is a tile)"""
    pix = np.asarray(pix)
    uniform = np.minimum(np.arange(-(-npix // tp) + 1) * tp, npix)
    hits = np.bincount(pix[pix >= 0], minlength=npix)
    nvalid = int(hits.sum())
    if not balance_parts or nvalid == 0:
        return uniform
    loads = np.add.reduceat(hits, uniform[:-1])
    hot_min = max(int(0.5 * (float(nvalid) / float(len(loads)))), K_HOT_TILE_MIN)
    hot = np.flatnonzero(hits >= hot_min)
    if loads.max() < hot_min or hot.size == 0:
        return uniform
    return np.unique(np.concatenate([uniform, hot, hot + 1]))


# ------------------------------------------------------------------ half angles ----
def half_angle(c, s):
    """what the plan stores: h = s / (1 + c) for c >= 0 (-0.0 included), s / (1 - c) and the sign bit otherwise"""
    c, s = np.asarray(c, np.float64), np.asarray(s, np.float64)
    neg = c < 0.0
    with np.errstate(all="ignore"):
        h = np.where(neg, s / (1.0 - c), s / (1.0 + c))
    return h, neg


def rebuild(h, neg):
    """what the kernels rebuild from it, operation for operation"""
    h2 = h * h
    inv = 1.0 / (1.0 + h2)
    cc = (1.0 - h2) * inv
    ss = (h + h) * inv
    return np.where(neg, -cc, cc), ss


def on_circle(c, s):
    r = (c * c + s * s) - 1.0
    return bool(np.all(np.abs(r) <= CIRCLE_TOL))


# ------------------------------------------------------------------------ sums ----
def segsum(terms, starts, init=None, long_from=512):
    """((init + t_0) + t_1) + ... of every segment [starts[i], starts[i + 1]) of terms [n, ncomp]; init defaults
    to +0.0.  Vectorised by rank within the segment; a long segment is one np.cumsum (a sequential scan)."""
    terms = np.asarray(terms, np.float64)
    starts = np.asarray(starts, np.int64)
    lens = np.diff(starts)
    acc = np.zeros((len(lens), terms.shape[1])) if init is None else np.array(init, np.float64)
    for i in np.flatnonzero(lens > long_from):
        acc[i] = np.cumsum(np.concatenate([acc[i:i + 1], terms[starts[i]:starts[i + 1]]], axis=0), axis=0)[-1]
    idx = np.flatnonzero((lens <= long_from) & (lens > 0))
    r = 0
    while idx.size:
        acc[idx] += terms[starts[idx] + r]
        r += 1
        idx = idx[lens[idx] > r]
    return acc


def _starts(*keys):
    """start of every run of equal key tuples in sorted arrays, closed by the length"""
    n = len(keys[0])
    if n == 0:
        return np.zeros(1, np.int64)
    new = np.zeros(n, bool)
    new[0] = True
    for k in keys:
        new[1:] |= k[1:] != k[:-1]
    return np.concatenate([np.flatnonzero(new), [n]]).astype(np.int64)


# ------------------------------------------------------------------------ plan ----
class Plan(object):
    """The tile order of a pointing.  tb_src[k]: time sample at TB position k (a stable sort of the unflagged
    samples by tile); tb_dst[t]: TB position of time sample t (-1 flagged); tile_off; q, cc, ss per TB position."""

    def __init__(self, nt, npix, pol, pix, cos, sin, tile_p0, S, full_angles=False):
        self.nt, self.npix, self.pol, self.S = int(nt), int(npix), int(pol), int(S)
        pix = np.asarray(pix, np.int64)
        assert pix.shape == (self.nt,) and pix.min() >= -1 and pix.max() < npix
        self.tile_p0 = np.asarray(tile_p0, np.int64)
        self.ntiles = len(self.tile_p0) - 1
        self.ok = pix >= 0
        tile = np.searchsorted(self.tile_p0, pix, side="right") - 1
        t_ok = np.flatnonzero(self.ok)
        self.tb_src = t_ok[np.argsort(tile[t_ok], kind="stable")]
        self.nvalid = len(self.tb_src)
        self.tb_dst = np.full(self.nt, -1, np.int64)
        self.tb_dst[self.tb_src] = np.arange(self.nvalid)
        self.count = np.bincount(tile[t_ok], minlength=self.ntiles).astype(np.int64)
        self.tile_off = np.concatenate([[0], np.cumsum(self.count)]).astype(np.int64)
        self.width = np.diff(self.tile_p0)
        self.q = pix[self.tb_src]
        self.tile_tb = np.repeat(np.arange(self.ntiles), self.count)
        self.nslices = -(-self.count // self.S) if self.S else None
        self.half = False
        self.cc = self.ss = None
        if pol > 1:
            c, s = np.asarray(cos, np.float64), np.asarray(sin, np.float64)
            self.half = (not full_angles) and on_circle(c, s)
            if self.half:
                self.h, self.neg = half_angle(c[self.tb_src], s[self.tb_src])
                self.cc, self.ss = rebuild(self.h, self.neg)
            else:
                self.cc, self.ss = c[self.tb_src].copy(), s[self.tb_src].copy()

    # -- permutations
    def to_tiles(self, v):
        return np.asarray(v)[self.tb_src]

    def to_time(self, v_tb):
        out = np.zeros(self.nt, np.asarray(v_tb).dtype)
        out[self.tb_src] = v_tb
        return out

    # -- P
    def P(self, x):
        x = np.asarray(x, np.float64).reshape(self.npix, self.pol)[self.q]
        if self.pol == 1:
            return 0.0 + x[:, 0]
        if self.pol == 2:
            return 0.0 + (x[:, 0] * self.cc + x[:, 1] * self.ss)
        return 0.0 + ((x[:, 0] + x[:, 1] * self.cc) + x[:, 2] * self.ss)

    # -- P^T
    def terms(self, v_tb):
        """[nvalid, pol]: the rounded products in the order of the map's components"""
        v = np.asarray(v_tb, np.float64)
        if self.pol == 1:
            return v[:, None].copy()
        t1, t2 = v * self.cc, v * self.ss
        return np.stack([t1, t2] if self.pol == 2 else [v, t1, t2], axis=1)

    def hot(self):
        return (self.width == 1) & (self.count >= K_HOT_TILE_MIN)

    def parts(self, target):
        """parts of every tile for the forced target (None / 0: one workgroup per tile), as parts_plan does:
        hot tiles carry no load, and a plan in which no tile is split keeps one workgroup per tile"""
        k = np.ones(self.ntiles, np.int64)
        if not target or self.S == 0:
            return k
        load = np.where(self.hot(), 0, self.count)
        if load.sum() == 0:
            return k
        for b in range(self.ntiles):
            if load[b]:
                k[b] = parts_of(int(load[b]), int(self.nslices[b]), int(target))
        return k

    def workgroups(self, target):
        """(pt_parts()["workgroups"], ["tiles_split"])"""
        k = self.parts(target)
        split = int((k > 1).sum())
        return (int(k.sum()) if split else self.ntiles), split

    def Pt(self, v_tb, mode, target=None, chunk=K_CHUNK, chunk_inclusive=False, part_ceil=False,
           tree="halving"):
        """P^T of a TB-order vector in mode 1 (default order) or 2 (serial).  chunk, chunk_inclusive, part_ceil
        and tree select the deliberately WRONG variants that tests/test_tiles_ref_cpu.py tells apart."""
        assert mode in (1, 2)
        T = self.terms(v_tb)
        out = np.zeros((self.npix, self.pol))
        hot = self.hot() if mode == 1 else np.zeros(self.ntiles, bool)
        k = self.parts(target) if mode == 1 else np.ones(self.ntiles, np.int64)
        limit = (K_CHUNK_MIN - (1 if chunk_inclusive else 0)) if mode == 1 else np.iinfo(np.int64).max
        # ---- every tile that is not hot: copies (parts) x pixels
        sel = np.flatnonzero(~hot[self.tile_tb])
        tile = self.tile_tb[sel]
        sl = (sel - self.tile_off[tile]) // self.S              # slice within the tile
        part = np.zeros(len(sel), np.int64)
        for b in np.flatnonzero(k > 1):
            cut = np.array([part_slice(int(self.nslices[b]), j, int(k[b]), part_ceil) for j in range(int(k[b]) + 1)])
            m = tile == b
            part[m] = np.searchsorted(cut, sl[m], side="right") - 1
        copy0 = np.concatenate([[0], np.cumsum(k)])
        copy = copy0[tile] + part
        order = np.lexsort((self.q[sel], copy))                 # stable: time order within (copy, pixel)
        copy, q, sl, Ts = copy[order], self.q[sel][order], sl[order], T[sel][order]
        run = _starts(copy, q, sl)
        rlen = np.diff(run)
        keep = np.ones(len(q), bool)
        for r in np.flatnonzero(rlen > limit):                  # chunked runs: one item, the total
            a, e = run[r], run[r + 1]
            cs = segsum(Ts[a:e], np.concatenate([np.arange(0, e - a, chunk), [e - a]]))
            tot = cs[0].copy()
            for c in cs[1:]:
                tot = tot + c
            Ts[a] = tot
            keep[a + 1:e] = False
        copy, q, Ts = copy[keep], q[keep], Ts[keep]
        seg = _starts(copy, q)
        val = segsum(Ts, seg)
        scopy, sq = copy[seg[:-1]], q[seg[:-1]]
        stile = np.searchsorted(copy0, scopy, side="right") - 1
        one = k[stile] == 1
        out[sq[one]] = val[one]
        for b in np.flatnonzero(k > 1):
            copies = np.zeros((int(k[b]), int(self.width[b]), self.pol))
            m = stile == b
            copies[scopy[m] - copy0[b], sq[m] - self.tile_p0[b]] = val[m]
            acc = copies[0].copy()
            for j in range(1, int(k[b])):
                acc = acc + copies[j]
            out[self.tile_p0[b]:self.tile_p0[b + 1]] = acc
        # ---- hot tiles: ranges, lanes, tree, range sums
        for b in np.flatnonzero(hot):
            t = T[self.tile_off[b]:self.tile_off[b + 1]]
            n = len(t)
            nr = -(-n // K_HOT_CHUNK)
            pad = np.zeros((nr * K_HOT_CHUNK, self.pol))
            pad[:n] = t
            pad = pad.reshape(nr, K_HOT_CHUNK // K_HOT_T, K_HOT_T, self.pol)
            valid = (np.arange(nr * K_HOT_CHUNK) < n).reshape(nr, K_HOT_CHUNK // K_HOT_T, K_HOT_T)
            red = np.zeros((nr, K_HOT_T, self.pol))
            for j in range(K_HOT_CHUNK // K_HOT_T):
                red[valid[:, j]] += pad[:, j][valid[:, j]]
            if tree == "halving":
                h = K_HOT_T // 2
                while h >= 1:
                    red[:, :h] += red[:, h:2 * h]
                    h //= 2
            else:                                               # wrong: lane t paired with t + 1, then t + 2, ...
                s = 1
                while s < K_HOT_T:
                    red[:, ::2 * s] += red[:, s::2 * s]
                    s *= 2
            out[self.tile_p0[b]] = segsum(red[:, 0], [0, nr], long_from=0)[0]
        return out.reshape(-1)

    def atomic_bound(self, v_tb, serial=None):
        """(serial result, gamma_n sum|terms|, hits n) per element, each [npix * pol]; the bound in long double"""
        T = self.terms(v_tb)
        order = np.argsort(self.q, kind="stable")
        seg = _starts(self.q[order])
        n = np.zeros(self.npix, np.int64)
        sabs = np.zeros((self.npix, self.pol), LD)
        if len(order):
            n[self.q[order][seg[:-1]]] = np.diff(seg)
            sabs[self.q[order][seg[:-1]]] = np.add.reduceat(np.abs(T[order]).astype(LD), seg[:-1], axis=0)
        nu = n.astype(LD) * U
        serial = self.Pt(v_tb, 2) if serial is None else serial
        return serial, ((nu / (1 - nu))[:, None] * sabs).reshape(-1), np.repeat(n, self.pol)


def assert_atomic_ok(got, plan, v_tb, what, serial=None):
    """every element of an atomic-order result within gamma_n sum|terms| of the serial sum, exact +0.0 where the
    pixel has no hit; returns the largest share of the bound that was used"""
    serial, bound, n = plan.atomic_bound(v_tb, serial)
    err = np.abs(np.asarray(got, np.float64).astype(LD) - serial.astype(LD))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, "%s: %d elements outside gamma_n sum|terms|, first at %d: got %r, serial %r, bound %.3g" % (
        what, bad.size, bad[0], got[bad[0]], serial[bad[0]], float(bound[bad[0]]))
    assert_bit_equal(np.asarray(got)[n == 0], np.zeros(int((n == 0).sum())), what + ": pixels without a hit")
    worst = float((err[n > 0] / np.maximum(bound[n > 0], LD(1e-300))).max()) if (n > 0).any() else 0.0
    return worst


# ----------------------------------------------------------------------- cases ----
COMBOS = [(1, "half"), (2, "half"), (2, "full"), (3, "half"), (3, "full")]      # the five <POL, HALF> instances
RAMP_COMBOS = [(3, "half"), (1, "half")]


def _merge(seqs):
    """one time stream from per-tile pixel sequences: sample i of a sequence of n at time (i + 0.5) / n, so that
    every tile's samples are spread over the whole stream and keep their order"""
    key = np.concatenate([(np.arange(len(s)) + 0.5) / max(len(s), 1) for s in seqs])
    return np.concatenate(seqs)[np.argsort(key, kind="stable")].astype(np.int64)


def _flag_every(pix, every, at):
    """a flagged sample in front of every `every`-th sample"""
    out = []
    for i in range(0, len(pix), every):
        blk = pix[i:i + every]
        out += [blk[:at], [-1], blk[at:]]
    return np.concatenate(out).astype(np.int64)


def _perm(n, mult):
    while np.gcd(mult, n) != 1:
        mult += 1
    return (np.arange(n) * mult) % n


def _slice_of_runs(lengths, pixels, mult=1009):
    """samples of one slice: pixel pixels[i] hit lengths[i] times, in a fixed shuffled order"""
    s = np.repeat(np.asarray(pixels), np.asarray(lengths))
    return s[_perm(len(s), mult)]


T3_RUNS = [60, 1, 4, 5, 8, 59, 61, 255, 256, 257, 600, 288, 2, 3] + [20] * 7 + [1] * 49      # 2048 samples
T5_RUNS = [59, 8, 5] + [20] * 7 + [60, 1, 4, 61, 255, 256, 257, 600, 288, 2, 3] + [1] * 49    # the same runs
T3_LAST = [300, 100, 61, 60, 30, 8, 5, 4, 3, 2] + [1] * 27                                     # 600 samples


def _runs_case(runs):
    assert sum(runs) == 2048 and sum(T3_LAST) == 600
    tp, npix = 256, 2 * 256 + 100
    ids = np.arange(len(runs))
    tile0 = np.concatenate([_slice_of_runs(runs, ids), _slice_of_runs(runs, ids[::-1] + 100, 811),
                            _slice_of_runs(T3_LAST, np.arange(len(T3_LAST)) * 5 + 1, 409)])
    tile1 = 256 + (np.arange(500) * 7 + np.arange(500) // 11) % 256
    tile2 = 512 + (np.arange(300) * 3) % 100
    return dict(tp=tp, npix=npix, pix=_flag_every(_merge([tile0, tile1, tile2]), 17, 5),
                env={"CM2_PT_SLICE": "2048"}, S=2048, runs=runs)


def _tile_seq(p0, width, n, a=7, d=13):
    i = np.arange(n)
    return p0 + (i * a + i // d) % width


T6_LOADS = [900, 1100, 1101, 0, 5000, 4300, 700]


def _hot_case(nhot, loads, S, target):
    """pixel 70 of 200 hit nhot times; uniform tiles of 64 pixels otherwise loaded with `loads` samples"""
    beside = np.concatenate([np.arange(64, 70), np.arange(71, 128)])            # the hot pixel's uniform tile
    seqs = [_tile_seq(0, 64, loads[0]), beside[_tile_seq(0, 63, loads[1])], np.full(nhot, 70),
            _tile_seq(128, 64, loads[2]), _tile_seq(192, 8, loads[3], 3, 5)]
    return dict(tp=64, npix=200, pix=_flag_every(_merge(seqs), 29, 11),
                env={"CM2_TILE_BALANCE": "parts", "CM2_PT_PARTS": str(target), "CM2_PT_SLICE": str(S)},
                S=S, target=target, balance_parts=True, nhot=nhot)


def case(name, arg=None):
    """The pointing of a case: nt, npix, tp, pix, the switches (env), for the CPU checks the slice length S where
    the switches fix it, and the forced part target"""
    if name == "T1":
        nt, tp, npix = int(arg), 64, 360
        allowed = np.concatenate([np.arange(0, 128), np.arange(192, 360)])       # tile 2 gets no sample
        t = np.arange(nt)
        pix = allowed[(t * 37 + t // 64) % len(allowed)]
        pix[t % 10 == 3] = -1
        nwin = -(-nt // K_PERM_WIN)
        if nwin > 1:                                                             # one window flagged entirely
            w = nwin // 2
            pix[w * K_PERM_WIN:(w + 1) * K_PERM_WIN] = -1
        d = dict(tp=tp, npix=npix, pix=pix, env={}, S=None)
    elif name == "T2":
        S, tp, sl = int(arg), 64, (64, 1000, 1024, 1536, 2048)
        counts = [s + 1 for s in sl] + [2 * s for s in sl] + [777]
        seqs = [_tile_seq(64 * b, 64, n, 5, 9) for b, n in enumerate(counts)]
        d = dict(tp=tp, npix=64 * len(counts), pix=_flag_every(_merge(seqs), 23, 7), env={"CM2_PT_SLICE": str(S)}, S=S)
    elif name == "T3":
        d = _runs_case(T3_RUNS)
    elif name == "T5":
        d = _runs_case(T5_RUNS)
    elif name == "T4":
        # every pixel that is hit is hit 5 times per slice: 409 pixels (5 x 512 samples do not fit a slice of 2048) and
        # three singles fill it, two groups per run of 5: 819 groups for 512 threads
        def sl(first, npx, nsingle):
            p = (first + np.arange(npx + nsingle)) % 512
            return _slice_of_runs([5] * npx + [1] * nsingle, p, 1013)
        tile0 = np.concatenate([sl(0, 409, 3), sl(200, 409, 3), sl(77, 200, 0)])
        d = dict(tp=512, npix=1034, pix=_flag_every(_merge([tile0, _tile_seq(512, 512, 900), _tile_seq(1024, 10, 40, 3, 5)]),
                                                    31, 3), env={"CM2_PT_SLICE": "2048"}, S=2048)
    elif name in ("T6", "T6s"):
        S, target = (512, 1000) if name == "T6" else (1024, 600)
        seqs = [_tile_seq(64 * b, 64 if b < 6 else 40, n) for b, n in enumerate(T6_LOADS)]
        d = dict(tp=64, npix=424, pix=_flag_every(_merge(seqs), 19, 2),
                 env={"CM2_TILE_BALANCE": "parts", "CM2_PT_PARTS": str(target), "CM2_PT_SLICE": str(S)},
                 S=S, target=target, balance_parts=True)
    elif name == "T8":
        d = _hot_case(32768, [1500, 1200, 1500, 300], 2048, 0)
    elif name == "T9a":
        d = _hot_case(32768 + 16384 + 1, [1500, 1200, 4000, 300], 512, 1500)
    elif name == "T9b":
        d = _hot_case(256 * 16384 + 1, [600, 500, 600, 100], 2048, 0)
    elif name == "T10":
        d = _runs_case(T3_RUNS)
        d["cos_scale"] = 0.5
    else:
        raise KeyError(name)
    d.setdefault("target", None)
    d.setdefault("balance_parts", False)
    d.setdefault("cos_scale", 1.0)
    cs = SimpleNamespace(name=name, arg=arg, nt=len(d["pix"]), **d)
    phi = 0.3 + 0.0785 * np.arange(cs.nt)
    cs.cos, cs.sin = cs.cos_scale * np.cos(2 * phi), np.sin(2 * phi)
    return cs


def inputs(cs, pol, seed=0):
    """(map x, time stream v) of a case: standard normals (of a seed at which every case designed to regroup differs
    from the serial sum in every storage form, which tests/test_tiles_ref_cpu.py asserts)"""
    rng = np.random.default_rng(1001 + seed)
    return rng.standard_normal(cs.npix * pol), rng.standard_normal(cs.nt)


def plan_of(cs, pol, angles="half", S=None, tile_p0=None):
    """the reference plan of a case from the restated tile rule (a GPU test passes what the plan reports)"""
    if tile_p0 is None:
        tile_p0 = expected_tile_p0(cs.pix, cs.npix, cs.tp, cs.balance_parts)
    return Plan(cs.nt, cs.npix, pol, cs.pix, cs.cos, cs.sin, tile_p0, S or cs.S or 1536, full_angles=(angles == "full"))


def slice_runs(plan):
    """[(tile, slice, pixel, length)] of every run: the samples of one pixel inside one slice"""
    sl = (np.arange(plan.nvalid) - plan.tile_off[plan.tile_tb]) // plan.S
    order = np.lexsort((plan.q, sl, plan.tile_tb))
    t, s, q = plan.tile_tb[order], sl[order], plan.q[order]
    st = _starts(t, s, q)
    return np.stack([t[st[:-1]], s[st[:-1]], q[st[:-1]], np.diff(st)], axis=1)


def groups_per_slice(plan):
    """{(tile, slice): groups of four a slice needs at least}: ceil(L / 4) for every run of 5 .. 60, and the
    shorter runs four entries to a group (both builders need at least this many)"""
    out = {}
    for t, s, q, L in slice_runs(plan):
        g, short = out.get((t, s), (0, 0))
        if 4 < L <= K_GROUP_RUN_MAX:
            g += -(-L // 4)
        elif L <= 4:
            short += L
        out[(t, s)] = (g, short)
    return {key: g + -(-short // 4) for key, (g, short) in out.items()}
