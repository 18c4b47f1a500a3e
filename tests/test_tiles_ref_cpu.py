"""
The references of tests/_tiles_ref.py, checked on the CPU before tests/test_gpu_tile_kernels.py relies on them:

  * mode 2 of the restatement with full angles equals the oracle's serial scatter loop bit for bit, and P the
    oracle's gather, on every case;
  * mode 1 equals mode 2 bit for bit where no run is longer than 256, no tile is split and no tile is hot, and
    differs in at least one bit on every case designed to regroup -- whose designed property (run lengths, groups
    per slice, parts per tile, ranges) is asserted here, so that the GPU test of that branch is not vacuous;
  * the restated policy numbers equal the literal cases tests/test_plan_policy_cpu.py pins for the header;
  * each deliberately wrong regrouping (chunks of 31, chunked from 256 instead of above 256, part boundaries
    rounded up, a tree that pairs lane t with t + 1) differs from the right one on its case.

Half-angle storage, measured here against np.longdouble cos and sin over 2e6 angles of [-pi, pi] and the
delicate ones (c = +-1, 0, -0.0; s = +-1; tiny s; pi - 1e-7): the rebuilt cos is within 3.4e-16 and the rebuilt
sin within 2.8e-16 of the true values (3.3e-16 / 2.2e-16 of the stored doubles); at the delicate angles the
rebuilt pair equals the stored one bit for bit.  First-order bound of the six roundings: 8 x 2^-53 = 8.9e-16.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ref as R  # noqa: E402

LD = R.LD
CASES = [("T1", 8191), ("T1", 8192), ("T1", 8193), ("T1", 9 * 8192 + 5)] + [("T2", s) for s in (64, 1000, 1024, 1536, 2048)] + \
    [(n, None) for n in ("T3", "T4", "T5", "T6", "T6s", "T8", "T9a", "T9b", "T10")]
SAME = ("T1", "T2", "T4")                       # mode 1 = mode 2: nothing regroups
IDS = ["%s-%s" % c if c[1] else c[0] for c in CASES]


@pytest.fixture(scope="module")
def computed(oracle):
    """(plan, v_tb, mode 1, mode 2) of a case, computed once and left unchanged"""
    cache = {}

    def get(name, arg, pol, angles):
        key = (name, arg, pol, angles)
        if key not in cache:
            cs = R.case(name, arg)
            pl = R.plan_of(cs, pol, angles)
            x, v = R.inputs(cs, pol)
            v_tb = pl.to_tiles(v)
            cache[key] = (cs, pl, x, v, v_tb, pl.Pt(v_tb, 1, cs.target), pl.Pt(v_tb, 2))
        return cache[key]
    return get


@pytest.mark.parametrize("name,arg", CASES, ids=IDS)
def test_serial_order_and_gather_equal_the_oracle(computed, oracle, name, arg):
    for pol in ((3,) if name == "T9b" else (1, 2, 3)):
        cs, pl, x, v, v_tb, m1, m2 = computed(name, arg, pol, "full")
        what = "%s pol %d" % (name, pol)
        assert not pl.half
        R.assert_bit_equal(m2, oracle.sparse_rmult(pol, cs.npix, cs.pix, cs.cos, cs.sin, v), what + ": mode 2")
        got = pl.to_time(pl.P(x))
        R.assert_bit_equal(got[pl.ok], oracle.sparse_mult(pol, cs.pix, cs.cos, cs.sin, x)[pl.ok], what + ": P")
        R.assert_bit_equal(got[~pl.ok], np.zeros(int((~pl.ok).sum())), what + ": flagged samples")
        # the tile order is a stable sort by tile: ascending tiles, ascending time inside a tile
        tile = np.searchsorted(pl.tile_p0, cs.pix[pl.tb_src], side="right") - 1
        assert np.all(np.diff(tile) >= 0) and np.all(np.diff(pl.tb_src)[np.diff(tile) == 0] > 0)
        assert np.array_equal(np.sort(pl.tb_src), np.flatnonzero(cs.pix >= 0))


@pytest.mark.parametrize("name,arg", CASES, ids=IDS)
def test_default_order_regroups_exactly_where_designed(computed, name, arg):
    for pol, angles in ([(3, "half")] if name == "T9b" else R.COMBOS):
        cs, pl, x, v, v_tb, m1, m2 = computed(name, arg, pol, angles)
        runs = R.slice_runs(pl)
        regroups = bool((runs[:, 3] > R.K_CHUNK_MIN).any() or (pl.parts(cs.target) > 1).any() or pl.hot().any())
        assert regroups == (name not in SAME)
        differ = int((R.bits(m1) != R.bits(m2)).sum())
        if regroups:
            assert differ > 0, "%s: the default order gives the serial bits, the case cannot tell them apart" % name
        else:
            R.assert_bit_equal(m1, m2, "%s: mode 1 against mode 2" % name)
        assert pl.half == (pol > 1 and angles == "half" and name != "T10")


def test_T1_windows_tiles_and_flags():
    for nt in (8191, 8192, 8193, 9 * 8192 + 5):
        cs = R.case("T1", nt)
        pl = R.plan_of(cs, 1)
        assert cs.nt == nt and 0.08 < (cs.pix < 0).mean() < 0.25
        assert pl.ntiles == 6 and pl.width[-1] == 40 < cs.tp and pl.count[2] == 0 and (np.delete(pl.count, 2) > 0).all()
        nwin = -(-nt // R.K_PERM_WIN)
        assert nwin == {8191: 1, 8192: 1, 8193: 2, 9 * 8192 + 5: 10}[nt]
        if nwin > 1:                                        # a window without one unflagged sample
            w = [bool((cs.pix[i * R.K_PERM_WIN:(i + 1) * R.K_PERM_WIN] < 0).all()) for i in range(nwin)]
            assert sum(w) == 1
    assert (10 + 7) // 8 * 8 > 10                           # the grid of 16 workgroups for 10 windows: six exit


def test_T2_last_slices_and_values_per_thread():
    vpt = set()
    for S in (64, 1000, 1024, 1536, 2048):
        pl = R.plan_of(R.case("T2", S), 3)
        assert pl.S == S
        last = pl.count - (pl.nslices - 1) * S
        assert (last == 1).any() and ((last == S) & (pl.nslices > 1)).any()
        vpt.add(max(2, -(-S // R.K_FX_T)))
    assert vpt == {2, 3, 4}                                 # the three VPT instances of k_Pt_tiles_fixed


def test_T3_T5_run_lengths_chunks_and_the_straddling_run():
    for name in ("T3", "T5", "T10"):
        pl = R.plan_of(R.case(name), 3)
        runs = R.slice_runs(pl)
        first = runs[(runs[:, 0] == 0) & (runs[:, 1] == 0)]
        assert first[:, 3].sum() == 2048 == pl.S
        assert {1, 2, 3, 4, 5, 8, 20, 59, 60, 61, 255, 256, 257, 288, 600} == set(first[:, 3].tolist())
        chunked = first[first[:, 3] > R.K_CHUNK_MIN, 3]
        assert sorted(chunked.tolist()) == [257, 288, 600]          # several chunked runs in one slice
        assert 257 % R.K_CHUNK == 1 and 288 % R.K_CHUNK == 0        # a last chunk of 1 and of 32
        assert sum(-(-int(L) // R.K_CHUNK) for L in chunked) <= 128  # (policy::kFxChunkSums)
        assert (runs[(runs[:, 0] == 0) & (runs[:, 1] == 2), 3] > R.K_CHUNK_MIN).any() and pl.nslices[0] == 3
        # groups of the runs of 5 .. 60 that precede the run of 60 in pixel order: both builders place runs in
        # that order, so in T5 the 15 groups of the run of 60 would cross a multiple of 64 without padding
        in_groups = first[(first[:, 3] > 4) & (first[:, 3] <= R.K_GROUP_RUN_MAX)]
        at = int(np.flatnonzero(in_groups[:, 3] == 60)[0])
        before = int(sum(-(-int(L) // 4) for L in in_groups[:at, 3]))
        assert (before % 64 + 15 > 64) == (name == "T5"), (name, before)


def test_T4_more_groups_than_threads():
    pl = R.plan_of(R.case("T4"), 3)
    g = R.groups_per_slice(pl)
    assert pl.S == 2048 and pl.nslices[0] == 3 and g[(0, 0)] > R.K_FX_T and g[(0, 1)] > R.K_FX_T
    assert g[(0, 2)] <= R.K_FX_T                            # (and a slice that fits one round)


def test_T6_parts():
    want = {"T6": ([1, 1, 2, 1, 5, 5, 1], (3, 3)), "T6s": ([1, 2, 2, 1, 5, 5, 1], (4, 4))}
    for name, (parts, (wg_extra, split)) in want.items():
        cs = R.case(name)
        pl = R.plan_of(cs, 3)
        assert pl.count.tolist() == R.T6_LOADS and not pl.hot().any()
        k = pl.parts(cs.target)
        assert k.tolist() == parts
        assert pl.workgroups(cs.target) == (int(sum(parts)), split)
    # T6: 1100 = 1.1 x target stays whole, 1101 is split; two parts of three slices; an empty tile inside
    pl = R.plan_of(R.case("T6"), 3)
    assert pl.nslices.tolist() == [2, 3, 3, 0, 10, 9, 2]
    assert [R.part_slice(3, j, 2) for j in range(3)] == [0, 1, 3] and [R.part_slice(9, j, 5) for j in range(6)] == [0, 1, 3, 5, 7, 9]
    # T6s: as many parts as slices
    pl = R.plan_of(R.case("T6s"), 3)
    assert pl.nslices.tolist() == [1, 2, 2, 0, 5, 5, 1] and pl.parts(600)[4] == pl.nslices[4] == 5


@pytest.mark.parametrize("name,ranges,last", [("T8", 2, 16384), ("T9a", 4, 1), ("T9b", 257, 1)])
def test_hot_tiles_and_their_ranges(name, ranges, last):
    cs = R.case(name)
    pl = R.plan_of(cs, 1)
    assert pl.tile_p0.tolist() == [0, 64, 70, 71, 128, 192, 200]
    assert pl.hot().tolist() == [False, False, True, False, False, False]
    n = int(pl.count[2])
    assert n == cs.nhot and -(-n // R.K_HOT_CHUNK) == ranges and n - (ranges - 1) * R.K_HOT_CHUNK == last
    assert (ranges > R.K_STAGE) == (name == "T9b")          # a second staging round of the range sums
    assert (pl.parts(cs.target) > 1).any() == (name == "T9a")
    # without the switch the uniform tiles stay and nothing is hot: the one-workgroup-per-tile plan
    assert R.expected_tile_p0(cs.pix, cs.npix, cs.tp, False).tolist() == [0, 64, 128, 192, 200]


def test_policy_numbers_equal_the_pinned_cases():
    """the literal rules of tests/test_plan_policy_cpu.py (its _parts_items, is_hot, hot_min and tile formulas)"""
    for ld, n, target in [(22000, 9, 20000), (22001, 9, 20000), (22001, 1, 20000), (100000, 3, 9000), (100000, 40, 9000),
                          (9900, 5, 9000), (9901, 5, 9000), (1, 1, 9000), (1101, 3, 1000), (1100, 3, 1000)]:
        pinned = 1 if (ld * 10 <= target * 11 or n <= 1) else min(-(-ld // target), n)
        assert R.parts_of(ld, n, target) == pinned
    assert [R.parts_of(*a) for a in [(22000, 9, 20000), (22001, 9, 20000), (100000, 3, 9000), (100000, 40, 9000)]] == [1, 2, 3, 12]
    assert R.K_HOT_TILE_MIN == 32768 and R.K_HOT_CHUNK == 16384 and R.K_FX_T == 512     # HOT_MIN_FLOOR, CHUNK, threads
    assert R.is_hot_tile(1, 32768) and not R.is_hot_tile(1, 32767) and not R.is_hot_tile(2, 10 ** 6)
    assert [R.part_slice(7, j, 3) for j in range(4)] == [0, 2, 4, 7]
    # the tiles with a hot pixel: unique(uniform boundaries, hot, hot + 1), hot_min = max(int(0.5 mean load), floor)
    rng = np.random.default_rng(17)
    npix, tp, nt = 32768, 64, 1 << 21
    pix = rng.integers(0, npix, nt)
    pix[rng.random(nt) < 0.05] = npix // 3
    hits = np.bincount(pix, minlength=npix)
    hot_min = max(int(0.5 * nt / (npix // tp)), 32768)
    hot = np.flatnonzero(hits >= hot_min)
    assert list(hot) == [npix // 3]
    want = np.unique(np.concatenate([np.arange(0, npix, tp), hot, hot + 1, [npix]]))
    assert np.array_equal(R.expected_tile_p0(pix, npix, tp, True), want)
    assert np.array_equal(R.expected_tile_p0(pix, npix, tp, False), np.arange(0, npix + 1, tp))
    # the LDS of k_Pt_tiles_fixed decides the values per thread: 2 up to 1024 samples, then 3 and 4
    assert [max(2, -(-S // 512)) for S in (64, 1024, 1025, 1536, 2048)] == [2, 2, 3, 3, 4]


def test_half_angles_against_long_double():
    delicate = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-0.0, 1.0), (-0.0, -1.0), (1.0, 1e-300),
                (-1.0, 1e-300), (-1.0, -1e-170), (1.0, -1e-8), (np.cos(np.pi - 1e-7), np.sin(np.pi - 1e-7)),
                (np.cos(np.pi), np.sin(np.pi))]
    c, s = np.array(delicate).T
    h, neg = R.half_angle(c, s)
    assert neg.tolist() == [False, True, False, False, False, False, False, True, True, False, True, True]
    assert np.all(np.abs(h) <= 1.0)
    cc, ss = R.rebuild(h, neg)
    R.assert_bit_equal(cc, c + 0.0, "delicate angles: cos")         # (-0.0 comes back as +0.0)
    R.assert_bit_equal(ss, s, "delicate angles: sin")
    th = np.linspace(-np.pi, np.pi, 2000001)
    c, s = np.cos(th), np.sin(th)
    assert R.on_circle(c, s) and not R.on_circle(0.5 * c, s)
    h, neg = R.half_angle(c, s)
    assert np.all(np.abs(h) <= 1.0)
    cc, ss = R.rebuild(h, neg)
    ec, es = np.abs(cc - np.cos(th.astype(LD))).max(), np.abs(ss - np.sin(th.astype(LD))).max()
    dc, ds = np.abs(cc.astype(LD) - c).max(), np.abs(ss.astype(LD) - s).max()
    print("half angles: |cos - true| %.3g, |sin - true| %.3g, against the stored doubles %.3g, %.3g" % (ec, es, dc, ds))
    bound = 8 * 2.0 ** -53
    assert max(ec, es, dc, ds) <= bound
    assert max(ec, es) > 2.2e-16                                    # (the headers used to say ~2e-16)


WRONG = [("T3", dict(chunk=31)), ("T3", dict(chunk_inclusive=True)), ("T6", dict(part_ceil=True)),
         ("T9a", dict(tree="adjacent"))]


@pytest.mark.parametrize("name,variant", WRONG, ids=["%s-%s" % (n, list(v)[0]) for n, v in WRONG])
def test_a_wrong_regrouping_is_told_apart(computed, name, variant):
    for pol, angles in [(3, "half"), (1, "half")]:
        cs, pl, x, v, v_tb, m1, m2 = computed(name, None, pol, angles)
        R.assert_bit_equal(pl.Pt(v_tb, 1, cs.target), m1, name + ": the same call again")
        wrong = pl.Pt(v_tb, 1, cs.target, **variant)
        assert (R.bits(wrong) != R.bits(m1)).any(), "%s: %r gives the right bits" % (name, variant)
        assert np.abs(wrong - m2).max() <= 1e-12 * np.abs(m2).max()   # (still a sum of the same terms)


def test_atomic_bound_accepts_any_order_and_rejects_a_wrong_term(computed):
    cs, pl, x, v, v_tb, m1, m2 = computed("T6", None, 3, "half")
    assert R.assert_atomic_ok(m1, pl, v_tb, "T6, the default order") <= 1.0
    assert R.assert_atomic_ok(m2, pl, v_tb, "T6, the serial order") == 0.0
    serial, bound, n = pl.atomic_bound(v_tb)
    assert (n == 0).any() and (bound[n == 0] == 0).all() and (bound[n > 0] > 0).all()
    bad = m2.copy()
    i = int(np.flatnonzero(n == n[n > 0].min())[0])
    bad[i] += 4 * float(bound[i]) + 1e-300
    with pytest.raises(AssertionError):
        R.assert_atomic_ok(bad, pl, v_tb, "T6, one element off")
