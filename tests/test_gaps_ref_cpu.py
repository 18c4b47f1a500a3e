"""
The restatements of the gap kernels (tests/_gaps_ref.py) checked without a GPU: against the independent scalar
forms of tests/test_gpu_gap_fill.py, against their own wrong variants (MUTATIONS), and for the features that
tests/test_gpu_gap_kernels.py relies on in every layout.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gaps_ref as G  # noqa: E402
from test_gpu_gap_fill import linear_ref, runs_ref  # noqa: E402

ALL = sorted(G._LAYOUTS)


@pytest.mark.parametrize("name", ALL)
def test_index_equals_the_scalar_form(name):
    cs = G.case(name)
    ix = G.index(cs.mask, cs.sizes)
    np.testing.assert_array_equal(ix.pos, np.flatnonzero(cs.mask))
    assert ix.pos.dtype == np.uint32
    np.testing.assert_array_equal(ix.runs, runs_ref(cs.mask, list(cs.sizes)))
    np.testing.assert_array_equal(ix.j0, np.concatenate([[0], np.cumsum(ix.runs[:, 1])]))
    assert ix.longest == ix.runs[:, 1].max()
    for enc in (cs.i32, cs.u8, cs.mask):
        np.testing.assert_array_equal(G.flagged(enc), cs.mask)


@pytest.mark.parametrize("name", ALL)
def test_linear_equals_the_scalar_forms(name):
    cs = G.case(name)
    for nedge in G.nedges(cs):
        got = G.linear_of(name, nedge)
        G.assert_bit_equal(got, G.linear_scalar(cs.d, cs.mask, cs.sizes, nedge), "%s nedge %d: scalar" % (name, nedge))
        G.assert_bit_equal(got, linear_ref(cs.d, cs.mask, list(cs.sizes), nedge), "%s nedge %d: gap_fill's" % (name, nedge))
        assert np.isfinite(got).all() and np.abs(got).max() < 1e3
        G.assert_bit_equal(got[~cs.mask], cs.d[~cs.mask], "valid samples")


def test_linear_clamps_nedge_to_the_stream():
    cs = G.case("E")
    G.assert_bit_equal(G.linear(cs.d, cs.mask, cs.sizes, 2 ** 63 - 1), G.linear_of("E", cs.nt), "nedge 2^63 - 1")
    G.assert_bit_equal(G.linear(cs.d, cs.mask, cs.sizes, 2 ** 70), G.linear_of("E", cs.nt), "nedge 2^70")


def test_every_mutation_changes_an_element():
    good = {name: G.outputs(G.case(name)) for name in G.SMALL}
    for name in G.SMALL:
        assert G.differing(good[name], G.outputs(G.case(name))) == 0
    missed = []
    for mut in sorted(G.MUTATIONS):
        seen = {name: G.differing(good[name], G.outputs(G.case(name), mut)) for name in G.SMALL}
        best = max(seen, key=seen.get)
        print("%-24s %s: caught on %s, %d elements differ (%s)"
              % (mut, "caught" if seen[best] else "MISSED", best, seen[best],
                 ", ".join("%s %d" % kv for kv in sorted(seen.items()) if kv[1])))
        if not seen[best]:
            missed.append(mut)
    assert not missed, missed


def test_nothing_flagged_reaches_an_output():
    for name in G.SMALL:
        cs = G.case(name)
        assert not np.isfinite(cs.d[cs.mask]).all() or not cs.mask.any()
        for key, arr in G.outputs(cs).items():
            if np.asarray(arr).dtype == np.float64:
                assert np.isfinite(arr).all() and np.abs(arr).max() < 1e3, (name, key)


def test_permutation_restatements_invert_each_other():
    cs = G.case("W1")
    pos = np.flatnonzero(cs.mask)
    src = np.random.default_rng(1).permutation(np.flatnonzero(~cs.mask))
    time = np.arange(cs.nt, dtype=np.float64)
    tb, comp = G.to_tiles(src, time, pos)
    np.testing.assert_array_equal(tb, src)
    np.testing.assert_array_equal(comp, pos)
    G.assert_bit_equal(G.to_time(src, tb, comp, pos, cs.nt), time, "there and back")


# ------------------------------------------------------- the features of the layouts ----
def _runs(name):
    return G.index(G.case(name).mask, G.case(name).sizes).runs.tolist()


def test_layout_e_has_its_edges():
    cs, runs = G.case("E"), _runs("E")
    off = G.offsets(cs.sizes)
    assert cs.nt == 16461 == 2 * 8192 + 77 and cs.sizes == (1, 8191, 1, 4000, 4268)
    assert G.WIN in off.tolist()                                       # a block boundary on a window end
    assert [0, 1, 0] in runs and G.linear_of("E", 32)[0] == 0.0        # a wholly flagged block of one sample
    assert [8185, 7, 1] in runs and [8192, 1, 2] in runs and [8193, 3, 3] in runs
    assert [100, 1, 1] in runs                                         # isolated
    assert [200, 5, 1] in runs and [206, 4, 1] in runs and not cs.mask[205]
    assert G.index(cs.mask, cs.sizes).longest == 50 > 32
    assert [3, 4, 1] in runs and 3 - off[1] < 5                        # fewer than nedge samples to its left
    assert [12193, 7, 4] in runs and off[4] == 12193                   # starts its block
    assert [12150, 43, 3] in runs                                      # ends its block
    assert [cs.nt - 11, 11, 4] in runs                                 # ends its block and the stream
    assert sum(1 for s, ln, b in runs if 1000 <= s < 1700) == 350      # run_of searches several hundred runs
    assert len(runs) > 256
    table = G.window_table(np.flatnonzero(cs.mask), cs.nt)
    assert table.size == 4 and np.diff(table.astype(np.int64)).min() > 0
    # every window of E holds a flagged sample (0, 8192, the stream's end): Ew has none in its last window
    tw = G.window_table(np.flatnonzero(G.case("Ew").mask), cs.nt)
    assert np.diff(tw.astype(np.int64)).tolist()[2] == 0
    for enc, values in ((cs.i32[cs.mask], (-1, -7, G.INT32_MIN)), (cs.i32[~cs.mask], (0, 5, G.INT32_MAX)),
                        (cs.u8[cs.mask], (1, 2, 0x80, 0xFF))):
        assert sorted(set(enc.tolist())) == sorted(values)
    valid = cs.d[~cs.mask]
    assert (G.bits(valid) == G.bits(np.array(-0.0))).any() and (G.bits(valid) == 0).any() and (valid == 5e-324).any()
    junk = cs.d[cs.mask]
    assert np.isnan(junk).any() and np.isposinf(junk).any() and (junk == 1e300).any()


def test_layout_m_has_many_blocks():
    cs, runs = G.case("M"), np.array(_runs("M"))
    assert len(cs.sizes) == 257 and set(cs.sizes) == {1, 2, 3, 37, 64} and 5000 <= cs.nt <= 6000
    assert 0.3 <= cs.mask.mean() <= 0.37
    assert len(set(runs[:, 2].tolist())) > 150 and len(set(cs.a0.tolist())) == 257
    off = G.offsets(cs.sizes)
    assert (cs.mask[off[1:-1]] & cs.mask[off[1:-1] - 1]).sum() >= 10   # runs cut at a block boundary
    assert len(_runs("Mall")) == 257 and not G.linear_of("Mall", 32).any()


def test_layout_s_takes_every_loop_round():
    for name, nruns in (("S1", 530001), ("S3", 530002)):
        cs = G.case(name)
        ix = G.index(cs.mask, cs.sizes)
        assert cs.nt == 1100000 > G.GRID_THREADS and ix.pos.size == 550000 > G.GRID_THREADS
        assert len(ix.runs) == nruns > G.GRID_THREADS > G.EDGE_THREADS and ix.longest in (20000, 10000)
    assert len(G.case("S3").sizes) == 3 and [1080000, 10000, 2] in G.index(G.case("S3").mask, G.case("S3").sizes).runs[-2:].tolist()


def test_layout_w_has_its_windows():
    for name, last in (("W0", 0), ("W1", 1)):
        cs = G.case(name)
        assert cs.nt == 65537 == 8 * 8192 + 1
        table = G.window_table(np.flatnonzero(cs.mask), cs.nt)
        assert table.size == 10                                        # 9 windows: 16 workgroups, two per XCD
        assert np.diff(table.astype(np.int64)).tolist() == [0, 1, 255, 256, 257, 8192, 8191, 10, last]
        assert cs.mask[7 * 8192 - 1] and cs.mask[7 * 8192]             # a run across a window end
        assert G.offsets(cs.sizes)[1] % G.WIN == 0
    assert G.window_table(np.flatnonzero(G.case("P8191").mask), 8191) is None
    assert G.window_table(np.flatnonzero(G.case("P8192").mask), 8192).size == 2
