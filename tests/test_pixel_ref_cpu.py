"""
The restatements of the time-order pointing and per-pixel kernels (tests/_pixel_ref.py) checked without a GPU:
bit for bit against the oracle's serial loops, for the feature each case claims in the tables of
tests/test_gpu_pointing_kernels.py and tests/test_gpu_pixel_kernels.py, and against their own wrong variants (a case
that claims a branch must tell a restatement altered in that branch from the true one).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_ref as R  # noqa: E402

ALL_LAYOUTS = R.POINTING_CASES + ["hotw"]


def _pairs(names):
    return [(n, pol) for n in names for pol in R.pols_of(n)]


# ------------------------------------------------------------------ the cases' claims ----
@pytest.mark.parametrize("name", ALL_LAYOUTS)
def test_layout_is_as_prescribed(name):
    cs = R.case(name)
    assert cs.pix.dtype == np.int32 and cs.nt == cs.hits.sum() + cs.nflag
    np.testing.assert_array_equal(np.bincount(cs.pix[cs.pix >= 0], minlength=cs.npix), cs.hits)
    assert (cs.pix == -1).sum() == cs.nflag and cs.pix.min(initial=-1) >= -1
    if cs.nt > 100:
        assert np.any(np.diff(cs.pix) < 0), "samples are interleaved, not sorted by pixel"


def test_tails_reaches_every_tail_and_short_lanes():
    cs = R.case("tails")
    assert cs.npix == 130 and R.nslices(130) * 64 - 130 == 62
    for h in R.TAIL_HITS:
        assert (cs.hits == h).sum() >= 9
    for unroll in (4, 8):           # every tail length, after a body and without one
        assert {int(h) % unroll for h in cs.hits if h >= unroll} == set(range(unroll)) - ({2, 3, 4, 5} if unroll == 8 else set())
        assert {int(h) for h in cs.hits if h < unroll} == set(range(unroll))
    assert 0.08 < cs.nflag / cs.nt < 0.12
    sell_pix, sell_cnt, slice_ptr, sell_t = R.sell_direct(cs)
    width = np.diff(slice_ptr) // 64
    assert np.any(sell_cnt.reshape(-1, 64) < width[:, None]), "no lane shorter than its slice"
    assert (sell_t == 0xFFFFFFFF).sum() == slice_ptr[-1] - cs.hits.sum() > 0
    assert (sell_pix == -1).sum() == 62


@pytest.mark.parametrize("npix", R.POW2)
def test_pow2_sits_on_the_key_width(npix):
    cs = R.case("pow2-%d" % npix)
    assert cs.npix == npix and cs.hits[0] > 0 and cs.hits[-1] > 0 and cs.nflag > 0
    b = R.end_bit(npix)
    assert (1 << b) > npix >= (1 << (b - 1)), "the key npix of a flagged sample needs exactly end_bit bits"
    assert R.nslices(npix) * 64 - npix == {63: 1, 64: 0, 65: 63, 4095: 1, 4096: 0, 4097: 63}[npix]


def test_empty_and_hot_and_stride_shapes():
    e, z, h, s = R.case("empty-flagged"), R.case("empty-nt0"), R.case("hot"), R.case("stride")
    assert e.nt == 20 and e.npix == 70 and (e.pix == -1).all() and R.sell_len(e.hits) == 0
    assert z.nt == 0 and z.npix == 70 and R.sell_len(z.hits) == 0
    _, _, ptr, _ = R.sell_direct(h)
    assert list(np.diff(ptr) // 64) == [20000, 0] and h.hits[64:].sum() == 0 and h.hits[:64].min() >= 1
    assert sorted(set(h.hits[:64])) == [1, 2, 3, 20000]
    assert s.nt > R.GRID_TRIP and s.npix + 1 > R.GRID_TRIP and R.sell_len(s.hits) > R.GRID_TRIP
    assert s.npix == 524293 and (s.hits == 2).sum() == 200000 and (s.hits == 1).sum() == 200001
    assert s.hits[-1] == 1 and s.nflag == 5000 and s.nt <= 610000
    assert [R.nslices(c.npix) * 64 - c.npix for c in (e, z, s)] == [58, 58, 59], "padding slots"
    w = R.case("hotw")
    assert w.nt < 50000 and sorted(w.hits[w.hits > 100]) == [8191, 8192, 8193, 12543]
    assert 8193 % R.CHUNK == 1 and 12543 % R.CHUNK == 255 and (w.hits >= R.HOT_MIN).sum() == 3


@pytest.mark.parametrize("name", R.POINTING_CASES)
def test_sell_len_formula_equals_the_direct_construction(name):
    cs = R.case(name)
    _, sell_cnt, slice_ptr, _ = R.sell_direct(cs)
    assert R.sell_len(cs.hits) == slice_ptr[-1]
    assert np.all(np.diff(sell_cnt[:cs.npix]) <= 0) and len(slice_ptr) == R.nslices(cs.npix) + 1


# ------------------------------------------------------- restatements against the oracle ----
@pytest.mark.parametrize("name,pol", _pairs(R.POINTING_CASES))
def test_pointing_equals_the_oracle(oracle, name, pol):
    cs = R.case(name)
    x = cs.x[:pol * cs.npix]
    R.assert_bit_equal(R.P(pol, cs.pix, cs.cos, cs.sin, x), oracle.sparse_mult(pol, cs.pix, cs.cos, cs.sin, x), "P")
    want = oracle.sparse_rmult(pol, cs.npix, cs.pix, cs.cos, cs.sin, cs.v)
    R.assert_bit_equal(R.Pt(pol, cs.npix, cs.pix, cs.cos, cs.sin, cs.v), want, "Pt")
    R.assert_bit_equal(R.Pt_struct(cs, pol), want, "Pt through the index")
    for w in (cs.w, cs.w2):
        want = oracle.ptnp_diag(pol, cs.npix, cs.pix, cs.cos, cs.sin, w, x)
        R.assert_bit_equal(R.fused(pol, cs.npix, cs.pix, cs.cos, cs.sin, w, x), want, "fused")
    R.assert_bit_equal(R.fused_struct(cs, pol), oracle.ptnp_diag(pol, cs.npix, cs.pix, cs.cos, cs.sin, cs.w, x),
                       "fused through the index")
    # unit weights: the fused product is P^T (P x) bit for bit
    R.assert_bit_equal(R.fused(pol, cs.npix, cs.pix, cs.cos, cs.sin, None, x),
                       R.Pt(pol, cs.npix, cs.pix, cs.cos, cs.sin, R.P(pol, cs.pix, cs.cos, cs.sin, x)), "w = NULL")
    if cs.nt == cs.nflag:
        assert not R.Pt(pol, cs.npix, cs.pix, cs.cos, cs.sin, cs.v).view(np.int64).any(), "exact +0.0 everywhere"


@pytest.mark.parametrize("name,pol", [(n, p) for n in R.WEIGHT_CASES + ["hotw", "hot"] for p in (1, 2, 3)])
def test_processing_chain_equals_the_oracle(oracle, name, pol):
    """serial weight sums -> mask -> compaction -> flagging against oracle.process_time_samples"""
    cs = R.case(name)
    for w in (cs.w, None):
        pixs = cs.pix.copy()
        r = oracle.process_time_samples(pixs, cs.npix, pol=pol, phi=cs.phi, w=w)
        ws = R.weights(cs, pol, w)
        z = np.zeros(cs.npix)
        keep, _ = R.pixel_mask(pol, *[z if ws[k] is None else ws[k] for k in ("counts", "cos2", "sin2", "sincos")],
                               1e3)
        old2new, new_npix = R.compact(keep)
        np.testing.assert_array_equal(np.flatnonzero(keep), r.mask)
        np.testing.assert_array_equal(old2new, r.old2new)
        assert new_npix == r.new_npix
        for k in R.WRITTEN[pol]:
            R.assert_bit_equal(R.compact_apply(old2new, ws[k], np.nan)[:new_npix], getattr(r, k), k)
        np.testing.assert_array_equal(R.flag(cs.pix, old2new), pixs)
        if w is None and pol != 2:
            R.assert_bit_equal(ws["counts"], cs.hits.astype(np.float64), "unit weights: the hit counts")


@pytest.mark.parametrize("pol", (1, 2, 3))
@pytest.mark.parametrize("npix", (130, 524293))
def test_block_operators_equal_the_oracle(oracle, npix, pol):
    b = R.blocks(npix)
    x = b.x[:pol * npix]
    det, mask = R.bd_det_mask(pol, b)
    odet, omask = oracle.bd_det_mask(pol, b)
    np.testing.assert_array_equal(mask, omask)
    if pol > 1:
        R.assert_bit_equal(det, odet, "det")
        assert list(det[:4]) == [R.DET_MIN, R.DET_UP, -R.DET_MIN, -R.DET_UP] and list(mask[:4]) == [0, 1, 0, 1]
        assert det[4] == 0.0 and mask[4] == 0
    else:
        assert mask[4] == 0 and b.counts[4] == 0.0
    assert 0 < mask.sum() < npix
    R.assert_bit_equal(R.bd_precond(pol, b, det, mask, x), oracle.bd_precond_mult(pol, b, x), "M_BD")
    R.assert_bit_equal(R.bd_apply(pol, b, x), oracle.bd_mult(pol, b, x), "block apply")


@pytest.mark.parametrize("pol", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(R.SKIES))
def test_sky_maps_equal_the_oracle(oracle, name, pol):
    sk = R.sky(name)
    assert sk.obspix[0] == 0 and sk.obspix[-1] == sk.nfull - 1 and sk.npix < sk.nfull
    assert np.all(np.diff(sk.obspix) > 0)
    m = sk.map[:pol * sk.npix]
    full = R.cut_to_full(pol, sk.obspix, m, sk.nfull)
    R.assert_bit_equal(full, np.concatenate(oracle.reorganize_map(m, sk.obspix, sk.npix, sk.nside, pol)), "full")
    unseen = np.ones(sk.nfull, dtype=bool)
    unseen[sk.obspix] = False
    assert not full.reshape(pol, sk.nfull)[:, unseen].view(np.int64).any()
    back = oracle.full2cutskymap(list(full.reshape(pol, sk.nfull)), pol, sk.npix, sk.obspix)
    back = back[0] if pol == 1 else back
    R.assert_bit_equal(R.full_to_cut(pol, sk.obspix, full, sk.nfull), np.ascontiguousarray(back), "cut")
    R.assert_bit_equal(R.full_to_cut(pol, sk.obspix, full, sk.nfull), m, "round trip")


# -------------------------------------------------------------------- boundary values ----
def test_mask_rows_are_what_they_claim():
    counts, cos2, sin2, sincos = R.mask_arrays(len(R.MASK_ROWS))
    _, cond = R.pixel_mask(2, counts, cos2, sin2, sincos, 1e3)
    assert cond[0] == 1000.0 and np.isnan(cond[1]) and np.isinf(cond[2])
    assert R.THRESHOLDS[1] < 1000.0 == R.THRESHOLDS[0]
    assert counts[3] == 2.0 < counts[4] == np.nextafter(2.0, 3.0) and counts[7] == 5e-324 > 0.0 == counts[6]
    for pol in (1, 2, 3):
        for ti, thr in enumerate(R.THRESHOLDS):
            keep, _ = R.pixel_mask(pol, counts, cos2, sin2, sincos, thr)
            assert tuple(keep) == R.MASK_KEEP[(pol, ti)], (pol, ti, tuple(keep))
    big = R.mask_arrays(524293)
    assert big[0].size == 524293 > R.GRID_TRIP and big[1][11] == 1000.0


@pytest.mark.parametrize("name", R.COMPACT_CASES)
def test_compaction_patterns(name):
    keep = R.keep_pattern(name)
    old2new, new_npix = R.compact(keep)
    assert new_npix == keep.sum() and old2new.dtype == np.int32
    np.testing.assert_array_equal(old2new[keep == 1], np.arange(new_npix))
    assert (old2new[keep == 0] == -1).all()
    want = {"all": (130, 130, 1), "none": (130, 0, 0), "last-kept": (130, None, 1), "last-dropped": (130, None, 0),
            "one-kept": (1, 1, 1), "one-dropped": (1, 0, 0), "stride": (524293, None, 1)}[name]
    assert keep.size == want[0] and keep[-1] == want[2] and (want[1] is None or new_npix == want[1])
    data = np.arange(keep.size, dtype=np.float64) + 0.5
    out = R.compact_apply(old2new, data, np.nan)
    R.assert_bit_equal(out[:new_npix], data[keep == 1], "kept values in order")
    assert np.isnan(out[new_npix:]).all()


# ------------------------------------------------------------------------- hot sums ----
def test_hot_restatement_is_within_the_counted_bound():
    """(n + 2) 2^-53 sum |term|: n - 1 additions and two product roundings per term, whatever the order"""
    shares = {}
    for name in ("hotw", "hot"):
        cs = R.case(name)
        for pol in (1, 2, 3):
            for w in (cs.w, None):
                for order in ("hot", "serial"):
                    got = R.weights(cs, pol, w, order)
                    shares[(name, pol, w is not None, order)] = R.hot_share(cs, pol, w, got)
                    if w is None and pol != 2:
                        R.assert_bit_equal(got["counts"], cs.hits.astype(np.float64), "counts are exact integers")
    worst = max(shares.values())
    print("largest share of the bound: %.3g" % worst)
    assert worst <= 1.0, shares


def test_hot_sum_is_a_regrouping_only_from_the_threshold():
    cs = R.case("hotw")
    serial, hot = R.weights(cs, 3, cs.w), R.weights(cs, 3, cs.w, "hot")
    below = cs.hits < R.HOT_MIN
    for k in R.WSUMS:
        R.assert_bit_equal(hot[k][below], serial[k][below], k + " below the threshold")
    assert any(R.differing(hot[k], serial[k]) for k in R.WSUMS), "the hot order equals the serial one on this data"
    t = np.flatnonzero(cs.pix == 20)
    assert t.size == 8192 and R.hot_sum(np.ones(8193)) == 8193.0 and R.hot_sum(np.zeros(0)) == 0.0


# ---------------------------------------------------------------------- sharpness ----
def test_the_cases_tell_the_wrong_variants_apart():
    tails = R.case("tails")
    for pol in (1, 2, 3):
        assert R.differing(R.Pt_struct(tails, pol), R.Pt_struct(tails, pol, drop_tail=True)) >= pol * 80
        assert R.differing(R.fused_struct(tails, pol), R.fused_struct(tails, pol, drop_tail=True)) >= pol * 80
    for n in R.POW2:
        cs = R.case("pow2-%d" % n)
        short = R.end_bit(n) - 1
        for pol in (1, 3):
            assert R.differing(R.Pt_struct(cs, pol), R.Pt_struct(cs, pol, key_bits=short)) > 0, (n, pol)
            assert R.differing(R.fused_struct(cs, pol), R.fused_struct(cs, pol, key_bits=short)) > 0, (n, pol)
    for n in (64, 4096):            # a power of two: the flagged samples of a short key land in pixel 0
        cs = R.case("pow2-%d" % n)
        _, ptr, _ = R.pixindex(cs.pix, n, R.end_bit(n) - 1)
        assert ptr[1] - ptr[0] == cs.hits[0] + cs.nflag
    hotw = R.case("hotw")
    good, bad = R.weights(hotw, 3, hotw.w, "hot"), R.weights(hotw, 3, hotw.w, "hot", chunk=4095)
    assert sum(R.differing(good[k], bad[k]) for k in R.WSUMS) > 0, "chunk length 4095 goes unnoticed"
    for name in ("all", "last-kept", "one-kept", "stride"):
        keep = R.keep_pattern(name)
        assert R.compact(keep)[1] == R.compact(keep, use_last_keep=False)[1] + 1
    for name in ("none", "last-dropped", "one-dropped"):
        keep = R.keep_pattern(name)
        assert R.compact(keep)[1] == R.compact(keep, use_last_keep=False)[1]
