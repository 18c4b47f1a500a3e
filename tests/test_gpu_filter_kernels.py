"""
Every branch of the time-stream filter kernels (csrc/cm2_filter.hip) against the references of
tests/_filter_ref.py.

Conventions of every case: each output buffer and each tile-order buffer is the middle of a larger
buffer pre-filled with a sentinel whose bits must be unchanged after the call, and holds NaN
before the call: a sample nobody wrote stays NaN.  A result is accepted, element by element, when
it is bit-equal to the float64 restatement or when |got - ref| <= c 2^-53 S; where S = 0 (gaps,
skipped chunks, flagged samples of the fit) it must be exactly 0.  On top of that the mean and
the no-flag fit must be bit-equal to the restatement for all three chunk carriers, and the tile
order must be bit-equal to the time order at every unflagged sample.

Kernels and the case that reaches them (to be kept in step with the dispatch code by hand):

  cm2_filter_create       k_filter_setup<2..8>          test_time_order[1..7]: chunks with fewer than K,
                                                        exactly K - 1, exactly K, all and some samples
                                                        unflagged; first / last sample flagged
  cm2_filter_apply        k_filter_mean                 test_time_order[0]; test_single_chunk[0]
                          k_filter_poly<2..8>           test_time_order[1..7]; test_single_chunk[3]
                            RegChunk<8>                 chunks of 1 .. 512 samples
                            RegChunk<32>                513 .. 2048
                            MemChunk                    2049, 4100 (and 8193 in test_tile_order[d-*])
                          hipMemsetAsync (no chunk)     tests/test_gpu_parity.py
  cm2_filter_apply_tiles  filter_windows_build          test_tile_order: layouts a, b1, b7, b8, c0 .. c3
                                                        (tileable), d (a chunk of 8193 samples: not)
                          k_win_keys, window_lists      every tileable layout; rebuilt for another plan id
                          (cm2_tiles.hip)               in test_tile_order_second_plan
                          k_filter_windows<0,2..8>      test_tile_order[a-0..7]; nwin = 9 (16 workgroups,
                                                        7 exit), 1, 7, 8, 2
                          hipMemsetAsync (win_memset)   test_tile_order[c1|c2|c3-*]
  cm2_ground_bin_sums     k_ground_bin                  test_ground_kernels (1 .. 8192 bins: 64 KB of LDS)
  cm2_ground_subtract     k_ground_subtract             test_ground_kernels
  GroundFilterLO with 8193 bins (P^T route)             test_ground_filter_more_bins_than_lds
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8DEAD0000BEEF        # a NaN with a payload: no kernel produces these bits
GUARD = 8                            # sentinels in front of and behind the data


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, L=L, D=device, hip=_hip, torch=torch)


class Guarded(object):
    """n doubles in the middle of a sentinel-filled buffer; data=None: NaN (an output)"""

    def __init__(self, cm, n, data=None):
        torch = cm.torch
        self.cm, self.n = cm, int(n)
        self.buf = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.int64,
                              device=cm.D.dev()).view(torch.float64)
        self.v = self.buf[GUARD:GUARD + self.n]
        if data is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(cm.D.to_dev(np.ascontiguousarray(data, dtype=np.float64).reshape(-1)))

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        self.cm.torch.cuda.synchronize()
        return self.v.cpu().numpy().copy()

    def intact(self, what):
        raw = self.buf.view(self.cm.torch.int64)
        assert bool((raw[:GUARD] == SENTINEL).all().item()) and \
            bool((raw[GUARD + self.n:] == SENTINEL).all().item()), \
            "%s: wrote outside its %d elements" % (what, self.n)


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def _tables(F):
    return getattr(F, "legendres", {})


def _accept(what, got, want, ref, S, c, starts, lens, kinds):
    """the acceptance rule on a whole stream, and the promised bit-equalities chunk by chunk;
    -> (flagged chunks bit-equal to the restatement, flagged chunks, largest share of the bound)"""
    assert not np.isnan(got).any(), what + ": a NaN is left"
    covered = np.zeros(got.size, dtype=bool)
    same = total = 0
    for (a, n), kind in zip(zip(starts, lens), kinds):
        sl = slice(int(a), int(a + n))
        covered[sl] = True
        if kind == 2:
            total += 1
            same += int((R.bits(got[sl]) == R.bits(want[sl])).all())
        else:
            R.assert_bit_equal(got[sl], want[sl], "%s: chunk at %d, %d samples, kind %s" % (what, a, n, kind))
    R.assert_bit_equal(got[~covered], np.zeros(int((~covered).sum())), what + ": gaps")
    equal = R.bits(got) == R.bits(want)
    e = R.excess(got[~equal], ref[~equal], S[~equal], c[~equal])
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 S" % (what, e)
    return same, total, e


# ===================================================================== time order ===
@functools.lru_cache(maxsize=None)
def time_refs(order, scale):
    from cosmomap2_amd.utilities.linear_algebra_funcs import get_legendre_polynomials
    case = R.time_case(order)
    leg = {int(n): get_legendre_polynomials(order, int(n)) for n in set(case.lens) if n > 0} if order else {}
    d = case.d * scale
    ref, S, c, kinds = R.stream_ref(order, case.starts, case.lens, case.pix, d, leg)
    want = R.stream_f64(order, case.starts, case.lens, case.pix, d, leg)
    return case, d, ref, S, c, kinds, want, leg


@pytest.mark.parametrize("order", range(8))
def test_time_order(cm, order):
    case = R.time_case(order)
    F = cm.I.FilterLO(case.nt, case.args[0], case.args[1], case.args[2], case.pix, poly_order=order)
    h = F._plan_for(order).h
    leg = time_refs(order, 1.0)[-1]                        # the references read the same tables
    assert sorted(leg) == sorted(_tables(F))               # as the handle was given
    for n in leg:
        R.assert_bit_equal(F.legendres[n], leg[n], "Legendre table, %d samples" % n)
    for scale in (1.0, 2.0 ** 20):
        case, d, ref, S, c, kinds, want, _ = time_refs(order, scale)
        what = "order %d, input x %g" % (order, scale)
        gin, out = Guarded(cm, case.nt, d), Guarded(cm, case.nt)
        call(cm, "cm2_filter_apply", h, gin.ptr, out.ptr)
        got = out.get()
        out.intact(what)
        gin.intact(what)
        same, total, e = _accept(what, got, want, ref, S, c, case.starts, case.lens, kinds)
        print("%s: %d chunks; %d of %d flagged chunks bit-equal to the restatement, the others use "
              "%.3f of the bound (c = %s)" % (what, len(kinds), same, total, e,
                                              R.c_flagged(order) if order else "-"))
        R.assert_bit_equal(gin.get(), d, what + ": input untouched")
    info = F.filter_info()
    assert info["nchunks"] == len(case.starts) and info["covered"] == int(case.lens.sum())
    count = [kinds.count(k) if order else 0 for k in (0, 1, 2)]
    assert [info["skipped"], info["unflagged"], info["flagged"]] == count, (info, count)


@pytest.mark.parametrize("order", [0, 3])
def test_single_chunk(cm, order):
    """nseg = 1: three of the workgroup's four waves have no chunk"""
    rng = np.random.default_rng(40 + order)
    nt = 150
    pix = rng.integers(0, 50, size=nt).astype(np.int32)
    pix[rng.random(nt) < 0.1] = -1
    d = rng.standard_normal(nt) + 3.0
    starts, lens = np.array([5], dtype=np.int64), np.array([100], dtype=np.int64)
    F = cm.I.FilterLO(nt, [lens, starts], nt, 1, pix, poly_order=order)
    leg = _tables(F)
    ref, S, c, kinds = R.stream_ref(order, starts, lens, pix, d, leg)
    want = R.stream_f64(order, starts, lens, pix, d, leg)
    gin, out = Guarded(cm, nt, d), Guarded(cm, nt)
    call(cm, "cm2_filter_apply", F._plan_for(order).h, gin.ptr, out.ptr)
    _accept("one chunk, order %d" % order, out.get(), want, ref, S, c, starts, lens, kinds)
    out.intact("one chunk")
    assert F.filter_info()["nchunks"] == 1


# ===================================================================== tile order ===
@functools.lru_cache(maxsize=None)
def tile_refs(name, order):
    from cosmomap2_amd.utilities.linear_algebra_funcs import get_legendre_polynomials
    case = R.tile_case(name, order)
    leg = {int(n): get_legendre_polynomials(order, int(n)) for n in set(case.lens) if n > 0} if order else {}
    ref, S, c, kinds = R.stream_ref(order, case.starts, case.lens, case.pix, case.d, leg)
    want = R.stream_f64(order, case.starts, case.lens, case.pix, case.d, leg)
    return case, ref, S, c, kinds, want, R.windows_plan(case.starts, case.lens, case.nt)


def _tile_plan(cm, case, tile_pixels):
    P = cm.I.SparseLO(R.NPIX_TILES, case.nt, case.pix, pol=1)
    T = cm.L._sparse_tiles(P, tile_pixels=tile_pixels, slice_samples=4096)
    assert T.nvalid == int((case.pix >= 0).sum())
    return P, T


def _time_order(cm, F, case, refs, what):
    _, ref, S, c, kinds, want, _ = refs
    gin, out = Guarded(cm, case.nt, case.d), Guarded(cm, case.nt)
    call(cm, "cm2_filter_apply", F._plan_for(case.order).h, gin.ptr, out.ptr)
    got = out.get()
    out.intact(what)
    _accept(what + ", time order", got, want, ref, S, c, case.starts, case.lens, kinds)
    return gin, got


def _through_tiles(cm, F, T, case, refs, gin, time_out, what):
    """time -> tiles, _apply_tiles, tiles -> time; every buffer NaN between sentinels"""
    _, ref, S, c, kinds, want, plan = refs
    ok = case.pix >= 0
    d_tb, out_tb, back = Guarded(cm, T.nvalid), Guarded(cm, T.nvalid), Guarded(cm, case.nt)
    call(cm, "cm2_tod_time_to_tiles", T.h, gin.ptr, d_tb.ptr)
    assert not np.isnan(d_tb.get()).any()
    done = F._apply_tiles(T, d_tb.v, out_tb.v)
    assert done == plan.ok, "%s: windows_plan says %r, _apply_tiles returned %r" % (what, plan.ok, done)
    for g in (d_tb, out_tb):
        g.intact(what)
    if not done:
        assert np.isnan(out_tb.get()).all(), what + ": wrote although it declined"
        return
    assert not np.isnan(out_tb.get()).any(), what + ": a NaN is left in the tile order"
    call(cm, "cm2_tod_tiles_to_time", T.h, out_tb.ptr, back.ptr)
    got = back.get()
    back.intact(what)
    R.assert_bit_equal(got[ok], time_out[ok], what + ": tile order against time order")
    R.assert_bit_equal(got[~ok], np.zeros(int((~ok).sum())), what + ": flagged samples")
    equal = R.bits(got) == R.bits(want)
    e = R.excess(got[ok & ~equal], ref[ok & ~equal], S[ok & ~equal], c[ok & ~equal])
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 S" % (what, e)


@pytest.mark.parametrize("name,order", [(n, o) for n, orders in R.TILE_LAYOUTS.items() for o in orders],
                         ids=lambda v: str(v))
def test_tile_order(cm, name, order):
    refs = tile_refs(name, order)
    case, plan = refs[0], refs[-1]
    what = "layout %s, order %d" % (name, order)
    if name == "a":
        assert plan.nwin == 9 and [w[3] - w[2] for w in plan.wins] == case.per_window
    if plan.ok:
        assert plan.memset == case.memset
    P, T = _tile_plan(cm, case, 64)
    F = cm.I.FilterLO(case.nt, case.args[0], case.args[1], case.args[2], case.pix, poly_order=order)
    assert F._tile_compatible(P)
    gin, time_out = _time_order(cm, F, case, refs, what)
    _through_tiles(cm, F, T, case, refs, gin, time_out, what)


@pytest.mark.parametrize("order", R.TILE_ORDERS_FEW)
def test_tile_order_second_plan(cm, order):
    """the window lists belong to one tile plan: another plan, then the first one again"""
    refs = tile_refs(R.TILE_LAYOUT_E, order)
    case = refs[0]
    (P1, T1), (P2, T2) = _tile_plan(cm, case, 64), _tile_plan(cm, case, 256)
    assert T1.plan_id != T2.plan_id
    F = cm.I.FilterLO(case.nt, case.args[0], case.args[1], case.args[2], case.pix, poly_order=order)
    gin, time_out = _time_order(cm, F, case, refs, "second plan, order %d" % order)
    for T, what in ((T1, "first plan"), (T2, "second plan"), (T1, "first plan again"), (T2, "second again")):
        _through_tiles(cm, F, T, case, refs, gin, time_out, "%s, order %d" % (what, order))


# ================================================================== ground filter ===
@functools.lru_cache(maxsize=None)
def ground_refs(nt, nbins):
    g, v = R.ground_case(nt, nbins)
    return (g, v) + R.ground_ref(g, v, nbins)


@pytest.mark.parametrize("nt,nbins", R.GROUND_SHAPES)
def test_ground_kernels(cm, nt, nbins):
    g, v, sums_ref, mags, hits, out_ref, S, hs = ground_refs(nt, nbins)
    what = "ground nt=%d nbins=%d" % (nt, nbins)
    ok = g >= 0
    lab = cm.D.i32(g)
    gv, sums = Guarded(cm, nt, v), Guarded(cm, nbins)
    call(cm, "cm2_ground_bin_sums", nt, nbins, lab.data_ptr(), gv.ptr, sums.ptr)
    got = sums.get()
    sums.intact(what)
    e = R.assert_within(got, sums_ref, mags, R.c_ground_sums(hits), what + ": bin sums")
    print("%s: bin sums use %.3f of the bound" % (what, e))
    # the subtraction alone, from the sums just made: one rounding, the same bits every time
    binned = np.where(hits > 0, got / np.maximum(hits, 1), 0.0)
    gb = Guarded(cm, nbins, binned)
    want = np.where(ok, v - binned[np.where(ok, g, 0)], v)
    for _ in range(2):
        out = Guarded(cm, nt)
        call(cm, "cm2_ground_subtract", nt, lab.data_ptr(), gb.ptr, gv.ptr, out.ptr)
        R.assert_bit_equal(out.get(), want, what + ": subtract")
        out.intact(what)
    R.assert_within(want, out_ref, S, R.c_ground_filtered(hs), what + ": subtract against the reference")
    # the operator
    Fg = cm.I.GroundFilterLO(g)
    assert Fg.nbins == nbins and Fg.n == nt
    y = Fg * v
    R.assert_within(y, out_ref, S, R.c_ground_filtered(hs), what + ": GroundFilterLO")
    R.assert_bit_equal(y[~ok], v[~ok], what + ": samples without a bin")
    np.testing.assert_array_equal(Fg.counts_in_groundbins(g), hits.astype(np.float64))


def test_ground_filter_more_bins_than_lds(cm):
    """8193 bins: the bin sums go through the pixel-major P^T"""
    nt, nbins = 100001, 8193
    g, v, sums_ref, mags, hits, out_ref, S, hs = ground_refs(nt, nbins)
    Fg = cm.I.GroundFilterLO(g)
    assert Fg.nbins == nbins > Fg.LDS_BINS
    y = Fg * v
    R.assert_within(y, out_ref, S, R.c_ground_filtered(hs), "GroundFilterLO, 8193 bins")
    R.assert_bit_equal(y[g < 0], v[g < 0], "samples without a bin")
    R.assert_within(cm.D.to_host(Fg._bin_sums(cm.D.f64(v))), sums_ref, mags, R.c_ground_sums(hits), "P^T bin sums")
