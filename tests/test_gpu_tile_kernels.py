"""
The tile-order pointing kernels (csrc/cm2_tiles.hip, csrc/cm2_tiles_fixed.hip, csrc/cm2_fx_lists.hip) against the
references of tests/_tiles_ref.py, element by element and -- except for the atomic P^T -- bit for bit.

Conventions of every case: each input and output is the middle of a larger buffer pre-filled with a sentinel
whose bits must be unchanged after the call, an output holds NaN before the call, and every input must come
back bit-identical.  Plans are built through L._sparse_tiles with the switches set before creation.  The
reference gets only what the plan reports: the tile boundaries (pixel_range), the slice length
(fixed_order_info) and the forced part target.  The time -> tile permutation of the ramp v[t] = t must be the
stable order, tile -> time its inverse with exact zeros at the flagged samples.  P of the maps (I = pixel
index), (Q = 1), (U = 1) returns the stored pixel, cos and sin of every sample; P of a random map the restated
expression.  P^T in the default order (mode 1) and in the exact order (mode 2) must equal their restatements
bit for bit, on an output prefilled with NaN and again with 123.0; mode 2 with full angles also equals the
oracle's serial loop, and mode 1 restored afterwards gives its earlier bits.  The atomic P^T (mode 0) adds
the same terms in an order that is not fixed: every element within gamma_n sum|terms| of the serial sum, a
pixel without a hit exactly +0.0.  The cases (tests/_tiles_ref.py: case) lay their samples out by
construction; tests/test_tiles_ref_cpu.py asserts that each has the property its row claims.

Kernels and branches, and the case that reaches them (to be kept in step with the dispatch code by hand):

  k_tile_rank, k_tile_offsets (multisplit)        every case without [sort]
  k_tile_place_staged<POL>   half angles, pol 1   every case [*-1-half | *-2-half | *-3-half] but T10
  k_tile_place<POL, false>   pol > 1, both arrays [*-2-full | *-3-full]; T10 (cos = 0.5 c: the plan refuses
                                                  half angles although they were asked for)
  k_tile_keys, k_tile_bounds, k_tile_fill<POL, HALF>
                             CM2_TILE_BUILD=sort  test_plan_built_by_the_sort: T1-73733 and T3, five forms
  k_unit_circle                                   every pol > 1 case with half angles; T10 (off the circle)
  k_time_to_tiles, k_tiles_to_time (per sample)   T1-8191 (shorter than one window)
  k_perm_keys, k_perm_unpack, k_perm_windows<to time | to tiles>
                                                  T1-8192 (one full window), T1-8193 (a second window of one
                                                  sample, flagged), T1-73733 (10 windows on a grid of 16:
                                                  six workgroups exit; window 5 holds no unflagged sample),
                                                  and every other case (nt >= 8192)
  k_i32_time_to_tiles                             T1-*
  k_P_tiles<POL, HALF>: the five instances        every case x [1-half, 2-half, 2-full, 3-half, 3-full];
                                                  several work items a tile (slice_samples = 1024), an
                                                  empty tile (T1 tile 2, T6 tile 3), a narrow last tile
  k_Pt_tiles<POL, HALF> (atomic): five instances  every case, mode 0; the 4-way unrolled loop and its tail
  k_Pt_tiles_fixed<POL, HALF, VPT>
    VPT = 2, 3, 4                                 T2-64 / -1000 / -1024 (2), T2-1536 (3), T2-2048 and every
                                                  case with S = 2048 (4); T1 (tuned S)
    a last slice of 1 sample, of S samples        T2-* (clamped loads at len - 1)
    a tile without a sample is written as zeros   T1 (tile 2), T6 (tile 3: an empty tile in a parts plan)
    levels 0 .. 14 (runs of 5 .. 60 in pieces)    T3, T5, T10: runs of 1, 2, 3, 4, 5, 8, 20, 59, 60
    runs walked by one thread (61 .. 256)         T3, T5, T10: runs of 61, 255, 256
    chunked runs (> 256), cbase walk              T3, T5, T10: runs of 257 (last chunk of 1), 288 (of 32), 600
                                                  in ONE slice; T8, T9a, T9b in the one-workgroup plan
    more groups than threads (g0 > 0 round)       T4: 819 groups in a slice of 2048
    run pieces kept inside one wave               T5: the run of 60 follows 54 groups of shorter runs
    parts: 1, 2, as many as slices; k_parts_combine
                                                  T6 (S 512, target 1000: 1100 samples whole, 1101 split,
                                                  2 parts of 3 slices, 5 of 10 and of 9), T6s (S 1024,
                                                  target 600: 5 parts of 5 slices); T9a (parts beside a hot tile)
    tile_part0 / tiles_in_range (range form)      test_range_form: T6, T6s, T9a group by group, shuffled,
                                                  with an empty range
  fx_hot_item<POL, HALF> (fused), k_Pt_hot + k_hot_combine (CM2_PT_FUSE=0)
                                                  T8 (two full ranges), T9a (a last range of 1 sample), T9b
                                                  (257 ranges: the second staging round of the range sums)
  k_fx_build (default) and k_fx_keys + k_fx_pack (CM2_FX_BUILD=serial)
                                                  test_list_builders_agree: T3, T4, T5
  graph capture of P and P^T on a prepared plan   test_P_and_Pt_are_captured_into_a_graph: T9a
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ref as R  # noqa: E402
from _guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("CM2_PT_ORDER", "CM2_TILE_BUILD", "CM2_TILE_BALANCE", "CM2_TILE_ANGLES", "CM2_FX_BUILD", "CM2_PT_SLICE",
            "CM2_PT_PARTS", "CM2_PT_FUSE", "CM2_TILE_PIXELS", "CM2_TILE_SLICE")
ONE_WG = {"CM2_TILE_BALANCE": "0", "CM2_PT_PARTS": None}      # uniform tiles, one workgroup per tile
NAN_BITS = np.array([float("nan")]).view(np.int64)[0]


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, L=L, D=device, hip=_hip, torch=torch)


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


_REF, _CASE = {}, {}


def the_case(name, arg):
    if (name, arg) not in _CASE:
        _CASE[(name, arg)] = R.case(name, arg)
    return _CASE[(name, arg)]


def reference(name, arg, pol, angles, tile_p0, S):
    """the case, its reference plan for what the GPU plan reports, inputs and the two fixed orders: computed once
    per storage form, shared by the tests and left unchanged"""
    key = (name, arg, pol, angles, tuple(tile_p0), S)
    if key not in _REF:
        cs = the_case(name, arg)
        pl = R.plan_of(cs, pol, angles, S=S, tile_p0=np.asarray(tile_p0))
        x, v = R.inputs(cs, pol)
        v_tb = pl.to_tiles(v)
        _REF[key] = SimpleNamespace(cs=cs, pl=pl, x=x, v=v, v_tb=v_tb, order={})
    return _REF[key]


def ordered(ref, mode, target):
    if (mode, target) not in ref.order:
        ref.order[(mode, target)] = ref.pl.Pt(ref.v_tb, mode, target)
    return ref.order[(mode, target)]


def make_plan(cm, monkeypatch, cs, pol, angles, extra=None):
    env = dict(cs.env)
    if angles == "full":
        env["CM2_TILE_ANGLES"] = "full"
    env.update(extra or {})
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        if val is not None:
            monkeypatch.setenv(k, val)
    ang = SimpleNamespace(cos=cs.cos, sin=cs.sin) if pol > 1 else None
    P = cm.I.SparseLO(cs.npix, cs.nt, cs.pix.astype(np.int32), pol=pol, angle_processed=ang)
    T = cm.L._sparse_tiles(P, tile_pixels=cs.tp, slice_samples=1024)
    tile_p0 = [T.pixel_range(b, b + 1)[0] for b in range(T.ntiles)] + [T.pixel_range(0, T.ntiles)[1]]
    return P, T, tile_p0, T.fixed_order_info()[0]


def apply_Pt(cm, T, gv, what, prefill=None):
    """cm2_Pt_tiles_apply into a guarded output that holds NaN (or prefill) -> the result"""
    out = Guarded(cm, T.nout)
    if prefill is not None:
        out.v.fill_(prefill)
    call(cm, "cm2_Pt_tiles_apply", T.h, gv.ptr, out.ptr)
    got = out.get()
    out.intact(what)
    gv.intact(what)
    return got


def plan_and_reference(cm, monkeypatch, name, arg, pol, angles, extra=None):
    cs = the_case(name, arg)
    P, T, tile_p0, S = make_plan(cm, monkeypatch, cs, pol, angles, extra)
    T.nout = cs.npix * pol                                    # (kept with the handle for apply_Pt)
    ref = reference(name, arg, pol, angles, tile_p0, S)
    pl = ref.pl
    what = "%s%s pol %d %s angles" % (name, "-%s" % arg if arg else "", pol, angles)
    assert (T.nt, T.nvalid, T.ntiles, T.tile_pixels) == (cs.nt, pl.nvalid, pl.ntiles, cs.tp), what
    assert T.half_angle == pl.half and T.pt_mode == 1, what
    assert S > 0 and (cs.S is None or S == cs.S), (what, S)
    balance_parts = cs.balance_parts and not (extra and extra.get("CM2_TILE_BALANCE") == "0")
    assert np.array_equal(tile_p0, R.expected_tile_p0(cs.pix, cs.npix, cs.tp, balance_parts)), (what, tile_p0)
    return cs, P, T, ref, what


def check_order_and_gather(cm, cs, T, ref, what, i32=False):
    """the two permutations, the stored pixel and angles, P of a random map"""
    pl, pol = ref.pl, ref.pl.pol
    ramp = np.arange(cs.nt, dtype=np.float64)
    gin, tb, back = Guarded(cm, cs.nt, ramp), Guarded(cm, pl.nvalid), Guarded(cm, cs.nt)
    call(cm, "cm2_tod_time_to_tiles", T.h, gin.ptr, tb.ptr)
    R.assert_bit_equal(tb.get(), pl.tb_src.astype(np.float64), what + ": time -> tiles of the ramp")
    call(cm, "cm2_tod_tiles_to_time", T.h, tb.ptr, back.ptr)
    R.assert_bit_equal(back.get(), np.where(pl.ok, ramp, 0.0), what + ": tiles -> time")
    for g in (gin, tb, back):
        g.intact(what + ": permutations")
    R.assert_bit_equal(gin.get(), ramp, what + ": the ramp")
    R.assert_bit_equal(tb.get(), pl.tb_src.astype(np.float64), what + ": the ramp in tile order")
    if i32:
        t = cm.torch
        src = t.arange(cs.nt, dtype=t.int32, device=cm.D.dev())
        dst = t.full((pl.nvalid + 16,), -7, dtype=t.int32, device=cm.D.dev())
        call(cm, "cm2_i32_time_to_tiles", T.h, src.data_ptr(), dst[8:].data_ptr())
        t.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[8:8 + pl.nvalid], pl.tb_src.astype(np.int32)), what + ": int32 time -> tiles"
        assert (got[:8] == -7).all() and (got[8 + pl.nvalid:] == -7).all(), what + ": int32 wrote outside"
    # P: the stored pixel, cos and sin of every sample, then a random map
    maps = np.zeros((pol, cs.npix, pol))
    want = []
    if pol != 2:
        maps[0, :, 0] = np.arange(cs.npix)
        want.append(pl.q.astype(np.float64))
    if pol > 1:
        maps[pol - 2, :, pol - 2] = 1.0
        maps[pol - 1, :, pol - 1] = 1.0
        want += [pl.cc + 0.0, pl.ss + 0.0]
    for m, w, label in zip(maps, want, ["pixel", "cos", "sin"] if pol == 3 else (["pixel"] if pol == 1 else ["cos", "sin"])):
        R.assert_bit_equal(pl.P(m), w, what + ": the restatement of the stored " + label)
    for m, label in list(zip(maps, ["map 0", "map 1", "map 2"])) + [(ref.x, "a random map")]:
        gx, out = Guarded(cm, cs.npix * pol, m), Guarded(cm, pl.nvalid)
        call(cm, "cm2_P_tiles_apply", T.h, gx.ptr, out.ptr)
        got = out.get()
        out.intact(what + ": P")
        gx.intact(what + ": P")
        R.assert_bit_equal(gx.get(), np.asarray(m).reshape(-1), what + ": P, the map")
        R.assert_bit_equal(got, pl.P(m), what + ": P of " + label)


def check_fixed_orders(cm, oracle, cs, T, ref, what, angles):
    """modes 1, 2, 0 and 1 again against the restatements -> (mode 1 bits, mode 2 bits)"""
    pl = ref.pl
    gv = Guarded(cm, pl.nvalid, ref.v_tb)
    want1, want2 = ordered(ref, 1, cs.target), ordered(ref, 2, None)
    got1 = apply_Pt(cm, T, gv, what + ": P^T, mode 1")
    R.assert_bit_equal(got1, want1, what + ": P^T in the default order")
    R.assert_bit_equal(apply_Pt(cm, T, gv, what, prefill=123.0), want1, what + ": P^T over 123.0")
    T.set_pt_order(2)
    got2 = apply_Pt(cm, T, gv, what + ": P^T, mode 2")
    R.assert_bit_equal(got2, want2, what + ": P^T in the exact order")
    R.assert_bit_equal(apply_Pt(cm, T, gv, what, prefill=123.0), want2, what + ": exact P^T over 123.0")
    if angles == "full" or pl.pol == 1:
        R.assert_bit_equal(got2, oracle.sparse_rmult(pl.pol, cs.npix, cs.pix, cs.cos, cs.sin, ref.v),
                           what + ": exact order against the oracle")
    T.set_pt_order(0)
    got0 = apply_Pt(cm, T, gv, what + ": P^T, mode 0")
    worst = R.assert_atomic_ok(got0, pl, ref.v_tb, what + ": atomic P^T", serial=want2)
    R.assert_atomic_ok(apply_Pt(cm, T, gv, what, prefill=123.0), pl, ref.v_tb, what + ": atomic P^T over 123.0",
                       serial=want2)
    T.set_pt_order(1)
    R.assert_bit_equal(apply_Pt(cm, T, gv, what), got1, what + ": mode 1 restored")
    R.assert_bit_equal(gv.get(), ref.v_tb, what + ": the time stream in tile order")
    print("%s: S = %d, %d tiles, %d of %d elements regrouped by the default order; atomic order used %.3g of its bound"
          % (what, pl.S, pl.ntiles, int((R.bits(want1) != R.bits(want2)).sum()), len(want1), worst))
    return got1, got2


CASES = [("T1", n, c) for n in (8191, 8192, 8193, 9 * 8192 + 5) for c in R.RAMP_COMBOS] + \
    [("T2", s, c) for s in (64, 1000, 1024, 1536, 2048) for c in R.RAMP_COMBOS] + \
    [(n, None, c) for n in ("T3", "T4", "T5", "T6", "T6s", "T8", "T9a", "T9b", "T10") for c in R.COMBOS]


def _id(c):
    return "%s%s-%d-%s" % (c[0], "-%s" % c[1] if c[1] else "", c[2][0], c[2][1])


@pytest.mark.parametrize("name,arg,combo", CASES, ids=[_id(c) for c in CASES])
def test_tile_kernels(cm, oracle, monkeypatch, name, arg, combo):
    pol, angles = combo
    cs, P, T, ref, what = plan_and_reference(cm, monkeypatch, name, arg, pol, angles)
    check_order_and_gather(cm, cs, T, ref, what, i32=(name == "T1"))
    if name in ("T6", "T6s", "T9a"):
        info = T.pt_parts()
        assert (info["workgroups"], info["tiles_split"]) == ref.pl.workgroups(cs.target), (what, info)
    if name in ("T8", "T9a", "T9b"):
        assert T.ntiles == 6 and ref.pl.hot().sum() == 1, what
    got1, got2 = check_fixed_orders(cm, oracle, cs, T, ref, what, angles)
    if name in ("T6", "T6s", "T8", "T9a", "T9b"):
        # the one-workgroup-per-tile plan (uniform tiles): its exact order gives the same bits
        cs0, P0, T0, ref0, what0 = plan_and_reference(cm, monkeypatch, name, arg, pol, angles, extra=ONE_WG)
        assert T0.pt_parts()["tiles_split"] == 0 and T0.ntiles == -(-cs.npix // cs.tp), what0
        T0.set_pt_order(2)
        gv0 = Guarded(cm, ref0.pl.nvalid, ref0.v_tb)
        R.assert_bit_equal(apply_Pt(cm, T0, gv0, what0), got2, what0 + ": exact order of the one-workgroup plan")
    if name in ("T8", "T9a", "T9b"):
        # the ranges of the hot tile in kernels of their own: the same bits as in the fused launch
        extra = {"CM2_PT_FUSE": "0"}
        cs1, P1, T1, ref1, what1 = plan_and_reference(cm, monkeypatch, name, arg, pol, angles, extra=extra)
        gv1 = Guarded(cm, ref1.pl.nvalid, ref1.v_tb)
        R.assert_bit_equal(apply_Pt(cm, T1, gv1, what1), got1, what1 + ": CM2_PT_FUSE=0")
        R.assert_bit_equal(apply_Pt(cm, T1, gv1, what1, prefill=123.0), got1, what1 + ": CM2_PT_FUSE=0 over 123.0")


SORT_CASES = [(n, a, c) for n, a in (("T1", 9 * 8192 + 5), ("T3", None)) for c in R.COMBOS]


@pytest.mark.parametrize("name,arg,combo", SORT_CASES, ids=[_id(c) for c in SORT_CASES])
def test_plan_built_by_the_sort(cm, oracle, monkeypatch, name, arg, combo):
    """CM2_TILE_BUILD=sort: radix sort and k_tile_fill instead of the multisplit -- the same plan"""
    pol, angles = combo
    cs, P, T, ref, what = plan_and_reference(cm, monkeypatch, name, arg, pol, angles, extra={"CM2_TILE_BUILD": "sort"})
    check_order_and_gather(cm, cs, T, ref, what + " [sort]", i32=(name == "T1"))
    check_fixed_orders(cm, oracle, cs, T, ref, what + " [sort]", angles)


BUILDER_CASES = [(n, c) for n in ("T3", "T4", "T5") for c in R.COMBOS]


@pytest.mark.parametrize("name,combo", BUILDER_CASES, ids=["%s-%d-%s" % (n, c[0], c[1]) for n, c in BUILDER_CASES])
def test_list_builders_agree(cm, oracle, monkeypatch, name, combo):
    """k_fx_build and the serial pair k_fx_keys / k_fx_pack pack other lists for the same sums: both give the
    restatement's bits in the default and in the exact order"""
    pol, angles = combo
    res = []
    for build in (None, "serial"):
        cs, P, T, ref, what = plan_and_reference(cm, monkeypatch, name, None, pol, angles, extra={"CM2_FX_BUILD": build})
        gv = Guarded(cm, ref.pl.nvalid, ref.v_tb)
        got1 = apply_Pt(cm, T, gv, what)
        R.assert_bit_equal(got1, ordered(ref, 1, None), "%s [%s lists]: default order" % (what, build))
        T.set_pt_order(2)
        got2 = apply_Pt(cm, T, gv, what)
        R.assert_bit_equal(got2, ordered(ref, 2, None), "%s [%s lists]: exact order" % (what, build))
        res.append((got1, got2))
    R.assert_bit_equal(res[0][0], res[1][0], what + ": the two builders, default order")
    R.assert_bit_equal(res[0][1], res[1][1], what + ": the two builders, exact order")


RANGE_CASES = [(n, c) for n in ("T6", "T6s", "T9a") for c in R.COMBOS]


@pytest.mark.parametrize("name,combo", RANGE_CASES, ids=["%s-%d-%s" % (n, c[0], c[1]) for n, c in RANGE_CASES])
def test_range_form(cm, monkeypatch, name, combo):
    """T7: P^T applied tile group by tile group (cm2_tiles_group_tiles) in shuffled order: every group writes its
    pixels with the bits of the whole application and leaves the NaN bits of every other pixel alone; an empty
    range writes nothing"""
    pol, angles = combo
    cs, P, T, ref, what = plan_and_reference(cm, monkeypatch, name, None, pol, angles)
    want = ordered(ref, 1, cs.target)
    gv = Guarded(cm, ref.pl.nvalid, ref.v_tb)
    out = Guarded(cm, cs.npix * pol)
    cuts = (ctypes.c_int64 * 9)()
    cm.hip.call("cm2_tiles_group_tiles", T.h, 8, cuts)
    cuts = [int(c) for c in cuts]
    assert cuts[0] == 0 and cuts[8] == T.ntiles and any(cuts[g] == cuts[g + 1] for g in range(8)), cuts
    done = np.zeros(cs.npix * pol, bool)
    for g in (5, 0, 2, 7, 1, 6, 3, 4):
        lo, hi = cuts[g], cuts[g + 1]
        call(cm, "cm2_Pt_tiles_apply_range", T.h, gv.ptr, out.ptr, lo, hi)
        p0, p1 = T.pixel_range(lo, hi)
        assert (lo == hi) == (p0 == p1)
        done[p0 * pol:p1 * pol] = True
        got = out.get()
        out.intact(what + ": range form")
        R.assert_bit_equal(got[done], want[done], "%s: tiles [%d, %d)" % (what, lo, hi))
        assert (R.bits(got[~done]) == NAN_BITS).all(), "%s: tiles [%d, %d) wrote outside their pixels" % (what, lo, hi)
    assert done.all()
    call(cm, "cm2_Pt_tiles_apply_range", T.h, gv.ptr, out.ptr, 2, 2)
    R.assert_bit_equal(out.get(), want, what + ": after an empty range")
    gv.intact(what)
    R.assert_bit_equal(gv.get(), ref.v_tb, what + ": the time stream in tile order")


def test_P_and_Pt_are_captured_into_a_graph(cm, monkeypatch):
    """On a prepared plan one P and one P^T allocate nothing and never synchronise: they are recorded into a graph,
    and the graph replayed twice gives the restatement's bits (T9a: split tiles and a hot tile in one launch)"""
    t = cm.torch
    cs, P, T, ref, what = plan_and_reference(cm, monkeypatch, "T9a", None, 3, "half")
    pl = ref.pl
    gx, d_tb = Guarded(cm, cs.npix * 3, ref.x), Guarded(cm, pl.nvalid)
    gv, out = Guarded(cm, pl.nvalid, ref.v_tb), Guarded(cm, cs.npix * 3)
    call(cm, "cm2_P_tiles_apply", T.h, gx.ptr, d_tb.ptr)              # (first launches outside the capture)
    call(cm, "cm2_Pt_tiles_apply", T.h, gv.ptr, out.ptr)
    t.cuda.synchronize()
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            call(cm, "cm2_P_tiles_apply", T.h, gx.ptr, d_tb.ptr)
            call(cm, "cm2_Pt_tiles_apply", T.h, gv.ptr, out.ptr)
        for fill in (float("nan"), 123.0):
            d_tb.v.fill_(fill)
            out.v.fill_(fill)
            g.replay()
            side.synchronize()
            R.assert_bit_equal(d_tb.get(), pl.P(ref.x), what + ": P replayed")
            R.assert_bit_equal(out.get(), ordered(ref, 1, cs.target), what + ": P^T replayed")
    t.cuda.current_stream().wait_stream(side)
    for gd in (gx, d_tb, gv, out):
        gd.intact(what + ": graph")
