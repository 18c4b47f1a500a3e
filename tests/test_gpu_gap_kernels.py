"""
Every kernel and entry point of csrc/cm2_gaps.hip against the restatements of tests/_gaps_ref.py, element by
element and bit for bit.

Conventions of every case: each double buffer the library reads or writes -- stream, compact or tile order -- is a
tests/_guarded.Guarded: the middle of a larger buffer pre-filled with a sentinel whose bits must be unchanged after
the call; an output holds NaN before the call, an input must be unchanged after it.  Every comparison is
assert_bit_equal; there is no tolerance anywhere (the fused N^-1 was found reproducible from call to call, so the
bound the fused comparison could have fallen back to is not used).  The data has +0.0, -0.0 and a denormal among
the valid samples and NaN, +Inf and 1e300 at the flagged ones of d: none of these may reach an output.

Layouts (tests/_gaps_ref.py; tests/test_gaps_ref_cpu.py asserts their features): E = 16 461 samples in blocks of
1, 8191, 1, 4000, 4268 (a block boundary on the window end at 8192; 362 runs), in four flag encodings that must give
the same bits (int32 from {-1, -7, INT32_MIN} / {0, 5, INT32_MAX}; bytes from {1, 2, 0x80, 0xFF} through
cm2_gaps_create; a bool array; a uint8 tensor); Ew = E with nothing flagged in its last window (each of E's three
windows necessarily holds a flagged sample: 0, 8192 and the stream's end); M = 5460 samples in 257 blocks, Mall the
same wholly flagged; S1 / S3 = 1 100 000 samples with 550 000 flagged in 530 001 / 530 002 runs, in 1 / 3 blocks;
W0 / W1 = 65 537 samples, nine permutation windows holding 0, 1, 255, 256, 257, 8192, 8191, 10 and 0 / 1 flagged
samples; P8191, P8192 = below one window, exactly one.

Kernels and entry points, and the case that reaches them (second time round the grid-stride loop: S1 / S3, whose
nt, ng and nruns all exceed the 524 288 threads of a full grid, nruns the 131 072 of k_gap_edges):

  cm2_gaps_create: hipCUB sum / select over FlagAt<0 | 1>  every handle; <0> int32, <1> bytes / bool / uint8
    RunStartAt, block_of over 257 blocks                   test_many_blocks (M, Mall: nruns == nblocks)
    k_gap_runs                                             test_index_and_jacobi, test_many_blocks; loop: S1 / S3
    k_gap_jacobi, run_of over 362 runs                     test_index_and_jacobi (through cm2_gaps_precond_apply on
                                                           ones), distinct a_0 per block: M; loop: S1 / S3
  cm2_gaps_info, cm2_gaps_index                            test_index_and_jacobi, with and without a_0
  k_gap_gather, k_gap_scatter                              test_gather_and_scatter; loop: S1 / S3
  k_gap_masked_diff<0 | 1> (n, n == NULL)                  test_masked_diff_and_finish; loop: S1 <0>, S3 <1>
  k_gap_copy_valid<0 | 1>, k_gap_finish                    test_masked_diff_and_finish (n, n == NULL, in place,
    (cm2_gaps_finish)                                      ng == 0); loop: S1 / S3
  k_gap_edges<0 | 1>, k_gap_interp                         test_linear_fill: nedge 1, 5, 32, nt, nt + 5, in and out
    (cm2_gaps_fill_linear)                                 of place; test_nedge_beyond_the_stream (2^63 - 1);
                                                           loop: S1 <0>, S3 <1>
  cm2_gaps_normal_apply, cm2_gaps_rhs                      test_through_the_direct_sum (lambda 8),
                                                           test_through_the_fused_kernel (lambda 64)
  k_gap_compare<0 | 1> (cm2_gaps_prepare_tiles)            test_merging_permutations, test_prepare_names_the_sample;
                                                           loop: S1 (a mismatch at sample 1 000 000 is found)
  k_gap_window_table (cm2_gaps_window_table)               test_merging_permutations: E, Ew, W0, W1, P8192; P8191:
                                                           no table.  Its loop needs more than 524 288 windows
                                                           (4.3e9 samples): no small shape can reach it
  k_gap_perm_windows<true | false>                         test_merging_permutations: E / Ew (3 windows: 8
    (cm2_gaps_tiles_to_time, cm2_gaps_time_to_tiles)       workgroups, 5 exit), W0 / W1 (9 windows: 16 workgroups,
                                                           two windows per XCD), P8192 (one full window), S1 (135
                                                           windows); one workgroup per window: no loop over windows
    the per-sample route (nwin == 0)                       test_merging_permutations[P8191]
  cm2_PtNP_gaps_apply                                      test_ptnp_gaps_apply_is_its_five_calls (pol 1, 3)
  argument checks of every entry point                     test_argument_errors

Left out, by name: the grid-stride loop of k_gap_window_table (above); hipCUB's behaviour at nt >= 2^31; the
solver-level properties (fill, the gap-aware solve), which tests/test_gpu_gap_fill.py and
tests/test_gpu_gap_aware.py cover.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gaps_ref as G  # noqa: E402
import _noise_ref as N  # noqa: E402
from _guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

ENCODINGS = ("i32", "bytes", "bool", "u8tensor")
_I64P, _DBLP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd.utilities import gap_fill
    return SimpleNamespace(I=I, L=L, D=device, hip=_hip, gf=gap_fill, torch=torch)


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def refused(cm, name, *args):
    """the call returns CM2_ERR_ARGUMENT with a message that names the entry point -> the message"""
    lib = cm.hip.load()
    rc = getattr(lib, name)(*(list(args) + [cm.D.stream()]))
    msg = lib.cm2_last_error()
    cm.torch.cuda.synchronize()
    assert rc == cm.hip.ERR_ARGUMENT, (name, rc, msg)
    assert name.encode() in msg, (name, msg)
    return msg


def create(cm, flags_dev, kind, nt, sizes, a0, nblocks=None):
    """cm2_gaps_create through the C entry point -> (rc, handle value or None)"""
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    pa = None if a0 is None else np.ascontiguousarray(a0, dtype=np.float64).ctypes.data_as(_DBLP)
    h = ctypes.c_void_p(0xDEAD)
    rc = cm.hip.load().cm2_gaps_create(ctypes.byref(h), cm.D.ptr(flags_dev), kind, nt, sz.ctypes.data_as(_I64P),
                                       len(sizes) if nblocks is None else nblocks, pa, cm.D.stream())
    return rc, h


_handles = {}


def handle(cm, cs, enc, a0=True, fresh=False):
    """The handle of a case's flags in one encoding, shared between the tests; a0: True = the case's a_0, None =
    made without"""
    key = (cs.name, enc, a0 is True)
    if key in _handles and not fresh:
        return _handles[key]
    a = cs.a0 if a0 is True else None
    if enc == "bytes":
        flags = cm.D.to_dev(cs.u8)
        rc, h = create(cm, flags, 1, cs.nt, cs.sizes, a)
        assert rc == 0, cm.hip.load().cm2_last_error()
        H = cm.hip.Handle("cm2_gaps_destroy", h, keep=flags)
    else:
        flags = {"i32": cs.i32, "bool": cs.mask, "u8tensor": cm.torch.from_numpy(cs.u8.copy())}[enc]
        H = cm.gf._Gaps(flags, cs.sizes, a)
    if not fresh:
        _handles[key] = H
    return H


# ------------------------------------------------------------ the checks of one handle ----
def check_index(cm, H, cs, with_a0, what):
    ix = G.index(cs.mask, cs.sizes)
    info = (ctypes.c_int64 * 5)()
    cm.hip.call("cm2_gaps_info", H.h, info)
    assert list(info) == [cs.nt, ix.pos.size, len(ix.runs), ix.longest, 16 * cs.nt if with_a0 else 0], (what, list(info))
    pos = np.full(ix.pos.size, 0xFFFFFFFF, dtype=np.uint32)
    runs = np.full((len(ix.runs), 3), -1, dtype=np.int64)
    call(cm, "cm2_gaps_index", H.h, pos.ctypes.data, runs.ctypes.data)
    cm.torch.cuda.synchronize()
    np.testing.assert_array_equal(pos, ix.pos, what + ": positions")
    np.testing.assert_array_equal(runs, ix.runs, what + ": runs")


def check_jacobi(cm, H, cs, what):
    ng = int(cs.mask.sum())
    ones, z = Guarded(cm, ng, np.ones(ng)), Guarded(cm, ng)
    call(cm, "cm2_gaps_precond_apply", H.h, ones.ptr, z.ptr)
    _same(z, G.jacobi(np.flatnonzero(cs.mask), cs.sizes, cs.a0), what + ": Jacobi vector")
    _unchanged(ones, np.ones(ng), what + ": ones")


def _same(g, want, what):
    """a guarded output: bit-equal to `want`, nothing written outside"""
    got = g.get()
    g.intact(what)
    G.assert_bit_equal(got, want, what)
    return got


def _unchanged(g, data, what):
    g.intact(what)
    G.assert_bit_equal(g.get(), data, what + ": the input")


def _all_nan(g, what):
    g.intact(what)
    assert np.isnan(g.get()).all(), what + ": the output was written"


def check_gather_scatter(cm, H, cs, what):
    pos, ng = np.flatnonzero(cs.mask), int(cs.mask.sum())
    s, c = Guarded(cm, cs.nt, cs.n), Guarded(cm, ng)
    call(cm, "cm2_gaps_gather", H.h, s.ptr, c.ptr)
    _same(c, cs.n[pos], what + ": gather")
    _unchanged(s, cs.n, what + ": gather's stream")
    y = Guarded(cm, ng, cs.y)
    call(cm, "cm2_gaps_scatter", H.h, y.ptr, s.ptr)
    want = cs.n.copy()
    want[pos] = cs.y                       # the ng positions only: every other sample keeps its bits
    _same(s, want, what + ": scatter")
    _unchanged(y, cs.y, what + ": scatter's compact vector")


def check_masked_diff(cm, H, cs, what):
    d, n = Guarded(cm, cs.nt, cs.d), Guarded(cm, cs.nt, cs.n)
    for gn, hn, form in ((n, cs.n, "n"), (None, None, "n == NULL")):
        u = Guarded(cm, cs.nt)
        call(cm, "cm2_gaps_masked_diff", H.h, gn.ptr if gn else None, d.ptr, u.ptr)
        got = _same(u, G.masked_diff(cs.mask, hn, cs.d), "%s: masked_diff, %s" % (what, form))
        assert np.isfinite(got).all() and np.abs(got).max() < 1e3
    _unchanged(d, cs.d, what + ": masked_diff's d")
    _unchanged(n, cs.n, what + ": masked_diff's n")


def check_finish(cm, H, cs, what):
    ng = int(cs.mask.sum())
    d, n, y = Guarded(cm, cs.nt, cs.d), Guarded(cm, cs.nt, cs.n), Guarded(cm, ng, cs.y)
    for gn, hn, form in ((n, cs.n, "n"), (None, None, "n == NULL")):
        out = Guarded(cm, cs.nt)
        call(cm, "cm2_gaps_finish", H.h, d.ptr, gn.ptr if gn else None, y.ptr, out.ptr)
        got = _same(out, G.finish(cs.mask, cs.d, hn, cs.y), "%s: finish, %s" % (what, form))
        assert np.isfinite(got).all() and np.abs(got).max() < 1e3
    for g, data in ((d, cs.d), (n, cs.n), (y, cs.y)):
        _unchanged(g, data, what + ": finish")
    call(cm, "cm2_gaps_finish", H.h, d.ptr, n.ptr, y.ptr, d.ptr)
    _same(d, G.finish(cs.mask, cs.d, cs.n, cs.y), what + ": finish in place")


def check_linear(cm, H, cs, nedge, what, want=None):
    want = G.linear_of(cs.name, min(nedge, cs.nt)) if want is None else want
    d, out = Guarded(cm, cs.nt, cs.d), Guarded(cm, cs.nt)
    call(cm, "cm2_gaps_fill_linear", H.h, d.ptr, out.ptr, nedge)
    got = _same(out, want, "%s: linear fill, nedge %d" % (what, nedge))
    assert np.isfinite(got).all() and np.abs(got).max() < 1e3
    _unchanged(d, cs.d, "%s: linear fill, nedge %d" % (what, nedge))
    call(cm, "cm2_gaps_fill_linear", H.h, d.ptr, d.ptr, nedge)
    _same(d, want, "%s: linear fill in place, nedge %d" % (what, nedge))


# ======================================================================= layout E ===
@pytest.mark.parametrize("enc", ENCODINGS)
def test_index_and_jacobi(cm, enc):
    cs = G.case("E")
    check_index(cm, handle(cm, cs, enc), cs, True, "E %s" % enc)
    check_index(cm, handle(cm, cs, enc, a0=None), cs, False, "E %s, no a_0" % enc)
    check_jacobi(cm, handle(cm, cs, enc), cs, "E %s" % enc)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_gather_and_scatter(cm, enc):
    cs = G.case("E")
    check_gather_scatter(cm, handle(cm, cs, enc), cs, "E %s" % enc)
    check_gather_scatter(cm, handle(cm, cs, enc, a0=None), cs, "E %s, no a_0" % enc)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_masked_diff_and_finish(cm, enc):
    cs = G.case("E")
    H = handle(cm, cs, enc, a0=None)
    check_masked_diff(cm, H, cs, "E %s" % enc)
    check_finish(cm, H, cs, "E %s" % enc)
    # ng == 0: a copy of d with all its bits, the NaN and the Inf included; y is not looked at
    flags = {"i32": np.where(cs.mask, 5, 0).astype(np.int32), "bool": np.zeros(cs.nt, dtype=bool)}.get(
        enc, cm.torch.zeros(cs.nt, dtype=cm.torch.uint8))
    H0 = cm.gf._Gaps(flags, cs.sizes)
    assert H0.info()["ng"] == 0 and H0.info()["runs"] == 0
    d, n, out = Guarded(cm, cs.nt, cs.d), Guarded(cm, cs.nt, cs.n), Guarded(cm, cs.nt)
    call(cm, "cm2_gaps_finish", H0.h, d.ptr, n.ptr, None, out.ptr)
    _same(out, cs.d, "E %s: finish, ng == 0" % enc)
    _unchanged(d, cs.d, "E %s: finish, ng == 0" % enc)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_linear_fill(cm, enc):
    cs = G.case("E")
    for nedge in G.E_NEDGES:
        check_linear(cm, handle(cm, cs, enc, a0=None), cs, nedge, "E %s" % enc)
    # the Python entry point: the same bits from every kind of flags it accepts
    flags = {"i32": cs.i32, "bytes": cs.i32.astype(np.int64), "bool": cs.mask,
             "u8tensor": cm.torch.from_numpy(cs.u8.copy())}[enc]
    G.assert_bit_equal(cm.gf.fill_gaps_linear(cs.d, flags, list(cs.sizes), nedge=5), G.linear_of("E", 5),
                       "fill_gaps_linear, %s" % enc)


def test_nedge_beyond_the_stream(cm):
    """nedge is clamped to nt: 2^63 - 1 (where e + nedge used to wrap, the right-hand window came out empty and
    every run took its left level) and, through Python, an integer beyond int64 (which ctypes used to wrap to a
    small one) give the bits of nedge = nt"""
    cs = G.case("E")
    want = G.linear_of("E", cs.nt)
    for enc in ("i32", "bytes"):
        check_linear(cm, handle(cm, cs, enc, a0=None), cs, 2 ** 63 - 1, "E %s" % enc, want)
    for nedge in (2 ** 63 - 1, 2 ** 64 + 1, 2 ** 70):
        for flags in (cs.i32, cs.mask):
            G.assert_bit_equal(cm.gf.fill_gaps_linear(cs.d, flags, list(cs.sizes), nedge=nedge), want,
                               "fill_gaps_linear, nedge %d" % nedge)


# ======================================================================= layout M ===
@pytest.mark.parametrize("enc", ["i32", "bytes"])
def test_many_blocks(cm, enc):
    cs = G.case("M")
    H = handle(cm, cs, enc)
    check_index(cm, H, cs, True, "M %s" % enc)
    check_jacobi(cm, H, cs, "M %s" % enc)
    check_gather_scatter(cm, H, cs, "M %s" % enc)
    check_masked_diff(cm, H, cs, "M %s" % enc)
    check_finish(cm, H, cs, "M %s" % enc)
    check_linear(cm, H, cs, 32, "M %s" % enc)
    ca = G.case("Mall")                    # every sample flagged: one run per block, the linear fill all zeros
    Ha = handle(cm, ca, enc)
    check_index(cm, Ha, ca, True, "Mall %s" % enc)
    assert len(G.index(ca.mask, ca.sizes).runs) == len(ca.sizes) == 257        # nruns == nblocks, checked above
    check_jacobi(cm, Ha, ca, "Mall %s" % enc)
    check_linear(cm, Ha, ca, 32, "Mall %s" % enc, np.zeros(ca.nt))
    check_masked_diff(cm, Ha, ca, "Mall %s" % enc)


# ======================================================================= layout S ===
@pytest.mark.parametrize("name,enc", [("S1", "i32"), ("S3", "bytes")])
def test_grid_stride(cm, name, enc):
    """nt, ng and nruns beyond the threads of a full grid: every kernel goes round its loop"""
    cs = G.case(name)
    H = handle(cm, cs, enc, fresh=True)
    what = "%s %s" % (name, enc)
    check_index(cm, H, cs, True, what)
    check_jacobi(cm, H, cs, what)
    check_gather_scatter(cm, H, cs, what)
    check_masked_diff(cm, H, cs, what)
    check_finish(cm, H, cs, what)
    check_linear(cm, H, cs, 2, what)


# ================================================================== through N^-1 ===
def _noise_case(cm, lam, method):
    cs = G.case("E")
    bands = N.make_bands(lam, len(cs.sizes))
    op = cm.I.BlockLO(list(cs.sizes), [b for b in bands], offdiag=True, method=method)
    assert op.noise_info()["method"] == method
    return cs, bands, op, np.flatnonzero(cs.mask)


def _normal_apply(cm, H, op, y, what):
    gy, out = Guarded(cm, len(y), y), Guarded(cm, len(y))
    call(cm, "cm2_gaps_normal_apply", H.h, op._noise.h, gy.ptr, out.ptr)
    got = out.get()
    out.intact(what)
    _unchanged(gy, y, what)
    assert np.isfinite(got).all(), what
    return got


def _rhs(cm, H, op, cs, n, what):
    d, gn = Guarded(cm, cs.nt, cs.d), (Guarded(cm, cs.nt, n) if n is not None else None)
    u, b = Guarded(cm, cs.nt), Guarded(cm, int(cs.mask.sum()))
    call(cm, "cm2_gaps_rhs", H.h, op._noise.h, gn.ptr if gn else None, d.ptr, u.ptr, b.ptr)
    _same(u, G.masked_diff(cs.mask, n, cs.d), what + ": u")
    _unchanged(d, cs.d, what)
    if gn:
        _unchanged(gn, n, what)
    got = b.get()
    b.intact(what)
    assert np.isfinite(got).all(), what
    return got


def test_through_the_direct_sum(cm):
    """lambda = 8, the direct sum, which equals its restatement bit for bit (tests/test_gpu_noise_kernels.py)"""
    cs, bands, op, pos = _noise_case(cm, 8, N.DIRECT)
    a0 = bands[:, 0]
    H = cm.gf._Gaps(cs.i32, cs.sizes, a0)
    y1 = cs.y
    y2 = np.random.default_rng(31).standard_normal(pos.size)

    def ref(y):
        s = np.zeros(cs.nt)
        s[pos] = y
        return N.direct_f64(cs.sizes, bands, s)[pos]

    G.assert_bit_equal(_normal_apply(cm, H, op, y1, "Q_GG y1"), ref(y1), "Q_GG y1 against gather(direct(scatter))")
    # y2 after y1 on one handle: the scatter buffer is still zero on the valid samples
    got2 = _normal_apply(cm, H, op, y2, "Q_GG y2")
    G.assert_bit_equal(got2, ref(y2), "Q_GG y2 after y1")
    fresh = cm.gf._Gaps(cs.mask, cs.sizes, a0)
    G.assert_bit_equal(_normal_apply(cm, fresh, op, y2, "Q_GG y2, fresh handle"), got2, "Q_GG y2: fresh handle")
    for n, form in ((cs.n, "n"), (None, "n == NULL")):
        want = N.direct_f64(cs.sizes, bands, G.masked_diff(cs.mask, n, cs.d))[pos]
        G.assert_bit_equal(_rhs(cm, H, op, cs, n, "rhs, " + form), want, "rhs against gather(direct(masked_diff)), " + form)


def test_through_the_fused_kernel(cm):
    """lambda = 64, the fused overlap-save kernel: normal_apply and rhs equal the three calls made by hand on the
    test's own buffers, bit for bit"""
    cs, bands, op, pos = _noise_case(cm, 64, N.FUSED)
    H = cm.gf._Gaps(cs.i32, cs.sizes, bands[:, 0])
    ng = pos.size

    def by_hand(stream_in):
        s, w, c = Guarded(cm, cs.nt, stream_in), Guarded(cm, cs.nt), Guarded(cm, ng)
        call(cm, "cm2_noise_apply", op._noise.h, s.ptr, w.ptr)
        call(cm, "cm2_gaps_gather", H.h, w.ptr, c.ptr)
        for g in (s, w, c):
            g.intact("by hand")
        return c.get()

    def scattered(y):
        s, gy = Guarded(cm, cs.nt, np.zeros(cs.nt)), Guarded(cm, ng, y)
        call(cm, "cm2_gaps_scatter", H.h, gy.ptr, s.ptr)
        s.intact("scatter")
        return s.get()

    y2 = np.random.default_rng(32).standard_normal(ng)
    for y, form in ((cs.y, "y1"), (y2, "y2 after y1")):
        want = by_hand(scattered(y))
        G.assert_bit_equal(by_hand(scattered(y)), want, "the fused N^-1 twice, " + form)
        G.assert_bit_equal(_normal_apply(cm, H, op, y, "Q_GG " + form), want, "Q_GG %s against the calls by hand" % form)
    fresh = cm.gf._Gaps(cs.mask, cs.sizes, bands[:, 0])
    G.assert_bit_equal(_normal_apply(cm, fresh, op, y2, "Q_GG y2, fresh handle"), want, "Q_GG y2: fresh handle")
    G.assert_bit_equal(_rhs(cm, H, op, cs, cs.n, "rhs"), by_hand(G.masked_diff(cs.mask, cs.n, cs.d)),
                       "rhs against the calls by hand")


# ========================================================== merging permutations ===
NTILES = 16
_plans = {}


def plan(cm, name, pol=1):
    """SparseLO and tile plan (64-pixel tiles, slices of 4096) of a layout, pixels -1 exactly at the flags, and
    src[k] = the time sample held at tile-order position k: the ramp v[t] = t sent through cm2_tod_time_to_tiles,
    a permutation pinned by tests/test_gpu_tile_kernels.py"""
    if (name, pol) in _plans:
        return _plans[(name, pol)]
    cs = G.case(name)
    npix = 64 * NTILES
    pix = N.make_pointing("random", cs.nt, npix, ~cs.mask).astype(np.int32)
    assert np.array_equal(pix == -1, cs.mask) and np.array_equal(pix < 0, cs.mask)
    angles = None
    if pol > 1:
        phi = np.random.default_rng(41).uniform(0.0, np.pi, cs.nt)
        angles = SimpleNamespace(cos=np.cos(2.0 * phi), sin=np.sin(2.0 * phi))
    P = cm.I.SparseLO(npix, cs.nt, pix, pol=pol, angle_processed=angles)
    T = cm.L._sparse_tiles(P, tile_pixels=64, slice_samples=4096)
    ng = int(cs.mask.sum())
    assert (T.ntiles, T.nvalid) == (NTILES, cs.nt - ng), (T.ntiles, T.nvalid)
    ramp, tb = Guarded(cm, cs.nt, np.arange(cs.nt, dtype=np.float64)), Guarded(cm, T.nvalid)
    call(cm, "cm2_tod_time_to_tiles", T.h, ramp.ptr, tb.ptr)
    src = tb.get()
    tb.intact(name + ": the ramp")
    np.testing.assert_array_equal(np.sort(src), np.flatnonzero(~cs.mask))
    _plans[(name, pol)] = SimpleNamespace(cs=cs, pix=pix, P=P, T=T, src=src.astype(np.int64), ng=ng,
                                          pos=np.flatnonzero(cs.mask))
    return _plans[(name, pol)]


def window_table(cm, H):
    nwin = ctypes.c_int64(-1)
    call(cm, "cm2_gaps_window_table", H.h, ctypes.byref(nwin), None)
    if not nwin.value:
        return None
    table = np.full(nwin.value + 1, 0xFFFFFFFF, dtype=np.uint32)
    call(cm, "cm2_gaps_window_table", H.h, ctypes.byref(nwin), table.ctypes.data)
    cm.torch.cuda.synchronize()
    return table


@pytest.mark.parametrize("name", ["E", "Ew", "W0", "W1", "P8191", "P8192", "S1"])
def test_merging_permutations(cm, name):
    p = plan(cm, name)
    cs, T = p.cs, p.T
    rng = np.random.default_rng(51)
    for kind, flags in ((0, p.pix), (1, cs.u8)):
        what = "%s, flag kind %d" % (name, kind)
        H = cm.gf._Gaps(flags if kind == 0 else cm.torch.from_numpy(flags.copy()), cs.sizes)
        call(cm, "cm2_gaps_prepare_tiles", H.h, T.h)
        table, want = window_table(cm, H), G.window_table(p.pos, cs.nt)
        if want is None:
            assert table is None, what
        else:
            np.testing.assert_array_equal(table, want, what + ": window table")
        h_tb, h_comp, h_time = rng.standard_normal(T.nvalid), rng.standard_normal(p.ng), rng.standard_normal(cs.nt)
        tb, comp, time = Guarded(cm, T.nvalid, h_tb), Guarded(cm, p.ng, h_comp), Guarded(cm, cs.nt)
        call(cm, "cm2_gaps_tiles_to_time", H.h, T.h, tb.ptr, comp.ptr, time.ptr)
        got = _same(time, G.to_time(p.src, h_tb, h_comp, p.pos, cs.nt), what + ": tiles -> time")
        assert not np.isnan(got).any(), what + ": a NaN is left"
        _unchanged(tb, h_tb, what + ": tiles -> time")
        _unchanged(comp, h_comp, what + ": tiles -> time")
        time, tb, comp = Guarded(cm, cs.nt, h_time), Guarded(cm, T.nvalid), Guarded(cm, p.ng)
        call(cm, "cm2_gaps_time_to_tiles", H.h, T.h, time.ptr, tb.ptr, comp.ptr)
        want_tb, want_comp = G.to_tiles(p.src, h_time, p.pos)
        _same(tb, want_tb, what + ": time -> tiles")
        _same(comp, want_comp, what + ": time -> compact")
        _unchanged(time, h_time, what + ": time -> tiles")


@pytest.mark.parametrize("pol", [1, 3])
def test_ptnp_gaps_apply_is_its_five_calls(cm, pol):
    p = plan(cm, "E", pol)
    cs, T = p.cs, p.T
    bands = N.make_bands(8, len(cs.sizes))
    op = cm.I.BlockLO(list(cs.sizes), [b for b in bands], offdiag=True)
    H = cm.gf._Gaps(p.pix, cs.sizes, bands[:, 0])
    call(cm, "cm2_gaps_prepare_tiles", H.h, T.h)
    nmap = pol * 64 * NTILES
    hz = np.random.default_rng(61).standard_normal(nmap + p.ng)
    z = Guarded(cm, nmap + p.ng, hz)

    def buffers():
        return Guarded(cm, nmap + p.ng), Guarded(cm, T.nvalid), Guarded(cm, cs.nt), Guarded(cm, cs.nt)

    out, tb, t1, t2 = buffers()
    call(cm, "cm2_PtNP_gaps_apply", T.h, op._noise.h, H.h, z.ptr, out.ptr, tb.ptr, t1.ptr, t2.ptr)
    out2, tb2, t1b, t2b = buffers()
    call(cm, "cm2_P_tiles_apply", T.h, z.ptr, tb2.ptr)
    call(cm, "cm2_gaps_tiles_to_time", H.h, T.h, tb2.ptr, z.ptr + 8 * nmap, t1b.ptr)
    call(cm, "cm2_noise_apply", op._noise.h, t1b.ptr, t2b.ptr)
    call(cm, "cm2_gaps_time_to_tiles", H.h, T.h, t2b.ptr, tb2.ptr, out2.ptr + 8 * nmap)
    call(cm, "cm2_Pt_tiles_apply", T.h, tb2.ptr, out2.ptr)
    for a, b, what in ((out, out2, "A_e z"), (tb, tb2, "tile-order scratch"), (t1, t1b, "time 1"), (t2, t2b, "time 2")):
        got = _same(a, b.get(), "pol %d, %s" % (pol, what))
        b.intact(what)
        assert np.isfinite(got).all(), what
    _unchanged(z, hz, "pol %d: z" % pol)


def test_prepare_names_the_sample(cm):
    """flags that differ from the plan's at samples 5 and 9000, as many flagged: the message names sample 5"""
    p = plan(cm, "E")
    other = p.cs.mask.copy()
    assert other[5] and not other[9000]
    other[5], other[9000] = False, True
    for flags in (np.where(other, -1, 0).astype(np.int32), other):
        H = cm.gf._Gaps(flags, p.cs.sizes)
        assert H.info()["ng"] == p.ng
        msg = refused(cm, "cm2_gaps_prepare_tiles", H.h, p.T.h)
        assert b"sample 5 " in msg, msg


def test_prepare_compares_beyond_one_grid(cm):
    """S1: the comparison goes round its loop; flags that differ from the plan's at samples 1 000 000 and 1 000 001
    only are told apart, and the message names the first"""
    p = plan(cm, "S1")
    other = p.cs.mask.copy()
    assert other[1000000] and not other[1000001] and 1000000 > G.GRID_THREADS
    other[1000000], other[1000001] = False, True
    for flags in (np.where(other, -7, 5).astype(np.int32), other):
        H = cm.gf._Gaps(flags, p.cs.sizes)
        assert b"sample 1000000 " in refused(cm, "cm2_gaps_prepare_tiles", H.h, p.T.h)


# ================================================================ argument errors ===
def test_argument_errors(cm):
    cs = G.case("E")
    flags = cm.D.to_dev(cs.i32)
    lib = cm.hip.load()

    def no_handle(sizes, kind=0, a0=None, nt=cs.nt, nblocks=None):
        rc, h = create(cm, flags, kind, nt, sizes, a0, nblocks)
        msg = lib.cm2_last_error()
        assert rc == cm.hip.ERR_ARGUMENT and b"cm2_gaps_create" in msg, (rc, msg)
        assert not h.value, "*out is not NULL"
        return msg

    no_handle((1, 8191, 1, 4000, 4267))                    # less than nt
    no_handle((1, 8191, 1, 4000, 4269))                    # more than nt
    no_handle((1, 8191, 0, 4001, 4268))                    # a block of size 0
    no_handle((1, 1, 1, 1), nt=3, nblocks=4)               # nblocks > nt
    no_handle(cs.sizes, kind=2)
    for bad in (0.0, -1.0, np.nan):
        a0 = cs.a0.copy()
        a0[3] = bad
        no_handle(cs.sizes, a0=a0)
    cm.torch.cuda.synchronize()

    ng = int(cs.mask.sum())
    H, Hno = handle(cm, cs, "i32"), handle(cm, cs, "i32", a0=None)
    d, n, y = Guarded(cm, cs.nt, cs.d), Guarded(cm, cs.nt, cs.n), Guarded(cm, ng, cs.y)
    out, comp = Guarded(cm, cs.nt), Guarded(cm, ng)

    refused(cm, "cm2_gaps_masked_diff", H.h, n.ptr, d.ptr, d.ptr)
    refused(cm, "cm2_gaps_masked_diff", H.h, n.ptr, d.ptr, n.ptr)
    refused(cm, "cm2_gaps_finish", H.h, d.ptr, n.ptr, y.ptr, n.ptr)
    refused(cm, "cm2_gaps_fill_linear", H.h, d.ptr, out.ptr, 0)
    bands = N.make_bands(8, len(cs.sizes))
    op = cm.I.BlockLO(list(cs.sizes), [b for b in bands], offdiag=True)
    assert b"without a_0" in refused(cm, "cm2_gaps_normal_apply", Hno.h, op._noise.h, y.ptr, comp.ptr)
    assert b"without a_0" in refused(cm, "cm2_gaps_rhs", Hno.h, op._noise.h, n.ptr, d.ptr, out.ptr, comp.ptr)
    assert b"without a_0" in refused(cm, "cm2_gaps_precond_apply", Hno.h, y.ptr, comp.ptr)
    longer = cm.I.BlockLO([1, 8191, 1, 4000, 4269], [b for b in bands], offdiag=True)
    fewer = cm.I.BlockLO([1, 8191, 1, 8268], [b for b in bands[:4]], offdiag=True)
    for other in (longer, fewer):
        refused(cm, "cm2_gaps_normal_apply", H.h, other._noise.h, y.ptr, comp.ptr)
        refused(cm, "cm2_gaps_rhs", H.h, other._noise.h, n.ptr, d.ptr, out.ptr, comp.ptr)
    p = plan(cm, "E")
    tb = Guarded(cm, p.T.nvalid, np.zeros(p.T.nvalid))
    unprepared = cm.gf._Gaps(p.pix, cs.sizes)
    assert b"has not been called" in refused(cm, "cm2_gaps_tiles_to_time", unprepared.h, p.T.h, tb.ptr, y.ptr, out.ptr)
    # nothing was written, nothing was changed
    _all_nan(out, "refused calls: stream output")
    _all_nan(comp, "refused calls: compact output")
    for g, data in ((d, cs.d), (n, cs.n), (y, cs.y)):
        _unchanged(g, data, "refused calls")
