"""
The order-independent ground-bin sums on the GPU (cm2_ground_sums_*, GroundFilterLO(..., reproducible=True)) against
the restatement of _ground_exact_ref.py, bit for bit.

Shapes (nt, nbins): one sample; a tail shorter than a workgroup; more than one workgroup with an odd bin count; the
LDS route's last size (2048) and the first beyond it; both sides of the 8192 bins the default route is limited to.
Every case kind of the reference at (16385, 257), `normal` and `wide` everywhere; route 0 and each forced route the
shape allows.  The labels include -1 and, at the C ABI, values >= nbins, which the kernels skip.
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_ref as F  # noqa: E402
import _ground_exact_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(nt, nbins, kind) for nt, nbins in R.SHAPES for kind in (R.KINDS if (nt, nbins) == (16385, 257)
                                                                  else ("normal", "wide"))]


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, U=U, L=L, D=device, hip=_hip, cg=cosmomap2_amd.cg, torch=torch)


@functools.lru_cache(maxsize=None)
def reference(kind, nt, nbins):
    g, v = R.case(kind, nt, nbins, beyond=True)
    want = R.exact_sums(g, v, nbins)
    want.setflags(write=False)
    return g, v, want


def routes_of(nbins):
    return (0, 1, 2) if nbins <= R.LDS_BINS else (0, 2)


def sums_on_gpu(cm, h, g, v, route):
    return cm.D.to_host(h.apply(len(g), cm.D.i32(g), cm.D.f64(v), route))


def assert_same_bits(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)
    assert (R.bits(got)[~np.isnan(want)] == R.bits(want)[~np.isnan(want)]).all(), what + ": the sign of a zero"


@pytest.mark.parametrize("nt,nbins,kind", CASES)
def test_apply_equals_the_reference_on_every_route(cm, nt, nbins, kind):
    g, v, want = reference(kind, nt, nbins)
    h = cm.L._GroundSums(nbins)
    assert h.info() == dict(nbins=nbins, lds_bins=2048, lds_bytes=24 * nbins if nbins <= 2048 else 0,
                            route=1 if nbins <= 2048 else 2)
    for route in routes_of(nbins):
        assert_same_bits(sums_on_gpu(cm, h, g, v, route), want, "%s nt=%d nbins=%d route %d" % (kind, nt, nbins, route))
    if kind == "zeros":
        assert (R.bits(want) == 0).all()


@pytest.mark.parametrize("nt,nbins", [(255, 3), (16385, 257), (70000, 2048), (70000, 2049), (100001, 8192)])
def test_twice_and_permuted_give_the_same_bits(cm, nt, nbins):
    g, v, want = reference("wide", nt, nbins)
    p = np.random.default_rng(nt + nbins).permutation(nt)
    h = cm.L._GroundSums(nbins)
    for route in routes_of(nbins):
        for gg, vv, what in ((g, v, "first"), (g, v, "second"), (g[p], v[p], "permuted")):
            assert_same_bits(sums_on_gpu(cm, h, gg, vv, route), want, "%s, route %d" % (what, route))


def test_nan_poisons_every_bin_only_when_it_is_counted(cm):
    nt, nbins = 16385, 257
    g, v, want = reference("normal", nt, nbins)
    at = int(np.flatnonzero(g == 5)[0])
    h = cm.L._GroundSums(nbins)
    for bad in (np.nan, np.inf, -np.inf):
        vb = v.copy()
        vb[at] = bad
        for route in routes_of(nbins):
            assert np.isnan(sums_on_gpu(cm, h, g, vb, route)).all(), (bad, route)
    for label in (-1, nbins, 2 ** 31 - 1):
        gb, vb = g.copy(), v.copy()
        gb[at], vb[at] = label, np.nan
        g1 = g.copy()
        g1[at] = label
        for route in routes_of(nbins):
            assert_same_bits(sums_on_gpu(cm, h, gb, vb, route), R.exact_sums(g1, v, nbins), "NaN under %d" % label)
    assert_same_bits(sums_on_gpu(cm, h, g, v, 0), want, "the handle after the poisoned calls")


@functools.lru_cache(maxsize=None)
def filter_refs(nt, nbins):
    g, v = F.ground_case(nt, nbins)
    return (g, v) + F.ground_ref(g, v, nbins)


@pytest.mark.parametrize("nt,nbins", [(255, 3), (16385, 257), (70000, 2049), (70000, 8193)])
def test_reproducible_operator(cm, nt, nbins):
    g, v, sums_ref, mags, hits, out_ref, S, hs = filter_refs(nt, nbins)
    Fg = cm.I.GroundFilterLO(g, reproducible=True)
    assert Fg.reproducible is True and Fg.nbins == nbins and Fg.n == nt
    y = Fg * v
    F.assert_within(y, out_ref, S, F.c_ground_filtered(hs), "GroundFilterLO(reproducible=True), %d bins" % nbins)
    F.assert_bit_equal(y[g < 0], v[g < 0], "samples without a bin")
    assert_same_bits(cm.D.to_host(Fg._bin_sums(cm.D.f64(v))), R.exact_sums(g, v, nbins), "G^T v")
    np.testing.assert_array_equal(Fg * v, y)
    np.testing.assert_array_equal(cm.I.GroundFilterLO(g, reproducible=True) * v, y)
    np.testing.assert_array_equal(Fg.counts_in_groundbins(g), hits.astype(np.float64))


def test_default_operator_makes_no_handle(cm):
    g, v = F.ground_case(255, 3)
    Fg = cm.I.GroundFilterLO(g)
    Fg * v
    assert Fg.reproducible is False and getattr(Fg, "_sums", None) is None


def chain_problem(cm, pol, nbins, seed):
    nt, npix = 5000, 300
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, npix, nt).astype(np.int32)
    pix[rng.random(nt) < 0.05] = -1
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=rng.random(nt))
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    az = rng.integers(-1, nbins, nt).astype(np.int32)
    az[-1] = nbins - 1
    return SimpleNamespace(P=P, ces=ces, n=n, az=az, x=rng.standard_normal(pol * n), d=rng.standard_normal(nt))


def chain(cm, c):
    return c.P.T * cm.I.GroundFilterLO(c.az, reproducible=True) * c.P


@pytest.fixture
def tiled(cm):
    before = cm.L.POINTING_MODE
    cm.L.set_pointing_mode("tiled")
    yield
    cm.L.set_pointing_mode(before)


@pytest.mark.parametrize("pol", [1, 3])
def test_tiled_chain_is_bit_identical_and_equals_the_exact_order(cm, tiled, pol):
    c = chain_problem(cm, pol, 20, 40 + pol)
    A1, A2 = chain(cm, c), chain(cm, c)
    y1 = A1 * c.x
    assert [type(op).__name__ for op in A1._compiled()] == ["_TiledNormalLO"]
    np.testing.assert_array_equal(A2 * c.x, y1)
    np.testing.assert_array_equal(A1 * c.x, y1)
    cm.L.set_pointing_mode("exact")
    exact = chain(cm, c) * c.x
    assert np.linalg.norm(y1 - exact) / np.linalg.norm(exact) < 1e-13


@pytest.mark.parametrize("nbins", [20, 9000])
def test_time_order_and_tile_order_give_the_same_sums(cm, nbins):
    """the tile order lacks the flagged-pixel samples, which hold 0 in P x, and keeps the others in another order"""
    c = chain_problem(cm, 3, nbins, 5)
    D, st = cm.D, cm.D.stream()
    Fg = cm.I.GroundFilterLO(c.az, reproducible=True)
    T = cm.L._sparse_tiles(c.P)
    tod = D.f64(c.P * c.x)
    assert T.nt == tod.numel() and 0 < T.nvalid < T.nt
    tb, lab, az = D.empty(T.nvalid), D.empty(T.nvalid, cm.torch.int32), D.i32(c.az)
    cm.hip.call("cm2_tod_time_to_tiles", T.h, D.ptr(tod), D.ptr(tb), st)
    cm.hip.call("cm2_i32_time_to_tiles", T.h, D.ptr(az), D.ptr(lab), st)
    in_time = D.to_host(Fg._bin_sums(tod))
    assert_same_bits(D.to_host(Fg._sums.apply(T.nvalid, lab, tb)), in_time, "tile order")
    assert_same_bits(in_time, R.exact_sums(c.az, D.to_host(tod), nbins), "time order")


def test_tiled_chain_with_9000_bins_stays_on_the_tile_order(cm, tiled):
    c = chain_problem(cm, 3, 9000, 9)
    ran = {}
    for reproducible in (True, False):
        Fg = cm.I.GroundFilterLO(c.az, reproducible=reproducible)
        assert Fg.nbins == 9000 > Fg.LDS_BINS
        inner = Fg._apply_tiles
        seen = ran[reproducible] = []
        Fg._apply_tiles = lambda T, a, b, inner=inner, seen=seen: seen.append(inner(T, a, b)) or seen[-1]
        A = c.P.T * Fg * c.P
        y = A * c.x
        plan = A._compiled()
        assert len(plan) == 1 and isinstance(plan[0], cm.L._TiledNormalLO)
        if reproducible:
            y_rep = y
    assert ran == {True: [True], False: [False]}         # the default leaves the tile order above 8192 bins
    cm.L.set_pointing_mode("exact")
    exact = chain(cm, c) * c.x
    assert np.linalg.norm(y_rep - exact) / np.linalg.norm(exact) < 1e-13


def test_pcg_runs_are_identical(cm, tiled):
    c = chain_problem(cm, 3, 20, 77)
    M = cm.I.BlockDiagonalPreconditionerLO(c.ces, c.n, pol=3)
    runs = []
    for _ in range(2):
        Fg = cm.I.GroundFilterLO(c.az, reproducible=True)
        A = c.P.T * Fg * c.P
        b = c.P.T * (Fg * c.d)
        its = []
        x, info = cm.cg(A, b, M=M, rtol=1e-8, callback=lambda xk: its.append(np.array(xk, copy=True)))
        assert info == 0 and len(its) > 3
        runs.append((b, x, its))
    (b1, x1, its1), (b2, x2, its2) = runs
    np.testing.assert_array_equal(b1, b2)
    assert len(its1) == len(its2)
    for k, (u, w) in enumerate(zip(its1, its2)):
        np.testing.assert_array_equal(u, w, err_msg="iterate %d" % k)
    np.testing.assert_array_equal(x1, x2)
