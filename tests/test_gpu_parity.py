"""
GPU parity tests: the HIP path (through the C ABI, via the drop-in Python classes)
against the CPU oracle on the same seeded inputs, and against the golden vectors made
from the reference's own code.  Integer/index results and every deterministic
fixed-order kernel are compared BIT FOR BIT; reductions whose summation tree differs
from the BLAS/NumPy one are compared at 1e-12 relative.
"""
import os

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    import cosmomap2_amd
    from types import SimpleNamespace
    return SimpleNamespace(I=I, U=U, cg=cosmomap2_amd.cg, torch=torch)


def make_problem(oracle, seed, nt, npix, nb, pol, flag_frac=0.0, bandsize=2):
    rng = np.random.default_rng(seed)
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb, bandsize)
    if flag_frac:
        pairs[rng.random(nt) < flag_frac] = -1
    return d, pairs, phi, t, diag


# ------------------------------------------------------------------ a6 / a7 ------
@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("nt,npix", [(80, 50), (10000, 100), (20000, 600)])
def test_process_time_samples_bitexact(cm, oracle, pol, nt, npix):
    d, pairs, phi, t, diag = make_problem(oracle, 11 + pol, nt, npix, 4, pol, flag_frac=0.05)
    w = np.random.default_rng(3).random(nt)
    p_o = pairs.copy()
    ro = oracle.process_time_samples(p_o, npix, pol=pol, phi=phi, w=w)
    p_g = pairs.astype(np.int64)                 # callers pass int64 (np.random.randint)
    rg = cm.U.ProcessTimeSamples(p_g, npix, pol=pol, phi=phi, w=w)
    assert rg.get_new_pixel[0] == ro.new_npix
    np.testing.assert_array_equal(rg.old2new, ro.old2new)
    np.testing.assert_array_equal(rg.mask, ro.mask)
    np.testing.assert_array_equal(p_g, p_o)      # flagged IN PLACE
    np.testing.assert_array_equal(rg.get_new_pixel[1], ro.obspix)
    keys = {1: ("counts",), 2: ("cos2", "sin2", "sincos"),
            3: ("counts", "cosine", "sine", "cos2", "sin2", "sincos")}[pol]
    for k in keys:
        np.testing.assert_array_equal(getattr(rg, k), getattr(ro, k), err_msg=k)
    if pol > 1:
        np.testing.assert_array_equal(rg.cos, ro.cos)
        np.testing.assert_array_equal(rg.sin, ro.sin)


def test_process_time_samples_removes_bad_pixels(cm, oracle):
    # pixel 0 never observed, pixel 1 observed twice (pol=3 needs counts>2), pixel 2 observed at
    # a single angle (singular QU block): all three must go, ids compact in order.
    nt, npix = 400, 12
    rng = np.random.default_rng(0)
    pairs = rng.integers(3, npix, size=nt).astype(np.int32)
    phi = oracle.angles_gen(0.1, nt)
    pairs[[5, 9]] = 1
    pairs[[20, 40, 60, 80]] = 2
    phi[[20, 40, 60, 80]] = 0.7
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=3, phi=phi)
    pg = pairs.copy()
    rg = cm.U.ProcessTimeSamples(pg, npix, pol=3, phi=phi)
    assert ro.new_npix == npix - 3 and rg.get_new_pixel[0] == npix - 3
    assert list(rg.old2new[:4]) == [-1, -1, -1, 0]
    np.testing.assert_array_equal(pg, po)
    assert (pg[[5, 9, 20, 40]] == -1).all()


# ------------------------------------------------------------------ a2 / a3 ------
@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("nt,npix", [(1000, 17), (65536, 300), (200000, 4097)])
def test_pointing_bitexact(cm, oracle, pol, nt, npix):
    d, pairs, phi, t, diag = make_problem(oracle, 100 + pol, nt, npix, 5, pol, flag_frac=0.1)
    rng = np.random.default_rng(7)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    from types import SimpleNamespace
    ces = SimpleNamespace(cos=c, sin=s)
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=ces)
    assert P.shape == (nt, pol * npix) and P.maptype == {1: "I", 2: "QU", 3: "IQU"}[pol]
    x = rng.standard_normal(pol * npix)
    v = rng.standard_normal(nt)
    np.testing.assert_array_equal(P * x, oracle.sparse_mult(pol, pairs, c, s, x))
    np.testing.assert_array_equal(P.T * v, oracle.sparse_rmult(pol, npix, pairs, c, s, v))
    # fused P^T diag(w) P == the three stages, bit for bit
    w = rng.random(nt)
    ref = oracle.ptnp_diag(pol, npix, pairs, c, s, w, x)
    P._attach_weights(SimpleNamespace(_device_diag=lambda: cm.torch.from_numpy(w).cuda()))
    np.testing.assert_array_equal(P.fused_normal_matvec(x, P._weights_keepalive), ref)
    info = P.plan_info()
    assert info["nvalid"] == int((pairs >= 0).sum()) and info["nslices"] == (npix + 63) // 64


@pytest.mark.parametrize("angles", ["half", "full"])
@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("nt,npix,tp", [(300000, 5000, 2048), (50000, 100, 64), (400000, 70000, 1024),
                                      (40000, 20, 64)])    # the last two: runs of 5..60 and > 60 per slice
def test_tiled_pointing(cm, oracle, monkeypatch, pol, nt, npix, tp, angles):
    """Tile-bucketed order: permutations exact, fixed-order scatter bit-exact / reproducible,
    LDS-atomic scatter to rounding, the tiled P^T N P equal to the exact three stages to 1e-13.  The gather is bit-exact when the tile
    plan keeps cos and sin ("full"); in the default half-angle storage (one double per sample,
    cos and sin rebuilt from tan of the half angle) it differs by an ulp or two of the map
    values."""
    from types import SimpleNamespace
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import linearoperators as L
    monkeypatch.setenv("CM2_TILE_ANGLES", angles)
    d, pairs, phi, t, diag = make_problem(oracle, 300 + pol, nt, npix, 4, pol, flag_frac=0.1)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    # angles where the half-angle form is most delicate: cos = +-1, 0 and sin = +-1, tiny sin
    c[:8] = [1.0, -1.0, 0.0, 0.0, np.cos(1e-9), -np.cos(1e-9), np.cos(np.pi - 1e-7), 6.123233995736766e-17]
    s[:8] = [0.0, 0.0, 1.0, -1.0, np.sin(1e-9), np.sin(1e-9), np.sin(np.pi - 1e-7), 1.0]
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
    T = L._sparse_tiles(P, tile_pixels=tp, slice_samples=4096)
    assert T.nvalid == int((pairs >= 0).sum())
    # (uniform tiles; a run with CM2_TILE_BALANCE=1 re-cuts them to equal sample counts)
    assert T.ntiles == (npix + tp - 1) // tp or os.environ.get("CM2_TILE_BALANCE") == "1"
    assert T.half_angle == (angles == "half" and pol > 1)
    if pol > 1:
        # weights that are not a (cos, sin) pair: the plan must keep both arrays
        P2 = cm.I.SparseLO(npix, nt, pairs, pol=pol,
                           angle_processed=SimpleNamespace(cos=0.5 * c, sin=s))
        assert not L._sparse_tiles(P2, tile_pixels=tp, slice_samples=4096).half_angle
    rng = np.random.default_rng(9)
    x = rng.standard_normal(pol * npix)
    v = rng.standard_normal(nt)
    st = D.stream()
    xd, vd = D.f64(x), D.f64(v)
    d_tb, tod, out = D.empty(T.nvalid), D.empty(nt), D.empty(pol * npix)
    _hip.call("cm2_P_tiles_apply", T.h, D.ptr(xd), D.ptr(d_tb), st)
    _hip.call("cm2_tod_tiles_to_time", T.h, D.ptr(d_tb), D.ptr(tod), st)
    gather_ref = oracle.sparse_mult(pol, pairs, c, s, x)
    if angles == "full" or pol == 1:
        np.testing.assert_array_equal(tod.cpu().numpy(), gather_ref)
    else:
        np.testing.assert_allclose(tod.cpu().numpy(), gather_ref, rtol=0,
                                   atol=1e-15 * np.abs(x).max())
    v_tb = D.empty(T.nvalid)
    _hip.call("cm2_tod_time_to_tiles", T.h, D.ptr(vd), D.ptr(v_tb), st)
    back = D.empty(nt)
    _hip.call("cm2_tod_tiles_to_time", T.h, D.ptr(v_tb), D.ptr(back), st)
    np.testing.assert_array_equal(back.cpu().numpy(), np.where(pairs >= 0, v, 0.0))
    # P^T, default = fixed order: every pixel's terms are added in time order starting from 0,
    # as in the reference's serial loop.  With both angle arrays that is the oracle's result bit
    # for bit; with half angles it differs by the rebuilt cos / sin (3.4e-16) but is still
    # bitwise reproducible from run to run.
    assert T.pt_fixed
    _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(v_tb), D.ptr(out), st)
    ref = oracle.sparse_rmult(pol, npix, pairs, c, s, v)
    fixed = out.cpu().numpy().copy()
    if angles == "full" or pol == 1:
        np.testing.assert_array_equal(fixed, ref)
    else:
        assert rel_l2(fixed, ref) < 1e-14
    out.fill_(123.0)                                    # the kernel must overwrite, not add
    _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(v_tb), D.ptr(out), st)
    np.testing.assert_array_equal(out.cpu().numpy(), fixed)
    # tile ranges (the multi-GPU overlap path) give the same bits
    out.fill_(-7.0)
    cuts = [0, T.ntiles // 3, T.ntiles // 3, T.ntiles]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _hip.call("cm2_Pt_tiles_apply_range", T.h, D.ptr(v_tb), D.ptr(out), lo, hi, st)
    np.testing.assert_array_equal(out.cpu().numpy(), fixed)
    # the LDS-atomic form: same terms, unspecified order
    T.set_pt_order(False)
    _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(v_tb), D.ptr(out), st)
    assert rel_l2(out.cpu().numpy(), ref) < 1e-14
    T.set_pt_order(True)
    sizes = [nt // 4] * 4
    bands = [np.array([1.0 + 0.2 * b, 0.3, -0.1]) for b in range(4)]
    N = cm.I.BlockLO(sizes, bands, offdiag=True)
    tiled = L._TiledNormalLO(P, N)
    exact = P.T * (N * (P * x))
    assert rel_l2(tiled * x, exact) < 1e-13
    # N^-1 applied directly on the tile order by the fused overlap-save kernel
    lam = 40
    kk = np.arange(lam)
    bands_l = [(1.0 + 0.1 * b) * np.exp(-kk / 9.0) for b in range(4)]
    Nl = cm.I.BlockLO(sizes, bands_l, offdiag=True, method=3)
    exact_l = P.T * (cm.I.BlockLO(sizes, bands_l, offdiag=True, method=1) * (P * x))
    assert rel_l2(L._TiledNormalLO(P, Nl) * x, exact_l) < 1e-12
    L.set_pointing_mode("tiled")
    try:
        assert rel_l2((P.T * N * P) * x, exact) < 1e-13
        L.set_pointing_mode("exact")
        np.testing.assert_array_equal((P.T * N * P) * x, exact)
    finally:
        L.set_pointing_mode("auto")


def test_full_size_properties_c2(cm):
    """BASELINE config C2 at full size (nside 128 IQU, 1e7 samples, diagonal N, generated in
    HBM): size-independent identities instead of an oracle run -- P^T P 1 = hit counts
    (exact integers), fused chain == stepwise chain (bit for bit), tiled chain == exact chain
    (rounding), symmetry x.Ay = y.Ax, M_BD A x = x, linearity."""
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd import device as D
    t = cm.torch
    nside, nt, nb, pol = 128, 10_000_000, 100, 3
    npix = 12 * nside * nside
    g = t.Generator(device="cuda").manual_seed(20161203)
    pix = t.randint(0, npix, (nt,), generator=g, device="cuda", dtype=t.int32)
    phi = 0.7 + (2 * np.pi * 2.5 / 200.0) * t.arange(nt, device="cuda", dtype=t.float64)
    wts = list(np.random.default_rng(1).random(nb) + 0.5)
    N = cm.I.BlockLO(nt // nb, wts)
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi, w=N._device_diag())
    n = ces.get_new_pixel[0]
    assert n == npix                                   # ~51 hits per pixel: nothing is removed
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    hits = t.bincount(pix.long(), minlength=npix).double()
    P1 = cm.I.SparseLO(n, nt, pix, pol=1)
    assert t.equal(P1.T * (P1 * t.ones(n, dtype=t.float64, device="cuda")), hits)
    x = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64)
    y = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64)
    A = P.T * N * P
    Ax = A * x
    assert t.equal(Ax, P.T * (N * (P * x)))            # fused kernel == three stages
    Ay = A * y
    dots = D.dot(y, Ax), D.dot(x, Ay)
    assert abs(dots[0] - dots[1]) <= 1e-12 * abs(dots[0])
    assert float((M * Ax - x).norm() / x.norm()) < 1e-12          # diagonal N: M_BD = A^-1
    lin = A * (2.0 * x + y) - (2.0 * Ax + Ay)
    assert float(lin.norm() / Ax.norm()) < 1e-14
    # the same pointing with a short Toeplitz band: tile-bucketed chain vs exact chain
    band = [np.array([1.0 + 0.01 * b, 0.25, -0.05]) for b in range(nb)]
    Nt = cm.I.BlockLO(nt // nb, band, offdiag=True)
    exact = P.T * (Nt * (P * x))
    tiled = L._TiledNormalLO(P, Nt) * x
    assert float((tiled - exact).norm() / exact.norm()) < 1e-13
    assert L._use_tiles(P)                              # >= 2^20 samples: the default takes it
    assert float(((P.T * Nt * P) * x - exact).norm() / exact.norm()) < 1e-13


def test_pointing_errors(cm):
    with pytest.raises(RuntimeError):
        cm.I.SparseLO(10, 20, np.zeros(20, dtype=np.int32), pol=4)      # linearoperators.py:549
    with pytest.raises(RuntimeError):
        cm.I.SparseLO(10, 20, np.full(20, 10, dtype=np.int32))          # pixel id out of range
    P = cm.I.SparseLO(10, 20, np.zeros(20, dtype=np.int32))
    with pytest.raises(cm.I.lp.ShapeError):
        P * np.ones(11)
    # all samples flagged, empty pixels
    P = cm.I.SparseLO(70, 20, np.full(20, -1, dtype=np.int32))
    assert not (P * np.ones(70)).any() and not (P.T * np.ones(20)).any()
    # the tile plan is a C entry point of its own: it validates the pixel range itself
    import ctypes
    from cosmomap2_amd import _hip, device as D
    bad = D.i32(np.array([0, 3, 12, 5] * 64, dtype=np.int32))
    h = ctypes.c_void_p()
    with pytest.raises(_hip.HipError, match="outside"):
        _hip.call("cm2_tiles_create", ctypes.byref(h), D.ptr(bad), None, None, bad.numel(), 10, 1,
                  64, 4096, D.stream())
    assert not h.value
    # a tile plan of a pointing without valid samples still gives P^T = 0 through both orders
    from cosmomap2_amd.interfaces import linearoperators as L
    T = L._sparse_tiles(P, tile_pixels=64, slice_samples=4096)
    out = D.empty(70)
    for fixed in (True, False):
        T.set_pt_order(fixed)
        out.fill_(5.0)
        _hip.call("cm2_Pt_tiles_apply", T.h, None, D.ptr(out), D.stream())
        assert not out.cpu().numpy().any()


def test_device_resident_vectors(cm, oracle):
    """torch tensors in HBM go in and come out without a host round trip."""
    nt, npix, pol = 5000, 64, 3
    d, pairs, phi, t, diag = make_problem(oracle, 5, nt, npix, 1, pol)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    P = cm.I.SparseLO(ces.get_new_pixel[0], nt, pairs, pol=pol, angle_processed=ces)
    x = cm.torch.ones(P.shape[1], dtype=cm.torch.float64, device="cuda")
    y = P.T * (P * x)
    assert y.is_cuda and y.dtype == cm.torch.float64
    np.testing.assert_array_equal(y.cpu().numpy(), P.T * (P * np.ones(P.shape[1])))


# ------------------------------------------------------------------ a8 / a9 ------
@pytest.mark.parametrize("pol", [1, 2, 3])
def test_block_operators_bitexact(cm, oracle, golden, pol):
    d, pairs, phi, t, diag = make_problem(oracle, 21, 20000, 100, 4, pol)
    po = pairs.copy()
    ro = oracle.process_time_samples(po, 100, pol=pol, phi=phi)
    pg = pairs.copy()
    rg = cm.U.ProcessTimeSamples(pg, 100, pol=pol, phi=phi)
    n = rg.get_new_pixel[0]
    x = np.random.default_rng(1).standard_normal(pol * n)
    M = cm.I.BlockDiagonalPreconditionerLO(rg, n, pol=pol)
    B = cm.I.BlockDiagonalLO(rg, n, pol=pol)
    np.testing.assert_array_equal(M * x, oracle.bd_precond_mult(pol, ro, x))
    np.testing.assert_array_equal(B * x, oracle.bd_mult(pol, ro, x))
    # golden vectors from the reference's own BlockDiagonalLO.mult
    from types import SimpleNamespace
    W = SimpleNamespace(counts=golden["bd_counts"], cosine=golden["bd_cos"], sine=golden["bd_sin"],
                        cos2=golden["bd_cos2"], sin2=golden["bd_sin2"], sincos=golden["bd_sincos"])
    Bg = cm.I.BlockDiagonalLO(W, 23, pol=pol)
    np.testing.assert_array_equal(Bg * golden["bd_x%d" % pol], golden["bd_y%d" % pol])


def test_bd_preconditioner_masks_singular_pixels(cm, oracle, golden):
    from types import SimpleNamespace
    W = SimpleNamespace(counts=golden["bdp1_counts"])
    M = cm.I.BlockDiagonalPreconditionerLO(W, 23, pol=1)
    np.testing.assert_array_equal(M * golden["bdp1_x"], golden["bdp1_y"])
    z = np.zeros(4)
    W3 = SimpleNamespace(counts=z + 5, cosine=z, sine=z, cos2=z + 1e-3, sin2=z + 1e-3, sincos=z)
    M3 = cm.I.BlockDiagonalPreconditionerLO(W3, 4, pol=3)     # |det| = 5e-6 <= 1e-5 -> zero
    assert not (M3 * np.ones(12)).any()


# ------------------------------------------------------------------ a4 / a5 ------
@pytest.mark.parametrize("lam", [1, 2, 33])
def test_toeplitz_direct_bitexact_vs_reference(cm, golden, lam):
    a, v = golden["toep_a%d" % lam], golden["toep_v"]
    T = cm.I.ToeplitzLO(a, len(v), method=1)
    np.testing.assert_array_equal(T * v, golden["toep_y%d" % lam])
    assert T.symmetric and T.T is T


def test_toeplitz_band_longer_than_block(cm, golden):
    T = cm.I.ToeplitzLO(golden["toep_a9"], 5, method=1)
    np.testing.assert_array_equal(T * golden["toep_vshort"], golden["toep_yshort"])


@pytest.mark.parametrize("lam,sizes", [(2, [500, 400, 124]), (33, [1000, 50, 3000]),
                                       (257, [5000, 7000]), (2048, [30000, 20000])])
def test_toeplitz_fft_matches_direct(cm, oracle, lam, sizes):
    rng = np.random.default_rng(lam)
    nb = len(sizes)
    k = np.arange(lam)
    bands = [(1.0 + 0.3 * rng.random()) * np.exp(-k / (0.2 * lam + 1.0)) *
             np.cos(0.5 * k / (lam + 1.0)) for _ in range(nb)]
    v = rng.standard_normal(sum(sizes))
    ref = oracle.blocklo_mult(sizes, bands, True, v)
    Nd = cm.I.BlockLO(sizes, bands, offdiag=True, method=1)
    Nf = cm.I.BlockLO(sizes, bands, offdiag=True, method=2)
    np.testing.assert_array_equal(Nd * v, ref)
    assert rel_l2(Nf * v, ref) < 1e-12
    assert Nf.noise_info()["method"] == 2 and Nf.noise_info()["fft_len"] > 2 * (lam - 1)
    # hand-written register FFT (one kernel, 8192 points whatever the band length is)
    Nk = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
    assert Nk.noise_info()["method"] == 3
    assert Nk.noise_info()["fft_len"] == 8192
    assert rel_l2(Nk * v, ref) < 1e-12
    ek = np.zeros(sum(sizes))
    ek[sizes[0] - 1] = 1.0
    assert np.abs((Nk * ek)[sizes[0]:]).max() < 1e-13
    if lam > 32:
        assert cm.I.BlockLO(sizes, bands, offdiag=True).noise_info()["method"] == 3   # AUTO
    # zero boundary: an impulse at a block edge must not leak into the neighbour block
    e = np.zeros(sum(sizes))
    e[sizes[0] - 1] = 1.0
    out = Nf * e
    assert np.abs(out[sizes[0]:]).max() < 1e-13


def test_toeplitz_long_band_register_kernel_on_time_order(cm, oracle):
    """The overlap-save kernel on the time order with the longest bands it serves, ragged blocks
    (one barely longer than a window's hop), against the direct band sum."""
    rng = np.random.default_rng(77)
    sizes = [21000, 9000, 4098]
    for lam in (2048, 2049):
        k = np.arange(lam)
        bands = [(1.0 + 0.2 * b) * np.exp(-k / 400.0) * np.cos(k / 700.0) for b in range(3)]
        v = rng.standard_normal(sum(sizes))
        ref = oracle.blocklo_mult(sizes, bands, True, v)
        Np = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
        assert rel_l2(Np * v, ref) < 1e-12


@pytest.mark.parametrize("method", [1, 2, 3])
def test_toeplitz_tiny_and_ragged_blocks(cm, oracle, method):
    """Blocks shorter than the band, of length 1, and ragged sizes: zero boundary everywhere."""
    rng = np.random.default_rng(31 + method)
    for lam, sizes in [(33, [5, 1, 7, 100, 2]), (9, [3, 3, 3]), (130, [64, 700, 129, 1]),
                       (600, [599, 601, 50])]:
        k = np.arange(lam)
        bands = [np.exp(-k / (0.3 * lam)) * (1.0 + 0.1 * b) for b in range(len(sizes))]
        v = rng.standard_normal(sum(sizes))
        ref = oracle.blocklo_mult(sizes, bands, True, v)
        N = cm.I.BlockLO(sizes, bands, offdiag=True, method=method)
        got = N * v
        if method == 1:
            np.testing.assert_array_equal(got, ref)
        else:
            assert rel_l2(got, ref) < 1e-12, (lam, sizes)


@pytest.mark.parametrize("pol", [1, 3])
def test_pointing_degenerate_shapes(cm, oracle, pol):
    """One sample, wave-size boundaries, one hot pixel holding almost every sample, a noise
    block whose samples are all flagged -- exact and tile-bucketed forms against the oracle."""
    from types import SimpleNamespace
    from cosmomap2_amd.interfaces import linearoperators as L
    rng = np.random.default_rng(17)
    cases = []
    for nt in (1, 63, 64, 65, 257):
        cases.append((nt, 3, rng.integers(0, 3, nt).astype(np.int32)))
    hot = rng.integers(0, 200, 50000).astype(np.int32)
    hot[rng.random(50000) < 0.9] = 77                      # 90 % of the samples in one pixel
    cases.append((50000, 200, hot))
    dead = rng.integers(0, 130, 4000).astype(np.int32)
    dead[1000:2000] = -1                                    # second noise block fully flagged
    cases.append((4000, 130, dead))
    for nt, npix, pairs in cases:
        phi = oracle.angles_gen(0.4, nt)
        c, s = np.cos(2 * phi), np.sin(2 * phi)
        P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
        x = rng.standard_normal(pol * npix)
        v = rng.standard_normal(nt)
        np.testing.assert_array_equal(P * x, oracle.sparse_mult(pol, pairs, c, s, x))
        np.testing.assert_array_equal(P.T * v, oracle.sparse_rmult(pol, npix, pairs, c, s, v))
        if nt >= 4:
            sizes = [nt // 4] * 3 + [nt - 3 * (nt // 4)]
            bands = [np.array([1.0, 0.3, -0.1][:min(3, max(1, sz))]) for sz in sizes]
            bands = [np.pad(b, (0, 3 - len(b))) for b in bands]
            N = cm.I.BlockLO(sizes, bands, offdiag=True)
            exact = P.T * (N * (P * x))
            tiled = L._TiledNormalLO(P, N) * x
            denom = np.linalg.norm(exact)
            # the per-pixel terms are added in a different order (LDS atomics): a pixel that
            # sums 45 000 terms of both signs loses ~sqrt(n) ulp to cancellation
            assert np.linalg.norm(tiled - exact) <= 1e-11 * max(denom, 1.0)


def test_blocklo_diag_and_errors(cm, oracle):
    sizes = 2 * [500, 400, 124]
    t = list(np.random.default_rng(2).random(6))
    N = cm.I.BlockLO(sizes, t)
    assert not N.isoffdiag and N.shape == (sum(sizes), sum(sizes))
    np.testing.assert_array_equal(N.diag, oracle.blocklo_diag(sizes, t))
    v = np.random.default_rng(3).standard_normal(sum(sizes))
    np.testing.assert_array_equal(N * v, oracle.blocklo_mult(sizes, t, False, v))
    N2 = cm.I.BlockLO(100, t[:3])
    np.testing.assert_array_equal(N2.diag, oracle.blocklo_diag(100, t[:3]))
    assert len(N2.blocklist) == 3 and N2.blocklist[0].shape == (100, 100)
    with pytest.raises(cm.I.lp.ShapeError):
        N2 * np.ones(299)


# ----------------------------------------------------- reference test invariants ---
def test_PtP_ones_equals_counts(cm):
    # tests/test_matrix_vector_product.py:9-23
    np.random.seed(0)
    nt, npix = 80, 50
    pairs = cm.U.pairs_gen(nt, npix)
    processd = cm.U.ProcessTimeSamples(pairs, npix)
    npix = processd.get_new_pixel[0]
    P = cm.I.SparseLO(npix, nt, pairs)
    y = P.T * P * np.ones(npix)
    assert np.allclose(y, processd.counts)


@pytest.mark.parametrize("pol", [1, 2, 3])
def test_explicit_blockdiagonal_preconditioner(cm, pol):
    # tests/test_matrix_vector_product.py:26-63 and :65-94
    from scipy.linalg import inv
    np.random.seed(1)
    nt = 10000
    phi = cm.U.angles_gen(2., nt)
    for npix in [10, 50, 100, 300, 600]:
        pairs = cm.U.pairs_gen(nt, npix)
        processd = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
        npix = processd.get_new_pixel[0]
        P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=processd)
        x = np.ones(npix * pol)
        v = P.T * P * x
        v2 = v * 0.
        Mbd = cm.I.BlockDiagonalPreconditionerLO(processd, npix, pol=pol)
        if pol == 1:
            v2 = v / processd.counts
        elif pol == 3:
            for j in range(npix):
                matr = np.array([[Mbd.counts[j], Mbd.cos[j], Mbd.sin[j]],
                                 [Mbd.cos[j], Mbd.cos2[j], Mbd.sincos[j]],
                                 [Mbd.sin[j], Mbd.sincos[j], Mbd.sin2[j]]])
                v2[3 * j:3 * j + 3] = inv(matr).dot(v[3 * j:3 * j + 3])
        else:
            for j in range(npix):
                matr = np.array([[Mbd.cos2[j], Mbd.sincos[j]], [Mbd.sincos[j], Mbd.sin2[j]]])
                v2[2 * j:2 * j + 2] = inv(matr).dot(v[2 * j:2 * j + 2])
        assert np.allclose(v2, Mbd * v)
        xt = {1: np.ones(npix), 3: np.tile([0, 0, 1.], npix), 2: np.tile([0, 1.], npix)}[pol]
        assert np.allclose(Mbd * P.T * P * xt, xt)


@pytest.mark.parametrize("pol", [1, 2, 3])
def test_block_diagonal_operator_and_spd(cm, pol):
    # tests/test_block_diagonal_operator.py:8-64
    np.random.seed(2)
    nt, npix = 2 ** 14, 128
    d, pairs, phi, t, diag = cm.U.system_setup(nt, npix, 1)
    processd = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    npix = processd.get_new_pixel[0]
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=processd)
    x = np.ones(pol * npix)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(processd, npix, pol=pol)
    invMbd = cm.I.BlockDiagonalLO(processd, npix, pol=pol)
    assert np.allclose(invMbd * x, P.T * P * x)
    assert np.allclose(Mbd * invMbd * x, x)
    nb, blocksize = 6, 2 * [500, 400, 124]
    nt = sum(blocksize)
    d, pairs, phi, t, diag = cm.U.system_setup(nt, 64, nb)
    N = cm.I.BlockLO(blocksize, diag, offdiag=False)
    processd = cm.U.ProcessTimeSamples(pairs, 64, pol=pol, phi=phi, w=N.diag)
    npix = processd.get_new_pixel[0]
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=processd)
    r = np.random.rand(pol * npix)
    A = P.T * N * P
    assert np.allclose(A * r, A.T * r) and cm.U.scalprod(r, A * r) > 0.
    Mbd = cm.I.BlockDiagonalPreconditionerLO(processd, npix, pol)
    assert np.allclose(Mbd * r, Mbd.T * r) and cm.U.scalprod(r, Mbd * r) > 0.
    # tests/test_toeplitz_vector_multiplication.py:58-76: BlockDiagonalLO == P^T N P, w = N.diag
    PtNP = cm.I.BlockDiagonalLO(processd, npix, pol=pol)
    assert np.allclose(PtNP * np.ones(pol * npix), P.T * N * P * np.ones(pol * npix))


@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("offdiag", [False, True])
def test_composed_equals_stepwise(cm, oracle, pol, offdiag):
    # tests/test_toeplitz_vector_multiplication.py:6-55; the composed product takes the
    # fused kernel for diagonal N -- it must give the same bits as the three stages.
    np.random.seed(3)
    nb, blocksize = 6, 2 * [500, 400, 124]
    nt = sum(blocksize)
    d, pairs, phi, t, diag = cm.U.system_setup(nt, 64, nb)
    N = cm.I.BlockLO(blocksize, t if offdiag else diag, offdiag=offdiag)
    processd = cm.U.ProcessTimeSamples(pairs, 64, pol=pol, phi=phi,
                                       w=None if offdiag else N.diag)
    npix = processd.get_new_pixel[0]
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=processd)
    x = np.random.rand(pol * npix)
    z = P.T * (N * (P * x))
    z2 = P.T * N * P * x
    np.testing.assert_array_equal(z2, z)
    c = processd.cos if pol > 1 else None
    s = processd.sin if pol > 1 else None
    zo = oracle.sparse_rmult(pol, npix, pairs, c, s, oracle.blocklo_mult(
        blocksize, t if offdiag else diag, offdiag, oracle.sparse_mult(pol, pairs, c, s, x)))
    np.testing.assert_array_equal(z, zo)


# ------------------------------------------------------------- a15 BLAS helpers ---
def test_blas_helpers(cm, golden):
    G = golden
    np.testing.assert_allclose(cm.U.dgemm(G["la_A"], G["la_B"]), G["la_dgemm"], rtol=1e-13)
    assert cm.U.norm2(G["la_q"]) == pytest.approx(float(G["la_norm2"]), rel=1e-14)
    assert cm.U.scalprod(G["la_q"], G["la_q2"]) == pytest.approx(float(G["la_scalprod"]), rel=1e-13,
                                                                 abs=1e-14)
    x = np.random.default_rng(0).standard_normal(1_000_003)
    assert cm.U.norm2(x) == pytest.approx(np.linalg.norm(x), rel=1e-13)
    assert cm.U.scalprod(x, x[::-1].copy()) == pytest.approx(float(x.dot(x[::-1])), rel=1e-10,
                                                             abs=1e-9)


def test_generators_match_reference_streams(cm, golden):
    import random
    G = golden
    np.testing.assert_array_equal(cm.U.angles_gen(0.3, 50), G["gen_angles"])
    np.random.seed(int(G["gen_seed"]))
    random.seed(int(G["gen_seed"]))
    d, pairs, phi, t, diag = cm.U.system_setup(120, 17, 3)
    np.testing.assert_array_equal(d, G["gen_d"])
    np.testing.assert_array_equal(pairs, G["gen_pairs"])
    np.testing.assert_array_equal(phi, G["gen_phi"])
    np.testing.assert_array_equal(np.asarray(t), G["gen_t"])
    np.testing.assert_array_equal(np.asarray(diag), G["gen_diag"])


# -------------------------------------------------------- a10 / a11 deflation ---
def test_deflation_and_coarse_vs_reference(cm, golden, oracle):
    G = golden
    Z, A, v = G["defl_Z"], G["coarse_A"], G["coarse_v"]
    Zd = cm.I.DeflationLO(Z)
    np.testing.assert_array_equal(Zd * G["defl_y"], G["defl_Zy"])       # same term order
    np.testing.assert_allclose(Zd.T * G["defl_x"], G["defl_Ztx"], rtol=1e-13)
    np.testing.assert_allclose(Zd.H * G["defl_x"], G["defl_Ztx"], rtol=1e-13)
    assert len(Zd.z) == 4 and np.array_equal(Zd.z[2], Z[:, 2])
    Az = A @ Z
    lu = cm.I.CoarseLO(Z, Az, 4, apply='LU')
    np.testing.assert_allclose(lu.E, G["coarse_E"], rtol=1e-13)
    np.testing.assert_allclose(lu * v, G["coarse_lu_x"], rtol=1e-11)
    eig = cm.I.CoarseLO(Z, Az, 4, apply='eig')
    np.testing.assert_allclose(eig.invE, G["coarse_invE"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(eig * v, G["coarse_eig_x"], rtol=1e-9)
    vd = cm.torch.from_numpy(v).cuda()
    np.testing.assert_allclose((lu * vd).cpu().numpy(), G["coarse_lu_x"], rtol=1e-10)
    Zdup = Z.copy()
    Zdup[:, 3] = Zdup[:, 0]
    deg = cm.I.CoarseLO(Zdup, A @ Zdup, 4, apply='eig')
    assert deg.n_discarded == 1
    np.testing.assert_allclose(deg.invE, G["coarse_deg_invE"], rtol=1e-7, atol=1e-11)


@pytest.mark.parametrize("r", [5, 16, 32, 64])
def test_coarse_matrix_mfma_and_tall_skinny(cm, r):
    rng = np.random.default_rng(r)
    n = 3 * 40000 + 7
    Z = rng.standard_normal((n, r))
    AZ = rng.standard_normal((n, r))
    E = cm.I.CoarseLO(Z, AZ, r, apply='eig').E
    ref = Z.T @ AZ
    assert rel_l2(E, ref) < 1e-13
    Zd = cm.I.DeflationLO(Z)
    x = rng.standard_normal(n)
    y = rng.standard_normal(r)
    assert rel_l2(Zd.T * x, Z.T @ x) < 1e-12
    assert rel_l2(Zd * y, Z @ y) < 1e-13


# ------------------------------------------------------------- a13 arnoldi -----
def test_arnoldi_vs_reference(cm, golden):
    G = golden
    A, b = G["arn_A"], G["arn_b"]
    Aop = cm.I.lp.LinearOperator(30, 30, lambda x: A @ x, symmetric=True)
    vs, hs, j = cm.I.arnoldi(Aop, b, x0=np.zeros(30), tol=1e-8, inner_m=30)
    assert j == int(G["arn_j"])
    np.testing.assert_allclose(np.asarray(vs), G["arn_V"], rtol=0, atol=1e-9)
    H = cm.I.build_hess(hs, j)
    np.testing.assert_allclose(H, G["arn_H"], rtol=0, atol=1e-9)
    Z, r = cm.I.build_Z(G["arn_ritz"], np.linalg.eigh(G["arn_H"])[1], G["arn_V"].T.copy(), 1e-2)
    assert r == int(G["arn_r"])
    np.testing.assert_allclose(Z, G["arn_Z"], rtol=1e-11, atol=1e-13)
    Z2, _ = cm.I.build_Z(G["arn_ritz"], np.linalg.eigh(G["arn_H"])[1], list(G["arn_V"]), 1e-2)
    np.testing.assert_allclose(Z2, G["arn_Z"], rtol=1e-11, atol=1e-13)
    with pytest.raises(RuntimeError):
        cm.I.arnoldi(Aop, b, x0=np.zeros(30), tol=1e-8, inner_m=3)
    with pytest.raises(ValueError):
        cm.I.arnoldi(Aop, b * np.nan, x0=np.zeros(30))
    assert cm.I.arnoldi(Aop, A @ np.ones(30), x0=np.ones(30), tol=1e-5)[2] == 0
    with pytest.raises(RuntimeError):
        cm.I.build_Z(G["arn_ritz"], np.eye(j), G["arn_V"].T.copy(), 1e-9)


# ---------------------------------------------------------------- a16 PCG -------
def _mapmaking_system(cm, oracle, seed, nt, npix, nb, pol, offdiag):
    np.random.seed(seed)
    import random
    random.seed(seed)
    d, pairs, phi, t, diag = cm.U.system_setup(nt, npix, nb)
    if offdiag:        # SPD banded inverse noise
        t = [np.array([1.0 + 0.5 * ti[0], 0.3 * ti[1]]) for ti in t]
    pairs = pairs.astype(np.int32)
    po = pairs.copy()
    N = cm.I.BlockLO(nt // nb, t if offdiag else diag, offdiag=offdiag)
    w = None if offdiag else N.diag
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi, w=w)
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi, w=w)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    A = P.T * N * P
    b = P.T * N * d
    c, s = (ro.cos, ro.sin)
    tt = t if offdiag else diag

    def A_o(x):
        return oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(
            nt // nb, tt, offdiag, oracle.sparse_mult(pol, po, c, s, x)))
    b_o = oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(nt // nb, tt, offdiag, d))
    M_o = lambda x: oracle.bd_precond_mult(pol, ro, x)
    return A, b, M, A_o, b_o, M_o, n


@pytest.mark.parametrize("pol,offdiag", [(1, False), (3, False), (3, True), (2, True)])
def test_pcg_matches_oracle_iterations_and_solution(cm, oracle, pol, offdiag):
    A, b, M, A_o, b_o, M_o, n = _mapmaking_system(cm, oracle, 10 + pol, 40000, 300, 4, pol, offdiag)
    np.testing.assert_array_equal(b, b_o)
    its_g, its_o = [], []
    xg, info_g = cm.cg(A, b, M=M, rtol=1e-6, callback=lambda x: its_g.append(1))
    xo, info_o = oracle.cg(A_o, b_o, M=M_o, rtol=1e-6, callback=lambda x: its_o.append(1))
    assert info_g == 0 and info_o == 0
    assert len(its_g) == len(its_o)                   # identical PCG iteration counts
    assert rel_l2(xg, xo) < 1e-6                      # north_star tolerance
    import scipy.sparse.linalg as spla
    its_s = []
    xs, info_s = spla.cg(A, b, M=M, rtol=1e-6, callback=lambda x: its_s.append(1))
    assert info_s == 0 and len(its_s) == len(its_g) and rel_l2(xs, xg) < 1e-8
    # maxiter exhaustion and device-resident call
    if offdiag:      # (with diagonal N, M_BD is the exact inverse: one step converges)
        x1, info1 = cm.cg(A, b, M=M, rtol=1e-14, maxiter=2)
        assert info1 == 2
    else:
        assert len(its_g) == 1
    bd = cm.torch.from_numpy(b).cuda()
    xd, info_d = cm.cg(A, bd, M=M, tol=1e-6)
    assert info_d == 0 and xd.is_cuda
    np.testing.assert_array_equal(xd.cpu().numpy(), xg)
    inv = cm.I.InverseLO(A, method=cm.cg, preconditioner=M)
    assert rel_l2(inv * b, xo) < 1e-4 and inv.converged == 0


@pytest.mark.parametrize("pol,lam,angles,flags", [(3, 40, "half", 0.03), (3, 40, "full", 0.0),
                                                  (2, 64, "half", 0.0), (1, 12, "half", 0.05)])
def test_tiled_path_pcg_iteration_count_equals_oracle(cm, oracle, monkeypatch, pol, lam, angles, flags):
    """The path bench.py times -- tile-bucketed order, half-angle storage, fixed-order P^T,
    register-resident overlap-save FFT -- forced with set_pointing_mode("tiled") on a problem
    the oracle can still run (2^21 samples, direct band sum of `lam` terms): the PCG iteration
    count must be the oracle's, strictly, the residual history must agree to rounding, and the
    solution to the north_star's 1e-6 (it agrees to ~1e-11)."""
    from cosmomap2_amd.interfaces import linearoperators as L
    monkeypatch.setenv("CM2_TILE_ANGLES", angles)
    nt, npix, nb = 1 << 21, 12 * 32 * 32, 8
    rng = np.random.default_rng(77 + pol)
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb)
    if flags:
        pairs[rng.random(nt) < flags] = -1
    kk = np.arange(lam)
    bands = [(1.0 + 0.03 * b) * np.where(kk == 0, 1.0, -0.22 * np.exp(-kk / 9.0)) for b in range(nb)]
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    assert n == ro.new_npix and np.array_equal(pairs, po)
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    N = cm.I.BlockLO(nt // nb, bands, offdiag=True, method=3)
    c, s = ro.cos, ro.sin

    def A_o(x):
        return oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(
            nt // nb, bands, True, oracle.sparse_mult(pol, po, c, s, x)))
    M_o = lambda x: oracle.bd_precond_mult(pol, ro, x)
    b_o = oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(nt // nb, bands, True, d))
    L.set_pointing_mode("tiled")
    try:
        A = P.T * N * P
        assert any(isinstance(op, L._TiledNormalLO) for op in A._compiled())
        T = L._sparse_tiles(P)
        assert T.pt_fixed and T.half_angle == (angles == "half" and pol > 1)
        b = P.T * (N * d)
        assert rel_l2(b, b_o) < 1e-12
        res_g, res_o = [], []
        xg, info_g = cm.cg(A, b, M=M, rtol=1e-6, maxiter=300,
                           callback=lambda x: res_g.append(np.linalg.norm(b - A * x)))
        xo, info_o = oracle.cg(A_o, b_o, M=M_o, rtol=1e-6, maxiter=300,
                               callback=lambda x: res_o.append(np.linalg.norm(b_o - A_o(x))))
        assert info_g == 0 and info_o == 0
        assert len(res_g) == len(res_o), (len(res_g), len(res_o))        # strictly identical
        np.testing.assert_allclose(res_g, res_o, rtol=1e-6)
        assert rel_l2(xg, xo) < 1e-9
        # not a knife-edge: the last residual is not within 1e-3 (relative) of the threshold
        thr = 1e-6 * np.linalg.norm(b_o)
        assert abs(res_o[-1] - thr) > 1e-3 * thr and (len(res_o) < 2 or abs(res_o[-2] - thr) > 1e-3 * thr)
        # bitwise reproducible from run to run (no atomics anywhere on the path)
        xg2, _ = cm.cg(A, b, M=M, rtol=1e-6, maxiter=300)
        np.testing.assert_array_equal(xg2, xg)
    finally:
        L.set_pointing_mode("auto")


def test_hot_pixel_is_summed_in_fixed_chunks(cm, oracle):
    """One pixel holds 5 % of 2^21 samples (a stare at a source).  Summing its terms one after
    the other is a chain of 1e5 dependent additions; the default fixed-order P^T cuts such a run
    (more than 256 hits inside one slice of a tile) into chunks of 32 consecutive terms, adds each
    chunk in time order and the chunk sums in time order: reproducible bit for bit, independent
    of the hit map, equal to the serial sum to rounding -- the PCG iteration count is the
    oracle's, strictly -- and much faster than the one-thread walk that "exact" keeps."""
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd import _hip, device as D
    t = cm.torch
    pol, lam = 3, 16
    nt, npix, nb = 1 << 21, 12 * 32 * 32, 8
    rng = np.random.default_rng(2024)
    d, pairs, phi, tt, diag = oracle.system_setup(rng, nt, npix, nb)
    hot_pix = 777
    pairs[rng.random(nt) < 0.05] = hot_pix
    pairs[rng.random(nt) < 0.01] = -1
    kk = np.arange(lam)
    bands = [(1.0 + 0.03 * b) * np.where(kk == 0, 1.0, -0.22 * np.exp(-kk / 9.0)) for b in range(nb)]
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    assert n == ro.new_npix and np.array_equal(pairs, po)
    assert int((po == hot_pix).sum()) > 0.04 * nt
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    N = cm.I.BlockLO(nt // nb, bands, offdiag=True, method=3)
    c, s = ro.cos, ro.sin

    def A_o(x):
        return oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(
            nt // nb, bands, True, oracle.sparse_mult(pol, po, c, s, x)))
    M_o = lambda x: oracle.bd_precond_mult(pol, ro, x)
    b_o = oracle.sparse_rmult(pol, n, po, c, s, oracle.blocklo_mult(nt // nb, bands, True, d))
    L.set_pointing_mode("tiled")
    try:
        A = P.T * N * P
        T = L._sparse_tiles(P)
        assert T.pt_mode == 1                               # default: fixed order, hot runs chunked
        # P^T alone: chunked (default) against the pure time order, bits and time
        v_tb = D.f64(rng.standard_normal(T.nvalid))
        out = {}
        ms = {}
        for mode in (1, 2):
            T.set_pt_order(mode)
            o = D.empty(pol * n)
            call = lambda: _hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(v_tb), D.ptr(o), D.stream())
            call()
            t.cuda.synchronize()
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                call()
            e1.record()
            t.cuda.synchronize()
            ms[mode] = e0.elapsed_time(e1) / 5
            out[mode] = o.clone()
            call()
            assert t.equal(o, out[mode])                     # reproducible bit for bit
        T.set_pt_order(1)
        err = float((out[1] - out[2]).norm() / out[2].norm())
        assert err < 1e-14, err                             # a regrouped sum, nothing else
        assert not t.equal(out[1], out[2])                  # (and it IS regrouped: the hot run is chunked)
        assert ms[1] < 0.5 * ms[2], ms                       # one-thread walk of 1e5 terms vs chunks
        # the whole solve on the default path: the oracle's iteration count, strictly
        b = P.T * (N * d)
        assert rel_l2(b, b_o) < 1e-12
        its_g, its_o = [], []
        xg, info_g = cm.cg(A, b, M=M, rtol=1e-6, maxiter=300, callback=lambda x: its_g.append(1))
        xo, info_o = oracle.cg(A_o, b_o, M=M_o, rtol=1e-6, maxiter=300, callback=lambda x: its_o.append(1))
        assert info_g == 0 and info_o == 0 and len(its_g) == len(its_o), (len(its_g), len(its_o))
        assert rel_l2(xg, xo) < 1e-9
        xg2, _ = cm.cg(A, b, M=M, rtol=1e-6, maxiter=300)
        np.testing.assert_array_equal(xg2, xg)
    finally:
        L.set_pointing_mode("auto")


def test_ritz_deflation_basis_speeds_up_pcg(cm, oracle):
    """Arnoldi (M inner product) -> Ritz vectors -> CoarseLO -> fused M2, all in HBM."""
    nt, npix, nb, pol = 60000, 400, 4, 3
    rng = np.random.default_rng(8)
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb)
    lam = 64
    k = np.arange(lam)
    band = 0.6 * np.exp(-k / 20.0)
    band[0] = 1.0 + 2 * band[1:].sum() * 0.98           # nearly singular at DC: ill-conditioned A
    band[1:] *= -1.0
    N = cm.I.BlockLO(nt // nb, [band * (1 + 0.05 * b) for b in range(nb)], offdiag=True)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    A = P.T * N * P
    b = cm.torch.from_numpy(P.T * (N * d)).cuda()
    r = 8
    Z, theta = cm.I.ritz_deflation_basis(A, M, b, r, 40)
    assert tuple(Z.shape) == (pol * n, r) and np.all(np.diff(theta) >= 0)
    # the smallest Ritz pair approximates an eigenpair of M A
    assert theta[0] > 0                                   # M A is SPD in the M^-1 inner product
    z0 = Z[:, 0].contiguous()
    res = (M * (A * z0)) - theta[0] * z0
    assert float(res.norm() / z0.norm()) < 1e-3 * theta[-1]
    AZ = cm.torch.empty_like(Z)
    for j in range(r):
        AZ[:, j] = A * Z[:, j].contiguous()
    E = cm.I.CoarseLO(Z, AZ, r, apply='eig')
    M2 = cm.I.TwoLevelPreconditionerLO(M, cm.I.DeflationLO(Z), cm.I.DeflationLO(AZ), E)
    n1, n2 = [], []
    x1, i1 = cm.cg(A, b, M=M, rtol=1e-8, maxiter=2000, callback=lambda xk: n1.append(1))
    x2, i2 = cm.cg(A, b, M=M2, rtol=1e-8, maxiter=2000, callback=lambda xk: n2.append(1))
    # With the reference generator's uniformly random pointing, M_BD A has ONE small eigenvalue
    # (the constant I map, the only map the DC-suppressing band sees as a slow time-domain mode:
    # 0.62 against a cluster at 23..25.4, dense eigen-decomposition of the oracle's operators).
    # CG disposes of one isolated eigenvalue in about one step and M2 moves the deflated ones to
    # 1, still outside the cluster, so both preconditioners need the same number of steps here.
    assert i1 == 0 and i2 == 0 and len(n2) <= len(n1)
    assert float((x2 - x1).norm() / x1.norm()) < 1e-6
    for j in range(r):                                    # deflated directions are solved exactly
        zj = Z[:, j].contiguous()
        assert float(((M2 * (A * zj)) - zj).norm() / zj.norm()) < 1e-8


def test_ritz_deflation_on_raster_scan_needs_fewer_iterations(cm, oracle):
    """What the two-level preconditioner is for: with a coherent scan the slow time-domain modes
    the 1/f band suppresses ARE smooth maps, M_BD A has a tail of small eigenvalues and deflating
    them pays (dense check on the oracle's operators for this problem: 48 PCG steps with M_BD, 33
    with the 8 smallest eigenvectors deflated).  Strictly fewer iterations, same solution."""
    nt, npix, nb, pol, dwell = 60000, 400, 4, 3, 5
    rng = np.random.default_rng(8)
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb)
    tt = np.arange(nt)
    sweep, col = (tt // dwell) // npix, (tt // dwell) % npix
    pairs = np.where(sweep % 2 == 0, col, npix - 1 - col).astype(np.int32)
    lam = 64
    k = np.arange(lam)
    band = 0.6 * np.exp(-k / 20.0)
    band[0] = 1.0 + 2 * band[1:].sum() * 0.98
    band[1:] *= -1.0
    bands = [band * (1 + 0.05 * b) for b in range(nb)]
    N = cm.I.BlockLO(nt // nb, bands, offdiag=True)
    po = pairs.copy()
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    A = P.T * N * P
    b = cm.torch.from_numpy(P.T * (N * d)).cuda()
    r = 8
    Z, theta = cm.I.ritz_deflation_basis(A, M, b, r, 60)
    AZ = cm.torch.empty_like(Z)
    for j in range(r):
        AZ[:, j] = A * Z[:, j].contiguous()
    E = cm.I.CoarseLO(Z, AZ, r, apply='eig')
    M2 = cm.I.TwoLevelPreconditionerLO(M, cm.I.DeflationLO(Z), cm.I.DeflationLO(AZ), E)
    n1, n2, no = [], [], []
    x1, i1 = cm.cg(A, b, M=M, rtol=1e-8, maxiter=2000, callback=lambda xk: n1.append(1))
    x2, i2 = cm.cg(A, b, M=M2, rtol=1e-8, maxiter=2000, callback=lambda xk: n2.append(1))

    def A_o(v):
        return oracle.sparse_rmult(pol, n, po, ro.cos, ro.sin, oracle.blocklo_mult(
            nt // nb, bands, True, oracle.sparse_mult(pol, po, ro.cos, ro.sin, v)))
    xo, io = oracle.cg(A_o, b.cpu().numpy(), M=lambda v: oracle.bd_precond_mult(pol, ro, v),
                       rtol=1e-8, maxiter=2000, callback=lambda xk: no.append(1))
    assert i1 == 0 and i2 == 0 and io == 0
    assert len(n1) == len(no)                              # M_BD: the oracle's count, strictly
    assert len(n2) < len(n1) and len(n2) <= 0.8 * len(n1), (len(n1), len(n2))
    assert float((x2 - x1).norm() / x1.norm()) < 1e-6
    assert rel_l2(x1.cpu().numpy(), xo) < 1e-6


# ------------------------------------------------------- a12 two-level precond ---
@pytest.mark.parametrize("pol", [1, 2, 3])
def test_two_level_preconditioner_invariants(cm, pol):
    # tests/test_2level_preconditioner.py:8-53 and tests/test_coarse_operator.py:6-43
    import scipy.sparse.linalg as spla
    import scipy.linalg as la
    import random
    np.random.seed(40 + pol)
    random.seed(40 + pol)
    nt, npix, nb = 500, 40, 1
    d, pairs, phi, t, diag = cm.U.system_setup(nt, npix, nb)
    t = [np.array([1.0 + 0.5 * ti[0], 0.3 * ti[1]]) for ti in t]
    N = cm.I.BlockLO(nt // nb, t, offdiag=True)
    processd = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    npix = processd.get_new_pixel[0]
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=processd)
    M = cm.I.BlockDiagonalPreconditionerLO(processd, npix, pol=pol)
    B = cm.I.BlockDiagonalLO(processd, npix, pol=pol)
    x0 = np.ones(pol * npix)
    tol = 1.e-4
    A = P.T * N * P
    eigv, Z = spla.eigsh(A, M=B, Minv=M, k=5, v0=x0, which='SM', ncv=15, tol=tol)
    r = Z.shape[1]
    Az = Z * 0.
    for i in range(r):
        Az[:, i] = A * Z[:, i]
    E = cm.I.CoarseLO(Z, Az, r)
    Zd = cm.I.DeflationLO(Z)
    # tests/test_deflation_operator.py:33-53: independent columns, Zd and Zd.H against dense Z
    assert np.linalg.matrix_rank(Z) == r and la.det(cm.U.dgemm(Z, Z.T)) != 0
    assert np.allclose(Zd * np.ones(r), Z.dot(np.ones(r)))
    assert np.allclose(Zd.H * x0, Z.T.dot(x0))
    I = cm.I.lp.IdentityOperator(pol * npix)
    R = I - A * Zd * E * Zd.T
    M2 = M * R + Zd * E * Zd.T
    AZd = cm.I.DeflationLO(Az)
    M2f = cm.I.TwoLevelPreconditionerLO(M, Zd, AZd, E)
    Eeig = cm.I.CoarseLO(Z, Az, r, apply='eig')
    Emat = cm.U.dgemm(Z, Az.T)
    v = np.ones(r)
    assert np.allclose(np.dot(Emat, Eeig * v), v) and np.allclose(la.solve(Emat, v), Eeig * v)
    assert abs(np.linalg.cond(Eeig.to_array())) < 1e3 * np.linalg.cond(Emat) + 1
    for i in range(r):
        assert np.allclose(M2 * A * Z[:, i], Z[:, i])
        assert np.allclose(M2f * (A * Z[:, i]), Z[:, i])
        assert cm.U.norm2(R * A * Z[:, i]) <= 1.e-10
        its = []
        x, info = spla.cg(M2 * A, Z[:, i], rtol=tol, maxiter=2, callback=lambda xk: its.append(1))
        assert info == 0
        assert len(its) == 1                          # tests/test_arnoldi_algorithm.py:91-93
    rr = np.random.rand(pol * npix)
    assert rel_l2(M2f * rr, M2 * rr) < 1e-10
    # PCG with M_BD and with M2: the counts must be those of the same recurrence run on the CPU
    # with dense copies of the operators (the oracle's PCG), strictly.
    b = P.T * N * d
    n1, n2, o1, o2 = [], [], [], []
    x1, i1 = cm.cg(A, b, M=M, tol=1e-8, callback=lambda xk: n1.append(1))
    x2, i2 = cm.cg(A, b, M=M2f, tol=1e-8, callback=lambda xk: n2.append(1))
    Ad, Md, M2d = A.to_array(), M.to_array(), M2f.to_array()
    from oracle import oracle as orc
    orc.cg(lambda v: Ad.dot(v), b, rtol=1e-8, M=lambda v: Md.dot(v), callback=lambda xk: o1.append(1))
    orc.cg(lambda v: Ad.dot(v), b, rtol=1e-8, M=lambda v: M2d.dot(v), callback=lambda xk: o2.append(1))
    assert i1 == 0 and i2 == 0 and len(n1) == len(o1) and len(n2) == len(o2)
    assert rel_l2(x2, x1) < 1e-6
    # M2 maps the deflated eigenvalues of M_BD A to exactly 1.  That helps when they are the
    # SMALL end of the spectrum and 1 lies inside or above the rest; it does not when the whole
    # spectrum of M_BD A lies above 1, as for the reference's test problem with pol = 2 (band
    # diagonal 1 + 0.5 u > 1, no hit-count normalisation of the QU block: spectrum in
    # [1.43, 1.56], M2 adds an eigenvalue at 1.0 and the condition number goes from 1.09 to 1.56;
    # the CPU recurrence needs 6 steps against 5 as well).  So "M2 never needs more steps" is
    # asserted exactly where the theory gives it.
    lam_mbd = np.sort(np.linalg.eigvals(Md.dot(Ad)).real)
    if lam_mbd[r - 1] <= 1.0 <= lam_mbd[-1]:
        assert len(n2) <= len(n1), (len(n1), len(n2))
    else:
        assert lam_mbd[0] > 1.0 and len(n2) <= len(n1) + 1, (lam_mbd[0], len(n1), len(n2))


# ------------------------------------------------------------- f1: FilterLO -------
def _golden_filter_args(golden):
    ss = [[golden["filt_subscan0"], golden["filt_subscan1"]],
          [golden["filt_tstart0"], golden["filt_tstart1"]]]
    return ss, [int(x) for x in golden["filt_nsamples"]], [int(x) for x in golden["filt_nbolos"]]


def _structural_zeros(oracle, nt, pix, ss, ns, nb, order):
    """Samples the filter must leave at exactly 0 (gaps, skipped chunks, flagged samples of
    the Legendre fit): those at 0 for two unrelated inputs."""
    z = np.ones(nt, dtype=bool)
    for seed in (1, 2):
        x = np.random.default_rng(seed).standard_normal(nt) + 10.0
        f = (oracle.filter_mean(x, pix, ss, ns, nb) if order == 0 else
             oracle.filter_poly(x, pix, ss, ns, nb, order))
        z &= f == 0
    return z


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_filter_lo_against_reference_vectors(cm, oracle, golden, order):
    ss, ns, nb = _golden_filter_args(golden)
    d, pix = golden["filt_d"], golden["filt_pix"]
    F = cm.I.FilterLO(d.size, ss, ns, nb, pix, poly_order=order)
    y = F * d
    if order == 0:
        ref = oracle.filter_mean(d, pix, ss, ns, nb)        # weave loop: oracle only
    else:
        ref = golden["filt_out%d" % order]                  # the reference's polyfilter output
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-13 * np.abs(d).max())
    assert not y[_structural_zeros(oracle, d.size, pix, ss, ns, nb, order)].any()
    assert F.filter_info()["nchunks"] == 20
    if order:
        np.testing.assert_array_equal(F.legendres[40], oracle.get_legendre_polynomials(order, 40))
        np.testing.assert_allclose(F.mult(d), oracle.filter_mean(d, pix, ss, ns, nb), atol=1e-12)


def _random_scan(rng, nces, lo=150, hi=900):
    subs, ts, ns, nb = [], [], [], []
    for _ in range(nces):
        nsub = int(rng.integers(5, 40))
        sizes = rng.integers(lo, hi, size=nsub)
        gaps = rng.integers(0, 60, size=nsub)
        starts = np.cumsum(gaps + np.concatenate([[0], sizes[:-1]]))
        subs.append(sizes)
        ts.append(starts)
        ns.append(int(starts[-1] + sizes[-1] + rng.integers(0, 50)))
        nb.append(int(rng.integers(2, 9)))
    return subs, ts, ns, nb


@pytest.mark.parametrize("order", [0, 1, 3, 7])
def test_filter_lo_random_scans(cm, oracle, order):
    rng = np.random.default_rng(100 + order)
    subs, ts, ns, nb = _random_scan(rng, 6)
    nt = int(sum(a * b for a, b in zip(ns, nb)))
    pix = rng.integers(0, 1000, size=nt).astype(np.int32)
    pix[rng.random(nt) < 0.1] = -1
    blk = rng.integers(0, nt - 3000)
    pix[blk:blk + 3000] = -1                               # a long flagged stretch
    d = rng.standard_normal(nt) + 3.0 + 1e-3 * np.arange(nt)
    F = cm.I.FilterLO(nt, [subs, ts], ns, nb, pix, poly_order=order)
    ref = (oracle.filter_mean(d, pix, [subs, ts], ns, nb) if order == 0 else
           oracle.filter_poly(d, pix, [subs, ts], ns, nb, order))
    y = F * d
    # Chunk by chunk: the reference orthonormalises legendres[unflagged] by QR, whose span is
    # accurate to cond * eps; the kernel's recurrence basis is orthonormal to rounding.  So the
    # two agree to ~1e-14 * cond relative to the chunk's input (which rides on an offset + ramp
    # of ~400 that the filter removes), and to 1e-14 where no flag or no inverse is involved.
    starts, lens = oracle.filter_segments(*oracle.filter_normalise_args([subs, ts], ns, nb))
    worst = 0.0
    for a, n in zip(starts, lens):
        m = pix[a:a + n] >= 0
        cond = 1.0
        if order and order < m.sum() < n:
            cond = np.linalg.cond(oracle.get_legendre_polynomials(order, int(n))[m])
        err = np.linalg.norm(y[a:a + n] - ref[a:a + n])
        worst = max(worst, err / (1e-14 * cond * np.linalg.norm(d[a:a + n])))
    assert worst < 20.0, worst
    assert not y[_structural_zeros(oracle, nt, pix, [subs, ts], ns, nb, order)].any()
    # device-resident input -> device-resident output, identical numbers
    yd = F * cm.torch.from_numpy(d).cuda()
    assert yd.is_cuda
    np.testing.assert_array_equal(yd.cpu().numpy(), y)
    # filtering twice changes nothing where the basis is orthonormal on the kept samples
    if order == 0:
        assert rel_l2(F * y, y) < 1e-13


def test_filter_lo_conventions_and_errors(cm, oracle):
    from cosmomap2_amd._hip import HipError
    rng = np.random.default_rng(9)
    nt, ns, nb = 3000, 1000, 3
    pix = rng.integers(0, 50, size=nt).astype(np.int64)
    pix[::7] = -1
    d = rng.standard_normal(nt)
    sizes, starts = np.array([300, 250, 400]), np.array([10, 320, 590])
    # one CES given as scalars (:269-273), sub-scans listed out of order
    F = cm.I.FilterLO(nt, [sizes[::-1], starts[::-1]], ns, nb, pix, poly_order=2)
    ref = oracle.filter_poly(d, pix, [sizes, starts], ns, nb, 2)
    assert rel_l2(F * d, ref) < 1e-12
    # no chunk at all: everything is filtered to 0 (:130)
    F0 = cm.I.FilterLO(nt, [np.array([], dtype=int), np.array([], dtype=int)], ns, nb, pix)
    assert not (F0 * d).any()
    # zero-length and one-sample chunks; a chunk whose samples are all flagged
    p2 = pix.copy()
    p2[100:140] = -1
    F1 = cm.I.FilterLO(nt, [np.array([0, 1, 40, 5]), np.array([3, 50, 100, 200])], ns, nb, p2)
    np.testing.assert_allclose(F1 * d, oracle.filter_mean(
        d, p2, [np.array([0, 1, 40, 5]), np.array([3, 50, 100, 200])], ns, nb), atol=1e-14)
    with pytest.raises(HipError):                          # overlapping chunks
        cm.I.FilterLO(nt, [np.array([300, 300]), np.array([0, 200])], ns, nb, pix)
    with pytest.raises(Exception):                         # chunk past the end
        cm.I.FilterLO(nt, [np.array([300]), np.array([900])], ns, nb, pix)
    with pytest.raises(Exception):
        cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix[:-1])
    with pytest.raises(Exception):
        F * d[:-1]


def test_filter_lo_in_operator_products(cm, oracle):
    """Mbd * P.T * F * d as in the reference's src/test_poly.py:121-140."""
    rng = np.random.default_rng(21)
    pol, npix, ns, nb = 3, 300, 4000, 5
    nt = ns * nb
    d, pairs, phi, t, diag = make_problem(oracle, 77, nt, npix, nb, pol, flag_frac=0.05)
    sizes, starts = np.array([900, 950, 1000, 1000]), np.array([20, 940, 1900, 2950])
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi)
    CES = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    n2 = CES.get_new_pixel[0]
    P = cm.I.SparseLO(n2, nt, pairs, pol=pol, angle_processed=CES)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(CES, n2, pol)
    F1 = cm.I.FilterLO(nt, [sizes, starts], ns, nb, P.pairs, poly_order=1)
    m = Mbd * P.T * F1 * d
    fd = oracle.filter_poly(d, po, [sizes, starts], ns, nb, 1)
    ref = oracle.bd_precond_mult(pol, ro, oracle.sparse_rmult(pol, ro.new_npix, po, ro.cos,
                                                              ro.sin, fd))
    assert rel_l2(m, ref) < 1e-12


def test_filter_lo_full_size_properties(cm):
    """2e7 samples, 40000 chunks: zero mean of the kept samples in every chunk, flagged samples
    and gaps at 0, linearity, and F(F d) = F d for the QR-orthonormalised chunks."""
    torch = cm.torch
    rng = np.random.default_rng(1)
    ns, nb, L = 100000, 200, 500
    nt = ns * nb
    starts = np.arange(0, ns, L)
    sizes = np.full(starts.size, L - 10)                   # a 10-sample gap after every chunk
    pix = rng.integers(0, 1 << 20, size=nt).astype(np.int32)
    pix[rng.random(nt) < 0.08] = -1
    d = torch.from_numpy(rng.standard_normal(nt) + 5.0).cuda()
    e = torch.from_numpy(rng.standard_normal(nt)).cuda()
    valid = torch.from_numpy(pix >= 0).cuda()
    F0 = cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix, poly_order=0)
    F2 = cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix, poly_order=2)
    y0, y2 = F0 * d, F2 * d
    gaps = torch.ones(nt, dtype=torch.bool, device="cuda").view(-1, L)
    gaps[:, :L - 10] = False
    assert not y0.view(-1, L)[gaps].any() and not y2.view(-1, L)[gaps].any()
    assert not y2[~valid].any()
    kept = torch.where(valid, y0, torch.zeros_like(y0)).view(-1, L).sum(dim=1)
    assert kept.abs().max().item() < 1e-10
    kept2 = torch.where(valid, y2, torch.zeros_like(y2)).view(-1, L).sum(dim=1)
    assert kept2.abs().max().item() < 1e-10                # order >= 0 removes the offset too
    lin = F2 * (d + 0.5 * e)
    assert (lin - y2 - 0.5 * (F2 * e)).abs().max().item() < 1e-11
    assert (F2 * y2 - y2).abs().max().item() < 1e-11       # every chunk here has flags -> Q Q^T
    assert (F0 * y0 - y0).abs().max().item() < 1e-12


# -------------------------------------------------------- f2: GroundFilterLO ------
@pytest.mark.parametrize("nbins", [400, 9000])           # LDS histogram / pixel-major P^T
def test_ground_filter_lo(cm, nbins):
    from oracle import oracle as O
    rng = np.random.default_rng(4)
    nt = 200000
    g = rng.integers(-1, nbins, size=nt)
    g[g == 17] = 18                                        # an empty bin -> 1/0 guarded (:788-790)
    g[-1] = nbins - 1
    v = rng.standard_normal(nt)
    Fg = cm.I.GroundFilterLO(g)
    assert Fg.nbins == nbins and Fg.n == nt
    ref = O.ground_filter(g, v)
    y = Fg * v
    assert rel_l2(y, ref) < 1e-13
    np.testing.assert_array_equal(y[g == -1], v[g == -1])
    assert rel_l2(Fg.Pg * v, v - ref) < 1e-12              # the explicit product of :57
    np.testing.assert_array_equal(Fg.counts_in_groundbins(g),
                                  np.bincount(g[g >= 0], minlength=nbins).astype(float))
    yd = Fg * cm.torch.from_numpy(v).cuda()
    assert rel_l2(yd.cpu().numpy(), y) < 1e-14             # atomic order differs run to run
    assert rel_l2(Fg * y, y) < 1e-12                       # projector


def test_pcg_with_filter_as_noise_operator(cm, oracle):
    """A = P^T F P, the operator of the production runs (src/test_M2_precond_onto_real_data.py:
    79-86): PCG with M_BD against the oracle's PCG on the oracle's operators."""
    pol, npix, ns, nb = 3, 400, 6000, 6
    nt = ns * nb
    d, pairs, phi, t, diag = make_problem(oracle, 5, nt, npix, nb, pol, flag_frac=0.04)
    sizes = np.array([1400, 1500, 1450, 1500])
    starts = np.array([0, 1440, 2980, 4470])
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=pol, phi=phi)
    CES = cm.U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    n = CES.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pairs, pol=pol, angle_processed=CES)
    M = cm.I.BlockDiagonalPreconditionerLO(CES, n, pol)
    for order in (0, 2):
        F = cm.I.FilterLO(nt, [sizes, starts], ns, nb, P.pairs, poly_order=order)
        A = P.T * F * P
        filt = ((lambda v: oracle.filter_mean(v, po, [sizes, starts], ns, nb)) if order == 0 else
                (lambda v: oracle.filter_poly(v, po, [sizes, starts], ns, nb, order)))

        def A_o(x):
            return oracle.sparse_rmult(pol, n, po, ro.cos, ro.sin,
                                       filt(oracle.sparse_mult(pol, po, ro.cos, ro.sin, x)))
        x = np.random.default_rng(order).standard_normal(pol * n)
        assert rel_l2(A * x, A_o(x)) < 1e-12
        xd = cm.torch.from_numpy(x).cuda()
        assert rel_l2((A * xd).cpu().numpy(), A_o(x)) < 1e-12       # stays in HBM
        b = P.T * F * d
        its, itso = [], []
        xs, info = cm.cg(A, b, M=M, rtol=1e-8, maxiter=200, callback=lambda xk: its.append(1))
        xo, info_o = oracle.cg(A_o, b, M=lambda v: oracle.bd_precond_mult(pol, ro, v), rtol=1e-8,
                               maxiter=200, callback=lambda xk: itso.append(1))
        assert info == 0 and info_o == 0
        assert len(its) == len(itso), (len(its), len(itso))    # identical iteration counts
        assert rel_l2(A * xs, b) < 1e-7


@pytest.mark.parametrize("tp,lam", [(2048, 40), (64, 40), (1024, 300), (2048, 1500), (512, 2049)])
def test_overlap_save_on_tile_order(cm, oracle, tp, lam):
    """The overlap-save kernel reaching the tile-ordered TOD through its three address-sorted
    lists per segment pair, for short and long bands, with flagged samples, ragged blocks whose
    last pair ends mid-window, a block shorter than one window, and tiles so small (64 pixels)
    that every sample is its own address run."""
    from types import SimpleNamespace
    from cosmomap2_amd.interfaces import linearoperators as L
    pol, nt, npix, nblk = 3, 240000, 70000, 5
    d, pairs, phi, t, diag = make_problem(oracle, 900 + lam, nt, npix, nblk, pol, flag_frac=0.07)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
    L._sparse_tiles(P, tile_pixels=tp, slice_samples=4096)
    sizes = [100000, 60000, 70000, 7000, 3000]
    kk = np.arange(lam)
    bands = [(1.0 + 0.1 * b) * np.exp(-kk / (lam / 4.0)) for b in range(nblk)]
    x = np.random.default_rng(1).standard_normal(pol * npix)
    Nf = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
    Nd = cm.I.BlockLO(sizes, bands, offdiag=True, method=(1 if lam <= 300 else 2))
    exact = P.T * (Nd * (P * x))
    assert rel_l2(L._TiledNormalLO(P, Nf) * x, exact) < 1e-12


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("lists", ["plain", "rc", "inv"])
@pytest.mark.parametrize("tp,lam,npix", [(1024, 300, 70000), (2048, 2049, 70000), (64, 40, 200000)])
def test_overlap_save_kernel_variants(cm, oracle, monkeypatch, lists, flat, tp, lam, npix):
    """Every instantiation of the overlap-save kernel the dispatcher can choose (list format
    CM2_OS_LISTS = plain | rc | inv; buffer descriptors, or flat addressing as for TOD buffers of 4 GB
    and more, CM2_OS_FLAT) on the tile order AND on the time order against the direct sum / rocFFT;
    the last case has 3125 tiles, more address runs per list than the run tables hold, where
    run-coding falls back to plain lists by itself."""
    from types import SimpleNamespace
    from cosmomap2_amd.interfaces import linearoperators as L
    kernel = "real32"
    monkeypatch.setenv("CM2_OS_LISTS", lists)
    if flat:
        monkeypatch.setenv("CM2_OS_FLAT", "1")
    pol, nt, nblk = 3, 240000, 5
    d, pairs, phi, t, diag = make_problem(oracle, 900 + lam, nt, npix, nblk, pol, flag_frac=0.07)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
    L._sparse_tiles(P, tile_pixels=tp, slice_samples=4096)
    sizes = [100000, 60000, 70000, 7000, 3000]
    kk = np.arange(lam)
    bands = [(1.0 + 0.1 * b) * np.exp(-kk / (lam / 4.0)) for b in range(nblk)]
    x = np.random.default_rng(1).standard_normal(pol * npix)
    Nf = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
    Nd = cm.I.BlockLO(sizes, bands, offdiag=True, method=(1 if lam <= 300 else 2))
    tod = P * x
    want = Nd * tod
    assert rel_l2(Nf * tod, want) < 1e-12                                  # time order
    exact = P.T * want
    assert rel_l2(L._TiledNormalLO(P, Nf) * x, exact) < 1e-12              # tile order
    info = Nf.tile_kernel_info()
    assert info["os_kernel"] == kernel
    many_tiles = npix // tp > 2048
    assert info["os_lists"] == ("plain" if lists == "plain" or many_tiles
                                else ("inverse run-coded" if lists == "inv" else "run-coded"))


def test_overlap_save_lists_built_in_chunks(cm, oracle, monkeypatch):
    """The address lists are sorted in chunks of at most 2^30 entries (hipCUB counts in int);
    with the chunk forced down to 3 segment pairs the operator must not change."""
    from types import SimpleNamespace
    from cosmomap2_amd.interfaces import linearoperators as L
    pol, nt, npix, nblk, lam = 3, 240000, 70000, 5, 300
    d, pairs, phi, t, diag = make_problem(oracle, 1234, nt, npix, nblk, pol, flag_frac=0.05)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    sizes = [100000, 60000, 70000, 7000, 3000]
    kk = np.arange(lam)
    bands = [(1.0 + 0.1 * b) * np.exp(-kk / (lam / 4.0)) for b in range(nblk)]
    x = np.random.default_rng(1).standard_normal(pol * npix)
    outs = []
    monkeypatch.setenv("CM2_OS_LIST_BUILD", "sort")
    for chunk in (None, "3"):
        if chunk:
            monkeypatch.setenv("CM2_OS_LIST_CHUNK_PAIRS", chunk)
        P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
        L._sparse_tiles(P, tile_pixels=1024, slice_samples=4096)
        Nf = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
        outs.append(np.asarray(L._TiledNormalLO(P, Nf) * x))
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("lists,tp", [("rc", 1024), ("plain", 1024), ("rc", 64), ("plain", 256)])
def test_overlap_save_lists_written_directly_equal_the_sorted_ones(cm, oracle, monkeypatch, lists, tp):
    """The address lists of the tile-order overlap-save kernel are written straight from the tile
    plan's offsets (k_real_lists: count / lowest address per tile, a scan, slot = base + address -
    lowest).  They must describe the same gather / scatter as the lists that come out of the
    segmented sort (CM2_OS_LIST_BUILD=sort): the operator is bit-identical, with flagged samples,
    ragged noise blocks shorter than a window, run-coded and plain lists, and more tiles (tp = 64:
    1094 tiles) than a window has samples per tile."""
    from types import SimpleNamespace
    from cosmomap2_amd.interfaces import linearoperators as L
    pol, nt, npix, nblk, lam = 3, 240000, 70000, 5, 300
    d, pairs, phi, t, diag = make_problem(oracle, 4321, nt, npix, nblk, pol, flag_frac=0.05)
    c, s = np.cos(2 * phi), np.sin(2 * phi)
    sizes = [100000, 60000, 70000, 7000, 3000]
    kk = np.arange(lam)
    bands = [(1.0 + 0.1 * b) * np.exp(-kk / (lam / 4.0)) for b in range(nblk)]
    x = np.random.default_rng(2).standard_normal(pol * npix)
    monkeypatch.setenv("CM2_OS_LISTS", lists)
    outs = []
    for build in ("direct", "sort"):
        monkeypatch.setenv("CM2_OS_LIST_BUILD", build)
        P = cm.I.SparseLO(npix, nt, pairs, pol=pol, angle_processed=SimpleNamespace(cos=c, sin=s))
        L._sparse_tiles(P, tile_pixels=tp, slice_samples=4096)
        Nf = cm.I.BlockLO(sizes, bands, offdiag=True, method=3)
        outs.append(np.asarray(L._TiledNormalLO(P, Nf) * x))
        assert Nf.tile_kernel_info()["os_lists"] == ("plain" if lists == "plain" else "run-coded")
    assert np.array_equal(outs[0], outs[1])
    Nd = cm.I.BlockLO(sizes, bands, offdiag=True, method=1)          # direct band sum
    tod = np.asarray(P * x)
    assert rel_l2(outs[0], np.asarray(P.T * (Nd * tod))) < 1e-12


def _full_size_toeplitz_properties(cm, nside, nt, nb, seed, two_level_rank=0):
    """Size-independent properties of P^T N^-1 P at a BASELINE configuration's full size
    (generated in HBM).  No oracle run at this size (the direct band sum is 2e11 multiply-adds
    per matvec on one core); instead: the tile-order chain with the register FFT against the
    time-order chain built from independent pieces (exact pixel-major P^T, rocFFT overlap-save),
    symmetry, positivity, linearity, run-to-run bit reproducibility, the zero boundary between
    noise blocks, and a PCG solve with M_BD checked through its true residual."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import toeplitz_band
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd import device as D
    t = cm.torch
    pol, lam = 3, 2048
    npix = 12 * nside * nside
    g = t.Generator(device="cuda").manual_seed(seed)
    pix = t.randint(0, npix, (nt,), generator=g, device="cuda", dtype=t.int32)
    phi = 0.3 + (2 * np.pi * 2.5 / 200.0) * t.arange(nt, device="cuda", dtype=t.float64)
    rng = np.random.default_rng(11)
    bands = [toeplitz_band(lam, rng) for _ in range(nb)]
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    del phi
    n = ces.get_new_pixel[0]
    # (>= 40 hits per pixel: at most a handful of pixels whose hits happen to share an angle fail
    # the condition-number test of process_ces.py:544-550 and are compacted away)
    assert npix - 8 <= n <= npix
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    Nf = cm.I.BlockLO(nt // nb, bands, offdiag=True, method=3)       # register / LDS FFT
    Nr = cm.I.BlockLO(nt // nb, bands, offdiag=True, method=2)       # rocFFT
    x = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64) - 0.5
    y = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64) - 0.5
    A = P.T * Nf * P
    assert L._use_tiles(P) and L._sparse_tiles(P).pt_fixed
    Ax = A * x
    assert t.equal(A * x, Ax)                             # fixed-order P^T: same bits every run
    exact = P.T * (Nr * (P * x))
    assert float((Ax - exact).norm() / exact.norm()) < 1e-12
    Ay = A * y
    dxy, dyx = D.dot(y, Ax), D.dot(x, Ay)
    assert abs(dxy - dyx) <= 1e-11 * abs(dxy)
    assert D.dot(x, Ax) > 0 and D.dot(y, Ay) > 0
    lin = A * (2.0 * x + y) - (2.0 * Ax + Ay)
    assert float(lin.norm() / Ax.norm()) < 1e-13
    del exact, lin
    # zero boundary: an impulse on the first sample of block 1 spreads lambda-1 samples
    # forward inside the block and not at all into block 0
    bs = nt // nb
    e = t.zeros(nt, dtype=t.float64, device="cuda")
    e[bs] = 1.0
    for Nop in (Nf, Nr):
        r = Nop * e
        assert float(r[:bs].abs().max()) == 0.0
        np.testing.assert_allclose(r[bs:bs + lam].cpu().numpy(), bands[1], rtol=0,
                                   atol=1e-12 * abs(bands[1][0]))
        assert float(r[bs + lam:bs + 3 * lam].abs().max()) < 1e-12 * abs(bands[1][0])
    del e, r
    # PCG to the metric's 1e-6 with M_BD: converged, true residual at the tolerance, and the
    # count reproducible (the bench prints this number for its own seed)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=pol)
    d = t.rand(nt, generator=g, device="cuda", dtype=t.float64)
    b = P.T * (Nf * d)
    its = []
    xs, info = cm.cg(A, b, M=M, rtol=1e-6, maxiter=200, callback=lambda v: its.append(1))
    assert info == 0 and 2 <= len(its) <= 30
    true_res = float((b - A * xs).norm() / b.norm())
    assert true_res < 2e-6, true_res
    its_b = []
    xs_b, _ = cm.cg(A, b, M=M, rtol=1e-6, maxiter=200, callback=lambda v: its_b.append(1))
    assert len(its_b) == len(its) and t.equal(xs_b, xs)
    # the same solve on the exact-order path (time-ordered gather, rocFFT overlap-save, pixel-major
    # P^T in the reference's order -- each piece tied to the oracle at sizes it can run): the
    # iteration count bench.py prints for this configuration is that path's count, strictly
    L.set_pointing_mode("exact")
    try:
        A_x = P.T * Nr * P
        assert not any(isinstance(op, L._TiledNormalLO) for op in A_x._compiled())
        b_x = P.T * (Nr * d)
        assert float((b_x - b).norm() / b.norm()) < 1e-12
        its_x = []
        xs_x, info_x = cm.cg(A_x, b_x, M=M, rtol=1e-6, maxiter=200, callback=lambda v: its_x.append(1))
        assert info_x == 0 and len(its_x) == len(its), (len(its_x), len(its))
        assert float((xs_x - xs).norm() / xs.norm()) < 1e-9
        del A_x, b_x, xs_x
    finally:
        L.set_pointing_mode("auto")
    if two_level_rank:
        # BASELINE C4: two-level preconditioner, Arnoldi-built deflation space of dimension 32;
        # its solution must be the M_BD one (1e-6) in no more iterations
        r = two_level_rank
        Z, theta, AZ = cm.I.ritz_deflation_basis(A, M, b, r, 96, with_AZ=True)
        AZx = cm.I.apply_to_columns(A, Z)              # the reference's r applications of A
        assert float((AZ - AZx).norm() / AZx.norm()) < 1e-9
        del AZx
        E = cm.I.CoarseLO(Z, AZ, r, apply='eig')
        M2 = cm.I.TwoLevelPreconditionerLO(M, cm.I.DeflationLO(Z), cm.I.DeflationLO(AZ), E)
        its2 = []
        x2, info2 = cm.cg(A, b, M=M2, rtol=1e-6, maxiter=200, callback=lambda v: its2.append(1))
        assert info2 == 0 and len(its2) <= len(its), (len(its2), len(its))
        assert float((x2 - xs).norm() / xs.norm()) < 1e-6
        assert float((b - A * x2).norm() / b.norm()) < 2e-6


def test_full_size_properties_c3(cm):
    """BASELINE config C3: nside 128 IQU, 1e8 samples, Toeplitz lambda 2048 (100 blocks)."""
    _full_size_toeplitz_properties(cm, 128, 100_000_000, 100, 20161205)


def test_full_size_properties_c4(cm):
    """BASELINE config C4 (one GPU's 1e8 samples): nside 256 IQU, lambda 2048, two-level
    preconditioner with an Arnoldi-built deflation space of dimension 32."""
    _full_size_toeplitz_properties(cm, 256, 100_000_000, 100, 20161204, two_level_rank=32)


def test_full_size_properties_c5_share(cm):
    """One GPU's share of BASELINE config C5: nside 512 IQU, 1.25e8 samples = 8 detector blocks
    of 15 625 000, lambda 2048, Toeplitz N^-1 + two-level preconditioner (deflation space of
    dimension 32), as BASELINE config 5 names it."""
    _full_size_toeplitz_properties(cm, 512, 125_000_000, 8, 20161206, two_level_rank=32)


def test_config_c1_reference_runnable_case(cm, oracle):
    """BASELINE configs[0]: nside 16, temperature only, 1e4 samples, N = I, block-diagonal
    preconditioner -- the case the reference itself runs on a CPU.  Whole solve on the GPU
    against the oracle's operators driven by the LOCAL scipy.sparse.linalg.cg (the solver the
    reference calls): same solution, same residual history, same iteration count; with M_BD
    (the exact inverse of the diagonal A = P^T P) one iteration."""
    import scipy.sparse.linalg as spla
    nside, nt, pol, nb = 16, 10000, 1, 10
    npix = 12 * nside * nside
    rng = np.random.default_rng(20161202)
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb)
    po = pairs.copy()
    ro = oracle.process_time_samples(po, npix, pol=pol)
    CES = cm.U.ProcessTimeSamples(pairs, npix, pol=pol)
    n = CES.get_new_pixel[0]
    assert n == ro.new_npix and n < npix                 # ~3 hits per pixel: some never seen
    np.testing.assert_array_equal(pairs, po)
    P = cm.I.SparseLO(n, nt, pairs, pol=pol)
    N = cm.I.BlockLO(nt // nb, [1.0] * nb)               # N = I
    M = cm.I.BlockDiagonalPreconditionerLO(CES, n, pol)
    A = P.T * N * P
    b = P.T * (N * d)
    A_o = spla.LinearOperator((n, n), dtype=np.float64, matvec=lambda x: oracle.sparse_rmult(
        pol, n, po, None, None, oracle.sparse_mult(pol, po, None, None, x)))
    M_o = spla.LinearOperator((n, n), dtype=np.float64,
                              matvec=lambda x: oracle.bd_precond_mult(pol, ro, x))
    b_o = oracle.sparse_rmult(pol, n, po, None, None, d)
    np.testing.assert_array_equal(b, b_o)
    # without preconditioner: CG needs one iteration per distinct hit count
    hist_g, hist_o = [], []
    xg, ig = cm.cg(A, b, rtol=1e-6, callback=lambda x: hist_g.append(np.linalg.norm(b - A * x)))
    xo, io = spla.cg(A_o, b_o, rtol=1e-6, callback=lambda x: hist_o.append(
        np.linalg.norm(b_o - A_o.matvec(x))))
    assert ig == 0 and io == 0 and len(hist_g) == len(hist_o) > 3
    np.testing.assert_allclose(hist_g, hist_o, rtol=1e-8, atol=1e-12 * np.linalg.norm(b))
    assert rel_l2(xg, xo) < 1e-10
    # with M_BD: one iteration, map = hit-weighted mean of the samples per pixel
    its = []
    xm, im = cm.cg(A, b, M=M, rtol=1e-6, callback=lambda x: its.append(1))
    xs, i_s = spla.cg(A_o, b_o, M=M_o, rtol=1e-6)
    assert im == 0 and i_s == 0 and len(its) == 1
    assert rel_l2(xm, xs) < 1e-12
    binned = np.bincount(po[po >= 0], weights=d[po >= 0], minlength=n) / np.bincount(
        po[po >= 0], minlength=n)
    assert rel_l2(xm, binned) < 1e-12


# ----------------------------------------------- f3: map vector <-> full-sky maps ------
@pytest.mark.parametrize("pol", [1, 2, 3])
def test_map_reorganisation(cm, oracle, golden, pol):
    obs, full = golden["cut_obspix"], list(golden["cut_full"][:pol])
    res = cm.U.full2cutskymap(full, pol, obs.size, obs)
    assert isinstance(res, list) == (pol == 1)            # the reference's pol=1 quirk (:386-387)
    vec = res[0] if pol == 1 else res
    np.testing.assert_array_equal(vec, golden["cut_out%d" % pol])     # reference output
    maps = cm.U.reorganize_map(vec, obs, obs.size, 4, pol)
    ref = oracle.reorganize_map(vec, obs, obs.size, 4, pol)
    assert len(maps) == pol
    for a, b in zip(maps, ref):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(cm.U.obspix2mask(obs, 4), np.isin(np.arange(192), obs) * 1.0)
    # a real-size map, HBM-resident in and out, unordered pixel list
    rng = np.random.default_rng(pol)
    nside = 128
    nfull = 12 * nside * nside
    obs2 = rng.permutation(nfull)[:150000]
    x = rng.standard_normal(pol * obs2.size)
    xd = cm.torch.from_numpy(x).cuda()
    md = cm.U.reorganize_map(xd, cm.torch.from_numpy(obs2).cuda(), obs2.size, nside, pol)
    assert all(m.is_cuda and m.numel() == nfull for m in md)
    for a, b in zip(md, oracle.reorganize_map(x, obs2, obs2.size, nside, pol)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    back = cm.U.full2cutskymap(md, pol, obs2.size, obs2)
    back = back[0] if pol == 1 else back
    np.testing.assert_array_equal(back.cpu().numpy(), x)
    with pytest.raises(Exception):                        # pixel id outside the sky
        cm.U.reorganize_map(x, obs2 + nfull, obs2.size, nside, pol)
    # fname: the maps also go to a HEALPix FITS file (hp.write_map of the reference, :103, :46)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, "map.fits")
        maps = cm.U.reorganize_map(x, obs2, obs2.size, nside, pol, fname=fn)
        got = cm.U.read_map(fn, field=None)
        assert len(got) == pol
        for a, b in zip(got, maps):
            np.testing.assert_array_equal(a, b.astype(np.float32).astype(np.float64))
        # ... and read back they give the cut-sky vector again (to the file's float32)
        back = cm.U.full2cutskymap(got, pol, obs2.size, obs2)
        back = back[0] if pol == 1 else back
        np.testing.assert_allclose(back, x, rtol=1e-6, atol=1e-7)
        fm = os.path.join(tmp, "mask.fits")
        mask = cm.U.obspix2mask(obs2, nside, fname=fm)
        np.testing.assert_array_equal(cm.U.read_map(fm), mask)


def test_reference_api_surface(cm, oracle):
    """Constructor signatures and attributes the reference's drivers and tests rely on
    (SURVEY 8b "constructor signatures to keep"), and scipy's eigsh / cg driving the operators
    through the linop protocol."""
    import scipy.sparse.linalg as spla
    import cosmomap2_amd
    I, U = cm.I, cm.U
    rng = np.random.default_rng(0)
    nt, npix, nb, pol = 6000, 60, 3, 3
    d, pairs, phi, t, diag = oracle.system_setup(rng, nt, npix, nb)
    t = [np.array([1.0 + ti[0], 0.3 * ti[1]]) for ti in t]            # SPD two-lag bands

    def has(obj, names):
        missing = [a for a in names.split() if not hasattr(obj, a)]
        assert not missing, (type(obj).__name__, missing)

    CES = U.ProcessTimeSamples(pairs, npix, pol=pol, phi=phi)
    has(CES, "counts cosine sine cos2 sin2 sincos cos sin mask old2new obspix nsamples oldnpix")
    n, obspix = CES.get_new_pixel
    P = I.SparseLO(n, nt, pairs, pol=pol, angle_processed=CES)
    has(P, "ncols nrows pol pairs cos sin maptype shape T H matvec dtype symmetric")
    has(I.ToeplitzLO(np.array([1.0, 0.2]), 100), "array shape")
    N = I.BlockLO(nt // nb, t, offdiag=True)
    has(N, "blocksize covnoise blocklist diag isoffdiag")
    has(I.BlockLO(nt // nb, diag), "blocksize covnoise blocklist diag isoffdiag")
    M = I.BlockDiagonalPreconditionerLO(CES, n, pol)
    has(M, "counts cos sin cos2 sin2 sincos size pol")
    A = P.T * N * P
    has(I.InverseLO(A, method=cosmomap2_amd.cg, preconditioner=M), "method converged preconditioner")
    w, Z = spla.eigsh(A, k=4, which='SM', tol=1e-8, ncv=40)          # as tests/test_coarse_operator.py:29
    AZ = np.column_stack([A * Z[:, j] for j in range(4)])
    Zd = I.DeflationLO(Z)
    has(Zd, "z nrows ncols")
    has(I.CoarseLO(Z, AZ, 4), "L U")
    E = I.CoarseLO(Z, AZ, 4, apply='eig')
    has(E, "invE")
    assert (Zd.T * Zd).to_array().shape == (4, 4)
    R = I.lp.IdentityOperator(pol * n) - A * Zd * E * Zd.T           # test_2level_preconditioner.py:45-46
    M2 = M * R + Zd * E * Zd.T
    b = P.T * N * d
    x1, info1 = spla.cg(A, b, M=M, rtol=1e-8)
    x2, info2 = spla.cg(A, b, M=M2, rtol=1e-8)
    assert info1 == 0 and info2 == 0 and rel_l2(x2, x1) < 1e-6


def test_throughput_path_equals_exact_path_end_to_end(cm):
    """The whole solve on the throughput path (tile order, half-angle storage, fixed-order P^T,
    register-resident FFT) against the exact path (time order, fixed-order P^T, direct band
    sum = the oracle's arithmetic): same PCG iteration count, maps equal far below the
    north_star's 1e-6."""
    from cosmomap2_amd.interfaces import linearoperators as L
    t = cm.torch
    nside, nt, nb, pol, lam = 64, 4_000_000, 40, 3, 700
    npix = 12 * nside * nside
    g = t.Generator(device="cuda").manual_seed(3)
    pix = t.randint(0, npix, (nt,), generator=g, device="cuda", dtype=t.int32)
    pix[t.rand(nt, generator=g, device="cuda") < 0.02] = -1
    phi = 0.9 + (2 * np.pi * 2.5 / 200.0) * t.arange(nt, device="cuda", dtype=t.float64)
    d = t.rand(nt, generator=g, device="cuda", dtype=t.float64)
    kk = np.arange(lam)
    bands = [(1.0 + 0.02 * b) * np.where(kk == 0, 1.0, 0.25 * np.exp(-kk / 200.0)) for b in range(nb)]
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol)
    sols = {}
    for mode, method in (("exact", 1), ("tiled", 3)):
        L.set_pointing_mode(mode)
        try:
            N = cm.I.BlockLO(nt // nb, bands, offdiag=True, method=method)
            A = P.T * N * P
            b = P.T * (N * d)
            its = []
            x, info = cm.cg(A, b, M=M, rtol=1e-9, maxiter=300, callback=lambda v: its.append(1))
            assert info == 0
            sols[mode] = (x, len(its))
        finally:
            L.set_pointing_mode("auto")
    (xe, ie), (xt, it) = sols["exact"], sols["tiled"]
    assert ie == it, (ie, it)
    assert float((xt - xe).norm() / xe.norm()) < 1e-8


def test_filter_chain_on_tile_order(cm):
    """A = P^T F P (and the ground filter likewise) above 2^20 samples runs on the tile order
    around the time-order filter; it must equal the exact-order chain to rounding."""
    from cosmomap2_amd.interfaces import linearoperators as L
    t = cm.torch
    nside, ns, nb, pol = 32, 150000, 10, 3
    nt = ns * nb
    npix = 12 * nside * nside
    g = t.Generator(device="cuda").manual_seed(5)
    pix = t.randint(0, npix, (nt,), generator=g, device="cuda", dtype=t.int32)
    pix[t.rand(nt, generator=g, device="cuda") < 0.04] = -1
    phi = 0.2 + (2 * np.pi * 2.5 / 200.0) * t.arange(nt, device="cuda", dtype=t.float64)
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    starts = np.arange(0, ns - 1500 + 1, 1540)
    sizes = np.full(starts.size, 1500)
    x = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64) - 0.5
    az = ((t.arange(nt, device="cuda") % 3080) - 1540).abs().to(t.int32)
    tiny_starts = np.arange(0, ns - 100, 100)
    ops = [cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix, poly_order=0),
           cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix, poly_order=2),
           # chunks longer than the 8192-sample window: the chain goes through the time order
           cm.I.FilterLO(nt, [np.array([9000, 20000]), np.array([100, 30000])], ns, nb, pix, poly_order=1),
           # two short chunks per detector pair, long stretches outside any chunk (-> 0)
           cm.I.FilterLO(nt, [np.array([700, 900]), np.array([5000, 120000])], ns, nb, pix, poly_order=3),
           # 1500 chunks of 90 samples per pair
           cm.I.FilterLO(nt, [np.full(tiny_starts.size, 90), tiny_starts], ns, nb, pix, poly_order=1),
           cm.I.GroundFilterLO(az),
           # more bins than the LDS histogram holds: binning through the pixel-major P^T
           cm.I.GroundFilterLO(t.randint(0, 9000, (nt,), generator=g, device="cuda", dtype=t.int32))]
    for F in ops:
        res = {}
        for mode in ("exact", "tiled"):
            L.set_pointing_mode(mode)
            try:
                A = P.T * F * P
                res[mode] = A * x
                plan = A._compiled()
                assert (len(plan) == 1 and isinstance(plan[0], L._TiledNormalLO)) == (mode == "tiled")
            finally:
                L.set_pointing_mode("auto")
        err = float((res["tiled"] - res["exact"]).norm() / res["exact"].norm())
        assert err < 1e-12, (type(F).__name__, err)
    # a filter whose flags differ from the pointing's stays on the time order (same numbers)
    pix2 = pix.clone()
    pix2[::1000] = -1
    F2 = cm.I.FilterLO(nt, [sizes, starts], ns, nb, pix2, poly_order=1)
    L.set_pointing_mode("tiled")
    try:
        A2 = P.T * F2 * P
        y2 = A2 * x
        assert not any(isinstance(op, L._TiledNormalLO) for op in A2._compiled())
    finally:
        L.set_pointing_mode("auto")
    ref2 = P.T * (F2 * (P * x))
    assert float((y2 - ref2).norm() / ref2.norm()) < 1e-13


@pytest.mark.parametrize("nt,npix,pol", [(5000, 300, 3), (900, 40, 2), (8191, 100, 1), (8193, 100, 3)])
def test_small_problems_forced_onto_the_tile_path(cm, nt, npix, pol):
    """Sizes around and below one 8192-sample window, every kind of operator between P^T and
    P (fused and direct Toeplitz, sub-scan filter, ground filter): tile path == exact path."""
    from cosmomap2_amd.interfaces import linearoperators as L
    rng = np.random.default_rng(nt)
    pix = rng.integers(0, npix, nt).astype(np.int32)
    pix[rng.random(nt) < 0.05] = -1
    phi = rng.random(nt)
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    x = rng.standard_normal(pol * n)
    lam = 30
    bands = [np.where(np.arange(lam) == 0, 1.0, 0.1 * np.exp(-np.arange(lam) / 5.0))]
    ops = [cm.I.BlockLO(nt, bands, offdiag=True, method=3),
           cm.I.BlockLO(nt, bands, offdiag=True, method=1),
           cm.I.FilterLO(nt, [np.array([nt // 3, nt // 3]), np.array([5, nt // 2])], nt, 1, pix,
                         poly_order=1),
           cm.I.GroundFilterLO(rng.integers(-1, 20, nt))]
    for op in ops:
        res = {}
        for mode in ("exact", "tiled"):
            L.set_pointing_mode(mode)
            try:
                res[mode] = (P.T * op * P) * x
            finally:
                L.set_pointing_mode("auto")
        assert rel_l2(res["tiled"], res["exact"]) < 1e-13, type(op).__name__


@pytest.mark.parametrize("lam", [2, 33, 200])
def test_default_method_noise_on_tile_order(cm, lam):
    """BlockLO(..., offdiag=True) with the method left to the library: the direct sum (short
    band) or the fused kernel on the time order, the fused overlap-save kernel on the tile
    order whatever the band length; the product P^T N P must agree on the two paths."""
    from cosmomap2_amd.interfaces import linearoperators as L
    t = cm.torch
    nside, nt, nb, pol = 32, 1_200_000, 8, 3
    npix = 12 * nside * nside
    g = t.Generator(device="cuda").manual_seed(lam)
    pix = t.randint(0, npix, (nt,), generator=g, device="cuda", dtype=t.int32)
    phi = 0.3 + 0.0785 * t.arange(nt, device="cuda", dtype=t.float64)
    ces = cm.U.ProcessTimeSamples(pix, npix, pol=pol, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pix, pol=pol, angle_processed=ces)
    kk = np.arange(lam)
    bands = [np.where(kk == 0, 1.0, 0.2 * np.exp(-kk / 10.0)) for _ in range(nb)]
    N = cm.I.BlockLO(nt // nb, bands, offdiag=True)                  # method = AUTO
    info = N.noise_info()
    assert info["method"] == (1 if lam <= 32 else 3) and info["tiles_ok"]
    x = t.rand(pol * n, generator=g, device="cuda", dtype=t.float64) - 0.5
    res = {}
    for mode in ("exact", "tiled"):
        L.set_pointing_mode(mode)
        try:
            A = P.T * N * P
            res[mode] = A * x
        finally:
            L.set_pointing_mode("auto")
    assert float((res["tiled"] - res["exact"]).norm() / res["exact"].norm()) < 1e-12
