"""
The offset prior on the GPU (cm2_offset_prior.hip, cosmomap2_amd/utilities/offset_prior.py) against the restatement
in np.longdouble of _offset_prior_ref.py, within the forward error bound derived there, and end to end in a destriping
solve on the common case of _destriper_ref.py.

Inputs: nperseg 256 with L = 1 (K = 129, M = 512, lam = 256), L = 3 (K = 43, M = 128, lam = 64), L = 37 (K = 3, M = 8,
lam = 4 and 1) and L = 64 (K = 2, M = 4, lam = 2); nperseg 1024 with L = 37 (K = 13, M = 32, lam = 16).  As PSDs the
Welch PSD of seeded 1/f noise and of seeded white noise, the analytic flat PSD (every bin floored) and an analytic PSD
whose correlated part is zero above n/8; the white variance given and estimated.  The references are computed once
and shared.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _destriper_ref as DR
import _offset_prior_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

PSD_NAMES = ("welch_1f", "welch_white", "flat", "band_limited")
RTOL, OP_TOL = 1e-10, 1e-12
_DBLP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd.utilities import offset_prior
    return SimpleNamespace(I=I, U=U, L=L, D=D, hip=_hip, op=offset_prior, torch=torch)


_inputs, _refs = {}, {}


def inputs(n):
    if n not in _inputs:
        _inputs[n] = R.psd_inputs(n)
    return _inputs[n]


def reference(n, L, lam, name, given):
    key = (n, L, lam, name, given)
    if key not in _refs:
        row, s2 = inputs(n)[name]
        _refs[key] = R.prior(row, L, lam, sigma2=s2 if given else None, bound=True)
    return _refs[key]


def share(got, ref):
    """Largest |got - ref| / bound over the band, and the same for sigma^2."""
    eb = float((np.abs(np.asarray(got[0], dtype=R.LD) - ref.band) / ref.band_err).max())
    es = float(abs(R.LD(got[1]) - ref.sigma2) / ref.sigma2_err)
    return eb, es


# ------------------------------------------------------------- 1: bands and sigma^2 within the bound ------
@pytest.mark.parametrize("n,L,lam", R.GEOMETRIES)
def test_bands_and_white_level_within_the_derived_bound(cm, n, L, lam):
    worst = 0.0
    for given in (False, True):
        psd = np.array([inputs(n)[name][0] for name in PSD_NAMES])
        s_in = [inputs(n)[name][1] for name in PSD_NAMES] if given else None
        bands, sigma2 = cm.op.offset_prior_bands(psd, L, lam, sigma2=s_in)
        assert isinstance(bands, np.ndarray) and bands.shape == (4, lam) and sigma2.shape == (4,)
        dev_bands, dev_sigma2 = cm.op.offset_prior_bands(cm.D.f64(psd), L, lam, sigma2=s_in)
        assert dev_bands.is_cuda and dev_sigma2.is_cuda and tuple(dev_bands.shape) == (4, lam)
        np.testing.assert_array_equal(cm.D.to_host(dev_bands), bands)
        np.testing.assert_array_equal(cm.D.to_host(dev_sigma2), sigma2)
        for b, name in enumerate(PSD_NAMES):
            ref = reference(n, L, lam, name, given)
            eb, es = share((bands[b], sigma2[b]), ref)
            print("\nn %d L %d lam %d %s sigma2 %s: band error %.3g of the bound, sigma2 error %.3g of its bound"
                  % (n, L, lam, name, "given" if given else "estimated", eb, es))
            assert eb <= 1.0 and es <= 1.0, (name, given, eb, es)
            if given:
                assert sigma2[b] == s_in[b]
            worst = max(worst, eb)
            if name == "flat":                               # the closed form: L / (floor sigma^2) on the diagonal
                want = np.zeros(lam, dtype=R.LD)
                want[0] = R.LD(L) / (R.LD(np.float64(1e-6)) * R.LD(2.5))
                assert sigma2[b] == 2.5
                assert np.all(np.abs(bands[b].astype(R.LD) - want) <= ref.band_err)
    print("\nn %d L %d lam %d: largest band error %.3g of the bound" % (n, L, lam, worst))


def test_fsample_and_floor_reach_the_kernels(cm):
    """fs = 200: the PSD row scales by 1 / fs and S does not; floor = 0.25 changes the floored bins only."""
    n, L, lam = 256, 37, 4
    row, s2 = R.psd_inputs(n, fs=200.0)["welch_white"]
    for floor in (1e-6, 0.25):
        ref = R.prior(row, L, lam, fs=200.0, floor=floor, bound=True)
        bands, sigma2 = cm.op.offset_prior_bands(row[None, :], L, lam, fsample=200.0, floor=floor)
        eb, es = share((bands[0], sigma2[0]), ref)
        assert eb <= 1.0 and es <= 1.0, (floor, eb, es)
        assert abs(sigma2[0] / s2 - 1.0) < 0.1


# --------------------------------------------------------------- 2: blocks do not see each other ------
@pytest.mark.parametrize("n,L,lam", [(256, 1, 256), (256, 37, 4), (1024, 37, 16)])
def test_three_blocks_are_bit_equal_to_each_block_alone(cm, n, L, lam):
    """White levels 1.1, 2.6 and 40 (the 1/f row scaled by 40) in one call."""
    rows = inputs(n)
    psd = np.array([rows["welch_1f"][0], rows["welch_white"][0], 40.0 * rows["welch_1f"][0]])
    for s_in in (None, [1.0, 2.5, 40.0]):
        bands, sigma2 = cm.op.offset_prior_bands(psd, L, lam, sigma2=s_in)
        assert sigma2[0] < sigma2[1] < sigma2[2]
        again = cm.op.offset_prior_bands(psd, L, lam, sigma2=s_in)
        np.testing.assert_array_equal(again[0], bands)
        for b in range(3):
            alone = cm.op.offset_prior_bands(psd[b:b + 1], L, lam, sigma2=None if s_in is None else s_in[b])
            np.testing.assert_array_equal(alone[0][0], bands[b])
            np.testing.assert_array_equal(alone[1][0], sigma2[b])
        ref = R.prior(psd[2], L, lam, sigma2=None if s_in is None else 40.0, bound=True)
        eb, es = share((bands[2], sigma2[2]), ref)
        assert eb <= 1.0 and es <= 1.0, (eb, es)


# ------------------------------------------------------------------------------------ 3: refusals ------
def raw_call(cm, psd, nb, n, fs, L, lam, s_in, floor, bands, s_out):
    lib = cm.hip.load()
    rc = lib.cm2_offset_prior_from_psd(cm.D.ptr(psd), nb, n, fs, L, lam, s_in, floor, cm.D.ptr(bands), s_out,
                                       cm.D.stream())
    return rc, lib.cm2_last_error()


def test_bad_bin_in_block_1_names_the_block_and_the_bin(cm):
    n, L, lam = 256, 37, 4
    rows = inputs(n)
    for value in (0.0, -3.0, np.nan, np.inf):
        psd = np.array([rows["welch_1f"][0], rows["welch_white"][0], rows["band_limited"][0]])
        psd[1, 77] = value
        psd[2, 5] = value
        d_psd, bands = cm.D.f64(psd), cm.D.empty(3 * lam)
        rc, msg = raw_call(cm, d_psd, 3, n, 1.0, L, lam, None, 1e-6, bands, None)
        assert rc == cm.hip.ERR_ARGUMENT, (rc, msg)
        assert b"block 1 " in msg and b"bin 77 " in msg, msg
        with pytest.raises(ValueError, match=r"block 1\b.*bin 77\b"):
            cm.op.offset_prior_bands(d_psd, L, lam)
        with pytest.raises(ValueError, match=r"block 1\b.*bin 77\b"):
            cm.op.offset_prior_bands(psd, L, lam)
    psd = np.array([rows["welch_1f"][0]] * 2)
    psd[:, 0] = np.nan                                       # the DC bin is not used
    bands, sigma2 = cm.op.offset_prior_bands(cm.D.f64(psd), L, lam)
    assert np.all(np.isfinite(cm.D.to_host(bands))) and np.all(np.isfinite(cm.D.to_host(sigma2)))


def test_the_library_refuses_bad_arguments(cm):
    n, lam = 256, 4
    psd, bands = cm.D.f64(np.ones((2, n // 2 + 1))), cm.D.f64(np.full(2 * 4, 7.0))
    two = (ctypes.c_double * 2)
    s_out = two(-1.0, -1.0)
    for args, word in (((2, n, 1.0, 65, 1, None, 1e-6), b"smallest nperseg that would do is 512"),
                       ((2, n, 1.0, 37, 5, None, 1e-6), b"lambda=5"),
                       ((2, n, 1.0, 37, 0, None, 1e-6), b"lambda=0"),
                       ((2, n, 1.0, 37, lam, None, 0.0), b"floor"),
                       ((2, n, 1.0, 37, lam, None, 1.5), b"floor"),
                       ((2, n, 1.0, 37, lam, None, float("nan")), b"floor"),
                       ((2, n, 1.0, 37, lam, two(1.0, 0.0), 1e-6), b"sigma2 of block 1"),
                       ((2, n, 1.0, 37, lam, two(np.inf, 1.0), 1e-6), b"sigma2 of block 0"),
                       ((2, n, 0.0, 37, lam, None, 1e-6), b"fsample"),
                       ((2, 300, 1.0, 37, lam, None, 1e-6), b"nperseg"),
                       ((0, n, 1.0, 37, lam, None, 1e-6), b"nb="),
                       ((2, n, 1.0, 0, lam, None, 1e-6), b"baseline_length")):
        nb, nn, fs, L, la, s_in, floor = args
        rc, msg = raw_call(cm, psd, nb, nn, fs, L, la, s_in, floor, bands, s_out)
        assert rc == cm.hip.ERR_ARGUMENT and b"cm2_offset_prior_from_psd" in msg and word in msg, (args, rc, msg)
    assert list(s_out) == [-1.0, -1.0]
    np.testing.assert_array_equal(cm.D.to_host(bands), np.full(8, 7.0))         # nothing was written
    rc, msg = raw_call(cm, psd, 2, n, 1.0, 37, lam, two(1.0, 2.0), 1e-6, bands, s_out)
    assert rc == 0 and list(s_out) == [1.0, 2.0]
    rc, msg = raw_call(cm, psd, 2, n, 1.0, 37, lam, None, 1e-6, bands, None)    # h_sigma2_out may be NULL
    assert rc == 0


# ---------------------------------------------------------------------------------- 4: end to end ------
_e2e = {}


def e2e_case(cm, pol):
    """The common case of _destriper_ref.py (nt = 34002 in blocks of 14000 and 20002, L = 37, nside 4) with 1/f noise
    (knee 0.05, slope 1.5) of white variance 1 and 0.4 from a fixed seed, the prior estimated from the residual of
    the unweighted binned map (zero on the flagged samples) with nperseg = 8192, and the dense system built from the
    same bands and weights."""
    if pol in _e2e:
        return _e2e[pol]
    nt, sizes, _, Lb, flags = DR.LAYOUTS["common37"]
    c = SimpleNamespace(pol=pol, nt=nt, sizes=list(sizes), L=Lb, mask=flags(), npix=192)
    c.pix, c.phi = DR.scan(nt, c.npix, c.mask, 11)
    c.valid = ~c.mask
    c.B = DR.baselines(sizes, Lb)
    rng = np.random.default_rng(20240521)
    c.sky = rng.standard_normal(pol * c.npix)
    c.Pref = DR.pointing(c.pix, c.phi, c.npix, pol)
    noise = np.concatenate([np.sqrt(v) * R.one_over_f(rng, s) for v, s in zip((1.0, 0.4), sizes)])
    c.d = c.Pref @ c.sky + noise
    c.d[c.mask] = 1e3

    def operators(wt):
        pairs = c.pix.copy()
        ces = cm.U.ProcessTimeSamples(pairs, c.npix, pol=pol, phi=c.phi, w=wt)
        assert ces.get_new_pixel[0] == c.npix and np.array_equal(pairs, c.pix)
        P = cm.I.SparseLO(c.npix, nt, pairs, pol=pol, angle_processed=ces)
        return P, cm.I.BlockDiagonalPreconditionerLO(ces, c.npix, pol=pol)

    # the residual of the unweighted binned map
    P1, M1 = operators(np.ones(nt))
    F1 = cm.I.OffsetsLO(P1, c.sizes, Lb)
    c.binned = cm.I.DestriperNormalLO(P1, F1, M1).map(c.d, np.zeros(c.B.na))
    c.r = np.where(c.valid, c.d - c.Pref @ c.binned, 0.0)
    c.w, c.prior, c.info = cm.op.estimate_offset_prior(c.r, c.sizes, Lb, nperseg=8192)
    c.bands = [np.asarray(b, dtype=np.float64) for b in c.prior.covnoise]
    c.P, c.Mbd = operators(DR.sample_weights(sizes, c.w, np.ones(nt, dtype=bool)))
    # the dense system from the same bands: without the identity rows of the empty baselines, plus the prior
    s = DR.system(c.sizes, c.w, Lb, c.pix, c.phi, c.npix, pol, c.d, prior=False)
    A = s.A.copy()
    A[s.empty, s.empty] = 0.0
    offs = np.concatenate([[0], np.cumsum(c.B.per_block)])
    for b, K in enumerate(c.B.per_block):
        A[offs[b]:offs[b + 1], offs[b]:offs[b + 1]] += R.toeplitz(c.bands[b], K)
    ev = np.linalg.eigvalsh(A)
    c.sys, c.A, c.kappa = s, A, ev.max() / ev.min()
    assert ev.min() > 0
    c.a_ref = np.linalg.solve(A, s.b)
    c.m_ref = DR.map_of(s, c.a_ref)
    _e2e[pol] = c
    return c


@pytest.fixture(params=["tiled", "exact"])
def mode(cm, request):
    before = cm.L.POINTING_MODE
    cm.L.set_pointing_mode(request.param)
    yield request.param
    cm.L.set_pointing_mode(before)


def without_monopole(m, pol):
    m = np.array(m, dtype=np.float64)
    if pol in (1, 3):
        m[0::pol] -= m[0::pol].mean()
    return m


@pytest.mark.parametrize("pol", [1, 3])
def test_destriping_with_the_estimated_prior_equals_the_dense_solve(cm, mode, pol):
    """Offsets and map within kappa_2(A) (rtol + 1e-12) of numpy.linalg.solve on the dense A with the same bands:
    kappa times the relative residual, cg's stopping rule plus the operator's rounding bound (test_gpu_destriper.py
    uses the same).  The map errors are records of one seed."""
    c = e2e_case(cm, pol)
    assert (c.info["K"], c.info["M"], c.info["lam"], c.info["nperseg"]) == (110, 256, 128, 8192)
    assert c.prior.shape == (c.B.na, c.B.na) and len(c.bands) == 2 and c.bands[0].shape == (128,)
    np.testing.assert_array_equal(c.w, 1.0 / c.info["sigma2"])
    m, a, info, op = cm.I.solve_destriped(c.P, c.sizes, c.L, c.d, c.Mbd, weights=c.w, prior=c.prior, rtol=RTOL,
                                          maxiter=5000)
    bound = c.kappa * (RTOL + OP_TOL)
    ea, em = rel_l2(a, c.a_ref), rel_l2(m, c.m_ref)
    m0, a0, info0, op0 = cm.I.solve_destriped(c.P, c.sizes, c.L, c.d, c.Mbd, weights=c.w, rtol=RTOL, maxiter=5000)
    errs = [np.linalg.norm(without_monopole(x - c.sky, pol)) / np.sqrt(c.sky.size) for x in (c.binned, m0, m)]
    print("\n%s pol %d: sigma2 %s, kappa_2 %.4g, bound %.3g, %d iterations with the prior (%d without), offsets %.3g,"
          " map %.3g; map error (rms per value, I monopole removed): binned %.4f, no prior %.4f, prior %.4f"
          % (mode, pol, np.array2string(c.info["sigma2"], precision=4), c.kappa, bound, op.iterations,
             op0.iterations, ea, em, errs[0], errs[1], errs[2]))
    assert info == 0 and info0 == 0
    assert ea <= bound and em <= bound, (ea, em, bound)
