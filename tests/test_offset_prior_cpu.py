"""
The offset prior without a GPU: the restatement of _offset_prior_ref.py against its own definition (the closed-form
covariance of baseline means against the double sum over irfft(R), positive definiteness, the flat PSD), the float64
restatement within the derived bound and the bound within 1e-9 of band_0 on every input of the GPU tests, and every
refusal of cosmomap2_amd.utilities.offset_prior before the device is touched.
"""
import os
import re

import numpy as np
import pytest

import _offset_prior_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSD_NAMES = ("welch_1f", "welch_white", "flat", "band_limited")
_inputs = {}


def inputs(n):
    if n not in _inputs:
        _inputs[n] = R.psd_inputs(n)
    return _inputs[n]


@pytest.fixture
def op():
    from cosmomap2_amd.utilities import offset_prior
    return offset_prior


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


# ------------------------------------------------------------------------------ the definition ------
@pytest.mark.parametrize("L", [1, 3, 37, 64])
def test_closed_form_q_equals_the_double_sum_over_the_autocovariance(L):
    """q_j = (1/L^2) sum_{|s| < L} (L - |s|) r_{|jL + s|} with r = irfft(R, n), to 1e-12 of q_0 (measured 2e-16 to
    8e-16 in float64 at n = 256)."""
    n = 256
    for name in ("welch_1f", "band_limited"):
        row, s2 = inputs(n)[name]
        for dtype in (R.LD, np.float64):
            ref = R.prior(row, L, 1, sigma2=s2, dtype=dtype)
            brute = R.q_brute(ref.R, n, L, ref.K)
            e = float(np.abs(ref.q.astype(R.LD) - brute).max() / brute[0])
            print("\nL = %d, %s, %s: closed form against the double sum %.3g of q_0" % (L, name, dtype.__name__, e))
            assert brute[0] > 0 and e <= 1e-12, e


@pytest.mark.parametrize("n,L,lam", R.GEOMETRIES)
def test_every_band_is_positive_definite(n, L, lam):
    for name in PSD_NAMES:
        row, s2 = inputs(n)[name]
        for sigma2 in (None, s2):
            band = R.prior(row, L, lam, sigma2=sigma2, dtype=np.float64).band
            ev = np.linalg.eigvalsh(R.toeplitz(band, 3 * lam))
            assert ev.min() > 0, (name, sigma2, ev.min())


@pytest.mark.parametrize("n,L,lam", R.GEOMETRIES)
def test_flat_psd_gives_the_floor_on_the_diagonal(n, L, lam):
    """S = sigma^2 in every bin: R = 0, Q = 0, every bin floored, band = L / (floor sigma^2) delta_i.  The sums of
    steps 2 to 5 are exact in floating point here (S = 2.5), the last one is not (odd multiples of H, cosines that
    cancel only in exact arithmetic): equal within the derived bound, which is below 1e-13 of band_0."""
    row, s2 = inputs(n)["flat"]
    for floor in (1e-6, 0.25, 1.0):
        for sigma2 in (None, s2):
            ref = R.prior(row, L, lam, sigma2=sigma2, floor=floor, bound=True)
            f64 = R.prior(row, L, lam, sigma2=sigma2, floor=floor, dtype=np.float64)
            want = np.zeros(lam, dtype=R.LD)
            want[0] = R.LD(L) / (R.LD(np.float64(floor)) * R.LD(2.5))
            assert ref.floored == ref.M // 2 + 1 and ref.sigma2 == 2.5 and f64.sigma2 == 2.5
            assert np.all(f64.Q == 0.0)
            assert np.all(np.abs(ref.band - want) <= ref.band_err)
            assert np.all(np.abs(f64.band.astype(R.LD) - want) <= ref.band_err)
            assert float(ref.band_err.max() / want[0]) <= 1e-13


@pytest.mark.parametrize("n,L,lam", R.GEOMETRIES)
def test_float64_restatement_within_the_bound_and_the_bound_below_1e_9(n, L, lam):
    """The cap keeps the bound from being vacuous (measured: float64 against np.longdouble at most 4.3e-14 of band_0,
    the bound at most 2.5e-10 of band_0)."""
    for name in PSD_NAMES:
        row, s2 = inputs(n)[name]
        for sigma2 in (None, s2):
            ref = R.prior(row, L, lam, sigma2=sigma2, bound=True)
            f64 = R.prior(row, L, lam, sigma2=sigma2, dtype=np.float64)
            err = np.abs(f64.band.astype(R.LD) - ref.band)
            cap = float(ref.band_err.max() / ref.band[0])
            print("\nn %d L %d lam %d %s sigma2 %s: float64 %.3g of band_0, %.3g of the bound; bound %.3g of band_0"
                  % (n, L, lam, name, "given" if sigma2 else "estimated", float(err.max() / ref.band[0]),
                     float((err / ref.band_err).max()), cap))
            assert ref.band[0] > 0 and np.all(ref.band_err > 0)
            assert np.all(err <= ref.band_err), (name, sigma2)
            assert abs(R.LD(f64.sigma2) - ref.sigma2) <= ref.sigma2_err
            assert cap <= 1e-9, (name, sigma2, cap)


def test_geometry():
    assert [R.geometry(256, L) for L in (1, 3, 37, 64)] == [(129, 512), (43, 128), (3, 8), (2, 4)]
    assert R.geometry(1024, 37) == (13, 32) and R.geometry(8192, 37) == (110, 256)


# ----------------------------------------------------------------------------------- refusals ------
PSD = np.ones((2, 129))


def test_exported_from_utilities():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd.utilities import offset_prior
    for name in ("offset_prior_bands", "estimate_offset_prior"):
        assert getattr(U, name) is getattr(offset_prior, name)
    assert U.noise_psd is not None


def test_too_few_baseline_lags_names_the_smallest_nperseg(op, no_gpu):
    with pytest.raises(ValueError, match=r"smallest nperseg that would do is 512\b"):
        op.offset_prior_bands(PSD, 65, 1)
    with pytest.raises(ValueError, match=r"smallest nperseg that would do is 65536\b"):
        op.offset_prior_bands(PSD, 16384, 1)
    with pytest.raises(ValueError, match="too long for any nperseg"):
        op.offset_prior_bands(PSD, 20000, 1)
    with pytest.raises(ValueError, match=r"smallest nperseg that would do is 512\b"):
        op.estimate_offset_prior(np.zeros(4096), 2048, 65, nperseg=256)
    for L in (0, -3, 1.5, "37", True):
        with pytest.raises(ValueError, match="baseline_length"):
            op.offset_prior_bands(PSD, L, 1)
        with pytest.raises(ValueError, match="baseline_length"):
            op.estimate_offset_prior(np.zeros(4096), 2048, L)


@pytest.mark.parametrize("L,lam", [(37, 5), (37, 0), (64, 3), (1, 257), (3, -1), (3, 2.0)])
def test_band_longer_than_half_the_offset_spectrum(op, no_gpu, L, lam):
    with pytest.raises(ValueError, match="lam"):
        op.offset_prior_bands(PSD, L, lam)


@pytest.mark.parametrize("floor", [0.0, -1e-6, 1.0000001, np.inf, np.nan, "x", None])
def test_floor_outside_zero_to_one(op, no_gpu, floor):
    with pytest.raises(ValueError, match="floor"):
        op.offset_prior_bands(PSD, 37, 4, floor=floor)
    with pytest.raises(ValueError, match="floor"):
        op.estimate_offset_prior(np.zeros(4096), 2048, 37, floor=floor)


@pytest.mark.parametrize("sigma2", [0.0, -1.0, np.inf, np.nan, [1.0, 0.0], [1.0, np.nan], [1.0], [1.0, 2.0, 3.0],
                                    [[1.0, 2.0]], "x"])
def test_bad_white_variance(op, no_gpu, sigma2):
    with pytest.raises(ValueError, match="sigma2"):
        op.offset_prior_bands(PSD, 37, 4, sigma2=sigma2)


def test_bad_psd_bin_names_the_block_and_the_bin(op, no_gpu):
    for value in (0.0, -1.0, np.nan, np.inf):
        psd = np.ones((3, 129))
        psd[1, 77] = value
        psd[2, 5] = value
        with pytest.raises(ValueError, match=r"block 1\b.*bin 77\b"):
            op.offset_prior_bands(psd, 37, 4)
    psd = np.ones((3, 129))
    psd[:, 0] = np.nan                                       # the DC bin is not used
    psd[2, 1] = 0.0
    with pytest.raises(ValueError, match=r"block 2\b.*bin 1\b"):
        op.offset_prior_bands(psd, 37, 4)
    for shape in ((129,), (2, 128), (0, 129)):
        with pytest.raises(ValueError, match="PSD"):
            op.offset_prior_bands(np.ones(shape), 37, 4)
    with pytest.raises(ValueError, match="fsample"):
        op.offset_prior_bands(PSD, 37, 4, fsample=0.0)


def test_estimate_refusals(op, no_gpu):
    r = np.zeros(6000)
    with pytest.raises(ValueError, match="blocksize"):
        op.estimate_offset_prior(r, 4096, 37)
    with pytest.raises(ValueError, match="shortest block"):
        op.estimate_offset_prior(r, [5000, 1000], 37, nperseg=2048)
    with pytest.raises(ValueError, match="shortest block"):
        op.estimate_offset_prior(r, [5800, 200], 37)
    with pytest.raises(ValueError, match="nperseg"):
        op.estimate_offset_prior(r, [5000, 1000], 37, nperseg=1000)
    for lam in (9, 0, 2.5):                                  # nperseg 512, L = 37: K = 6, M = 16, lam <= 8
        with pytest.raises(ValueError, match="lam"):
            op.estimate_offset_prior(r, [5000, 1000], 37, lam=lam, nperseg=512)
    with pytest.raises(ValueError, match="detrend"):
        op.estimate_offset_prior(r, [5000, 1000], 37, detrend="linear")
    with pytest.raises(ValueError, match="fsample"):
        op.estimate_offset_prior(r, [5000, 1000], 37, fsample=-1.0)
    with pytest.raises(ValueError, match="one-dimensional"):
        op.estimate_offset_prior(np.zeros((2, 3000)), 3000, 37)


def test_estimate_defaults_and_chain(op, monkeypatch):
    """nperseg=None is the largest allowed power of two no longer than the shortest block, lam=None the smaller of
    M/2 and the fewest baselines of a block; the chain is noise_psd -> offset_prior_bands -> BlockLO on the baselines
    per block.  The three stages are replaced by recorders: no GPU."""
    from cosmomap2_amd.interfaces import linearoperators
    seen = {}

    def psd(r, blocksize, nperseg, fsample, detrend):
        seen["psd"] = (blocksize, nperseg, fsample, detrend)
        return None, np.ones((2, nperseg // 2 + 1))

    def bands(p, L, lam, fsample, sigma2, floor):
        seen["bands"] = (p.shape, L, lam, fsample, sigma2, floor)
        return np.tile(np.arange(lam, 0.0, -1.0), (p.shape[0], 1)), np.array([4.0, 0.5])

    def blocklo(sizes, t, offdiag=False):
        seen["blocklo"] = (list(sizes), [len(b) for b in t], offdiag)
        return "prior"

    monkeypatch.setattr(op, "noise_psd", psd)
    monkeypatch.setattr(op, "offset_prior_bands", bands)
    monkeypatch.setattr(linearoperators, "BlockLO", blocklo)
    w, prior, info = op.estimate_offset_prior(np.zeros(6000), [5000, 1000], 37, fsample=20.0, floor=0.5)
    assert seen["psd"] == ([5000, 1000], 512, 20.0, "constant")              # 512 <= 1000 < 1024
    assert seen["bands"] == ((2, 257), 37, 8, 20.0, None, 0.5)               # K = 6, M = 16; 136 and 28 baselines
    assert seen["blocklo"] == ([136, 28], [8, 8], True) and prior == "prior"
    np.testing.assert_array_equal(w, [0.25, 2.0])
    assert (info["K"], info["M"], info["lam"], info["nperseg"]) == (6, 16, 8, 512)
    np.testing.assert_array_equal(info["sigma2"], [4.0, 0.5])
    w, prior, info = op.estimate_offset_prior(np.zeros(140000), 70000, 37, lam=3)
    assert seen["psd"][1] == 65536 and seen["bands"][2] == 3 and info["M"] == 2048


def test_valid_calls_raise_hip_error_without_a_gpu(op, no_gpu):
    from cosmomap2_amd import _hip
    r = np.random.default_rng(0).standard_normal(6000)
    for call in (lambda: op.offset_prior_bands(PSD, 37, 4),
                 lambda: op.offset_prior_bands(PSD, 1, 256, fsample=20.0, sigma2=[1.0, 2.0], floor=1.0),
                 lambda: op.offset_prior_bands(PSD, 64, 2, sigma2=0.5),
                 lambda: op.estimate_offset_prior(r, [5000, 1000], 37),
                 lambda: op.estimate_offset_prior(r, 3000, 37, lam=3, nperseg=512, detrend=False)):
        with pytest.raises(_hip.HipError):
            call()


def test_the_library_refuses_bad_arguments_before_the_device():
    """Every argument check of cm2_offset_prior_from_psd comes before its first HIP call: no GPU is needed to meet
    them, and the pointers are never read."""
    import ctypes
    from cosmomap2_amd import _hip
    lib = _hip.load()
    psd, bands = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    two = (ctypes.c_double * 2)
    s_out = two(-1.0, -1.0)
    for args, word in (((2, 256, 1.0, 65, 1, None, 1e-6), b"smallest nperseg that would do is 512"),
                       ((2, 256, 1.0, 16384, 1, None, 1e-6), b"smallest nperseg that would do is 65536"),
                       ((2, 256, 1.0, 20000, 1, None, 1e-6), b"too long for any nperseg"),
                       ((2, 256, 1.0, 2 ** 62, 1, None, 1e-6), b"too long for any nperseg"),
                       ((2, 256, 1.0, 37, 5, None, 1e-6), b"lambda=5"),
                       ((2, 256, 1.0, 37, 0, None, 1e-6), b"lambda=0"),
                       ((2, 256, 1.0, 37, 4, None, 0.0), b"floor"),
                       ((2, 256, 1.0, 37, 4, None, 1.5), b"floor"),
                       ((2, 256, 1.0, 37, 4, None, float("nan")), b"floor"),
                       ((2, 256, 1.0, 37, 4, two(1.0, 0.0), 1e-6), b"sigma2 of block 1"),
                       ((2, 256, 1.0, 37, 4, two(float("inf"), 1.0), 1e-6), b"sigma2 of block 0"),
                       ((2, 256, 0.0, 37, 4, None, 1e-6), b"fsample"),
                       ((2, 300, 1.0, 37, 4, None, 1e-6), b"nperseg"),
                       ((2, 131072, 1.0, 37, 4, None, 1e-6), b"nperseg"),
                       ((0, 256, 1.0, 37, 4, None, 1e-6), b"nb="),
                       ((2, 256, 1.0, 0, 4, None, 1e-6), b"baseline_length")):
        nb, n, fs, L, lam, s_in, floor = args
        rc = lib.cm2_offset_prior_from_psd(psd, nb, n, fs, L, lam, s_in, floor, bands, s_out, None)
        msg = lib.cm2_last_error()
        assert rc == _hip.ERR_ARGUMENT and b"cm2_offset_prior_from_psd" in msg and word in msg, (args, rc, msg)
    assert list(s_out) == [-1.0, -1.0]
    assert lib.cm2_offset_prior_from_psd(None, 2, 256, 1.0, 37, 4, None, 1e-6, bands, None, None) == _hip.ERR_ARGUMENT
    assert lib.cm2_offset_prior_from_psd(psd, 2, 256, 1.0, 37, 4, None, 1e-6, None, None, None) == _hip.ERR_ARGUMENT


def test_abi_lists_name_the_new_entry_point():
    from cosmomap2_amd import _hip, kernel_resources as KR
    name = "cm2_offset_prior_from_psd"
    assert name in _hip.PROTOTYPES and name in _hip.RESTARTABLE and len(_hip.PROTOTYPES[name]) == 11
    text = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
    assert m and len(m.group(1).split(",")) == len(_hip.PROTOTYPES[name])
    assert m.group(1).startswith("const double *d_psd, int64_t nb, int64_t nperseg, double fsample,")
    assert re.search(r"#define CM2_ABI_VERSION 2\b", text)
    src = "".join(open(os.path.join(ROOT, "cosmomap2_amd", "csrc", f)).read()
                  for f in ("cm2_offset_prior.hip", "cm2_psd_bands.h"))
    kernels = set(re.findall(r"\bvoid (k_\w+)\(", src))
    assert {"k_bands_spectrum", "k_bands_cos_table", "k_oprior_q", "k_oprior_invert", "k_oprior_band"} <= kernels
    for kernel in kernels:
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel
    assert "atomicAdd" not in src
