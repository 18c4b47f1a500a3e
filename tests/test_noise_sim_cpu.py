"""
cosmomap2_amd.utilities.noise_sim without a GPU: every bad argument is refused with ValueError before the
device is touched, a valid call raises HipError when there is no GPU, and the new entry points and
kernels are listed where the build and the binding look for them.
"""
import os
import re
import shutil

import numpy as np
import pytest


@pytest.fixture
def ns():
    from cosmomap2_amd.utilities import noise_sim
    return noise_sim


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


PSD = np.ones((1, 129))                  # L = 256


def test_exported_from_utilities():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd.utilities import noise_sim
    for name in ("white_noise", "noise_filter_bands", "NoiseSimulator", "simulate_noise"):
        assert getattr(U, name) is getattr(noise_sim, name)


@pytest.mark.parametrize("lam", [0, -3, 129, 1.5, "4", True])
def test_lambda_outside_one_to_half_nperseg(ns, no_gpu, lam):
    with pytest.raises(ValueError, match="lam"):
        ns.noise_filter_bands(PSD, lam)
    with pytest.raises(ValueError, match="lam"):
        ns.NoiseSimulator([1000, 2000], PSD, lam)
    with pytest.raises(ValueError, match="lam"):
        ns.simulate_noise([1000, 2000], PSD, lam, seed=1)


@pytest.mark.parametrize("shape", [(129,), (2, 128), (2, 130), (0, 129), (2, 129, 1), (2, 2), (1, 65538)])
def test_psd_of_the_wrong_shape(ns, no_gpu, shape):
    with pytest.raises(ValueError, match="PSD"):
        ns.noise_filter_bands(np.ones(shape), 4)
    with pytest.raises(ValueError, match="PSD"):
        ns.NoiseSimulator([1000, 2000], np.ones(shape), 4)


def test_psd_rows_against_the_blocks(ns, no_gpu):
    with pytest.raises(ValueError, match="PSD has 3 rows for 2 blocks"):
        ns.NoiseSimulator([1000, 2000], np.ones((3, 129)), 4)
    with pytest.raises(ValueError, match="PSD has 2 rows for 4 blocks"):
        ns.simulate_noise(1000, np.ones((2, 129)), 4, seed=0, nt=4000)


@pytest.mark.parametrize("blocksize,nt", [(1000, 4096), (0, 4096), (-1024, 4096), ([2048, 2047], 4096),
                                          ([4096, 1], 4096), ([], 4096), ([2048, 0, 2048], 4096),
                                          ([2048.5, 2047.5], 4096), (1024, 0), (1024, -4096), (1024, 4096.0)])
def test_blocksize_not_matching_nt(ns, no_gpu, blocksize, nt):
    with pytest.raises(ValueError, match="blocksize|nt"):
        ns.NoiseSimulator(blocksize, PSD, 4, nt=nt)
    with pytest.raises(ValueError, match="blocksize|nt"):
        ns.simulate_noise(blocksize, PSD, 4, seed=0, nt=nt)


@pytest.mark.parametrize("blocksize", [0, -5, [], [100, 0], [100, -1], 10.5, [10.5], "100"])
def test_block_sizes_that_are_not_positive_integers(ns, no_gpu, blocksize):
    with pytest.raises(ValueError, match="blocksize"):
        ns.NoiseSimulator(blocksize, PSD, 4)


@pytest.mark.parametrize("bad", [-1, 1 << 64, (1 << 64) + 5, 1.0, "3", None, True])
def test_stream_indices_outside_64_bits(ns, no_gpu, bad):
    for name in ("seed", "realization", "block"):
        kw = dict(seed=1)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            ns.white_noise(16, **kw)
    for name in ("seed", "first_block"):
        with pytest.raises(ValueError, match=name):
            ns.NoiseSimulator([1000], PSD, 4, **{name: bad})
    for name in ("seed", "realization", "first_block"):
        kw = dict(seed=1)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            ns.simulate_noise([1000], PSD, 4, **kw)


def test_first_block_plus_blocks_past_two_to_the_64(ns, no_gpu):
    with pytest.raises(ValueError, match="first_block"):
        ns.NoiseSimulator([100, 100, 100], PSD, 4, first_block=(1 << 64) - 2)


@pytest.mark.parametrize("first", [-1, -4, 1 << 62, 0.0, "0"])
def test_bad_first_sample(ns, no_gpu, first):
    with pytest.raises(ValueError, match="first"):
        ns.white_noise(16, 1, first=first)


@pytest.mark.parametrize("n", [-1, 2.0, "8", None])
def test_bad_sample_count(ns, no_gpu, n):
    with pytest.raises(ValueError, match="n"):
        ns.white_noise(n, 1)


@pytest.mark.parametrize("kind", ["gauss", "Normal", 1, None, b"normal"])
def test_bad_kind(ns, no_gpu, kind):
    with pytest.raises(ValueError, match="kind"):
        ns.white_noise(16, 1, kind=kind)


@pytest.mark.parametrize("fs", [0.0, -1.0, np.inf, np.nan, "x"])
def test_bad_sampling_rate(ns, no_gpu, fs):
    with pytest.raises(ValueError, match="fsample"):
        ns.noise_filter_bands(PSD, 4, fsample=fs)
    with pytest.raises(ValueError, match="fsample"):
        ns.NoiseSimulator([1000], PSD, 4, fsample=fs)


@pytest.mark.parametrize("out", [np.zeros(2999), np.zeros(3001), np.zeros((3, 1000)), np.zeros(3000, dtype=np.float32),
                                 np.zeros(3000, dtype=np.int64), np.zeros(6000)[::2], [0.0] * 3000, "out"])
def test_out_of_the_wrong_length_or_dtype(ns, no_gpu, out):
    with pytest.raises(ValueError, match="out"):
        ns.simulate_noise([1000, 2000], PSD, 4, seed=1, out=out)


def test_out_tensors_that_are_not_float64_in_hbm(ns, no_gpu):
    torch = pytest.importorskip("torch")
    for out in (torch.zeros(3000, dtype=torch.float64), torch.zeros(3000, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out"):
            ns.simulate_noise([1000, 2000], PSD, 4, seed=1, out=out)


def test_other_bad_draw_arguments(ns, no_gpu):
    out = np.zeros(3000)
    with pytest.raises(ValueError, match="add"):
        ns.simulate_noise([1000, 2000], PSD, 4, seed=1, out=out, add=1)
    with pytest.raises(ValueError, match="add=True needs an out"):
        ns.simulate_noise([1000, 2000], PSD, 4, seed=1, add=True)
    for scale in (np.nan, np.inf, "x", None):
        with pytest.raises(ValueError, match="scale"):
            ns.simulate_noise([1000, 2000], PSD, 4, seed=1, out=out, scale=scale)
    ro = np.zeros(3000)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="out"):
        ns.simulate_noise([1000, 2000], PSD, 4, seed=1, out=ro)


def test_valid_calls_raise_hip_error_without_a_gpu(ns, no_gpu):
    from cosmomap2_amd import _hip
    big = (1 << 64) - 1
    for call in (lambda: ns.white_noise(1000, 1),
                 lambda: ns.white_noise(0, big, realization=big, block=big, first=(1 << 62) - 1, kind="uniform"),
                 lambda: ns.noise_filter_bands(np.ones((3, 129)), 128, fsample=20.0),
                 lambda: ns.noise_filter_bands(np.zeros((1, 129)), 1),
                 lambda: ns.NoiseSimulator([1000, 2000], np.ones((2, 129)), 64, fsample=200.0, seed=big,
                                           first_block=big - 1),
                 lambda: ns.NoiseSimulator(1000, PSD, 4, nt=4000),
                 lambda: ns.NoiseSimulator(1000, PSD, 1),
                 lambda: ns.simulate_noise([1000, 2000], PSD, 128, seed=3, realization=big, out=np.zeros(3000),
                                           add=True, scale=-2.5)):
        with pytest.raises(_hip.HipError):
            call()


def test_abi_lists_name_the_new_entry_points():
    from cosmomap2_amd import _hip, kernel_resources as KR
    for name in ("cm2_rng_fill", "cm2_noise_filter_from_psd", "cm2_noise_sim_create"):
        assert name in _hip.PROTOTYPES and name in _hip.RESTARTABLE
    for name in ("cm2_noise_sim_draw", "cm2_noise_sim_destroy", "cm2_noise_sim_info"):
        assert name in _hip.PROTOTYPES
    assert "cm2_noise_sim_draw" not in _hip.RESTARTABLE          # add=True: a second run would add twice
    for kernel in ("k_rng_fill<0>", "k_rng_fill<1>", "k_sim_interior", "cm2::psd::k_bands_spectrum<1>"):
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel


def test_header_declares_what_the_binding_lists():
    from cosmomap2_amd import _hip
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "cosmomap2.h")).read()
    assert re.search(r"#define CM2_ABI_VERSION 2\b", text)
    for name in ("cm2_rng_fill", "cm2_noise_filter_from_psd", "cm2_noise_sim_create", "cm2_noise_sim_draw",
                 "cm2_noise_sim_destroy", "cm2_noise_sim_info"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.PROTOTYPES[name]), name


def test_library_cross_compiles_with_no_scratch_in_the_new_kernels():
    """python -m cosmomap2_amd.build for gfx950 (a no-op when the library is up to date), then the
    resource table of the shipped objects: the new kernels are there and use no scratch."""
    from cosmomap2_amd import build as B, kernel_resources as KR
    if not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)):
        pytest.fail("hipcc not found at %s: the library cannot be built" % B.HIPCC)
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all()}
    for kernel in ("k_rng_fill<0>", "k_rng_fill<1>", "k_sim_interior", "cm2::psd::k_bands_spectrum<1>"):
        assert kernel in rows, sorted(rows)
        assert rows[kernel].get("scratch_bytes_per_lane", 0) == 0, rows[kernel]
        assert rows[kernel].get("vgpr_spill", 0) == 0, rows[kernel]
    assert KR.offenders(list(rows.values())) == []

