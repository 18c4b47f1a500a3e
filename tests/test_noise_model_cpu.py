"""
cosmomap2_amd.utilities.noise_model without a GPU: every bad argument is refused with ValueError
before the device is touched, and a valid call raises HipError when there is no GPU.
"""
import numpy as np
import pytest


@pytest.fixture
def nm():
    from cosmomap2_amd.utilities import noise_model
    return noise_model


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


def test_exported_from_utilities():
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd.utilities import noise_model
    for name in ("noise_psd", "inverse_noise_bands", "estimate_inverse_noise"):
        assert getattr(U, name) is getattr(noise_model, name)


@pytest.mark.parametrize("nperseg", [300, 128, 131072, 0, -256, 1000, 256.0, "256", True])
def test_nperseg_not_a_power_of_two_in_range(nm, no_gpu, nperseg):
    with pytest.raises(ValueError, match="nperseg"):
        nm.noise_psd(np.zeros(4096), 1024, nperseg)


def test_nperseg_longer_than_the_shortest_block(nm, no_gpu):
    d = np.zeros(4096)
    with pytest.raises(ValueError, match="shortest block"):
        nm.noise_psd(d, [2048, 1024, 1024], 2048)
    with pytest.raises(ValueError, match="shortest block"):
        nm.noise_psd(d, 512, 1024)
    with pytest.raises(ValueError, match="shortest block"):
        nm.estimate_inverse_noise(d, [3840, 256], 64, nperseg=512)
    with pytest.raises(ValueError, match="shortest block"):     # default nperseg = 4 * next_pow2(lam) = 1024
        nm.estimate_inverse_noise(d, 512, 200)


@pytest.mark.parametrize("blocksize", [1000, 0, -1024, [2048, 2047], [4096, 1], [], [2048, 0, 2048],
                                       [2048.5, 2047.5]])
def test_blocksize_not_matching_the_tod(nm, no_gpu, blocksize):
    with pytest.raises(ValueError, match="blocksize"):
        nm.noise_psd(np.zeros(4096), blocksize, 256)
    with pytest.raises(ValueError, match="blocksize"):
        nm.estimate_inverse_noise(np.zeros(4096), blocksize, 16, nperseg=256)


@pytest.mark.parametrize("lam,nperseg", [(0, 256), (-3, 256), (129, 256), (2049, 4096), (1.5, 256)])
def test_lambda_outside_one_to_half_nperseg(nm, no_gpu, lam, nperseg):
    psd = np.ones((2, nperseg // 2 + 1))
    with pytest.raises(ValueError, match="lam"):
        nm.inverse_noise_bands(psd, lam)
    with pytest.raises(ValueError, match="lam"):
        nm.estimate_inverse_noise(np.zeros(2 * nperseg), nperseg, lam, nperseg=nperseg)


@pytest.mark.parametrize("shape", [(129,), (2, 128), (2, 130), (0, 129), (2, 129, 1), (2, 2),
                                   (1, 65538), (3, 1001)])
def test_psd_of_the_wrong_shape(nm, no_gpu, shape):
    with pytest.raises(ValueError, match="PSD"):
        nm.inverse_noise_bands(np.ones(shape), 4)


@pytest.mark.parametrize("fs", [0.0, -1.0, np.inf, np.nan, "x"])
def test_bad_sampling_rate(nm, no_gpu, fs):
    with pytest.raises(ValueError, match="fsample"):
        nm.noise_psd(np.zeros(1024), 512, 256, fsample=fs)
    with pytest.raises(ValueError, match="fsample"):
        nm.inverse_noise_bands(np.ones((1, 129)), 4, fsample=fs)


def test_other_bad_arguments(nm, no_gpu):
    with pytest.raises(ValueError, match="detrend"):
        nm.noise_psd(np.zeros(1024), 512, 256, detrend="linear")
    with pytest.raises(ValueError, match="detrend"):
        nm.noise_psd(np.zeros(1024), 512, 256, detrend=True)
    with pytest.raises(ValueError, match="one-dimensional"):
        nm.noise_psd(np.zeros((2, 512)), 512, 256)
    with pytest.raises(ValueError, match="work_bytes"):
        nm.noise_psd(np.zeros(1024), 512, 256, work_bytes=0)


def test_valid_calls_raise_hip_error_without_a_gpu(nm, no_gpu):
    from cosmomap2_amd import _hip
    rng = np.random.default_rng(0)
    d = rng.standard_normal(4096)
    for call in (lambda: nm.noise_psd(d, 2048, 256),
                 lambda: nm.noise_psd(d, [1024, 3072], 1024, fsample=200.0, detrend=False, work_bytes=1 << 20),
                 lambda: nm.inverse_noise_bands(np.ones((3, 129)), 128, fsample=20.0),
                 lambda: nm.estimate_inverse_noise(d, 1024, 64),
                 lambda: nm.estimate_inverse_noise(d, [2048, 2048], 1, nperseg=2048)):
        with pytest.raises(_hip.HipError):
            call()


def test_abi_lists_name_the_new_entry_points():
    from cosmomap2_amd import _hip, kernel_resources as KR
    import re
    for name in ("cm2_psd_create", "cm2_psd_welch", "cm2_noise_bands_from_psd"):
        assert name in _hip.PROTOTYPES and name in _hip.RESTARTABLE
    assert "cm2_psd_destroy" in _hip.PROTOTYPES and "cm2_psd_info" in _hip.PROTOTYPES
    for kernel in ("k_psd_pack", "k_psd_accumulate", "k_psd_finish", "cm2::psd::k_bands_spectrum<0>", "k_bands_lags"):
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel
