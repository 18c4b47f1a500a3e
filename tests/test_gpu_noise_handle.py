"""
The cm2_noise handle on the GPU (cm2_noise.hip): the tiled direct route at its LDS boundaries, a direct
operator that is complete when cm2_noise_create_toeplitz returns (nothing is allocated by an application,
two host threads may share a fresh operator), a refused build that gives its memory back, and the two users
of rocFFT (cm2_psd, the method-2 operator) in one process in either order.
"""
import ctypes
import gc
import threading

import numpy as np
import pytest
import scipy.signal as ss

from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd.utilities import noise_model
    from types import SimpleNamespace
    return SimpleNamespace(I=I, D=D, L=L, hip=_hip, nm=noise_model, torch=torch)


def _bands(lam, nb):
    k = np.arange(lam)
    return [(1.0 + 0.1 * b) * np.exp(-k / (0.2 * lam + 1.0)) * np.cos(0.5 * k / (lam + 1.0)) for b in range(nb)]


def _library_memory(cm):
    """(requests the library's allocator has served, bytes its live objects hold)"""
    m = cm.D.memory_info()
    return m["cache_hits"] + m["driver_allocations"], m["live_bytes"]


# kDirTile = 2048 outputs per workgroup: the tiled kernel needs 8 (2048 + 2 (lam - 1)) bytes of LDS.
#   3073 -> 65536, the last band served without the dynamic-LDS attribute; 3074 -> 65552, the first with it;
#   8577 -> 153600 = 150 KiB, the last tiled one; 8578 -> 153616, the first that takes the plain loop.
@pytest.mark.parametrize("lam", [3073, 3074, 8577, 8578])
def test_direct_route_at_its_lds_boundaries(cm, oracle, lam):
    sizes = [2049, 1, 2047, 5000]
    bands = _bands(lam, len(sizes))
    v = np.random.default_rng(lam).standard_normal(sum(sizes))
    N = cm.I.BlockLO(sizes, bands, offdiag=True, method=1)
    np.testing.assert_array_equal(N * v, oracle.blocklo_mult(sizes, bands, True, v))


def test_direct_operator_is_complete_at_creation(cm, oracle):
    """The tile list of a CM2_TOEPLITZ_DIRECT operator exists when the create call returns: an application
    asks the library's allocator for nothing."""
    lam, sizes = 9, [2047, 2048, 2049, 1]
    bands = _bands(lam, len(sizes))
    v = np.random.default_rng(9).standard_normal(sum(sizes))
    x, out = cm.D.f64(v), cm.D.empty(sum(sizes))
    gc.collect()                                    # no handle of an earlier test is freed in between
    h = cm.L._make_toeplitz(np.vstack(bands), sizes, 1)
    created = _library_memory(cm)
    for _ in range(2):
        cm.hip.call("cm2_noise_apply", h.h, cm.D.ptr(x), cm.D.ptr(out), cm.D.stream())
        assert _library_memory(cm) == created
    np.testing.assert_array_equal(cm.D.to_host(out), oracle.blocklo_mult(sizes, bands, True, v))


def test_two_threads_on_a_fresh_direct_operator(cm):
    """Two host threads, each on its own stream, make the first applications of one direct operator: both
    get the bits of the sequential run, and the operator holds afterwards what it held before."""
    t = cm.torch
    nt, lam = 300000, 9
    sizes = [100000] * 3
    bands = np.vstack(_bands(lam, 3))
    rng = np.random.default_rng(17)
    ins = [cm.D.f64(rng.standard_normal(nt)) for _ in range(2)]
    want = []
    seq = cm.L._make_toeplitz(bands, sizes, 1)
    for a in ins:
        b = cm.D.empty(nt)
        cm.hip.call("cm2_noise_apply", seq.h, cm.D.ptr(a), cm.D.ptr(b), cm.D.stream())
        want.append(b)
    t.cuda.synchronize()
    gc.collect()
    fresh = cm.L._make_toeplitz(bands, sizes, 1)
    live0 = _library_memory(cm)[1]
    outs, errs = {}, []

    def work(k):
        try:
            st = t.cuda.Stream()
            with t.cuda.stream(st):
                for _ in range(5):
                    b = cm.D.empty(nt)
                    cm.hip.call("cm2_noise_apply", fresh.h, cm.D.ptr(ins[k]), cm.D.ptr(b), cm.D.stream())
                st.synchronize()
                outs[k] = b
        except Exception as e:                      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for h in th:
        h.start()
    for h in th:
        h.join()
    assert not errs, errs
    for k in (0, 1):
        assert t.equal(outs[k], want[k])
    assert _library_memory(cm)[1] == live0


def test_refused_build_returns_its_memory(cm, oracle):
    """lambda = 2050 is the first band the fused kernel refuses: the create call fails with CM2_ERR_ARGUMENT
    after the offsets and the bands went to the device, and frees them; the rocFFT route serves the same
    arguments."""
    lam, sizes = 2050, [4096]
    bands = _bands(lam, 1)
    gc.collect()
    live0 = _library_memory(cm)[1]
    with pytest.raises(cm.hip.HipError) as e:
        cm.L._make_toeplitz(np.vstack(bands), sizes, 3)
    assert e.value.status == cm.hip.ERR_ARGUMENT
    assert _library_memory(cm)[1] == live0
    v = np.random.default_rng(2050).standard_normal(sum(sizes))
    N = cm.I.BlockLO(sizes, bands, offdiag=True, method=2)
    assert N.noise_info()["method"] == 2
    assert rel_l2(N * v, oracle.blocklo_mult(sizes, bands, True, v)) < 1e-12


def _psd_and_fft_operator(cm, oracle, psd_first):
    """A cm2_psd (nperseg 256) and a method-2 operator built one after the other, both alive, then both
    used: what test_psd_and_bands_match_scipy and test_toeplitz_fft_matches_direct require of each."""
    L, fs, psd_sizes = 256, 20.0, [5000, 12345, 256, 8191]
    lam, sizes = 33, [1000, 50, 3000]
    bands = _bands(lam, len(sizes))

    def make_psd():
        return cm.nm._Psd(L, 1, None)

    def make_op():
        return cm.I.BlockLO(sizes, bands, offdiag=True, method=2)
    if psd_first:
        h = make_psd()
        N = make_op()
    else:
        N = make_op()
        h = make_psd()
    assert h.info()["nperseg"] == L and N.noise_info()["method"] == 2
    rng = np.random.default_rng(5)
    # the operator
    v = rng.standard_normal(sum(sizes))
    assert rel_l2(N * v, oracle.blocklo_mult(sizes, bands, True, v)) < 1e-12
    e = np.zeros(sum(sizes))
    e[sizes[0] - 1] = 1.0                           # zero boundary: nothing leaks into the next block
    assert np.abs((N * e)[sizes[0]:]).max() < 1e-13
    # the PSD
    n, nb = sum(psd_sizes), len(psd_sizes)
    x = rng.standard_normal(n) + 0.5 * np.convolve(rng.standard_normal(n), np.ones(16) / 4.0, mode="same")
    xd, psd = cm.D.f64(x), cm.D.empty(nb * (L // 2 + 1))
    sz = np.ascontiguousarray(psd_sizes, dtype=np.int64)
    cm.hip.call("cm2_psd_welch", h.h, cm.D.ptr(xd), sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nb, fs,
                cm.D.ptr(psd), cm.D.stream())
    psd = cm.D.to_host(psd.view(nb, L // 2 + 1))
    off = np.concatenate([[0], np.cumsum(psd_sizes)])
    for b in range(nb):
        _, pr = ss.welch(x[off[b]:off[b + 1]], fs, window="hann", nperseg=L, noverlap=L // 2, detrend="constant",
                         scaling="density", average="mean")
        assert rel_l2(psd[b], pr) <= 1e-12, b
        assert np.max(np.abs(psd[b] - pr) / pr) <= 1e-9, b


def test_psd_then_fft_operator(cm, oracle):
    _psd_and_fft_operator(cm, oracle, True)


def test_fft_operator_then_psd(cm, oracle):
    _psd_and_fft_operator(cm, oracle, False)
