"""
Noise time streams drawn from a PSD on the GPU (cm2_noise_sim.hip, cosmomap2_amd/utilities/noise_sim.py):
the Philox stream against numpy.random.Philox bit for bit, the normals and the colouring band against
their NumPy restatements, a draw against scipy.signal.fftconvolve(..., 'valid') on the restated normals
over the direct, fused and rocFFT routes, sharding, and the closures: spectrum, estimator, GLS map.
All deterministic from fixed seeds.
"""
import time

import numpy as np
import pytest
import scipy.signal as ss

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DIRECT, FFT, FUSED = 1, 2, 3             # CM2_TOEPLITZ_* of include/cosmomap2.h


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    import cosmomap2_amd
    from cosmomap2_amd.utilities import noise_model, noise_sim
    from cosmomap2_amd import device as D
    from types import SimpleNamespace
    return SimpleNamespace(I=I, U=U, nm=noise_model, ns=noise_sim, cg=cosmomap2_amd.cg, torch=torch, D=D,
                           dev=torch.device("cuda", 0))


def to_dev(cm, a):
    return cm.D.f64(np.ascontiguousarray(a))


def to_host(cm, t):
    return cm.D.to_host(t)


# ------------------------------------------------------------------ restatements in NumPy ------
def np_uniform(seed, realization, block, n):
    """The first n uniforms of the stream (seed, realization, block).  (Key and counter as uint64 arrays:
    a list that mixes small integers with one >= 2^63 would go through float64 and lose its low bits.)"""
    bg = np.random.Philox(key=np.array([seed, realization], dtype=np.uint64),
                          counter=np.array([0, block, 0, 0], dtype=np.uint64))
    return np.random.Generator(bg).random(n)


def np_normal(seed, realization, block, n):
    """Box-Muller over the pairs (u0, u1), (u2, u3) of every counter block, with cos(2 pi u)."""
    u = np_uniform(seed, realization, block, 4 * ((n + 3) // 4)).reshape(-1, 4)
    z = np.empty_like(u)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(1.0 - u[:, a]))
        z[:, a] = r * np.cos(2.0 * np.pi * u[:, b])
        z[:, b] = r * np.sin(2.0 * np.pi * u[:, b])
    return z.ravel()[:n]


def filter_ref(psd, lam, fs=1.0):
    """g_j = (1 - j/lam) irfft(sqrt(S), L)[j], S = P fs / m, S_0 := S_1."""
    psd = np.atleast_2d(psd)
    L = 2 * (psd.shape[1] - 1)
    m = np.full(L // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    out = []
    for P in psd:
        S = P * fs / m
        S[0] = S[1]
        out.append((1.0 - np.arange(lam) / lam) * np.fft.irfft(np.sqrt(S), L)[:lam])
    return np.array(out)


def draw_ref(sizes, g, seed, realization, first_block=0):
    """Block b: the valid part of w_b convolved with [g_{lam-1} .. g_0 .. g_{lam-1}]."""
    lam = g.shape[1]
    out = []
    for b, n in enumerate(sizes):
        w = np_normal(seed, realization, first_block + b, n + 2 * (lam - 1))
        out.append(ss.fftconvolve(w, np.concatenate([g[b][:0:-1], g[b]]), "valid"))
    return out


def symbol(a, nw):
    """a0 + 2 sum_j a_j cos(w j) at w = 2 pi k / nw, k = 0..nw/2."""
    g = np.zeros(nw)
    g[:len(a)] = a
    g[nw - len(a) + 1:] = a[1:][::-1]
    return np.fft.rfft(g).real


def model_psd(L, sigma=1.0, fknee=0.02, alpha=1.5, fs=1.0):
    """One-sided PSD [L/2+1] of the two-sided S(f) = sigma^2 (1 + (fknee/f)^alpha); bin 0 (not used) = bin 1."""
    f = np.fft.rfftfreq(L, 1.0 / fs)
    S = np.empty_like(f)
    S[1:] = sigma ** 2 * (1.0 + (fknee / f[1:]) ** alpha)
    S[0] = S[1]
    m = np.full(L // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    return S * m / fs


def block_psds(nb, L, fs=1.0):
    return np.array([model_psd(L, sigma=0.5 + 0.3 * b, fknee=0.01 * (b + 1) * fs, alpha=1.0 + 0.25 * b, fs=fs)
                     for b in range(nb)])


STREAMS = [(0, 0, 0), (1, 2, 3), (20161202, 7, 1 << 32), ((1 << 40) + 3, 1 << 33, (1 << 63) + 5),
           ((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1)]


# ------------------------------------------------------------------------------- white ------
@pytest.mark.parametrize("seed,realization,block", STREAMS)
def test_uniforms_are_bit_equal_to_numpy(cm, seed, realization, block):
    ref = np_uniform(seed, realization, block, 70000)
    for first, n in ((0, 4096), (0, 1), (0, 65537), (1, 1000), (2, 999), (3, 7), (5, 3), (4, 4), (1021, 65001),
                     (69999, 1), (6, 1), (3, 66997)):
        u = to_host(cm, cm.ns.white_noise(n, seed, realization, block, first=first, kind="uniform"))
        assert u.dtype == np.float64 and u.shape == (n,)
        np.testing.assert_array_equal(u, ref[first:first + n], err_msg=str((first, n)))


def test_streams_differ(cm):
    a = to_host(cm, cm.ns.white_noise(64, 5, kind="uniform"))
    for other in (dict(seed=6), dict(seed=5, realization=1), dict(seed=5, block=1)):
        kw = dict(seed=5)
        kw.update(other)
        assert not np.any(to_host(cm, cm.ns.white_noise(64, kind="uniform", **kw)) == a)


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_chunking_does_not_change_the_stream(cm, kind):
    n = 100003
    whole = to_host(cm, cm.ns.white_noise(n, 11, 3, 9, kind=kind))
    cuts = [0, 1, 2, 5, 9, 4096, 4099, 50001, 50002, 99999, n]
    parts = [to_host(cm, cm.ns.white_noise(b - a, 11, 3, 9, first=a, kind=kind)) for a, b in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(np.concatenate(parts), whole)
    t = cm.ns.white_noise(n, 11, 3, 9, kind=kind)
    assert t.is_cuda and t.dtype == cm.torch.float64
    # an odd first sample: the counter blocks start on an odd double of the output, the 8-byte store path
    odd = to_host(cm, cm.ns.white_noise(n + 1, 11, 3, 9, first=1, kind=kind))
    np.testing.assert_array_equal(odd[:-1], to_host(cm, cm.ns.white_noise(n + 1, 11, 3, 9, kind=kind))[1:])


@pytest.mark.parametrize("seed,realization,block", STREAMS[1:4])
def test_normals_match_the_numpy_restatement(cm, seed, realization, block):
    """|z| <= sqrt(2 53 ln 2) = 8.58; the angle 2 pi u rounded in NumPy gives <= 2 pi 2^-53 8.58 ~ 6e-15, a few
    ulp of log, sqrt, sin, cos the same order: 1e-13 leaves about ten times that."""
    ref = np_normal(seed, realization, block, 200000)
    for first, n in ((0, 200000), (1, 4095), (2, 3), (3, 100000), (7, 1)):
        z = to_host(cm, cm.ns.white_noise(n, seed, realization, block, first=first))
        err = np.max(np.abs(z - ref[first:first + n]))
        print("\nnormals (%d, %d, %d) first %d n %d: max abs error %.3g" % (seed, realization, block, first, n, err))
        assert err <= 1e-13, (first, n, err)


def test_moments_of_the_normals(cm):
    """2^24 draws (restatement on the CPU: mean sqrt(n) = 0.76, var - 1 = 5.4e-4, kurtosis excess 8e-4)."""
    n = 1 << 24
    z = to_host(cm, cm.ns.white_noise(n, 7, 1, 2))
    mean, var = z.mean(), z.var()
    kurt = np.mean((z - mean) ** 4) / var ** 2
    print("\n2^24 normals: mean sqrt(n) %.3f, var - 1 %.3g, kurtosis - 3 %.3g" % (mean * np.sqrt(n), var - 1, kurt - 3))
    assert np.all(np.isfinite(z))
    assert abs(mean) * np.sqrt(n) <= 5.0
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs(kurt - 3.0) <= 5.0 * np.sqrt(24.0 / n)


def test_realisations_and_blocks_are_uncorrelated(cm):
    n = 1 << 22
    a = to_host(cm, cm.ns.white_noise(n, 42, 0, 0))
    for realization, block in ((1, 0), (0, 1), (1, 1)):
        b = to_host(cm, cm.ns.white_noise(n, 42, realization, block))
        c = np.dot(a - a.mean(), b - b.mean()) / (n * a.std() * b.std())
        print("\ncross-correlation with (realization %d, block %d): %.3g (5/sqrt(n) = %.3g)"
              % (realization, block, c, 5 / np.sqrt(n)))
        assert abs(c) < 5.0 / np.sqrt(n), (realization, block, c)


# -------------------------------------------------------------------------------- bands ------
@pytest.mark.parametrize("L", [256, 4096])
@pytest.mark.parametrize("where", ["host", "device"])
def test_colouring_band_matches_the_restatement(cm, L, where):
    fs = 20.0
    psd = block_psds(3, L, fs)
    psd[1] *= 1.0 + 0.5 * np.random.default_rng(L).random(L // 2 + 1)          # not smooth
    for lam in (1, 7, L // 8, L // 2):
        g = cm.ns.noise_filter_bands(psd if where == "host" else to_dev(cm, psd), lam, fsample=fs)
        if where == "device":
            assert g.is_cuda and g.dtype == cm.torch.float64
            g = to_host(cm, g)
        assert isinstance(g, np.ndarray) and g.shape == (3, lam)
        ref = filter_ref(psd, lam, fs)
        for b in range(3):
            assert rel_l2(g[b], ref[b]) <= 1e-12, (lam, b, rel_l2(g[b], ref[b]))
            assert symbol(g[b], 8 * L).min() >= 0.0, (lam, b)
    # zero power is allowed (a band that is zero), one row serves as well as three
    z = cm.ns.noise_filter_bands(np.zeros((1, L // 2 + 1)), 5)
    np.testing.assert_array_equal(z, np.zeros((1, 5)))


def test_negative_or_nan_bin_is_refused_naming_block_and_bin(cm):
    psd = block_psds(3, 1024)
    psd[2, 77] = np.nan
    with pytest.raises(ValueError, match=r"block 2\b.*bin 77\b"):
        cm.ns.noise_filter_bands(psd, 16)
    psd[2, 77] = -1.0
    with pytest.raises(ValueError, match=r"block 2\b.*bin 77\b"):
        cm.ns.noise_filter_bands(to_dev(cm, psd), 16)
    psd[1, 300] = np.inf
    with pytest.raises(ValueError, match=r"block 1\b.*bin 300\b"):
        cm.ns.NoiseSimulator([1000, 1000, 1000], psd, 16)
    psd[1, 300] = 1.0
    psd[2, 77] = 0.0
    cm.ns.noise_filter_bands(psd, 16)


# -------------------------------------------------------------------------------- draws ------
@pytest.mark.parametrize("lam,method", [(1, DIRECT), (2, DIRECT), (64, FUSED), (2049, FUSED), (4096, FFT)])
def test_draw_equals_the_restatement(cm, lam, method):
    sizes = [5000, 12345, 8191]
    L = max(256, 2 * (1 << (lam - 1).bit_length()))
    psd = block_psds(len(sizes), L)
    seed, realization, first_block = 20161202, 5, 1 << 32
    sim = cm.ns.NoiseSimulator(sizes, psd, lam, seed=seed, first_block=first_block)
    info = sim.info()
    assert info["method"] == method and info["nt"] == sum(sizes) and info["lam"] == lam, info
    assert info["padded_samples"] == sum(sizes) + 2 * (lam - 1) * len(sizes)
    y = sim.draw(realization)
    assert y.is_cuda and y.dtype == cm.torch.float64 and y.shape == (sum(sizes),)
    y = to_host(cm, y)
    g = filter_ref(psd, lam)
    assert rel_l2(sim.bands, g) <= 1e-12
    ref = draw_ref(sizes, sim.bands, seed, realization, first_block)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b in range(len(sizes)):
        e = rel_l2(y[off[b]:off[b + 1]], ref[b])
        print("\nlam %d block %d: rel l2 against fftconvolve %.3g" % (lam, b, e))
        assert e <= 1e-12, (lam, b, e)
    # the same realisation again: the same bits; another one: other samples
    np.testing.assert_array_equal(to_host(cm, sim.draw(realization)), y)
    assert not np.any(to_host(cm, sim.draw(realization + 1)) == y)
    # the one-shot form
    np.testing.assert_array_equal(
        to_host(cm, cm.ns.simulate_noise(sizes, psd, lam, seed, realization, first_block=first_block)), y)
    # out given: overwritten, or out + s y
    base = np.random.default_rng(lam).standard_normal(sum(sizes))
    s = -2.5
    for make in (lambda: to_dev(cm, base), lambda: base.copy()):
        out = make()
        res = sim.draw(realization, out=out)
        assert res is out
        np.testing.assert_array_equal(to_host(cm, out), y)
        out = make()
        res = sim.draw(realization, out=out, add=True, scale=s)
        assert res is out
        assert rel_l2(to_host(cm, out), base + s * y) <= 1e-15
    # a PSD shared by all blocks
    shared = cm.ns.NoiseSimulator(sizes, psd[1:2], lam, seed=seed, first_block=first_block)
    ys = to_host(cm, shared.draw(realization))
    one = cm.ns.NoiseSimulator(sizes[1], psd[1:2], lam, seed=seed, first_block=first_block + 1)
    y1 = to_host(cm, one.draw(realization))
    assert rel_l2(ys[off[1]:off[2]], y1) <= 1e-13
    assert rel_l2(y1, draw_ref([sizes[1]], filter_ref(psd[1:2], lam), seed, realization, first_block + 1)[0]) <= 1e-12


def test_equal_blocks_from_nt(cm):
    psd = block_psds(1, 256)
    a = cm.ns.NoiseSimulator(3000, psd, 33, seed=4, nt=12000)
    b = cm.ns.NoiseSimulator([3000] * 4, psd, 33, seed=4)
    np.testing.assert_array_equal(to_host(cm, a.draw(2)), to_host(cm, b.draw(2)))


def test_draws_allocate_nothing_of_tod_size(cm):
    t = cm.torch
    sizes = [1 << 20] * 4
    sim = cm.ns.NoiseSimulator(sizes, block_psds(1, 1024), 256, seed=1)
    out = cm.D.empty(sum(sizes))
    sim.draw(0, out=out)
    t.cuda.synchronize()
    lib0, torch0 = cm.D.memory_info(), t.cuda.memory_allocated()
    t.cuda.reset_peak_memory_stats()
    for r in range(3):
        sim.draw(r, out=out, add=bool(r), scale=0.5)
    t.cuda.synchronize()
    lib1 = cm.D.memory_info()
    assert lib1["live_bytes"] == lib0["live_bytes"] and lib1["driver_allocations"] == lib0["driver_allocations"]
    assert t.cuda.max_memory_allocated() - torch0 < 1 << 20


@pytest.mark.parametrize("lam,exact", [(2, True), (64, True), (2049, True), (4096, False)])
def test_a_shard_draws_the_samples_of_the_whole(cm, lam, exact):
    """Blocks [k0, k1) drawn with first_block = k0.  The direct sum works sample by sample and the fused
    overlap-save kernel cuts its windows per block (a window never spans two blocks, and a block's spectrum
    is computed from its own band alone), so a block's samples do not depend on the other blocks of the
    operator: bit-equal.  Beyond lam = 2049 the operator is rocFFT's, whose transform length follows the
    longest block of the operator and whose kernels may follow the batch count: rel l2 <= 1e-13."""
    sizes = [7000, 20000, 5000, 12345, 9001]
    L = max(256, 2 * (1 << (lam - 1).bit_length()))
    psd = block_psds(len(sizes), L)
    off = np.concatenate([[0], np.cumsum(sizes)])
    base = 1 << 40
    whole = to_host(cm, cm.ns.NoiseSimulator(sizes, psd, lam, seed=9, first_block=base).draw(3))
    for k0, k1 in ((0, 2), (2, 5), (1, 2), (4, 5)):
        part = to_host(cm, cm.ns.NoiseSimulator(sizes[k0:k1], psd[k0:k1], lam, seed=9, first_block=base + k0).draw(3))
        ref = whole[off[k0]:off[k1]]
        if exact:
            np.testing.assert_array_equal(part, ref, err_msg=str((k0, k1)))
        else:
            assert rel_l2(part, ref) <= 1e-13, (k0, k1, rel_l2(part, ref))


# ----------------------------------------------------------------------------- closures ------
def test_spectrum_of_a_draw_is_the_bands_symbol_squared(cm):
    """S = sigma^2 (1 + (0.02/f)^1.5), one block of 2^22 samples, L = 4096, lam = 512: the Welch PSD of the draw
    (Hann, 50 % overlap, K = 2047 segments, no detrend) against m_k/fs |g^(w_k)|^2 over bins 2 .. L/2-1, max
    relative deviation <= 5 sigma_W, sigma_W = sqrt(11/(9K)).  Seed 99: the restatement on the CPU gives
    2.96 sigma_W (RMS 0.93); it is formed here as well and held to the same bound."""
    n, L, lam, seed, sigma = 1 << 22, 4096, 512, 99, 1.0
    psd = model_psd(L, sigma=sigma)[None, :]
    sim = cm.ns.NoiseSimulator(n, psd, lam, seed=seed)
    y = sim.draw(0)
    _, P = cm.nm.noise_psd(y, n, L, detrend=False)
    P = to_host(cm, P)[0]
    m = np.full(L // 2 + 1, 2.0)
    m[0] = m[-1] = 1.0
    expect = m * symbol(sim.bands[0], L) ** 2
    K = (n - L) // (L // 2) + 1
    assert K == 2047
    sw = np.sqrt(11.0 / (9.0 * K))
    dev = np.abs(P[2:L // 2] / expect[2:L // 2] - 1.0)
    yr = draw_ref([n], filter_ref(psd, lam), seed, 0)[0]
    Pr = ss.welch(yr, 1.0, window="hann", nperseg=L, noverlap=L // 2, detrend=False, scaling="density",
                  average="mean")[1]
    devr = np.abs(Pr[2:L // 2] / expect[2:L // 2] - 1.0)
    print("\nspectrum closure: device max %.3f sigma_W (rms %.3f), restatement max %.3f sigma_W"
          % (dev.max() / sw, np.sqrt(np.mean(dev ** 2)) / sw, devr.max() / sw))
    assert devr.max() <= 5.0 * sw
    assert dev.max() <= 5.0 * sw


def test_estimator_recovers_the_band_of_the_model(cm):
    """The bounds of test_recovers_a_known_one_over_f_band: a0 within 1 %, band rel l2 < 3 % (restatement on the
    CPU for seeds 99, 20161202, 5: a0 within 0.3 %, band within 0.8 %)."""
    n, L, lam, sigma = 1 << 22, 4096, 512, 0.7
    psd = model_psd(L, sigma=sigma)[None, :]
    at = cm.nm.inverse_noise_bands(psd, lam)[0]
    for seed in (99, 20161202, 5):
        y = cm.ns.simulate_noise(n, psd, lam, seed)
        N = cm.nm.estimate_inverse_noise(y, n, lam, nperseg=L)
        a = np.asarray(N.covnoise[0])
        print("\nseed %d: a0 %.4f of the model's, band rel l2 %.4f" % (seed, a[0] / at[0], rel_l2(a, at)))
        assert abs(a[0] / at[0] - 1.0) < 0.01, (seed, a[0], at[0])
        assert rel_l2(a, at) < 0.03, (seed, rel_l2(a, at))


def test_gls_map_with_simulated_noise(cm):
    """The construction of test_gls_map_with_the_estimated_band (nside 32 IQU, 4 blocks of 2^20 samples,
    lambda = 256), with the noise drawn on the device and accumulated onto P m_sky."""
    from cosmomap2_amd.interfaces import linearoperators as Lmod
    nb, bs, lam = 4, 1 << 20, 256
    nt, npix = nb * bs, 12 * 32 * 32
    rng = np.random.default_rng(32)
    pairs = rng.integers(0, npix, nt).astype(np.int32)
    phi = rng.uniform(0, np.pi) + (2 * np.pi * 2.5 / 200.0) * np.arange(nt)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=3, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nt, pairs, pol=3, angle_processed=ces)
    M = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=3)
    m_sky = rng.standard_normal(3 * n) * np.tile([10.0, 1.0, 1.0], n)
    Lm = 4 * lam
    psd = model_psd(Lm)[None, :]
    sim = cm.ns.NoiseSimulator(bs, psd, Lm // 2, seed=32, nt=nt)
    d_dev = to_dev(cm, P * m_sky)
    assert sim.draw(0, out=d_dev, add=True) is d_dev
    d = to_host(cm, d_dev)
    r = d - P * (M * (P.T * d))
    N_est = cm.nm.estimate_inverse_noise(r, bs, lam)
    N_true = cm.I.BlockLO(bs, [cm.nm.inverse_noise_bands(psd, lam)[0]] * nb, offdiag=True)
    assert Lmod._use_tiles(P)
    res = {}
    for name, N in (("est", N_est), ("true", N_true)):
        A = P.T * N * P
        b = P.T * N * d
        its = []
        m, info = cm.cg(A, b, M=M, rtol=1e-6, maxiter=500, callback=lambda xk: its.append(1))
        assert info == 0, name
        res[name] = (len(its), np.linalg.norm(m - m_sky))
    print("\nGLS map, simulated noise: estimated band %d iterations, |m - m_sky| %.6g; true band %d iterations, %.6g"
          % (res["est"][0], res["est"][1], res["true"][0], res["true"][1]))
    assert abs(res["est"][0] - res["true"][0]) <= 1, res
    assert res["est"][1] <= 1.02 * res["true"][1], res


def test_draw_of_1e8_samples_is_not_a_host_path(cm):
    """1e8 samples (100 blocks of 1e6), lambda = 2048, drawn into a kept tensor, warm, best of 3, against the
    NumPy restatement (Philox normals and fftconvolve) of 2^22 samples on one host core: the GPU's time per
    sample must be at least 10 times smaller.  A host fallback would sit near 1x; the kernels are projected at
    about 1000x, and ten separates the two on any machine."""
    t = cm.torch
    nb, bs, lam, L = 100, 1000000, 2048, 4096
    psd = model_psd(L)[None, :]
    sim = cm.ns.NoiseSimulator(bs, psd, lam, seed=8, nt=nb * bs)
    assert sim.info()["method"] == FUSED
    out = cm.D.empty(nb * bs)
    sim.draw(0, out=out)
    t.cuda.synchronize()
    times = []
    for r in range(3):
        t0 = time.perf_counter()
        sim.draw(r + 1, out=out)
        t.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    nh = 1 << 22
    g = sim.bands
    t0 = time.perf_counter()
    w = np_normal(8, 0, 0, nh + 2 * (lam - 1))
    t1 = time.perf_counter()
    ss.fftconvolve(w, np.concatenate([g[0][:0:-1], g[0]]), "valid")
    t2 = time.perf_counter()
    gpu, host = min(times) / (nb * bs), (t2 - t0) / nh
    print("\ndraw, 1e8 samples in HBM, 100 blocks, lambda 2048: %s ms; host restatement of 2^22 samples: "
          "normals %.3f s, convolution %.3f s; per sample GPU %.3g ns, host %.3g ns, ratio %.0f"
          % (", ".join("%.2f" % (1e3 * s) for s in times), t1 - t0, t2 - t1, 1e9 * gpu, 1e9 * host, host / gpu))
    assert out.is_cuda and np.isfinite(float(out[::100003].sum()))
    assert gpu * 10.0 <= host, (gpu, host)
    del out
