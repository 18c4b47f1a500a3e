"""
The references, restatements and bounds of tests/_noise_model_ref.py, checked without a GPU: the extended
references against SciPy and NumPy, the stored constants against what is measured now, every mutation of the
restatements against the check that tests/test_gpu_noise_model_kernels.py applies, and the batch geometry
that the PSD cases were chosen for.
"""
import os
import sys

import numpy as np
import pytest
import scipy.signal as ss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_model_ref as R  # noqa: E402
from conftest import rel_l2  # noqa: E402


def test_cases_are_what_they_claim():
    assert R.seg_counts(R.PSD_SIZES[256], 256) == [1, 1, 2, 2, 3, 9, 1]
    assert R.seg_offsets(R.PSD_SIZES[256], 256).tolist() == [0, 1, 2, 4, 6, 9, 18, 19]
    assert R.tails(R.PSD_SIZES[256], 256) == [0, 127, 0, 127, 0, 120, 0]
    assert R.seg_counts(R.PSD_SIZES[512], 512) == [1, 3, 4] and R.tails(R.PSD_SIZES[512], 512) == [0, 255, 0]
    assert sum(R.PSD_SIZES[256]) == 3702 and sum(R.PSD_SIZES[512]) == 3071
    # L + L/2 - 1 (one segment, the longest tail), L + L/2 (two segments), 2 L - 1
    assert {256, 256 + 127, 256 + 128, 511} <= set(R.PSD_SIZES[256])
    assert len(R.psd_keys()) == 2 * 5 * 2 * 2
    for L in (256, 512):
        for detrend in (True, False):
            dr = R.dynamic_range(R.psd_case(L, "red", detrend, 1.0))
            assert dr.min() >= 1e6, (L, detrend, dr)
        # the tone is on its bin: all but three bins of every block are 1e-25 of it or less
        p = np.asarray(R.psd_case(L, "tone", False, 1.0).ref, dtype=np.float64)
        k0 = R.TONE_BIN[L]
        far = np.ones(L // 2 + 1, dtype=bool)
        far[k0 - 1:k0 + 2] = False
        assert (p[:, far].max(axis=1) <= 1e-25 * p[:, k0]).all()
        # impulses: every one sits in a tail or where the window of each segment that holds it is >= 1/2
        off, half = R.offsets(R.PSD_SIZES[L]), L // 2
        w = np.asarray(R.hann_ld(L), dtype=np.float64)
        in_tail = 0
        for b, (places, K) in enumerate(zip(R.IMPULSES[L], R.seg_counts(R.PSD_SIZES[L], L))):
            for p_ in places:
                assert 0 <= p_ < R.PSD_SIZES[L][b]
                segs = [s for s in range(K) if s * half <= p_ < s * half + L]
                in_tail += not segs
                assert all(w[p_ - s * half] >= 0.5 for s in segs), (L, b, p_)
        assert in_tail >= 2
    # block 1 of the L = 256 impulses has its only impulse in the tail: reference and bound are exactly zero
    cs = R.psd_case(256, "impulses", True, 1.0)
    assert not cs.ref[1].any() and not R.psd_bound(cs.parts, 256, 1.0, 256)[1].any() and cs.ref[0].all()
    # band cases: thread counts of k_bands_lags, one-bin PSDs
    assert [R.BAND_NB * lam for lam in R.BAND_LAMS] == [3, 6, 21, 384] and 384 > R.K_BLOCK > 21
    assert sorted(k for v in R.ONE_BINS.values() for k in v) == [1, 2, 63, 64, 127, 128]
    for name in R.ONE_BINS:
        a = np.asarray(R.band_case(name, R.SQRT, 128).ref, dtype=np.float64)
        assert np.isfinite(a).all()
    a = np.asarray(R.band_case("onebin_b", R.SQRT, 128).ref)          # k0 = 64: cos = 0 at every odd lag
    assert not a[0, 1::2].any() and a[0, 0::2][:-1].all()


def test_welch_reference_agrees_with_scipy():
    """per bin, on `white`: |ref - scipy| <= 1e-13 scipy"""
    for L in (256, 512):
        for detrend in (True, False):
            for fs in R.PSD_FS:
                cs = R.psd_case(L, "white", detrend, fs)
                off = R.offsets(cs.sizes)
                for b in range(len(cs.sizes)):
                    _, p = ss.welch(cs.x[off[b]:off[b + 1]], fs, window="hann", nperseg=L, noverlap=L // 2,
                                    detrend="constant" if detrend else False, scaling="density", average="mean")
                    err = np.max(np.abs(np.asarray(cs.ref[b], dtype=np.float64) - p) / p)
                    assert err <= 1e-13, (L, detrend, fs, b, err)


def test_band_reference_agrees_with_numpy():
    """in the norm: rel_l2 <= 1e-13 against (1 - j/lam) irfft(G, L)[j]"""
    for name in ("red", "rough"):
        for mode in R.MODES:
            for lam in R.BAND_LAMS:
                cs = R.band_case(name, mode, lam)
                L = R.BAND_L
                S = cs.psd * cs.fs / R.m_of(L)
                S[:, 0] = S[:, 1]
                G = 1.0 / S if mode == R.INVERSE else np.sqrt(S)
                want = (1.0 - np.arange(lam) / lam) * np.fft.irfft(G, L, axis=1)[:, :lam]
                for b in range(R.BAND_NB):
                    assert rel_l2(np.asarray(cs.ref[b], dtype=np.float64), want[b]) <= 1e-13, (name, mode, lam, b)


def test_bin_zero_is_never_read_by_the_references():
    for v in R.GARBAGE:
        for mode in R.MODES:
            cs = R.band_case("red", mode, 7)
            P = R.with_bin0(cs.psd, v)
            R.assert_bit_equal(np.asarray(R.bands_ref(P, 7, cs.fs, mode)[0], dtype=np.float64),
                               np.asarray(cs.ref, dtype=np.float64), "reference, bin 0 = %r" % v)
            R.assert_bit_equal(R.bands_f64(P, 7, cs.fs, mode), R.bands_f64(cs.psd, 7, cs.fs, mode),
                               "restatement, bin 0 = %r" % v)


def test_psd_constants_are_fresh_and_the_restatement_meets_its_bounds():
    worst = R.measure_worst_psd()
    print("welch_f64: largest |restatement - ref| / E(c = 1) per (L, detrend): %s; c = %s"
          % ({k: round(v, 2) for k, v in sorted(worst.items())}, {k: R.c_psd(*k) for k in sorted(worst)}))
    assert {k: R.round_up(v) for k, v in worst.items()} == R.WORST_PSD, "WORST_PSD is stale"
    for key in R.psd_keys():
        cs = R.psd_case(*key)
        got = R.welch_f64(cs.x, cs.sizes, cs.L, cs.fs, cs.detrend)
        assert R.psd_share(got, cs, c=R.WORST_PSD[(cs.L, cs.detrend)]) <= 1.0, key      # c = 1 x its own share
        assert R.psd_share(got, cs) <= 1.0 / 8.0, key
    assert {k: R.c_psd(*k) for k in R.WORST_PSD} == {(256, True): 256, (256, False): 256, (512, True): 1024,
                                                      (512, False): 1024}


def test_lag_constant_and_the_restatement():
    assert R.C_LAG(256) == 139 and R.C_LAG(512) == 267
    worst = R.measure_worst_lag()
    print("bands_f64: largest share of C_LAG 2^-53 B_j per mode: %s"
          % {R.MODE_NAMES[k]: round(v, 4) for k, v in sorted(worst.items())})
    assert {k: R.round_up2(v) for k, v in worst.items()} == R.WORST_LAG, "WORST_LAG is stale"
    assert max(worst.values()) <= 1.0


def test_zero_bins_in_sqrt_mode():
    """S = 0 is allowed: finite bands; an all-zero PSD gives exact zeros and a zero bound"""
    P = np.zeros((1, R.BAND_L // 2 + 1))
    ref, B = R.bands_ref(P, 7, 1.0, R.SQRT)
    assert not ref.any() and not B.any() and not R.bands_f64(P, 7, 1.0, R.SQRT).any()


@pytest.mark.parametrize("name", sorted(R.PSD_MUTATIONS))
def test_every_psd_mutation_fails_its_check(name):
    cs = R.psd_case(*R.PSD_MUTATIONS[name])
    good = R.welch_f64(cs.x, cs.sizes, cs.L, cs.fs, cs.detrend)
    bad = R.welch_f64(cs.x, cs.sizes, cs.L, cs.fs, cs.detrend, mut=name)
    assert R.psd_share(good, cs) <= 1.0 / 8.0
    factor = R.psd_share(bad, cs)
    print("%s on %r: x %.3g the bound" % (name, R.PSD_MUTATIONS[name], factor))
    assert factor >= 100.0, "%s: only %.3g x the bound" % (name, factor)


@pytest.mark.parametrize("name", sorted(R.BAND_MUTATIONS))
def test_every_band_mutation_fails_its_check(name):
    cs = R.band_case(*R.BAND_MUTATIONS[name])
    assert R.band_share(R.bands_f64(cs.psd, cs.lam, cs.fs, cs.mode), cs) <= 1.0
    factor = R.band_share(R.bands_f64(cs.psd, cs.lam, cs.fs, cs.mode, mut=name), cs)
    print("%s on %r: x %.3g the bound" % (name, R.BAND_MUTATIONS[name], factor))
    assert factor >= 100.0, "%s: only %.3g x the bound" % (name, factor)


def test_the_mutations_are_there():
    assert len(R.PSD_MUTATIONS) == 8 and len(R.BAND_MUTATIONS) == 5


def test_subtle_psd_error_is_seen_by_the_bound_and_not_by_the_norm():
    """1e-8 on the bins k >= L/4 of `red`: beyond the bound, and rel_l2 < 1e-12 over each block does not notice"""
    cs = R.psd_case(*R.SUBTLE_PSD_CASE)
    good = R.welch_f64(cs.x, cs.sizes, cs.L, cs.fs, cs.detrend)
    bad = R.subtle_psd(good, cs.L)
    ref = np.asarray(cs.ref, dtype=np.float64)
    norms = [rel_l2(bad[b], ref[b]) for b in range(len(cs.sizes))]
    factor = R.psd_share(bad, cs)
    print("subtle PSD error: x %.3g the bound (c = %d); rel_l2 per block at most %.3g"
          % (factor, R.c_psd(cs.L, cs.detrend), max(norms)))
    assert R.psd_share(good, cs) <= 1.0 / 8.0 and factor > 1.0
    assert max(norms) < 1e-12, norms


def test_subtle_band_error():
    """1e-9 on the lags j >= lambda/2 of the `red` band at lambda = 128: beyond the bound over the case (on the
    block with the knee at 0.01 fs).  Per block it is 0.044, 0.48 and 52 of the bound (knees 0.1, 0.03, 0.01):
    with the knee at 0.1 fs the far lags are 1e-7 of B_j and a relative error of 1e-9 of them lies below the
    rounding of the sum itself.  rel_l2 <= 1e-11 over the band does not notice any of it."""
    cs = R.band_case(*R.SUBTLE_BAND_CASE)
    good = R.bands_f64(cs.psd, cs.lam, cs.fs, cs.mode)
    bad = R.subtle_band(good)
    bound = R.LD(R.C_LAG(R.BAND_L)) * R.U53 * cs.B
    per_block = [R.ratio(bad[b], cs.ref[b], bound[b]) for b in range(R.BAND_NB)]
    norm = rel_l2(bad, np.asarray(cs.ref, dtype=np.float64))
    print("subtle band error: x %s the bound per block (knees %r); rel_l2 %.3g: rel_l2 <= 1e-11 would %s"
          % (["%.3g" % f for f in per_block], R.RED_KNEES, norm,
             "NOT have noticed" if norm <= 1e-11 else "have noticed"))
    assert R.band_share(good, cs) <= 1.0 and R.band_share(bad, cs) > 1.0
    assert per_block[2] > 10.0 and per_block[0] < 1.0
    assert norm <= 1e-11


def test_batch_geometry():
    sizes, L = R.PSD_SIZES[256], 256
    geo = R.batch_geometry(sizes, L, 1)
    assert len(geo) == 19 and all(bt.real == 1 and bt.pad == 0 and len(bt.blocks) == 1 for bt in geo)
    assert R.geometry_facts(sizes, L, 1) == dict(straddle=True, boundary_on_block=True, two_whole=False,
                                                 padded_last=False)
    for B in (2, 3, 4):
        facts = R.geometry_facts(sizes, L, B)
        assert all(facts.values()), (B, facts)
        geo = R.batch_geometry(sizes, L, B)
        assert sum(bt.real for bt in geo) == 19 and geo[-1].pad == B - 19 % B
        # every segment of every block is added exactly once, in order
        seen = {}
        for bt in geo:
            for b, s0, s1 in bt.blocks:
                seen.setdefault(b, []).extend(range(s0, s1))
        so = R.seg_offsets(sizes, L)
        assert all(seen[b] == list(range(so[b], so[b + 1])) for b in range(len(sizes)))
    geo = R.batch_geometry(sizes, L, 3)
    assert geo[0].blocks == [(0, 0, 1), (1, 1, 2), (2, 2, 3)] and geo[0].whole == [0, 1]
    assert geo[1].blocks == [(2, 3, 4), (3, 4, 6)] and geo[1].whole == [3]
    assert geo[-1] == R.Batch(18, 1, 2, [(6, 18, 19)], [6])
    big = R.batch_geometry(sizes, L, R.K_BATCH_SAMPLES // L)               # the default: one batch
    assert len(big) == 1 and big[0].pad == 65536 - 19 and big[0].whole == list(range(7))
    assert R.per_segment_bytes(256) == 2048 + 16 * 129
