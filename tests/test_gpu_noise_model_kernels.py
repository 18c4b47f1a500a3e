"""
The noise-model kernels (csrc/cm2_noise_model.hip, csrc/cm2_psd_bands.h) against the references of
tests/_noise_model_ref.py, bin by bin and lag by lag, through the C entry points.

Conventions of every case: the stream, the PSD and the bands are the middle of a larger buffer pre-filled with
a sentinel whose bits must be unchanged after the call, and an output holds NaN before the call.  A PSD is
accepted when |got - ref| <= E_{b,k} for EVERY bin (E from the windowed raw segments, c from the float64
restatement), a band when |got - ref| <= C_LAG 2^-53 B_j for every lag; where a bound is 0 the result must be
exactly 0.  Across batch sizes only the bound is promised; at one batch size a block alone has the bits of
the same block inside a group.

Kernels and the case that reaches them (to be kept in step with the code by hand):

  k_psd_pack          one sample per thread (L = 256)   test_psd_every_bin[256-*]: blocks of L, L + L/2 - 1 (one
                                                        segment, the longest ignored tail), L + L/2 (two), 2 L - 1,
                                                        2 L, 1400 (nine), L again
                      two samples per thread (L = 512)  test_psd_every_bin[512-*]: 1, 3, 4 segments
                      detrend on / off                  [*-detrend-*] / [*-raw-*]; the mean against 1e6: `offset`
                      zero segments (g >= nseg)         [*-default] (65536 | 32768 per batch, 19 | 8 of them real),
                                                        [*-middle] (the padded last batch)
                      a tail is never read              test_tails_are_never_read, the tail impulses of `impulses`
                      the last segment stays in its block
                                                        test_blocks_alone_and_twice (guards behind a block alone),
                                                        test_a_nan_stays_in_its_block
  k_psd_accumulate    one batch holds every block       [*-default]
                      one segment per batch             [*-one]: every sum goes through the output 19 | 8 times
                      a block across a batch boundary, a boundary on a block boundary, several whole blocks in a
                      batch                             [256-*-middle] (2 to 4 segments per batch, asserted on the
                                                        geometry of the size the handle reports)
  k_psd_finish        fs = 1, 20; K_b = 1 .. 9          every PSD case
  exact zeros                                           test_constant_block_gives_exact_zeros; block 1 of the
                                                        L = 256 `impulses` (nothing but a tail impulse)
  k_bands_spectrum<0> (1/S), k_bands_spectrum<1> (sqrt(S)), spectrum_at
                      S_0 := S_1, bin 0 never read      test_bands_every_lag (bin 0 = NaN, -1, +inf)
                      m = 1 at the Nyquist bin          the one-bin PSD at k0 = 128
                      S = 0 under sqrt                  the one-bin PSDs; test_zero_psd_under_sqrt
                      the refusals, the smallest flat index
                                                        test_refusals, test_overflowing_inverse_is_refused
  k_bands_cos_table, k_bands_lags (cos_sum)
                      3, 6, 21 threads; 384 (a second workgroup with a guarded remainder)
                                                        test_bands_every_lag[*-1 | 2 | 7 | 128]
                      every branch of the phase walk, the Nyquist sign, exact zeros where cos = 0
                                                        the one-bin PSDs at k0 = 1, 2, 63, 64, 127, 128
                      a block alone                     test_single_block_is_bit_equal_to_its_row
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_model_ref as R  # noqa: E402
from _guarded import Guarded  # noqa: E402
from conftest import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.utilities import noise_model, noise_sim
    return SimpleNamespace(D=device, hip=_hip, torch=torch, nm=noise_model, ns=noise_sim)


# ============================================================================ PSD ===
SETTINGS = ("default", "one", "middle")


def work_bytes_of(setting, L):
    """default: the library's cap; one: a byte, which gives one segment per batch; middle: four segments' worth"""
    return {"default": None, "one": 1, "middle": 4 * R.per_segment_bytes(L)}[setting]


class Welch(object):
    """cm2_psd_create and cm2_psd_welch on guarded buffers"""

    def __init__(self, cm, L, detrend, setting):
        self.cm, self.L, self.setting = cm, L, setting
        self.h = cm.nm._Psd(L, int(bool(detrend)), work_bytes_of(setting, L))
        info = self.h.info()
        assert info["nperseg"] == L
        self.B = info["segments_per_batch"]
        if setting == "one":
            assert self.B == 1, "work_bytes = 1 gave %d segments per batch" % self.B
        elif setting == "middle":
            assert 2 <= self.B <= 4, "four segments' worth of workspace gave %d segments per batch" % self.B
        else:
            assert self.B >= 1024 and (R.K_BATCH_SAMPLES // L) % self.B == 0, \
                "the default workspace gave %d segments per batch" % self.B

    def __call__(self, x, sizes, fs, what, nan_allowed=False):
        cm, nb, nfreq = self.cm, len(sizes), self.L // 2 + 1
        assert len(x) == sum(sizes)
        x = np.array(x, dtype=np.float64)                  # (the shared cases are read-only)
        gin, out = Guarded(cm, len(x), x), Guarded(cm, nb * nfreq)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        cm.hip.call("cm2_psd_welch", self.h.h, gin.ptr, sz.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nb,
                    float(fs), out.ptr, cm.D.stream())
        got = out.get().reshape(nb, nfreq)
        out.intact(what)
        gin.intact(what + " (the stream)")
        R.assert_bit_equal(gin.get(), x, what + ": the stream")
        if not nan_allowed:
            assert not np.isnan(got).any(), what + ": a NaN is left"
        return got


def _psd_params():
    return [pytest.param(L, d, s, id="%d-%s-%s" % (L, "detrend" if d else "raw", s))
            for L in sorted(R.PSD_SIZES) for d in (True, False) for s in SETTINGS]


@pytest.mark.parametrize("L,detrend,setting", _psd_params())
def test_psd_every_bin(cm, L, detrend, setting):
    welch = Welch(cm, L, detrend, setting)
    if setting == "middle" and L == 256:
        facts = R.geometry_facts(R.PSD_SIZES[L], L, welch.B)
        assert all(facts.values()), (welch.B, facts)
    worst = {}
    for key in R.psd_keys(L, detrend):
        cs = R.psd_case(*key)
        what = "L %d %s fs %g %s, %d segments per batch" % (L, cs.inp, cs.fs, "detrend" if detrend else "raw", welch.B)
        e = R.psd_share(welch(cs.x, cs.sizes, cs.fs, what), cs)
        worst[cs.inp] = max(worst.get(cs.inp, 0.0), e)
        assert e <= 1.0, "%s: |got - ref| is %.3g x the bound E (c = %d)" % (what, e, R.c_psd(L, detrend))
    print("PSD L %d %s, %s (%d segments per batch): largest share of the bound %.3g (c = %d); per input %s"
          % (L, "detrend" if detrend else "raw", setting, welch.B, max(worst.values()), R.c_psd(L, detrend),
             {k: float("%.3g" % v) for k, v in worst.items()}))


def _poisoned(L, inp="red"):
    """-> the stream, the stream with its ignored tails as NaN"""
    sizes = R.PSD_SIZES[L]
    x = R.psd_input(L, inp)
    y = x.copy()
    off = R.offsets(sizes)
    for b, t in enumerate(R.tails(sizes, L)):
        if t:
            y[off[b + 1] - t:off[b + 1]] = np.nan
    assert np.isnan(y).sum() == sum(R.tails(sizes, L)) > 0
    return x, y


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("L", sorted(R.PSD_SIZES))
def test_blocks_alone_and_twice(cm, L, setting):
    """At one batch size: two calls agree bit for bit, and every block alone (its own guarded buffer: whatever
    its last segment read behind it would be a NaN) has the bits of the block inside the group."""
    sizes = R.PSD_SIZES[L]
    off = R.offsets(sizes)
    for detrend in (True, False):
        welch = Welch(cm, L, detrend, setting)
        x = R.psd_input(L, "red")
        what = "L %d %s %s" % (L, "detrend" if detrend else "raw", setting)
        group = welch(x, sizes, 20.0, what)
        R.assert_bit_equal(welch(x, sizes, 20.0, what), group, what + ": the second call")
        for b, n in enumerate(sizes):
            alone = welch(x[off[b]:off[b + 1]], [n], 20.0, "%s, block %d alone" % (what, b))
            R.assert_bit_equal(alone[0], group[b], "%s: block %d alone" % (what, b))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("L", sorted(R.PSD_SIZES))
def test_tails_are_never_read(cm, L, setting):
    sizes = R.PSD_SIZES[L]
    for detrend in (True, False):
        welch = Welch(cm, L, detrend, setting)
        x, y = _poisoned(L)
        what = "L %d %s %s" % (L, "detrend" if detrend else "raw", setting)
        R.assert_bit_equal(welch(y, sizes, 1.0, what + ", tails of NaN"), welch(x, sizes, 1.0, what),
                           what + ": tails of NaN")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("L", sorted(R.PSD_SIZES))
def test_a_nan_stays_in_its_block(cm, L, setting):
    """a NaN in a used sample of block 2 (in its first two segments where it has two)"""
    sizes = R.PSD_SIZES[L]
    off = R.offsets(sizes)
    for detrend in (True, False):
        welch = Welch(cm, L, detrend, setting)
        x = R.psd_input(L, "white")
        y = x.copy()
        y[off[2] + L // 2 + 9] = np.nan
        what = "L %d %s %s" % (L, "detrend" if detrend else "raw", setting)
        clean, got = welch(x, sizes, 1.0, what), welch(y, sizes, 1.0, what + ", a NaN in block 2", nan_allowed=True)
        for b in range(len(sizes)):
            if b != 2:
                R.assert_bit_equal(got[b], clean[b], "%s: block %d beside the NaN" % (what, b))
        assert not np.isfinite(got[2]).any(), what + ": block 2 has finite bins"


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("L", sorted(R.PSD_SIZES))
def test_constant_block_gives_exact_zeros(cm, L, setting):
    """under detrend; the constants have few bits, so that the tree's sum of them is exact"""
    sizes = R.PSD_SIZES[L]
    off = R.offsets(sizes)
    welch = Welch(cm, L, True, setting)
    x = R.psd_input(L, "white").copy()
    consts = {1: 2.5, len(sizes) - 2: -3.0e5}
    for b, v in consts.items():
        x[off[b]:off[b + 1]] = v
    got = welch(x, sizes, 20.0, "L %d %s, constant blocks" % (L, setting))
    for b in range(len(sizes)):
        if b in consts:
            assert not got[b].any(), (L, setting, b, got[b][np.flatnonzero(got[b])[:4]])
        else:
            assert (got[b, 1:] > 0).all()


def test_subtle_error_on_the_gpu_result(cm):
    """The GPU's PSD of `red` times 1 + 1e-8 on the bins k >= L/4 (a copy, multiplied on the host): beyond the
    bound, while rel_l2 <= 1e-12 over each block still passes."""
    cs = R.psd_case(*R.SUBTLE_PSD_CASE)
    got = Welch(cm, cs.L, cs.detrend, "default")(cs.x, cs.sizes, cs.fs, "red")
    bad = R.subtle_psd(got, cs.L)
    ref = np.asarray(cs.ref, dtype=np.float64)
    norms = [rel_l2(bad[b], ref[b]) for b in range(len(cs.sizes))]
    good_share, bad_share = R.psd_share(got, cs), R.psd_share(bad, cs)
    print("subtle PSD error on the GPU result: %.3g -> %.3g x the bound; rel_l2 per block at most %.3g"
          % (good_share, bad_share, max(norms)))
    assert good_share <= 1.0 < bad_share
    assert max(norms) <= 1e-12, norms


# ========================================================================== bands ===
ENTRY = {R.INVERSE: "cm2_noise_bands_from_psd", R.SQRT: "cm2_noise_filter_from_psd"}


def bands_c(cm, psd, lam, fs, mode, what):
    """the C entry point on guarded buffers -> [nb, lam]"""
    psd = np.array(np.atleast_2d(psd), dtype=np.float64)
    nb, L = psd.shape[0], 2 * (psd.shape[1] - 1)
    gin, out = Guarded(cm, psd.size, psd), Guarded(cm, nb * lam)
    try:
        cm.hip.call(ENTRY[mode], gin.ptr, nb, L, float(fs), int(lam), out.ptr, cm.D.stream())
    finally:
        got = out.get().reshape(nb, lam)
        out.intact(what)
        gin.intact(what + " (the PSD)")
        R.assert_bit_equal(gin.get(), psd.reshape(-1), what + ": the PSD")
    return got


def bands_py(cm, psd, lam, fs, mode):
    fn = cm.nm.inverse_noise_bands if mode == R.INVERSE else cm.ns.noise_filter_bands
    return fn(np.array(psd), lam, fsample=fs)


@pytest.mark.parametrize("lam", R.BAND_LAMS)
@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
def test_bands_every_lag(cm, mode, lam):
    worst = {}
    for name in R.BAND_PSDS:
        cs = R.band_case(name, mode, lam)
        what = "%s bands of `%s`, lambda %d" % (R.MODE_NAMES[mode], name, lam)
        got = bands_c(cm, cs.psd, lam, cs.fs, mode, what)
        assert not np.isnan(got).any(), what + ": a NaN is left"
        worst[name] = R.band_share(got, cs)
        assert worst[name] <= 1.0, "%s: |got - ref| is %.3g x the bound (C_LAG = %d)" % (what, worst[name],
                                                                                       R.C_LAG(R.BAND_L))
        if mode == R.SQRT and name in R.ONE_BINS:                 # where cos = 0 the lag is an exact zero
            zero = np.asarray(cs.ref == 0)
            assert zero[:, 0].sum() == 0 and not got[zero].any(), what
        R.assert_bit_equal(bands_py(cm, cs.psd, lam, cs.fs, mode), got, what + ": the Python layer")
        for v in R.GARBAGE:                                       # bin 0 is not used: no refusal, the same bits
            P = R.with_bin0(cs.psd, v)
            R.assert_bit_equal(bands_c(cm, P, lam, cs.fs, mode, what), got, "%s, bin 0 = %r" % (what, v))
            R.assert_bit_equal(bands_py(cm, P, lam, cs.fs, mode), got, "%s, bin 0 = %r, the Python layer" % (what, v))
    print("%s bands, lambda %d: largest share of the bound %.3g (C_LAG = %d); per PSD %s"
          % (R.MODE_NAMES[mode], lam, max(worst.values()), R.C_LAG(R.BAND_L),
             {k: float("%.3g" % v) for k, v in worst.items()}))


def test_zero_psd_under_sqrt(cm):
    """zero bins are allowed (the one-bin cases above are finite); an all-zero PSD gives exact zeros"""
    P = np.zeros((2, R.BAND_L // 2 + 1))
    for lam in (1, 128):
        assert not bands_c(cm, P, lam, 1.0, R.SQRT, "all-zero PSD").any()
    got = bands_c(cm, R.band_psd("onebin_b", R.SQRT), 128, 1.0, R.SQRT, "one-bin PSDs")
    assert np.isfinite(got).all()


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
def test_single_block_is_bit_equal_to_its_row(cm, mode):
    for name in ("red", "rough"):
        cs = R.band_case(name, mode, 128)
        for lam in (7, 128):
            three = bands_c(cm, cs.psd, lam, cs.fs, mode, name)
            alone = bands_c(cm, cs.psd[2:3], lam, cs.fs, mode, name)
            R.assert_bit_equal(alone[0], three[2], "%s lambda %d" % (name, lam))
            R.assert_bit_equal(bands_c(cm, cs.psd, lam, cs.fs, mode, name), three, "%s: the second call" % name)


def _refused(cm, P, lam, fs, mode, match):
    """the C entry refuses with an argument error that names block and bin, and leaves the bands untouched; the
    Python layer raises ValueError with the same words"""
    nb, L = P.shape[0], 2 * (P.shape[1] - 1)
    gin, out = Guarded(cm, P.size, P), Guarded(cm, nb * lam)
    with pytest.raises(cm.hip.HipError, match=match) as ei:
        cm.hip.call(ENTRY[mode], gin.ptr, nb, L, float(fs), int(lam), out.ptr, cm.D.stream())
    assert ei.value.status == cm.hip.ERR_ARGUMENT
    assert np.isnan(out.get()).all(), "a refused call wrote to the bands"
    out.intact("refused call")
    gin.intact("refused call (the PSD)")
    with pytest.raises(ValueError, match=match):
        bands_py(cm, P, lam, fs, mode)


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
def test_refusals(cm, mode):
    clean = R.band_psd("red", mode)
    for bad in (-1.0, float("nan"), float("inf")) + ((0.0,) if mode == R.INVERSE else ()):
        P = clean.copy()                                          # the smallest flat index wins
        P[2, 5] = P[1, 100] = bad
        _refused(cm, P, 7, 1.0, mode, r"block 1\b.*bin 100\b")
        P = clean.copy()                                          # bin 1 is read for bin 0 too: named as bin 1
        P[0, 1] = bad
        _refused(cm, P, 7, 1.0, mode, r"block 0\b.*bin 1\b")
        P = clean.copy()
        P[2, 128] = bad
        _refused(cm, P, 128, 20.0, mode, r"block 2\b.*bin 128\b")


def test_overflowing_inverse_is_refused(cm):
    """S = 2.5e-310 is positive and finite, 1 / S is not: refused like a non-positive bin.  The square root of
    the same PSD is an ordinary colouring band."""
    P = R.band_psd("red", R.INVERSE).copy()
    P[1, 40] = 5e-310
    _refused(cm, P, 7, 1.0, R.INVERSE, r"block 1\b.*bin 40\b")
    got = bands_c(cm, P, 7, 1.0, R.SQRT, "sqrt of a subnormal bin")
    ref, B = R.bands_ref(P, 7, 1.0, R.SQRT)
    assert R.ratio(got, ref, R.LD(R.C_LAG(R.BAND_L)) * R.U53 * B) <= 1.0
