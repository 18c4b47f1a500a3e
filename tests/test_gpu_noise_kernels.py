"""
Every route of the inverse noise operator N^-1 (csrc/cm2_noise.hip, csrc/cm2_overlap_save.hip) against the
references of tests/_noise_ref.py, element by element.

Conventions of every case: each input, output and tile-order buffer is the middle of a larger buffer
pre-filled with a sentinel whose bits must be unchanged after the call, and an output holds NaN before the
call: a sample nobody wrote stays NaN.  The FFT routes are accepted when |got - ref| <= c 2^-53 B_i for
EVERY element (B_i: the window's error scale, c from the float64 restatement: tests/_noise_ref.py); where
B_i = 0 the result must be exactly 0.  The direct and the diagonal kernels must equal their float64
restatement bit for bit.  On a tile order the reference gets the input with the flagged samples as zeros,
the comparison runs over the unflagged samples and the flagged ones must come back as exact zeros.

Kernels and the case that reaches them (to be kept in step with the dispatch code by hand):

  k_os_real<0, flat>        time order            test_fused_time_order: E1 (15 windows: 16 workgroups, one
                                                  exits; blocks of 1, 2, RLEN -1/0/+1, HOP -1/0/+1, HALO
                                                  -1/0/+1, 2 HOP + 1 samples), E2 (blocks shorter than the
                                                  band, lambda - 1 = the kernel's halo, a second window of
                                                  one sample), E3 (5 samples), E8 (8 windows), E9 (9)
  k_os_real<1, BUF | flat>  plain lists           test_fused_tile_order[plain-*]; [auto-2100], [sort-plain]
  k_os_real<2, BUF | flat>  run-coded lists       test_fused_tile_order[rc-*]; [auto-100], [sort-rc],
                                                  [one-pixel] (one run per list), [first-last]
  k_os_real<3, BUF | flat>  inverse lists         test_fused_tile_order[inv-*]; [auto-800], [block]
    a result list without a valid entry           [*-randomwin], [auto-800] (`window` flags)
    a window without a sample, a window of zeros  [*-randomwin] (B = 0: exact zeros)
  k_real_cos_table, k_real_spectrum,
  k_real_alpha_beta, k_real_twiddles              every fused case (the impulse inputs return the band)
  list builders: direct (k_real_rc / k_real_lists), inverse, segmented sort
                                                  [rc-* | plain-*], [inv-*], [sort-*]
  AUTO -> fused, built on the first tile order    test_auto_method (lambda 2, 32: direct on the time order)
  k_pack, k_spectrum, rocFFT, k_spec_mul, k_unpack
                                                  test_rocfft_route: L = 4 (the L < 2 halo + 2 branch), 256
                                                  (segments of hop - 1, hop, hop + 1, 2 hop + 1), 16384,
                                                  CM2_FFT_LEN = 1024
  k_toeplitz_direct_tiled                         test_direct_routes[E1-2 | E1-33 | E2-300]: tiles of 2048
                                                  against blocks of 2047, 2048, 2049
  k_toeplitz_direct (band too long for the LDS)   test_direct_routes[D1-8578]
  k_diag_apply (v, and v = NULL: expand_diag)     test_diagonal[equal | ragged]
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_ref as R  # noqa: E402
from _guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, L=L, D=device, hip=_hip, torch=torch)


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def _operator(cm, cs, method):
    return cm.I.BlockLO(list(cs.sizes), [b for b in cs.bands], offdiag=True, method=method)


def _apply_time(cm, op, v, what):
    """cm2_noise_apply on guarded buffers -> the whole output, no NaN left, nothing written outside"""
    gin, out = Guarded(cm, len(v), v), Guarded(cm, len(v))
    call(cm, "cm2_noise_apply", op._noise.h, gin.ptr, out.ptr)
    got = out.get()
    out.intact(what)
    gin.intact(what)
    R.assert_bit_equal(gin.get(), v, what + ": the input")
    assert not np.isnan(got).any(), what + ": a NaN is left"
    return got


def _held(got, cs, route, what, fft_len=None, only=None):
    e = R.share(got, cs, route, fft_len, only)
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 B (c = %d)" % (what, e, R.c_of(route, cs.lam))
    return e


# ====================================================== fused kernel, time order ===
@pytest.mark.parametrize("name,lam,inp,flags", R.TIME_CASES, ids=["%s-%d-%s" % c[:3] for c in R.TIME_CASES])
def test_fused_time_order(cm, name, lam, inp, flags):
    cs = R.case(name, lam, inp, flags)
    op = _operator(cm, cs, R.FUSED)
    assert op.noise_info()["fft_len"] == R.N
    what = "fused, time order, %s lambda %d %s" % (name, lam, inp)
    e = _held(_apply_time(cm, op, cs.v, what), cs, "fused", what)
    print("%s: %d windows, largest share of the bound %.3g (c = %d)"
          % (what, len(R.windows(R.offsets(cs.sizes))), e, R.c_of("fused", lam)))


# ====================================================== fused kernel, tile order ===
def _tile_order(cm, monkeypatch, tc, method):
    if tc.lists:
        monkeypatch.setenv("CM2_OS_LISTS", tc.lists)
    if tc.flat:
        monkeypatch.setenv("CM2_OS_FLAT", "1")
    if tc.sort:
        monkeypatch.setenv("CM2_OS_LIST_BUILD", "sort")
    cs = R.case(tc.name, tc.lam, tc.inp, tc.flags)
    what = "tile order %s (%s lambda %d)" % (tc.id, tc.name, tc.lam)
    nt, npix, ok = len(cs.v), 64 * tc.ntiles, cs.ok
    pix = R.make_pointing(tc.pointing, nt, npix, ok)
    P = cm.I.SparseLO(npix, nt, pix, pol=1)
    T = cm.L._sparse_tiles(P, tile_pixels=64, slice_samples=4096)
    assert (T.ntiles, T.nvalid) == (tc.ntiles, int(ok.sum())), (T.ntiles, T.nvalid)
    op = _operator(cm, cs, method)
    # time -> tiles (the values of the flagged samples stay behind), N^-1 on the tile order, tiles -> time
    gin = Guarded(cm, nt, cs.raw)
    d_tb, out_tb, back = Guarded(cm, T.nvalid), Guarded(cm, T.nvalid), Guarded(cm, nt)
    call(cm, "cm2_tod_time_to_tiles", T.h, gin.ptr, d_tb.ptr)
    assert not np.isnan(d_tb.get()).any(), what + ": a NaN is left by time -> tiles"
    before = d_tb.get()
    call(cm, "cm2_noise_apply_tiles", op._noise.h, T.h, d_tb.ptr, out_tb.ptr)
    tb = out_tb.get()
    for g in (gin, d_tb, out_tb):
        g.intact(what)
    R.assert_bit_equal(d_tb.get(), before, what + ": the input in tile order")
    assert not np.isnan(tb).any(), what + ": a NaN is left in the tile order"
    call(cm, "cm2_tod_tiles_to_time", T.h, out_tb.ptr, back.ptr)
    got = back.get()
    back.intact(what)
    assert not np.isnan(got).any(), what + ": a NaN is left"
    R.assert_bit_equal(got[~ok], np.zeros(int((~ok).sum())), what + ": flagged samples")
    want = int(["auto", "plain", "rc", "inv"].index(tc.lists or "auto"))
    assert op.tile_kernel_info()["os_lists"] == R.LIST_NAMES[R.choose_lists(want, tc.sort, tc.ntiles)]
    e = _held(got, cs, "fused", what, only=ok)
    return cs, op, got, e, what


@pytest.mark.parametrize("tc", R.TILE_CASES, ids=[t.id for t in R.TILE_CASES])
def test_fused_tile_order(cm, monkeypatch, tc):
    cs, op, got, e, what = _tile_order(cm, monkeypatch, tc, R.FUSED)
    # the same operator on the time order: both are held to the bound; bit-equality is reported, not promised
    # (each instantiation of the kernel is optimised separately, with FMA contraction on)
    time = _apply_time(cm, op, cs.v, what + ", time order")
    et = _held(time, cs, "fused", what + ", time order")
    same = int((R.bits(got[cs.ok]) == R.bits(time[cs.ok])).sum())
    print("%s: %s lists, largest share of the bound %.3g (time order %.3g, c = %d); %d of %d unflagged samples "
          "bit-equal to the time order" % (what, op.tile_kernel_info()["os_lists"], e, et, R.c_of("fused", cs.lam),
                                           same, int(cs.ok.sum())))


# ============================================================== method left open ===
@pytest.mark.parametrize("tc", R.AUTO_TILE_CASES, ids=[t.id for t in R.AUTO_TILE_CASES])
def test_auto_method(cm, monkeypatch, tc):
    """CM2_TOEPLITZ_AUTO: on a tile order the fused kernel, built on first use, held to the fused bound; on the
    time order the direct sum up to lambda = 32 (bit-equal to its restatement), the fused kernel beyond"""
    cs, op, got, e, what = _tile_order(cm, monkeypatch, tc, R.AUTO)
    info = op.noise_info()
    assert info["tiles_ok"]
    time = _apply_time(cm, op, cs.v, what + ", time order")
    if tc.lam <= 32:
        assert info["method"] == R.DIRECT
        R.assert_bit_equal(time, R.direct_f64(cs.sizes, cs.bands, cs.v), what + ", time order: direct sum")
    else:
        assert info["method"] == R.FUSED and info["fft_len"] == R.N
        _held(time, cs, "fused", what + ", time order")
    print("%s: largest share of the fused bound %.3g (c = %d)" % (what, e, R.c_of("fused", cs.lam)))


# ================================================================== rocFFT route ===
@pytest.mark.parametrize("name,lam,inp,fft_len", R.FFT_CASES,
                         ids=["%s-%d-%s-%s" % c for c in R.FFT_CASES])
def test_rocfft_route(cm, monkeypatch, name, lam, inp, fft_len):
    if fft_len:
        monkeypatch.setenv("CM2_FFT_LEN", str(fft_len))
    cs = R.case(name, lam, inp)
    op = _operator(cm, cs, R.FFT)
    L, halo, hop, segs = R.fft_geometry(lam, cs.sizes, fft_len)
    info = op.noise_info()
    assert (info["method"], info["fft_len"]) == (R.FFT, L)
    what = "rocFFT, %s lambda %d %s, L = %d" % (name, lam, inp, L)
    e = _held(_apply_time(cm, op, cs.v, what), cs, "fft", what, fft_len=fft_len)
    print("%s: %d segments, largest share of the bound %.3g (c = %d)" % (what, len(segs), e, R.c_of("fft", lam)))


# ================================================================= direct routes ===
@pytest.mark.parametrize("name,lam", R.DIRECT_CASES, ids=["%s-%d" % c for c in R.DIRECT_CASES])
def test_direct_routes(cm, name, lam):
    for inp in ("normal", "impulses"):
        cs = R.case(name, lam, inp)
        op = _operator(cm, cs, R.DIRECT)
        assert op.noise_info()["method"] == R.DIRECT
        what = "direct, %s lambda %d %s" % (name, lam, inp)
        R.assert_bit_equal(_apply_time(cm, op, cs.v, what), R.direct_f64(cs.sizes, cs.bands, cs.v), what)
    print("direct, %s lambda %d: bit-equal to the restatement (%d tiles of %d)"
          % (name, lam, len(R.dir_tiles(R.offsets(cs.sizes))), R.K_DIR_TILE))


# ====================================================================== diagonal ===
@pytest.mark.parametrize("name", ["G8", "E2"], ids=["equal", "ragged"])
def test_diagonal(cm, name):
    sizes = R.SIZES[name]
    t = [0.5 + 0.37 * b for b in range(len(sizes))]
    v = R.make_input(name, "normal")
    op = cm.I.BlockLO(list(sizes), t, offdiag=False)
    what = "diagonal, %s" % name
    R.assert_bit_equal(_apply_time(cm, op, v, what), R.diag_f64(sizes, t, v), what)
    w = Guarded(cm, len(v))
    call(cm, "cm2_noise_expand_diag", op._noise.h, w.ptr)
    got = w.get()
    w.intact(what + ", expand_diag")
    R.assert_bit_equal(got, R.diag_f64(sizes, t), what + ", expand_diag")
    print("%s: bit-equal to t_b v and t_b" % what)
