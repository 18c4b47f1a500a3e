"""
Every kernel and entry point of csrc/cm2_pointing.hip and csrc/cm2_pixindex.hip against the restatements of
tests/_pixel_ref.py, element by element and bit for bit (the translation units are built with -ffp-contract=off and
the kernels add each pixel's terms in time order: there is no tolerance anywhere).

Conventions of every case: each array the library reads or writes is the middle of a guarded buffer
(tests/_guarded.py) whose sentinels must be unchanged after the call; an output holds NaN before the call, an input
comes back bit-identical; every call runs twice and gives the same bits; P^T and the fused product, which overwrite
their output, run once more on an output prefilled with 123.0 and give the same bits again.  A refused call returns
CM2_ERR_ARGUMENT and leaves every output NaN.  The data has -0.0 and a denormal in it.

Layouts (tests/_pixel_ref.py; tests/test_pixel_ref_cpu.py asserts the feature of every row, proves the restatements
against the oracle's serial loops and shows that a restatement without the tail of the 4- / 8-row loop, or with the
flagged key one bit short, differs on the case that claims the branch):

  tails          130 pixels, 9-10 each with 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17 hits, 100 of 1069 flagged
  pow2-N         N = 63, 64, 65, 4095, 4096, 4097 pixels, pixel 0 and N - 1 hit, N / 8 + 3 flagged (pol 1, 3)
  empty-flagged  20 samples, all flagged, 70 pixels        empty-nt0   no sample, 70 pixels
  hot            pixel 5 with 20 000 hits, 63 pixels with 1-3, a second slice of 64 pixels without a hit
  stride         524 293 pixels, 200 000 with two hits, 200 001 with one (the last among them), 5 000 flagged:
                 nt = 605 001, npix + 1 and sell_len = 600 064 all exceed the 524 288 threads of a capped grid

Kernel / branch -> the case that reaches it:

  k_check_pix (cm2_pointing_create)        every case; nvalid of cm2_pointing_info; second trip: stride; a pixel id
                                           of npix or -2: test_refusals
    the nt == 0 branch                     empty-nt0 (also of cm2_P_apply and build_pixindex)
  k_P_time<1 | 2 | 3>                      every case at its pols; flagged samples give +0.0; second trip: stride
  build_pixindex: k_make_keys, the radix   every case; end_bit at npix = 2^k - 1, 2^k, 2^k + 1 with flagged samples
    sort on end_bit bits, k_lower_bound    present: pow2-N; second trip (nt, npix + 1): stride
  k_counts, the descending sort            every case; second trip: stride
  k_pad_slots                              padding slots 62: tails, 1 / 0 / 63: pow2-N, 58: the empty cases, 59: stride
  k_slice_len, the exclusive sum           sell_len of cm2_pointing_info = 64 x sum of the slice maxima, every case;
                                           a slice of width 0: hot, sell_len = 0: the empty cases
  k_fill_sell<1 | 2 | 3>                   every case; lanes shorter than their slice (kInvalidSample rows): tails, hot
  k_Pt_sell<1 | 2 | 3>                     body of 4 rows and tails of 0-3 rows, with and without a body: tails; a lane
                                           of 20 000 rows: hot; exact zeros everywhere: the empty cases
  k_gather_w (cm2_pointing_set_weights)    w, then NULL (the fused product equals P^T (P x) bit for bit), then
                                           another w into the same buffer: every case; second trip: stride
  k_PtNP_sell<1 | 2 | 3>                   body of 8 rows and tails of 0-7 rows: tails; hot; the empty cases
  cm2_pointing_info                        -1, -1, -1 before the first use, nvalid / sell_len / nslices after it
  cm2_pointing_build_sell                  test_build_sell_alone
  argument checks                          test_refusals
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_ref as R  # noqa: E402
from _guarded import GUARD, Guarded, GuardedInt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device
    return SimpleNamespace(D=device, hip=_hip, torch=torch)


def addr(g):
    """device address of a guarded buffer's data (of where it would be, for an empty one)"""
    return g.buf.data_ptr() + GUARD * g.buf.element_size()


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def refused(cm, name, *args):
    lib = cm.hip.load()
    rc = getattr(lib, name)(*args)
    cm.torch.cuda.synchronize()
    assert rc == cm.hip.ERR_ARGUMENT, (name, rc, lib.cm2_last_error())


def _same(g, want, what):
    got = g.get()
    g.intact(what)
    R.assert_bit_equal(got, want, what)


def _all_nan(g, what):
    g.intact(what)
    assert np.isnan(g.get()).all(), what + ": the output was written"


class Plan(object):
    """a cm2_pointing over guarded copies of a case's streams"""

    def __init__(self, cm, cs, pol):
        self.cm, self.cs, self.pol = cm, cs, pol
        self.pix = GuardedInt(cm, cs.nt, "int32", cs.pix)
        self.cos, self.sin = Guarded(cm, cs.nt, cs.cos), Guarded(cm, cs.nt, cs.sin)
        h = ctypes.c_void_p(0xDEAD)
        rc = cm.hip.load().cm2_pointing_create(ctypes.byref(h), addr(self.pix), addr(self.cos) if pol > 1 else None,
                                               addr(self.sin) if pol > 1 else None, cs.nt, cs.npix, pol,
                                               cm.D.stream())
        assert rc == 0, cm.hip.load().cm2_last_error()
        self.H = cm.hip.Handle("cm2_pointing_destroy", h, keep=(self.pix, self.cos, self.sin))
        self.h = h

    def info(self):
        out = (ctypes.c_int64 * 6)()
        self.cm.hip.call("cm2_pointing_info", self.h, out)
        return list(out)

    def streams_unchanged(self):
        cs = self.cs
        self.pix.intact("pix")
        np.testing.assert_array_equal(self.pix.get(), cs.pix)
        _same(self.cos, cs.cos, "cos stream")
        _same(self.sin, cs.sin, "sin stream")


def _overwriting(cm, name, h, src, n, want, what):
    """an entry point that overwrites its output: from NaN, a second time, and over 123.0"""
    out = Guarded(cm, n)
    call(cm, name, h, addr(src), addr(out))
    _same(out, want, what)
    call(cm, name, h, addr(src), addr(out))
    _same(out, want, what + ", second call")
    out.v.fill_(123.0)
    call(cm, name, h, addr(src), addr(out))
    _same(out, want, what + ", over 123.0")


@pytest.mark.parametrize("name,pol", [(n, p) for n in R.POINTING_CASES for p in R.pols_of(n)])
def test_pointing(cm, name, pol):
    cs = R.case(name)
    npix, nt = cs.npix, cs.nt
    xh = cs.x[:pol * npix]
    pl = Plan(cm, cs, pol)
    assert pl.info() == [nt, npix, pol, -1, -1, -1]
    x, v = Guarded(cm, pol * npix, xh), Guarded(cm, nt, cs.v)
    # P: builds nothing
    want_P = R.P(pol, cs.pix, cs.cos, cs.sin, xh)
    tod = Guarded(cm, nt)
    for rep in ("", ", second call"):
        call(cm, "cm2_P_apply", pl.h, addr(x), addr(tod))
        _same(tod, want_P, "P" + rep)
    assert pl.info()[3:] == [-1, -1, -1]
    # P^T: the first user builds the pixel-major plan
    want_Pt = R.Pt(pol, npix, cs.pix, cs.cos, cs.sin, cs.v)
    _overwriting(cm, "cm2_Pt_apply", pl.h, v, pol * npix, want_Pt, "Pt")
    assert pl.info() == [nt, npix, pol, nt - cs.nflag, R.sell_len(cs.hits), R.nslices(npix)]
    if nt == cs.nflag:
        assert not want_Pt.view(np.int64).any()
    # the fused product: w, NULL, another w into the same buffer
    w, w2 = Guarded(cm, nt, cs.w), Guarded(cm, nt, cs.w2)
    for gw, hw, what in ((w, cs.w, "w"), (None, None, "w = NULL"), (w2, cs.w2, "a second w")):
        call(cm, "cm2_pointing_set_weights", pl.h, addr(gw) if gw else None)
        want = R.fused(pol, npix, cs.pix, cs.cos, cs.sin, hw, xh)
        if gw is None:
            R.assert_bit_equal(want, R.Pt(pol, npix, cs.pix, cs.cos, cs.sin, want_P), "P^T (P x)")
        _overwriting(cm, "cm2_PtNP_diag_apply", pl.h, x, pol * npix, want, "fused, " + what)
    pl.streams_unchanged()
    for g, data, what in ((x, xh, "x"), (v, cs.v, "v"), (w, cs.w, "w"), (w2, cs.w2, "w2")):
        _same(g, data, what + " (an input)")


def test_build_sell_alone(cm):
    cs = R.case("tails")
    pl = Plan(cm, cs, 3)
    call(cm, "cm2_pointing_build_sell", pl.h)
    assert pl.info() == [cs.nt, cs.npix, 3, cs.nt - cs.nflag, R.sell_len(cs.hits), 3]
    call(cm, "cm2_pointing_build_sell", pl.h)
    x = Guarded(cm, 3 * cs.npix, cs.x)
    out = Guarded(cm, 3 * cs.npix)
    st = cm.D.stream()
    refused(cm, "cm2_PtNP_diag_apply", pl.h, addr(x), addr(out), st)      # no weights yet
    _all_nan(out, "fused before cm2_pointing_set_weights")
    pl.streams_unchanged()


def test_refusals(cm):
    cs = R.case("tails")
    lib, st = cm.hip.load(), cm.D.stream()
    c, s = Guarded(cm, cs.nt, cs.cos), Guarded(cm, cs.nt, cs.sin)

    def create(pixels, npix, pol, cos=c, sin=s, byref=True):
        pix = GuardedInt(cm, len(pixels), "int32", pixels)
        h = ctypes.c_void_p(0xDEAD)
        rc = lib.cm2_pointing_create(ctypes.byref(h) if byref else None, addr(pix), addr(cos) if cos else None,
                                     addr(sin) if sin else None, len(pixels), npix, pol, st)
        cm.torch.cuda.synchronize()
        pix.intact("pix")
        assert rc == cm.hip.ERR_ARGUMENT, (rc, lib.cm2_last_error())
        assert not byref or h.value is None, "a refused create left a handle behind"

    create(cs.pix, cs.npix, 0)
    create(cs.pix, cs.npix, 4)
    create(cs.pix, 0, 3)
    create(cs.pix, -1, 1)
    for bad in (cs.npix, -2):
        p = cs.pix.copy()
        p[cs.nt // 2] = bad
        create(p, cs.npix, 1)
        create(p, cs.npix, 3)
    create(cs.pix, cs.npix, 3, cos=None)
    create(cs.pix, cs.npix, 2, sin=None)
    create(cs.pix, cs.npix, 1, byref=False)
    h = ctypes.c_void_p(0xDEAD)
    assert lib.cm2_pointing_create(ctypes.byref(h), None, addr(c), addr(s), cs.nt, cs.npix, 3, st) \
        == cm.hip.ERR_ARGUMENT and h.value is None
    info = (ctypes.c_int64 * 6)()
    assert lib.cm2_pointing_info(None, info) == cm.hip.ERR_ARGUMENT
    for name in ("cm2_pointing_build_sell", "cm2_pointing_set_weights"):
        refused(cm, name, *([None] * (len(cm.hip.PROTOTYPES[name]) - 1) + [st]))

    pl = Plan(cm, cs, 3)
    assert lib.cm2_pointing_info(pl.h, None) == cm.hip.ERR_ARGUMENT
    x, v = Guarded(cm, 3 * cs.npix, cs.x), Guarded(cm, cs.nt, cs.v)
    tod, m = Guarded(cm, cs.nt), Guarded(cm, 3 * cs.npix)
    refused(cm, "cm2_P_apply", None, addr(x), addr(tod), st)
    refused(cm, "cm2_P_apply", pl.h, None, addr(tod), st)
    refused(cm, "cm2_P_apply", pl.h, addr(x), None, st)
    refused(cm, "cm2_Pt_apply", None, addr(v), addr(m), st)
    refused(cm, "cm2_Pt_apply", pl.h, None, addr(m), st)
    refused(cm, "cm2_Pt_apply", pl.h, addr(v), None, st)
    assert pl.info()[3:] == [-1, -1, -1], "a refused call built the plan"
    refused(cm, "cm2_PtNP_diag_apply", pl.h, addr(x), addr(m), st)        # before any weights were set
    call(cm, "cm2_pointing_set_weights", pl.h, None)
    refused(cm, "cm2_PtNP_diag_apply", None, addr(x), addr(m), st)
    refused(cm, "cm2_PtNP_diag_apply", pl.h, None, addr(m), st)
    refused(cm, "cm2_PtNP_diag_apply", pl.h, addr(x), None, st)
    _all_nan(tod, "P after the refusals")
    _all_nan(m, "P^T and the fused product after the refusals")
    _same(x, cs.x, "x")
    _same(v, cs.v, "v")
    pl.streams_unchanged()
    assert cm.hip.load().cm2_pointing_destroy(None) == 0
