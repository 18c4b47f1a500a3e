"""
Every kernel and entry point of csrc/cm2_pixel.hip against the restatements of tests/_pixel_ref.py, element by
element and bit for bit.  The one exception is the hot-pixel weight sums in the default order: they are bit-equal to
the restatement of the order the source states (R.hot_sum), and they lie within (n + 2) 2^-53 sum |term| of the
np.longdouble sum of the terms (n - 1 additions, at most two product roundings per term: counted, not measured).

Conventions of every case: each array the library reads or writes is the middle of a guarded buffer
(tests/_guarded.py: Guarded for doubles, GuardedInt for int32 / uint8 / int64) whose sentinels must be unchanged
after the call; a double output holds NaN before the call and an integer output a fill value that no kernel
produces; an input comes back bit-identical; every call runs twice and gives the same bits; the weight sums and the
full-sky map, which are overwritten, are computed once more over 123.0.  What an entry point does not write keeps its
fill: counts / cosine / sine at pol 2, everything but counts at pol 1, positions >= new_npix of cm2_compact_*.  A
refused call returns CM2_ERR_ARGUMENT and leaves every output untouched.  cm2_set_exact_order is set through the
fixture `order`, which restores -1; CM2_WEIGHTS_ORDER only through monkeypatch.

Layouts: tails, pow2-64, pow2-4096, stride, hotw of tests/_pixel_ref.py (tests/test_pixel_ref_cpu.py asserts their
features and proves every restatement against the oracle's serial loops); stride has nt = 605 001 samples and
524 293 pixels, beyond the 524 288 threads of a capped grid; hotw is one stream of 38 662 samples with pixels of
8191, 8192, 8193 and 12 543 = 3 * 4096 + 255 hits among 60 ordinary ones.

Kernel / branch -> the case that reaches it:

  k_cos_sin_pairs                          test_weights_serial, pol 2, 3; second trip: stride
  k_weights<1 | 2 | 3>, w and w == NULL    test_weights_serial: tails, pow2-64, pow2-4096, stride (second trip: npix)
    a pixel of 8191 hits stays serial      test_weights_hot (pixel 3 of hotw)
  k_weights_hot<1 | 2 | 3>,                test_weights_hot[default]: 8192 (two full chunks), 8193 (a last chunk of one
  k_weights_hot_combine<1 | 2 | 3>         sample), 12 543 (a last chunk of 255: thread 255 idle); bit-equal to
                                           R.hot_sum, within the counted bound, unit weights give the exact counts
    cm2_set_exact_order(1)                 test_weights_hot[call-exact]: the serial sums
    CM2_WEIGHTS_ORDER=exact alone          test_weights_hot[env-exact]: the serial sums
    cm2_set_exact_order(0) over the        test_weights_hot[call-wins]: the hot order
    environment's exact
  k_pixel_mask, pol 1 | 2 | 3              test_mask: cond == threshold kept, the next threshold below drops it; 0/0 =
                                           NaN and lmin = 0 (inf) dropped; counts 2.0 / nextafter(2, 3) / 3.0 at
                                           pol 3; counts 0 / 5e-324 at pol 1; 524 293 pixels: second trip
  k_keep_to_i32, the exclusive sum,        test_compaction: all kept, none kept (new_npix = 0), last pixel kept /
  k_rank_to_old2new (cm2_pixel_compact)    dropped, npix = 1 kept / dropped, 524 293 pixels; npix = 0 refused
  k_compact<double | int64_t>              test_compaction: writes exactly the positions < new_npix
  k_flag (cm2_flag_samples)                test_flagging: in place, -1 stays -1, ids mapped to -1 and to new ranks;
                                           nt = 0; second trip: stride
  k_bd_det_mask, pol 1 | 2 | 3             test_block_operators: |det| = 1e-5 -> 0, nextafter(1e-5, 1) -> 1, both
                                           signs; counts 0 at pol 1; 130 and 524 293 pixels
  k_bdprecond<1 | 2 | 3>                   test_block_operators: masked pixels give +0.0, the others the closed form
  k_bd_apply<1 | 2 | 3>                    test_block_operators
  k_obspix_range, k_cut_to_full,           test_sky: a strict subset with pixel 0 and nfull - 1, every other pixel +0.0,
  k_full_to_cut, pol 1 | 2 | 3             the round trip is the identity; npix = 0; 524 293 of 786 432 pixels: second
                                           trip; an id of -1 or nfull: refused with the output untouched
  argument checks of every entry point     test_refusals
"""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_ref as R  # noqa: E402
from _guarded import GUARD, INT_FILL, Guarded, GuardedInt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    from cosmomap2_amd import _hip, device
    return SimpleNamespace(D=device, hip=_hip, torch=torch)


@pytest.fixture
def order(cm):
    """cm2_set_exact_order for one test; -1 (the environment decides) afterwards"""
    yield lambda on: cm.hip.call("cm2_set_exact_order", on)
    cm.hip.call("cm2_set_exact_order", -1)


def addr(g):
    """device address of a guarded buffer's data (of where it would be, for an empty one)"""
    return None if g is None else g.buf.data_ptr() + GUARD * g.buf.element_size()


def call(cm, name, *args):
    cm.hip.call(name, *(list(args) + [cm.D.stream()]))


def refused(cm, name, *args):
    lib = cm.hip.load()
    rc = getattr(lib, name)(*(list(args) + [cm.D.stream()]))
    cm.torch.cuda.synchronize()
    assert rc == cm.hip.ERR_ARGUMENT, (name, rc, lib.cm2_last_error())


def _same(g, want, what):
    got = g.get()
    g.intact(what)
    R.assert_bit_equal(got, want, what)
    return got


def _untouched(g, what, fill=None):
    g.intact(what)
    got = g.get()
    if isinstance(g, GuardedInt):
        assert (got == g.fill).all(), what + ": written"
    elif fill is None:
        assert np.isnan(got).all(), what + ": written"
    else:
        assert (got == fill).all(), what + ": written"


# ------------------------------------------------------------------------- weight sums ----
class Streams(object):
    def __init__(self, cm, cs):
        self.cs = cs
        self.pix = GuardedInt(cm, cs.nt, "int32", cs.pix)
        self.cos, self.sin = Guarded(cm, cs.nt, cs.cos), Guarded(cm, cs.nt, cs.sin)
        self.w = Guarded(cm, cs.nt, cs.w)

    def unchanged(self):
        cs = self.cs
        _same(self.pix, cs.pix, "pix")
        _same(self.cos, cs.cos, "cos")
        _same(self.sin, cs.sin, "sin")
        _same(self.w, cs.w, "w")


def accumulate(cm, st, pol, with_w, want, what):
    """cm2_weights_accumulate from NaN, a second time, over 123.0 -> the sums of the last run"""
    cs = st.cs
    out = {k: Guarded(cm, cs.npix) for k in R.WSUMS}
    got = {}
    for fill, rep in ((None, ""), (None, ", second call"), (123.0, ", over 123.0")):
        if fill is not None:
            for g in out.values():
                g.v.fill_(fill)
        call(cm, "cm2_weights_accumulate", pol, cs.nt, cs.npix, addr(st.pix), addr(st.w) if with_w else None,
             addr(st.cos), addr(st.sin), *[addr(out[k]) for k in R.WSUMS])
        for k in R.WSUMS:
            if k in R.WRITTEN[pol]:
                got[k] = _same(out[k], want[k], "%s: %s%s" % (what, k, rep))
            else:
                _untouched(out[k], "%s: %s%s" % (what, k, rep), fill)
    return got


@functools.lru_cache(maxsize=None)
def want_weights(name, pol, with_w, how):
    cs = R.case(name)
    return R.weights(cs, pol, cs.w if with_w else None, how)


@pytest.mark.parametrize("pol", (1, 2, 3))
@pytest.mark.parametrize("name", R.WEIGHT_CASES)
def test_weights_serial(cm, name, pol):
    cs = R.case(name)
    assert cs.hits.max() < R.HOT_MIN
    st = Streams(cm, cs)
    for with_w in (True, False):
        got = accumulate(cm, st, pol, with_w, want_weights(name, pol, with_w, "serial"),
                         "%s pol %d %s" % (name, pol, "w" if with_w else "w = NULL"))
        if not with_w and pol != 2:
            R.assert_bit_equal(got["counts"], cs.hits.astype(np.float64), "the hit counts")
    st.unchanged()


@pytest.mark.parametrize("mode", ("default", "call-exact", "env-exact", "call-wins"))
def test_weights_hot(cm, order, monkeypatch, mode):
    cs = R.case("hotw")
    monkeypatch.delenv("CM2_WEIGHTS_ORDER", raising=False)
    if mode in ("env-exact", "call-wins"):
        monkeypatch.setenv("CM2_WEIGHTS_ORDER", "exact")
    if mode == "call-exact":
        order(1)
    if mode == "call-wins":
        order(0)
    how = "hot" if mode in ("default", "call-wins") else "serial"
    st = Streams(cm, cs)
    for pol in (1, 2, 3):
        for with_w in (True, False):
            what = "hotw %s pol %d %s" % (mode, pol, "w" if with_w else "w = NULL")
            got = accumulate(cm, st, pol, with_w, want_weights("hotw", pol, with_w, how), what)
            share = R.hot_share(cs, pol, cs.w if with_w else None, got)
            print("%s: %.3g of the bound (n + 2) 2^-53 sum |term|" % (what, share))
            assert share <= 1.0, (what, share)
            if not with_w and pol != 2:
                R.assert_bit_equal(got["counts"], cs.hits.astype(np.float64), what + ": the hit counts")
    st.unchanged()


# -------------------------------------------------------------------------------- mask ----
@pytest.mark.parametrize("pol", (1, 2, 3))
def test_mask(cm, pol):
    npix = 524293
    host = R.mask_arrays(npix)
    dev = [Guarded(cm, npix, a) for a in host]
    for ti, thr in enumerate(R.THRESHOLDS):
        keep = GuardedInt(cm, npix, "uint8")
        want, _ = R.pixel_mask(pol, *host, thr)
        R.assert_bit_equal(want, np.resize(np.asarray(R.MASK_KEEP[(pol, ti)], dtype=np.uint8), npix), "by hand")
        for rep in ("", ", second call"):
            call(cm, "cm2_pixel_mask", pol, npix, *[addr(g) for g in dev], thr, addr(keep))
            _same(keep, want, "keep, pol %d threshold %r%s" % (pol, thr, rep))
    for g, a in zip(dev, host):
        _same(g, a, "an input of the mask")
    keep = GuardedInt(cm, npix, "uint8")
    refused(cm, "cm2_pixel_mask", 0, npix, *[addr(g) for g in dev], 1e3, addr(keep))
    refused(cm, "cm2_pixel_mask", 4, npix, *[addr(g) for g in dev], 1e3, addr(keep))
    refused(cm, "cm2_pixel_mask", pol, npix, *[addr(g) for g in dev], 1e3, None)
    _untouched(keep, "keep of a refused cm2_pixel_mask")


# -------------------------------------------------------------------------- compaction ----
@pytest.mark.parametrize("name", R.COMPACT_CASES)
def test_compaction(cm, name):
    hk = R.keep_pattern(name)
    npix = hk.size
    want_o2n, want_n = R.compact(hk)
    keep = GuardedInt(cm, npix, "uint8", hk.copy())
    o2n = GuardedInt(cm, npix, "int32")
    for rep in ("", ", second call"):
        n = ctypes.c_int64(-777)
        call(cm, "cm2_pixel_compact", npix, addr(keep), addr(o2n), ctypes.byref(n))
        assert n.value == want_n == int(hk.sum()), (name, n.value, want_n)
        _same(o2n, want_o2n, "old2new" + rep)
    rng = np.random.default_rng(5)
    f_in, i_in = rng.standard_normal(npix), rng.integers(-2 ** 62, 2 ** 62, npix)
    gf, gi = Guarded(cm, npix, f_in), GuardedInt(cm, npix, "int64", i_in)
    of, oi = Guarded(cm, npix), GuardedInt(cm, npix, "int64")
    for rep in ("", ", second call"):
        call(cm, "cm2_compact_f64", npix, addr(o2n), addr(gf), addr(of))
        call(cm, "cm2_compact_i64", npix, addr(o2n), addr(gi), addr(oi))
        got = _same(of, R.compact_apply(want_o2n, f_in, np.nan), "compact_f64" + rep)
        assert np.isnan(got[want_n:]).all() and not np.isnan(got[:want_n]).any()
        got = _same(oi, R.compact_apply(want_o2n, i_in, INT_FILL["int64"]), "compact_i64" + rep)
        assert (got[want_n:] == INT_FILL["int64"]).all()
    _same(keep, hk, "keep")
    _same(o2n, want_o2n, "old2new after its users")
    _same(gf, f_in, "the doubles")
    _same(gi, i_in, "the int64s")


def test_compaction_refusals(cm):
    hk = R.keep_pattern("last-kept")
    keep, o2n = GuardedInt(cm, hk.size, "uint8", hk.copy()), GuardedInt(cm, hk.size, "int32")
    n = ctypes.c_int64(-777)
    refused(cm, "cm2_pixel_compact", 0, addr(keep), addr(o2n), ctypes.byref(n))       # reads element npix - 1
    refused(cm, "cm2_pixel_compact", -3, addr(keep), addr(o2n), ctypes.byref(n))
    refused(cm, "cm2_pixel_compact", hk.size, None, addr(o2n), ctypes.byref(n))
    refused(cm, "cm2_pixel_compact", hk.size, addr(keep), None, ctypes.byref(n))
    refused(cm, "cm2_pixel_compact", hk.size, addr(keep), addr(o2n), None)
    assert n.value == -777
    _untouched(o2n, "old2new of a refused cm2_pixel_compact")
    _same(keep, hk, "keep")
    of, oi = Guarded(cm, hk.size), GuardedInt(cm, hk.size, "int64")
    for nm, out in (("cm2_compact_f64", of), ("cm2_compact_i64", oi)):
        refused(cm, nm, hk.size, None, addr(of), addr(out))
        refused(cm, nm, hk.size, addr(o2n), None, addr(out))
        refused(cm, nm, hk.size, addr(o2n), addr(of), None)
        _untouched(out, "the output of a refused " + nm)


# ---------------------------------------------------------------------------- flagging ----
@pytest.mark.parametrize("name", ("tails", "stride"))
def test_flagging(cm, name):
    cs = R.case(name)
    old2new, new_npix = R.compact(cs.hits >= 2)              # pixels of 0 or 1 hits go: ids map to -1 and to ranks
    want = R.flag(cs.pix, old2new)
    valid = cs.pix >= 0
    assert 0 < new_npix < cs.npix and (want[~valid] == -1).all()
    assert (want[valid] == -1).any() and (want[valid] >= 0).any() and want.max() == new_npix - 1
    o2n = GuardedInt(cm, cs.npix, "int32", old2new)
    for rep in ("", ", second run"):
        pix = GuardedInt(cm, cs.nt, "int32", cs.pix)
        call(cm, "cm2_flag_samples", cs.nt, addr(pix), addr(o2n))
        _same(pix, want, "flagged stream" + rep)
    _same(o2n, old2new, "old2new")
    # nt = 0: nothing is read or written
    pix = GuardedInt(cm, 4, "int32")
    call(cm, "cm2_flag_samples", 0, addr(pix), addr(o2n))
    _untouched(pix, "nt = 0")
    refused(cm, "cm2_flag_samples", 4, None, addr(o2n))
    refused(cm, "cm2_flag_samples", 4, addr(pix), None)
    _untouched(pix, "a refused cm2_flag_samples")


# --------------------------------------------------------------------- block operators ----
@pytest.mark.parametrize("pol", (1, 2, 3))
@pytest.mark.parametrize("npix", (130, 524293))
def test_block_operators(cm, npix, pol):
    b = R.blocks(npix)
    hx = b.x[:pol * npix]
    names = ("counts", "cosine", "sine", "cos2", "sin2", "sincos")
    sums = [Guarded(cm, npix, getattr(b, k)) for k in names]
    ps = [addr(g) for g in sums]
    want_det, want_mask = R.bd_det_mask(pol, b)
    det, mask = Guarded(cm, npix), GuardedInt(cm, npix, "uint8")
    x, y = Guarded(cm, pol * npix, hx), Guarded(cm, pol * npix)
    want_y = R.bd_precond(pol, b, want_det, want_mask, hx)
    assert not want_y.reshape(npix, pol)[want_mask == 0].view(np.int64).any(), "masked pixels give +0.0"
    for rep in ("", ", second call"):
        call(cm, "cm2_bd_det_mask", pol, npix, *ps, addr(det), addr(mask))
        _same(det, want_det, "det" + rep)
        _same(mask, want_mask, "mask" + rep)
        call(cm, "cm2_bdprecond_apply", pol, npix, *ps, addr(det), addr(mask), addr(x), addr(y))
        _same(y, want_y, "M_BD x" + rep)
    if pol > 1:
        assert list(want_mask[:5]) == [0, 1, 0, 1, 0] and want_det[0] == 1e-5 and want_det[2] == -1e-5
    else:
        assert want_mask[4] == 0
    y2 = Guarded(cm, pol * npix)
    for rep in ("", ", second call"):
        call(cm, "cm2_bd_apply", pol, npix, *ps, addr(x), addr(y2))
        _same(y2, R.bd_apply(pol, b, hx), "block apply" + rep)
    for g, k in zip(sums, names):
        _same(g, getattr(b, k), k + " (an input)")
    _same(x, hx, "x")
    _same(det, want_det, "det (an input of M_BD)")
    _same(mask, want_mask, "mask (an input of M_BD)")


def test_block_operator_refusals(cm):
    npix = 130
    b = R.blocks(npix)
    sums = [Guarded(cm, npix, getattr(b, k)) for k in ("counts", "cosine", "sine", "cos2", "sin2", "sincos")]
    ps = [addr(g) for g in sums]
    det, mask = Guarded(cm, npix), GuardedInt(cm, npix, "uint8")
    x, y = Guarded(cm, 3 * npix, b.x), Guarded(cm, 3 * npix)
    for pol in (0, 4):
        refused(cm, "cm2_bd_det_mask", pol, npix, *ps, addr(det), addr(mask))
        refused(cm, "cm2_bdprecond_apply", pol, npix, *ps, addr(det), addr(mask), addr(x), addr(y))
        refused(cm, "cm2_bd_apply", pol, npix, *ps, addr(x), addr(y))
    refused(cm, "cm2_bd_det_mask", 3, npix, *ps, None, addr(mask))
    refused(cm, "cm2_bd_det_mask", 3, npix, *ps, addr(det), None)
    refused(cm, "cm2_bdprecond_apply", 3, npix, *ps, addr(det), None, addr(x), addr(y))
    refused(cm, "cm2_bdprecond_apply", 3, npix, *ps, addr(det), addr(mask), None, addr(y))
    refused(cm, "cm2_bdprecond_apply", 3, npix, *ps, addr(det), addr(mask), addr(x), None)
    refused(cm, "cm2_bd_apply", 3, npix, *ps, None, addr(y))
    refused(cm, "cm2_bd_apply", 3, npix, *ps, addr(x), None)
    _untouched(det, "det")
    _untouched(mask, "mask")
    _untouched(y, "y")


# ------------------------------------------------------------------- cut sky <-> full sky ----
@pytest.mark.parametrize("pol", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(R.SKIES))
def test_sky(cm, name, pol):
    sk = R.sky(name)
    npix, nfull = sk.npix, sk.nfull
    hm = sk.map[:pol * npix]
    obs, m = GuardedInt(cm, npix, "int64", sk.obspix), Guarded(cm, pol * npix, hm)
    full = Guarded(cm, pol * nfull)
    want = R.cut_to_full(pol, sk.obspix, hm, nfull)
    for fill, rep in ((None, ""), (None, ", second call"), (123.0, ", over 123.0")):
        if fill is not None:
            full.v.fill_(fill)
        call(cm, "cm2_cutsky_to_fullsky", pol, npix, addr(obs), addr(m), nfull, addr(full))
        _same(full, want, "full sky" + rep)
    back = Guarded(cm, pol * npix)
    for rep in ("", ", second call"):
        call(cm, "cm2_fullsky_to_cutsky", pol, npix, addr(obs), addr(full), nfull, addr(back))
        _same(back, hm, "the round trip" + rep)
    _same(obs, sk.obspix, "obspix")
    _same(m, hm, "the map")
    _same(full, want, "full sky (an input of the way back)")
    if name == "small":
        # npix = 0: a full sky of exact zeros, and nothing on the way back
        call(cm, "cm2_cutsky_to_fullsky", pol, 0, None, None, nfull, addr(full))
        _same(full, np.zeros(pol * nfull), "npix = 0")
        none = Guarded(cm, 4)
        call(cm, "cm2_fullsky_to_cutsky", pol, 0, None, None, nfull, addr(none))
        _untouched(none, "npix = 0, the way back")
        # an observed pixel outside the full sky: refused, nothing written
        for bad in (-1, nfull):
            ids = sk.obspix.copy()
            ids[npix // 2] = bad
            gb, out, cut = GuardedInt(cm, npix, "int64", ids), Guarded(cm, pol * nfull), Guarded(cm, pol * npix)
            refused(cm, "cm2_cutsky_to_fullsky", pol, npix, addr(gb), addr(m), nfull, addr(out))
            refused(cm, "cm2_fullsky_to_cutsky", pol, npix, addr(gb), addr(full), nfull, addr(cut))
            _untouched(out, "full sky of a refused call (id %d)" % bad)
            _untouched(cut, "cut sky of a refused call (id %d)" % bad)


def test_refusals(cm):
    """what the tests above leave: cm2_weights_accumulate and the sizes / NULLs of the sky maps"""
    cs = R.case("tails")
    st = Streams(cm, cs)
    out = {k: Guarded(cm, cs.npix) for k in R.WSUMS}
    po = [addr(out[k]) for k in R.WSUMS]

    def acc(pol, nt, npix, pix, cos, sin, outs):
        refused(cm, "cm2_weights_accumulate", pol, nt, npix, pix, addr(st.w), cos, sin, *outs)

    a = (addr(st.pix), addr(st.cos), addr(st.sin))
    acc(0, cs.nt, cs.npix, *a, po)
    acc(4, cs.nt, cs.npix, *a, po)
    acc(3, cs.nt, 0, *a, po)
    acc(3, -1, cs.npix, *a, po)
    acc(3, cs.nt, cs.npix, a[0], None, a[2], po)
    acc(2, cs.nt, cs.npix, a[0], a[1], None, po)
    for k in range(6):
        acc(3, cs.nt, cs.npix, *a, po[:k] + [None] + po[k + 1:])
    acc(1, cs.nt, cs.npix, *a, [None] + po[1:])
    acc(2, cs.nt, cs.npix, *a, po[:3] + [None] + po[4:])
    for bad in (cs.npix, -2):
        p = cs.pix.copy()
        p[7] = bad
        gp = GuardedInt(cm, cs.nt, "int32", p)
        acc(1, cs.nt, cs.npix, addr(gp), a[1], a[2], po)
        acc(3, cs.nt, cs.npix, addr(gp), a[1], a[2], po)
    sk = R.sky("small")
    obs, m = GuardedInt(cm, sk.npix, "int64", sk.obspix), Guarded(cm, 3 * sk.npix, sk.map)
    full, cut = Guarded(cm, 3 * sk.nfull), Guarded(cm, 3 * sk.npix)
    for pol in (0, 4):
        refused(cm, "cm2_cutsky_to_fullsky", pol, sk.npix, addr(obs), addr(m), sk.nfull, addr(full))
        refused(cm, "cm2_fullsky_to_cutsky", pol, sk.npix, addr(obs), addr(full), sk.nfull, addr(cut))
    refused(cm, "cm2_cutsky_to_fullsky", 3, -1, addr(obs), addr(m), sk.nfull, addr(full))
    refused(cm, "cm2_cutsky_to_fullsky", 3, sk.npix, None, addr(m), sk.nfull, addr(full))
    refused(cm, "cm2_cutsky_to_fullsky", 3, sk.npix, addr(obs), None, sk.nfull, addr(full))
    refused(cm, "cm2_cutsky_to_fullsky", 3, sk.npix, addr(obs), addr(m), sk.nfull, None)
    refused(cm, "cm2_fullsky_to_cutsky", 3, sk.npix, addr(obs), addr(full), -1, addr(cut))
    refused(cm, "cm2_fullsky_to_cutsky", 3, sk.npix, addr(obs), addr(full), sk.nfull, None)
    for k in R.WSUMS:
        _untouched(out[k], k + " of a refused cm2_weights_accumulate")
    _untouched(full, "full sky")
    _untouched(cut, "cut sky")
    st.unchanged()
