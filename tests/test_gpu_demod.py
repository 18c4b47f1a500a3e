"""
The demodulator on the GPU against the NumPy restatement of _demod_ref.py: T, Q, U, the classes and the counts bit for
bit (values as uint64 views; positions where both sides are NaN count as equal, the sign of a generated NaN differs
between hosts).  The shapes are the smallest at which the kernel can go wrong (the lists are in _demod_ref.py and
checked in test_demod_cpu.py); outputs sit in the sentinel-guarded buffers of _guarded.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import _demod_ref as R
import _pointing_expand_ref as PE
from _guarded import Guarded, GuardedInt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import importlib
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.utilities import gap_fill
    M = importlib.import_module("cosmomap2_amd.utilities.demodulate")
    return SimpleNamespace(U=U, I=I, M=M, hip=_hip, torch=torch, D=D, cg=cosmomap2_amd.cg,
                           flags_to_dev=gap_fill._flags_to_dev)


class Raw(object):
    """The C entry points on guarded buffers: every output comes back with its guards checked."""

    def __init__(self, cm, sizes, D, h):
        self.cm, self.sizes, self.nt, self.nb, self.D = cm, sizes, sum(sizes), len(sizes), D
        self.M = sum(R.out_sizes(sizes, D))
        self.g = cm.M._Demod(self.nt, sizes, D, h)
        self.st = cm.D.stream()

    def run(self, d, flags=None, cosv=None, sinv=None, min_weight=0.5, shift=0):
        """shift = 1: the inputs start 8 bytes into their buffers, so no 16-byte load is possible"""
        cm, carrier = self.cm, cosv is not None

        def inp(a):
            if a is None:
                return None
            return Guarded(cm, self.nt + shift, np.concatenate([np.full(shift, np.nan), a]))
        x, co, si = inp(d), inp(cosv), inp(sinv)
        if flags is not None and flags.dtype == np.uint8:              # bytes as a uint8 tensor brings them: kind 1
            f, kind = cm.D.to_dev(flags), 1
        else:
            f, kind = (None, 0) if flags is None else cm.flags_to_dev(flags)
        T, cls, counts = Guarded(cm, self.M), GuardedInt(cm, self.M, "uint8"), GuardedInt(cm, 3 * self.nb, "int64")
        Q, U = (Guarded(cm, self.M), Guarded(cm, self.M)) if carrier else (None, None)
        ptr = lambda b: None if b is None else b.ptr + 8 * shift
        out = lambda b: None if b is None else b.ptr
        cm.hip.call("cm2_demod_run", self.g.h, ptr(x), ptr(co), ptr(si), cm.D.ptr(f), kind, float(min_weight), out(T),
                    out(Q), out(U), cls.ptr, counts.ptr, self.st)
        got = SimpleNamespace(T=T.get(), Q=Q.get() if carrier else None, U=U.get() if carrier else None,
                              cls=cls.get(), counts=counts.get().reshape(self.nb, 3))
        for buf, what in ((T, "T"), (Q, "Q"), (U, "U"), (cls, "classes"), (counts, "counts"), (x, "d"), (co, "cos"),
                          (si, "sin")):
            if buf is not None:
                buf.intact("cm2_demod_run (%s)" % what)
        assert R.same_bits(x.get()[shift:], d)
        return got

    def pick(self, pix, cls, drop_from):
        cm = self.cm
        p, c = GuardedInt(cm, self.nt, "int32", pix), GuardedInt(cm, self.M, "uint8", cls)
        o = GuardedInt(cm, self.M, "int32")
        cm.hip.call("cm2_demod_pick", self.g.h, p.ptr, c.ptr, int(drop_from), o.ptr, self.st)
        got = o.get()
        for buf, what in ((o, "output"), (p, "pixels"), (c, "classes")):
            buf.intact("cm2_demod_pick (%s)" % what)
        return got


def check(got, want, what):
    for name in ("T", "Q", "U"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            bad = np.flatnonzero((R.bits(a) != R.bits(b)) & ~(np.isnan(a) & np.isnan(b)))
            assert bad.size == 0, (what, name, bad[:10], a[bad[:10]], b[bad[:10]], want.cls[bad[:10]])
    assert np.array_equal(got.cls, want.cls), (what, np.flatnonzero(got.cls != want.cls)[:10])
    assert np.array_equal(got.counts, want.counts), (what, got.counts, want.counts)


# the variants of a case: with its carrier and its own flags (int32), decimation with the flags as bytes, and with
# nothing flagged (which brings the units that take W = Wfull)
VARIANTS = [(True, "own"), (False, "uint8"), (True, "none"), (False, "bool")]


@pytest.mark.parametrize("name", R.CASES)
def test_cases_bit_for_bit(cm, name):
    c = R.case(name)
    raw = Raw(cm, c.sizes, c.D, c.h)
    info = raw.g.info()
    assert (info["nt"], info["nblocks"], info["factor"], info["ntaps"]) == (sum(c.sizes), len(c.sizes), c.D, c.h.size)
    assert (info["M"], info["unit"], info["outputs_per_thread"]) == (raw.M, R.unit_len(c.D), R.rounds(c.D))
    assert info["lds_bytes"] == R.lds_bytes(c.D, c.h.size) and info["bytes"] >= 8 * c.h.size + 3 * 8 * (len(c.sizes) + 1)
    for carrier, flags in VARIANTS:
        v, want = R.variant(c, carrier, flags), R.expected(name, carrier, flags)
        check(raw.run(v.d, v.flags, v.cosv, v.sinv, v.min_weight), want, (name, carrier, flags))
    # the same bits from arrays that no 16-byte load can read
    v, want = R.variant(c, True, "own"), R.expected(name, True, "own")
    check(raw.run(v.d, v.flags, v.cosv, v.sinv, v.min_weight, shift=1), want, (name, "shifted"))


def test_the_shortcut_gives_the_bits_of_the_masked_chains(cm):
    """the unit of the case `shortcut` that stages nothing unusable takes W = Wfull; flag one sample in its reach that
    only its last output reads, and every other output of the unit must keep its bits"""
    c, want = R.case("shortcut"), R.expected("shortcut")
    unit, per, half = R.unit_len(c.D), R.per_unit(c.D), (c.h.size - 1) // 2
    raw = Raw(cm, c.sizes, c.D, c.h)
    check(raw.run(c.d, c.flags, c.cosv, c.sinv), want, "shortcut")
    flags = c.flags.copy()
    flags[2 * unit - c.D + half] = -1                                     # the last sample unit 1 stages
    masked = raw.run(c.d, flags, c.cosv, c.sinv)
    assert masked.cls[2 * per - 1] == R.PARTIAL and (masked.cls[per:2 * per - 1] == R.FULL).all()
    for a, b in ((masked.T, want.T), (masked.Q, want.Q), (masked.U, want.U)):
        assert R.same_bits(a[per:2 * per - 1], b[per:2 * per - 1])
    check(masked, R.run(c.d, c.sizes, c.D, c.h, flags, c.cosv, c.sinv), "shortcut, masked")


@pytest.mark.parametrize("name", ["sizes_D8_L17", "sizes_D3_L7", "flag_run"])
def test_pick(cm, name):
    c, want = R.case(name), R.expected(name)
    raw = Raw(cm, c.sizes, c.D, c.h)
    pix = c.flags.copy()
    e = R.edges(c.sizes)
    pix[e[:-1]] = np.where(np.arange(len(c.sizes)) % 2 == 0, -7, pix[e[:-1]])      # negative centre pixels
    assert {R.FULL, R.PARTIAL, R.REJECTED} <= set(want.cls) and (pix[::c.D] < 0).any()
    for drop_from in (1, 2):
        got = raw.pick(pix, want.cls, drop_from)
        assert np.array_equal(got, R.pick(pix, want.cls, c.sizes, c.D, drop_from)), (name, drop_from)
    keep1, keep2 = raw.pick(pix, want.cls, 1) >= 0, raw.pick(pix, want.cls, 2) >= 0
    assert (keep1 <= keep2).all() and (keep2 & ~keep1).any() and not keep2[want.cls == R.REJECTED].any()


# --------------------------------------------------------------------- the Python layer ----
def test_python_layer_gives_the_same_results(cm):
    c = R.case("sizes_D8_L17")
    want, plain = R.expected(c.name), R.expected(c.name, False, "own")
    dm = cm.U.Demodulator(c.sizes, c.D, taps=c.h)
    t = cm.torch
    for d, flags, car in ((c.d, c.flags, (c.cosv, c.sinv)),
                          (cm.D.f64(c.d), cm.D.i32(c.flags), (cm.D.f64(c.cosv), cm.D.f64(c.sinv))),
                          (c.d, c.flags < 0, (c.cosv, cm.D.f64(c.sinv))), (c.d, c.flags.astype(np.int64), (c.cosv, c.sinv))):
        T, Q, U, cls, info = dm.demodulate(d, car, flags=flags)
        assert all(cm.D.is_dev(x) for x in (T, Q, U, cls)) and T.dtype == t.float64 and cls.dtype == t.uint8
        got = SimpleNamespace(T=cm.D.to_host(T), Q=cm.D.to_host(Q), U=cm.D.to_host(U), cls=cm.D.to_host(cls),
                              counts=info["counts"])
        check(got, want, "demodulate")
        assert info["M"] == want.M == T.numel() and info["out_blocksize"] == R.out_sizes(c.sizes, c.D)
        assert info["Wfull"] == want.wfull and np.array_equal(info["taps"], c.h)
        T1, cls1, info1 = dm.decimate(d, flags=flags)
        got = SimpleNamespace(T=cm.D.to_host(T1), Q=None, U=None, cls=cm.D.to_host(cls1), counts=info1["counts"])
        check(got, plain, "decimate")
        if cm.D.is_dev(d):
            assert R.same_bits(cm.D.to_host(d), c.d)                      # the input is left alone
    # pixels and classes in every kind, host arrays together too (both are uploaded for the call and must live through it)
    for pix in (c.flags, cm.D.i32(c.flags), c.flags.astype(np.int64)):
        for classes in (cls, want.cls.copy(), cm.torch.from_numpy(want.cls.copy())):
            for drop_from in (1, 2):
                slow = dm.pick(pix, classes, drop_from=drop_from)
                assert cm.D.is_dev(slow) == cm.D.is_dev(pix)
                assert np.array_equal(np.asarray(cm.D.to_host(slow)),
                                      R.pick(c.flags, want.cls, c.sizes, c.D, drop_from)), (type(pix), type(classes))
    T2, Q2, U2, cls2, _ = cm.U.demodulate(c.d, c.sizes, c.D, (c.cosv, c.sinv), taps=c.h, flags=c.flags)
    assert R.same_bits(cm.D.to_host(Q2), want.Q) and np.array_equal(cm.D.to_host(cls2), want.cls)
    T3, cls3, _ = cm.U.decimate(c.d, c.sizes, c.D, taps=c.h, flags=c.flags)
    assert R.same_bits(cm.D.to_host(T3), plain.T)
    # the default taps, and min_weight handed through
    c = R.case("sizes_D4_L65")
    T4, cls4, info4 = cm.U.decimate(c.d, c.sizes, 4, flags=c.flags, min_weight=0.9)
    w4 = R.run(c.d, c.sizes, 4, R.default_taps(4), c.flags, min_weight=0.9)
    assert R.same_bits(cm.D.to_host(T4), w4.T) and np.array_equal(info4["counts"], w4.counts)
    assert dm.info(sum(R.case("sizes_D8_L17").sizes))["factor"] == 8


# ------------------------------------------------------------------ guards and overlap ----
def test_overlaps_and_bad_arguments_are_refused(cm):
    nt, sizes, D = 1000, [600, 400], 4
    g = cm.M._Demod(nt, sizes, D, [0.25, 0.5, 0.25])
    M = 250
    buf = Guarded(cm, 4 * nt, np.zeros(4 * nt))
    before = buf.get()
    p = buf.ptr
    t = cm.torch
    T, Q, U = cm.D.zeros(M), cm.D.zeros(M), cm.D.zeros(M)
    cls, counts, fl = cm.D.zeros(M, t.uint8), cm.D.zeros(6, t.int64), cm.D.zeros(nt, t.uint8)
    pix, slow = cm.D.zeros(nt, t.int32), cm.D.zeros(M, t.int32)
    P = cm.D.ptr
    st = cm.D.stream()
    co, si = p + 8 * nt, p + 16 * nt                                      # the carrier: the second and third quarter

    def refused(name, *args):
        with pytest.raises(cm.hip.HipError) as e:
            cm.hip.call(name, *args)
        assert e.value.status == cm.hip.ERR_ARGUMENT and name in str(e.value), str(e.value)

    run = "cm2_demod_run"
    refused(run, g.h, p, None, None, None, 0, 0.5, p, None, None, P(cls), P(counts), st)                 # T is d
    refused(run, g.h, p, None, None, None, 0, 0.5, p + 8 * (nt - 1), None, None, P(cls), P(counts), st)   # one shared sample
    refused(run, g.h, p, co, si, None, 0, 0.5, P(T), si + 8, P(U), P(cls), P(counts), st)                # Q inside sin
    refused(run, g.h, p, co, si, None, 0, 0.5, P(T), P(Q), co, P(cls), P(counts), st)                    # U is cos
    refused(run, g.h, p, co, si, None, 0, 0.5, P(T), P(T), P(U), P(cls), P(counts), st)                  # two outputs
    refused(run, g.h, p, co, si, P(fl), 1, 0.5, P(T), P(Q), P(U), P(fl), P(counts), st)                  # classes on flags
    refused(run, g.h, p, co, si, None, 0, 0.5, P(T), P(Q), P(U), P(cls), p + 8, st)                      # counts inside d
    refused(run, g.h, p, co, None, None, 0, 0.5, P(T), P(Q), P(U), P(cls), P(counts), st)                # half a carrier
    refused(run, g.h, p, co, si, None, 0, 0.5, P(T), None, P(U), P(cls), P(counts), st)                  # a carrier without Q
    refused(run, g.h, p, None, None, None, 0, 0.5, P(T), P(Q), None, P(cls), P(counts), st)              # Q without a carrier
    refused(run, g.h, p, co, si, P(fl), 2, 0.5, P(T), P(Q), P(U), P(cls), P(counts), st)                 # flag_kind
    for mw in (0.0, -0.5, 1.5, float("nan")):
        refused(run, g.h, p, co, si, None, 0, mw, P(T), P(Q), P(U), P(cls), P(counts), st)               # min_weight
    refused(run, g.h, None, co, si, None, 0, 0.5, P(T), P(Q), P(U), P(cls), P(counts), st)
    refused("cm2_demod_pick", g.h, P(pix), P(cls), 0, P(slow), st)
    refused("cm2_demod_pick", g.h, P(pix), P(cls), 3, P(slow), st)
    refused("cm2_demod_pick", g.h, P(pix), P(cls), 2, P(pix) + 4 * (nt - 1), st)                         # one shared pixel
    refused("cm2_demod_pick", g.h, P(pix), P(cls), 2, None, st)
    assert R.same_bits(buf.get(), before)
    buf.intact("refused calls")
    # outputs right behind the inputs are none of it
    cm.hip.call(run, g.h, p, co, si, None, 0, 0.5, p + 24 * nt, P(Q), P(U), P(cls), P(counts), st)
    cm.hip.call("cm2_demod_pick", g.h, P(pix), P(cls), 2, P(slow), st)
    assert not buf.get().any() and cm.D.to_host(counts).tolist() == [149, 1, 0, 99, 1, 0]
    assert not cm.D.to_host(slow).any()
    buf.intact("the accepted calls")


# --------------------------------------------------------------------------- end to end ----
def test_end_to_end_from_pointing_to_three_maps(cm):
    """expand_pointing(hwp=chi) -> demodulate -> pick -> three pol = 1 maps of a sky that is constant in I, Q and U.
    The boresight moves along a meridian with the detectors turned about it only, so the polarisation angle on the sky
    is constant and the carrier is the plate's alone, a tone of f_m = 4 x 2 Hz / 100 Hz = 0.08 cycles per sample: the
    bound of test_demod_cpu.py applies as it stands, to every full output and so to every mean of full outputs."""
    nside, nd, D, fm = 16, 3, 8, 0.08
    npix, ns = 12 * nside * nside, PE.NS
    I0, Q0, U0 = R.QUALITY_IQU
    i = np.arange(ns)
    bore = PE.qmul_E(PE._rot(2, np.full(ns, 0.7)), PE._rot(1, 0.4 + 2.2 * i / ns))
    dets = PE._rot(2, np.array([0.0, 0.5, 1.3]))
    pixs, cos2, sin2 = cm.U.expand_pointing(bore, dets, nside, hwp=PE.hwp_angles())
    h_pix, h_c, h_s = cm.D.to_host(pixs).copy(), cm.D.to_host(cos2).copy(), cm.D.to_host(sin2).copy()
    rate = np.diff(np.unwrap(np.arctan2(h_s, h_c).reshape(nd, ns), axis=1), axis=1) / (2.0 * np.pi)
    assert np.abs(rate - fm).max() < 1e-9                                 # the carrier is the tone the bound is for
    flags = h_pix.copy()
    flags[[5000, 9000]] = -1                                              # two samples dropped: partial outputs inside
    d = cm.D.f64(I0 + Q0 * h_c + U0 * h_s)
    dm = cm.U.Demodulator([ns] * nd, D)
    T, Q, U, cls, info = dm.demodulate(d, (cos2, sin2), flags=cm.D.i32(flags))
    want = R.run(cm.D.to_host(d), [ns] * nd, D, R.default_taps(D), flags, h_c, h_s)
    check(SimpleNamespace(T=cm.D.to_host(T), Q=cm.D.to_host(Q), U=cm.D.to_host(U), cls=cm.D.to_host(cls),
                          counts=info["counts"]), want, "end to end")
    slow = dm.pick(cm.D.i32(flags), cls, drop_from=2)
    h_slow = cm.D.to_host(slow).copy()
    blocks = dm.out_blocksize(nd * ns)
    assert blocks == [-(-ns // D)] * nd and sum(blocks) == h_slow.size == info["M"]
    ces = cm.U.ProcessTimeSamples(slow.clone(), npix, pol=1)
    n, obspix = ces.get_new_pixel
    P = cm.I.SparseLO(n, info["M"], ces.pixs, pol=1, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=1)
    N = cm.I.BlockLO(blocks, [1.0] * nd)
    hits_any = np.bincount(h_slow[h_slow >= 0], minlength=npix)
    full_pix = h_slow[(h_slow >= 0) & (want.cls == R.FULL)]
    hits_full = np.bincount(full_pix, minlength=npix)
    only_full = (hits_full > 0) & (hits_full == hits_any)
    assert only_full.sum() >= 1 and (hits_any > hits_full).any()          # a condition, not a skip
    bT, bQ = R.quality_bounds(R.default_taps(D), fm)
    sel = only_full[np.asarray(obspix)]
    assert sel.sum() == only_full.sum()
    for stream, truth, bound in ((T, I0, bT), (Q, Q0, bQ), (U, U0, bQ)):
        m, _ = cm.cg(P.T * N * P, P.T * (N * stream), M=Mbd, rtol=1e-12, maxiter=50)
        m = np.asarray(cm.D.to_host(m))
        binned = np.asarray(cm.D.to_host(Mbd * (P.T * stream)))
        assert np.abs(m - binned).max() <= 1e-12
        err = np.abs(m - truth)
        print("map of %g: |error| <= %.3g on %d pixels hit by full outputs only (bound %.3g), <= %.3g on the other %d"
              % (truth, err[sel].max(), sel.sum(), bound, err[~sel].max(), (~sel).sum()))
        assert (err[sel] <= bound).all()
