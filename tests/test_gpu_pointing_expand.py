"""
The pointing expansion on the GPU (cm2_pointing_expand.hip, cosmomap2_amd/utilities/pointing_expand.py) against the
two restatements of _pointing_expand_ref.py: pixels equal to the long-double restatement (L) on every sample of the
committed sets (tests/test_pointing_expand_cpu.py checks that none of them is undecided), cos 2 psi and sin 2 psi
equal to the double restatement (E) bit for bit, and with a plate angle within (k_E + k_dev) 2^-53 2 of (L), k_E being
the largest difference of (E) from (L) on the same set, and within (sqrt(2) (k_dev + 1) + 3) 2^-53 of (E).

k_dev: no document of the installed ROCm states a maximum error of the double-precision device sin / cos (no file
under its tree mentions ulps for them), so K_DEV = 4 is taken.

Every output lies in a sentinel-guarded buffer (_guarded.py); the guards are checked after every call.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _pointing_expand_ref as R
from _guarded import Guarded

pytestmark = pytest.mark.gpu

D_CHUNK = 8                                  # kDetChunk of cm2_pointing_expand.hip
NDETS = (1, D_CHUNK - 1, D_CHUNK, D_CHUNK + 1, 2 * D_CHUNK + 1)
K_DEV = 4.0
_DBLP = ctypes.POINTER(ctypes.c_double)
_NAN_HI = 0x7FF80000                         # upper half of the NaN an output buffer holds before the call


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    return SimpleNamespace(I=I, U=U, D=D, hip=_hip, torch=torch)


class Out(object):
    """Guarded outputs of one call: n int32 pixels (in the doubles of a Guarded) and n cos, n sin."""

    def __init__(self, cm, n, pol=3):
        self.cm, self.n = cm, n
        self.gp = Guarded(cm, (n + 1) // 2)
        self.pix = self.gp.v.view(cm.torch.int32)[:n]
        self.gc = Guarded(cm, n) if pol > 1 else None
        self.gs = Guarded(cm, n) if pol > 1 else None

    def tensors(self):
        return (self.pix, None if self.gc is None else self.gc.v, None if self.gs is None else self.gs.v)

    def intact(self, what):
        self.gp.intact(what + " (pix)")
        if self.n & 1:                                     # the spare int32 behind an odd count
            assert int(self.gp.v.view(self.cm.torch.int32)[self.n].item()) == _NAN_HI, what
        for g in (self.gc, self.gs):
            if g is not None:
                g.intact(what)

    def untouched(self, what):
        """Nothing written at all: every output still holds the NaN it was filled with."""
        self.intact(what)
        raw = self.gp.v.view(self.cm.torch.int64)
        assert bool((raw == 0x7FF8000000000000).all().item()), what
        for g in (self.gc, self.gs):
            if g is not None:
                assert bool(self.cm.torch.isnan(g.v).all().item()), what

    def get(self):
        self.cm.torch.cuda.synchronize()
        return (self.pix.cpu().numpy().copy(), None if self.gc is None else self.gc.get(),
                None if self.gs is None else self.gs.get())


def run(cm, bore, det, nside, nest=False, pol=3, **kw):
    ndet, ns = len(det), len(bore)
    o = Out(cm, ndet * ns, pol)
    ret = cm.U.expand_pointing(bore, det, nside, nest=nest, pol=pol, out=o.tensors(), **kw)
    assert ret[0] is o.pix and (pol == 1 or (ret[1] is o.gc.v and ret[2] is o.gs.v))
    o.intact("expand_pointing ndet %d ns %d nside %d nest %s" % (ndet, ns, nside, nest))
    p, c, s = o.get()
    shape = (ndet, ns)
    return p.reshape(shape), None if c is None else c.reshape(shape), None if s is None else s.reshape(shape)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


SHAPES = [(nd, R.NS) for nd in NDETS] + [(D_CHUNK + 1, n) for n in (1, 63, 257)]


# ------------------------------------------------------------- 1: pixels ------
@pytest.mark.parametrize("nest", [False, True])
@pytest.mark.parametrize("nside", R.NSIDES)
@pytest.mark.parametrize("kind", ["random", "scan"])
def test_pixels_equal_the_long_double_restatement(cm, kind, nside, nest):
    b, d = R.inputs(kind)
    L = R.reference_L(kind, nside, nest)
    assert L.decided.all()
    bd, dd = cm.D.f64(b), cm.D.f64(d)
    for nd, ns in SHAPES:
        pix, _, _ = run(cm, bd[:ns].contiguous(), dd[:nd].contiguous(), nside, nest)
        bad = np.argwhere(pix != L.pix[:nd, :ns])
        assert bad.size == 0, ("first of %d differing (detector, sample): %r, got %d, want %d"
                               % (len(bad), tuple(bad[0]), pix[tuple(bad[0])], L.pix[tuple(bad[0])]))


# ------------------------------------------------------------- 2: angles without a plate ------
@pytest.mark.parametrize("kind", ["random", "scan"])
def test_angles_equal_the_double_restatement_bit_for_bit(cm, kind):
    b, d = R.inputs(kind)
    E = R.reference_E(kind, 64, False)
    for nd, ns in SHAPES:
        for nest in (False, True):
            _, c, s = run(cm, b[:ns], d[:nd], 64, nest)
            assert same_bits(c, E[1][:nd, :ns]), (kind, nd, ns, "cos", int((c != E[1][:nd, :ns]).sum()))
            assert same_bits(s, E[2][:nd, :ns]), (kind, nd, ns, "sin", int((s != E[2][:nd, :ns]).sum()))


# ------------------------------------------------------------- 3: angles with a plate ------
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("kind", ["random", "scan"])
def test_angles_with_a_plate_within_the_bound(cm, kind, big):
    b, d = R.inputs(kind)
    nd = D_CHUNK + 1
    chi = R.hwp_angles(big=big)
    E, L = R.expand_E(b, d[:nd], 64, False, hwp=chi), R.expand_L(b, d[:nd], 64, False, hwp=chi)
    pix, c, s = run(cm, b, d[:nd], 64, False, hwp=chi)
    np.testing.assert_array_equal(pix, L.pix)
    # against (L): k_E is the largest difference of (E) from (L) on this set with this chi, measured here
    k_e = float(np.maximum(np.abs(E[1].astype(R.LD) - L.cos), np.abs(E[2].astype(R.LD) - L.sin)).max()) / R.U
    err = np.maximum(np.abs(c.astype(R.LD) - L.cos), np.abs(s.astype(R.LD) - L.sin)).astype(np.float64)
    bound = (k_e + K_DEV) * R.U * 2.0
    # against (E): the same cos 2 psi, sin 2 psi bit for bit (the test above), so the two differ by sincos(4 chi) --
    # k_dev ulps on the device, one on the host, of values below 1 (an ulp is at most 2^-53), weighted by
    # |cos 2 psi| + |sin 2 psi| <= sqrt(2) -- and by the three roundings of the rotation on either side (half an ulp
    # of a value below 1 each): whatever the latitude
    err_e = np.maximum(np.abs(c - E[1]), np.abs(s - E[2]))
    bound_e = (np.sqrt(2.0) * (K_DEV + 1.0) + 3.0) * R.U
    print("\n%s, chi %s: k_E %.1f; largest error against (L) %.1f x 2^-53 (sin(theta) = %.3g), %.3g of the bound "
          "%.1f x 2^-53; against (E) %.2f x 2^-53, %.3g of the bound %.2f x 2^-53"
          % (kind, "near 1e6" if big else "2 Hz plate", k_e, err.max() / R.U, L.s.ravel()[err.argmax()],
             err.max() / bound, bound / R.U, err_e.max() / R.U, err_e.max() / bound_e, bound_e / R.U))
    assert (err <= bound).all()
    assert (err_e <= bound_e).all()
    # a device tensor of angles gives the same bytes as the host array
    _, c2, s2 = run(cm, b, d[:nd], 64, False, hwp=cm.D.f64(chi))
    assert same_bits(c, c2) and same_bits(s, s2)


# ------------------------------------------------------------- 4: the hand-made set ------
@pytest.mark.parametrize("nest", [False, True])
@pytest.mark.parametrize("nside", R.NSIDES)
def test_handmade_directions(cm, nside, nest):
    b, names = R.handmade()
    det = np.array([[0.0, 0.0, 0.0, 1.0]])
    E, L = R.expand_E(b, det, nside, nest), R.expand_L(b, det, nside, nest)
    pix, c, s = run(cm, b, det, nside, nest)
    for i, nm in enumerate(names):
        assert int(pix[0, i]) in L.allowed(0, i), (nm, int(pix[0, i]), L.allowed(0, i))
        if nm in ("+z", "-z", "+z rolled"):                # atan2(0, 0) = 0 on both sides
            assert pix[0, i] == E[0][0, i], nm
    assert same_bits(c, E[1]) and same_bits(s, E[2])


def test_flagged_samples(cm):
    b, d = R.random_inputs(3, ns=70)
    b = b.copy()
    b[5] = 0.0
    b[17, 2] = np.nan
    b[18, 3] = np.inf
    flags = np.zeros(70, dtype=np.uint8)
    flags[[0, 64, 69]] = (1, 255, 2)
    gone = [0, 5, 17, 18, 64, 69]
    E = R.expand_E(b, d, 64, True, flags=flags)
    for fl in (flags, flags.astype(bool), cm.D.to_dev(flags)):
        pix, c, s = run(cm, b, d, 64, True, flags=fl)
        assert (pix[:, gone] == -1).all() and (c[:, gone] == 1.0).all() and (s[:, gone] == 0.0).all()
        np.testing.assert_array_equal(pix, E[0])
        assert same_bits(c, E[1]) and same_bits(s, E[2])
    assert (pix >= 0).sum() == 3 * (70 - len(gone))


def test_frame_is_the_product_in_front(cm):
    b, d = R.scan_inputs(3, ns=257)
    frame = np.array([0.3, -0.2, 0.5, 0.7])                # not normalised: the product is normalised once
    want = run(cm, R.qmul_E(frame[None, :], b), d, 64, False)
    got = run(cm, b, d, 64, False, frame=frame)
    np.testing.assert_array_equal(got[0], want[0])
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    E = R.expand_E(b, d, 64, False, frame=frame)
    assert same_bits(got[1], E[1]) and same_bits(got[2], E[2])
    assert not np.array_equal(got[0], run(cm, b, d, 64, False)[0])


# ------------------------------------------------------------- 5: layout and variants ------
def test_rows_are_one_detector_calls(cm):
    b, d = R.inputs("scan")
    nd = D_CHUNK + 1
    chi = R.hwp_angles()
    pix, c, s = run(cm, b, d[:nd], 8192, True, hwp=chi)
    for k in range(nd):
        p1, c1, s1 = run(cm, b, d[k:k + 1], 8192, True, hwp=chi)
        np.testing.assert_array_equal(p1[0], pix[k])
        assert same_bits(c1[0], c[k]) and same_bits(s1[0], s[k])


def test_pol_1_and_out(cm):
    b, d = R.inputs("random")
    nd = 3
    pix, c, s = run(cm, b, d[:nd], 64, False)
    p1, c1, s1 = run(cm, b, d[:nd], 64, False, pol=1, hwp=R.hwp_angles())
    assert c1 is None and s1 is None
    np.testing.assert_array_equal(p1, pix)
    before = cm.torch.cuda.memory_allocated()
    fresh = cm.U.expand_pointing(cm.D.f64(b), cm.D.f64(d[:nd]), 64, pol=1)
    assert fresh[1] is None and fresh[2] is None and fresh[0].dtype == cm.torch.int32
    assert cm.torch.cuda.memory_allocated() - before < 8 * nd * R.NS      # the pixels; less than one angle array
    np.testing.assert_array_equal(fresh[0].cpu().numpy().reshape(nd, -1), pix)
    full = cm.U.expand_pointing(b, d[:nd], 64)
    assert full[0].is_cuda and full[0].dtype == cm.torch.int32 and full[1].dtype == cm.torch.float64
    assert tuple(full[0].shape) == (nd * R.NS,) == tuple(full[1].shape) == tuple(full[2].shape)
    assert same_bits(full[1].cpu().numpy().reshape(nd, -1), c)
    # two calls, the same bytes
    again = run(cm, b, d[:nd], 64, False)
    np.testing.assert_array_equal(again[0], pix)
    assert same_bits(again[1], c) and same_bits(again[2], s)


# ------------------------------------------------------------- 6: error codes ------
def test_error_codes_leave_the_outputs_untouched(cm):
    b, d = R.random_inputs(3, ns=100)
    bd, dd = cm.D.f64(b), cm.D.f64(d)
    lib = cm.hip.load()
    o = Out(cm, 300)
    pix, c, s = o.tensors()
    ptr = cm.D.ptr

    def call(ns=100, ndet=3, det=dd, frame=None, nside=64, cosp=ptr(c), sinp=ptr(s)):
        fr = None if frame is None else np.asarray(frame, dtype=np.float64).ctypes.data_as(_DBLP)
        rc = lib.cm2_pointing_expand(ns, ndet, ptr(bd), ptr(det), fr, None, None, nside, 0, ptr(pix), cosp, sinp,
                                     cm.D.stream())
        cm.torch.cuda.synchronize()
        return rc

    zero_det, nan_det = d.copy(), d.copy()
    zero_det[1] = 0.0
    nan_det[2, 0] = np.nan
    refused = [dict(nside=3), dict(nside=0), dict(nside=16384), dict(nside=-64), dict(ndet=0), dict(ns=-1),
               dict(sinp=None), dict(cosp=None), dict(det=cm.D.f64(zero_det)), dict(det=cm.D.f64(nan_det)),
               dict(frame=[0.0, 0.0, 0.0, 0.0]), dict(frame=[np.inf, 0.0, 0.0, 1.0])]
    for kw in refused:
        assert call(**kw) == cm.hip.ERR_ARGUMENT, kw
        assert lib.cm2_last_error()
        o.untouched("refused call %r" % (kw,))
    assert call(det=cm.D.f64(zero_det)) == 2 and b"detector 1" in lib.cm2_last_error()
    assert call(ns=0) == 0
    o.untouched("ns = 0")
    with pytest.raises(ValueError, match="detector 1"):
        cm.U.expand_pointing(bd, cm.D.f64(zero_det), 64)
    assert call() == 0
    o.intact("valid call")
    assert not np.isnan(o.get()[1]).any()


# ------------------------------------------------------------- 7: end to end ------
def test_expansion_feeds_the_pointing_operator(cm):
    nside, nd = 16, 3
    npix = 12 * nside * nside
    b, d = R.inputs("scan")
    d = d[:nd]
    flags = np.zeros(R.NS, dtype=np.uint8)
    flags[100:140] = 1
    pixs, c, s = cm.U.expand_pointing(b, d, nside, hwp=R.hwp_angles(), flags=flags)
    h_pix, h_c, h_s = cm.D.to_host(pixs).copy(), cm.D.to_host(c).copy(), cm.D.to_host(s).copy()
    assert (h_pix.reshape(nd, -1)[:, 100:140] == -1).all()
    with pytest.raises(ValueError):
        cm.U.ProcessTimeSamples(pixs, npix, pol=3, phi=np.zeros(nd * R.NS), cos_sin=(c, s))
    with pytest.raises(ValueError):
        cm.U.ProcessTimeSamples(pixs, npix, pol=3, cos_sin=(h_c, h_s))

    def chain(pix_in, **angles):
        ces = cm.U.ProcessTimeSamples(pix_in, npix, pol=3, **angles)
        n = ces.get_new_pixel[0]
        P = cm.I.SparseLO(n, nd * R.NS, pix_in, pol=3, angle_processed=ces)
        x = np.random.default_rng(3).standard_normal(3 * n)
        return n, ces, P.T * (P * x)

    n1, ces1, y1 = chain(pixs, cos_sin=(c, s))
    assert ces1._d_cos is c and ces1._d_sin is s             # adopted, not copied
    n2, _, y2 = chain(h_pix.copy(), cos_sin=(cm.D.f64(h_c), cm.D.f64(h_s)))
    assert n1 == n2 and 0 < n1 < npix
    assert same_bits(y1, y2)
    # through phi = atan2(sin, cos) / 2 the same operator to rounding
    n3, _, y3 = chain(h_pix.copy(), phi=0.5 * np.arctan2(h_s, h_c))
    assert n3 == n1
    assert np.linalg.norm(y3 - y1) <= 1e-12 * np.linalg.norm(y1)
