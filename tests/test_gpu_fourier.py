"""
The Fourier filter on the GPU against the extended-precision definition of _fourier_ref.py: every output sample within
c(L) E of ``ref_ld`` (E the error scale of the block, c(L) from the restatement's own loss on a CPU, times 8), the
response within its counted bound at every bin, a bad block all quiet NaN and no other block touched, the same bits
run to run, in place and from arrays no 16-byte access can reach, every overlap refused, the transpose through the
inner product, and a round trip from pointing to a map.  The cases are the shared ones of _fourier_ref.py
(test_fourier_cpu.py checks what they cover); buffers are the sentinel-guarded ones of _guarded.py.
"""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import _fourier_ref as R
import _pointing_expand_ref as PE
from _guarded import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    M = importlib.import_module("cosmomap2_amd.utilities.fourier_filter")
    return SimpleNamespace(U=U, I=I, M=M, hip=_hip, torch=torch, D=D, cg=cosmomap2_amd.cg)


def kwargs(P, **more):
    kw = dict(tau=P.tau, mode=("deconvolve", "convolve")[P.mode], lowpass=P.lp, highpass=P.hp, notch=P.notch,
              response=P.table, detrend=("none", "ends")[P.detrend], end_mean=P.end_mean, pad=P.pad,
              conjugate=bool(P.conjugate))
    kw.update(more)
    return kw


class Raw(object):
    """The C entry points on guarded buffers: the output comes back with its guards and the input checked."""

    def __init__(self, cm, sizes, P, **more):
        self.cm, self.sizes, self.nt = cm, list(sizes), sum(sizes)
        self.ff = cm.M.FourierFilter(self.sizes, P.fs, **kwargs(P, **more))
        self.g = self.ff._handle(self.nt, self.sizes)
        self.st = cm.D.stream()

    def apply(self, x, shift=0, inplace=False):
        """shift = 1: input and output start 8 bytes into their buffers, so no 16-byte access is possible"""
        cm = self.cm
        src = Guarded(cm, self.nt + shift, np.concatenate([np.full(shift, np.nan), x]))
        dst = src if inplace else Guarded(cm, self.nt + shift)
        cm.hip.call("cm2_fourier_apply", self.g.h, src.ptr + 8 * shift, dst.ptr + 8 * shift, self.st)
        got = dst.get()
        dst.intact("cm2_fourier_apply (output)")
        src.intact("cm2_fourier_apply (input)")
        if not inplace:
            assert np.array_equal(R.bits(src.get()[shift:]), R.bits(x)), "the input changed"
            assert shift == 0 or np.isnan(got[0])                             # the sample in front is not the output's
        return got[shift:]

    def response(self, b):
        L = R.fft_length(self.sizes[b], self.ff.pad)
        H = Guarded(self.cm, 2 * (L // 2 + 1))
        self.cm.hip.call("cm2_fourier_response", self.g.h, b, H.ptr, self.st)
        got = H.get()
        H.intact("cm2_fourier_response")
        return got.view(np.complex128)


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


# ----------------------------------------------------------------------- the shared cases ----
@pytest.mark.parametrize("name", R.CASES)
def test_cases_against_the_reference(cm, name):
    c = R.case(name)
    raw = Raw(cm, c.sizes, c.P)
    info = raw.g.info()
    lengths = [R.fft_length(n, c.P.pad) for n in c.sizes]
    order = list(dict.fromkeys(lengths))
    assert (info["nt"], info["nblocks"], info["lengths"]) == (sum(c.sizes), len(c.sizes), order)
    assert info["blocks"] == [lengths.count(L) for L in order] and info["bad_blocks"] == 0
    assert info["batches"] == [R.first_batch(L, lengths.count(L), 512 << 20) for L in order]
    got = raw.apply(c.x)
    share = R.assert_output(got, name)
    print("%s: |got - ref| <= %.3g of the bound c(L) E" % (name, share))
    assert raw.g.info()["bad_blocks"] == 0
    # the same bits again, in place, and from arrays that no 16-byte access can reach
    assert same_bits(raw.apply(c.x), got), "not reproducible"
    assert same_bits(raw.apply(c.x, inplace=True), got), "in place"
    assert same_bits(raw.apply(c.x, shift=1), got), "unaligned"
    assert same_bits(raw.apply(c.x, shift=1, inplace=True), got), "unaligned, in place"
    # the response as the kernel evaluates it, bin by bin
    for b in sorted({c.sizes.index(n) for n in set(c.sizes)} | set(range(min(len(c.sizes), 3)))):
        H = raw.response(b)
        ex = R.response_excess(H, c.P, b, lengths[b])
        print("%s: response of block %d at %.3g of its counted bound" % (name, b, ex))
        assert ex <= 1.0, (name, b, ex)
        assert H.imag[0] == 0 and H.imag[-1] == 0 and not np.signbit(H.imag[[0, -1]]).any()


def test_three_batches_with_a_short_last_one(cm):
    """seven blocks of one length under a cap that holds three rows: batches of 3, 3 and 1 real rows"""
    c = R.case("seven")
    sizes = [1000] * 7
    x = R.walk(11, 7000)
    row = R.row_bytes(1024)
    P = c.P
    # the plan's own work buffer counts against the cap and its size is the library's: of these caps one leaves three
    # rows, directly (three rows and at most one row's bytes of plan) or after one halving of six
    raw = None
    for cap in (3 * row + 512, 4 * row - 1, 6 * row + 512, 7 * row - 1):
        raw = Raw(cm, sizes, P, max_work_bytes=cap)
        info = raw.g.info()
        print("cap %d: batch %s, %d bytes of rows and plan" % (cap, info["batches"], info["work_bytes"]))
        assert info["work_bytes"] <= cap
        if info["batches"] == [3]:
            break
    assert info["lengths"] == [1024] and info["batches"] == [3] and info["blocks"] == [7], info
    want = SimpleNamespace(**dict(zip(("out", "E", "bad"), R.ref_ld(x, sizes, P))))
    got = raw.apply(x)
    share = R.assert_output_of(got, want, sizes, P.pad, "three batches")
    whole = Raw(cm, sizes, P).apply(x)
    assert Raw(cm, sizes, P).g.info()["batches"] == [7]
    R.assert_output_of(whole, want, sizes, P.pad, "one batch")
    print("three batches: %.3g of the bound; bit-equal to one batch: %s" % (share, same_bits(got, whole)))
    assert same_bits(raw.apply(x, inplace=True), got)
    # one row that does not fit is refused with the bytes it needs
    with pytest.raises(cm.hip.HipError) as e:
        Raw(cm, sizes, P, max_work_bytes=row - 1)
    assert e.value.status == cm.hip.ERR_ARGUMENT and str(row) in str(e.value), str(e.value)


# ------------------------------------------------------------------------------ bad blocks ----
@pytest.mark.parametrize("name,where", [("seven", {1: (0, np.inf), 2: (500, np.nan)}),
                                        ("edge_4095_4096_4097", {2: (4096, -np.inf)}),
                                        ("edge_4095_4096_4097", {0: (4094, np.nan), 1: (2000, np.inf)}),
                                        ("detrend_none", {1: (39, np.nan)})])
def test_a_bad_block_is_all_quiet_nan_and_no_other_block_changes(cm, name, where):
    c = R.case(name)
    raw = Raw(cm, c.sizes, c.P)
    clean = raw.apply(c.x)
    off = R.offsets(c.sizes)
    x = c.x.copy()
    for b, (i, v) in where.items():
        x[off[b] + i] = v
    for shift in (0, 1):
        got = raw.apply(x, shift=shift)
        for b in range(len(c.sizes)):
            sl = slice(off[b], off[b + 1])
            if b in where:
                assert (R.bits(got[sl]) == R.QUIET_NAN).all(), (name, b)
            else:
                assert same_bits(got[sl], clean[sl]), (name, b)
        assert raw.g.info()["bad_blocks"] == len(where)
    assert same_bits(raw.apply(x, inplace=True), got)
    assert same_bits(raw.apply(c.x), clean) and raw.g.info()["bad_blocks"] == 0     # the count is the last apply's


# ------------------------------------------------------------------ guards and overlap ----
def test_overlaps_and_bad_arguments_are_refused(cm):
    c = R.case("seven")
    raw = Raw(cm, c.sizes, c.P)
    nt = raw.nt
    buf = Guarded(cm, 3 * nt, R.walk(9, 3 * nt))
    before = buf.get()
    p, st = buf.ptr, raw.st

    def refused(name, *args):
        with pytest.raises(cm.hip.HipError) as e:
            cm.hip.call(name, *args)
        assert e.value.status == cm.hip.ERR_ARGUMENT and name in str(e.value), str(e.value)

    ap = "cm2_fourier_apply"
    refused(ap, raw.g.h, p, p + 8, st)                                        # shifted by one sample
    refused(ap, raw.g.h, p + 8, p, st)
    refused(ap, raw.g.h, p, p + 8 * (nt - 1), st)                             # one shared sample
    refused(ap, raw.g.h, p + 8 * (nt - 1), p, st)
    refused(ap, raw.g.h, None, p, st)
    refused(ap, raw.g.h, p, None, st)
    refused("cm2_fourier_response", raw.g.h, len(c.sizes), p, st)
    refused("cm2_fourier_response", raw.g.h, -1, p, st)
    refused("cm2_fourier_response", raw.g.h, 0, None, st)
    assert same_bits(buf.get(), before)
    buf.intact("refused calls")
    cm.hip.call(ap, raw.g.h, p, p + 8 * nt, st)                               # right behind the input is none of it
    got = buf.get()
    assert same_bits(got[:nt], before[:nt]) and same_bits(got[2 * nt:], before[2 * nt:])
    assert not same_bits(got[nt:2 * nt], before[nt:2 * nt])
    buf.intact("the accepted call")


# --------------------------------------------------------------------------- transposes ----
def _inner_bound(u, v, sizes, P):
    """the bound on |<u, F v> - <u, F v>_exact| for F v within c(L) E of the definition: sum |u_i| c E_i(v)"""
    c = np.concatenate([np.full(n, R.c_out(R.fft_length(n, P.pad))) for n in sizes])
    return float((np.abs(u) * c * R.error_scale(v, sizes, P)).sum())


@pytest.mark.parametrize("name", ["seven_conjugate", "table_complex", "highpass_4", "notch_16"])
def test_the_transpose_through_the_inner_product(cm, name):
    """<u, F v> = <F^T u, v> with F^T the conjugate handle (complex H), <u, F v> = <F u, v> for a real H; each within
    the two sides' E (the dot products are formed in extended precision)."""
    c = R.case(name)
    P = c.P.but(detrend=0, conjugate=0)
    nt = sum(c.sizes)
    kw = kwargs(P)
    kw.pop("conjugate")
    F = cm.I.FourierFilterLO(c.sizes, P.fs, **kw)
    real = P.tau is None and P.table_kind != 2
    assert F.symmetric == real and F.shape == (nt, nt) and (F.T is F) == real
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal(nt), R.walk(4, nt)
    Fv, Ftu = F * v, F.T * u
    lhs, rhs = float(np.dot(u.astype(R.LD), Fv)), float(np.dot(Ftu.astype(R.LD), v))
    bound = _inner_bound(u, v, c.sizes, P) + _inner_bound(v, u, c.sizes, P.but(conjugate=1))
    print("%s: <u, F v> - <F^T u, v> = %.3g, bound %.3g (of %.3g)" % (name, lhs - rhs, bound, abs(lhs)))
    assert abs(lhs - rhs) <= bound
    if not real:                                                              # and the transpose is not F itself
        assert abs(float(np.dot((F * u).astype(R.LD), v)) - lhs) > 1e6 * bound
    # the conjugate handle against the definition
    want = SimpleNamespace(**dict(zip(("out", "E", "bad"), R.ref_ld(u, c.sizes, P.but(conjugate=1)))))
    R.assert_output_of(Ftu, want, c.sizes, P.pad, name + " transposed")
    E = cm.I.FourierFilterLO(c.sizes, P.fs, **dict(kw, detrend="ends"))
    with pytest.raises(ValueError):
        E.T * u
    assert E.filter_info()["lengths"] == F.filter_info()["lengths"]


# --------------------------------------------------------------------------- Python layer ----
def test_python_layer_gives_the_same_results(cm):
    c = R.case("all")
    raw = Raw(cm, c.sizes, c.P)
    want = raw.apply(c.x)
    kw = kwargs(c.P)
    kw.pop("conjugate")
    ff = cm.U.FourierFilter(c.sizes, c.P.fs, **kw)
    got = ff.apply(c.x)
    assert isinstance(got, np.ndarray) and same_bits(got, want)
    t = cm.D.to_dev(c.x)
    dev = ff.apply(t)
    assert cm.D.is_tensor(dev) and dev.is_cuda and same_bits(cm.D.to_host(dev), want)
    assert same_bits(cm.D.to_host(t), c.x)
    out = cm.D.empty(len(c.x))
    assert ff.apply(t, out=out) is out and same_bits(cm.D.to_host(out), want)
    assert ff.apply(t, out=t) is t and same_bits(cm.D.to_host(t), want)       # in place
    host = np.empty(len(c.x))
    assert ff.apply(c.x, out=host) is host and same_bits(host, want)
    assert same_bits(cm.U.fourier_filter(c.x, c.sizes, c.P.fs, **kw), want)
    info = ff.info()
    assert info["lengths"] == [1024, 750] and info["blocks"] == [2, 1] and info["bad_blocks"] == 0
    assert info["work_bytes"] >= 2 * R.row_bytes(1024)
    for b in range(3):
        assert same_bits(ff.response(b).view(np.float64), raw.response(b).view(np.float64))
        assert ff.fft_length(b) == info["lengths"][0 if b != 1 else 1]
        assert ff.response(b).size == ff.fft_length(b) // 2 + 1
    # the one-call deconvolution is the filter with a time constant and a low-pass; a scalar tau is every block's
    d = R.case("seven")
    tau = 5 / R.FS
    one = cm.U.deconvolve_time_constant(d.x, d.sizes, R.FS, tau, lowpass=R.LP4)
    two = cm.U.FourierFilter(d.sizes, R.FS, tau=[tau] * 7, lowpass=R.LP4).apply(d.x)
    assert same_bits(one, two)
    with pytest.raises(cm.hip.HipError):                                     # a refusal of the library reaches the caller
        cm.U.FourierFilter(d.sizes, R.FS, max_work_bytes=100).apply(d.x)


# --------------------------------------------------------------------------- end to end ----
def test_end_to_end_time_constants_are_undone_in_the_map(cm):
    """Eight detectors from expand_pointing scan a smooth sky along a meridian; each stream is convolved with its own
    time constant (mode="convolve"), deconvolved with a low-pass (deconvolve_time_constant) and mapped by cg(P^T P).
    The map is compared with the map of the same streams only low-passed.

    The sky is exactly 0 for the first and the last 900 samples of every block, so both end means are 0, the trend is
    0, and what the zero padding cuts off the convolved stream, e^(-900 / 5) of it at the longest time constant, is 0
    in double precision: in exact arithmetic deconvolve(convolve(x)) with the low-pass IS the low-passed x, but for the
    Nyquist bin, where the two responses are not inverse (the definition drops the imaginary part there); the sky is
    smooth, the bin holds next to nothing of it and the low-pass leaves 1.6e-3 of that (asserted).  What is left is
    rounding.  Per block, with c = c(L) and E the error scale of a call:
        the low-passed stream B:            |B - B_exact| <= c E_lp
        the convolved stream y:             |y - y_exact| <= c E_conv =: e
        the deconvolved stream A = F2 y:    |A - F2_exact y| <= c E_dec, and F2_exact, linear, takes the error e of
        its input to at most (2 max|H_dec| sqrt(n) + 1) max e: the trend of e is at most max e, the filter's l2 gain is
        max|H_dec| on an input of norm at most 2 sqrt(n) max e, and Re H(0) = 1 puts the trend back.
    A pixel of the binned map is a mean of samples, so the streams' bound is the map's, plus the rounding of the
    mean itself, hits 2^-53 max|d| per map, plus what the solver leaves (asserted against the binned map)."""
    nside, nd, fs = 16, 8, 100.0
    npix, ns = 12 * nside * nside, PE.NS
    i = np.arange(ns)
    theta = 0.4 + 2.2 * i / ns
    bore = PE.qmul_E(PE._rot(2, np.full(ns, 0.7)), PE._rot(1, theta))
    dets = PE._rot(2, np.linspace(0.0, 1.4, nd))
    pixs, _, _ = cm.U.expand_pointing(bore, dets, nside)
    s = (theta - 0.9) / 1.2
    inside = (s > 0) & (s < 1)
    sky = np.where(inside, np.sin(np.pi * s) ** 4 * (1.0 + 0.5 * np.sin(7 * np.pi * s)), 0.0)
    quiet = int(np.flatnonzero(inside)[0])
    assert quiet >= 900 and ns - 1 - int(np.flatnonzero(inside)[-1]) >= 900 and not sky[:900].any() and not sky[-900:].any()
    sizes = [ns] * nd
    x = np.tile(sky, nd)
    tau = (1.0 + 4.0 * np.arange(nd) / (nd - 1)) / fs                          # 1 .. 5 samples
    lp = (10.0, 4)
    L = R.fft_length(ns, 1024)
    assert L in R.WORST and np.exp(-900 / (tau.max() * fs)) < 2.0 ** -200
    nyquist = abs(float(np.sum(np.where(i % 2 == 0, 1.0, -1.0) * sky))) / L / np.sqrt(1 + (0.5 * fs / lp[0]) ** (2 * lp[1]))
    assert nyquist < 1e-17
    conv = cm.U.FourierFilter(sizes, fs, tau=tau, mode="convolve")
    y = conv.apply(cm.D.to_dev(x))
    A = cm.U.deconvolve_time_constant(y, sizes, fs, tau, lowpass=lp)
    B = cm.U.fourier_filter(cm.D.to_dev(x), sizes, fs, lowpass=lp)
    Y = cm.U.fourier_filter(y, sizes, fs, lowpass=lp)                         # no deconvolution
    # the propagated bound
    c = R.c_out(L)
    Pc, Pd, Pl = R.Par(fs, tau=tau, mode=1), R.Par(fs, tau=tau, lp=lp), R.Par(fs, lp=lp)
    h_y = cm.D.to_host(y)
    E_conv, E_dec, E_lp = R.error_scale(x, sizes, Pc), R.error_scale(h_y, sizes, Pd), R.error_scale(x, sizes, Pl)
    gain = max(float(np.sqrt(H.re ** 2 + H.im ** 2).max()) for H in (R.response_ld(Pd, b, L) for b in range(nd)))
    stream_bound = c * E_lp.max() + c * E_dec.max() + (2 * gain * np.sqrt(ns) + 1) * c * E_conv.max()
    h_A, h_B = cm.D.to_host(A), cm.D.to_host(B)
    print("streams: |A - B| <= %.3g, bound %.3g (max |H_dec| = %.3g)" % (np.abs(h_A - h_B).max(), stream_bound, gain))
    assert np.abs(h_A - h_B).max() <= stream_bound
    # the maps
    ces = cm.U.ProcessTimeSamples(pixs.clone(), npix, pol=1)
    n, obspix = ces.get_new_pixel
    P = cm.I.SparseLO(n, nd * ns, ces.pixs, pol=1, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=1)
    hits = np.bincount(cm.D.to_host(pixs), minlength=npix).max()
    maps = []
    for stream in (A, B, Y):
        m, info = cm.cg(P.T * P, P.T * stream, M=Mbd, rtol=1e-12, maxiter=50)
        m = np.asarray(cm.D.to_host(m))
        binned = np.asarray(cm.D.to_host(Mbd * (P.T * stream)))
        assert info == 0 and np.abs(m - binned).max() <= 1e-12
        maps.append(m)
    map_bound = stream_bound + 2 * hits * 2.0 ** -53 * np.abs(x).max() + 2e-12
    err, err_none = np.abs(maps[0] - maps[1]).max(), np.abs(maps[2] - maps[1]).max()
    print("map: deconvolved - low-passed only <= %.3g (bound %.3g); without deconvolution %.3g" % (err, map_bound, err_none))
    assert err <= map_bound
    assert err_none > map_bound and err_none > 1e-4                           # the smear tau v_scan is in the map
