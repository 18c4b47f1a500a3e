"""
The HWP-synchronous signal filter on the GPU (cm2_hwpss_*, HWPSSFilterLO) against tests/_hwpss_ref.py.

Acceptance, element by element: bit-equal to the float64 restatement (run from the device's own tables), or within
c 2^-53 S of the extended-precision reference; exactly 0 where S = 0 (flagged samples, skipped units).  c comes from
_hwpss_ref.py (operation count x the CPU-measured headroom) and is never measured here.  The tables are held to
2 x 2^-53 of the long-double cos / sin of the same float64 chi.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hwpss_ref as R  # noqa: E402
import _pointing_expand_ref as PE  # noqa: E402
from _guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
LD, U53 = R.LD, R.U53


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device
    from cosmomap2_amd.interfaces import linearoperators as L
    return SimpleNamespace(I=I, U=U, L=L, D=device, hip=_hip, cg=cosmomap2_amd.cg, torch=torch)


_made = {}


def made(cm, H, rate):
    """the operator of a shared case and the restatement run from ITS tables, once per process"""
    key = (H, rate)
    if key not in _made:
        cs = R.case(H, rate)
        F = cm.I.HWPSSFilterLO(cs.chi, cs.pix, ndet=cs.ndet, nharm=H, chunks=cs.edges)
        c1, s1 = [cm.D.to_host(t).copy() for t in F.harmonic_tables()]
        fact = R.factor_f64(c1, s1, cs.pix, cs.ndet, cs.edges, H)
        f64 = R.hwpss_f64(c1, s1, cs.pix, cs.ndet, cs.edges, H, cs.v, fact)
        _made[key] = SimpleNamespace(F=F, c1=c1, s1=s1, fact=fact, f64=f64)
    return _made[key]


def same_bits(a, b):
    return np.array_equal(R.bits(np.asarray(a)), R.bits(np.asarray(b)))


def unit_slices(cs):
    for k in range(cs.ndet):
        for c in range(len(cs.lens)):
            yield k, c, slice(k * cs.ns + int(cs.edges[c]), k * cs.ns + int(cs.edges[c + 1]))


# ---------------------------------------------------------------- 1: the tables ----
@pytest.mark.parametrize("rate", sorted(R.RATES))
def test_tables_are_within_an_ulp_of_the_long_double_values(cm, rate):
    cs = R.case(4, rate)
    m = made(cm, 4, rate)
    for got, want in ((m.c1, np.cos(R._ld(cs.chi))), (m.s1, np.sin(R._ld(cs.chi)))):
        err = float(np.abs(R._ld(got) - want).max() / U53)
        print("%s: tables off by %.3f x 2^-53 at most" % (rate, err))
        assert err <= 2.0


# ------------------------------------------------------------ 2: apply and fit ----
@pytest.mark.parametrize("H,rate", R.CASES)
def test_apply_and_fit_on_the_shared_cases(cm, H, rate):
    cs = R.case(H, rate)
    m = made(cm, H, rate)
    _, ref = R.case_ref(H, rate)
    F, K, C = m.F, cs.K, len(cs.lens)
    d_in = Guarded(cm, cs.nt, cs.v)
    d_out, d_cf = Guarded(cm, cs.nt), Guarded(cm, cs.ndet * C * K)
    st = cm.D.stream()
    cm.hip.call("cm2_hwpss_apply", F._handle.h, d_in.ptr, d_out.ptr, st)
    cm.hip.call("cm2_hwpss_fit", F._handle.h, d_in.ptr, d_cf.ptr, st)
    out, cf = d_out.get(), d_cf.get().reshape(cs.ndet, C, K)
    for g in (d_in, d_out, d_cf):
        g.intact("case %r" % ((H, rate),))
    assert same_bits(d_in.get(), cs.v)
    # the counts, then the zeros
    info = F.filter_info()
    want = dict(ns=cs.ns, ndet=cs.ndet, nchunks=C, nharm=H, fitted=int((ref.marks == 0).sum()),
                skipped_few=int((ref.marks == 1).sum()), skipped_pivot=int((ref.marks == 2).sum()),
                segment=R.SEG, segments=cs.ndet * int(R.segments_of(cs.edges).sum()))
    assert info == want and info["skipped_few"] >= 2 and info["skipped_pivot"] >= 3
    assert np.array_equal(m.f64.marks, ref.marks)
    assert not out[cs.pix < 0].any()
    for k, c, sl in unit_slices(cs):
        if ref.marks[k, c]:
            assert not out[sl].any() and not cf[k, c].any(), (k, c)
    # element by element
    same_o = float((R.bits(out) == R.bits(m.f64.out)).mean())
    same_c = float((R.bits(cf) == R.bits(m.f64.coeff)).mean())
    eo = R.assert_accepted(out, m.f64.out, ref.out, ref.S, R.c_samples(cs.ndet, cs.edges, H), "apply")
    ec = R.assert_accepted(cf, m.f64.coeff, ref.coeff, ref.Sc, R.c_coeffs(cs.ndet, cs.edges, H), "fit")
    print("H=%d %s: %.4f of the outputs and %.4f of the coefficients bit-equal to the restatement; the others use "
          "%.3g / %.3g of the bound" % (H, rate, same_o, same_c, eo, ec))
    # the operator's own methods: the same bits, and the same bits again
    y = F * cs.v
    assert isinstance(y, np.ndarray) and same_bits(y, out) and same_bits(F.mult(cs.v), out)
    assert same_bits(F.coefficients(cs.v), cf) and F.coefficients(cs.v).shape == (cs.ndet, C, K)
    assert F.shape == (cs.nt, cs.nt) and F.symmetric


# ------------------------------------------------------------------- 3: a NaN ----
def test_a_nan_stays_in_its_unit(cm):
    H, rate = 4, "fast"
    cs = R.case(H, rate)
    F = made(cm, H, rate).F
    clean = F * cs.v
    c_hit = cs.lens.index(R.SEG + 1)
    ok = cs.pix >= 0
    for what in ("valid", "flagged"):
        v = cs.v.copy()
        cand = np.flatnonzero(ok if what == "valid" else ~ok)
        lo, hi = cs.ns + int(cs.edges[c_hit]), cs.ns + int(cs.edges[c_hit + 1])     # detector 1: 30 % flags
        at = cand[(cand >= lo) & (cand < hi)][-1]
        v[at] = np.nan
        got = F * v
        for k, c, sl in unit_slices(cs):
            if (k, c) == (1, c_hit) and what == "valid":
                assert np.isnan(got[sl][ok[sl]]).all() and not got[sl][~ok[sl]].any()
            else:
                assert same_bits(got[sl], clean[sl]), (what, k, c)


# ------------------------------------------------- 4: device and host inputs ----
def test_device_tensors_and_host_arrays_give_the_same_bits(cm):
    H, rate = 8, "slow"
    cs = R.case(H, rate)
    m = made(cm, H, rate)
    pix_t, chi_t, v_t = cm.D.i32(cs.pix), cm.D.f64(cs.chi), cm.D.f64(cs.v)
    Fd = cm.I.HWPSSFilterLO(chi_t, pix_t, ndet=cs.ndet, nharm=H, chunks=cs.edges)
    assert Fd._d_pix.data_ptr() == pix_t.data_ptr()                     # adopted, not copied
    y = Fd * v_t
    assert cm.D.is_dev(y) and same_bits(cm.D.to_host(y), m.F * cs.v)
    cf = Fd.coefficients(v_t)
    assert cm.D.is_dev(cf) and same_bits(cm.D.to_host(cf), m.F.coefficients(cs.v))
    assert Fd.filter_info() == m.F.filter_info()
    # an int chunk length and None plan as hwpss_plan says
    F1 = cm.I.HWPSSFilterLO(cs.chi[:5000], cs.pix[:5000], nharm=2, chunks=2048)
    assert F1.filter_info()["nchunks"] == 3 and F1.filter_info()["segments"] == 3
    F2 = cm.I.HWPSSFilterLO(cs.chi[:5000], cs.pix[:5000], nharm=2)
    assert F2.filter_info()["nchunks"] == 1 and F2.filter_info()["segments"] == 2


# ------------------------------------------------------------- 5: error codes ----
def test_refused_calls_leave_their_outputs_untouched(cm):
    H, rate = 1, "fast"
    cs = R.case(H, rate)
    F = made(cm, H, rate).F
    lib, st, h = cm.hip.load(), cm.D.stream(), F._handle.h
    C, K = len(cs.lens), cs.K
    d_in, d_out, d_cf = Guarded(cm, cs.nt, cs.v), Guarded(cm, cs.nt), Guarded(cm, cs.ndet * C * K)
    d_c, d_s = Guarded(cm, cs.ns), Guarded(cm, cs.ns)

    def untouched(what):
        for g in (d_out, d_cf, d_c, d_s):
            g.intact(what)
            assert np.isnan(g.get()).all(), what + ": an output was written"
        assert same_bits(d_in.get(), cs.v), what

    refused = [
        ("cm2_hwpss_apply", (None, d_in.ptr, d_out.ptr, st)),
        ("cm2_hwpss_apply", (h, None, d_out.ptr, st)),
        ("cm2_hwpss_apply", (h, d_in.ptr, None, st)),
        ("cm2_hwpss_apply", (h, d_in.ptr, d_in.ptr, st)),                       # aliased
        ("cm2_hwpss_apply", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),     # overlapping by one element
        ("cm2_hwpss_fit", (None, d_in.ptr, d_cf.ptr, st)),
        ("cm2_hwpss_fit", (h, None, d_cf.ptr, st)),
        ("cm2_hwpss_fit", (h, d_in.ptr, None, st)),
        ("cm2_hwpss_fit", (h, d_in.ptr, d_in.ptr + 8, st)),
        ("cm2_hwpss_tables", (None, d_c.ptr, d_s.ptr, st)),
        ("cm2_hwpss_tables", (h, None, d_s.ptr, st)),
        ("cm2_hwpss_tables", (h, d_c.ptr, None, st)),
        ("cm2_hwpss_tables", (h, d_c.ptr, d_c.ptr, st)),
    ]
    for name, args in refused:
        assert getattr(lib, name)(*args) == cm.hip.ERR_ARGUMENT, (name, args)
        assert lib.cm2_last_error()
        untouched("%s%r" % (name, args))
    assert lib.cm2_hwpss_info(None, (ctypes.c_int64 * 9)()) == cm.hip.ERR_ARGUMENT
    # create: the handle variable keeps its value
    chi_t, pix_t = cm.D.f64(cs.chi), cm.D.i32(cs.pix)
    MARK = 0x1234
    I64 = ctypes.c_int64

    def create(ns=cs.ns, ndet=cs.ndet, edges=cs.edges, chi=chi_t, pix=pix_t, nharm=H, out=True):
        e = None if edges is None else (I64 * len(edges))(*[int(x) for x in edges])
        nch = 0 if edges is None else len(edges) - 1
        hv = ctypes.c_void_p(MARK)
        rc = lib.cm2_hwpss_create(ctypes.byref(hv) if out else None, ns, ndet, nch, e, cm.D.ptr(chi), cm.D.ptr(pix),
                                  nharm, st)
        return rc, hv

    for kw in (dict(nharm=0), dict(nharm=9), dict(nharm=-1), dict(ns=0, edges=[0, 0]), dict(ndet=0),
               dict(edges=[0, cs.ns - 1]), dict(edges=[1, cs.ns]), dict(edges=[0, 100, 100, cs.ns]),
               dict(edges=[0, 200, 100, cs.ns]), dict(edges=None), dict(chi=None), dict(pix=None),
               dict(ns=1 << 40, edges=[0, 1 << 40]), dict(ns=1 << 30, ndet=(1 << 16) + 1, edges=[0, 1 << 30]),
               dict(ns=1 << 20, ndet=1 << 23, edges=[0, 1 << 20])):
        rc, hv = create(**kw)
        assert rc == cm.hip.ERR_ARGUMENT and hv.value == MARK, kw
        assert lib.cm2_last_error()
    assert create(out=False)[0] == cm.hip.ERR_ARGUMENT
    untouched("after the refused creates")
    rc, hv = create()
    assert rc == 0 and hv.value not in (None, MARK)
    assert lib.cm2_hwpss_apply(hv, d_in.ptr, d_out.ptr, st) == 0
    assert lib.cm2_hwpss_tables(hv, d_c.ptr, d_s.ptr, st) == 0
    assert same_bits(d_out.get(), F * cs.v) and same_bits(d_c.get(), made(cm, H, rate).c1)
    for g in (d_out, d_c, d_s):
        g.intact("valid calls")
    assert lib.cm2_hwpss_destroy(hv) == 0 and lib.cm2_hwpss_destroy(None) == 0
    with pytest.raises(cm.L.lp.ShapeError):
        F * cs.v[:-1]


# --------------------------------------------------------- 6: the tiled chain ----
def test_filter_between_tile_order_P_and_Pt(cm):
    rng = np.random.default_rng(31)
    ndet, ns, npix, pol = 3, 5001, 300, 3
    nt = ndet * ns
    p = rng.integers(0, npix, nt).astype(np.int32)
    p[rng.random(nt) < 0.1] = -1
    phi = rng.uniform(0, np.pi, nt)
    chi = 50.0 + 0.13 * np.arange(ns) + 0.002 * rng.standard_normal(ns)
    ang = type("Ang", (), {"cos": np.cos(2 * phi), "sin": np.sin(2 * phi)})()
    P = cm.I.SparseLO(npix, nt, p, pol=pol, angle_processed=ang)
    Fh = cm.I.HWPSSFilterLO(chi, p, ndet=ndet, nharm=4, chunks=2048)
    assert Fh._tile_compatible(P) and not hasattr(Fh, "_apply_tiles")
    other = p.copy()
    other[np.flatnonzero(other >= 0)[0]] = -1
    assert not cm.I.HWPSSFilterLO(chi, other, ndet=ndet, nharm=4, chunks=2048)._tile_compatible(P)
    x = rng.standard_normal(pol * npix)
    exact = P.T * (Fh * (P * x))
    cm.L.set_pointing_mode("tiled")
    try:
        A = P.T * Fh * P
        assert any(isinstance(op, cm.L._TiledNormalLO) for op in A._compiled())
        y1, y2 = np.asarray(A * x), np.asarray(A * x)
    finally:
        cm.L.set_pointing_mode("auto")
    assert same_bits(y1, y2)
    # what the existing tile tests allow for the tile-order P^T (test_gpu_round2.py): 1e-12 of the norm
    assert np.linalg.norm(y1 - exact) <= 1e-12 * np.linalg.norm(exact)


# ------------------------------------------------------------- 7: end to end ----
def test_plate_harmonics_do_not_reach_the_map(cm):
    """expand_pointing(hwp=chi) -> P; d = P m + noise, with and without plate harmonics 1, 2 and 4 a thousand times
    the noise; filter, bin, M_BD.  The two maps may differ by what the rounding of the two filter applications
    (c 2^-53 S each) and of P^T and M_BD gives, pushed through |M_BD| |P|^T."""
    nside, nd, H = 16, 3, 4
    npix, ns = 12 * nside * nside, PE.NS
    b, dq = PE.inputs("scan")
    chi = PE.hwp_angles()
    pixs, c, s = cm.U.expand_pointing(b, dq[:nd], nside, hwp=chi)
    ces = cm.U.ProcessTimeSamples(pixs, npix, pol=3, cos_sin=(c, s))
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nd * ns, pixs, pol=3, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=3)
    edges = cm.I.hwpss_plan(ns, [0, 2048, ns])
    Fh = cm.I.HWPSSFilterLO(chi, pixs, ndet=nd, nharm=H, chunks=edges)
    assert Fh.filter_info()["fitted"] == nd * (len(edges) - 1)
    rng = np.random.default_rng(77)
    m_true = rng.standard_normal(3 * n)
    base = np.asarray(P * m_true) + rng.standard_normal(nd * ns)
    amp = 1.0e3 * rng.standard_normal((nd, 6))
    t = np.tile(chi, nd).reshape(nd, ns)
    hw = sum(amp[:, [2 * i]] * np.cos(k * t) + amp[:, [2 * i + 1]] * np.sin(k * t) for i, k in enumerate((1, 2, 4)))
    dirty = base + hw.reshape(-1)
    to_map = lambda v: np.asarray(Mbd * (P.T * v))
    f_dirty, f_base = np.asarray(Fh * dirty), np.asarray(Fh * base)
    map_dirty, map_base, map_raw = to_map(f_dirty), to_map(f_base), to_map(dirty)
    # the bound, on the host
    h_pix, h_c, h_s = cm.D.to_host(pixs), cm.D.to_host(c), cm.D.to_host(s)
    r1 = R.hwpss_ref(chi, h_pix, nd, edges, H, dirty)
    r0 = R.hwpss_ref(chi, h_pix, nd, edges, H, base)
    ok = h_pix >= 0
    hits = np.bincount(h_pix[ok], minlength=n)
    cF = R._ld(R.c_samples(nd, edges, H))
    e = U53 * (cF * (r1.S + r0.S) + LD(int(hits.max()) + 10) * (np.abs(R._ld(f_dirty)) + np.abs(R._ld(f_base))))
    pt = np.zeros((n, 3), dtype=LD)
    for k, w in enumerate((np.ones(nd * ns), np.abs(h_c), np.abs(h_s))):
        np.add.at(pt[:, k], h_pix[ok], (e * R._ld(w))[ok])
    cols = []
    for k in range(3):                                  # |M_BD|: its blocks, column by column
        u = np.zeros((n, 3))
        u[:, k] = 1.0
        cols.append(np.abs(np.asarray(Mbd * u.reshape(-1))).reshape(n, 3))
    bound = sum(R._ld(cols[k]) * pt[:, [k]] for k in range(3)).reshape(-1)
    diff = np.abs(R._ld(map_dirty) - R._ld(map_base))
    raw = np.abs(map_raw - map_base)
    print("filtered maps differ by %.3g at most (%.3g of the bound); the unfiltered map is off by %.3g"
          % (float(diff.max()), float((diff / bound).max()), float(raw.max())))
    assert (bound > 0).all() and (diff <= bound).all()
