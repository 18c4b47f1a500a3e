"""
The template filter on the GPU (cm2_template_*, TemplateFilterLO) against tests/_template_ref.py.

The outputs, the coefficients, the marks and the centred table are compared BIT FOR BIT with the float64 restatement,
which runs from the handle's own table; the restatement itself is held to c 2^-53 S of the extended-precision
reference on the CPU (tests/test_template_cpu.py), with c from _template_ref.py (operation count x the CPU-measured
headroom), never measured here.  The end-to-end tests use that bound.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _template_ref as R  # noqa: E402
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


def same_bits(a, b):
    return np.array_equal(R.bits(np.asarray(a)), R.bits(np.asarray(b)))


def build(cm, cs):
    return cm.I.TemplateFilterLO(cs.tab, cs.pix, ndet=cs.ndet, chunks=cs.edges, add_constant=cs.cst)


_made = {}


def made(cm, K, cst, variant="clean"):
    """the operator of a shared case and the CPU evaluation run from ITS table, once per process"""
    key = (K, cst, variant)
    if key not in _made:
        cs = R.case(K, cst, variant)
        F = build(cm, cs)
        tab = cm.D.to_host(F.template_tables()).copy()
        _made[key] = SimpleNamespace(F=F, tab=tab, ev=R.evaluate(cs, tab))
    return _made[key]


def unit_slices(cs):
    for k in range(cs.ndet):
        for c in range(len(cs.lens)):
            yield k, c, slice(k * cs.ns + int(cs.edges[c]), k * cs.ns + int(cs.edges[c + 1]))


def check_table(cs, tab):
    """the handle's table: the restatement's centring to the bit (the caller's values without the constant)"""
    assert tab.shape == (cs.J, cs.ns)
    want = R.centre_f64(cs.tab, cs.edges)[0] if cs.cst and cs.J else np.asarray(cs.tab, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(tab), fin)
    assert same_bits(tab[fin], want[fin])
    assert np.array_equal(np.isnan(tab), np.isnan(want))


def run_abi(cm, cs, F, what):
    """apply and fit through the C ABI on guarded buffers -> (out, coeff); the input must come back unchanged"""
    C = len(cs.lens)
    d_in = Guarded(cm, cs.nt, cs.v)
    d_out, d_cf = Guarded(cm, cs.nt), Guarded(cm, cs.ndet * C * cs.K)
    st = cm.D.stream()
    cm.hip.call("cm2_template_apply", F._handle.h, d_in.ptr, d_out.ptr, st)
    cm.hip.call("cm2_template_fit", F._handle.h, d_in.ptr, d_cf.ptr, st)
    out, cf = d_out.get(), d_cf.get().reshape(cs.ndet, C, cs.K)
    for g in (d_in, d_out, d_cf):
        g.intact(what)
    assert same_bits(d_in.get(), cs.v), what
    return out, cf


def check_against(cs, F, ev, out, cf, what):
    """apply, fit, status and info against the restatement (bit for bit) and the reference's classes"""
    C = len(cs.lens)
    ref, f64 = ev.ref, ev.f64
    info = F.filter_info()
    want = dict(ns=cs.ns, ndet=cs.ndet, nchunks=C, K=cs.K, add_constant=int(cs.cst),
                fitted=int((ref.marks == R.FITTED).sum()), skipped_few=int((ref.marks == R.FEW).sum()),
                skipped_pivot=int((ref.marks == R.PIVOT).sum()), segment=R.SEG,
                segments=cs.ndet * int(R.segments_of(cs.edges).sum()))
    assert info == want, what
    status = F.status()
    assert status.dtype == np.uint8 and status.shape == (cs.ndet, C)
    assert np.array_equal(status, ref.marks) and np.array_equal(f64.marks, ref.marks), what
    same_o = float((R.bits(out) == R.bits(f64.out)).mean())
    same_c = float((R.bits(cf) == R.bits(f64.coeff)).mean())
    print("%s: %.6f of the outputs and %.6f of the coefficients bit-equal to the restatement" % (what, same_o, same_c))
    R.assert_bit_equal(out, f64.out, what + ": apply")
    R.assert_bit_equal(cf, f64.coeff, what + ": fit")
    assert not out[cs.pix < 0].any()
    for k, c, sl in unit_slices(cs):
        if ref.marks[k, c]:
            assert not out[sl].any() and not cf[k, c].any(), (what, k, c)
    # and so within the bound of the extended reference, as the CPU test holds the restatement to it
    R.assert_accepted(out, f64.out, ref.out, ref.S, R.c_samples(cs.ndet, cs.edges, cs.K), what)
    R.assert_accepted(cf, f64.coeff, ref.coeff, ref.Sc, R.c_coeffs(cs.ndet, cs.edges, cs.K), what)


# ---------------------------------------------------- 1: bit for bit, shared cases ----
@pytest.mark.parametrize("K,cst", R.MODES)
def test_apply_fit_status_and_tables_on_the_shared_cases(cm, K, cst):
    cs = R.case(K, cst)
    m = made(cm, K, cst)
    check_table(cs, m.tab)
    if cs.cst and cs.J:                                  # the means themselves, against the long-double ones
        mu = R.centre_f64(cs.tab, cs.edges)[1]
        mu_ref, S = R.centre_ref(cs.tab, cs.edges)
        c = np.array([R.c_centre(n) for n in cs.lens])[None, :]
        assert (np.abs(R._ld(mu) - mu_ref) <= R._ld(c) * U53 * S).all()
    out, cf = run_abi(cm, cs, m.F, "case %r" % ((K, cst),))
    check_against(cs, m.F, m.ev, out, cf, "K=%d constant=%s" % (K, cst))
    info = m.F.filter_info()
    assert info["skipped_few"] >= 2 and info["fitted"] >= 0.8 * cs.ndet * len(cs.lens)
    assert info["skipped_pivot"] >= 3 or (K, cst) == (1, True)
    # the operator's own methods: the same bits, and the same bits again
    y = m.F * cs.v
    assert isinstance(y, np.ndarray) and same_bits(y, out) and same_bits(m.F.mult(cs.v), out)
    assert same_bits(m.F.coefficients(cs.v), cf) and m.F.coefficients(cs.v).shape == (cs.ndet, len(cs.lens), K)
    assert m.F.shape == (cs.nt, cs.nt) and m.F.symmetric


@pytest.mark.parametrize("K,cst", R.MODES)
def test_detector_counts_around_the_tile(cm, K, cst):
    """1, Dt - 1, Dt and 2 Dt + 1 detectors: a lone detector, a short tile, whole tiles, whole tiles and one more"""
    for ndet in R.sweep_ndets(K):
        cs = R.sweep_case(K, cst, ndet)
        F = build(cm, cs)
        tab = cm.D.to_host(F.template_tables()).copy()
        check_table(cs, tab)
        out, cf = run_abi(cm, cs, F, "sweep %r" % ((K, cst, ndet),))
        check_against(cs, F, R.evaluate(cs, tab), out, cf, "K=%d constant=%s ndet=%d" % (K, cst, ndet))


@pytest.mark.parametrize("K,cst", [(3, True), (16, True), (3, False)])
def test_a_non_finite_template_value(cm, K, cst):
    clean = made(cm, K, cst)
    cs0 = R.case(K, cst)
    y0, c0 = clean.F * cs0.v, clean.F.coefficients(cs0.v)
    ok = (cs0.pix >= 0).reshape(cs0.ndet, cs0.ns)
    for variant in ("valid", "flagged"):
        cs, m = R.case(K, cst, variant), made(cm, K, cst, variant)
        check_table(cs, m.tab)
        out, cf = run_abi(cm, cs, m.F, "%s %r" % (variant, (K, cst)))
        check_against(cs, m.F, m.ev, out, cf, "K=%d constant=%s %s" % (K, cst, variant))
        bad = np.flatnonzero(~np.isfinite(cs.tab).all(axis=0))
        status = m.F.status()
        assert np.isfinite(out).all() and np.isfinite(cf).all()
        if variant == "valid":                            # its unit is skipped as a pivot failure, the others as before
            for k, c, sl in unit_slices(cs):
                if c != cs.poisoned:
                    assert same_bits(out[sl], y0[sl]) and same_bits(cf[k, c], c0[k, c]), (k, c)
                    assert status[k, c] == clean.ev.ref.marks[k, c]
                elif clean.ev.ref.marks[k, c] == R.FITTED and ok[k, bad].any():
                    assert status[k, c] == R.PIVOT and not out[sl].any() and not cf[k, c].any()
            assert status[0, cs.poisoned] == R.PIVOT
        else:                                             # under flags only: no unit changes its class
            assert not ok[:, bad].any() and np.array_equal(status, clean.ev.ref.marks)
            a, b = int(cs.edges[cs.poisoned]), int(cs.edges[cs.poisoned + 1])
            inside = np.tile((np.arange(cs.ns) >= a) & (np.arange(cs.ns) < b), cs.ndet)
            assert same_bits(out[~inside], y0[~inside])
            if not cst:                                   # no mean is taken: to the bit everywhere
                assert same_bits(out, y0) and same_bits(cf, c0)
            else:                                         # the means of that chunk lost two values: the constant absorbs it
                R.assert_accepted(out, y0, clean.ev.ref.out, clean.ev.ref.S, R.c_samples(cs.ndet, cs.edges, K), variant)


# ------------------------------------------------------------------- 2: a NaN ----
def test_a_nan_in_the_data_stays_in_its_unit(cm):
    K, cst = 9, True
    cs = R.case(K, cst)
    F = made(cm, K, cst).F
    clean = F * cs.v
    c_hit = cs.lens.index(R.SEG + 1)
    ok = cs.pix >= 0
    for what in ("valid", "flagged"):
        v = cs.v.copy()
        cand = np.flatnonzero(ok if what == "valid" else ~ok)
        lo, hi = cs.ns + int(cs.edges[c_hit]), cs.ns + int(cs.edges[c_hit + 1])     # detector 1: 10 % flags
        at = cand[(cand >= lo) & (cand < hi)][-1]
        v[at] = np.nan
        got = F * v
        for k, c, sl in unit_slices(cs):
            if (k, c) == (1, c_hit) and what == "valid":
                assert np.isnan(got[sl][ok[sl]]).all() and not got[sl][~ok[sl]].any()
            else:
                assert same_bits(got[sl], clean[sl]), (what, k, c)


# ------------------------------------------------- 3: device and host inputs ----
def test_device_tensors_and_host_arrays_give_the_same_bits(cm):
    K, cst = 16, True
    cs = R.case(K, cst)
    m = made(cm, K, cst)
    pix_t, tab_t, v_t = cm.D.i32(cs.pix), cm.D.f64(cs.tab), cm.D.f64(cs.v)
    before = cm.D.to_host(tab_t).copy()
    Fd = cm.I.TemplateFilterLO(tab_t, pix_t, ndet=cs.ndet, chunks=cs.edges)
    assert Fd._d_pix.data_ptr() == pix_t.data_ptr()                     # adopted, not copied
    assert same_bits(cm.D.to_host(tab_t), before)                       # the caller's table is copied, not centred
    tab_t.fill_(float("nan"))                                           # ... and may go away
    y = Fd * v_t
    assert cm.D.is_dev(y) and same_bits(cm.D.to_host(y), m.F * cs.v)
    assert same_bits(cm.D.to_host(Fd * v_t), cm.D.to_host(y))           # twice: the same bits
    cf = Fd.coefficients(v_t)
    assert cm.D.is_dev(cf) and same_bits(cm.D.to_host(cf), m.F.coefficients(cs.v))
    assert Fd.filter_info() == m.F.filter_info() and np.array_equal(Fd.status(), m.F.status())
    assert same_bits(np.nan_to_num(cm.D.to_host(Fd.template_tables())), np.nan_to_num(m.tab))
    # one template as a 1-D array, an int chunk length and None plan as hwpss_plan says
    F1 = cm.I.TemplateFilterLO(cs.tab[0, :5000], cs.pix[:5000], chunks=2048)
    i1 = F1.filter_info()
    assert (i1["nchunks"], i1["segments"], i1["K"], i1["add_constant"]) == (3, 3, 2, 1)
    assert F1.template_tables().shape == (1, 5000)
    F2 = cm.I.TemplateFilterLO(cs.tab[:2, :5000], cs.pix[:5000], add_constant=False)
    i2 = F2.filter_info()
    assert (i2["nchunks"], i2["segments"], i2["K"], i2["add_constant"]) == (1, 2, 2, 0)
    F3 = cm.I.TemplateFilterLO(np.zeros((0, 5000)), cs.pix[:5000])      # the constant alone
    assert F3.filter_info()["K"] == 1 and F3.template_tables().shape == (0, 5000)


# ------------------------------------------------------------- 4: error codes ----
def test_refused_calls_leave_their_outputs_untouched(cm):
    K, cst = 3, True
    cs = R.case(K, cst)
    m = made(cm, K, cst)
    F = m.F
    lib, st, h = cm.hip.load(), cm.D.stream(), F._handle.h
    C = len(cs.lens)
    d_in, d_out, d_cf = Guarded(cm, cs.nt, cs.v), Guarded(cm, cs.nt), Guarded(cm, cs.ndet * C * K)
    d_tab, d_st = Guarded(cm, cs.J * cs.ns), Guarded(cm, cs.ndet * C)     # (the marks: bytes inside doubles)

    def untouched(what):
        for g in (d_out, d_cf, d_tab, d_st):
            g.intact(what)
            assert np.isnan(g.get()).all(), what + ": an output was written"
        assert same_bits(d_in.get(), cs.v), what

    refused = [
        ("cm2_template_apply", (None, d_in.ptr, d_out.ptr, st)),
        ("cm2_template_apply", (h, None, d_out.ptr, st)),
        ("cm2_template_apply", (h, d_in.ptr, None, st)),
        ("cm2_template_apply", (h, d_in.ptr, d_in.ptr, st)),                       # aliased
        ("cm2_template_apply", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),     # overlapping by one element
        ("cm2_template_fit", (None, d_in.ptr, d_cf.ptr, st)),
        ("cm2_template_fit", (h, None, d_cf.ptr, st)),
        ("cm2_template_fit", (h, d_in.ptr, None, st)),
        ("cm2_template_fit", (h, d_in.ptr, d_in.ptr + 8, st)),
        ("cm2_template_tables", (None, d_tab.ptr, st)),
        ("cm2_template_tables", (h, None, st)),
        ("cm2_template_status", (None, d_st.ptr, st)),
        ("cm2_template_status", (h, None, st)),
    ]
    for name, args in refused:
        assert getattr(lib, name)(*args) == cm.hip.ERR_ARGUMENT, (name, args)
        assert lib.cm2_last_error()
        untouched("%s%r" % (name, args))
    assert lib.cm2_template_info(None, (ctypes.c_int64 * 10)()) == cm.hip.ERR_ARGUMENT
    assert lib.cm2_template_info(h, None) == cm.hip.ERR_ARGUMENT
    # create: the handle variable keeps its value
    tab_t, pix_t = cm.D.f64(cs.tab), cm.D.i32(cs.pix)
    MARK = 0x1234
    I64 = ctypes.c_int64

    def create(ns=cs.ns, ndet=cs.ndet, edges=cs.edges, J=cs.J, tab=tab_t, add=1, pix=pix_t, out=True):
        e = None if edges is None else (I64 * len(edges))(*[int(x) for x in edges])
        nch = 0 if edges is None else len(edges) - 1
        hv = ctypes.c_void_p(MARK)
        rc = lib.cm2_template_create(ctypes.byref(hv) if out else None, ns, ndet, nch, e, J, cm.D.ptr(tab), add,
                                     cm.D.ptr(pix), st)
        return rc, hv

    for kw in (dict(J=-1), dict(J=-1, add=2), dict(add=2), dict(add=-1), dict(J=0, add=0), dict(J=16), dict(J=17, add=0),
               dict(ns=0, edges=[0, 0]), dict(ndet=0), dict(edges=[0, cs.ns - 1]), dict(edges=[1, cs.ns]),
               dict(edges=[0, 100, 100, cs.ns]), dict(edges=[0, 200, 100, cs.ns]), dict(edges=None), dict(tab=None),
               dict(pix=None), dict(ns=1 << 40, edges=[0, 1 << 40]),
               dict(ns=1 << 30, ndet=(1 << 16) + 1, edges=[0, 1 << 30]), dict(ns=1 << 20, ndet=1 << 23, edges=[0, 1 << 20])):
        rc, hv = create(**kw)
        assert rc == cm.hip.ERR_ARGUMENT and hv.value == MARK, kw
        assert lib.cm2_last_error()
    assert create(out=False)[0] == cm.hip.ERR_ARGUMENT
    untouched("after the refused creates")
    rc, hv = create()
    assert rc == 0 and hv.value not in (None, MARK)
    assert lib.cm2_template_apply(hv, d_in.ptr, d_out.ptr, st) == 0
    assert lib.cm2_template_tables(hv, d_tab.ptr, st) == 0
    assert lib.cm2_template_status(hv, d_st.ptr, st) == 0
    assert same_bits(d_out.get(), F * cs.v) and same_bits(d_tab.get().reshape(cs.J, cs.ns), m.tab)
    marks = d_st.get().view(np.uint8)
    assert np.array_equal(marks[:cs.ndet * C].reshape(cs.ndet, C), F.status())
    assert same_bits(d_st.get()[-(-cs.ndet * C // 8):], np.full(cs.ndet * C - -(-cs.ndet * C // 8), np.nan))
    for g in (d_out, d_tab, d_st):
        g.intact("valid calls")
    rc0, h0 = create(J=0, tab=None)                                     # the constant alone needs no table
    assert rc0 == 0 and lib.cm2_template_tables(h0, None, st) == 0 and lib.cm2_template_destroy(h0) == 0
    assert lib.cm2_template_destroy(hv) == 0 and lib.cm2_template_destroy(None) == 0
    with pytest.raises(cm.L.lp.ShapeError):
        F * cs.v[:-1]


# --------------------------------------------------------- 5: the tiled chain ----
def test_filter_between_tile_order_P_and_Pt(cm):
    rng = np.random.default_rng(31)
    ndet, ns, npix, pol = 3, 5001, 300, 3
    nt = ndet * ns
    p = rng.integers(0, npix, nt).astype(np.int32)
    p[rng.random(nt) < 0.1] = -1
    phi = rng.uniform(0, np.pi, nt)
    tab = np.vstack([0.1 + 1e-5 * np.arange(ns), rng.standard_normal(ns)])
    ang = type("Ang", (), {"cos": np.cos(2 * phi), "sin": np.sin(2 * phi)})()
    P = cm.I.SparseLO(npix, nt, p, pol=pol, angle_processed=ang)
    Ft = cm.I.TemplateFilterLO(tab, p, ndet=ndet, chunks=2048)
    assert Ft._tile_compatible(P) and not hasattr(Ft, "_apply_tiles")
    other = p.copy()
    other[np.flatnonzero(other >= 0)[0]] = -1
    Fo = cm.I.TemplateFilterLO(tab, other, ndet=ndet, chunks=2048)
    assert not Fo._tile_compatible(P)
    x = rng.standard_normal(pol * npix)
    exact = P.T * (Ft * (P * x))
    exact_o = P.T * (Fo * (P * x))
    D, st = cm.D, cm.D.stream()
    cm.L.set_pointing_mode("tiled")
    try:
        A = P.T * Ft * P
        assert any(isinstance(op, cm.L._TiledNormalLO) for op in A._compiled())
        y1, y2 = np.asarray(A * x), np.asarray(A * x)
        # the same stages by hand: tile-order P, to the time order, the filter, back, tile-order P^T
        T = cm.L._sparse_tiles(P)
        d_tb, tod, out = D.empty(max(T.nvalid, 1)), D.empty(nt), D.empty(pol * npix)
        cm.hip.call("cm2_P_tiles_apply", T.h, D.ptr(D.f64(x)), D.ptr(d_tb), st)
        cm.hip.call("cm2_tod_tiles_to_time", T.h, D.ptr(d_tb), D.ptr(tod), st)
        tod2 = Ft.mult(tod)
        cm.hip.call("cm2_tod_time_to_tiles", T.h, D.ptr(tod2), D.ptr(d_tb), st)
        cm.hip.call("cm2_Pt_tiles_apply", T.h, D.ptr(d_tb), D.ptr(out), st)
        by_hand = D.to_host(out)
        Ao = P.T * Fo * P                                 # other flags: not on the tile order
        assert not any(isinstance(op, cm.L._TiledNormalLO) for op in Ao._compiled())
        yo = np.asarray(Ao * x)
    finally:
        cm.L.set_pointing_mode("auto")
    assert same_bits(y1, y2) and same_bits(y1, by_hand)
    # what the existing tile tests allow for the tile-order P^T against the exact order (test_gpu_round2.py)
    assert np.linalg.norm(y1 - exact) <= 1e-12 * np.linalg.norm(exact)
    assert np.linalg.norm(yo - exact_o) <= 1e-12 * np.linalg.norm(exact_o)


# ------------------------------------------------------------- 6: an el nod ----
def test_elevation_nod_gives_the_relative_gains(cm):
    """d_k = g_k a(t) + o_k, a = 1 / sin(el) over a nod, which is g_k T_1(t) + (o_k + g_k mu) with the handle's
    centred T_1 = fl(a - mu).  The samples are the float64 roundings of that line (two roundings, 2 x 2^-53 (|g_k a| +
    |o_k|) at most) and T_1 carries the rounding of the centring (2^-53 |g_k T_1|): together at most 3 x 2^-53 S_t,
    which the fit carries into the coefficients with |G^-1| sum |T| |.|, that is 3 x 2^-53 Sc.  Hence c + 3 where the
    ref module gives c."""
    rng = np.random.default_rng(88)
    ndet, ns = 8, 6000
    t = np.arange(ns) / ns
    el = np.radians(50.0 + 5.0 * np.sin(2 * np.pi * 3 * t))
    a = 1.0 / np.sin(el)
    g, o = rng.uniform(0.5, 1.5, ndet) * 1.0e3, rng.uniform(-1.0, 1.0, ndet) * 1.0e2
    pix = rng.integers(0, 500, ndet * ns).astype(np.int32)
    pix[rng.random(ndet * ns) < 0.1] = -1
    d = (g[:, None] * a[None, :] + o[:, None]).reshape(-1)
    edges = R.plan(ns, None)
    F = cm.I.TemplateFilterLO(a, pix, ndet=ndet)
    assert F.filter_info()["fitted"] == ndet
    cf = F.coefficients(d)
    out = F * d
    T = R.design(cm.D.to_host(F.template_tables()), True)
    ref = R.template_ref(T, pix, ndet, edges, d)
    c = R.c_bound(int(R.segments_of(edges)[0]), 2) + 3
    got = cf[:, 0, 1]
    e_g = R.excess(got, g, ref.Sc[:, 0, 1], c)
    e_o = R.excess(out, np.zeros(ndet * ns), ref.S, c)
    print("gains: %.3g of the bound (relative error %.3g at most); residual: %.3g of the bound, %.3g at most"
          % (e_g, float(np.abs(got / g - 1).max()), e_o, float(np.abs(out).max())))
    assert e_g <= 1.0 and e_o <= 1.0
    # c_0 is the offset at the chunk mean of the air mass, o_k + g_k mu with the mean the handle subtracted
    mu = LD(R.centre_f64(a, edges)[1][0, 0])
    assert R.excess(cf[:, 0, 0], R._ld(o) + R._ld(g) * mu, ref.Sc[:, 0, 0], c) <= 1.0


# ------------------------------------------------------------- 7: end to end ----
def test_a_drift_does_not_reach_the_map(cm):
    """expand_pointing -> P; d = P m0 + g_k theta(t) with a smooth theta a thousand times the sky, fitted as given
    (no constant: P^T F P keeps the mean of the map).  x = cg(P^T F P, P^T F d).  With e = x - m0:
    A e = (A x - b) + (b - A m0), the solver's residual plus what rounding leaves of the drift in b = P^T F d, and
    rho |e|^2 = e^T A e <= |e| |A e| with rho the Rayleigh quotient of e itself, so |e| <= (|A x - b| + |b - A m0|) / rho.
    The residual is checked to be below 1e-8 |b| (the solve stops at rtol = 1e-10), and what is left of the drift to
    be below 1e-12 of what P^T makes of the drift itself.  Without the filter the drift goes into the map."""
    nside, nd = 16, 12
    npix, ns = 12 * nside * nside, PE.NS
    b, dq = PE.inputs("scan")
    rng = np.random.default_rng(81)
    pixs, c, s = cm.U.expand_pointing(b, dq[:nd], nside)
    drop = cm.torch.from_numpy(rng.random(nd * ns) < 0.05).to(pixs.device)
    pixs[drop] = -1
    ces = cm.U.ProcessTimeSamples(pixs, npix, pol=3, cos_sin=(c, s))
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nd * ns, pixs, pol=3, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=3)
    t = np.arange(ns) / ns
    theta = 1.0 + 0.5 * np.sin(2 * np.pi * 1.3 * t) + t * t
    edges = cm.I.hwpss_plan(ns, [0, 2048, ns])
    F = cm.I.TemplateFilterLO(theta, pixs, ndet=nd, chunks=edges, add_constant=False)
    assert F.filter_info()["fitted"] == nd * (len(edges) - 1)
    m0 = rng.standard_normal(3 * n)
    drift = (1.0e3 * rng.uniform(0.5, 1.5, nd)[:, None] * theta[None, :]).reshape(-1)
    d = np.asarray(P * m0) + drift
    A = P.T * F * P
    rhs = np.asarray(P.T * (F * d))
    x, i1 = cm.cg(A, rhs, M=Mbd, rtol=1e-10, maxiter=2000)
    x_raw, i2 = cm.cg(P.T * P, np.asarray(P.T * d), M=Mbd, rtol=1e-10, maxiter=2000)
    assert i1 == 0 and i2 == 0
    x = np.asarray(x)
    res = float(np.linalg.norm(rhs - np.asarray(A * x)))
    assert res <= 1e-8 * np.linalg.norm(rhs)
    e = x - m0
    rho = float(e @ np.asarray(A * e) / (e @ e))
    left = float(np.linalg.norm(rhs - np.asarray(A * m0)))
    assert left <= 1e-12 * np.linalg.norm(np.asarray(P.T * drift))
    bound = (res + left) / rho * (1.0 + 1e-3)
    off, off_raw = float(np.linalg.norm(e)), float(np.linalg.norm(np.asarray(x_raw) - m0))
    print("map off by %.3g (bound %.3g; residual %.3g, drift left %.3g, Rayleigh quotient %.3g); unfiltered by %.3g; "
          "|m0| = %.3g" % (off, bound, res, left, rho, off_raw, float(np.linalg.norm(m0))))
    assert off <= bound
    assert off_raw >= 100.0 * bound                                      # orders of magnitude without the filter


# ---------------------------------------------- the template filter is the HWPSS filter ----
def hwpss_as_templates(cm, H, seed=11):
    """HWPSSFilterLO of nharm = H on a small stream, and what TemplateFilterLO needs to be the same filter: the rows
    [ones, T_1, ..., T_2H] formed on the host from the handle's own (cos chi, sin chi), every product rounded on its
    own as on the device.  Three detectors (one ragged tile), chunks of K - 1 (too few samples), 300 and kSeg + 1
    (two segments) samples, a tenth of the samples flagged."""
    import _hwpss_ref as RH
    K = 2 * H + 1
    edges = np.cumsum([0, K - 1, 300, R.SEG + 1]).astype(np.int64)
    ns, ndet = int(edges[-1]), 3
    rng = np.random.default_rng(seed + H)
    chi = 0.37 * np.arange(ns) + 0.01 * rng.standard_normal(ns)
    pix = np.where(rng.random(ndet * ns) < 0.1, -1, 5).astype(np.int32)
    v = rng.standard_normal(ndet * ns) + np.tile(3.0 * np.cos(2 * chi + 0.3), ndet)
    Fh = cm.I.HWPSSFilterLO(chi, pix, ndet=ndet, nharm=H, chunks=edges)
    c1, s1 = (cm.D.to_host(t) for t in Fh.harmonic_tables())
    rows = np.ascontiguousarray(RH.templates_f64(c1, s1, H).T)           # [K, ns], row 0 = ones
    assert np.all(rows[0] == 1.0)
    return SimpleNamespace(Fh=Fh, rows=rows, pix=pix, v=v, ndet=ndet, edges=edges, K=K)


def compare_with_hwpss(cm, H):
    s = hwpss_as_templates(cm, H)
    Ft = cm.I.TemplateFilterLO(s.rows, s.pix, ndet=s.ndet, chunks=s.edges, add_constant=False)
    out_h, out_t = np.asarray(s.Fh * s.v), np.asarray(Ft * s.v)
    cf_h, cf_t = np.asarray(s.Fh.coefficients(s.v)), np.asarray(Ft.coefficients(s.v))
    ih, it = s.Fh.filter_info(), Ft.filter_info()
    marks = Ft.status()
    assert same_bits(out_h, out_t) and same_bits(cf_h, cf_t)
    for key in ("fitted", "skipped_few", "skipped_pivot", "segment", "segments"):
        assert ih[key] == it[key], key
    # HWPSS has no status call: its marks show in the tally and in which units have coefficients
    assert (marks[:, 0] == R.FEW).all() and ih["skipped_few"] == s.ndet and ih["fitted"] == 2 * s.ndet
    assert np.array_equal(marks == R.FITTED, cf_h.any(axis=2)) and np.array_equal(marks == R.FITTED, cf_t.any(axis=2))
    assert out_h.any() and np.isfinite(out_h).all()
    return out_h, cf_h, marks


@pytest.mark.parametrize("H", (1, 4, 8))
def test_given_the_harmonic_tables_it_is_the_hwpss_filter(cm, H):
    """Both filters sum in the order cm2_chunkfit.h states and c_0 * 1.0 is exact: the outputs, the coefficients and
    the marks are the same bits.  K = 17 of H = 8 is more than the template filter takes: that is refused, and
    H = 7 (K = 15) is compared instead."""
    if 2 * H + 1 > cm.L.TEMPLATE_MAX_K:
        s = hwpss_as_templates(cm, H)
        with pytest.raises(ValueError) as e:
            cm.I.TemplateFilterLO(s.rows, s.pix, ndet=s.ndet, chunks=s.edges, add_constant=False)
        assert "K = 17" in str(e.value)
        H = 7
    compare_with_hwpss(cm, H)
