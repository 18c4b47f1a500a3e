"""
The common-mode filter on the GPU (cm2_cmode_*, CommonModeFilterLO) against tests/_cmode_ref.py.

Acceptance, element by element: bit-equal to the float64 restatement, or within c 2^-53 S of the extended-precision
reference; exactly 0 where S = 0 (flagged samples, skipped units).  c comes from _cmode_ref.py (operation count x the
CPU-measured headroom) and is never measured here.  The class of every unit must be the reference's.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cmode_ref as R  # noqa: E402
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


def made(cm, name, pattern):
    """the operator of a shared case under a flag pattern, once per process"""
    key = (name, pattern)
    if key not in _made:
        cs, d = R.case(name), R.data(name, pattern)
        _made[key] = cm.I.CommonModeFilterLO(d.pix, cs.ndet, modes=cs.modes, groups=cs.edges)
    return _made[key]


def same_bits(a, b):
    return np.array_equal(R.bits(np.asarray(a)), R.bits(np.asarray(b)))


class GuardedBytes(object):
    """n bytes in the middle of a buffer of 0xAB, themselves 0xCD before the call"""

    def __init__(self, cm, n):
        self.cm, self.n = cm, int(n)
        self.buf = cm.torch.full((64 + self.n + 64,), 0xAB, dtype=cm.torch.uint8, device=cm.D.dev())
        self.buf[64:64 + self.n] = 0xCD
        self.ptr = self.buf.data_ptr() + 64

    def get(self):
        self.cm.torch.cuda.synchronize()
        return self.buf[64:64 + self.n].cpu().numpy().copy()

    def intact(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:64] == 0xAB).all() and (b[64 + self.n:] == 0xAB).all(), "%s: wrote outside its bytes" % what


# ------------------------------------------- 1: apply, fit and status, every case ----
@pytest.mark.parametrize("name", R.CASES)
def test_apply_fit_and_status_on_the_shared_cases(cm, name):
    cs = R.case(name)
    G, K = len(cs.sizes), cs.K
    st = cm.D.stream()
    for pattern in R.BOUNDED:
        d, ref, f64 = R.data(name, pattern), R.case_ref(name, pattern), R.case_f64(name, pattern)
        F = made(cm, name, pattern)
        d_in = Guarded(cm, cs.nt, d.v)
        d_out, d_cf, d_st = Guarded(cm, cs.nt), Guarded(cm, G * K * cs.ns), GuardedBytes(cm, G * cs.ns)
        cm.hip.call("cm2_cmode_apply", F._handle.h, d_in.ptr, d_out.ptr, st)
        cm.hip.call("cm2_cmode_fit", F._handle.h, d_in.ptr, d_cf.ptr, st)
        cm.hip.call("cm2_cmode_status", F._handle.h, d_st.ptr)
        out, cf, status = d_out.get(), d_cf.get().reshape(G, K, cs.ns), d_st.get().reshape(G, cs.ns)
        for g in (d_in, d_out, d_cf, d_st):
            g.intact("case %r" % ((name, pattern),))
        assert same_bits(d_in.get(), d.v)
        # the classes and their counts
        assert np.array_equal(status, ref.status) and np.array_equal(f64.status, ref.status)
        count = np.bincount(ref.status.reshape(-1), minlength=4)
        want = dict(ns=cs.ns, ndet=cs.ndet, ngroups=G, K=K, fitted=int(count[0]), empty=int(count[1]),
                    few=int(count[2]), pivot=int(count[3]))
        assert F.filter_info() == want
        # the zeros
        skipped = np.repeat(ref.status != R.FITTED, cs.sizes, axis=0).reshape(-1)
        assert not out[(d.pix < 0) | skipped].any()
        assert not cf[np.broadcast_to((ref.status != R.FITTED)[:, None, :], cf.shape)].any()
        # element by element
        same_o = float((R.bits(out) == R.bits(f64.out)).mean())
        same_c = float((R.bits(cf) == R.bits(f64.coeff)).mean())
        eo = R.assert_accepted(out, f64.out, ref.out, ref.S, R.c_samples(cs.ndet, cs.ns, cs.edges, K), "apply")
        ec = R.assert_accepted(cf, f64.coeff, ref.coeff, ref.Sc, R.c_coeffs(cs.ns, cs.edges, K), "fit")
        print("%s %s: %.4f of the outputs and %.4f of the coefficients bit-equal to the restatement; the others use "
              "%.3g / %.3g of the bound" % (name, pattern, same_o, same_c, eo, ec))
        # the operator's own methods: the same bits
        y = F * d.v
        assert isinstance(y, np.ndarray) and same_bits(y, out) and same_bits(F.mult(d.v), out)
        got_cf = F.coefficients(d.v)
        assert got_cf.shape == (G, K, cs.ns) and same_bits(got_cf, cf)
        got_st = F.status()
        assert got_st.shape == (G, cs.ns) and got_st.dtype == np.uint8 and np.array_equal(got_st, status)
        assert F.shape == (cs.nt, cs.nt) and F.symmetric


# ------------------------------------------------ 2: in place, and twice the same ----
@pytest.mark.parametrize("name", ["gains7", "order3_16", "groups20"])
def test_in_place_and_repeated_applications_give_the_same_bits(cm, name):
    cs, d = R.case(name), R.data(name, "random")
    F = made(cm, name, "random")
    st, h = cm.D.stream(), F._handle.h
    d_in, d_a, d_b = Guarded(cm, cs.nt, d.v), Guarded(cm, cs.nt), Guarded(cm, cs.nt)
    cm.hip.call("cm2_cmode_apply", h, d_in.ptr, d_a.ptr, st)
    cm.hip.call("cm2_cmode_apply", h, d_in.ptr, d_b.ptr, st)
    assert same_bits(d_a.get(), d_b.get())
    cm.hip.call("cm2_cmode_apply", h, d_in.ptr, d_in.ptr, st)               # d_out == d_in exactly
    assert same_bits(d_in.get(), d_a.get())
    for g in (d_in, d_a, d_b):
        g.intact(name)
    d_c1, d_c2 = Guarded(cm, len(cs.sizes) * cs.K * cs.ns), Guarded(cm, len(cs.sizes) * cs.K * cs.ns)
    d_v = Guarded(cm, cs.nt, d.v)
    cm.hip.call("cm2_cmode_fit", h, d_v.ptr, d_c1.ptr, st)
    cm.hip.call("cm2_cmode_fit", h, d_v.ptr, d_c2.ptr, st)
    assert same_bits(d_c1.get(), d_c2.get())


# --------------------------- 3: a unit does not depend on ns, its place or other groups ----
def test_a_unit_keeps_its_bits_in_a_longer_stream_and_in_another_group(cm):
    name, pattern = "order2_12", "random"
    cs, d = R.case(name), R.data(name, pattern)
    F = made(cm, name, pattern)
    out, cf, status = F * d.v, F.coefficients(d.v), F.status()
    rng = np.random.default_rng(41)
    extra, ns2, at = 5, 1200, 301                     # five detectors in a group in front; columns 301 .. 301 + 773
    nd2 = extra + cs.ndet
    pix2 = rng.integers(0, 50, (nd2, ns2)).astype(np.int32)
    pix2[rng.random((nd2, ns2)) < 0.3] = -1
    v2 = rng.standard_normal((nd2, ns2)) * 30.0
    pix2[extra:, at:at + cs.ns] = d.pix.reshape(cs.ndet, cs.ns)
    v2[extra:, at:at + cs.ns] = d.v.reshape(cs.ndet, cs.ns)
    modes2 = np.concatenate([rng.standard_normal((extra, cs.K)), cs.modes])
    F2 = cm.I.CommonModeFilterLO(pix2.reshape(-1), nd2, modes=modes2, groups=[0, extra, nd2])
    out2 = (F2 * v2.reshape(-1)).reshape(nd2, ns2)
    assert same_bits(out2[extra:, at:at + cs.ns], out.reshape(cs.ndet, cs.ns))
    assert same_bits(F2.coefficients(v2.reshape(-1))[1, :, at:at + cs.ns], cf[0])
    assert np.array_equal(F2.status()[1, at:at + cs.ns], status[0])
    assert (F2.status()[0] != R.FITTED).all()         # five detectors cannot carry six templates
    assert not out2[:extra].any()


# ------------------------------------------------------------------- 4: a NaN ----
@pytest.mark.parametrize("name", ["order2_12", "groups20"])
def test_a_nan_stays_in_its_unit(cm, name):
    cs, d = R.case(name), R.data(name, "nan")
    g, s, k = d.nan_at
    F = made(cm, name, "nan")
    clean = (made(cm, name, "random") * R.data(name, "random").v).reshape(cs.ndet, cs.ns)
    got = (F * d.v).reshape(cs.ndet, cs.ns)
    mine = np.zeros((cs.ndet, cs.ns), dtype=bool)
    mine[cs.edges[g]:cs.edges[g + 1], s] = True
    assert np.isnan(got[mine & d.ok]).all() and not got[mine & ~d.ok].any()
    assert same_bits(got[~mine], clean[~mine])
    cf = F.coefficients(d.v)
    assert np.isnan(cf[g, :, s]).all() and np.isfinite(np.delete(cf, s, axis=2)).all()
    # a NaN on a flagged sample is never read
    v = R.data(name, "random").v.copy()
    v[np.flatnonzero(d.pix < 0)[::7]] = np.nan
    assert same_bits((F * v).reshape(cs.ndet, cs.ns), clean)


# ------------------------------------------------- 5: device and host inputs ----
def test_device_tensors_and_host_arrays_give_the_same_bits(cm):
    name, pattern = "groups20", "random"
    cs, d = R.case(name), R.data(name, pattern)
    F = made(cm, name, pattern)
    pix_t, v_t, modes_t = cm.D.i32(d.pix), cm.D.f64(d.v), cm.D.f64(cs.modes)
    Fd = cm.I.CommonModeFilterLO(pix_t, cs.ndet, modes=modes_t, groups=cs.edges)
    assert Fd._d_pix.data_ptr() == pix_t.data_ptr()                     # adopted, not copied
    modes_t.fill_(0.0)                                                  # the templates were copied
    y = Fd * v_t
    assert cm.D.is_dev(y) and same_bits(cm.D.to_host(y), F * d.v)
    cf = Fd.coefficients(v_t)
    assert cm.D.is_dev(cf) and tuple(cf.shape) == (4, 3, cs.ns) and same_bits(cm.D.to_host(cf), F.coefficients(d.v))
    assert Fd.filter_info() == F.filter_info() and np.array_equal(Fd.status(), F.status())
    # modes=None is the plain common mode; an int and None plan the groups as cmode_groups says
    ones = R.case("ones7")
    d1 = R.data("ones7", "random")
    assert same_bits(cm.I.CommonModeFilterLO(d1.pix, 7) * d1.v, made(cm, "ones7", "random") * d1.v)
    F3 = cm.I.CommonModeFilterLO(d1.pix, 7, groups=3)
    assert F3.filter_info()["ngroups"] == 3 and F3.edges.tolist() == [0, 3, 6, 7] and ones.K == F3.K == 1
    r3 = R.cmode_f64(d1.pix, 7, F3.edges, np.ones((7, 1)), d1.v)
    assert same_bits(F3 * d1.v, r3.out) and np.array_equal(F3.status(), r3.status)
    with pytest.raises(cm.L.lp.ShapeError):
        F * d.v[:-1]


# ------------------------------------------------------------- 6: error codes ----
def test_refused_calls_leave_their_outputs_untouched(cm):
    name, pattern = "order1_9", "random"
    cs, d = R.case(name), R.data(name, pattern)
    F = made(cm, name, pattern)
    lib, st, h = cm.hip.load(), cm.D.stream(), F._handle.h
    G, K = 1, cs.K
    d_in, d_out, d_cf = Guarded(cm, cs.nt, d.v), Guarded(cm, cs.nt), Guarded(cm, G * K * cs.ns)
    d_st = GuardedBytes(cm, G * cs.ns)

    def untouched(what):
        for g in (d_out, d_cf):
            g.intact(what)
            assert np.isnan(g.get()).all(), what + ": an output was written"
        d_st.intact(what)
        assert (d_st.get() == 0xCD).all(), what + ": the status was written"
        assert same_bits(d_in.get(), d.v), what

    refused = [
        ("cm2_cmode_apply", (None, d_in.ptr, d_out.ptr, st)),
        ("cm2_cmode_apply", (h, None, d_out.ptr, st)),
        ("cm2_cmode_apply", (h, d_in.ptr, None, st)),
        ("cm2_cmode_apply", (h, d_in.ptr, d_in.ptr + 8, st)),                   # overlapping, not the same
        ("cm2_cmode_apply", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),     # overlapping by one element
        ("cm2_cmode_apply", (h, d_in.ptr + 8 * (cs.nt - 1), d_in.ptr, st)),
        ("cm2_cmode_fit", (None, d_in.ptr, d_cf.ptr, st)),
        ("cm2_cmode_fit", (h, None, d_cf.ptr, st)),
        ("cm2_cmode_fit", (h, d_in.ptr, None, st)),
        ("cm2_cmode_fit", (h, d_in.ptr, d_in.ptr, st)),
        ("cm2_cmode_fit", (h, d_in.ptr, d_in.ptr + 8 * (cs.nt - 1), st)),
        ("cm2_cmode_status", (None, d_st.ptr)),
        ("cm2_cmode_status", (h, None)),
    ]
    for fn, args in refused:
        assert getattr(lib, fn)(*args) == cm.hip.ERR_ARGUMENT, (fn, args)
        assert lib.cm2_last_error()
        untouched("%s%r" % (fn, args))
    assert lib.cm2_cmode_info(None, (ctypes.c_int64 * 8)()) == cm.hip.ERR_ARGUMENT
    assert lib.cm2_cmode_info(h, None) == cm.hip.ERR_ARGUMENT
    # create: the handle variable keeps its value
    pix_t, modes_t = cm.D.i32(d.pix), cm.D.f64(cs.modes)
    MARK = 0x1234
    I64 = ctypes.c_int64

    def create(ns=cs.ns, ndet=cs.ndet, edges=cs.edges, K=K, modes=modes_t, pix=pix_t, out=True):
        e = None if edges is None else (I64 * len(edges))(*[int(x) for x in edges])
        ng = 0 if edges is None else len(edges) - 1
        hv = ctypes.c_void_p(MARK)
        rc = lib.cm2_cmode_create(ctypes.byref(hv) if out else None, ns, ndet, ng, e, K, cm.D.ptr(modes),
                                  cm.D.ptr(pix), st)
        return rc, hv

    for kw in (dict(K=0), dict(K=11), dict(K=-1), dict(ns=0), dict(ndet=0, edges=[0, 0]), dict(edges=[0]),
               dict(edges=[0, cs.ndet - 1]), dict(edges=[1, cs.ndet]), dict(edges=[0, 4, 4, cs.ndet]),
               dict(edges=[0, 6, 3, cs.ndet]), dict(edges=None), dict(modes=None), dict(pix=None),
               dict(ns=1 << 30, ndet=(1 << 16) + 1, edges=[0, (1 << 16) + 1]),              # ndet ns > 2^46
               dict(ns=((1 << 31) - 1) * 256 + 1, ndet=1, edges=[0, 1]),                    # 2^31 workgroups
               dict(ns=1 << 37, ndet=4, edges=[0, 1, 2, 3, 4])):                            # 4 x 2^29 workgroups
        rc, hv = create(**kw)
        assert rc == cm.hip.ERR_ARGUMENT and hv.value == MARK, kw
        assert lib.cm2_last_error()
    assert create(out=False)[0] == cm.hip.ERR_ARGUMENT
    untouched("after the refused creates")
    rc, hv = create()
    assert rc == 0 and hv.value not in (None, MARK)
    assert lib.cm2_cmode_apply(hv, d_in.ptr, d_out.ptr, st) == 0
    assert lib.cm2_cmode_status(hv, d_st.ptr) == 0
    assert same_bits(d_out.get(), F * d.v) and np.array_equal(d_st.get().reshape(1, -1), F.status())
    d_out.intact("valid calls")
    d_st.intact("valid calls")
    assert lib.cm2_cmode_destroy(hv) == 0 and lib.cm2_cmode_destroy(None) == 0


# --------------------------------------------------------- 7: the tiled chain ----
def test_filter_between_tile_order_P_and_Pt(cm):
    rng = np.random.default_rng(31)
    ndet, ns, npix, pol = 10, 2501, 300, 3               # groups of five: three templates leave a residual
    nt = ndet * ns
    p = rng.integers(0, npix, nt).astype(np.int32)
    p[rng.random(nt) < 0.1] = -1
    phi = rng.uniform(0, np.pi, nt)
    ang = type("Ang", (), {"cos": np.cos(2 * phi), "sin": np.sin(2 * phi)})()
    modes = cm.I.focalplane_modes(rng.uniform(-1, 1, (ndet, 2)), 1, 5)
    P = cm.I.SparseLO(npix, nt, p, pol=pol, angle_processed=ang)
    Fc = cm.I.CommonModeFilterLO(p, ndet, modes=modes, groups=5)
    assert Fc._tile_compatible(P) and not hasattr(Fc, "_apply_tiles")
    other = p.copy()
    other[np.flatnonzero(other >= 0)[0]] = -1
    assert not cm.I.CommonModeFilterLO(other, ndet, modes=modes, groups=5)._tile_compatible(P)
    x = rng.standard_normal(pol * npix)
    exact = P.T * (Fc * (P * x))
    cm.L.set_pointing_mode("tiled")
    try:
        A = P.T * Fc * P
        assert any(isinstance(op, cm.L._TiledNormalLO) for op in A._compiled())
        y1, y2 = np.asarray(A * x), np.asarray(A * x)
    finally:
        cm.L.set_pointing_mode("auto")
    assert same_bits(y1, y2)
    # what the existing tile tests allow for the tile-order P^T (test_gpu_round2.py): 1e-12 of the norm
    assert np.linalg.norm(y1 - exact) <= 1e-12 * np.linalg.norm(exact)


# ------------------------------------------------------------- 8: end to end ----
def test_common_mode_and_gradient_do_not_reach_the_map(cm):
    """expand_pointing -> P; d = P m + noise, with and without a common mode and a gradient over the focal plane a
    thousand times the noise; filter (order 1, two groups), bin, M_BD.  The two maps may differ by what the rounding
    of the two filter applications (c 2^-53 S each) and of P^T and M_BD gives, pushed through |M_BD| |P|^T."""
    nside, nd, order = 16, 12, 1
    npix, ns = 12 * nside * nside, PE.NS
    b, dq = PE.inputs("scan")
    rng = np.random.default_rng(78)
    flags = (rng.random(ns) < 0.02).astype(np.uint8)                    # whole samples: empty units
    pixs, c, s = cm.U.expand_pointing(b, dq[:nd], nside, flags=flags)
    drop = cm.torch.from_numpy(rng.random(nd * ns) < 0.05).to(pixs.device)
    pixs[drop] = -1                                                     # single detectors
    ces = cm.U.ProcessTimeSamples(pixs, npix, pol=3, cos_sin=(c, s))
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, nd * ns, pixs, pol=3, angle_processed=ces)
    Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, n, pol=3)
    edges = cm.I.cmode_groups(nd, 6)
    xy = rng.uniform(-1.0, 1.0, (nd, 2))
    modes = cm.I.focalplane_modes(xy, order, edges)
    Fc = cm.I.CommonModeFilterLO(pixs, nd, modes=modes, groups=edges)
    info = Fc.filter_info()
    assert info["fitted"] >= 0.9 * 2 * ns and info["empty"] >= 2 * int(flags.sum()) > 0
    m_true = rng.standard_normal(3 * n)
    base = np.asarray(P * m_true) + rng.standard_normal(nd * ns)
    t = np.arange(ns) / 100.0                                           # an atmosphere: slow in time, smooth in space
    amp = np.stack([1.0e3 * np.sin(2 * np.pi * f * t + ph) for f, ph in ((0.11, 0.3), (0.23, 1.1), (0.05, 2.0))])
    dirty = base + (modes @ amp).reshape(-1)
    to_map = lambda v: np.asarray(Mbd * (P.T * v))
    f_dirty, f_base = np.asarray(Fc * dirty), np.asarray(Fc * base)
    map_dirty, map_base, map_raw = to_map(f_dirty), to_map(f_base), to_map(dirty)
    # the bound, on the host
    h_pix, h_c, h_s = cm.D.to_host(pixs), cm.D.to_host(c), cm.D.to_host(s)
    r1 = R.cmode_ref(h_pix, nd, edges, modes, dirty)
    r0 = R.cmode_ref(h_pix, nd, edges, modes, base)
    ok = h_pix >= 0
    hits = np.bincount(h_pix[ok], minlength=n)
    cF = R._ld(R.c_samples(nd, ns, edges, modes.shape[1]))
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
    # grossly off without the filter: the contamination is slow, so the samples of a pixel do not average it away;
    # a hundred times the noise of one sample is a tenth of its amplitude
    assert raw.max() > 100.0
