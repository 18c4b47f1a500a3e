"""
The gap-aware normal operator on the GPU (cm2_gaps.hip, cosmomap2_amd/interfaces/gapaware.py) against the
restatement in NumPy / SciPy of _gap_aware_ref.py.  Every test runs in both pointing modes.

Shapes: nt = 4 * 8192 + 1234 = 34002 (five permutation windows, the last one partial) in blocks of 14000 and 20002
samples with different bands, nside 4 (192 pixels), I and IQU, uniform random pixels with at least 148 hits each;
flags at the stream's start and end, a run longer than the band, an isolated sample, runs across a window end and
across the block boundary, an alternating stretch, nothing in window 2 and -- for the application tests -- all of
window 3.  A second case of 5000 samples (blocks 3000 / 2000, nside 2) takes the per-sample permutations below one
window, a third has no flagged sample.  Band lengths 8 (direct sum), 64 (fused overlap-save) and 2049 (its limit).
The dense matrices of a case are built once and shared.

GPU iteration counts of the solve at rtol = 1e-10 (both modes) against scipy's cg on the dense A_e, M_e:
see DESIGN.md section 8.4.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse.linalg as sla

import _gap_aware_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

LAMS = [8, 64, 2049]
RTOL, OP_TOL = 1e-10, 1e-12            # cg's stopping rule; DESIGN.md section 4's bound of the FFT Toeplitz routes


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import linearoperators as L
    from cosmomap2_amd.utilities import gap_fill
    return SimpleNamespace(I=I, U=U, L=L, D=D, hip=_hip, gf=gap_fill, cg=cosmomap2_amd.cg, torch=torch)


@pytest.fixture(params=["tiled", "exact"], autouse=True)
def mode(cm, request):
    before = cm.L.POINTING_MODE
    cm.L.set_pointing_mode(request.param)
    yield request.param
    cm.L.set_pointing_mode(before)


_cases = {}


def case(cm, lam, pol, kind):
    """kind: 'gaps' (the five-window layout), 'whole' (with all of window 3 flagged), 'small' (below one window),
    'none' (no flagged sample).  The operators are shared between the tests and the two modes."""
    key = (lam, pol, kind)
    if key in _cases:
        return _cases[key]
    c = SimpleNamespace(lam=lam, pol=pol, kind=kind)
    if kind == "small":
        c.nt, c.sizes, c.npix, c.mask, seed = R.NT_SMALL, R.SIZES_SMALL, 48, R.flags_small(lam), 9
    else:
        c.nt, c.sizes, c.npix, seed = R.NT, R.SIZES, 192, 8
        c.mask = np.zeros(R.NT, dtype=bool) if kind == "none" else R.flags(lam, kind == "whole")
    c.pix, c.phi = R.scan(c.nt, c.npix, c.mask, seed)
    hits = np.bincount(c.pix[c.pix >= 0], minlength=c.npix)
    assert hits.min() >= (148 if kind in ("gaps", "none") else 60), hits.min()
    c.bands = R.bands(lam, R.SPECS)
    c.pos = np.flatnonzero(c.mask)
    c.nmap = pol * c.npix
    c.w = c.bands[:, 0][R.block_of(c.sizes, np.arange(c.nt))]
    c.N = cm.I.BlockLO(c.sizes, [b for b in c.bands], offdiag=True)
    pairs = c.pix.copy()
    ces = cm.U.ProcessTimeSamples(pairs, c.npix, pol=pol, phi=c.phi, w=c.w)
    assert ces.get_new_pixel[0] == c.npix and np.array_equal(pairs, c.pix)        # no pixel was cut
    c.P = cm.I.SparseLO(c.npix, c.nt, pairs, pol=pol, angle_processed=ces)
    c.Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, c.npix, pol=pol)
    c.op = cm.I.GapAwareNormalLO(c.P, c.N)
    assert c.op.ng == c.pos.size and c.op.nmap == c.nmap and c.op.shape == (c.nmap + c.pos.size,) * 2
    c.Pref = R.pointing(c.pix, c.phi, c.npix, pol)
    c.Pe = R.extended(c.Pref, c.pos)
    rng = np.random.default_rng(3)
    # data of the model itself: a map plus noise of the blocks' own spectra (see test_solve_equals_the_dense_solve)
    c.d = c.Pref @ (rng.standard_normal(c.nmap) * 10.0) + R.noise(c.sizes, R.SPECS, rng)
    c.d[c.mask] = 1e3
    c.dense = c.solved = None
    _cases[key] = c
    return c


def apply_ref(c, z):
    return c.Pe.T @ R.ninv(c.bands, c.sizes, c.Pe @ z)


def dense(c):
    """The dense system of a case with its reference solution, condition number and scipy's iteration count."""
    if c.dense is None:
        s = R.system(c.bands, c.sizes, c.pix, c.phi, c.npix, c.pol, c.d)
        s["z"] = np.linalg.solve(s["A"], s["b"])
        s["kappa"] = np.linalg.cond(s["A"])
        s["bound"] = s["kappa"] * (RTOL + OP_TOL)                # relative error <= kappa x relative residual
        its = []
        _, info = sla.cg(s["A"], s["b"], M=s["M"], rtol=RTOL, atol=0.0, callback=lambda xk: its.append(1))
        assert info == 0
        s["scipy_iterations"] = len(its)
        c.dense = s
    return c.dense


def solved(cm, c):
    """(z, info, iterations) of cg on the case's operator, per pointing mode."""
    if c.solved is None:
        c.solved = {}
    m = cm.L.POINTING_MODE
    if m not in c.solved:
        its = []
        z, info = cm.cg(c.op, c.op.rhs(c.d), M=c.op.preconditioner(c.Mbd), rtol=RTOL, maxiter=500,
                        callback=lambda zk: its.append(1))
        c.solved[m] = (z, info, len(its))
    return c.solved[m]


def part_errors(c, got, ref):
    n = c.nmap
    return rel_l2(got[:n], ref[:n]), (rel_l2(got[n:], ref[n:]) if ref.size > n else 0.0)


SHAPES = [(lam, pol, kind) for kind in ("gaps", "whole") for lam in LAMS for pol in (1, 3)] + \
         [(lam, pol, "small") for lam in (8, 64) for pol in (1, 3)]


# ------------------------------------------------------------------------------ application ------
@pytest.mark.parametrize("lam,pol,kind", SHAPES)
def test_application_equals_the_restatement(cm, mode, lam, pol, kind):
    c = case(cm, lam, pol, kind)
    z = np.random.default_rng(21).standard_normal(c.nmap + c.pos.size)
    out = c.op * z
    assert isinstance(out, np.ndarray) and out.shape == z.shape
    em, eg = part_errors(c, out, apply_ref(c, z))
    print("\n%s lam %d pol %d %s: ng %d, A_e z rel l2 map %.3g, gaps %.3g" % (mode, lam, pol, kind, c.pos.size, em, eg))
    assert em <= OP_TOL and eg <= OP_TOL, (em, eg)
    zd = cm.D.f64(z)
    od = c.op * zd
    assert od.is_cuda and od.dtype == cm.torch.float64
    np.testing.assert_array_equal(cm.D.to_host(od), out)
    m, g = c.op.split(od)
    assert m.numel() == c.nmap and g.numel() == c.pos.size and m.data_ptr() == od.data_ptr()
    if kind != "small":
        table = c.op.window_table()
        np.testing.assert_array_equal(table, R.window_table(c.pos, c.nt))
        if lam == 64:
            assert np.diff(table.astype(np.int64)).tolist() == [177, 37, 0, 8192 if kind == "whole" else 0, 204]
    else:
        assert c.op.window_table() is None


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("pol", [1, 3])
def test_without_flagged_samples_it_is_the_plain_normal_operator(cm, mode, lam, pol):
    c = case(cm, lam, pol, "none")
    assert c.op.ng == 0 and c.op.shape == (c.nmap, c.nmap)
    x = np.random.default_rng(22).standard_normal(c.nmap)
    out, plain = c.op * x, (c.P.T * c.N * c.P) * x
    assert rel_l2(out, plain) <= OP_TOL, rel_l2(out, plain)
    assert rel_l2(out, apply_ref(c, x)) <= OP_TOL
    b = c.op.rhs(c.d)
    assert rel_l2(b, c.Pref.T @ R.ninv(c.bands, c.sizes, c.d)) <= OP_TOL
    assert c.op.residual(c.d, x).shape == (c.nt,)


# ------------------------------------------------------------- the two permutations alone ------
@pytest.mark.parametrize("kind", ["gaps", "whole"])
@pytest.mark.parametrize("pol", [1, 3])
def test_merging_permutations_equal_the_two_call_forms_bit_for_bit(cm, kind, pol):
    c = case(cm, 64, pol, kind)
    T = c.op._tiles()
    g, st, ptr, D = c.op._gaps.h, cm.D.stream, cm.D.ptr, cm.D
    rng = np.random.default_rng(23)
    ng = c.pos.size
    assert T.nvalid + ng == c.nt
    tb, comp = D.f64(rng.standard_normal(T.nvalid)), D.f64(rng.standard_normal(ng))
    merged, plain = D.f64(np.full(c.nt, np.nan)), D.f64(np.full(c.nt, np.nan))
    cm.hip.call("cm2_gaps_tiles_to_time", g, T.h, ptr(tb), ptr(comp), ptr(merged), st())
    cm.hip.call("cm2_tod_tiles_to_time", T.h, ptr(tb), ptr(plain), st())
    cm.hip.call("cm2_gaps_scatter", g, ptr(comp), ptr(plain), st())
    merged_h = D.to_host(merged)
    assert np.all(np.isfinite(merged_h))
    np.testing.assert_array_equal(merged_h, D.to_host(plain))
    np.testing.assert_array_equal(merged_h[c.pos], D.to_host(comp))
    np.testing.assert_array_equal(np.sort(merged_h[~c.mask]), np.sort(D.to_host(tb)))
    time = D.f64(rng.standard_normal(c.nt))
    tb_m, tb_p = D.f64(np.full(T.nvalid, np.nan)), D.f64(np.full(T.nvalid, np.nan))
    comp_m, comp_p = D.f64(np.full(ng, np.nan)), D.f64(np.full(ng, np.nan))
    cm.hip.call("cm2_gaps_time_to_tiles", g, T.h, ptr(time), ptr(tb_m), ptr(comp_m), st())
    cm.hip.call("cm2_tod_time_to_tiles", T.h, ptr(time), ptr(tb_p), st())
    cm.hip.call("cm2_gaps_gather", g, ptr(time), ptr(comp_p), st())
    np.testing.assert_array_equal(D.to_host(tb_m), D.to_host(tb_p))
    np.testing.assert_array_equal(D.to_host(comp_m), D.to_host(comp_p))
    np.testing.assert_array_equal(D.to_host(comp_m), D.to_host(time)[c.pos])
    # there and back again
    back = D.f64(np.full(c.nt, np.nan))
    cm.hip.call("cm2_gaps_tiles_to_time", g, T.h, ptr(tb_m), ptr(comp_m), ptr(back), st())
    np.testing.assert_array_equal(D.to_host(back), D.to_host(time))


# --------------------------------------------------------------------------------- symmetry ------
@pytest.mark.parametrize("lam,pol,kind", SHAPES)
def test_symmetric_and_positive(cm, lam, pol, kind):
    c = case(cm, lam, pol, kind)
    rng = np.random.default_rng(24)
    u, v = rng.standard_normal(c.nmap + c.pos.size), rng.standard_normal(c.nmap + c.pos.size)
    Au, Av = c.op * u, c.op * v
    asym = abs(u @ Av - Au @ v) / (np.linalg.norm(u) * np.linalg.norm(Av))
    assert asym <= OP_TOL, asym
    assert v @ Av > 0 and u @ Au > 0


# ------------------------------------------------------------------------------------ solve ------
SOLVES = [(lam, pol, kind) for kind in ("gaps", "small") for lam in (8, 64) for pol in (1, 3)]


@pytest.mark.parametrize("lam,pol,kind", SOLVES)
def test_solve_equals_the_dense_solve(cm, mode, lam, pol, kind):
    """Relative error <= kappa_2(A_e) (rtol + 1e-12): kappa times the relative residual, which is cg's stopping
    rule plus the operator's rounding bound.  That inequality holds for the whole vector z = [m; g]; asked of each
    part alone it carries the factor |z| / |part|, so the parts must be of comparable norm.  The data is therefore
    drawn from the model (noise of each block's own spectrum, sigma 1 and 5): |g| / |m| is then 0.1 ... 0.5 and scipy's
    cg on the dense system leaves the gap part at 1e-8 ... 6e-8 of itself, a tenth of the bound (3.8e-7 ... 5.8e-7).
    White unit noise under these bands makes |g| / |m| = 0.02 and scipy's own cg misses the bound on the gap part
    (7e-7 against 4.75e-7 at lambda 8, I), and so does the GPU's, step for step."""
    c = case(cm, lam, pol, kind)
    s = dense(c)
    em, eg = part_errors(c, c.op.rhs(c.d), s["b"])
    assert em <= OP_TOL and eg <= OP_TOL, (em, eg)
    z, info, its = solved(cm, c)
    em, eg = part_errors(c, z, s["z"])
    es = rel_l2(z[:c.nmap], R.schur_map(s))
    print("\n%s lam %d pol %d %s: n %d + %d, kappa_2 %.4g, bound %.3g, %d iterations (scipy %d), map error %.3g, "
          "gap error %.3g, map against the Schur solve %.3g"
          % (mode, lam, pol, kind, c.nmap, c.pos.size, s["kappa"], s["bound"], its, s["scipy_iterations"], em, eg, es))
    assert info == 0
    assert em <= s["bound"] and eg <= s["bound"], (em, eg, s["bound"])
    assert es <= s["bound"], (es, s["bound"])
    assert abs(its - s["scipy_iterations"]) <= 1, (its, s["scipy_iterations"])
    # the one-call form: the same solve
    m, info, op = cm.I.solve_gls_with_gaps(c.P, c.N, c.d, M=c.Mbd, rtol=RTOL, maxiter=500)
    assert info == 0 and isinstance(info, int) and op.iterations == its
    np.testing.assert_array_equal(m, z[:c.nmap])
    np.testing.assert_array_equal(op.gap_solution, z[c.nmap:])


# --------------------------------------------------------------------------------- residual ------
@pytest.mark.parametrize("lam,pol,kind", SOLVES)
def test_residual_is_the_gap_filled_noise_residual(cm, lam, pol, kind):
    c = case(cm, lam, pol, kind)
    s = dense(c)
    z, _, _ = solved(cm, c)
    r = c.op.residual(c.d, z)
    assert isinstance(r, np.ndarray) and r.shape == (c.nt,)
    Pm = c.P * z[:c.nmap]
    np.testing.assert_array_equal(r[~c.mask], (c.d - Pm)[~c.mask])
    np.testing.assert_array_equal(r[c.mask], -z[c.nmap:])
    r0 = np.where(c.mask, 0.0, c.d - c.Pref @ s["z"][:c.nmap])
    Qgg = s["Q"][c.pos][:, c.pos].toarray()
    ref = -np.linalg.solve(Qgg, (s["Q"] @ r0)[c.pos])
    e = rel_l2(r[c.mask], ref)
    assert e <= s["bound"], (e, s["bound"])
    rd = c.op.residual(cm.D.f64(c.d), cm.D.f64(z))
    assert rd.is_cuda
    np.testing.assert_array_equal(cm.D.to_host(rd), r)


# ------------------------------------------------------------------------------- NaN safety ------
@pytest.mark.parametrize("lam", [8, 64])
def test_flagged_values_never_enter_the_solve(cm, lam):
    c = case(cm, lam, 3, "gaps")
    outs = []
    for junk in (np.nan, 1e30):
        d = c.d.copy()
        d[c.mask] = junk
        b = c.op.rhs(d)
        m, info, op = cm.I.solve_gls_with_gaps(c.P, c.N, d, M=c.Mbd, rtol=RTOL, maxiter=500)
        assert info == 0 and np.all(np.isfinite(b)) and np.all(np.isfinite(m)) and np.all(np.isfinite(op.gap_solution))
        outs.append((b, m, op.gap_solution, op.residual(d, np.concatenate([m, op.gap_solution]))))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(outs[0][3]))


# ------------------------------------------------------------------------------- allocation ------
def test_an_application_allocates_nothing_of_tod_size(cm):
    t = cm.torch
    c = case(cm, 64, 3, "gaps")
    z = cm.D.f64(np.random.default_rng(25).standard_normal(c.nmap + c.pos.size))
    M = c.op.preconditioner(c.Mbd)
    y, q = c.op * z, M * z                                   # the first application: plans, lists and scratch exist
    t.cuda.synchronize()
    t.cuda.reset_peak_memory_stats()
    lib0, torch0 = cm.D.memory_info(), t.cuda.memory_allocated()
    for _ in range(5):
        y, q = c.op * z, M * z
    t.cuda.synchronize()
    lib1, peak = cm.D.memory_info(), t.cuda.max_memory_allocated()
    assert lib1["live_bytes"] == lib0["live_bytes"] and lib1["driver_allocations"] == lib0["driver_allocations"]
    assert peak - torch0 < 8 * c.nt, (peak, torch0)


# -------------------------------------------------------------------------------- refusals ------
def test_prepare_refuses_a_handle_of_another_pointing(cm):
    c = case(cm, 64, 1, "gaps")
    T = c.op._tiles()
    lib, st = cm.hip.load(), cm.D.stream
    a0 = [b[0] for b in c.bands]

    def handle(mask, sizes=c.sizes):
        return cm.gf._Gaps(np.where(mask, -1, 0).astype(np.int32), sizes, a0)

    moved = np.roll(c.mask, 1)                               # as many flagged samples, other positions
    assert moved.sum() == c.mask.sum() and not np.array_equal(moved, c.mask)
    more = c.mask.copy()
    more[20000] = True
    for G, word in ((handle(moved), b"sample 3 "), (handle(more), b"valid samples"),
                    (handle(c.mask[:-1], [14000, 20001]), b"nt=")):
        rc = lib.cm2_gaps_prepare_tiles(G.h, T.h, st())
        msg = lib.cm2_last_error()
        assert rc == cm.hip.ERR_ARGUMENT, (rc, msg)
        assert b"cm2_gaps_prepare_tiles" in msg and word in msg, msg
        # a handle that was refused is not prepared: the permutations refuse it too
        buf = cm.D.empty(c.nt)
        rc = lib.cm2_gaps_tiles_to_time(G.h, T.h, cm.D.ptr(buf), cm.D.ptr(buf), cm.D.ptr(buf), st())
        assert rc == cm.hip.ERR_ARGUMENT and b"cm2_gaps_prepare_tiles has not been called" in lib.cm2_last_error()
    same = handle(c.mask)
    assert lib.cm2_gaps_prepare_tiles(same.h, T.h, st()) == 0
    assert lib.cm2_gaps_prepare_tiles(c.op._gaps.h, T.h, st()) == 0
    cm.torch.cuda.synchronize()
