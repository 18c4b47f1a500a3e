"""
Destriping on the GPU (cm2_offsets.hip, cosmomap2_amd/interfaces/destriper.py) against the restatement in NumPy /
SciPy of _destriper_ref.py, whose docstring has the definitions.

The common case: nt = 34002 = 4 * 8192 + 1234 (five windows, the last one partial) in blocks of 14000 and 20002
samples with weights 1.0 and 2.5, nside 4 (192 pixels), uniformly random pixels and angles, I and IQU; flagged: 40
samples from every 400th starting at 123, all of window 3, [13990, 14010) across the block boundary.  L = 37 / 1000 /
10000 gives 920 / 35 / 5 baselines of which 229 / 7 / 0 are empty.  The prior of the solves: per block the band
a_0 = 0.5, a_k = -0.15 0.6^k (1 <= k < 8).  Edge cases: 5000 samples (below one window: the per-sample permutations),
32768 samples in two blocks with L = 8192 (baselines equal windows), 9000 samples in blocks of 4000 and 5000 with
L = 1 and L = 6000 (one baseline per block), and the common stream without flags.  The dense matrices of a case are
built once and shared.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse.linalg as sla

import _destriper_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

RTOL, OP_TOL = 1e-10, 1e-12
COMMON = ["common37", "common1000", "common10000"]
EDGES = ["short", "windows", "every_sample", "one_per_block", "no_flags"]


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd import _hip, device as D
    from cosmomap2_amd.interfaces import destriper, linearoperators as L
    return SimpleNamespace(I=I, U=U, L=L, D=D, hip=_hip, ds=destriper, cg=cosmomap2_amd.cg, torch=torch)


@pytest.fixture(params=["tiled", "exact"])
def mode(cm, request):
    before = cm.L.POINTING_MODE
    cm.L.set_pointing_mode(request.param)
    yield request.param
    cm.L.set_pointing_mode(before)


_cases = {}


def case(cm, name, pol):
    """The operators and the dense restatement of a layout, shared between the tests and the two modes."""
    key = (name, pol)
    if key in _cases:
        return _cases[key]
    nt, sizes, weights, Lb, flags = R.LAYOUTS[name]
    c = SimpleNamespace(name=name, pol=pol, nt=nt, sizes=list(sizes), weights=weights, L=Lb, mask=flags())
    c.npix = 192 if nt > 20000 else 48
    c.pix, c.phi = R.scan(nt, c.npix, c.mask, 11)
    c.valid = ~c.mask
    c.B = R.baselines(sizes, Lb)
    c.wt = R.sample_weights(sizes, weights, np.ones(nt, dtype=bool))          # w_b of every sample
    pairs = c.pix.copy()
    ces = cm.U.ProcessTimeSamples(pairs, c.npix, pol=pol, phi=c.phi, w=c.wt)
    assert ces.get_new_pixel[0] == c.npix and np.array_equal(pairs, c.pix)    # no pixel was cut
    c.P = cm.I.SparseLO(c.npix, nt, pairs, pol=pol, angle_processed=ces)
    c.Mbd = cm.I.BlockDiagonalPreconditionerLO(ces, c.npix, pol=pol)
    c.F = cm.I.OffsetsLO(c.P, list(sizes), Lb, weights=None if weights is None else list(weights))
    c.nmap = pol * c.npix
    rng = np.random.default_rng(12)
    c.sky = rng.standard_normal(c.nmap)
    c.walk = np.cumsum(0.5 * rng.standard_normal(c.B.na))                      # a random walk of step 0.5
    c.Pref = R.pointing(c.pix, c.phi, c.npix, pol)
    c.d = c.Pref @ c.sky + c.walk[c.B.j_of_t] + rng.standard_normal(nt) / np.sqrt(c.wt)
    c.d[c.mask] = 1e3
    c.sys, c.ops, c.solved = {}, {}, {}
    _cases[key] = c
    return c


def dense(c, prior):
    if prior not in c.sys:
        s = R.system(c.sizes, c.weights, c.L, c.pix, c.phi, c.npix, c.pol, c.d, prior=prior)
        ev = np.linalg.eigvalsh(s.A)
        pos = ev[ev > 1e-9 * ev.max()]
        s.kappa = pos.max() / pos.min()                      # over the range of A (without a prior it has a null vector)
        its = []
        s.a_cg, info = sla.cg(s.A, s.b, M=np.diag(s.jac), rtol=RTOL, atol=0.0, callback=lambda xk: its.append(1))
        assert info == 0
        s.scipy_iterations = len(its)
        c.sys[prior] = s
    return c.sys[prior]


def operator(cm, c, prior):
    if prior not in c.ops:
        C = cm.I.BlockLO(c.F.baselines_per_block, [R.PRIOR_BAND] * len(c.sizes), offdiag=True) if prior else None
        c.ops[prior] = cm.I.DestriperNormalLO(c.P, c.F, c.Mbd, prior=C)
    return c.ops[prior]


def solve(cm, c, prior, d=None):
    op = operator(cm, c, prior)
    return cm.I.solve_destriped(c.P, c.sizes, c.L, c.d if d is None else d, c.Mbd,
                                weights=None if c.weights is None else list(c.weights), prior=op.prior, rtol=RTOL,
                                maxiter=500)


def raw(cm, c):
    return c.F._f.h, cm.D.stream, cm.D.ptr, cm.D


def without_monopole(m, pol):
    m = np.array(m, dtype=np.float64)
    if pol in (1, 3):
        m[0::pol] -= m[0::pol].mean()
    return m


ALL = [(n, 1) for n in COMMON + EDGES] + [(n, 3) for n in COMMON]


# ------------------------------------------------------------------------------- 1: the counts ------
@pytest.mark.parametrize("name,pol", ALL)
def test_counts_equal_numpy(cm, name, pol):
    c = case(cm, name, pol)
    nvalid, wsum = R.counts(c.B, c.valid, c.weights)
    assert c.F.na == c.B.na and c.F.baselines_per_block == c.B.per_block and c.F.shape == (c.nt, c.B.na)
    assert c.F.nvalid.dtype == np.int64
    np.testing.assert_array_equal(c.F.nvalid, nvalid)
    np.testing.assert_array_equal(c.F.wsum, wsum)
    info = c.F._f.info()
    assert (info["nt"], info["na"], info["nvalid"], info["baseline_length"]) == (c.nt, c.B.na, c.valid.sum(), c.L)
    if name.startswith("common"):
        assert (c.B.na, int((nvalid == 0).sum())) == {37: (920, 229), 1000: (35, 7), 10000: (5, 0)}[c.L]


# ------------------------------------------------------------------- 2: expand and residual ------
@pytest.mark.parametrize("name,pol", ALL)
def test_expand_and_residual_are_bit_equal_to_numpy(cm, name, pol):
    c = case(cm, name, pol)
    h, st, ptr, D = raw(cm, c)
    rng = np.random.default_rng(31)
    a = rng.standard_normal(c.B.na)
    aj = a[c.B.j_of_t]
    ad, dd = D.f64(a), D.f64(c.d)
    for weighted in (0, 1):
        w = c.wt if weighted else np.ones(c.nt)
        out = D.f64(np.full(c.nt, np.nan))
        cm.hip.call("cm2_offsets_expand", h, ptr(ad), weighted, ptr(out), st())
        np.testing.assert_array_equal(D.to_host(out), np.where(c.valid, w * aj, 0.0))
        cm.hip.call("cm2_offsets_residual", h, ptr(dd), ptr(ad), weighted, ptr(out), st())
        np.testing.assert_array_equal(D.to_host(out), np.where(c.valid, w * (c.d - aj), 0.0))
        cm.hip.call("cm2_offsets_residual", h, ptr(dd), None, weighted, ptr(out), st())
        np.testing.assert_array_equal(D.to_host(out), np.where(c.valid, w * c.d, 0.0))
        alias = dd.clone()                                   # out may be d
        cm.hip.call("cm2_offsets_residual", h, ptr(alias), ptr(ad), weighted, ptr(alias), st())
        np.testing.assert_array_equal(D.to_host(alias), np.where(c.valid, w * (c.d - aj), 0.0))
    np.testing.assert_array_equal(c.F * a, np.where(c.valid, aj, 0.0))
    assert (c.F * ad).is_cuda


# ---------------------------------------------------------------------------- 3: to the tiles ------
@pytest.mark.parametrize("name,pol", ALL)
def test_to_tiles_is_bit_equal_to_expand_then_permute(cm, name, pol):
    c = case(cm, name, pol)
    h, st, ptr, D = raw(cm, c)
    T = c.F._tiles()
    assert T.nvalid == c.valid.sum()
    assert c.F._f.info()["tile_forms"] == (2 if c.nt < R.WIN else 1)
    a = D.f64(np.random.default_rng(32).standard_normal(c.B.na))
    for weighted in (0, 1):
        fused, two = D.f64(np.full(T.nvalid, np.nan)), D.f64(np.full(T.nvalid, np.nan))
        time = D.empty(c.nt)
        cm.hip.call("cm2_offsets_to_tiles", h, T.h, ptr(a), weighted, ptr(fused), st())
        cm.hip.call("cm2_offsets_expand", h, ptr(a), weighted, ptr(time), st())
        cm.hip.call("cm2_tod_time_to_tiles", T.h, ptr(time), ptr(two), st())
        got = D.to_host(fused)
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, D.to_host(two))


# ---------------------------------------------------------------------------------- 4: the sum ------
@pytest.mark.parametrize("name,pol", ALL)
def test_sum_within_the_bound_of_any_summation_order(cm, name, pol):
    """|err_j| <= nvalid_j 2^-53 sum |y_t|: n - 1 additions, each rounding by at most 2^-53 of a partial sum that
    is at most sum |y_t| in magnitude (first order), whatever their order; the weighted form adds one rounding of the
    product, 2^-53 w_b |sum|."""
    c = case(cm, name, pol)
    h, st, ptr, D = raw(cm, c)
    y = np.random.default_rng(33).standard_normal(c.nt) * 10.0
    y[c.mask] = 1e30                                         # a flagged sample is never added
    s, sabs = R.exact_sums(c.B, c.valid, y)
    nvalid, _ = R.counts(c.B, c.valid, c.weights)
    wb = (np.ones(len(c.sizes)) if c.weights is None else np.asarray(c.weights))[c.B.block]
    yd = D.f64(y)
    out = D.f64(np.full(c.B.na, np.nan))
    cm.hip.call("cm2_offsets_sum", h, ptr(yd), 0, ptr(out), st())
    got = D.to_host(out)
    err, bound = np.abs(got - s), nvalid * 2.0 ** -53 * sabs
    print("\n%s pol %d: F^T y, worst error / bound %.3g" % (name, pol, (err / np.where(bound > 0, bound, np.inf)).max()))
    assert np.all(err <= bound), (err - bound).max()
    assert np.all(got[nvalid == 0] == 0.0)
    cm.hip.call("cm2_offsets_sum", h, ptr(yd), 1, ptr(out), st())
    np.testing.assert_array_equal(D.to_host(out), wb * got)                  # the weight once, on the sum
    np.testing.assert_array_equal(c.F.T * y, got)


# -------------------------------------------------------------------------- 5: from the tiles ------
@pytest.mark.parametrize("name,pol", ALL)
def test_from_tiles_is_bit_equal_to_permute_then_sum(cm, name, pol):
    c = case(cm, name, pol)
    h, st, ptr, D = raw(cm, c)
    T = c.F._tiles()
    tb = D.f64(np.random.default_rng(34).standard_normal(T.nvalid) * 10.0)
    for weighted in (0, 1):
        fused, again, two = (D.f64(np.full(c.B.na, np.nan)) for _ in range(3))
        time = D.f64(np.full(c.nt, np.nan))
        cm.hip.call("cm2_offsets_from_tiles", h, T.h, ptr(tb), weighted, ptr(fused), st())
        cm.hip.call("cm2_tod_tiles_to_time", T.h, ptr(tb), ptr(time), st())
        cm.hip.call("cm2_offsets_sum", h, ptr(time), weighted, ptr(two), st())
        cm.hip.call("cm2_offsets_from_tiles", h, T.h, ptr(tb), weighted, ptr(again), st())
        got = D.to_host(fused)
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, D.to_host(two))
        np.testing.assert_array_equal(got, D.to_host(again))


# ------------------------------------------------------------------------------------ 6: A a ------
# (with the prior only where a block has at least as many offsets as the band has values: not at L = 10000)
APPLY = [(n, p, prior) for n in COMMON + ["short", "no_flags"] for p in (1, 3) for prior in (False, True)
         if not (prior and n == "common10000") and (p == 1 or n in COMMON + ["short"])]


@pytest.mark.parametrize("name,pol,prior", APPLY)
def test_normal_operator_equals_the_dense_restatement(cm, mode, name, pol, prior):
    c = case(cm, name, pol)
    assert not prior or min(c.B.per_block) >= len(R.PRIOR_BAND)
    s, op = dense(c, prior), operator(cm, c, prior)
    assert op.shape == (c.B.na, c.B.na) and op.symmetric
    rng = np.random.default_rng(35)
    x, y = rng.standard_normal(c.B.na), rng.standard_normal(c.B.na)
    Ax, Ay = op * x, op * y
    scale = np.linalg.norm(s.wsum * x)                       # relative to the uncancelled term: A cancels along constants
    e = np.linalg.norm(Ax - s.A @ x) / scale
    asym = abs(x @ Ay - Ax @ y) / (np.linalg.norm(x) * np.linalg.norm(s.wsum * y))
    print("\n%s %s pol %d prior %d: A x error %.3g, asymmetry %.3g" % (mode, name, pol, prior, e, asym))
    assert e <= OP_TOL, e
    assert asym <= OP_TOL, asym
    if not prior:
        one = np.where(s.empty, 0.0, 1.0)
        null = np.linalg.norm(op * one) / np.linalg.norm(s.wsum)
        assert null <= OP_TOL, null
    assert rel_l2(op.rhs(c.d), s.b) <= 1e-11
    xd = cm.D.f64(x)
    assert (op * xd).is_cuda
    np.testing.assert_array_equal(cm.D.to_host(op * xd), Ax)


# ------------------------------------------------------------------- 7: the solve with the prior ------
@pytest.mark.parametrize("name,pol", [(n, p) for n in ("common37", "common1000") for p in (1, 3)])
def test_solve_with_the_prior_equals_the_dense_solve(cm, mode, name, pol):
    """Relative error <= kappa_2(A) (rtol + 1e-12): kappa times the relative residual, which is cg's stopping rule
    plus the operator's rounding bound.  SciPy's Jacobi-CG on the dense matrix takes 35 / 34 (L = 37, I / IQU) and
    12 / 13 (L = 1000) iterations."""
    c = case(cm, name, pol)
    s = dense(c, True)
    a_ref = np.linalg.solve(s.A, s.b)
    m_ref = R.map_of(s, a_ref)
    bound = s.kappa * (RTOL + OP_TOL)
    m, a, info, op = solve(cm, c, True)
    ea, em = rel_l2(a, a_ref), rel_l2(m, m_ref)
    print("\n%s %s pol %d: kappa_2 %.4g, bound %.3g, %d iterations (scipy %d), offsets %.3g, map %.3g"
          % (mode, name, pol, s.kappa, bound, op.iterations, s.scipy_iterations, ea, em))
    assert info == 0 and isinstance(a, np.ndarray) and a.shape == (c.B.na,) and m.shape == (c.nmap,)
    assert ea <= bound and em <= bound, (ea, em, bound)
    assert abs(op.iterations - s.scipy_iterations) <= 1, (op.iterations, s.scipy_iterations)
    assert op.F.na == c.B.na and op.prior is not None


# ---------------------------------------------------------------- 8: the solve without a prior ------
@pytest.mark.parametrize("name,pol", [(n, p) for n in COMMON for p in (1, 3)])
def test_solve_without_a_prior(cm, mode, name, pol):
    """A is singular along the constant on the non-empty baselines; d0 - F a - P m on the valid samples is unique and
    is compared with the least-squares solution's to 1e-8 (SciPy's own CG at this rtol leaves 2.5e-10).  The map is
    compared after the mean of the I difference is removed, within kappa (rtol + 1e-12) with kappa taken over the
    range of A: m = M P^T W (d0 - F a) is a bounded function of a, and a's error orthogonal to the null vector is
    bounded by kappa times cg's relative residual."""
    c = case(cm, name, pol)
    s = dense(c, False)
    r_ref, m_ref, _ = R.lstsq_residual(s)
    m, a, info, op = solve(cm, c, False)
    r = (s.d0 - s.F @ a - s.P @ m)[s.valid]
    er = rel_l2(r, r_ref)
    diff = m - m_ref
    diff[0::pol] -= diff[0::pol].mean()
    em = np.linalg.norm(diff) / np.linalg.norm(m_ref)
    bound = s.kappa * (RTOL + OP_TOL)
    print("\n%s %s pol %d: %d iterations (scipy %d), residual against lstsq %.3g, map %.3g (bound %.3g)"
          % (mode, name, pol, op.iterations, s.scipy_iterations, er, em, bound))
    assert info == 0
    assert er <= 1e-8, er
    assert em <= bound, (em, bound)
    assert np.all(a[s.empty] == 0.0)
    assert abs(op.iterations - s.scipy_iterations) <= 1, (op.iterations, s.scipy_iterations)
    np.testing.assert_array_equal(op.cleaned(c.d, a), np.where(c.valid, c.d - a[c.B.j_of_t], 0.0))


# ---------------------------------------------------------------------------------- 9: closure ------
@pytest.mark.parametrize("name,pol", [(n, p) for n in COMMON for p in (1, 3)])
def test_closure_binned_and_destriped_map_errors(cm, mode, name, pol):
    """Offsets from a random walk of step 0.5, white noise of variance 1 / w, a unit-normal sky: the error of the
    binned map and of the destriped map (I monopole removed) agree with the restatement's to 1e-8; their ratio is a
    record (9.4 / 6.5 at L = 37, 1.5 / 1.2 at L = 1000, 1.1 / 1.1 at L = 10000 for I / IQU in the issue's run)."""
    c = case(cm, name, pol)
    s = dense(c, False)
    _, m_ref, _ = R.lstsq_residual(s)
    m, a, info, op = solve(cm, c, False)
    binned = op.map(c.d, np.zeros(c.B.na))
    binned_ref = R.map_of(s, np.zeros(c.B.na))
    errs = [np.linalg.norm(without_monopole(x - c.sky, pol)) for x in (binned, binned_ref, m, m_ref)]
    print("\n%s %s pol %d: binned error %.4g, destriped error %.4g, ratio %.3g (restatement %.3g)"
          % (mode, name, pol, errs[0], errs[2], errs[0] / errs[2], errs[1] / errs[3]))
    assert abs(errs[0] - errs[1]) <= 1e-8 * errs[1], errs
    assert abs(errs[2] - errs[3]) <= 1e-8 * errs[3], errs


# ------------------------------------------------------------------------------ 10: NaN safety ------
@pytest.mark.parametrize("name", ["common37", "common10000"])
def test_flagged_values_never_enter(cm, mode, name):
    c = case(cm, name, 3)
    outs = []
    for junk in (0.0, np.nan, 1e30):
        d = c.d.copy()
        d[c.mask] = junk
        m, a, info, op = solve(cm, c, False, d=d)
        assert info == 0
        outs.append((op.rhs(d), m, a, op.cleaned(d, a), op.map(d, a)))
    for x in outs[0]:
        assert np.all(np.isfinite(x))
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------ 11: allocation ------
@pytest.mark.parametrize("prior", [False, True])
def test_an_application_allocates_its_result_only(cm, mode, prior):
    t = cm.torch
    c = case(cm, "common37", 3)
    op = operator(cm, c, prior)
    x = cm.D.f64(np.random.default_rng(36).standard_normal(c.B.na))
    y = op * x                                               # the first application: plans, lists and scratch exist
    t.cuda.synchronize()
    t.cuda.reset_peak_memory_stats()
    lib0, torch0 = cm.D.memory_info(), t.cuda.memory_allocated()
    for _ in range(5):
        y = op * x
    t.cuda.synchronize()
    lib1, peak = cm.D.memory_info(), t.cuda.max_memory_allocated()
    assert lib1["live_bytes"] == lib0["live_bytes"] and lib1["driver_allocations"] == lib0["driver_allocations"]
    assert t.cuda.memory_allocated() == torch0
    assert peak - torch0 < 8 * c.nt, (peak, torch0)                          # results of na values, nothing TOD-sized
    del y


# -------------------------------------------------------------------------------- 12: refusals ------
def test_prepare_refuses_a_handle_of_another_pointing(cm):
    c = case(cm, "common1000", 1)
    T = c.F._tiles()
    lib, st = cm.hip.load(), cm.D.stream

    def handle(mask, sizes=c.sizes):
        pix = np.where(mask, -1, 0).astype(np.int32)
        return cm.ds._Offsets(cm.D.i32(pix), sizes, c.L, None)

    moved = np.roll(c.mask, 1)                               # as many flagged samples, other positions
    assert moved.sum() == c.mask.sum() and np.flatnonzero(moved != c.mask)[0] == 123
    more = c.mask.copy()
    more[20000] = True
    assert not c.mask[20000]
    for G, word in ((handle(moved), b"sample 123 "), (handle(more), b"valid samples"),
                    (handle(c.mask[:-1], [14000, 20001]), b"nt=")):
        rc = lib.cm2_offsets_prepare_tiles(G.h, T.h, st())
        msg = lib.cm2_last_error()
        assert rc == cm.hip.ERR_ARGUMENT, (rc, msg)
        assert b"cm2_offsets_prepare_tiles" in msg and word in msg, msg
        # a handle that was refused is not prepared: the tile forms refuse it too
        buf = cm.D.empty(c.nt)
        rc = lib.cm2_offsets_to_tiles(G.h, T.h, cm.D.ptr(buf), 0, cm.D.ptr(buf), st())
        assert rc == cm.hip.ERR_ARGUMENT and b"cm2_offsets_prepare_tiles has not been called" in lib.cm2_last_error()
        rc = lib.cm2_offsets_from_tiles(G.h, T.h, cm.D.ptr(buf), 0, cm.D.ptr(buf), st())
        assert rc == cm.hip.ERR_ARGUMENT and b"cm2_offsets_prepare_tiles has not been called" in lib.cm2_last_error()
    same = handle(c.mask)
    assert lib.cm2_offsets_prepare_tiles(same.h, T.h, st()) == 0
    assert lib.cm2_offsets_prepare_tiles(c.F._f.h, T.h, st()) == 0
    cm.torch.cuda.synchronize()
