"""
Gap filling on the GPU (cm2_gaps.hip, cosmomap2_amd/utilities/gap_fill.py) against a dense restatement in NumPy:
Q_GG[i, j] = a_b[|t_i - t_j|] inside a block and below the band length, N^-1 on a stream by
scipy.signal.fftconvolve(..., 'same') per block, numpy.linalg.solve for the fill.  Two unequal blocks with
different bands, band lengths on the direct route (8), the fused overlap-save route (64) and its upper limit
(2049), one layout of flags that crosses window ends, the band and the block boundary.  Deterministic from
fixed seeds; the dense matrices of a band length are built once and shared.
"""
import gc

import numpy as np
import pytest
import scipy.signal as ss

from conftest import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [40000, 23456]
N0, NT = SIZES[0], sum(SIZES)
LAMS = [8, 64, 2049]
NPERSEG = {8: 256, 64: 256, 2049: 8192}
NG = {8: 306, 64: 362, 2049: 2347}
RTOL, OP_TOL = 1e-10, 1e-12            # cg's stopping rule; DESIGN.md section 4's bound of the FFT Toeplitz routes


@pytest.fixture(scope="module")
def cm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    import cosmomap2_amd.interfaces as I
    import cosmomap2_amd.utilities as U
    from cosmomap2_amd.utilities import noise_model, noise_sim, gap_fill
    from cosmomap2_amd import device as D
    from types import SimpleNamespace
    return SimpleNamespace(I=I, U=U, nm=noise_model, ns=noise_sim, gf=gap_fill, torch=torch, D=D)


def to_dev(cm, a):
    return cm.D.f64(np.ascontiguousarray(a))


def to_host(cm, t):
    return cm.D.to_host(t)


# ------------------------------------------------------------------ restatements in NumPy ------
def layout(lam):
    """The flagged samples of the issue's layout, as a bool mask."""
    m = np.zeros(NT, dtype=bool)
    m[0] = True
    m[12280:12300] = True                                   # crosses a window's output end
    m[16380:16390] = True                                   # crosses a window's input end
    m[20000:20000 + lam + 136] = True                       # longer than the band
    m[26000:26050] = True                                   # two runs coupled through the band
    m[26050 + lam // 2:26100 + lam // 2] = True
    m[N0 - 10:N0 + 10] = True                               # straddles the block boundary
    m[N0 + 5000] = True
    m[N0 + 7000:N0 + 7003] = True
    m[NT - 7:] = True
    return m


def runs_ref(mask, sizes):
    """Rows (start, length, block) of the runs of flagged samples, cut at the block boundaries."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = []
    for b in range(len(sizes)):
        idx = np.flatnonzero(mask[off[b]:off[b + 1]]) + off[b]
        if idx.size:
            for run in np.split(idx, np.flatnonzero(np.diff(idx) != 1) + 1):
                rows.append((run[0], run.size, b))
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


def psds(L):
    """One-sided PSDs [2, L/2+1]: block 0 from S = 1 + (0.02/f)^1.5, block 1 from S = 25 (1 + 0.05/f)."""
    f = np.fft.rfftfreq(L)
    S = np.empty((2, f.size))
    S[0, 1:] = 1.0 + (0.02 / f[1:]) ** 1.5
    S[1, 1:] = 25.0 * (1.0 + 0.05 / f[1:])
    S[:, 0] = S[:, 1]
    m = np.full(f.size, 2.0)
    m[0] = m[-1] = 1.0
    return S * m


def ninv_ref(bands, sizes, v):
    """N^-1 v: per block the zero-boundary product with the symmetric band."""
    out, o = np.empty_like(v), 0
    for a, n in zip(bands, sizes):
        out[o:o + n] = ss.fftconvolve(v[o:o + n], np.concatenate([a[:0:-1], a]), "same")
        o += n
    return out


def qgg_ref(bands, sizes, pos):
    off = np.concatenate([[0], np.cumsum(sizes)])
    blk = np.searchsorted(off, pos, side="right") - 1
    lam = len(bands[0])
    Q = np.zeros((pos.size, pos.size))
    for b, a in enumerate(bands):
        sel = np.flatnonzero(blk == b)
        dt = np.abs(pos[sel][:, None].astype(np.int64) - pos[sel][None, :].astype(np.int64))
        Q[np.ix_(sel, sel)] = np.concatenate([a, [0.0]])[np.minimum(dt, lam)]
    return Q


def linear_ref(d, mask, sizes, nedge):
    out = d.copy()
    off = np.concatenate([[0], np.cumsum(sizes)])
    for s, ln, b in runs_ref(mask, sizes):
        e, b0, b1 = s + ln, off[b], off[b + 1]
        level = []
        for rng in (range(max(b0, s - nedge), s), range(e, min(b1, e + nedge))):
            tot, cnt = 0.0, 0
            for i in rng:                                    # in time order
                if not mask[i]:
                    tot, cnt = tot + d[i], cnt + 1
            level.append(tot / cnt if cnt else None)
        L, R = level
        L = R if L is None else L
        R = L if R is None else R
        if L is None:
            L = R = 0.0
        for k in range(ln):
            out[s + k] = L + (R - L) * (k + 1) / (ln + 1)
    return out


_problems = {}


def problem(cm, lam):
    """Everything the tests of one band length share: bands, operator, filler, data, the dense matrices."""
    if lam in _problems:
        return _problems[lam]
    from types import SimpleNamespace
    p = SimpleNamespace(lam=lam, mask=layout(lam))
    p.psd = psds(NPERSEG[lam])
    p.bands = np.asarray(cm.nm.inverse_noise_bands(p.psd, lam))
    p.N = cm.I.BlockLO(SIZES, [b for b in p.bands], offdiag=True)
    p.pix = np.where(p.mask, -1, np.arange(NT) % 3072).astype(np.int32)
    p.gf = cm.gf.GapFiller(p.pix, p.N)
    p.pos = np.flatnonzero(p.mask)
    p.d = np.random.default_rng(3).standard_normal(NT)
    p.Q = qgg_ref(p.bands, SIZES, p.pos)
    p.kappa = np.linalg.cond(p.Q)
    p.bound = p.kappa * (RTOL + OP_TOL)                      # relative error <= kappa x relative residual
    p.qgv_d = ninv_ref(p.bands, SIZES, np.where(p.mask, 0.0, p.d))[p.pos]
    p.x_ref = -np.linalg.solve(p.Q, p.qgv_d)
    _problems[lam] = p
    return p


# -------------------------------------------------------------------------------- index ------
@pytest.mark.parametrize("lam", LAMS)
def test_index_structure(cm, lam):
    p = problem(cm, lam)
    runs = runs_ref(p.mask, SIZES)
    assert p.pos.size == NG[lam]
    for flags in (p.pix, p.mask, p.pix.astype(np.int64), cm.D.i32(p.pix), cm.D.to_dev(p.mask)):
        g = cm.gf.GapFiller(flags, p.N)
        info = g.info()
        assert info["nt"] == NT and info["ng"] == g.ng == NG[lam] and info["runs"] == len(runs) == 11, info
        assert info["longest_run"] == lam + 136 and info["buffer_bytes"] == 16 * NT, info
        pos, table = g.index()
        np.testing.assert_array_equal(pos, p.pos)
        np.testing.assert_array_equal(table, runs)
    # the run across the block boundary is two runs
    assert [N0 - 10, 10, 0] in runs.tolist() and [N0, 10, 1] in runs.tolist()


# ----------------------------------------------------------------------------- operator ------
@pytest.mark.parametrize("lam", LAMS)
def test_normal_operator_equals_dense_qgg(cm, lam):
    p = problem(cm, lam)
    y = np.random.default_rng(11).standard_normal(p.pos.size)
    out = to_host(cm, p.gf.normal_apply(to_dev(cm, y)))
    e = rel_l2(out, p.Q @ y)
    print("\nlam %d: Q_GG y against the dense product, rel l2 %.3g (kappa_2 %.4g)" % (lam, e, p.kappa))
    assert e <= OP_TOL, e
    # gather and scatter alone, through the C entry points
    from cosmomap2_amd import _hip
    s = np.random.default_rng(12).standard_normal(NT)
    sd, c = to_dev(cm, s), cm.D.empty(p.pos.size)
    _hip.call("cm2_gaps_gather", p.gf._gaps.h, cm.D.ptr(sd), cm.D.ptr(c), cm.D.stream())
    np.testing.assert_array_equal(to_host(cm, c), s[p.pos])
    yd = to_dev(cm, y)
    _hip.call("cm2_gaps_scatter", p.gf._gaps.h, cm.D.ptr(yd), cm.D.ptr(sd), cm.D.stream())
    s[p.pos] = y
    np.testing.assert_array_equal(to_host(cm, sd), s)


# ---------------------------------------------------------------------------- mean fill ------
@pytest.mark.parametrize("lam", LAMS)
def test_mean_fill_equals_the_dense_solve(cm, lam):
    """Relative error <= kappa_2(Q_GG) x relative residual, the residual being cg's stopping rule (rtol) plus
    the operator's rounding bound (1e-12)."""
    p = problem(cm, lam)
    filled, info = p.gf.fill(to_dev(cm, p.d), rtol=RTOL, maxiter=500)
    assert filled.is_cuda and filled.dtype == cm.torch.float64
    x = to_host(cm, filled)
    err = rel_l2(x[p.pos], p.x_ref)
    res = np.linalg.norm(p.Q @ x[p.pos] + p.qgv_d) / np.linalg.norm(p.qgv_d)
    print("\nlam %d: ng %d, kappa_2 %.4g, %d iterations, cg residual %.3g, gap error %.3g (bound %.3g), dense "
          "residual %.3g (bound %.3g)" % (lam, p.pos.size, p.kappa, p.gf.iterations, p.gf.relative_residual, err,
                                          p.bound, res, RTOL + p.kappa * OP_TOL))
    assert info == 0
    assert 0 < p.gf.iterations <= 500
    np.testing.assert_array_equal(x[~p.mask], p.d[~p.mask])
    assert err <= p.bound, (err, p.bound)
    assert res <= RTOL + p.kappa * OP_TOL, res
    assert p.gf.relative_residual <= RTOL + p.kappa * OP_TOL
    # NumPy in, NumPy out; a given out; in place
    xh, info = p.gf.fill(p.d, rtol=RTOL, maxiter=500)
    assert isinstance(xh, np.ndarray) and info == 0
    np.testing.assert_array_equal(xh, x)
    out = np.zeros(NT)
    assert p.gf.fill(p.d, rtol=RTOL, maxiter=500, out=out)[0] is out
    np.testing.assert_array_equal(out, x)
    dd = to_dev(cm, p.d)
    assert p.gf.fill(dd, rtol=RTOL, maxiter=500, out=dd)[0] is dd
    np.testing.assert_array_equal(to_host(cm, dd), x)


@pytest.mark.parametrize("lam", LAMS)
def test_flagged_values_never_reach_the_output(cm, lam):
    p = problem(cm, lam)
    outs = []
    for junk in (np.nan, 1e30):
        d = p.d.copy()
        d[p.mask] = junk
        x, info = p.gf.fill(d, rtol=RTOL, maxiter=500)
        assert info == 0 and np.all(np.isfinite(x))
        outs.append(x)
    np.testing.assert_array_equal(outs[0], outs[1])
    lin = [cm.gf.fill_gaps_linear(np.where(p.mask, junk, p.d), p.mask, SIZES) for junk in (np.nan, 1e30)]
    assert np.all(np.isfinite(lin[0]))
    np.testing.assert_array_equal(lin[0], lin[1])


# ----------------------------------------------------------------- constrained realisation ------
@pytest.mark.parametrize("lam", LAMS)
def test_constrained_realisation(cm, lam):
    p = problem(cm, lam)
    sim = cm.ns.NoiseSimulator(SIZES, p.psd, lam, seed=7)
    n = to_host(cm, sim.draw(3))
    y_ref = np.linalg.solve(p.Q, ninv_ref(p.bands, SIZES, np.where(p.mask, 0.0, n - p.d))[p.pos])
    x, info = p.gf.fill(p.d, sim=sim, realization=3, rtol=RTOL, maxiter=500)
    err = np.linalg.norm(x[p.pos] - (n[p.pos] + y_ref)) / np.linalg.norm(y_ref)
    print("\nlam %d: constrained realisation, %d iterations, gap error %.3g of |y| (bound %.3g)"
          % (lam, p.gf.iterations, err, p.bound))
    assert info == 0
    np.testing.assert_array_equal(x[~p.mask], p.d[~p.mask])
    assert err <= p.bound, (err, p.bound)
    again, _ = p.gf.fill(p.d, sim=sim, realization=3, rtol=RTOL, maxiter=500)
    np.testing.assert_array_equal(again, x)
    other, _ = p.gf.fill(p.d, sim=sim, realization=4, rtol=RTOL, maxiter=500)
    assert not np.any(other[p.pos] == x[p.pos])
    np.testing.assert_array_equal(other[~p.mask], x[~p.mask])


def test_a_shard_fills_its_block_like_the_whole(cm):
    """Block 1 alone, with its own GapFiller and a simulator made with first_block = 1, against the whole-stream
    fill on that block: within the bound of the mean fill, not bit-equal -- cg's scalars (rho, p.q, the stop
    test) span all the blocks a rank holds, so the iterates of a block depend on its neighbours."""
    lam = 64
    p = problem(cm, lam)
    sim = cm.ns.NoiseSimulator(SIZES, p.psd, lam, seed=7)
    whole, info = p.gf.fill(p.d, sim=sim, realization=3, rtol=RTOL, maxiter=500)
    assert info == 0
    N1 = cm.I.BlockLO(SIZES[1:], [p.bands[1]], offdiag=True)
    g1 = cm.gf.GapFiller(p.pix[N0:], N1)
    sim1 = cm.ns.NoiseSimulator(SIZES[1:], p.psd[1:], lam, seed=7, first_block=1)
    part, info = g1.fill(p.d[N0:], sim=sim1, realization=3, rtol=RTOL, maxiter=500)
    assert info == 0
    m1 = p.mask[N0:]
    assert g1.ng == m1.sum() == 10 + 1 + 3 + 7
    np.testing.assert_array_equal(part[~m1], p.d[N0:][~m1])
    e = rel_l2(part[m1], whole[N0:][m1])
    print("\nblock 1 alone against the whole stream: rel l2 %.3g (bound %.3g)" % (e, p.bound))
    assert e <= p.bound, (e, p.bound)


# -------------------------------------------------------------------------- linear fill ------
@pytest.mark.parametrize("lam,nedge", [(8, 32), (8, 5), (64, 32)])
def test_linear_fill_equals_the_restatement(cm, lam, nedge):
    mask = layout(lam)
    d = np.random.default_rng(5).standard_normal(NT) + 3.0 * np.sin(np.arange(NT) / 700.0)
    ref = linear_ref(d, mask, SIZES, nedge)
    for flags in (mask, np.where(mask, -1, 7).astype(np.int32)):
        out = cm.gf.fill_gaps_linear(d, flags, SIZES, nedge=nedge)
        assert isinstance(out, np.ndarray)
        np.testing.assert_array_equal(out[~mask], d[~mask])
        assert np.array_equal(out.view(np.int64), ref.view(np.int64)), int((out.view(np.int64) != ref.view(np.int64)).sum())
    # a run at the stream's start: constant from the right
    assert abs(out[0] - np.mean(d[1:1 + nedge])) <= 1e-14
    # a run at a block's end (and the stream's): constant from the left
    for lo, hi in ((N0 - 10, N0), (NT - 7, NT)):
        assert np.all(out[lo:hi] == out[lo])
        assert abs(out[lo] - np.mean(d[lo - nedge:lo])) <= 1e-14
    # the second half of the straddling run starts its block: constant from the right, its own level
    assert np.all(out[N0:N0 + 10] == out[N0]) and abs(out[N0] - np.mean(d[N0 + 10:N0 + 10 + nedge])) <= 1e-14
    assert out[N0] != out[N0 - 1]
    # an interior run is a line from L to R
    k = np.arange(20)
    L, R = np.mean(d[12280 - nedge:12280]), np.mean(d[12300:12300 + nedge])
    assert np.max(np.abs(out[12280:12300] - (L + (R - L) * (k + 1) / 21.0))) <= 1e-13
    # tensors, a kept out, in place
    dd = to_dev(cm, d)
    t = cm.gf.fill_gaps_linear(dd, cm.D.to_dev(mask), SIZES, nedge=nedge)
    assert t.is_cuda
    np.testing.assert_array_equal(to_host(cm, t), out)
    assert cm.gf.fill_gaps_linear(dd, mask, SIZES, nedge=nedge, out=dd) is dd
    np.testing.assert_array_equal(to_host(cm, dd), out)


def test_linear_fill_of_a_wholly_flagged_block(cm):
    mask = layout(8)
    mask[N0:] = True
    d = np.random.default_rng(6).standard_normal(NT) + 2.0
    out = cm.gf.fill_gaps_linear(d, mask, SIZES)
    np.testing.assert_array_equal(out[N0:], np.zeros(SIZES[1]))
    np.testing.assert_array_equal(out[~mask], d[~mask])
    assert np.array_equal(out.view(np.int64), linear_ref(d, mask, SIZES, 32).view(np.int64))
    # the constrained fill gives such a block the simulator's draw, zeros without one
    p = problem(cm, 8)
    g = cm.gf.GapFiller(mask, p.N)
    x, info = g.fill(d, rtol=RTOL, maxiter=500)
    assert info == 0
    np.testing.assert_array_equal(x[N0:], np.zeros(SIZES[1]))
    sim = cm.ns.NoiseSimulator(SIZES, p.psd, 8, seed=7)
    x, info = g.fill(d, sim=sim, realization=2, rtol=RTOL, maxiter=500)
    assert info == 0
    np.testing.assert_array_equal(x[N0:], to_host(cm, sim.draw(2))[N0:])


# ------------------------------------------------------------------------------ no gaps ------
def test_a_stream_without_gaps_comes_back_as_it_is(cm):
    p = problem(cm, 64)
    g = cm.gf.GapFiller(np.zeros(NT, dtype=np.int32), p.N)
    assert g.ng == 0 and g.info()["runs"] == 0
    pos, runs = g.index()
    assert pos.size == 0 and runs.shape == (0, 3)
    x, info = g.fill(p.d)
    np.testing.assert_array_equal(x, p.d)
    assert info == 0 and g.iterations == 0 and g.relative_residual == 0.0
    dd = to_dev(cm, p.d)
    t, info = g.fill(dd, sim=cm.ns.NoiseSimulator(SIZES, p.psd, 64, seed=7))
    assert info == 0 and t is not dd and g.iterations == 0
    np.testing.assert_array_equal(to_host(cm, t), p.d)
    np.testing.assert_array_equal(cm.gf.fill_gaps_linear(p.d, np.zeros(NT, dtype=bool), SIZES), p.d)


# ---------------------------------------------------------------------------- allocation ------
def test_the_solve_allocates_nothing_of_tod_size(cm):
    t = cm.torch
    p = problem(cm, 64)
    sim = cm.ns.NoiseSimulator(SIZES, p.psd, 64, seed=7)
    d, out = to_dev(cm, p.d), cm.D.empty(NT)
    p.gf.fill(d, sim=sim, realization=1, rtol=RTOL, maxiter=500, out=out)        # warm: the kept draw exists
    # operators of earlier tests that sit in reference cycles free their library memory when Python's cyclic
    # collector finds them: that happens here, not at some allocation count inside the window measured below
    gc.collect()
    seen = []

    def between_iterations(yk):
        if not seen:
            t.cuda.synchronize()
            t.cuda.reset_peak_memory_stats()
            seen.append((cm.D.memory_info(), t.cuda.memory_allocated()))
        seen.append((cm.D.memory_info(), t.cuda.max_memory_allocated()))

    _, info = p.gf.fill(d, sim=sim, realization=1, rtol=RTOL, maxiter=500, out=out, callback=between_iterations)
    assert info == 0 and len(seen) == p.gf.iterations + 1 >= 3
    (lib0, torch0), (lib1, peak) = seen[0], seen[-1]
    assert lib1["live_bytes"] == lib0["live_bytes"] and lib1["driver_allocations"] == lib0["driver_allocations"]
    assert peak - torch0 < 8 * NT, (peak, torch0)


# --------------------------------------------------------------------------- end to end ------
def test_filled_stream_gives_the_schur_complement_right_hand_side(cm):
    """nside 16, IQU, lambda = 64.  d = P m + noise with 1e3 written into every flagged sample.  P^T N^-1 d_filled
    against P^T [(Q_VV - Q_VG Q_GG^-1 Q_GV) d_V] formed densely: the two differ by P^T N^-1 (x_G - x_ref) on the
    gaps, so |difference|_2 <= |P^T|_2 |N^-1|_2 bound |x_ref|_2 with the mean fill's bound, |N^-1|_2 <= a_0 +
    2 sum |a_j| and |P^T|_2 <= sqrt(2 x most hits of a pixel) (a row of P is (1, cos, sin)).  Without the fill
    the flagged values leak into the map: more than 100 times that bound."""
    lam, npix = 64, 12 * 16 * 16
    p = problem(cm, lam)
    rng = np.random.default_rng(16)
    pairs = rng.integers(0, npix, NT).astype(np.int32)
    pairs[p.mask] = -1
    phi = rng.uniform(0, np.pi, NT)
    ces = cm.U.ProcessTimeSamples(pairs, npix, pol=3, phi=phi)
    n = ces.get_new_pixel[0]
    P = cm.I.SparseLO(n, NT, pairs, pol=3, angle_processed=ces)
    mask = pairs < 0                                         # the layout, plus what the pixel cuts flagged
    assert np.all(mask[p.mask])
    m_sky = rng.standard_normal(3 * n) * np.tile([10.0, 1.0, 1.0], n)
    d = P * m_sky + rng.standard_normal(NT)
    d[mask] = 1e3
    pos = np.flatnonzero(mask)
    Q = qgg_ref(p.bands, SIZES, pos)
    kappa = np.linalg.cond(Q)
    x_ref = -np.linalg.solve(Q, ninv_ref(p.bands, SIZES, np.where(mask, 0.0, d))[pos])
    d_ref = d.copy()
    d_ref[pos] = x_ref
    rhs_ref = P.T * ninv_ref(p.bands, SIZES, d_ref)
    g = cm.gf.GapFiller(pairs, p.N)
    filled, info = g.fill(d, rtol=RTOL, maxiter=500)
    assert info == 0
    np.testing.assert_array_equal(filled[~mask], d[~mask])
    rhs = P.T * p.N * filled
    norm_n = max(abs(a[0]) + 2.0 * np.abs(a[1:]).sum() for a in p.bands)
    norm_pt = np.sqrt(2.0 * np.bincount(pairs[~mask]).max())
    bound = norm_pt * norm_n * kappa * (RTOL + OP_TOL) * np.linalg.norm(x_ref)
    err = np.linalg.norm(rhs - rhs_ref)
    leak = np.linalg.norm(P.T * p.N * d - rhs_ref)
    print("\nend to end: |rhs - dense Schur rhs| %.3g (bound %.3g, |rhs| %.3g); without the fill %.3g"
          % (err, bound, np.linalg.norm(rhs_ref), leak))
    assert err <= bound, (err, bound)
    assert leak > 100.0 * bound, (leak, bound)
