"""
The gap-aware GLS solve without a GPU: the algebra the operator rests on, restated densely in NumPy
(_gap_aware_ref.py), the window table of the tiled path, and the argument checks of
cosmomap2_amd.interfaces.gapaware, which come before the device is touched.

The dense case: nt = 2400 in blocks of 1000 and 1400 samples with the bands of S = sigma^2 (1 + (f_knee / f)^1.5),
(sigma, f_knee) = (1, 0.1) and (2, 0.2), 24 pixels, 10 % of the samples flagged in runs of 40 every 400 plus a run
across the block boundary and the two ends of the stream.
"""
import re

import numpy as np
import pytest

import _gap_aware_ref as R

NT, SIZES, NPIX = 2400, [1000, 1400], 24
SPECS = [(1.0, 0.1), (2.0, 0.2)]


def dense_mask():
    m = np.zeros(NT, dtype=bool)
    for s in range(100, NT - 100, 400):
        m[s:s + 40] = True
    m[995:1005] = True
    m[0:3] = True
    m[NT - 4:] = True
    return m


_cases = {}


def dense_case(lam, pol):
    if (lam, pol) not in _cases:
        from types import SimpleNamespace
        c = SimpleNamespace(bands=R.bands(lam, SPECS), mask=dense_mask())
        c.pix, c.phi = R.scan(NT, NPIX, c.mask, 5)
        rng = np.random.default_rng(7)
        c.m = rng.standard_normal(pol * NPIX)
        c.P = R.pointing(c.pix, c.phi, NPIX, pol)
        c.d = c.P @ c.m + rng.standard_normal(NT)
        c.d[c.mask] = 1e3                                    # what a flagged sample holds must not matter
        c.sys = R.system(c.bands, SIZES, c.pix, c.phi, NPIX, pol, c.d)
        c.S, c.valid = R.schur_dense(c.sys["Q"], c.sys["pos"])
        c.Pv = c.P.toarray()[c.valid]
        _cases[(lam, pol)] = c
    return _cases[(lam, pol)]


@pytest.mark.parametrize("pol", [1, 3])
@pytest.mark.parametrize("lam", [8, 64])
def test_extended_system_gives_the_schur_complement_map(lam, pol):
    """(i) the map part of A_e^-1 b_e is (P^T S P)^-1 P^T S d_V, and the gap part is Q_GG^-1 Q_GV (d_V - P m)."""
    c = dense_case(lam, pol)
    z = np.linalg.solve(c.sys["A"], c.sys["b"])
    m_s = np.linalg.solve(c.Pv.T @ c.S @ c.Pv, c.Pv.T @ c.S @ c.d[c.valid])
    n = c.sys["nmap"]
    e = np.linalg.norm(z[:n] - m_s) / np.linalg.norm(m_s)
    print("\nlam %d pol %d: extended against Schur map, rel l2 %.3g" % (lam, pol, e))
    assert e <= 1e-12, e
    assert np.linalg.norm(R.schur_map(c.sys) - m_s) / np.linalg.norm(m_s) <= 1e-12
    Qd, pos = c.sys["Q"].toarray(), c.sys["pos"]
    g = np.linalg.solve(Qd[np.ix_(pos, pos)], Qd[np.ix_(pos, c.valid)] @ (c.d[c.valid] - c.Pv @ z[:n]))
    assert np.linalg.norm(z[n:] - g) / np.linalg.norm(g) <= 1e-10
    assert np.all(np.linalg.eigvalsh(c.sys["A"]) > 0)


@pytest.mark.parametrize("pol", [1, 3])
@pytest.mark.parametrize("lam", [8, 64])
def test_the_zero_filled_operator_under_the_schur_right_hand_side_is_biased(lam, pol):
    """(ii) the recipe the operator replaces: (P^T Q_VV P)^-1 P^T S P m is not m, before any noise."""
    c = dense_case(lam, pol)
    Qvv = c.sys["Q"].toarray()[np.ix_(c.valid, c.valid)]
    biased = np.linalg.solve(c.Pv.T @ Qvv @ c.Pv, c.Pv.T @ c.S @ (c.Pv @ c.m))
    bias = np.linalg.norm(biased - c.m) / np.linalg.norm(c.m)
    exact = np.linalg.solve(c.Pv.T @ c.S @ c.Pv, c.Pv.T @ c.S @ (c.Pv @ c.m))
    print("\nlam %d pol %d: bias of the zero-filled operator %.3g of |m|" % (lam, pol, bias))
    assert bias > 1e-3, bias
    assert np.linalg.norm(exact - c.m) / np.linalg.norm(c.m) <= 1e-12


# ------------------------------------------------------------------------- the window table ------
@pytest.mark.parametrize("lam,whole,counts", [(64, True, [177, 37, 0, 8192, 204]), (64, False, [177, 37, 0, 0, 204]),
                                              (8, True, [65, 37, 0, 8192, 204]), (2049, False, [344, 37, 0, 0, 204])])
def test_window_table_of_the_five_window_layout(lam, whole, counts):
    """(iv) c_w = lower_bound of w * 8192 in the ascending positions: a window without a flagged sample, a wholly
    flagged one, a partial last window."""
    pos = np.flatnonzero(R.flags(lam, whole))
    cw = R.window_table(pos, R.NT)
    assert cw.size == 6 and cw[0] == 0 and cw[-1] == pos.size == sum(counts)
    assert np.diff(cw.astype(np.int64)).tolist() == counts
    for w in range(5):
        own = pos[cw[w]:cw[w + 1]]
        assert np.all((own >= w * R.WIN) & (own < min((w + 1) * R.WIN, R.NT)))
    if whole:
        np.testing.assert_array_equal(pos[cw[3]:cw[4]], np.arange(3 * R.WIN, 4 * R.WIN))
    assert R.NT - 4 * R.WIN == 1234 and pos[-1] == R.NT - 1


def test_window_table_edges():
    assert R.window_table(np.array([], dtype=np.int64), R.NT).tolist() == [0] * 6
    assert R.window_table(np.arange(R.NT), R.NT).tolist() == [0, 8192, 16384, 24576, 32768, R.NT]
    assert R.window_table(np.array([8191, 8192]), 2 * R.WIN).tolist() == [0, 1, 2]
    assert R.window_table(np.flatnonzero(R.flags_small(8)), R.NT_SMALL).tolist() == [0, R.flags_small(8).sum()]


# -------------------------------------------------------------------------- argument checks ------
BANDS = [np.array([2.0, -0.5, 0.1]), np.array([1.0, -0.2, 0.05])]
ASIZES = [1000, 2000]
ANT = sum(ASIZES)


@pytest.fixture
def ga():
    from cosmomap2_amd.interfaces import gapaware
    return gapaware


@pytest.fixture
def no_gpu(monkeypatch):
    """As on a machine without a GPU, whether or not this one has one."""
    from cosmomap2_amd import device as D
    monkeypatch.setattr(D, "gpu_available", lambda: False)


def block_lo(sizes=ASIZES, t=BANDS, offdiag=True):
    """A BlockLO as its constructor leaves it on the host side (the constructor itself needs the GPU)."""
    from cosmomap2_amd.interfaces.linearoperators import BlockLO
    N = BlockLO.__new__(BlockLO)
    N._BlockLO__isoffdiag = offdiag
    N.blocksize, N.covnoise, N._sizes, N._nt = sizes, t, list(sizes), sum(sizes)
    return N


def sparse_lo(nt=ANT, npix=48, pol=3):
    """A SparseLO as far as the argument checks look at it."""
    from cosmomap2_amd.interfaces.linearoperators import SparseLO
    P = SparseLO.__new__(SparseLO)
    P.nrows, P.ncols, P.pol = nt, npix, pol
    return P


def test_exported_from_interfaces():
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd.interfaces import gapaware
    for name in ("GapAwareNormalLO", "solve_gls_with_gaps"):
        assert getattr(I, name) is getattr(gapaware, name)


def test_operators_of_the_wrong_kind(ga, no_gpu):
    """(iii) a diagonal N, something that is no BlockLO, a P that is no SparseLO, an nt mismatch, a_0 <= 0."""
    d = np.zeros(ANT)
    for N in (block_lo(t=[1.0, 2.0], offdiag=False), None, np.eye(3)):
        with pytest.raises(ValueError, match="Toeplitz BlockLO"):
            ga.GapAwareNormalLO(sparse_lo(), N)
        with pytest.raises(ValueError, match="Toeplitz BlockLO"):
            ga.solve_gls_with_gaps(sparse_lo(), N, d)
    for P in (None, np.eye(3), block_lo()):
        with pytest.raises(ValueError, match="SparseLO"):
            ga.GapAwareNormalLO(P, block_lo())
    for nt in (ANT - 1, ANT + 1):
        with pytest.raises(ValueError, match="samples"):
            ga.GapAwareNormalLO(sparse_lo(nt=nt), block_lo())
        with pytest.raises(ValueError, match="samples"):
            ga.solve_gls_with_gaps(sparse_lo(nt=nt), block_lo(), np.zeros(nt))
    with pytest.raises(ValueError, match="a_0"):
        ga.GapAwareNormalLO(sparse_lo(), block_lo(t=[np.array([1.0, 0.1]), np.array([0.0, 0.1])]))


@pytest.mark.parametrize("rtol", [0.0, -1e-8, np.nan, np.inf, "x", None])
def test_rtol_not_positive(ga, no_gpu, rtol):
    with pytest.raises(ValueError, match="rtol"):
        ga.solve_gls_with_gaps(sparse_lo(), block_lo(), np.zeros(ANT), rtol=rtol)


def test_other_bad_solve_arguments(ga, no_gpu):
    P, N = sparse_lo(), block_lo()
    for d in (np.zeros(ANT - 1), np.zeros((ANT, 1)), np.zeros(ANT, dtype=complex)):
        with pytest.raises(ValueError, match="samples|TOD"):
            ga.solve_gls_with_gaps(P, N, d)
    for maxiter in (0, -3, 2.5, "10"):
        with pytest.raises(ValueError, match="maxiter"):
            ga.solve_gls_with_gaps(P, N, np.zeros(ANT), maxiter=maxiter)
    for x0 in (np.zeros(3 * 48 - 1), np.zeros((3 * 48, 1)), 1.0):
        with pytest.raises(ValueError, match="x0"):
            ga.solve_gls_with_gaps(P, N, np.zeros(ANT), x0=x0)
    with pytest.raises(ValueError, match="M must"):
        ga.solve_gls_with_gaps(P, N, np.zeros(ANT), M=np.eye(5))
    with pytest.raises(ValueError, match="callback"):
        ga.solve_gls_with_gaps(P, N, np.zeros(ANT), callback=3)


def test_valid_calls_raise_hip_error_without_a_gpu(ga, no_gpu):
    from cosmomap2_amd import _hip
    for call in (lambda: ga.GapAwareNormalLO(sparse_lo(), block_lo()),
                 lambda: ga.GapAwareNormalLO(sparse_lo(pol=1), block_lo()),
                 lambda: ga.solve_gls_with_gaps(sparse_lo(), block_lo(), np.zeros(ANT)),
                 lambda: ga.solve_gls_with_gaps(sparse_lo(), block_lo(), np.zeros(ANT), rtol=1e-10, maxiter=50,
                                                x0=np.zeros(3 * 48), callback=lambda z: None)):
        with pytest.raises(_hip.HipError):
            call()


# ------------------------------------------------------------------------------ the C ABI ------
NEW = ("cm2_gaps_prepare_tiles", "cm2_gaps_window_table", "cm2_gaps_tiles_to_time", "cm2_gaps_time_to_tiles",
       "cm2_PtNP_gaps_apply")
KERNELS = ("k_gap_perm_windows<true>", "k_gap_perm_windows<false>", "k_gap_window_table", "k_gap_compare<0>",
           "k_gap_compare<1>")


def test_abi_lists_name_the_new_entry_points():
    import os
    from cosmomap2_amd import _hip, kernel_resources as KR
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "cosmomap2.h")).read()
    assert re.search(r"#define CM2_ABI_VERSION 2\b", text)
    for name in NEW:
        assert name in _hip.PROTOTYPES, name
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.PROTOTYPES[name]), name
    for name in NEW:
        assert (name in _hip.RESTARTABLE) == (name != "cm2_gaps_window_table"), name
    for kernel in KERNELS:
        assert any(re.search(p, kernel) for p in KR.NO_SPILL), kernel


def test_new_entry_points_refuse_null_arguments():
    """Their argument checks come before the first HIP call: no GPU is needed to meet them."""
    from cosmomap2_amd import _hip
    lib = _hip.load()
    assert lib.cm2_gaps_prepare_tiles(None, None, None) == _hip.ERR_ARGUMENT
    assert b"cm2_gaps_prepare_tiles" in lib.cm2_last_error()
    assert lib.cm2_gaps_tiles_to_time(None, None, None, None, None, None) == _hip.ERR_ARGUMENT
    assert lib.cm2_gaps_time_to_tiles(None, None, None, None, None, None) == _hip.ERR_ARGUMENT
    assert lib.cm2_PtNP_gaps_apply(None, None, None, None, None, None, None, None, None) == _hip.ERR_ARGUMENT
    assert b"cm2_PtNP_gaps_apply" in lib.cm2_last_error()


def test_new_kernels_use_no_scratch():
    """The resource table of the shipped objects lists the new kernels without scratch or spilled registers."""
    from cosmomap2_amd import build as B, kernel_resources as KR
    B.build(verbose=False)
    rows = {r["kernel"]: r for r in KR.load_all()}
    for kernel in KERNELS:
        assert kernel in rows, sorted(rows)
        assert rows[kernel].get("scratch_bytes_per_lane", 0) == 0, rows[kernel]
        assert rows[kernel].get("vgpr_spill", 0) == 0, rows[kernel]
    assert rows["k_gap_perm_windows<true>"]["lds_bytes"] == 8 * R.WIN
