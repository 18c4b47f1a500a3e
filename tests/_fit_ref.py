"""
What the references of the fit filters share (tests/_hwpss_ref.py, tests/_cmode_ref.py): the one NumPy restatement of
csrc/cm2_fit.h -- the row-by-row Cholesky factor with the pivot rule and the two triangular solves, batched over the
units, in the precision asked for --, the rule of an edge list, and the acceptance of a result element by element.
Plain NumPy, no GPU.  tests/test_fit_header_cpu.py compares the header, compiled for the host, with it bit for bit.
"""
from types import SimpleNamespace

import numpy as np

import _vector_ref as V

_ld, bits = V._ld, V.bits

TAU = 2.0 ** -10                     # CM2_HWPSS_TAU = CM2_CMODE_TAU
NEAR = 2.0 ** -20                    # a pivot ratio within TAU (1 +- NEAR) is reported as near the threshold


# ------------------------------------------------------------------ edge lists ----
def edges(N, parts):
    """the edges of the parts of N items, as hwpss_plan and cmode_groups of cosmomap2_amd.interfaces define them
    (restated: a reference must not import the code under test); nothing is checked"""
    N = int(N)
    if parts is None:
        return np.array([0, N], dtype=np.int64)
    if np.ndim(parts) == 0:
        return np.append(np.arange(0, N, int(parts), dtype=np.int64), N)
    return np.asarray(parts, dtype=np.int64)


def edges_ok(e, N):
    """0 = e_0 < e_1 < ... < e_n = N, which allows no more than N parts"""
    return len(e) - 1 <= N and e[0] == 0 and e[-1] == N and all(b > a for a, b in zip(e[:-1], e[1:]))


# -------------------------------------- Cholesky with the pivot rule, over the units ----
def cholesky(G, dtype):
    """Row-by-row factor of G[n, K, K] (its lower triangle) in `dtype`, the operation order written at the top of
    cm2_fit.h.  -> SimpleNamespace(L [n, K, K], failed [n]: a pivot p_j <= TAU G_jj was met, ratio [n]: the
    smallest p_j / G_jj tested -- the factorisation stops at the first failed pivot --, near [n]: a tested ratio
    lies within TAU (1 +- NEAR)).  What follows a failed pivot in L is not meaningful."""
    A = np.array(G, dtype=dtype)
    n, K = A.shape[0], A.shape[1]
    failed, near = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    worst = np.full(n, np.inf)
    tau = dtype(TAU)
    with np.errstate(all="ignore"):
        for j in range(K):
            gjj = A[:, j, j].copy()
            p = gjj.copy()
            for k in range(j):
                p = p - A[:, j, k] * A[:, j, k]
            ratio = np.where(gjj != 0, p / np.where(gjj != 0, gjj, 1), 0)
            ratio = np.where(np.isnan(ratio), 0, ratio)
            alive = ~failed
            worst = np.where(alive, np.minimum(worst, ratio.astype(np.float64)), worst)
            near |= alive & (np.abs(ratio - tau) <= tau * dtype(NEAR))
            failed |= alive & ~(p > tau * gjj)
            ljj = np.sqrt(p)
            A[:, j, j] = ljj
            for i in range(j + 1, K):
                t = A[:, i, j].copy()
                for k in range(j):
                    t = t - A[:, i, k] * A[:, j, k]
                A[:, i, j] = t / ljj
    return SimpleNamespace(L=A, failed=failed, ratio=worst, near=near)


def solve(L, b):
    """the two triangular solves of L[n, K, K], b[n, K], the known terms subtracted in ascending index order"""
    K = L.shape[1]
    y = np.array(b, dtype=L.dtype)
    with np.errstate(all="ignore"):
        for i in range(K):
            a = y[:, i].copy()
            for k in range(i):
                a = a - L[:, i, k] * y[:, k]
            y[:, i] = a / L[:, i, i]
        for i in range(K - 1, -1, -1):
            a = y[:, i].copy()
            for k in range(i + 1, K):
                a = a - L[:, k, i] * y[:, k]
            y[:, i] = a / L[:, i, i]
    return y


# ----------------------------------------------------------------- acceptance ----
def excess(got, ref, S, c):
    return V.excess(got, ref, _ld(S).reshape(-1) * _ld(c).reshape(-1), 1)


def assert_accepted(got, f64, ref, S, c, what=""):
    """element by element: bit-equal to the restatement, or within c 2^-53 S of the reference"""
    got, f64 = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(f64, dtype=np.float64).reshape(-1)
    same = bits(got) == bits(f64)
    ref, S, c = _ld(ref).reshape(-1), _ld(S).reshape(-1), _ld(c).reshape(-1)
    if same.all():
        return 0.0
    e = excess(got[~same], ref[~same], S[~same], c[~same])
    assert e <= 1.0, "%s: |got - ref| is %.3g x the bound c 2^-53 S" % (what, e)
    return e
