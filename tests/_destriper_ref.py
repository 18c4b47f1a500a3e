"""
Destriping restated in NumPy / SciPy for test_destriper_cpu.py and test_gpu_destriper.py.  Nothing here imports the
package under test.

Baselines.  Noise blocks [o_b, o_b + n_b); baseline_length L cuts block b into K_b = ceil(n_b / L) baselines
[o_b + k L, min(o_b + (k + 1) L, o_b + n_b)), global index j = sum_{b' < b} K_b' + k, na = sum K_b.
Weights.  A sample is valid when pix >= 0; w_t = w_b on the valid samples, 0 on the flagged ones; nvalid_j counts the
valid samples of baseline j, wsum_j = w_b nvalid_j.
Operators.  (F a)_t = a_j(t) on the valid samples, 0 on the flagged ones; (F^T y)_j = sum of y_t over the valid t of j.
System.  M = (P^T W P)^-1 per pixel, optional symmetric prior C on na values:

    A a = wsum o a - F^T W P M P^T W F a (+ C a)        b = F^T W (d0 - P M P^T W d0),  d0 = d on valid, 0 on flagged
    m   = M P^T W (d0 - F a)

the Schur complement of [P F]^T W [P F] z = [P F]^T W d0 with C added to the a block.  A baseline with nvalid_j = 0
has, without a prior, the identity as its row and column and b_j = 0.
"""
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from _gap_aware_ref import mbd_dense, pointing

WIN = 8192

# ------------------------------------------------------------------------------- the layouts ------
NT, SIZES, WEIGHTS = 4 * WIN + 1234, (14000, 20002), (1.0, 2.5)
LENGTHS = (37, 1000, 10000)


def common_flags():
    m = np.zeros(NT, dtype=bool)
    for s in range(123, NT, 400):
        m[s:s + 40] = True                                   # 40 samples from every 400th
    m[3 * WIN:4 * WIN] = True                                # all of window 3
    m[13990:14010] = True                                    # across the block boundary
    return m


def edge_flags(nt):
    m = np.zeros(nt, dtype=bool)
    for s in range(57, nt, 300):
        m[s:s + 25] = True
    return m


# name -> (nt, sizes, weights, L, flags)
LAYOUTS = {
    "common37": (NT, SIZES, WEIGHTS, 37, common_flags),
    "common1000": (NT, SIZES, WEIGHTS, 1000, common_flags),
    "common10000": (NT, SIZES, WEIGHTS, 10000, common_flags),
    "short": (5000, (3000, 2000), (1.0, 2.5), 64, lambda: edge_flags(5000)),             # below one window
    "windows": (32768, (16384, 16384), (1.0, 2.5), 8192, lambda: edge_flags(32768)),    # baselines = windows
    "every_sample": (9000, (4000, 5000), (1.0, 2.5), 1, lambda: edge_flags(9000)),
    "one_per_block": (9000, (4000, 5000), (1.0, 2.5), 6000, lambda: edge_flags(9000)),
    "no_flags": (NT, SIZES, None, 1000, lambda: np.zeros(NT, dtype=bool)),
}


# ------------------------------------------------------------------------------ the baselines ------
def baselines(sizes, L):
    """per_block [nb], start [na], end [na], block [na], j_of_t [nt]."""
    per_block, start, end, block = [], [], [], []
    o = 0
    for b, n in enumerate(sizes):
        K = -(-n // L)
        per_block.append(K)
        for k in range(K):
            start.append(o + k * L)
            end.append(min(o + (k + 1) * L, o + n))
            block.append(b)
        o += n
    start, end, block = np.array(start), np.array(end), np.array(block)
    j_of_t = np.repeat(np.arange(start.size), end - start)
    assert j_of_t.size == o
    return SimpleNamespace(per_block=per_block, start=start, end=end, block=block, j_of_t=j_of_t, na=start.size)


def window_baselines(B, nt, w):
    """(first, last) baseline that meets window w."""
    return int(B.j_of_t[w * WIN]), int(B.j_of_t[min((w + 1) * WIN, nt) - 1])


def segment_target(start, end, t0):
    """0: the baseline lies in the window starting at t0, 1: it began before it (head slot), 2: it began in it and ends
    after it (tail slot)."""
    if start < t0:
        return 1
    if end > t0 + WIN:
        return 2
    return 0


def counts(B, valid, weights):
    nvalid = np.bincount(B.j_of_t[valid], minlength=B.na).astype(np.int64)
    w = np.ones(len(B.per_block)) if weights is None else np.asarray(weights, dtype=np.float64)
    return nvalid, w[B.block] * nvalid


def f_matrix(B, valid):
    t = np.flatnonzero(valid)
    return sp.csr_matrix((np.ones(t.size), (t, B.j_of_t[t])), shape=(valid.size, B.na))


def sample_weights(sizes, weights, valid):
    w = np.ones(len(sizes)) if weights is None else np.asarray(weights, dtype=np.float64)
    return np.where(valid, np.repeat(w, sizes), 0.0)


def exact_sums(B, valid, y):
    """(F^T y)_j by math.fsum (correctly rounded), and sum |y_t| over the same samples."""
    s, sabs = np.zeros(B.na), np.zeros(B.na)
    for j in range(B.na):
        seg = y[B.start[j]:B.end[j]][valid[B.start[j]:B.end[j]]]
        s[j] = math.fsum(seg)
        sabs[j] = math.fsum(np.abs(seg))
    return s, sabs


# ---------------------------------------------------------------------------------- the prior ------
PRIOR_BAND = np.array([0.5] + [-0.15 * 0.6 ** k for k in range(1, 8)])


def prior_dense(per_block, band=PRIOR_BAND):
    blocks = []
    for K in per_block:
        k = min(len(band), K)
        offs = list(range(-(k - 1), k))
        blocks.append(sp.diags([np.full(K - abs(o), band[abs(o)]) for o in offs], offs, shape=(K, K)))
    return sp.block_diag(blocks).toarray()


# --------------------------------------------------------------------------------- the system ------
def scan(nt, npix, mask, seed):
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, npix, nt).astype(np.int32)
    phi = rng.uniform(0.0, np.pi, nt)
    pix[mask] = -1
    return pix, phi


def system(sizes, weights, L, pix, phi, npix, pol, d, prior=False):
    """Everything dense about one case."""
    valid = pix >= 0
    B = baselines(sizes, L)
    nvalid, wsum = counts(B, valid, weights)
    w = sample_weights(sizes, weights, valid)
    P = pointing(pix, phi, npix, pol)
    F = f_matrix(B, valid)
    W = sp.diags(w)
    M = mbd_dense(P, w, npix, pol)
    PtWF = (P.T @ W @ F).toarray()
    A = np.diag(wsum) - PtWF.T @ M @ PtWF
    A = 0.5 * (A + A.T)
    C = prior_dense(B.per_block) if prior else None
    empty = nvalid == 0
    if prior:
        A = A + C
    else:
        A[empty, empty] = 1.0
    d0 = np.where(valid, d, 0.0)
    PtWd = P.T @ (w * d0)
    b = F.T @ (w * (d0 - P @ (M @ PtWd)))
    c0 = np.repeat([PRIOR_BAND[0]] * len(sizes), B.per_block) if prior else 0.0
    s = wsum + c0
    jac = np.where(s != 0, 1.0 / np.where(s != 0, s, 1.0), 1.0)
    return SimpleNamespace(A=A, b=b, jac=jac, P=P, F=F, W=W, w=w, M=M, C=C, d0=d0, B=B, nvalid=nvalid, wsum=wsum,
                           empty=empty, valid=valid, nmap=pol * npix)


def map_of(s, a):
    return s.M @ (s.P.T @ (s.w * (s.d0 - s.F @ a)))


def _joint(s):
    PF = sp.hstack([s.P, s.F], format="csr")
    return PF, (PF.T @ s.W @ PF).toarray(), PF.T @ (s.w * s.d0)


def joint_solve(s):
    """(m, a) of the joint normal equations [P F]^T W [P F] z = [P F]^T W d0 with the prior on the a block."""
    _, J, rhs = _joint(s)
    n = s.nmap
    J[n:, n:] += s.C
    z = np.linalg.solve(J, rhs)
    return z[:n], z[n:]


def lstsq_residual(s):
    """(d0 - F a - P m on the valid samples, m, a) at the minimum-norm least-squares solution of the joint normal
    equations without a prior (they are singular: the I monopole, the empty baselines)."""
    PF, J, rhs = _joint(s)
    z = np.linalg.lstsq(J, rhs, rcond=None)[0]
    return (s.d0 - PF @ z)[s.valid], z[:s.nmap], z[s.nmap:]
