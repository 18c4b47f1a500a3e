"""
Reference, restatement and error bound for the common-mode filter (csrc/cm2_cmode.hip), and the cases the CPU and the
GPU tests share.  Plain NumPy, no GPU, in the manner of tests/_hwpss_ref.py.

  * ``cmode_ref``: the definition of include/cosmomap2.h (f2d) in np.longdouble: per (group, sample) unit
    G = sum Phi Phi^T, b = sum Phi v over the unflagged detectors, c = G^-1 b, out = v - Phi^T c.  With it comes S,
    the same formula with every operand replaced by its absolute value and every subtraction by an addition:
        S[k, i] = |v[k, i]| + |Phi_k|^T |G^-1| sum_u |Phi_u| |v[u, i]|      (|G^-1| entry by entry),
    and Sc = |G^-1| sum_u |Phi_u| |v[u, i]| for the coefficients.  S = 0 on flagged samples and skipped units.
  * ``cmode_f64``: a float64 restatement in the kernel's stated order, vectorised over the samples with a loop over
    the detectors: G_ab and b_a from 0 over the unflagged detectors in ascending k, the row-by-row Cholesky with the
    pivot rule, the two triangular solves and the projection.  The library is built with -ffp-contract=off and
    NumPy's elementwise loops do not fuse, so this is meant to match the GPU bit for bit.

Acceptance, element by element: bit-equal to the restatement, or |got - ref| <= c 2^-53 S; exactly 0 where S = 0.

The constant c = count x HEADROOM.  ``count`` is read from the kernel source (c_count below).  No operation count
gives what the rounding of G and of its factor does to c = G^-1 b; that is measured: WORST is the largest
|cmode_f64 - cmode_ref| / (2^-53 S) over the shared cases (tests/test_cmode_cpu.py re-measures it), and HEADROOM is
8 x WORST rounded up to a power of two, the project's established headroom between NumPy and the device.  Unlike
the plate harmonics of _hwpss_ref.py, the pivot ratios p_j / G_jj of these cases fill (0, 1) continuously, so no
band around tau can be kept empty of them: the conditioning of a fitted unit enters the bound through |G^-1|, and
the CPU test asserts that every unit has the same skip decision in both precisions and that no tested ratio lies
within tau (1 +- 2^-20).
"""
import functools
from types import SimpleNamespace

import numpy as np

import _fit_ref as F
import _vector_ref as V

LD, U53, _ld = V.LD, V.U53, V._ld
bits, assert_bit_equal, pow2_at_least = V.bits, V.assert_bit_equal, V.pow2_at_least
cholesky, solve, excess, assert_accepted = F.cholesky, F.solve, F.excess, F.assert_accepted

THREADS = 256                        # kThreads of cm2_cmode_policy.h
MAX_K = 10                           # kMaxK, CM2_CMODE_MAX_K
TAU = F.TAU                          # CM2_CMODE_TAU
NEAR = F.NEAR                        # no tested pivot ratio within TAU (1 +- NEAR)
FITTED, EMPTY, FEW, PIVOT = 0, 1, 2, 3

# largest |cmode_f64 - cmode_ref| / (2^-53 S) over outputs and coefficients of the shared cases, rounded up to one
# decimal; test_cmode_cpu.py::test_restatement_against_reference_and_worst keeps it honest
WORST = 13.4
HEADROOM = pow2_at_least(8.0 * WORST)


def c_count(nd, K):
    """Roundings on the longest chain from the inputs to an output sample, from cm2_cmode.hip, for a group of nd
    detectors:
    nd             b_a: one product per detector, then nd - 1 adds (0 + p is exact)
    2 K            the two triangular solves (a subtraction chain and a division per row, chains up to K long)
    K              terms of the projection (the first product, then a product and an add per term)
    1 + 2          v - p; second-order terms and the reference's own roundings"""
    return int(nd) + 2 * K + K + 1 + 2


def c_bound(nd, K):
    return c_count(nd, K) * HEADROOM


cmode_groups = F.edges               # (ndet, groups) -> edges, as cosmomap2_amd.interfaces.cmode_groups defines them


def focalplane_modes(xy, order, groups=None):
    """the monomials x^(d-j) y^j, d = 0..order, j = 0..d, of the positions centred and scaled to [-1, 1] per group
    (restated)"""
    xy = np.asarray(xy, dtype=np.float64)
    e = cmode_groups(len(xy), groups)
    u = np.zeros_like(xy)
    for a, b in zip(e[:-1], e[1:]):
        for ax in (0, 1):
            lo, hi = xy[a:b, ax].min(), xy[a:b, ax].max()
            if hi > lo:
                u[a:b, ax] = (xy[a:b, ax] - (hi + lo) / 2.0) / ((hi - lo) / 2.0)
    cols = []
    for d in range(order + 1):
        for j in range(d + 1):
            px, py = np.ones(len(xy)), np.ones(len(xy))         # powers are repeated products: x^3 = (x x) x
            for _ in range(d - j):
                px = px * u[:, 0]
            for _ in range(j):
                py = py * u[:, 1]
            cols.append(px * py)
    return np.stack(cols, axis=1)


def blocks_per_group(ns):
    return -(-int(ns) // THREADS)


def policy_status(ns, ndet, edges, K):
    """cm2::cmode::check restated: 0 ok, 1 K, 2 sizes, 3 edges, 4 too large"""
    G = len(edges) - 1
    if K < 1 or K > MAX_K:
        return 1
    if ns < 1 or ndet < 1 or G < 1:
        return 2
    if not F.edges_ok(edges, ndet):
        return 3
    if ndet >= 1 << 31 or ndet > (1 << 46) // ns:
        return 4
    if G > ((1 << 31) - 1) // blocks_per_group(ns):
        return 4
    return 0


def classes(m, K, failed):
    return np.where(m == 0, EMPTY, np.where(m < K, FEW, np.where(failed, PIVOT, FITTED))).astype(np.uint8)


# --------------------------------------------------------------- the reference ----
def cmode_ref(pix, ndet, edges, modes, v):
    """-> SimpleNamespace(out, S [ndet ns], coeff, Sc [G, K, ns], status [G, ns] uint8, ratio, near [G, ns]) in
    np.longdouble; ratio is NaN where m < K (no pivot is tested there)"""
    modes = np.asarray(modes, dtype=np.float64)
    K, G = modes.shape[1], len(edges) - 1
    ns = len(pix) // ndet
    ok = np.asarray(pix).reshape(ndet, ns) >= 0
    Phi = _ld(modes)
    v = np.where(ok, _ld(v).reshape(ndet, ns), LD(0))           # a flagged sample's value is never read
    out, S = np.zeros((ndet, ns), dtype=LD), np.zeros((ndet, ns), dtype=LD)
    coeff, Sc = np.zeros((G, K, ns), dtype=LD), np.zeros((G, K, ns), dtype=LD)
    status = np.zeros((G, ns), dtype=np.uint8)
    ratio, near = np.full((G, ns), np.nan), np.zeros((G, ns), dtype=bool)
    with np.errstate(all="ignore"):
        for g in range(G):
            a, b = int(edges[g]), int(edges[g + 1])
            M, P = ok[a:b].astype(LD), Phi[a:b]
            m = ok[a:b].sum(axis=0)
            Gm = np.einsum("ki,ka,kb->iab", M, P, P)
            bb = np.einsum("ki,ka->ia", v[a:b], P)
            ch = cholesky(Gm, LD)
            cls = classes(m, K, ch.failed)
            fit = cls == FITTED
            status[g] = cls
            ratio[g] = np.where(m >= K, ch.ratio, np.nan)
            near[g] = ch.near & (m >= K)
            cf = solve(ch.L, bb)
            Li = np.zeros((ns, K, K), dtype=LD)                 # L^-1 by forward substitution on the unit vectors
            for j in range(K):
                e = np.zeros((ns, K), dtype=LD)
                e[:, j] = 1
                for i in range(K):
                    t = e[:, i].copy()
                    for k in range(i):
                        t = t - ch.L[:, i, k] * e[:, k]
                    e[:, i] = t / ch.L[:, i, i]
                Li[:, :, j] = e
            Ginv_abs = np.abs(np.einsum("nki,nkj->nij", Li, Li))
            sc = np.einsum("nab,nb->na", Ginv_abs, np.einsum("ki,ka->ia", np.abs(v[a:b]), np.abs(P)))
            mask = ok[a:b] & fit[None, :]
            out[a:b] = np.where(mask, v[a:b] - np.einsum("ka,ia->ki", P, cf), LD(0))
            S[a:b] = np.where(mask, np.abs(v[a:b]) + np.einsum("ka,ia->ki", np.abs(P), sc), LD(0))
            coeff[g] = np.where(fit[None, :], cf.T, LD(0))
            Sc[g] = np.where(fit[None, :], sc.T, LD(0))
    return SimpleNamespace(out=out.reshape(-1), S=S.reshape(-1), coeff=coeff, Sc=Sc, status=status, ratio=ratio,
                           near=near)


# -------------------------------------------------------------- the restatement ----
def cmode_f64(pix, ndet, edges, modes, v):
    """-> SimpleNamespace(out [ndet ns], coeff [G, K, ns], status [G, ns] uint8, ratio, near [G, ns]) in float64, in
    the order of cm2_cmode.hip"""
    Phi = np.asarray(modes, dtype=np.float64)
    K, G = Phi.shape[1], len(edges) - 1
    ns = len(pix) // ndet
    ok = np.asarray(pix).reshape(ndet, ns) >= 0
    v = np.asarray(v, dtype=np.float64).reshape(ndet, ns)
    out, coeff = np.zeros((ndet, ns)), np.zeros((G, K, ns))
    status = np.zeros((G, ns), dtype=np.uint8)
    ratio, near = np.full((G, ns), np.nan), np.zeros((G, ns), dtype=bool)
    with np.errstate(all="ignore"):
        for g in range(G):
            a, b = int(edges[g]), int(edges[g + 1])
            Gm, bb = np.zeros((ns, K, K)), np.zeros((ns, K))
            m = np.zeros(ns, dtype=np.int64)
            for k in range(a, b):                               # step 1: ascending k, unflagged only
                m += ok[k]
                for i in range(K):
                    for j in range(i + 1):
                        Gm[:, i, j] = np.where(ok[k], Gm[:, i, j] + Phi[k, i] * Phi[k, j], Gm[:, i, j])
                    bb[:, i] = np.where(ok[k], bb[:, i] + Phi[k, i] * v[k], bb[:, i])
            ch = cholesky(Gm, np.float64)                       # step 2
            cls = classes(m, K, ch.failed)
            fit = cls == FITTED
            status[g] = cls
            ratio[g] = np.where(m >= K, ch.ratio, np.nan)
            near[g] = ch.near & (m >= K)
            cf = solve(ch.L, bb)
            for k in range(a, b):                               # step 3
                p = cf[:, 0] * Phi[k, 0]
                for j in range(1, K):
                    p = p + cf[:, j] * Phi[k, j]
                out[k] = np.where(ok[k] & fit, v[k] - p, 0.0)
            coeff[g] = np.where(fit[None, :], cf.T, 0.0)
    return SimpleNamespace(out=out.reshape(-1), coeff=coeff, status=status, ratio=ratio, near=near)


# ----------------------------------------------------------------- acceptance ----
def c_samples(ndet, ns, edges, K):
    """c per sample [ndet ns]: the size of its group enters"""
    per = np.repeat([c_bound(n, K) for n in np.diff(edges)], np.diff(edges))
    return np.repeat(per, ns)


def c_coeffs(ns, edges, K):
    """c per coefficient [G, K, ns]"""
    per = np.array([c_bound(n, K) for n in np.diff(edges)])
    return np.broadcast_to(per[:, None, None], (len(per), K, ns)).copy()


# ---------------------------------------------------------------------- cases ----
NS = 773                             # three full workgroups and a part, not a multiple of 64
SEED = 7100


def jittered_grid(rng, ncols, nrows, n):
    """n <= ncols nrows positions, column by column; the detectors of a column share their x exactly (the jitter of
    x is per column), y is jittered per detector.  -> (xy [n, 2], column [n])"""
    xs = np.arange(ncols) + 0.2 * rng.uniform(-1, 1, ncols)
    col = np.arange(n) // nrows
    y = (np.arange(n) % nrows) + 0.2 * rng.uniform(-1, 1, n)
    return np.stack([xs[col], y], axis=1), col


# name: (group sizes, (columns, rows) of each group's grid, what the templates are, ns)
#   what: "ones", "gains", ("order", d) or ("user", K)
LAYOUT = {
    "ones7": ([7], [(3, 3)], "ones", NS),
    "gains7": ([7], [(3, 3)], "gains", NS),
    "order1_9": ([9], [(3, 3)], ("order", 1), NS),
    "order2_12": ([12], [(4, 3)], ("order", 2), NS),
    "order3_16": ([16], [(4, 4)], ("order", 3), NS),
    "order3_24": ([24], [(6, 4)], ("order", 3), NS),
    "groups20": ([1, 3, 4, 12], [(1, 1), (2, 2), (2, 2), (4, 3)], ("order", 1), NS),
    "user2_8": ([8], [(3, 3)], ("user", 2), NS),
    "user7_14": ([14], [(4, 4)], ("user", 7), NS),
    "ns1": ([9], [(3, 3)], ("order", 1), 1),
    "ns64": ([12], [(4, 3)], ("order", 2), 64),
}
CASES = tuple(LAYOUT)
PATTERNS = ("none", "random", "dead", "special", "nan")
FLAG_RATE = 0.30


@functools.lru_cache(maxsize=None)
def case(name):
    """the detectors, groups and templates of a case, and a stream: noise of unit variance plus 50 x the templates
    with coefficients that change from sample to sample"""
    sizes, grids, what, ns = LAYOUT[name]
    rng = np.random.default_rng(SEED + CASES.index(name))
    edges = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ndet = int(edges[-1])
    parts = [jittered_grid(rng, c, r, n) for n, (c, r) in zip(sizes, grids)]
    xy = np.concatenate([p[0] for p in parts])
    col = np.concatenate([p[1] for p in parts])
    order = None
    if what == "ones":
        modes = np.ones((ndet, 1))
    elif what == "gains":
        modes = rng.uniform(0.5, 2.0, (ndet, 1))
    elif what[0] == "order":
        order = what[1]
        modes = focalplane_modes(xy, order, edges)
    else:
        K = what[1]
        modes = rng.standard_normal((ndet, K))
        modes[:K + 1, 1] = 2.0 * modes[:K + 1, 0]       # the first K + 1 detectors alone are exactly collinear
    K = modes.shape[1]
    amp = 50.0 * rng.standard_normal((ns, K))
    v = (modes @ amp.T + rng.standard_normal((ndet, ns))).reshape(-1)
    return SimpleNamespace(name=name, ndet=ndet, ns=ns, nt=ndet * ns, edges=edges, sizes=sizes, K=K, order=order,
                           what=what, xy=xy, col=col, modes=np.ascontiguousarray(modes), v=v)


def survivors_on_few_columns(cs):
    """per group, the detectors that leave the templates collinear: for the monomials of degree <= d those of the
    first d columns (d distinct x cannot carry 1, x, ..., x^d); for user templates the first K + 1 detectors; None
    for K = 1, where no choice of detectors is collinear"""
    if cs.K == 1:
        return None
    keep = np.zeros(cs.ndet, dtype=bool)
    if cs.order is not None:
        keep[cs.col < cs.order] = True
    else:
        keep[:cs.K + 1] = True
    return keep


@functools.lru_cache(maxsize=None)
def data(name, pattern):
    """(pix, v) of a case under a flag pattern:
    none     no flags
    random   30 % of the samples, independently
    dead     one detector flagged throughout (detector 1; in "groups20" detector 9, of the group of twelve)
    special  by sample index i mod 7: 1 every detector flagged; 2 each group keeps K - 1 detectors, 3 it keeps K
             (or all it has), chosen at random per sample; 4 it keeps survivors_on_few_columns; else no flags
    nan      "random", and one NaN on an unflagged sample of a fitted unit"""
    cs = case(name)
    rng = np.random.default_rng(SEED + 100 * (1 + PATTERNS.index(pattern)) + CASES.index(name))
    ok = np.ones((cs.ndet, cs.ns), dtype=bool)
    v = cs.v
    if pattern in ("random", "nan"):
        ok = np.random.default_rng(SEED + 100 + CASES.index(name)).random((cs.ndet, cs.ns)) >= FLAG_RATE
    elif pattern == "dead":
        ok[9 if name == "groups20" else 1] = False
    elif pattern == "special":
        few = survivors_on_few_columns(cs)
        for i in range(cs.ns):
            r = i % 7
            if r == 1:
                ok[:, i] = False
            elif r in (2, 3):
                for a, b in zip(cs.edges[:-1], cs.edges[1:]):
                    n = min(b - a, cs.K - 1 if r == 2 else cs.K)
                    ok[a:b, i] = False
                    ok[a + rng.choice(b - a, size=n, replace=False), i] = True
            elif r == 4 and few is not None:
                ok[:, i] = few
    pix = np.where(ok, rng.integers(0, 1000, size=ok.shape), -1 - rng.integers(0, 3, size=ok.shape))
    pix = pix.astype(np.int32).reshape(-1)
    at = None
    if pattern == "nan":
        st = cmode_f64(pix, cs.ndet, cs.edges, cs.modes, v).status
        g, i = [int(x[-1]) for x in np.nonzero(st == FITTED)]
        k = int(cs.edges[g]) + int(np.flatnonzero(ok[cs.edges[g]:cs.edges[g + 1], i])[-1])
        at = (g, i, k)
        v = v.copy()
        v[k * cs.ns + i] = np.nan
    return SimpleNamespace(pix=pix, v=v, ok=ok, nan_at=at)


@functools.lru_cache(maxsize=None)
def case_ref(name, pattern):
    """the reference of a case, computed once and shared"""
    cs, d = case(name), data(name, pattern)
    return cmode_ref(d.pix, cs.ndet, cs.edges, cs.modes, d.v)


@functools.lru_cache(maxsize=None)
def case_f64(name, pattern):
    cs, d = case(name), data(name, pattern)
    return cmode_f64(d.pix, cs.ndet, cs.edges, cs.modes, d.v)


BOUNDED = tuple(p for p in PATTERNS if p != "nan")      # the patterns whose results are all finite


def measure_worst(name, pattern):
    r, f = case_ref(name, pattern), case_f64(name, pattern)
    assert np.array_equal(r.status, f.status)
    return max(V.excess(f.out, r.out, r.S, 1), V.excess(f.coeff, r.coeff, r.Sc, 1))
