"""
Reference, restatement and error bound for the template filter (csrc/cm2_template.hip), and the cases the CPU and the
GPU tests share.  Plain NumPy, no GPU, in the manner of tests/_hwpss_ref.py, whose segment sums it reuses (the order
of a unit's sums is the same by definition).

  * ``centre_f64`` / ``centre_ref``: the chunk means of the caller's table in the kernel's stated order (thread t of
    one workgroup adds the finite values t, t + 256, ... of the whole chunk; shfl_down tree; ((w0 + w1) + w2) + w3;
    sum / count) and in np.longdouble, with the magnitude Smu = sum |x| / count.  ``design(tab, cst)`` puts the
    column of ones in front: T[ns, K], what both of the following start from.
  * ``template_ref``: the definition of include/cosmomap2.h (f2i) in np.longdouble from a given float64 T: per unit
    G = sum T T^T, b = sum T v over the unflagged samples, c = G^-1 b, out = v - T^T c, with the magnitudes S and Sc
    of tests/_hwpss_ref.py.  It starts from the centred table and not from the caller's, because centring moves c_0
    by c_j times the rounding of mu_j: the coefficients are defined on the table the handle holds.
  * ``template_f64``: the float64 restatement in the kernel's stated order from the same T.  The library is built with
    -ffp-contract=off and NumPy's elementwise loops do not fuse, so this matches the GPU bit for bit.

Acceptance, element by element: bit-equal to the restatement, or |got - ref| <= c 2^-53 S; exactly 0 where S = 0.
c = count x HEADROOM: ``count`` is read from the kernel source (c_count), HEADROOM is 8 x WORST rounded up to a power
of two, WORST the largest |template_f64 - template_ref| / (2^-53 S) over the shared cases, measured on the CPU
(tests/test_template_cpu.py re-measures it) and never on a GPU.  The skip decision stays out of the tolerance because
every unit of every case has its smallest pivot ratio either >= 2^-5 or <= 2^-40 (or not finite), in both precisions.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _fit_ref as F
import _hwpss_ref as H
import _vector_ref as V

LD, U53, _ld = V.LD, V.U53, V._ld
bits, assert_bit_equal, pow2_at_least = V.bits, V.assert_bit_equal, V.pow2_at_least
excess, assert_accepted = F.excess, F.assert_accepted
unit_sums_f64 = H.unit_sums_f64

SEG, THREADS = 4096, 256             # kSeg, kThreads of cm2_template_policy.h
PER = SEG // THREADS
assert (SEG, THREADS) == (H.SEG, H.THREADS)
TAU = F.TAU                          # CM2_TEMPLATE_TAU
MAX_K = 16                           # CM2_TEMPLATE_MAX_K
FITTED, FEW, PIVOT = 0, 1, 2         # CM2_TEMPLATE_FITTED, _FEW, _PIVOT
PIVOT_OK, PIVOT_GONE = 2.0 ** -5, 2.0 ** -40
# Status of cm2_template_policy.h
OK, BAD_COUNT, BAD_CONSTANT, BAD_K, BAD_SIZE, BAD_EDGES, TOO_LARGE = range(7)

# largest |template_f64 - template_ref| / (2^-53 S) over outputs and coefficients of the shared cases, rounded up to
# one decimal; test_template_cpu.py::test_restatement_against_reference_and_worst keeps it honest
WORST = 4.0
HEADROOM = pow2_at_least(8.0 * WORST)


def det_tile(K):
    """det_tile of cm2_template_policy.h: the detectors that share one read of the table"""
    return 4 if K <= 2 else 2


def c_count(nseg, K):
    """Roundings on the longest chain from the inputs to an output sample, from cm2_template.hip:
    PER            a thread's terms: one product, then PER - 1 adds (0 + p is exact)
    6 + 3          shfl_down tree, the four waves
    nseg           the unit's segments, added in order
    2 K            the two triangular solves (a subtraction chain and a division per row, chains up to K long)
    K              terms of the projection
    1 + 2          v - p; second-order terms and the reference's own roundings"""
    return PER + 6 + 3 + int(nseg) + 2 * K + K + 1 + 2


def c_bound(nseg, K):
    return c_count(nseg, K) * HEADROOM


def c_centre(n):
    """Roundings of mu over a chunk of n samples: ceil(n / 256) - 1 adds of a thread (0 + x is exact), the tree and
    the waves (6 + 3), the division, + 2 as everywhere.  No headroom: it is a plain sum."""
    return -(-int(n) // THREADS) - 1 + 6 + 3 + 1 + 2


plan = F.edges                       # (ns, chunks) -> edges, as cosmomap2_amd.interfaces.hwpss_plan defines them
segments_of = H.segments_of
cholesky, solve = H.cholesky, H.solve


# -------------------------------------------------------------------- centring ----
def _lane_sums(x):
    """x (n,) -> the 256 thread sums: thread t adds x[t], x[t + 256], ... in sequence, from 0"""
    n = len(x)
    rows = -(-n // THREADS)
    pad = np.zeros(rows * THREADS)
    pad[:n] = x
    pad = pad.reshape(rows, THREADS)
    acc = np.zeros(THREADS)
    for u in range(rows):
        acc = acc + pad[u]
    return acc


def _tree(acc):
    w = acc.reshape(4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def centre_f64(tab, edges):
    """-> (centred table [J, ns], mu [J, C]) in the order k_template_centre states"""
    tab = np.array(tab, dtype=np.float64, ndmin=2)
    out, mu = tab.copy(), np.zeros((tab.shape[0], len(edges) - 1))
    with np.errstate(invalid="ignore"):
        for j in range(tab.shape[0]):
            for c in range(len(edges) - 1):
                x = tab[j, edges[c]:edges[c + 1]]
                fin = np.isfinite(x)
                cnt = float(fin.sum())
                s = _tree(_lane_sums(np.where(fin, x, 0.0)))
                mu[j, c] = s / cnt if cnt > 0 else 0.0
                out[j, edges[c]:edges[c + 1]] = x - mu[j, c]
    return out, mu


def centre_ref(tab, edges):
    """-> (mu [J, C], Smu [J, C]) in np.longdouble: the mean of the finite values and the mean of their magnitudes"""
    tab = np.array(tab, dtype=np.float64, ndmin=2)
    mu, S = np.zeros((tab.shape[0], len(edges) - 1), dtype=LD), np.zeros((tab.shape[0], len(edges) - 1), dtype=LD)
    for j in range(tab.shape[0]):
        for c in range(len(edges) - 1):
            x = tab[j, edges[c]:edges[c + 1]]
            x = _ld(x[np.isfinite(x)])
            if x.size:
                mu[j, c], S[j, c] = x.sum() / LD(x.size), np.abs(x).sum() / LD(x.size)
    return mu, S


def design(tab, cst):
    """the handle's table [J, ns] (already centred when cst) -> T [ns, K]"""
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, np.shape(tab)[-1])
    return np.ascontiguousarray(np.vstack([np.ones((1, tab.shape[1]))] * int(cst) + [tab]).T)


# --------------------------------------------------------------- the reference ----
def _units(ndet, edges):
    for k in range(ndet):
        for c in range(len(edges) - 1):
            yield k, c, int(edges[c]), int(edges[c + 1])


def factor_ref(T, pix, ndet, edges):
    """what depends on the templates and the flags only: per unit (mark, smallest pivot ratio, T on the unflagged
    samples, L, |G^-1|)"""
    ns, K = T.shape
    Tl = _ld(T)
    out = {}
    with np.errstate(all="ignore"):
        for k, c, a, b in _units(ndet, edges):
            ok = np.asarray(pix[k * ns + a:k * ns + b]) >= 0
            if int(ok.sum()) < K:
                out[k, c] = SimpleNamespace(mark=FEW, ratio=None, ok=ok)
                continue
            Tv = Tl[a:b][ok]
            L, ratio = cholesky(Tv.T @ Tv, LD)
            if L is None:
                out[k, c] = SimpleNamespace(mark=PIVOT, ratio=ratio, ok=ok)
                continue
            Li = np.zeros((K, K), dtype=LD)
            for j in range(K):                          # L^-1 by forward substitution on the unit vectors
                e = np.zeros(K, dtype=LD)
                e[j] = 1
                for i in range(K):
                    e[i] = (e[i] - L[i, :i] @ e[:i]) / L[i, i]
                Li[:, j] = e
            out[k, c] = SimpleNamespace(mark=FITTED, ratio=ratio, ok=ok, Tv=Tv, L=L, Ginv_abs=np.abs(Li.T @ Li))
    return out


def template_ref(T, pix, ndet, edges, v, fact=None):
    """-> SimpleNamespace(out, S [nt], coeff, Sc [ndet, C, K], marks [ndet, C]) in np.longdouble"""
    ns, K = T.shape
    C = len(edges) - 1
    fact = fact or factor_ref(T, pix, ndet, edges)
    v = _ld(v)
    out, S = np.zeros(ndet * ns, dtype=LD), np.zeros(ndet * ns, dtype=LD)
    coeff, Sc = np.zeros((ndet, C, K), dtype=LD), np.zeros((ndet, C, K), dtype=LD)
    marks = np.zeros((ndet, C), dtype=np.int64)
    for k, c, a, b in _units(ndet, edges):
        f = fact[k, c]
        marks[k, c] = f.mark
        if f.mark:
            continue
        vv = v[k * ns + a:k * ns + b][f.ok]
        cf = solve(f.L, f.Tv.T @ vv)
        sc = f.Ginv_abs @ (np.abs(f.Tv).T @ np.abs(vv))
        o, s = np.zeros(b - a, dtype=LD), np.zeros(b - a, dtype=LD)
        o[f.ok] = vv - f.Tv @ cf
        s[f.ok] = np.abs(vv) + np.abs(f.Tv) @ sc
        out[k * ns + a:k * ns + b], S[k * ns + a:k * ns + b] = o, s
        coeff[k, c], Sc[k, c] = cf, sc
    return SimpleNamespace(out=out, S=S, coeff=coeff, Sc=Sc, marks=marks)


# -------------------------------------------------------------- the restatement ----
def factor_f64(T, pix, ndet, edges):
    ns, K = T.shape
    out = {}
    with np.errstate(all="ignore"):
        for k, c, a, b in _units(ndet, edges):
            ok = np.asarray(pix[k * ns + a:k * ns + b]) >= 0
            Tc = T[a:b]
            if int(ok.sum()) < K:                       # m: an integer count (k_template_count)
                out[k, c] = SimpleNamespace(mark=FEW, ratio=None, ok=ok, T=Tc)
                continue
            G = unit_sums_f64((Tc[:, None, :] * Tc[:, :, None]).reshape(b - a, K * K), ok).reshape(K, K)
            L, ratio = cholesky(G, np.float64)
            out[k, c] = SimpleNamespace(mark=FITTED if L is not None else PIVOT, ratio=ratio, ok=ok, T=Tc, L=L)
    return out


def template_f64(T, pix, ndet, edges, v, fact=None):
    """-> SimpleNamespace(out [nt], coeff [ndet, C, K], marks [ndet, C]) in float64"""
    ns, K = T.shape
    C = len(edges) - 1
    fact = fact or factor_f64(T, pix, ndet, edges)
    v = np.asarray(v, dtype=np.float64)
    out, coeff = np.zeros(ndet * ns), np.zeros((ndet, C, K))
    marks = np.zeros((ndet, C), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, c, a, b in _units(ndet, edges):
            f = fact[k, c]
            marks[k, c] = f.mark
            if f.mark:
                continue
            vv = v[k * ns + a:k * ns + b]
            cf = solve(f.L, unit_sums_f64(f.T * vv[:, None], f.ok))
            p = cf[0] * f.T[:, 0]
            for j in range(1, K):
                p = p + cf[j] * f.T[:, j]
            out[k * ns + a:k * ns + b] = np.where(f.ok, vv - p, 0.0)
            coeff[k, c] = cf
    return SimpleNamespace(out=out, coeff=coeff, marks=marks)


# ----------------------------------------------------------------- acceptance ----
def c_samples(ndet, edges, K):
    """c per sample: its unit's segment count enters"""
    per = np.repeat([c_bound(n, K) for n in segments_of(edges)], np.diff(edges))
    return np.tile(per, ndet)


def c_coeffs(ndet, edges, K):
    per = np.repeat([c_bound(n, K) for n in segments_of(edges)], K).reshape(-1, K)
    return np.tile(per[None], (ndet, 1, 1))


# ---------------------------------------------------------------------- cases ----
# (K, add_constant): the constant alone, one template alone, then J = K - 1 templates beside the constant, and three
# templates as given (the variants with a NaN are bit-exact statements there: no mean is taken)
MODES = [(1, True), (1, False), (2, True), (3, True), (9, True), (16, True), (3, False)]
RATES = (0.0, 0.10, 0.30)            # flag rate of detector k: RATES[k % 3], on the chunks of 200 samples and more
MODERATE = [200 + 37 * i for i in range(12)]
VARIANTS = ("clean", "valid", "flagged")


def chunk_lengths(K):
    """1, K - 1, K, K + 1 (those that exist, once each), twelve moderate chunks that keep the fitted share above
    80 %, then S - 1, S, S + 1, 2 S + 3"""
    short = sorted({n for n in (1, K - 1, K, K + 1) if n >= 1})
    return short + MODERATE + [SEG - 1, SEG, SEG + 1, 2 * SEG + 3]


def _tables(rng, lens, edges, K, cst):
    """J templates.  On the chunks of at most K + 1 samples: columns of the DCT-II, orthogonal to each other and to
    the constant, so that K samples already span them.  Elsewhere: template 0 a slow drift on a large pedestal,
    0.1 + 1e-5 ramp, the others white."""
    J = K - int(cst)
    ns = int(edges[-1])
    tab = rng.standard_normal((J, ns)) if J else np.zeros((0, ns))
    if J:
        tab[0] = 0.1 + 1.0e-5 * np.linspace(-1.0, 1.0, ns)
    for c, n in enumerate(lens):
        if n <= K + 1:
            q = np.arange(n) + 0.5
            for j in range(J):
                tab[j, edges[c]:edges[c + 1]] = np.cos(np.pi * q * (j + int(cst)) / n)
    return tab


def make_case(K, cst, lens, ndet, seed):
    """The chunk of S samples is the one no unit can fit: two equal templates (J >= 2), a template constant on the
    chunk beside the constant (K = 2), a template that vanishes there (one template alone).  The last detector is
    fully flagged in the chunk of S + 1 samples, detector 1 (if any) in the chunk of K + 1; the samples HOLE of the
    chunk of S - 1 samples are flagged in every detector."""
    rng = np.random.default_rng(seed)
    edges = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ns, J = int(edges[-1]), K - int(cst)
    at = lambda n: (int(edges[lens.index(n)]), int(edges[lens.index(n) + 1]))
    tab = _tables(rng, lens, edges, K, cst)
    if SEG in lens and J:
        a, b = at(SEG)
        if J >= 2:
            tab[1, a:b] = tab[0, a:b]
        elif cst:
            tab[0, a:b] = 0.1
        else:
            tab[0, a:b] = 0.0
    pix = rng.integers(0, 1000, size=ndet * ns).astype(np.int32)
    p2 = pix.reshape(ndet, ns)
    long_ = np.repeat(np.asarray(lens) >= 200, lens)
    for k in range(ndet):
        p2[k][long_ & (rng.random(ns) < RATES[k % 3])] = -1
    if SEG + 1 in lens:
        a, b = at(SEG + 1)
        p2[ndet - 1, a:b] = -1
    if ndet > 1 and K + 1 in lens:
        a, b = at(K + 1)
        p2[1, a:b] = -2
    hole = None
    if SEG - 1 in lens:
        a, b = at(SEG - 1)
        hole = (a + 100, a + 1500)
        p2[:, list(hole)] = -1
    t = np.arange(ns) / 1000.0
    v = rng.standard_normal(ndet * ns) + 3.0 + np.tile(50.0 * np.cos(2.0 * t + 0.3) + 20.0 * np.sin(0.7 * t), ndet)
    if J:
        v += (np.arange(1, ndet + 1)[:, None] * 1.0e6 * (tab[0] - 0.1)[None, :]).reshape(-1)
    return SimpleNamespace(K=K, cst=bool(cst), J=J, ns=ns, ndet=ndet, nt=ndet * ns, edges=edges, lens=list(lens),
                           tab=tab, pix=pix, v=v, hole=hole)


@functools.lru_cache(maxsize=None)
def case(K, cst, variant="clean"):
    """det_tile(K) + 1 detectors on every chunk length.  Variants: "valid" has a NaN and an Inf in the table on
    samples of the chunk of S + 1 samples that are unflagged in detector 0 (its flag rate is 0); "flagged" has them
    on the HOLE samples, which every detector flags."""
    lens = chunk_lengths(K)
    cs = make_case(K, cst, lens, det_tile(K) + 1, 7100 + 10 * K + int(cst))
    cs.variant = variant
    if variant != "clean":
        assert cs.J >= 1
        cs.tab = cs.tab.copy()
        if variant == "valid":
            a = int(cs.edges[lens.index(SEG + 1)])
            cs.poisoned = lens.index(SEG + 1)
            cs.tab[0, a + 7], cs.tab[cs.J - 1, a + 3000] = np.nan, np.inf
        else:
            cs.poisoned = lens.index(SEG - 1)
            cs.tab[0, cs.hole[0]], cs.tab[cs.J - 1, cs.hole[1]] = np.nan, -np.inf
    return cs


SWEEP_LENS = lambda K: [K + 1, 300, SEG + 1]


def sweep_ndets(K):
    """1, Dt - 1, Dt, 2 Dt + 1, each once (Dt + 1 is the shared case itself)"""
    Dt = det_tile(K)
    return tuple(sorted({1, Dt - 1, Dt, 2 * Dt + 1}))


@functools.lru_cache(maxsize=None)
def sweep_case(K, cst, ndet):
    cs = make_case(K, cst, SWEEP_LENS(K), ndet, 7300 + 100 * K + 10 * int(cst) + ndet)
    cs.variant = "sweep"
    return cs


def evaluate(cs, tab=None):
    """-> SimpleNamespace(T, fact_f64, f64, fact_ref, ref) of a case, from `tab`, the handle's table; None: from the
    restatement's own centring of cs.tab"""
    if tab is None:
        tab = centre_f64(cs.tab, cs.edges)[0] if cs.cst and cs.J else cs.tab
    T = design(np.asarray(tab).reshape(cs.J, cs.ns), cs.cst)
    ff = factor_f64(T, cs.pix, cs.ndet, cs.edges)
    fr = factor_ref(T, cs.pix, cs.ndet, cs.edges)
    return SimpleNamespace(T=T, fact_f64=ff, f64=template_f64(T, cs.pix, cs.ndet, cs.edges, cs.v, ff),
                           fact_ref=fr, ref=template_ref(T, cs.pix, cs.ndet, cs.edges, cs.v, fr))


@functools.lru_cache(maxsize=None)
def case_eval(K, cst, variant="clean"):
    """the CPU evaluation of a shared case, computed once"""
    return evaluate(case(K, cst, variant))


def measure_worst(K, cst):
    e = case_eval(K, cst)
    assert np.array_equal(e.ref.marks, e.f64.marks)
    return max(V.excess(e.f64.out, e.ref.out, e.ref.S, 1), V.excess(e.f64.coeff, e.ref.coeff, e.ref.Sc, 1))
