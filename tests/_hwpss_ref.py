"""
Reference, restatement and error bound for the HWP-synchronous signal filter (csrc/cm2_hwpss.hip), and the cases the
CPU and the GPU tests share.  Plain NumPy, no GPU, in the manner of tests/_filter_ref.py.

  * ``hwpss_ref``: the definition of include/cosmomap2.h (f2c) in np.longdouble, starting from chi: per unit
    G = sum T T^T, b = sum T v over the unflagged samples, c = G^-1 b, out = v - T^T c.  With it comes S, the same
    formula with every operand replaced by its absolute value and every subtraction by an addition:
        S_t = |v_t| + |T(t)|^T |G^-1| sum_u |T(u)| |v_u|      (|G^-1| entry by entry),
    and Sc = |G^-1| sum_u |T(u)| |v_u| for the coefficients.  S = 0 on flagged samples and skipped units.
  * ``hwpss_f64``: a float64 restatement in the kernel's stated order, starting from the two tables cos chi and
    sin chi: the angle-addition recurrence, the segment sums (thread t: its samples t, t + 256, ... in sequence;
    shfl_down tree 32..1; ((w0 + w1) + w2) + w3; segments in ascending order from 0), the row-by-row Cholesky with
    the pivot rule, the two triangular solves and the projection.  The library is built with -ffp-contract=off and
    NumPy's elementwise loops do not fuse, so this matches the GPU bit for bit when the tables are the device's.

Acceptance, element by element: bit-equal to the restatement, or |got - ref| <= c 2^-53 S; exactly 0 where S = 0.

The constant c = count x HEADROOM.  ``count`` is read from the kernel source (c_count below).  No operation count
gives what the rounding of G and of its factor does to c = G^-1 b; that is measured: WORST is the largest
|hwpss_f64 - hwpss_ref| / (2^-53 S) over the shared cases (tests/test_hwpss_cpu.py re-measures it), and HEADROOM is
8 x WORST rounded up to a power of two, the project's established headroom between NumPy and the device.  The skip
decision stays out of the tolerance because every unit of every case has its smallest pivot ratio p_j / G_jj either
>= 2^-5 or <= 2^-40, in both precisions (tau = 2^-10); the CPU test asserts it.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _fit_ref as F
import _vector_ref as V

LD, U53, _ld = V.LD, V.U53, V._ld
bits, assert_bit_equal, pow2_at_least = V.bits, V.assert_bit_equal, V.pow2_at_least
excess, assert_accepted = F.excess, F.assert_accepted

SEG, THREADS = 4096, 256             # kSeg, kThreads of cm2_hwpss_policy.h
PER = SEG // THREADS
TAU = F.TAU                          # CM2_HWPSS_TAU
MAX_HARM = 8
PIVOT_OK, PIVOT_GONE = 2.0 ** -5, 2.0 ** -40

# largest |hwpss_f64 - hwpss_ref| / (2^-53 S) over outputs and coefficients of the shared cases, rounded up to one
# decimal; test_hwpss_cpu.py::test_restatement_against_reference_and_worst keeps it honest
WORST = 5.0
HEADROOM = pow2_at_least(8.0 * WORST)


def c_count(nseg, H):
    """Roundings on the longest chain from the inputs to an output sample, from cm2_hwpss.hip:
    3 (H - 1) + 2  the recurrence up to harmonic H (two products and a sum per step) on tables good to 2 ulp
    PER            a thread's terms: one product, then PER - 1 adds (0 + p is exact)
    6 + 3          shfl_down tree, the four waves
    nseg           the unit's segments, added in order
    2 K            the two triangular solves (a subtraction chain and a division per row, chains up to K long)
    K              terms of the projection
    1 + 2          v - p; second-order terms and the reference's own roundings"""
    K = 2 * H + 1
    return 3 * (H - 1) + 2 + PER + 6 + 3 + int(nseg) + 2 * K + K + 1 + 2


def c_bound(nseg, H):
    return c_count(nseg, H) * HEADROOM


hwpss_plan = F.edges                 # (ns, chunks) -> edges, as cosmomap2_amd.interfaces.hwpss_plan defines them


def segments_of(edges):
    e = np.asarray(edges, dtype=np.int64)
    return -(-(e[1:] - e[:-1]) // SEG)


# ------------------------------------------------------------------ templates ----
def templates_ld(chi, H):
    chi = _ld(chi)
    T = np.ones((chi.size, 2 * H + 1), dtype=LD)
    for n in range(1, H + 1):
        T[:, 2 * n - 1] = np.cos(LD(n) * chi)
        T[:, 2 * n] = np.sin(LD(n) * chi)
    return T


def templates_f64(c1, s1, H):
    c1, s1 = np.asarray(c1, dtype=np.float64), np.asarray(s1, dtype=np.float64)
    T = np.ones((c1.size, 2 * H + 1))
    T[:, 1], T[:, 2] = c1, s1
    for n in range(2, H + 1):
        T[:, 2 * n - 1] = T[:, 2 * n - 3] * c1 - T[:, 2 * n - 2] * s1
        T[:, 2 * n] = T[:, 2 * n - 2] * c1 + T[:, 2 * n - 3] * s1
    return T


# ------------------------------------------------- Cholesky with the pivot rule ----
def cholesky(G, dtype):
    """one unit through the batched form of _fit_ref.py -> (L or None when a pivot failed, the smallest pivot
    ratio tested)"""
    ch = F.cholesky(np.asarray(G)[None], dtype)
    return (None if ch.failed[0] else np.tril(ch.L[0])), float(ch.ratio[0])


def solve(L, b):
    return F.solve(L[None], np.asarray(b)[None])[0]


# --------------------------------------------------------------- the reference ----
def _units(ndet, edges):
    for k in range(ndet):
        for c in range(len(edges) - 1):
            yield k, c, int(edges[c]), int(edges[c + 1])


def factor_ref(chi, pix, ndet, edges, H):
    """what depends on chi and the flags only: per unit (mark, smallest pivot ratio, T on the unflagged samples,
    L, |G^-1|); mark 0 fitted, 1 m < K, 2 pivot"""
    ns, K = len(chi), 2 * H + 1
    Tc = {c: templates_ld(chi[a:b], H) for _, c, a, b in _units(1, edges)}
    out = {}
    for k, c, a, b in _units(ndet, edges):
        ok = np.asarray(pix[k * ns + a:k * ns + b]) >= 0
        m = int(ok.sum())
        if m < K:
            out[k, c] = SimpleNamespace(mark=1, ratio=None, ok=ok)
            continue
        Tv = Tc[c][ok]
        L, ratio = cholesky(Tv.T @ Tv, LD)
        if L is None:
            out[k, c] = SimpleNamespace(mark=2, ratio=ratio, ok=ok)
            continue
        Li = np.zeros((K, K), dtype=LD)
        for j in range(K):                              # L^-1 by forward substitution on the unit vectors
            e = np.zeros(K, dtype=LD)
            e[j] = 1
            for i in range(K):
                e[i] = (e[i] - L[i, :i] @ e[:i]) / L[i, i]
            Li[:, j] = e
        out[k, c] = SimpleNamespace(mark=0, ratio=ratio, ok=ok, Tv=Tv, L=L, Ginv_abs=np.abs(Li.T @ Li))
    return out


def hwpss_ref(chi, pix, ndet, edges, H, v, fact=None):
    """-> SimpleNamespace(out, S [nt], coeff, Sc [ndet, C, K], marks [ndet, C]) in np.longdouble"""
    ns, K, C = len(chi), 2 * H + 1, len(edges) - 1
    fact = fact or factor_ref(chi, pix, ndet, edges, H)
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
def unit_sums_f64(terms, valid):
    """terms (n, M) of a unit's samples -> (M,) sums in the kernel's order"""
    n, M = terms.shape
    total = np.zeros(M)
    for s0 in range(0, n, SEG):
        blk, ok = terms[s0:s0 + SEG], valid[s0:s0 + SEG]
        pad = np.zeros((SEG, M))
        pad[:len(blk)] = np.where(ok[:, None], blk, 0.0)
        pad = pad.reshape(PER, THREADS, M)
        acc = np.zeros((THREADS, M))
        for u in range(PER):                            # acc += T_j v, samples t, t + 256, ...
            acc = acc + pad[u]
        w = acc.reshape(4, 64, M).copy()
        for off in (32, 16, 8, 4, 2, 1):                # x += shfl_down(x, off): lane 0's tree
            w[:, :off] = w[:, :off] + w[:, off:2 * off]
        total = total + (((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    return total


def factor_f64(c1, s1, pix, ndet, edges, H):
    ns, K = len(c1), 2 * H + 1
    Tc = {c: templates_f64(c1[a:b], s1[a:b], H) for _, c, a, b in _units(1, edges)}
    out = {}
    for k, c, a, b in _units(ndet, edges):
        ok = np.asarray(pix[k * ns + a:k * ns + b]) >= 0
        T = Tc[c]
        G = unit_sums_f64((T[:, None, :] * T[:, :, None]).reshape(b - a, K * K), ok).reshape(K, K)
        if G[0, 0] < K:
            out[k, c] = SimpleNamespace(mark=1, ratio=None, ok=ok, T=T)
            continue
        L, ratio = cholesky(G, np.float64)
        out[k, c] = SimpleNamespace(mark=0 if L is not None else 2, ratio=ratio, ok=ok, T=T, L=L)
    return out


def hwpss_f64(c1, s1, pix, ndet, edges, H, v, fact=None):
    """-> SimpleNamespace(out [nt], coeff [ndet, C, K], marks [ndet, C]) in float64"""
    ns, K, C = len(c1), 2 * H + 1, len(edges) - 1
    fact = fact or factor_f64(c1, s1, pix, ndet, edges, H)
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
            p = np.full(b - a, cf[0])
            for j in range(1, K):
                p = p + cf[j] * f.T[:, j]
            out[k * ns + a:k * ns + b] = np.where(f.ok, vv - p, 0.0)
            coeff[k, c] = cf
    return SimpleNamespace(out=out, coeff=coeff, marks=marks)


# ----------------------------------------------------------------- acceptance ----
def c_samples(ndet, edges, H):
    """c per sample: its unit's segment count enters"""
    per = np.repeat([c_bound(n, H) for n in segments_of(edges)], np.diff(edges))
    return np.tile(per, ndet)


def c_coeffs(ndet, edges, H):
    K = 2 * H + 1
    per = np.repeat([c_bound(n, H) for n in segments_of(edges)], K).reshape(-1, K)
    return np.tile(per[None], (ndet, 1, 1))


# ---------------------------------------------------------------------- cases ----
HARMS = (1, 4, 8)
RATES = {"slow": 0.13, "fast": 1.97}       # rad per sample, with 2 % jitter
CASES = [(H, r) for H in HARMS for r in ("slow", "fast")]
NDET = 3
STALL = 300                          # length of the chunk with a stalled plate


def chunk_lengths(H, rate):
    """fast plate: K and K + 1 samples already span every harmonic; at 0.13 rad a sample such chunks are neither
    well nor hopelessly conditioned, so the slow cases start at 40 (H <= 4) or 64 (H = 8) samples"""
    K = 2 * H + 1
    short = [K, K + 1, 40, 64, 257] if rate == "fast" else ([40, 64, 257] if H <= 4 else [64, 257])
    return short + [STALL, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG + 1, 2 * SEG]


@functools.lru_cache(maxsize=None)
def case(H, rate):
    """3 detectors; detector 0 without flags, detector 1 with 30 % random flags, detector 2 with one unit all
    flagged (the 64-sample chunk), one with m = K - 1 (the 257-sample chunk) and one whose first and last
    segments are entirely flagged (the chunk of 2 SEG + 1 samples).  The plate stands still in chunk STALL.  The
    last chunk is two full segments and ends at ns."""
    K = 2 * H + 1
    rng = np.random.default_rng(4100 + 10 * H + (rate == "fast"))
    lens = chunk_lengths(H, rate)
    edges = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ns = int(edges[-1])
    step = RATES[rate] * (1.0 + 0.02 * rng.standard_normal(ns))
    ci = lens.index(STALL)
    step[edges[ci] + 1:edges[ci + 1]] = 0.0
    chi = 1.0e4 + np.cumsum(step)
    pix = rng.integers(0, 1000, size=NDET * ns).astype(np.int32)
    pix[ns:2 * ns][rng.random(ns) < 0.30] = -1
    p2 = pix[2 * ns:]
    a, b = edges[lens.index(64)], edges[lens.index(64) + 1]
    p2[a:b] = -1
    a, b = edges[lens.index(257)], edges[lens.index(257) + 1]
    keep = a + rng.choice(b - a, size=K - 1, replace=False)
    p2[a:b] = -2
    p2[keep] = 7
    a, b = edges[lens.index(2 * SEG + 1)], edges[lens.index(2 * SEG + 1) + 1]
    p2[a:a + SEG] = -1
    p2[a + 2 * SEG:b] = -1
    t = np.tile(chi, NDET)
    v = rng.standard_normal(NDET * ns) + 3.0 + 50.0 * np.cos(2.0 * t + 0.3) + 20.0 * np.sin(4.0 * t) \
        + 5.0 * np.cos(t)
    return SimpleNamespace(H=H, K=K, rate=rate, ns=ns, ndet=NDET, nt=NDET * ns, edges=edges, lens=lens, chi=chi,
                           pix=pix, v=v, stalled=ci)


@functools.lru_cache(maxsize=None)
def case_ref(H, rate):
    """the reference of a case, computed once and shared"""
    cs = case(H, rate)
    fact = factor_ref(cs.chi, cs.pix, cs.ndet, cs.edges, H)
    return fact, hwpss_ref(cs.chi, cs.pix, cs.ndet, cs.edges, H, cs.v, fact)


def host_tables(chi):
    """cos chi and sin chi rounded from extended precision: what the restatement starts from on the CPU"""
    return np.cos(_ld(chi)).astype(np.float64), np.sin(_ld(chi)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case_f64(H, rate):
    cs = case(H, rate)
    c1, s1 = host_tables(cs.chi)
    fact = factor_f64(c1, s1, cs.pix, cs.ndet, cs.edges, H)
    return fact, hwpss_f64(c1, s1, cs.pix, cs.ndet, cs.edges, H, cs.v, fact)


def measure_worst(H, rate):
    cs = case(H, rate)
    _, r = case_ref(H, rate)
    _, f = case_f64(H, rate)
    assert np.array_equal(r.marks, f.marks)
    return max(V.excess(f.out, r.out, r.S, 1), V.excess(f.coeff, r.coeff, r.Sc, 1))
