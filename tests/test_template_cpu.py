"""
The template filter without a GPU: the names, the header and the prototype table; the plan of cm2_template_policy.h
compiled with the host compiler against Python; the constructor's argument checks; the float64 restatement of
_template_ref.py against the extended-precision reference (with the re-measurement of WORST) and its centring against
the long-double means; and the conditions on the shared cases that the GPU tests rely on.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _template_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
LD, U53 = R.LD, R.U53
ENTRY_POINTS = ("create", "destroy", "info", "apply", "fit", "status", "tables")


# ------------------------------------------------------------ names and header ----
def test_names_header_prototypes_and_constants_agree():
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, build as B, kernel_resources as KR
    from cosmomap2_amd.interfaces import linearoperators as L
    assert callable(I.TemplateFilterLO) and "TemplateFilterLO" in L.__all__
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint cm2_template_%s\(" % name, hdr), name
        assert "cm2_template_" + name in _hip.PROTOTYPES
    for name in ("create", "apply", "fit", "status", "tables"):               # the stream comes last
        decl = re.search(r"int cm2_template_%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.rstrip().endswith("void *stream"), name
        assert _hip.PROTOTYPES["cm2_template_" + name][-1] is _hip._vp
        assert "cm2_template_" + name in _hip.RESTARTABLE                     # they overwrite their outputs
    assert len(_hip.PROTOTYPES["cm2_template_create"]) == 10
    assert re.search(r"#define CM2_TEMPLATE_TAU 0\.0009765625\b", hdr) and R.TAU == 0.0009765625
    assert re.search(r"#define CM2_TEMPLATE_MAX_K %d\b" % R.MAX_K, hdr) and L.TEMPLATE_MAX_K == R.MAX_K == 16
    for name, val in (("FITTED", R.FITTED), ("FEW", R.FEW), ("PIVOT", R.PIVOT)):
        assert re.search(r"#define CM2_TEMPLATE_%s %d\b" % (name, val), hdr)
        assert getattr(L, "TEMPLATE_" + name) == val
    assert hdr.index("---- f2h:") < hdr.index("---- f2i:") < hdr.index("---- f3:")
    assert "offset AT THE CHUNK MEAN" in hdr                                  # what c_0 means is said where it is defined
    assert "chunk mean" in I.TemplateFilterLO.__doc__
    for k in ("k_template_sums<16, false>", "k_template_subtract<16>", "k_template_centre"):
        assert any(re.search(p, k) for p in KR.NO_SPILL), k                   # the build refuses spills in them
    assert "cm2_template.hip" not in B.FMA_OK


# --------------------------------------------------------- constructor refusals ----
def test_arguments_are_refused_before_the_gpu_is_needed():
    from cosmomap2_amd import _hip
    from cosmomap2_amd.interfaces import TemplateFilterLO
    from cosmomap2_amd.linop import ShapeError
    tab, pix = np.linspace(0.0, 9.0, 150).reshape(3, 50), np.zeros(100, dtype=np.int32)
    for kw in (dict(ndet=0), dict(ndet=1.5), dict(chunks=0), dict(chunks=[0, 60]), dict(chunks=[0, 20, 20, 50]),
               dict(chunks=[3, 50]), dict(add_constant=1), dict(add_constant=None), dict(add_constant="yes")):
        args = dict(ndet=2)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            TemplateFilterLO(tab, pix, **args)
        assert str(e.value)
    many = np.zeros((16, 50))
    for t, kw in ((many, dict()), (np.zeros((17, 50)), dict(add_constant=False)),
                  (np.zeros((0, 50)), dict(add_constant=False))):                  # K = 17, 17, 0
        with pytest.raises(ValueError) as e:
            TemplateFilterLO(t, pix, ndet=2, **kw)
        assert "K = " in str(e.value)
    for a, kw in (((tab, pix), dict(ndet=3)), ((tab, pix[:99]), dict(ndet=2)), ((tab.reshape(3, 5, 10), pix), dict(ndet=2)),
                  ((np.float64(1.0), pix), dict(ndet=2)), ((tab[:, :0], pix[:0]), dict(ndet=2)),
                  ((tab, pix), dict(ndet=2, chunks=[[0, 50]]))):
        with pytest.raises(ShapeError):
            TemplateFilterLO(*a, **kw)
    import torch
    if not torch.cuda.is_available():
        for t, kw in ((tab, dict()), (tab[0], dict()), (many, dict(add_constant=False)), (np.zeros((0, 50)), dict())):
            with pytest.raises(_hip.HipError):                                     # accepted: K = 4, 2, 16, 1
                TemplateFilterLO(t, pix, ndet=2, **kw)


# ------------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_template_policy.h"
#include <cstdio>
#include <cstdlib>
using namespace cm2::tmpl;
int main(int argc, char **argv)
{
    // driver ns ndet ntemplates add_constant e0 e1 ...
    if (argc < 6) return 2;
    printf("%d %d %d %d %d %d %d %d %d\n", kSeg, kThreads, kPer, kMaxK, packed(kMaxK), packed_at(3, 2), (int)kFitted,
           (int)kFew, (int)kPivot);
    for (int K = 1; K <= kMaxK; ++K) printf("%d ", det_tile(K));
    printf("\n%d %d %d %d %d %d %d\n", (int)kOk, (int)kBadCount, (int)kBadConstant, (int)kBadK, (int)kBadSize,
           (int)kBadEdges, (int)kTooLarge);
    std::vector<int64_t> e;
    for (int i = 5; i < argc; ++i) e.push_back(atoll(argv[i]));
    Plan p;
    const Status st = make_plan(&p, atoll(argv[1]), atoll(argv[2]), (int64_t)e.size() - 1, e.data(), atoi(argv[3]),
                                atoi(argv[4]));
    printf("%d\n", (int)st);
    if (st != kOk) return 0;
    printf("%lld %lld %lld %lld %d %d %d %d %lld %lld %lld %lld %lld\n", (long long)p.ns, (long long)p.ndet,
           (long long)p.nchunks, (long long)p.nt, p.J, p.K, p.add_constant, p.Dt, (long long)p.segs_per_det,
           (long long)p.nsegs, (long long)p.nunits, (long long)p.ntiles, (long long)p.ngroups);
    for (size_t c = 0; c < p.seg_first.size(); ++c) printf("%lld ", (long long)p.seg_first[c]);
    printf("\n");
    for (int64_t r = 0; r < p.segs_per_det; ++r) {
        int64_t t0, t1;
        segment_range(p, r, &t0, &t1);
        printf("%d %lld %lld\n", (int)p.seg_chunk[(size_t)r], (long long)t0, (long long)t1);
    }
    for (int64_t w = 0; w < p.ngroups && w < 4096; ++w) {
        int64_t r, k0, k1;
        group_range(p, w, &r, &k0, &k1);
        printf("%lld %lld %lld\n", (long long)r, (long long)k0, (long long)k1);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("template_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_policy_constants(driver):
    out = _run(driver, 10, 1, 1, 1, 0, 10)
    assert out[0] == [R.SEG, R.THREADS, R.PER, R.MAX_K, 136, 8, R.FITTED, R.FEW, R.PIVOT]
    assert out[1] == [R.det_tile(K) for K in range(1, R.MAX_K + 1)]
    assert all(R.det_tile(K) * K <= 32 for K in range(1, R.MAX_K + 1))          # the accumulators of a thread
    assert out[2] == [R.OK, R.BAD_COUNT, R.BAD_CONSTANT, R.BAD_K, R.BAD_SIZE, R.BAD_EDGES, R.TOO_LARGE]
    assert R.SEG == R.THREADS * R.PER == 4096


@pytest.mark.parametrize("ndet,J,cst,edges", [
    (1, 0, 1, [0, 1]), (3, 1, 0, [0, R.SEG]), (9, 7, 1, [0, R.SEG + 1]), (8, 8, 1, [0, 3, R.SEG + 2, 3 * R.SEG + 2]),
    (17, 2, 1, [0, 3, R.SEG + 2, 3 * R.SEG + 2, 3 * R.SEG + 3]), (5, 16, 0, [0, 5, 9]),
    (7, 2, 1, [int(e) for e in R.case(3, True).edges]), (3, 15, 1, [int(e) for e in R.case(16, True).edges]),
])
def test_segments_tile_every_chunk_and_groups_tile_the_detectors(driver, ndet, J, cst, edges):
    ns, C, K = edges[-1], len(edges) - 1, J + cst
    out = _run(driver, ns, ndet, J, cst, *edges)
    assert out[3] == [R.OK]
    nseg = [int(n) for n in R.segments_of(edges)]
    first = [0] + list(np.cumsum(nseg))
    Dt = R.det_tile(K)
    ntiles = -(-ndet // Dt)
    assert out[4] == [ns, ndet, C, ns * ndet, J, K, cst, Dt, first[-1], ndet * first[-1], ndet * C, ntiles,
                      ntiles * first[-1]]
    assert out[5] == first
    rows = out[6:6 + first[-1]]
    for c in range(C):
        mine = rows[first[c]:first[c + 1]]
        assert all(r[0] == c for r in mine)
        assert mine[0][1] == edges[c] and mine[-1][2] == edges[c + 1]
        assert all(b[1] == a[2] for a, b in zip(mine[:-1], mine[1:]))             # no gap, no overlap
        assert all(r[2] - r[1] == R.SEG for r in mine[:-1]) and 0 < mine[-1][2] - mine[-1][1] <= R.SEG
    groups = out[6 + first[-1]:]
    assert len(groups) == ntiles * first[-1]
    # tiles run fastest; every (row segment, detector) pair belongs to exactly one workgroup
    assert [g[0] for g in groups] == [w // ntiles for w in range(len(groups))]
    seen = set()
    for r, k0, k1 in groups:
        assert k0 % Dt == 0 and 0 < k1 - k0 <= Dt and k1 <= ndet
        seen.update((r, k) for k in range(k0, k1))
    assert len(seen) == first[-1] * ndet == sum(k1 - k0 for _, k0, k1 in groups)


def test_plan_refusals(driver):
    status = lambda *a: _run(driver, *a)[3][0]
    assert status(10, 1, -1, 1, 0, 10) == R.BAD_COUNT and status(10, 1, -1, 7, 0, 10) == R.BAD_COUNT
    assert status(10, 1, 1, 2, 0, 10) == R.BAD_CONSTANT and status(10, 1, 1, -1, 0, 10) == R.BAD_CONSTANT
    assert status(10, 1, 0, 0, 0, 10) == R.BAD_K and status(10, 1, 16, 1, 0, 10) == R.BAD_K
    assert status(10, 1, 17, 0, 0, 10) == R.BAD_K and status(10, 1, 2147483647, 1, 0, 10) == R.BAD_K
    assert status(10, 1, 16, 0, 0, 10) == R.OK and status(10, 1, 15, 1, 0, 10) == R.OK and status(10, 1, 0, 1, 0, 10) == R.OK
    assert status(0, 1, 1, 1, 0, 0) == R.BAD_SIZE and status(10, 0, 1, 1, 0, 10) == R.BAD_SIZE
    assert status(10, 1, 1, 1, 0, 9) == R.BAD_EDGES and status(10, 1, 1, 1, 1, 10) == R.BAD_EDGES
    assert status(10, 1, 1, 1, 0, 5, 5, 10) == R.BAD_EDGES and status(10, 1, 1, 1, 0, 7, 3, 10) == R.BAD_EDGES
    assert status(1 << 40, 1, 1, 1, 0, 1 << 40) == R.TOO_LARGE                         # ns
    assert status(1 << 30, (1 << 16) + 1, 1, 1, 0, 1 << 30) == R.TOO_LARGE             # ndet ns > 2^46
    assert status(1 << 20, 1 << 23, 1, 1, 0, 1 << 20) == R.TOO_LARGE                   # 2^31 segments
    assert status(1 << 20, 1 << 22, 1, 1, 0, 1 << 20) == R.OK


# ------------------------------------------------------ the conditions on the cases ----
@pytest.mark.parametrize("K,cst", R.MODES)
def test_case_has_what_the_tests_need(K, cst):
    cs = R.case(K, cst)
    e = R.case_eval(K, cst)
    Dt = R.det_tile(K)
    assert cs.ndet == Dt + 1 >= 3 and cs.nt <= 2.0e5 and cs.edges[-1] == cs.ns and cs.J == K - int(cst)
    for n in (1, K - 1, K, K + 1, R.SEG - 1, R.SEG, R.SEG + 1, 2 * R.SEG + 3):
        assert n in cs.lens or n < 1
    assert set(R.sweep_ndets(K) + (cs.ndet,)) == {1, Dt - 1, Dt, Dt + 1, 2 * Dt + 1}
    ok = (cs.pix >= 0).reshape(cs.ndet, cs.ns)
    long_ = np.repeat((np.asarray(cs.lens) >= 200) & (np.asarray(cs.lens) != R.SEG + 1), cs.lens)
    for k in range(min(cs.ndet, 3)):
        rate = 1 - ok[k, long_].mean()
        assert abs(rate - R.RATES[k]) < 0.03, (k, rate)
    c1 = cs.lens.index(R.SEG + 1)
    assert not ok[cs.ndet - 1, cs.edges[c1]:cs.edges[c1 + 1]].any()                     # one unit fully flagged
    assert not ok[:, list(cs.hole)].any()
    m = e.ref.marks
    assert np.array_equal(m, e.f64.marks)
    assert (m == R.FEW).sum() >= 2 and (m == R.FITTED).mean() >= 0.80
    if (K, cst) == (1, True):
        assert (m == R.PIVOT).sum() == 0          # G = m >= 1 is its own pivot: the constant alone cannot fail the test
    else:
        assert (m == R.PIVOT).sum() >= 3 and (m[:, cs.lens.index(R.SEG)] == R.PIVOT).all()
    if cs.J:                                      # the slow drift on its pedestal: fitted wherever there are samples
        big = [c for c, n in enumerate(cs.lens) if n >= 200 and n != R.SEG]
        drift = cs.tab[0][np.repeat(np.isin(np.arange(len(cs.lens)), big), cs.lens)]
        assert (m[:-1, big] == R.FITTED).all() and abs(drift.mean() - 0.1) < 1e-5 and 0 < np.ptp(drift) <= 2.1e-5


@pytest.mark.parametrize("K,cst", R.MODES)
def test_pivots_are_far_from_the_threshold_in_both_precisions(K, cst):
    variants = R.VARIANTS if K >= 2 else ("clean",)
    for variant in variants:
        e = R.case_eval(K, cst, variant)
        for key in e.fact_ref:
            fr, ff = e.fact_ref[key], e.fact_f64[key]
            assert fr.mark == ff.mark, (variant, key)
            for f in (fr, ff):
                if f.mark != R.FEW:                                  # m < K is decided by the count alone
                    assert f.ratio >= R.PIVOT_OK or f.ratio <= R.PIVOT_GONE, (variant, key, f.ratio)
                    assert (f.ratio >= R.PIVOT_OK) == (f.mark == R.FITTED)
    assert R.PIVOT_GONE < R.TAU < R.PIVOT_OK


def test_without_centring_the_pedestal_would_skip_every_unit():
    """the reason the handle centres: the same table beside the constant, as given, fails the pivot test wherever it
    is tried, and centred it is fitted; centring leaves the output where it was, to the bound"""
    cs = R.case(2, True)
    raw = R.factor_f64(R.design(cs.tab, True), cs.pix, cs.ndet, cs.edges)
    e = R.case_eval(2, True)
    tried = [key for key, f in raw.items() if f.mark != R.FEW and cs.lens[key[1]] >= 200]    # where the drift is
    assert len(tried) > 50 and all(raw[key].mark == R.PIVOT for key in tried)
    assert sum(e.fact_f64[key].mark == R.FITTED for key in tried) >= len(tried) - cs.ndet
    # in extended precision the pedestal can be fitted as given: the same output
    sub = np.repeat(np.asarray(cs.lens) == 237, cs.lens)
    a, b = np.flatnonzero(sub)[[0, -1]]
    edges, pix = np.array([0, b + 1 - a]), cs.pix[a:b + 1]
    v = cs.v[a:b + 1]
    T_raw = R._ld(R.design(cs.tab[:, a:b + 1], True))
    T_cen = R._ld(e.T[a:b + 1])
    okm = pix >= 0
    outs = []
    for T in (T_raw, T_cen):
        Tv, vv = T[okm], R._ld(v)[okm]
        outs.append(vv - Tv @ R.solve(_chol_ld(Tv.T @ Tv), Tv.T @ vv))
    r = R.template_ref(e.T[a:b + 1], pix, 1, edges, v)
    assert R.excess(outs[1], r.out[okm], r.S[okm], 1) <= 1.0
    # uncentred, G is conditioned like (0.1 / 1e-7)^2: what is left of 64 bits
    assert float(np.abs(outs[0] - outs[1]).max()) <= 1e-3 * float(np.abs(outs[1]).max())


def _chol_ld(G):
    """plain Cholesky in np.longdouble, no pivot rule"""
    K = G.shape[0]
    L = np.zeros_like(G)
    for j in range(K):
        L[j, j] = np.sqrt(G[j, j] - (L[j, :j] * L[j, :j]).sum())
        for i in range(j + 1, K):
            L[i, j] = (G[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


@pytest.mark.parametrize("K,cst", [(3, True), (16, True), (3, False)])
def test_a_non_finite_template_value_skips_the_units_that_see_it(K, cst):
    clean, cs0 = R.case_eval(K, cst), R.case(K, cst)
    ok = (cs0.pix >= 0).reshape(cs0.ndet, cs0.ns)
    # on unflagged samples: the units of that chunk that see one of the two values are skipped as pivot failures
    cs, e = R.case(K, cst, "valid"), R.case_eval(K, cst, "valid")
    bad = np.flatnonzero(~np.isfinite(cs.tab).all(axis=0))
    assert len(bad) == 2 and ok[0, bad].all()
    for res in (e.ref, e.f64):
        for k in range(cs.ndet):
            for c in range(len(cs.lens)):
                sl = slice(k * cs.ns + int(cs.edges[c]), k * cs.ns + int(cs.edges[c + 1]))
                if c == cs.poisoned and clean.ref.marks[k, c] == R.FITTED and ok[k, bad].any():
                    assert res.marks[k, c] == R.PIVOT and not np.asarray(res.out[sl]).any()
                elif c != cs.poisoned:                               # the neighbours: the same bits
                    assert res.marks[k, c] == clean.ref.marks[k, c]
                    if res is e.f64:
                        assert np.array_equal(R.bits(res.out[sl]), R.bits(clean.f64.out[sl])), (k, c)
                        assert np.array_equal(R.bits(res.coeff[k, c]), R.bits(clean.f64.coeff[k, c]))
    assert (e.f64.marks[0, cs.poisoned] == R.PIVOT) and np.isfinite(e.f64.out).all()
    # under flags only: nothing changes -- to the bit without the constant; with it the chunk's means move by the
    # two values that left them, which the constant absorbs to rounding
    cs, e = R.case(K, cst, "flagged"), R.case_eval(K, cst, "flagged")
    bad = np.flatnonzero(~np.isfinite(cs.tab).all(axis=0))
    assert len(bad) == 2 and not ok[:, bad].any()
    assert np.array_equal(e.ref.marks, clean.ref.marks) and np.array_equal(e.f64.marks, clean.f64.marks)
    assert np.isfinite(e.f64.out).all() and np.isfinite(e.f64.coeff).all()
    a, b = int(cs.edges[cs.poisoned]), int(cs.edges[cs.poisoned + 1])
    inside = np.tile((np.arange(cs.ns) >= a) & (np.arange(cs.ns) < b), cs.ndet)
    if not cst:
        assert np.array_equal(R.bits(e.f64.out), R.bits(clean.f64.out))
        assert np.array_equal(R.bits(e.f64.coeff), R.bits(clean.f64.coeff))
    else:
        assert np.array_equal(R.bits(e.f64.out[~inside]), R.bits(clean.f64.out[~inside]))
        c = R.c_samples(cs.ndet, cs.edges, K)
        assert R.excess(e.f64.out, clean.ref.out, clean.ref.S, c) <= 1.0


# ------------------------------------------------ restatement against reference ----
def test_restatement_against_reference_and_worst():
    worst = max(R.measure_worst(K, cst) for K, cst in R.MODES)
    print("largest |template_f64 - template_ref| / (2^-53 S): %.3f (WORST = %.1f)" % (worst, R.WORST))
    assert worst <= R.WORST <= worst + 0.1                           # the committed constant is the measured one
    assert R.HEADROOM == R.pow2_at_least(8 * R.WORST) == 32
    for K, cst in R.MODES:
        cs, e = R.case(K, cst), R.case_eval(K, cst)
        # a fortiori within the bound the GPU is held to, with the factor 8 to spare
        assert R.excess(e.f64.out, e.ref.out, e.ref.S, R.c_samples(cs.ndet, cs.edges, K)) <= 0.125
        assert R.excess(e.f64.coeff, e.ref.coeff, e.ref.Sc, R.c_coeffs(cs.ndet, cs.edges, K)) <= 0.125
        # zeros are zeros
        for res in (e.ref, e.f64):
            assert not np.asarray(res.out)[cs.pix < 0].any()
            assert not np.asarray(res.coeff)[e.ref.marks != R.FITTED].any()
        assert not e.ref.S[cs.pix < 0].any()
    assert R.c_count(1, 1) == 16 + 9 + 1 + 2 + 1 + 3 and R.c_count(3, 16) == 16 + 9 + 3 + 32 + 16 + 3


@pytest.mark.parametrize("K,cst", [(2, True), (16, True)])
def test_centring_in_the_stated_order_and_within_the_bound_of_the_long_double_means(K, cst):
    cs = R.case(K, cst, "flagged")                                   # with two values that must stay out of the means
    cen, mu = R.centre_f64(cs.tab, cs.edges)
    mu_ref, S = R.centre_ref(cs.tab, cs.edges)
    c = np.array([R.c_centre(n) for n in cs.lens])[None, :]
    err = np.abs(R._ld(mu) - mu_ref)
    assert (err <= R._ld(c) * U53 * S).all()
    print("means use %.3g of their bound at most" % float((err / np.where(S > 0, R._ld(c) * U53 * S, 1)).max()))
    fin = np.isfinite(cs.tab)
    assert np.array_equal(np.isfinite(cen), fin) and np.isfinite(mu).all()
    for j in range(cs.J):
        want = cs.tab[j] - np.repeat(mu[j], cs.lens)
        assert np.array_equal(R.bits(cen[j][fin[j]]), R.bits(want[fin[j]]))
    # a scalar walk of the order written in cm2_template.hip, on the chunk of 2 S + 3 samples
    ci = cs.lens.index(2 * R.SEG + 3)
    x = cs.tab[0, cs.edges[ci]:cs.edges[ci + 1]]
    lanes = []
    for t in range(R.THREADS):
        acc = 0.0
        for q in range(t, len(x), R.THREADS):
            acc += x[q]
        lanes.append(acc)
    waves = []
    for w in range(4):
        v = lanes[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            v = [v[i] + v[i + off] if i + off < len(v) else v[i] for i in range(len(v))]
        waves.append(v[0])
    total = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert float(total / len(x)).hex() == float(mu[0, ci]).hex()


def test_reference_is_idempotent_and_removes_what_the_templates_span():
    K, cst = 9, True
    cs, e = R.case(K, cst), R.case_eval(K, cst)
    Fr = lambda v: R.template_ref(e.T, cs.pix, cs.ndet, cs.edges, v, e.fact_ref)
    again, grown = Fr(e.ref.out), Fr(e.ref.S)
    assert R.excess(again.out, e.ref.out, grown.S, 1) <= 1.0
    a = np.random.default_rng(6).standard_normal(K).astype(LD) * 100
    r = Fr(np.tile(R._ld(e.T) @ a, cs.ndet))
    assert R.excess(r.out, np.zeros(cs.nt, dtype=LD), r.S, 1) <= 1.0
    fitted = r.marks == R.FITTED
    assert R.excess(r.coeff[fitted], np.broadcast_to(a, r.coeff.shape)[fitted], r.Sc[fitted], 1) <= 1.0
