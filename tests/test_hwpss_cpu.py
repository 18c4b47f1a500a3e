"""
The HWP-synchronous signal filter without a GPU: the extended-precision reference's own properties on the shared
cases of _hwpss_ref.py, the float64 restatement against it (with the re-measurement of WORST), the condition on the
pivots that keeps the skip decision out of the tolerance, the segment plan of cm2_hwpss_policy.h compiled with the
host compiler, hwpss_plan, the constructor's argument checks and the exported names.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _hwpss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
LD, U53 = R.LD, R.U53
ENTRY_POINTS = ("create", "destroy", "info", "apply", "fit", "tables")


# ------------------------------------------------------------ names and header ----
def test_names_are_exported_and_the_header_declares_the_entry_points():
    import cosmomap2_amd.interfaces as I
    from cosmomap2_amd import _hip, kernel_resources as KR
    assert callable(I.HWPSSFilterLO) and callable(I.hwpss_plan)
    hdr = open(os.path.join(ROOT, "include", "cosmomap2.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint cm2_hwpss_%s\(" % name, hdr), name
        assert "cm2_hwpss_" + name in _hip.PROTOTYPES
    assert re.search(r"#define CM2_HWPSS_TAU 0\.0009765625\b", hdr) and R.TAU == 0.0009765625
    assert re.search(r"#define CM2_HWPSS_MAX_HARM 8\b", hdr)
    assert re.search(r"#define CM2_ABI_VERSION 2\b", hdr)
    assert hdr.index("---- f2b:") < hdr.index("---- f2c:") < hdr.index("---- f3:")
    assert any(re.search(p, "k_hwpss_sums<8>") for p in KR.NO_SPILL)       # the build refuses spills in them
    from cosmomap2_amd import build as B
    assert "cm2_hwpss.hip" not in B.FMA_OK


# ------------------------------------------------------------------ hwpss_plan ----
def test_hwpss_plan():
    from cosmomap2_amd.interfaces import hwpss_plan
    from cosmomap2_amd.linop import ShapeError
    assert hwpss_plan(10).tolist() == [0, 10] and hwpss_plan(10).dtype == np.int64
    assert hwpss_plan(10, 5).tolist() == [0, 5, 10]
    assert hwpss_plan(10, 4).tolist() == [0, 4, 8, 10]              # a shorter last chunk
    assert hwpss_plan(10, 10).tolist() == [0, 10] and hwpss_plan(10, 11).tolist() == [0, 10]
    assert hwpss_plan(10, np.int64(3)).tolist() == [0, 3, 6, 9, 10]
    assert hwpss_plan(10, [0, 1, 10]).tolist() == [0, 1, 10]
    for ns, ch in ((37, None), (37, 5), (37, [0, 30, 37])):
        assert np.array_equal(hwpss_plan(ns, ch), R.hwpss_plan(ns, ch))
    for bad in (0, -3, 2.5, [1, 10], [0, 9], [0, 5, 5, 10], [0, 7, 3, 10]):
        with pytest.raises(ValueError):
            hwpss_plan(10, bad)
    for bad in ([0], [[0, 10]], [0.0, 10.0]):
        with pytest.raises(ShapeError):
            hwpss_plan(10, bad)
    with pytest.raises(ValueError):
        hwpss_plan(0)


def test_arguments_are_refused_before_the_gpu_is_needed():
    from cosmomap2_amd import _hip
    from cosmomap2_amd.interfaces import HWPSSFilterLO
    from cosmomap2_amd.linop import ShapeError
    chi, pix = np.linspace(0.0, 9.0, 50), np.zeros(100, dtype=np.int32)
    for kw in (dict(nharm=0), dict(nharm=9), dict(nharm=2.5), dict(ndet=0), dict(chunks=0), dict(chunks=[0, 60]),
               dict(chunks=[0, 20, 20, 50]), dict(chunks=[3, 50])):
        args = dict(ndet=2, nharm=4)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            HWPSSFilterLO(chi, pix, **args)
        assert str(e.value)
    for a, kw in (((chi, pix), dict(ndet=3)), ((chi, pix[:99]), dict(ndet=2)), ((chi.reshape(5, 10), pix), dict(ndet=2)),
                  ((chi[:0], pix[:0]), dict(ndet=2)), ((chi, pix), dict(ndet=2, chunks=[[0, 50]]))):
        with pytest.raises(ShapeError):
            HWPSSFilterLO(*a, **kw)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            HWPSSFilterLO(chi, pix, ndet=2)


# ------------------------------------------------------- the policy header, on a CPU ----
DRIVER = r"""
#include "cm2_hwpss_policy.h"
#include <cstdio>
#include <cstdlib>
using namespace cm2::hwpss;
int main(int argc, char **argv)
{
    // driver ns ndet nharm e0 e1 ...
    if (argc < 5) return 2;
    printf("%d %d %d %d %d %d %d\n", kSeg, kThreads, kPer, kMaxHarm, kMaxK, packed(kMaxK), packed_at(3, 2));
    std::vector<int64_t> e;
    for (int i = 4; i < argc; ++i) e.push_back(atoll(argv[i]));
    Plan p;
    const Status st = make_plan(&p, atoll(argv[1]), atoll(argv[2]), (int64_t)e.size() - 1, e.data(), atoi(argv[3]));
    printf("%d\n", (int)st);
    if (st != kOk) return 0;
    printf("%lld %lld %lld %lld %d %lld %lld %lld\n", (long long)p.ns, (long long)p.ndet, (long long)p.nchunks,
           (long long)p.nt, p.K, (long long)p.segs_per_det, (long long)p.nsegs, (long long)p.nunits);
    for (size_t c = 0; c < p.seg_first.size(); ++c) printf("%lld ", (long long)p.seg_first[c]);
    printf("\n");
    for (int64_t r = 0; r < p.segs_per_det; ++r) {
        int64_t t0, t1;
        segment_range(p, r, &t0, &t1);
        printf("%d %lld %lld\n", (int)p.seg_chunk[(size_t)r], (long long)t0, (long long)t1);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("hwpss_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_policy_constants(driver):
    out = _run(driver, 10, 1, 1, 0, 10)
    assert out[0] == [R.SEG, R.THREADS, R.PER, R.MAX_HARM, 17, 153, 8]
    assert R.SEG == R.THREADS * R.PER == 4096


@pytest.mark.parametrize("ndet,edges", [
    (1, [0, 1]), (3, [0, R.SEG]), (2, [0, R.SEG + 1]), (5, [0, 3, R.SEG + 2, 3 * R.SEG + 2, 3 * R.SEG + 3]),
    (3, [int(e) for e in R.case(8, "fast").edges]), (3, [int(e) for e in R.case(4, "slow").edges]),
])
def test_segments_tile_every_chunk(driver, ndet, edges):
    ns, C = edges[-1], len(edges) - 1
    out = _run(driver, ns, ndet, 4, *edges)
    assert out[1] == [0]
    nseg = [int(n) for n in R.segments_of(edges)]
    first = [0] + list(np.cumsum(nseg))
    assert out[2] == [ns, ndet, C, ns * ndet, 9, first[-1], ndet * first[-1], ndet * C]
    assert out[3] == first
    rows = out[4:]
    assert len(rows) == first[-1]
    at = 0
    for c in range(C):
        mine = rows[first[c]:first[c + 1]]
        assert all(r[0] == c for r in mine)
        assert mine[0][1] == edges[c] and mine[-1][2] == edges[c + 1]
        assert all(b[1] == a[2] for a, b in zip(mine[:-1], mine[1:]))             # no gap, no overlap
        assert all(r[2] - r[1] == R.SEG for r in mine[:-1]) and 0 < mine[-1][2] - mine[-1][1] <= R.SEG
        at += len(mine)
    assert at == len(rows)


def test_plan_refusals(driver):
    status = lambda *a: _run(driver, *a)[1][0]
    assert status(10, 1, 0, 0, 10) == 1 and status(10, 1, 9, 0, 10) == 1              # nharm
    assert status(0, 1, 4, 0, 0) == 2 and status(10, 0, 4, 0, 10) == 2                # sizes
    assert status(10, 1, 4, 0, 9) == 3 and status(10, 1, 4, 1, 10) == 3               # ends
    assert status(10, 1, 4, 0, 5, 5, 10) == 3 and status(10, 1, 4, 0, 7, 3, 10) == 3  # not strictly ascending
    assert status(1 << 40, 1, 4, 0, 1 << 40) == 4                                     # ns
    assert status(1 << 30, (1 << 16) + 1, 4, 0, 1 << 30) == 4                         # ndet ns > 2^46
    assert status(1 << 20, 1 << 23, 4, 0, 1 << 20) == 4                               # 2^31 segments
    assert status(1 << 20, 1 << 22, 4, 0, 1 << 20) == 0


# -------------------------------------------------- the reference's own properties ----
@pytest.mark.parametrize("H,rate", R.CASES)
def test_case_has_what_the_tests_need(H, rate):
    cs = R.case(H, rate)
    K = cs.K
    assert cs.ndet == 3 and 20000 < cs.ns < 60000 and cs.edges[-1] == cs.ns
    for n in (R.SEG - 1, R.SEG, R.SEG + 1, 2 * R.SEG - 1, 2 * R.SEG, 2 * R.SEG + 1, 64, 257):
        assert n in cs.lens
    assert cs.lens[-1] % R.SEG == 0                                  # the last unit ends at ns on a full segment
    if rate == "fast":
        assert K in cs.lens and K + 1 in cs.lens and 40 in cs.lens
    step = np.diff(cs.chi)
    a, b = cs.edges[cs.stalled], cs.edges[cs.stalled + 1]
    assert np.all(cs.chi[a:b] == cs.chi[a])                          # the stalled plate
    moving = np.delete(step, np.arange(a, b - 1))
    assert abs(np.median(moving) - R.RATES[rate]) < 0.01 and moving.std() > 0 and cs.chi[0] > 9.9e3
    ok = (cs.pix >= 0).reshape(3, cs.ns)
    assert ok[0].all() and 0.25 < 1 - ok[1].mean() < 0.35
    m2 = [int(ok[2, cs.edges[c]:cs.edges[c + 1]].sum()) for c in range(len(cs.lens))]
    assert 0 in m2 and K - 1 in m2
    c3 = cs.lens.index(2 * R.SEG + 1)
    u = ok[2, cs.edges[c3]:cs.edges[c3 + 1]]
    assert not u[:R.SEG].any() and not u[2 * R.SEG:].any() and u[R.SEG:2 * R.SEG].all()
    _, r = R.case_ref(H, rate)
    assert (r.marks == 0).sum() >= 20 and (r.marks[:, cs.stalled] == 2).all() and (r.marks == 1).sum() >= 2


@pytest.mark.parametrize("H,rate", R.CASES)
def test_pivots_are_far_from_the_threshold_in_both_precisions(H, rate):
    fr, _ = R.case_ref(H, rate)
    ff, _ = R.case_f64(H, rate)
    for key in fr:
        assert fr[key].mark == ff[key].mark, key
        for f in (fr[key], ff[key]):
            if f.mark != 1:                                          # m < K is decided by the count alone
                assert f.ratio >= R.PIVOT_OK or f.ratio <= R.PIVOT_GONE, (key, f.ratio)
                assert (f.ratio >= R.PIVOT_OK) == (f.mark == 0)
    assert R.PIVOT_GONE < R.TAU < R.PIVOT_OK


@pytest.mark.parametrize("H,rate", R.CASES)
def test_skipped_units_and_flagged_samples_are_exactly_zero(H, rate):
    cs = R.case(H, rate)
    _, r = R.case_ref(H, rate)
    _, f = R.case_f64(H, rate)
    for res in (r, f):
        out = np.asarray(res.out).reshape(3, cs.ns)
        for k in range(3):
            for c in range(len(cs.lens)):
                if r.marks[k, c]:
                    assert not out[k, cs.edges[c]:cs.edges[c + 1]].any() and not res.coeff[k, c].any()
        assert not np.asarray(res.out)[cs.pix < 0].any()
    assert not r.S[cs.pix < 0].any()
    assert (r.S[cs.pix >= 0] > 0).reshape(-1).sum() == sum(
        int((cs.pix.reshape(3, -1)[k, cs.edges[c]:cs.edges[c + 1]] >= 0).sum())
        for k in range(3) for c in range(len(cs.lens)) if r.marks[k, c] == 0)


@pytest.mark.parametrize("H,rate", [(1, "fast"), (4, "slow"), (8, "fast")])
def test_reference_is_idempotent_and_symmetric(H, rate):
    cs = R.case(H, rate)
    fact, r = R.case_ref(H, rate)
    F = lambda v: R.hwpss_ref(cs.chi, cs.pix, cs.ndet, cs.edges, H, v, fact)
    # F (F v) = F v: what the second application can change is bounded by the magnitude formula applied to S
    again, grown = F(r.out), F(r.S)
    assert R.excess(again.out, r.out, grown.S, 1) <= 1.0
    # <x, F v> = <F x, v>
    x = np.random.default_rng(5).standard_normal(cs.nt)
    fx = F(x)
    lhs, rhs = (R._ld(x) * r.out).sum(), (fx.out * R._ld(cs.v)).sum()
    bound = U53 * ((np.abs(R._ld(x)) * r.S).sum() + (fx.S * np.abs(R._ld(cs.v))).sum())
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("H,rate", R.CASES)
def test_harmonics_plus_a_constant_are_removed(H, rate):
    cs = R.case(H, rate)
    fact, _ = R.case_ref(H, rate)
    a = np.random.default_rng(6).standard_normal(cs.K).astype(LD) * 100
    v = np.tile(R.templates_ld(cs.chi, H) @ a, cs.ndet)             # kept in extended precision
    r = R.hwpss_ref(cs.chi, cs.pix, cs.ndet, cs.edges, H, v, fact)
    assert R.excess(r.out, np.zeros(cs.nt, dtype=LD), r.S, 1) <= 1.0
    fitted = r.marks == 0
    assert R.excess(r.coeff[fitted], np.broadcast_to(a, r.coeff.shape)[fitted], r.Sc[fitted], 1) <= 1.0


# ------------------------------------------------ restatement against reference ----
def test_restatement_against_reference_and_worst():
    worst = max(R.measure_worst(H, rate) for H, rate in R.CASES)
    print("largest |hwpss_f64 - hwpss_ref| / (2^-53 S): %.3f (WORST = %.1f)" % (worst, R.WORST))
    assert worst <= R.WORST <= worst + 0.1                           # the committed constant is the measured one
    assert R.HEADROOM == R.pow2_at_least(8 * R.WORST) == 64
    for H, rate in R.CASES:
        cs = R.case(H, rate)
        _, r = R.case_ref(H, rate)
        _, f = R.case_f64(H, rate)
        assert np.array_equal(r.marks, f.marks)
        # and a fortiori within the bound the GPU is held to, with the factor 8 to spare
        assert R.excess(f.out, r.out, r.S, R.c_samples(cs.ndet, cs.edges, H)) <= 0.125
    assert R.c_count(1, 1) == 0 + 2 + 16 + 9 + 1 + 6 + 3 + 3 and R.c_count(3, 8) == 21 + 2 + 16 + 9 + 3 + 34 + 17 + 3


def test_restatement_sums_in_the_stated_order():
    """unit_sums_f64 against a scalar walk of the order written in cm2_hwpss.hip, on a unit of three segments with
    flags; the magnitudes are spread so that any other order shows"""
    rng = np.random.default_rng(9)
    n = 2 * R.SEG + 77
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    ok = rng.random(n) < 0.7
    total = 0.0
    for s0 in range(0, n, R.SEG):
        lanes = []
        for t in range(R.THREADS):
            acc = 0.0
            for q in range(s0 + t, min(s0 + R.SEG, n), R.THREADS):
                if ok[q]:
                    acc += x[q]
            lanes.append(acc)
        waves = []
        for w in range(4):
            v = lanes[64 * w:64 * w + 64]
            for off in (32, 16, 8, 4, 2, 1):
                v = [v[i] + v[i + off] if i + off < len(v) else v[i] for i in range(len(v))]
            waves.append(v[0])
        total += ((waves[0] + waves[1]) + waves[2]) + waves[3]
    got = R.unit_sums_f64(x[:, None], ok)[0]
    assert got.hex() == float(total).hex()
