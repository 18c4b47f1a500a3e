"""
What the per-chunk fit filters share, without a GPU: the segment plan of cm2_chunkfit_policy.h compiled with the host
compiler against _hwpss_ref.segments_of and plain Python, its refusals against those of cm2_hwpss_policy.h and
cm2_template_policy.h for the same sizes and edges, and that the two policies use its constants, not copies.
"""
import os
import subprocess

import numpy as np
import pytest

import _hwpss_ref as R
import _template_ref as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
OK, BAD_SIZE, BAD_EDGES, TOO_LARGE = 0, 1, 2, 3

DRIVER = r"""
#include "cm2_chunkfit_policy.h"
#include "cm2_hwpss_policy.h"
#include "cm2_template_policy.h"
#include <cstdio>
#include <cstdlib>
namespace cf = cm2::chunkfit;
namespace hp = cm2::hwpss;
namespace tp = cm2::tmpl;
// the same objects, not equal copies
constexpr bool same(const int &a, const int &b) { return &a == &b; }
static_assert(same(hp::kSeg, cf::kSeg) && same(tp::kSeg, cf::kSeg), "kSeg");
static_assert(same(hp::kThreads, cf::kThreads) && same(tp::kThreads, cf::kThreads), "kThreads");
static_assert(same(hp::kPer, cf::kPer) && same(tp::kPer, cf::kPer), "kPer");
static_assert(!same(hp::kMaxK, tp::kMaxK), "same() tells two constants apart");
static_assert(hp::kFew == cf::kFew && tp::kPivot == cf::kPivot && hp::kFitted == tp::kFitted, "marks");
int main(int argc, char **argv)
{
    // driver ns ndet e0 e1 ...
    if (argc < 4) return 2;
    printf("%d %d %d %d %d %d\n", cf::kSeg, cf::kThreads, cf::kPer, (int)cf::kFitted, (int)cf::kFew, (int)cf::kPivot);
    printf("%d %d %d %d\n", (int)cf::kGeomOk, (int)cf::kGeomSize, (int)cf::kGeomEdges, (int)cf::kGeomLimit);
    std::vector<int64_t> e;
    for (int i = 3; i < argc; ++i) e.push_back(atoll(argv[i]));
    const int64_t ns = atoll(argv[1]), ndet = atoll(argv[2]), nchunks = (int64_t)e.size() - 1;
    cf::Geometry g;
    hp::Plan h;
    tp::Plan t;
    const cf::GeomStatus st = cf::make_geometry(&g, ns, ndet, nchunks, e.data());
    printf("%d %d %d\n", (int)st, (int)hp::make_plan(&h, ns, ndet, nchunks, e.data(), 4),
           (int)tp::make_plan(&t, ns, ndet, nchunks, e.data(), 1, 1));
    if (st != cf::kGeomOk) return 0;
    printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)g.ns, (long long)g.ndet, (long long)g.nchunks,
           (long long)g.nt, (long long)g.segs_per_det, (long long)g.nsegs, (long long)g.nunits);
    for (size_t c = 0; c < g.edges.size(); ++c) printf("%lld ", (long long)g.edges[c]);
    printf("\n");
    for (size_t c = 0; c < g.seg_first.size(); ++c) printf("%lld ", (long long)g.seg_first[c]);
    printf("\n");
    for (int64_t r = 0; r < g.segs_per_det; ++r) {
        int64_t t0, t1, a0, a1, b0, b1;
        cf::segment_range(g, r, &t0, &t1);
        hp::segment_range(h, r, &a0, &a1);            // the plans of the two filters hold the same geometry
        tp::segment_range(t, r, &b0, &b1);
        if (a0 != t0 || a1 != t1 || b0 != t0 || b1 != t1 || h.seg_chunk[(size_t)r] != g.seg_chunk[(size_t)r]) return 3;
        printf("%d %lld %lld\n", (int)g.seg_chunk[(size_t)r], (long long)t0, (long long)t1);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunkfit_policy")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]


def test_constants_are_those_of_the_references(driver):
    out = _run(driver, 10, 1, 0, 10)
    assert out[0] == [R.SEG, R.THREADS, R.PER, RT.FITTED, RT.FEW, RT.PIVOT]
    assert (RT.SEG, RT.THREADS, RT.PER) == (R.SEG, R.THREADS, R.PER) and R.SEG == R.THREADS * R.PER == 4096
    assert out[1] == [OK, BAD_SIZE, BAD_EDGES, TOO_LARGE]


def _edges_of(lens):
    return [0] + [int(x) for x in np.cumsum(lens)]


LENS = (1, R.SEG - 1, R.SEG, R.SEG + 1, 3 * R.SEG + 2)


@pytest.mark.parametrize("ndet,lens", [(1, (n,)) for n in LENS] + [(3, LENS), (2, LENS[::-1]), (5, (R.SEG, 1, R.SEG))])
def test_geometry_and_segment_ranges(driver, ndet, lens):
    edges = _edges_of(lens)
    ns, C = edges[-1], len(lens)
    out = _run(driver, ns, ndet, *edges)
    assert out[2] == [OK, 0, RT.OK]
    nseg = [int(n) for n in R.segments_of(edges)]
    assert nseg == [-(-n // R.SEG) for n in lens]
    first = [0] + [int(x) for x in np.cumsum(nseg)]
    assert out[3] == [ns, ndet, C, ns * ndet, first[-1], ndet * first[-1], ndet * C]
    assert out[4] == edges and out[5] == first
    want = [[c, edges[c] + i * R.SEG, min(edges[c] + (i + 1) * R.SEG, edges[c + 1])]
            for c in range(C) for i in range(nseg[c])]
    assert out[6:] == want
    assert all(0 < t1 - t0 <= R.SEG for _, t0, t1 in want)


@pytest.mark.parametrize("args,status", [
    ((0, 1, 0, 0), BAD_SIZE), ((10, 0, 0, 10), BAD_SIZE), ((10, 1, 10), BAD_SIZE),             # ns, ndet, no chunk
    ((10, 1, 0, 9), BAD_EDGES), ((10, 1, 1, 10), BAD_EDGES),                                   # ends
    ((10, 1, 0, 5, 5, 10), BAD_EDGES), ((10, 1, 0, 7, 3, 10), BAD_EDGES),                      # not strictly ascending
    ((1 << 40, 1, 0, 1 << 40), TOO_LARGE),                                                     # ns
    ((1 << 30, (1 << 16) + 1, 0, 1 << 30), TOO_LARGE),                                         # ndet ns > 2^46
    ((1 << 20, 1 << 23, 0, 1 << 20), TOO_LARGE),                                               # 2^31 segments
    ((1 << 20, 1 << 22, 0, 1 << 20), OK), ((10, 1, 0, 10), OK),
])
def test_refusals_agree_with_the_two_policies(driver, args, status):
    got, hw, tm = _run(driver, *args)[2]
    assert got == status
    # each policy has its own refusals first and then these, in this order
    assert hw == {OK: 0, BAD_SIZE: 2, BAD_EDGES: 3, TOO_LARGE: 4}[status]
    assert tm == {OK: RT.OK, BAD_SIZE: RT.BAD_SIZE, BAD_EDGES: RT.BAD_EDGES, TOO_LARGE: RT.TOO_LARGE}[status]
