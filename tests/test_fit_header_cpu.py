"""
csrc/cm2_fit.h without a GPU: the header is compiled with the host compiler into a driver that calls the very
functions the kernels inline -- the factor and the two solves with a compile-time K on a packed array (as
cm2_cmode.hip does) and with a run-time K on the rows of a K x K array (as cm2_hwpss.hip does) -- and both are
compared bit for bit with the NumPy restatement tests/_fit_ref.py.  edges_ok against the Python rule.
"""
import os
import subprocess

import numpy as np
import pytest

import _fit_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmomap2_amd", "csrc")
KS = (1, 2, 3, 10, 17)               # no inner loop; small; the common-mode maximum; the HWPSS maximum

DRIVER = r"""
#include "cm2_fit.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
namespace fit = cm2::fit;

static void print(bool failed, int K, const double *L, const double *c)
{
    printf("%d", failed ? 1 : 0);
    for (int e = 0; e < fit::packed(K); ++e) printf(" %a", L[e]);
    for (int i = 0; i < K; ++i) printf(" %a", c[i]);
    printf("\n");
}

// K a compile-time constant, the packed triangle in an array: cm2_cmode.hip
template <int K>
static void fixed(const std::vector<double> &G, const std::vector<double> &b, double tau)
{
    double L[fit::packed(K)], c[K];
    for (int i = 0; i < K; ++i) {
        c[i] = b[i];
        for (int j = 0; j <= i; ++j) L[fit::packed_at(i, j)] = G[i * K + j];
    }
    const bool failed = fit::factor(std::integral_constant<int, K>{}, L, tau);
    fit::solve(std::integral_constant<int, K>{}, L, c);
    print(failed, K, L, c);
}

// K a run-time value, the factor on the rows of a K x K array, the solves on the packed copy: cm2_hwpss.hip
static void by_value(int K, std::vector<double> G, const std::vector<double> &b, double tau)
{
    double L[fit::packed(17)], c[17];
    const fit::RowMajor rows{G.data(), K};
    const bool failed = fit::factor(K, rows, tau);
    for (int i = 0; i < K; ++i) {
        c[i] = b[i];
        for (int j = 0; j <= i; ++j) L[fit::packed_at(i, j)] = G[i * K + j];
    }
    fit::solve(K, L, c);
    print(failed, K, L, c);
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "edges")) {          // driver edges N e0 e1 ...
        std::vector<int64_t> e;
        for (int i = 3; i < argc; ++i) e.push_back(atoll(argv[i]));
        printf("%d\n", fit::edges_ok(e.data(), (int64_t)e.size() - 1, atoll(argv[2])) ? 1 : 0);
        return 0;
    }
    if (argc < 3) return 2;                                // driver K tau G_00 G_01 ... G_K-1,K-1 b_0 ... b_K-1
    const int K = atoi(argv[1]);
    const double tau = strtod(argv[2], nullptr);
    if (K < 1 || K > 17 || argc != 3 + K * K + K) return 2;
    std::vector<double> G, b;
    for (int e = 0; e < K * K; ++e) G.push_back(strtod(argv[3 + e], nullptr));
    for (int i = 0; i < K; ++i) b.push_back(strtod(argv[3 + K * K + i], nullptr));
    switch (K) {
        case 1: fixed<1>(G, b, tau); break;
        case 2: fixed<2>(G, b, tau); break;
        case 3: fixed<3>(G, b, tau); break;
        case 10: fixed<10>(G, b, tau); break;
        case 17: fixed<17>(G, b, tau); break;
        default: return 2;
    }
    by_value(K, G, b, tau);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("fit_header")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, str(src),
                           "-o", exe])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True)
    return [ln.split() for ln in p.stdout.splitlines()]


def gram(K, kind, rng):
    """G = A^T A in float64 and a right-hand side.  full: A random of 4 K rows; duplicate: its second column a
    copy of the first; short: K - 1 rows"""
    A = rng.standard_normal((K - 1 if kind == "short" else 4 * K, K))
    if kind == "duplicate":
        A[:, 1] = A[:, 0]
    return A.T @ A, rng.standard_normal(K) * 10.0


CASES = [(K, kind) for K in KS for kind in ("full", "duplicate", "short") if kind == "full" or K >= 2]


@pytest.mark.parametrize("K,kind", CASES)
def test_factor_and_solves_match_the_restatement_bit_for_bit(driver, K, kind):
    G, b = gram(K, kind, np.random.default_rng(100 * K + len(kind)))
    ch = F.cholesky(G[None], np.float64)
    assert not ch.near[0], ch.ratio[0]                               # the skip decision does not rest on rounding
    assert bool(ch.failed[0]) == (kind != "full")
    c = F.solve(ch.L, b[None])[0]
    want = np.concatenate([ch.L[0][np.tril_indices(K)], c])          # (row-major lower triangle = the packed order)
    rows = _run(driver, K, float(F.TAU).hex(), *[float(x).hex() for x in np.concatenate([G.reshape(-1), b])])
    assert len(rows) == 2                                            # compile-time K, run-time K
    for row in rows:
        assert int(row[0]) == int(ch.failed[0])
        got = np.array([float.fromhex(x) for x in row[1:]])
        assert got.size == want.size
        if not ch.failed[0]:                                         # after a failed pivot nothing is specified
            assert np.array_equal(F.bits(got), F.bits(want)), (K, kind)


# the refusal cases of test_hwpss_cpu.py::test_plan_refusals and test_cmode_cpu.py::test_policy_refusals that reach
# the edge rule, and lists that pass it
EDGES = [(10, [0, 9]), (10, [1, 10]), (10, [0, 5, 5, 10]), (10, [0, 7, 3, 10]), (10, [0, 10]),
         (4, [0, 3]), (4, [1, 4]), (4, [0, 2, 2, 4]), (4, [0, 3, 1, 4]), (2, [0, 1, 1, 2]), (4, [0, 4]),
         (20, [0, 1, 4, 8, 20]), (3, [0, 1, 2, 3]), (1 << 40, [0, 1 << 40]), (1 << 30, [0, 1 << 16])]


def test_edges_ok_is_the_python_rule(driver):
    seen = set()
    for N, e in EDGES:
        got = int(_run(driver, "edges", N, *e)[0][0])
        assert got == int(F.edges_ok(e, N)), (N, e)
        seen.add(got)
    assert seen == {0, 1}
