// cm2_fit.h -- the small least-squares fit of the time-stream filters (cm2_chunkfit.h for cm2_hwpss.hip and
// cm2_template.hip, cm2_modefit.h for cm2_cmode.hip and cm2_pca.hip), written once: the Cholesky factor with its
// pivot rule, the two triangular solves, the packed lower triangle and the rule of an edge list.  Plain C++17 with
// no HIP include of its own: the kernels inline it, and tests/test_fit_header_cpu.py compiles it with the host compiler and compares it bit for bit with
// tests/_fit_ref.py.
//
// The order of every operation (compile with -ffp-contract=off: every product and every sum is rounded on its own):
//   Factor: G = L L^T, row by row, p_j = G_jj - L_j0^2 - ... - L_j,j-1^2 (left to right); the pivot fails when
//   !(p_j > tau G_jj), that is p_j <= tau G_jj or a NaN; L_jj = sqrt(p_j),
//   L_ij = (G_ij - L_i0 L_j0 - ... - L_i,j-1 L_j,j-1) / L_jj for i > j, the terms subtracted with k ascending.
//   Solve: y_i = (b_i - L_i0 y_0 - ... - L_i,i-1 y_i-1) / L_ii for i = 0..K-1, then
//   c_i = (y_i - L_i+1,i c_i+1 - ... - L_K-1,i c_K-1) / L_ii for i = K-1..0, the terms subtracted left to right.
// The factor goes on after a failed pivot (the lanes of a wave need the instructions anyway); what it computes
// from there on is unspecified and the caller stores none of it.
//
// K is an int, or a std::integral_constant<int, K>: then every loop has a constant trip count and is unrolled, so
// that a register array is never indexed at run time.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#if defined(__HIPCC__)
#define CM2_FIT_FN __host__ __device__ __forceinline__
#define CM2_FIT_UNROLL _Pragma("unroll")
// with a run-time K the loops stay loops, and the compiler would say so for every such caller
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
#else
#define CM2_FIT_FN inline
#define CM2_FIT_UNROLL
#endif

namespace cm2 {
namespace fit {

constexpr int packed(int K) { return K * (K + 1) / 2; }                   // doubles of a lower triangle
constexpr int packed_at(int i, int j) { return i * (i + 1) / 2 + j; }     // entry (i, j), j <= i

// entry (i, j), j <= i, of the two storages of a lower triangle: an array is the packed triangle (in registers
// when every index is a constant), a RowMajor the rows of a K x K array
struct RowMajor {
    double *a;
    int K;
};
template <int N>
CM2_FIT_FN double &at(double (&a)[N], int i, int j) { return a[packed_at(i, j)]; }
CM2_FIT_FN double &at(const RowMajor &m, int i, int j) { return m.a[i * m.K + j]; }

// the lower triangle of G becomes L; true when a pivot failed the test
template <class KT, class Mat>
CM2_FIT_FN bool factor(KT K, Mat &G, double tau)
{
    const int n = K;
    bool failed = false;
    CM2_FIT_UNROLL
    for (int j = 0; j < n; ++j) {
        const double gjj = at(G, j, j);
        double pv = gjj;
        CM2_FIT_UNROLL
        for (int k = 0; k < j; ++k) pv -= at(G, j, k) * at(G, j, k);
        failed = failed || !(pv > tau * gjj);
        const double ljj = std::sqrt(pv);
        at(G, j, j) = ljj;
        CM2_FIT_UNROLL
        for (int i = j + 1; i < n; ++i) {
            double t = at(G, i, j);
            CM2_FIT_UNROLL
            for (int k = 0; k < j; ++k) t -= at(G, i, k) * at(G, j, k);
            at(G, i, j) = t / ljj;
        }
    }
    return failed;
}

// b (in y) becomes c
template <class KT, class Mat, class Vec>
CM2_FIT_FN void solve(KT K, Mat &L, Vec &y)
{
    const int n = K;
    CM2_FIT_UNROLL
    for (int i = 0; i < n; ++i) {
        double a = y[i];
        CM2_FIT_UNROLL
        for (int k = 0; k < i; ++k) a -= at(L, i, k) * y[k];
        y[i] = a / at(L, i, i);
    }
    CM2_FIT_UNROLL
    for (int i = n - 1; i >= 0; --i) {
        double a = y[i];
        CM2_FIT_UNROLL
        for (int k = i + 1; k < n; ++k) a -= at(L, k, i) * y[k];
        y[i] = a / at(L, i, i);
    }
}

// 0 = e[0] < e[1] < ... < e[n] = N, which allows no more than N parts
inline bool edges_ok(const int64_t *e, int64_t n, int64_t N)
{
    if (n > N || e[0] != 0 || e[n] != N) return false;
    for (int64_t i = 0; i < n; ++i)
        if (e[i + 1] <= e[i]) return false;
    return true;
}

}  // namespace fit
}  // namespace cm2

#if defined(__HIPCC__)
#pragma clang diagnostic pop
#endif
