// cm2_modefit.h -- the per-sample mode fit of the common-mode filter (cm2_cmode.hip) and the PCA filter
// (cm2_pca.hip), written once: per (group, time sample) unit, fit and remove K templates Phi[k, 0..K-1] across the
// unflagged detectors k of the group.  The two filters differ in where a thread finds its unit and in which Phi it
// reads; each fills a Frame with that and hands it to apply, coefficients or classify.  cm2_modefit_policy.h has the
// constants and the classes; the host helpers of the two handles are at the end.
//
// One thread per unit, 256 threads a workgroup, consecutive lanes on consecutive samples of one group: for every
// detector a wave reads 512 contiguous bytes of v and 256 of pix, and Phi[k, :] is the same for the whole wave.
// Everything of a unit lives in the registers of its thread: the lower triangle of G (K (K + 1) / 2 doubles, the
// factor overwrites it), b (y and then c overwrite it) and the count m.  K is a template parameter, every loop over
// the templates is unrolled, so no array is indexed at run time.
//
// The order of every operation (the unit is compiled with -ffp-contract=off: every product and sum is rounded on
// its own; no floating-point atomic, no cross-lane sum):
//   1. G_ab (a >= b) and b_a start at 0; the unflagged detectors of the group in ascending k:
//      G_ab += Phi_ka Phi_kb,  b_a += Phi_ka v[k, i].
//   2. Factor, skip test and the two solves of cm2_fit.h, which has the order of their operations; the unit is
//      skipped when a pivot fails with tau = CM2_CMODE_TAU = CM2_PCA_TAU (or when m < K).
//   3. p = c_0 Phi_k0, then p += c_j Phi_kj for j = 1..K-1; out[k, i] = v[k, i] - p on an unflagged sample, 0 on a
//      flagged one and on every sample of a skipped unit.
// A thread reads its whole column for step 1 before its first store and touches no other column: out may be v itself.
#pragma once
#include "cm2_common.h"
#include "cm2_modefit_policy.h"

namespace cm2 {
namespace modefit {

// what a thread needs about its unit: sample i of group g (live = false: the thread has none), the detectors [k0, k1).
// live is a flag of its own, computed by each filter's my_unit in that filter's way (i < ns; i >= 0 after i = -1), and
// classify takes a callable, because one sentinel in i for both and a Frame found before the tally change what the
// compiler makes of the kernels, measurably for the common-mode apply (profiles/cmode_filter.md, last section).
struct Frame {
    bool live;
    int64_t ns, g, i;
    int k0, k1;
    const double *phi;              // [ndet][K], the table this unit fits
    const int32_t *pix;             // [ndet ns]
};

// detectors whose loads a thread keeps in flight: a unit is a serial walk over its detectors, and with few time
// samples there are few threads, so the memory parallelism has to come from inside the walk
template <int K>
constexpr int kAhead = K <= 6 ? 8 : 4;

template <int K>
using KConst = std::integral_constant<int, K>;

// step 1.  WITH_B = false: G and m only (the class of a unit depends on Phi and the flags alone)
template <int K, bool WITH_B>
__device__ __forceinline__ int gram(const Frame &u, const double *v, double (&G)[packed(K)], double (&b)[K])
{
#pragma unroll
    for (int e = 0; e < packed(K); ++e) G[e] = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) b[a] = 0.0;
    int m = 0;
    auto take = [&](int k, int32_t px, double x) {
        if (px >= 0) {
            const double *__restrict__ ph = u.phi + (int64_t)k * K;
            ++m;
#pragma unroll
            for (int a = 0; a < K; ++a) {
                const double fa = ph[a];
#pragma unroll
                for (int c = 0; c <= a; ++c) G[packed_at(a, c)] += fa * ph[c];
                if (WITH_B) b[a] += fa * x;
            }
        }
    };
    // the loads of kAhead<K> detectors are issued before the first of them is used; the order of the sums is k's
    int k = u.k0;
    for (; k + kAhead<K> <= u.k1; k += kAhead<K>) {
        int32_t px[kAhead<K>];
        double x[kAhead<K>];
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) {
            const int64_t at = (int64_t)(k + j) * u.ns + u.i;
            px[j] = u.pix[at];
            x[j] = WITH_B ? v[at] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) take(k + j, px[j], x[j]);
    }
    for (; k < u.k1; ++k) {
        const int64_t at = (int64_t)k * u.ns + u.i;
        take(k, u.pix[at], WITH_B ? v[at] : 0.0);
    }
    return m;
}

__device__ __forceinline__ int class_of(int m, int K, bool failed)
{
    return m == 0 ? kEmpty : m < K ? kFew : failed ? kPivot : kFitted;
}

// steps 1 and 2 of a unit: its class, and c when it is fitted
template <int K>
__device__ __forceinline__ int fit_unit(const Frame &u, const double *v, double tau, double (&c)[K])
{
    double G[packed(K)];
    const int m = gram<K, true>(u, v, G, c);
    if (m < K) return class_of(m, K, false);
    if (fit::factor(KConst<K>{}, G, tau)) return kPivot;
    fit::solve(KConst<K>{}, G, c);
    return kFitted;
}

// steps 1 to 3.  v and out are not __restrict__: they may be the same array
template <int K>
__device__ __forceinline__ void apply(const Frame &u, double tau, const double *v, double *out)
{
    if (!u.live) return;
    double c[K];
    const int cls = fit_unit<K>(u, v, tau, c);
    if (cls != kFitted) {
        for (int k = u.k0; k < u.k1; ++k) out[(int64_t)k * u.ns + u.i] = 0.0;
        return;
    }
    auto residual = [&](int k, int32_t px, double x) {
        double o = 0.0;
        if (px >= 0) {
            const double *__restrict__ ph = u.phi + (int64_t)k * K;
            double p = c[0] * ph[0];
#pragma unroll
            for (int j = 1; j < K; ++j) p += c[j] * ph[j];
            o = x - p;
        }
        return o;
    };
    int k = u.k0;
    for (; k + kAhead<K> <= u.k1; k += kAhead<K>) {
        int32_t px[kAhead<K>];
        double x[kAhead<K>];
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) {
            const int64_t at = (int64_t)(k + j) * u.ns + u.i;
            px[j] = u.pix[at];
            x[j] = v[at];
        }
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) out[(int64_t)(k + j) * u.ns + u.i] = residual(k + j, px[j], x[j]);
    }
    for (; k < u.k1; ++k) {
        const int64_t at = (int64_t)k * u.ns + u.i;
        out[at] = residual(k, u.pix[at], v[at]);
    }
}

// coeff[(g K + j) ns + i] = c_j of unit (g, i), 0 for a skipped unit.  (The kernels declare their pointers
// __restrict__; here and in classify that would only scope the promise to the inlined body.)
template <int K>
__device__ __forceinline__ void coefficients(const Frame &u, double tau, const double *v, double *coeff)
{
    if (!u.live) return;
    double c[K];
    const int cls = fit_unit<K>(u, v, tau, c);
#pragma unroll
    for (int j = 0; j < K; ++j) coeff[(u.g * K + j) * u.ns + u.i] = cls == kFitted ? c[j] : 0.0;
}

// status[g ns + i] = the class of unit (g, i); counts[0..3] += the units of each class (integer atomics: LDS first,
// then one per class and workgroup).  Every thread of the workgroup calls it, with or without a unit; find() gives the
// thread's Frame and is called once the tally is zeroed.
template <int K, class Find>
__device__ __forceinline__ void classify(Find &&find, double tau, uint8_t *status, unsigned long long *counts)
{
    __shared__ unsigned int tally[4];
    if (threadIdx.x < 4) tally[threadIdx.x] = 0u;
    __syncthreads();
    const Frame u = find();
    if (u.live) {
        double G[packed(K)], unused[K];
        const int m = gram<K, false>(u, nullptr, G, unused);
        const bool failed = m >= K ? fit::factor(KConst<K>{}, G, tau) : false;
        const int cls = class_of(m, K, failed);
        status[u.g * u.ns + u.i] = (uint8_t)cls;
        atomicAdd(&tally[cls], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 4 && tally[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// ------------------------------------------------------------------ host side ----
inline bool apply_ok(const double *in, const double *out, int64_t nt)
{
    return apply_ok((uint64_t)reinterpret_cast<uintptr_t>(in), (uint64_t)reinterpret_cast<uintptr_t>(out), nt);
}

// the classes of every unit: launch_class(K) launches the class kernel of K on st with d_counts[4] as its counters;
// nclass[c] = the units of class c when this returns
template <class F>
inline int count_classes(int K, F &&launch_class, unsigned long long *d_counts, hipStream_t st, int64_t (&nclass)[4])
{
    CM2_HIP(hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), st));
    dispatch_int<1, kMaxK>(K, launch_class);
    CM2_LAUNCH_OK();
    unsigned long long got[4];
    CM2_HIP(cm2::download(got, d_counts, sizeof(got), st));
    CM2_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < 4; ++c) nclass[c] = (int64_t)got[c];
    return 0;
}

// the refusals of a create that both filters word alike.  ps is the Status of either policy: kBadK and kBadEdges have
// the same values in both (cm2_pca_policy.h asserts it); no other value may be compared here, the enums differ above 3
inline int check_create_status(const char *who, int ps, int ndet, int ngroups, int K)
{
    CM2_CHECK(ps != kBadK, "%s: K=%d outside [1, %d]", who, K, kMaxK);
    CM2_CHECK(ps != kBadEdges, "%s: the %d group edges must ascend strictly from 0 to ndet=%d", who, ngroups + 1, ndet);
    return 0;
}

// the classes a handle holds, to the caller's device array
inline int copy_status(uint8_t *d_dst, const uint8_t *d_src, int64_t units)
{
    CM2_HIP(hipMemcpyAsync(d_dst, d_src, (size_t)units, hipMemcpyDeviceToDevice, nullptr));
    CM2_HIP(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace modefit
}  // namespace cm2
