// cm2_cmode.hip -- the common-mode filter (CommonModeFilterLO), see include/cosmomap2.h (f2d): per (group, time
// sample) unit, fit and remove K templates Phi[k, 0..K-1] across the unflagged detectors k of the group.
// cm2_cmode_policy.h has the accepted arguments and the launch arithmetic.
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
//      skipped when a pivot fails with tau = CM2_CMODE_TAU (or when m < K).
//   3. p = c_0 Phi_k0, then p += c_j Phi_kj for j = 1..K-1; out[k, i] = v[k, i] - p on an unflagged sample, 0 on a
//      flagged one and on every sample of a skipped unit.
// A thread reads its whole column for step 1 before its first store and touches no other column: out may be v itself.
#include <vector>

#include "cm2_common.h"
#include "cm2_cmode_policy.h"

using namespace cm2;
namespace cp = cm2::cmode;

namespace {

struct Shape {
    int64_t ns, blocks_per_group;
    const int32_t *gedges;          // [ngroups + 1], device
    const double *modes;            // [ndet][K], device
    const int32_t *pix;             // [ndet ns], device, borrowed
};

// the unit of this thread: group g, sample i (i >= ns: none), detectors [k0, k1)
struct Unit {
    int64_t g, i;
    int k0, k1;
};

__device__ __forceinline__ Unit my_unit(const Shape &s)
{
    Unit u;
    u.g = (int64_t)blockIdx.x / s.blocks_per_group;
    u.i = ((int64_t)blockIdx.x - u.g * s.blocks_per_group) * cp::kThreads + threadIdx.x;
    u.k0 = s.gedges[u.g];
    u.k1 = s.gedges[u.g + 1];
    return u;
}

// detectors whose loads a thread keeps in flight: a unit is a serial walk over its detectors, and with few time
// samples there are few threads, so the memory parallelism has to come from inside the walk
template <int K>
constexpr int kAhead = K <= 6 ? 8 : 4;

template <int K>
using KConst = std::integral_constant<int, K>;

// step 1.  WITH_B = false: G and m only (the class of a unit depends on Phi and the flags alone)
template <int K, bool WITH_B>
__device__ __forceinline__ int gram(const Shape &s, const Unit &u, const double *v, double (&G)[cp::packed(K)],
                                    double (&b)[K])
{
#pragma unroll
    for (int e = 0; e < cp::packed(K); ++e) G[e] = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) b[a] = 0.0;
    int m = 0;
    auto take = [&](int k, int32_t px, double x) {
        if (px >= 0) {
            const double *__restrict__ ph = s.modes + (int64_t)k * K;
            ++m;
#pragma unroll
            for (int a = 0; a < K; ++a) {
                const double fa = ph[a];
#pragma unroll
                for (int c = 0; c <= a; ++c) G[cp::packed_at(a, c)] += fa * ph[c];
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
            const int64_t at = (int64_t)(k + j) * s.ns + u.i;
            px[j] = s.pix[at];
            x[j] = WITH_B ? v[at] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) take(k + j, px[j], x[j]);
    }
    for (; k < u.k1; ++k) {
        const int64_t at = (int64_t)k * s.ns + u.i;
        take(k, s.pix[at], WITH_B ? v[at] : 0.0);
    }
    return m;
}

__device__ __forceinline__ int class_of(int m, int K, bool failed)
{
    return m == 0 ? cp::kEmpty : m < K ? cp::kFew : failed ? cp::kPivot : cp::kFitted;
}

// steps 1 and 2 of a unit: its class, and c when it is fitted
template <int K>
__device__ __forceinline__ int fit_unit(const Shape &s, const Unit &u, const double *v, double tau, double (&c)[K])
{
    double G[cp::packed(K)];
    const int m = gram<K, true>(s, u, v, G, c);
    if (m < K) return class_of(m, K, false);
    if (fit::factor(KConst<K>{}, G, tau)) return cp::kPivot;
    fit::solve(KConst<K>{}, G, c);
    return cp::kFitted;
}

// v and out are not __restrict__: they may be the same array
template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_apply(Shape s, double tau, const double *v, double *out)
{
    const Unit u = my_unit(s);
    if (u.i >= s.ns) return;
    double c[K];
    const int cls = fit_unit<K>(s, u, v, tau, c);
    if (cls != cp::kFitted) {
        for (int k = u.k0; k < u.k1; ++k) out[(int64_t)k * s.ns + u.i] = 0.0;
        return;
    }
    auto residual = [&](int k, int32_t px, double x) {
        double o = 0.0;
        if (px >= 0) {
            const double *__restrict__ ph = s.modes + (int64_t)k * K;
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
            const int64_t at = (int64_t)(k + j) * s.ns + u.i;
            px[j] = s.pix[at];
            x[j] = v[at];
        }
#pragma unroll
        for (int j = 0; j < kAhead<K>; ++j) out[(int64_t)(k + j) * s.ns + u.i] = residual(k + j, px[j], x[j]);
    }
    for (; k < u.k1; ++k) {
        const int64_t at = (int64_t)k * s.ns + u.i;
        out[at] = residual(k, s.pix[at], v[at]);
    }
}

// coeff[(g K + j) ns + i] = c_j of unit (g, i), 0 for a skipped unit
template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_fit(Shape s, double tau, const double *__restrict__ v,
                                                             double *__restrict__ coeff)
{
    const Unit u = my_unit(s);
    if (u.i >= s.ns) return;
    double c[K];
    const int cls = fit_unit<K>(s, u, v, tau, c);
#pragma unroll
    for (int j = 0; j < K; ++j) coeff[(u.g * K + j) * s.ns + u.i] = cls == cp::kFitted ? c[j] : 0.0;
}

// status[g ns + i] = the class of unit (g, i); counts[0..3] += the units of each class (integer atomics: LDS first,
// then one per class and workgroup)
template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_class(Shape s, double tau, uint8_t *__restrict__ status,
                                                               unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int tally[4];
    if (threadIdx.x < 4) tally[threadIdx.x] = 0u;
    __syncthreads();
    const Unit u = my_unit(s);
    if (u.i < s.ns) {
        double G[cp::packed(K)], unused[K];
        const int m = gram<K, false>(s, u, nullptr, G, unused);
        const bool failed = m >= K ? fit::factor(KConst<K>{}, G, tau) : false;
        const int cls = class_of(m, K, failed);
        status[u.g * s.ns + u.i] = (uint8_t)cls;
        atomicAdd(&tally[cls], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 4 && tally[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

}  // namespace

struct cm2_cmode {
    cp::Launch launch;
    int64_t ns = 0, ndet = 0, ngroups = 0;
    int K = 0;
    const int32_t *d_pix = nullptr;        // borrowed
    int32_t *d_gedges = nullptr;
    double *d_modes = nullptr;
    uint8_t *d_status = nullptr;
    int64_t nclass[4] = {0, 0, 0, 0};
    Shape shape() const { return Shape{ns, launch.blocks_per_group, d_gedges, d_modes, d_pix}; }
};

extern "C" int cm2_cmode_destroy(cm2_cmode *h)
{
    if (!h) return 0;
    dev_release(h->d_gedges, h->d_modes, h->d_status);
    delete h;
    return 0;
}

namespace {

int cmode_fill(cm2_cmode *h, const int64_t *h_edges, const double *d_modes, hipStream_t st)
{
    std::vector<int32_t> e((size_t)h->ngroups + 1);
    for (size_t g = 0; g < e.size(); ++g) e[g] = (int32_t)h_edges[g];
    if (int rc = dev_put(&h->d_gedges, e.data(), e.size(), st)) return rc;
    const size_t mbytes = sizeof(double) * (size_t)h->ndet * (size_t)h->K;
    CM2_HIP(cm2::dev_malloc(&h->d_modes, mbytes));
    CM2_HIP(hipMemcpyAsync(h->d_modes, d_modes, mbytes, hipMemcpyDeviceToDevice, st));
    CM2_HIP(cm2::dev_malloc(&h->d_status, (size_t)h->launch.units));
    DevTemp<unsigned long long> counts;
    CM2_HIP(counts.alloc(4));
    CM2_HIP(hipMemsetAsync(counts.p, 0, 4 * sizeof(unsigned long long), st));
    dispatch_int<1, cp::kMaxK>(h->K, [&](auto K) {
        k_cmode_class<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, st>>>(h->shape(), CM2_CMODE_TAU,
                                                                                    h->d_status, counts.p);
    });
    CM2_LAUNCH_OK();
    unsigned long long got[4];
    CM2_HIP(cm2::download(got, counts.p, sizeof(got), st));
    CM2_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < 4; ++c) h->nclass[c] = (int64_t)got[c];
    return 0;
}

}  // namespace

extern "C" int cm2_cmode_create(cm2_cmode **out, int64_t ns, int ndet, int ngroups, const int64_t *h_group_edges,
                                int K, const double *d_modes, const int32_t *d_pix, void *stream)
{
    const char *who = "cm2_cmode_create";
    CM2_CHECK(out, "%s: null output handle", who);
    CM2_CHECK(h_group_edges && d_modes && d_pix, "%s: null array", who);
    cp::Launch l;
    const cp::Status ps = cp::check(&l, ns, ndet, ngroups, h_group_edges, K);
    CM2_CHECK(ps != cp::kBadK, "%s: K=%d outside [1, %d]", who, K, cp::kMaxK);
    CM2_CHECK(ps != cp::kBadSize, "%s: ns=%lld, ndet=%d, ngroups=%d must all be >= 1", who, (long long)ns, ndet,
              ngroups);
    CM2_CHECK(ps != cp::kBadEdges, "%s: the %d group edges must ascend strictly from 0 to ndet=%d", who, ngroups + 1,
              ndet);
    CM2_CHECK(ps == cp::kOk, "%s: ns=%lld x ndet=%d in %d groups overflows the index types or the grid", who,
              (long long)ns, ndet, ngroups);
    cm2_cmode *h = new cm2_cmode();
    h->launch = l;
    h->ns = ns;
    h->ndet = ndet;
    h->ngroups = ngroups;
    h->K = K;
    h->d_pix = d_pix;
    const int rc = cmode_fill(h, h_group_edges, d_modes, as_stream(stream));
    if (rc) {
        cm2_cmode_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_cmode_info(const cm2_cmode *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_cmode_info: null argument");
    h_info[0] = h->ns;
    h_info[1] = h->ndet;
    h_info[2] = h->ngroups;
    h_info[3] = h->K;
    for (int c = 0; c < 4; ++c) h_info[4 + c] = h->nclass[c];
    return 0;
}

extern "C" int cm2_cmode_apply(cm2_cmode *h, const double *d_in, double *d_out, void *stream)
{
    CM2_CHECK(h, "cm2_cmode_apply: null handle");
    CM2_CHECK(d_in && d_out, "cm2_cmode_apply: null vector");
    CM2_CHECK(d_in == d_out || !ranges_overlap(d_in, h->launch.nt, d_out, h->launch.nt),
              "cm2_cmode_apply: the output must be the input itself or not overlap it");
    dispatch_int<1, cp::kMaxK>(h->K, [&](auto K) {
        k_cmode_apply<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, as_stream(stream)>>>(
            h->shape(), CM2_CMODE_TAU, d_in, d_out);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_cmode_fit(cm2_cmode *h, const double *d_in, double *d_coeff, void *stream)
{
    CM2_CHECK(h, "cm2_cmode_fit: null handle");
    CM2_CHECK(d_in && d_coeff, "cm2_cmode_fit: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->launch.nt, d_coeff, h->launch.units * h->K),
              "cm2_cmode_fit: the coefficients must not alias the input");
    dispatch_int<1, cp::kMaxK>(h->K, [&](auto K) {
        k_cmode_fit<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, as_stream(stream)>>>(
            h->shape(), CM2_CMODE_TAU, d_in, d_coeff);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_cmode_status(const cm2_cmode *h, uint8_t *d_status)
{
    CM2_CHECK(h && d_status, "cm2_cmode_status: null argument");
    CM2_HIP(hipMemcpyAsync(d_status, h->d_status, (size_t)h->launch.units, hipMemcpyDeviceToDevice, nullptr));
    CM2_HIP(hipStreamSynchronize(nullptr));
    return 0;
}
