// cm2_ground_exact.hip -- G^T v of the ground template as exact integer sums: the same bits for every order of the
// samples, every grid and every run (include/cosmomap2.h states the contract, cm2_ground_exact_policy.h has the
// arithmetic).  It replaces the serial loop of the reference (linearoperators.py:394-400) where k_ground_bin of
// cm2_filter.hip adds fp64 terms in an order that changes from run to run.
//
//   k_gsum_absmax      M = max over the counted samples of the bit pattern of |v|: one 64-bit atomicMax per workgroup
//   k_gsum_bin_lds     nbins <= 2048: three 64-bit limb histograms per workgroup in LDS (ds_add_u64), the non-zero
//                      entries then added to the global limbs
//   k_gsum_bin_global  any nbins: the limbs added straight to the global limbs
//   k_gsum_finish      one thread per bin: the three limbs to one fp64, rounded once
// Integer adds are exact, so the limbs do not depend on the order in which the atomics arrive.  The scale e is read
// from the device word M by every kernel: no host round trip.  The limbs are kept plane by plane, [3][nbins], so
// that a workgroup's flush of a plane is a contiguous stream.
#include "cm2_common.h"
#include "cm2_ground_exact_policy.h"

using namespace cm2;
namespace gs = cm2::gsum;

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_gsum_absmax(int64_t nt, int nbins, const int32_t *__restrict__ bin,
                                                      const double *__restrict__ v, u64 *__restrict__ scale)
{
    __shared__ u64 part[4];
    u64 m = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride)
        if ((uint32_t)bin[i] < (uint32_t)nbins) {
            const u64 b = gs::abs_bits(v[i]);
            m = b > m ? b : m;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = part[w] > m ? part[w] : m;
        if (m) atomicMax(scale, m);
    }
}

__global__ __launch_bounds__(256) void k_gsum_bin_lds(int64_t nt, int nbins, const int32_t *__restrict__ bin,
                                                       const double *__restrict__ v, const u64 *__restrict__ scale,
                                                       u64 *__restrict__ limbs)
{
    extern __shared__ u64 gsum_acc[];               // [3][nbins]
    const u64 M = *scale;
    if (gs::kind_of(M) != gs::kFinite) return;      // all +0.0 or all NaN: k_gsum_finish needs no limbs
    const int e = gs::exponent_of(M);
    for (int i = threadIdx.x; i < 3 * nbins; i += 256) gsum_acc[i] = 0;
    __syncthreads();
    const int64_t per = (nt + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = per * blockIdx.x, b1 = (b0 + per < nt) ? b0 + per : nt;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
        const int32_t g = bin[i];
        if ((uint32_t)g >= (uint32_t)nbins) continue;
        int64_t l[3];
        gs::limbs(v[i], e, l);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (l[k]) atomicAdd(&gsum_acc[k * nbins + g], (u64)l[k]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * nbins; i += 256) {
        const u64 a = gsum_acc[i];
        if (a) atomicAdd(&limbs[i], a);
    }
}

__global__ __launch_bounds__(256) void k_gsum_bin_global(int64_t nt, int nbins, const int32_t *__restrict__ bin,
                                                          const double *__restrict__ v,
                                                          const u64 *__restrict__ scale, u64 *__restrict__ limbs)
{
    const u64 M = *scale;
    if (gs::kind_of(M) != gs::kFinite) return;
    const int e = gs::exponent_of(M);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const int32_t g = bin[i];
        if ((uint32_t)g >= (uint32_t)nbins) continue;
        int64_t l[3];
        gs::limbs(v[i], e, l);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (l[k]) atomicAdd(&limbs[(int64_t)k * nbins + g], (u64)l[k]);
    }
}

__global__ __launch_bounds__(256) void k_gsum_finish(int nbins, const u64 *__restrict__ scale,
                                                      const u64 *__restrict__ limbs, double *__restrict__ sums)
{
    const u64 M = *scale;
    const gs::Kind kind = gs::kind_of(M);
    const int e = gs::exponent_of(M);
    const int stride = gridDim.x * blockDim.x;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nbins; b += stride) {
        double r = 0.0;
        if (kind == gs::kPoisoned) r = gs::from_bits(gs::kNanBits);
        else if (kind == gs::kFinite)
            r = gs::round_sum((int64_t)limbs[b], (int64_t)limbs[(int64_t)nbins + b],
                              (int64_t)limbs[2 * (int64_t)nbins + b], e);
        sums[b] = r;
    }
}

}  // namespace

// (tests/test_ground_exact_cpu.py mirrors these two members to meet the refusals of apply without a device)
struct cm2_ground_sums {
    int nbins = 0;
    u64 *d_state = nullptr;           // [3 nbins] limbs, plane by plane, then the scale word M
};

static size_t state_bytes(int nbins) { return sizeof(u64) * (3 * (size_t)nbins + 1); }
static size_t lds_bytes(int nbins) { return nbins <= gs::kLdsBins ? sizeof(u64) * 3 * (size_t)nbins : 0; }

extern "C" int cm2_ground_sums_destroy(cm2_ground_sums *h)
{
    if (!h) return 0;
    cm2::dev_release(h->d_state);
    delete h;
    return 0;
}

static int sums_alloc(cm2_ground_sums *h)
{
    CM2_HIP(cm2::dev_malloc(&h->d_state, state_bytes(h->nbins)));
    return 0;
}

extern "C" int cm2_ground_sums_create(cm2_ground_sums **out, int nbins, void *stream)
{
    CM2_CHECK(out, "cm2_ground_sums_create: NULL output handle");
    *out = nullptr;
    CM2_CHECK(nbins >= 1, "cm2_ground_sums_create: nbins=%d < 1", nbins);
    (void)stream;                     // apply clears the state itself: nothing to queue here
    cm2_ground_sums *h = new cm2_ground_sums();
    h->nbins = nbins;
    if (int rc = sums_alloc(h)) {
        cm2_ground_sums_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_ground_sums_info(const cm2_ground_sums *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_ground_sums_info: NULL argument");
    h_info[0] = h->nbins;
    h_info[1] = gs::kLdsBins;
    h_info[2] = (int64_t)lds_bytes(h->nbins);
    h_info[3] = h->nbins <= gs::kLdsBins ? 1 : 2;
    return 0;
}

extern "C" int cm2_ground_sums_apply(cm2_ground_sums *h, int64_t nt, const int32_t *d_bin, const double *d_v,
                                     int route, double *d_sums, void *stream)
{
    CM2_CHECK(h && d_sums, "cm2_ground_sums_apply: NULL argument");
    CM2_CHECK(nt >= 0, "cm2_ground_sums_apply: nt=%lld < 0", (long long)nt);
    CM2_CHECK(nt < gs::kMaxSamples, "cm2_ground_sums_apply: nt=%lld is not below 2^31: the 64-bit limb sums could "
              "overflow", (long long)nt);
    CM2_CHECK(route >= 0 && route <= 2, "cm2_ground_sums_apply: route=%d (0 auto, 1 LDS, 2 global)", route);
    CM2_CHECK(route != 1 || h->nbins <= gs::kLdsBins, "cm2_ground_sums_apply: route=1 (LDS) holds at most %d bins, "
              "the handle has nbins=%d", gs::kLdsBins, h->nbins);
    CM2_CHECK(nt == 0 || (d_bin && d_v), "cm2_ground_sums_apply: NULL sample array");
    hipStream_t st = as_stream(stream);
    const int nbins = h->nbins;
    u64 *limbs = h->d_state, *scale = h->d_state + 3 * (size_t)nbins;
    CM2_HIP(hipMemsetAsync(h->d_state, 0, state_bytes(nbins), st));
    if (nt > 0) {
        k_gsum_absmax<<<grid_for(nt), kBlock, 0, st>>>(nt, nbins, d_bin, d_v, scale);
        CM2_LAUNCH_OK();
        if (route == 0) route = nbins <= gs::kLdsBins ? 1 : 2;
        if (route == 1) {
            // a workgroup takes 16384 samples or more, so that its flush of up to 3 nbins atomics stays small beside
            // its binning; three workgroups of 48 KB fit the LDS of a CU
            const int grid = grid_for(nt, 256 * 64, kNumCU * 3);
            k_gsum_bin_lds<<<grid, 256, lds_bytes(nbins), st>>>(nt, nbins, d_bin, d_v, scale, limbs);
        } else {
            k_gsum_bin_global<<<grid_for(nt), kBlock, 0, st>>>(nt, nbins, d_bin, d_v, scale, limbs);
        }
        CM2_LAUNCH_OK();
    }
    k_gsum_finish<<<grid_for(nbins), kBlock, 0, st>>>(nbins, scale, limbs, d_sums);
    CM2_LAUNCH_OK();
    return 0;
}
