// cm2_hwpss.hip -- the HWP-synchronous signal filter (HWPSSFilterLO), see include/cosmomap2.h (f2c): per (detector,
// chunk) unit, fit and remove the harmonics 1, cos(n chi), sin(n chi), n = 1..H, of the plate angle chi on the
// unflagged samples.  cm2_chunkfit.h has the order of every sum, the factor, the solve and the rule of a skipped unit
// (tau = CM2_HWPSS_TAU; m = G_00, the exact count since T_0 = 1); one workgroup per (detector, row segment).
//
// Templates of a sample, from the two tables c1 = cos chi, s1 = sin chi (device sincos, once at create time):
//   T_0 = 1, T_1 = c1, T_2 = s1,  T_{2n-1} = T_{2n-3} c1 - T_{2n-2} s1,  T_{2n} = T_{2n-2} c1 + T_{2n-3} s1   (n >= 2)
// every product and every sum rounded on its own (the unit is compiled with -ffp-contract=off).
//
// Subtract (k_hwpss_subtract): p = c_0, then p += c_{2n-1} T_{2n-1}, p += c_{2n} T_{2n} for n = 1..H; out = v - p on
// an unflagged sample, 0 on a flagged one and on every sample of a skipped unit.
#include "cm2_chunkfit.h"
#include "cm2_hwpss_policy.h"

using namespace cm2;
namespace hp = cm2::hwpss;
namespace cf = cm2::chunkfit;

namespace {

using namespace cm2::chunkfit;      // SegPos, seg_pos, segment_reduce
using PlanDev = GeomDev;

template <int H>
__device__ __forceinline__ void harmonics(double c1, double s1, double (&T)[2 * H + 1])
{
    T[0] = 1.0;
    T[1] = c1;
    T[2] = s1;
#pragma unroll
    for (int n = 2; n <= H; ++n) {
        T[2 * n - 1] = T[2 * n - 3] * c1 - T[2 * n - 2] * s1;
        T[2 * n] = T[2 * n - 2] * c1 + T[2 * n - 3] * s1;
    }
}

__global__ __launch_bounds__(256) void k_hwpss_tables(int64_t ns, const double *__restrict__ chi,
                                                       double *__restrict__ cosv, double *__restrict__ sinv)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += stride) {
        double s, c;
        sincos(chi[i], &s, &c);
        cosv[i] = c;
        sinv[i] = s;
    }
}

// row blockIdx.y of the segment's Gram sums: gp[(b K + row) K + i] = sum over the unflagged samples of T_i T_row
template <int H>
__global__ __launch_bounds__(hp::kThreads) void k_hwpss_gram(PlanDev p, const int32_t *__restrict__ pix,
                                                              const double *__restrict__ cosv,
                                                              const double *__restrict__ sinv,
                                                              double *__restrict__ gp)
{
    constexpr int K = 2 * H + 1;
    const int64_t b = blockIdx.x;
    const int row = blockIdx.y;
    const SegPos s = seg_pos(p, b);
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
#pragma unroll 2
    for (int u = 0; u < hp::kPer; ++u) {
        const int64_t t = s.t0 + threadIdx.x + (int64_t)u * hp::kThreads;
        if (t < s.t1 && pix[s.base + t] >= 0) {
            double T[K];
            harmonics<H>(cosv[t], sinv[t], T);
            double tr = T[0];
#pragma unroll
            for (int j = 1; j < K; ++j) tr = (j == row) ? T[j] : tr;
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j] += T[j] * tr;
        }
    }
    segment_reduce<K>(acc, gp + (b * K + row) * K);
}

// one workgroup of 64 threads per unit: adds the Gram sums of its segments, factorises, marks
__global__ __launch_bounds__(64) void k_hwpss_factor(PlanDev p, int K, double tau, const double *__restrict__ gp,
                                                      double *__restrict__ factor, uint8_t *__restrict__ skip)
{
    // G_00 = the number of unflagged samples, exact
    factor_unit<hp::kMaxK>(p, K, tau, gp, factor, skip, [](const double *G, const UnitSegs &) { return G[0]; });
}

template <int H>
__global__ __launch_bounds__(hp::kThreads) void k_hwpss_sums(PlanDev p, const uint8_t *__restrict__ skip,
                                                              const int32_t *__restrict__ pix,
                                                              const double *__restrict__ v,
                                                              const double *__restrict__ cosv,
                                                              const double *__restrict__ sinv,
                                                              double *__restrict__ partial)
{
    constexpr int K = 2 * H + 1;
    const int64_t b = blockIdx.x;
    const SegPos s = seg_pos(p, b);
    if (skip[s.unit]) return;                          // its sums are never read
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
#pragma unroll 4
    for (int u = 0; u < hp::kPer; ++u) {
        const int64_t t = s.t0 + threadIdx.x + (int64_t)u * hp::kThreads;
        if (t < s.t1) {
            const int32_t px = pix[s.base + t];
            const double x = v[s.base + t], c1 = cosv[t], s1 = sinv[t];
            if (px >= 0) {
                double T[K];
                harmonics<H>(c1, s1, T);
#pragma unroll
                for (int j = 0; j < K; ++j) acc[j] += T[j] * x;
            }
        }
    }
    segment_reduce<K>(acc, partial + b * K);
}

__global__ __launch_bounds__(64) void k_hwpss_solve(PlanDev p, int K, const uint8_t *__restrict__ skip,
                                                     const double *__restrict__ factor,
                                                     const double *__restrict__ partial, double *__restrict__ coeff)
{
    cf::solve_unit<hp::kMaxK>(p, K, skip, factor, partial, coeff);
}

template <int H>
__global__ __launch_bounds__(hp::kThreads) void k_hwpss_subtract(PlanDev p, const uint8_t *__restrict__ skip,
                                                                  const double *__restrict__ coeff,
                                                                  const int32_t *__restrict__ pix,
                                                                  const double *__restrict__ v,
                                                                  const double *__restrict__ cosv,
                                                                  const double *__restrict__ sinv,
                                                                  double *__restrict__ out)
{
    constexpr int K = 2 * H + 1;
    const int64_t b = blockIdx.x;
    const SegPos s = seg_pos(p, b);
    if (skip[s.unit]) {
        for (int64_t t = s.t0 + threadIdx.x; t < s.t1; t += hp::kThreads) out[s.base + t] = 0.0;
        return;
    }
    double c[K];
#pragma unroll
    for (int j = 0; j < K; ++j) c[j] = coeff[s.unit * K + j];
#pragma unroll 4
    for (int u = 0; u < hp::kPer; ++u) {
        const int64_t t = s.t0 + threadIdx.x + (int64_t)u * hp::kThreads;
        if (t < s.t1) {
            const int32_t px = pix[s.base + t];
            const double x = v[s.base + t], c1 = cosv[t], s1 = sinv[t];
            double o = 0.0;
            if (px >= 0) {
                double T[K];
                harmonics<H>(c1, s1, T);
                double pr = c[0];
#pragma unroll
                for (int j = 1; j < K; ++j) pr += c[j] * T[j];
                o = x - pr;
            }
            out[s.base + t] = o;
        }
    }
}

}  // namespace

struct cm2_hwpss {
    hp::Plan plan;
    const int32_t *d_pix = nullptr;       // borrowed
    cf::State state;
    double *d_cos = nullptr, *d_sin = nullptr;
    PlanDev dev() const { return state.dev(plan); }
};

extern "C" int cm2_hwpss_destroy(cm2_hwpss *h)
{
    if (!h) return 0;
    h->state.release();
    dev_release(h->d_cos, h->d_sin);
    delete h;
    return 0;
}

namespace {

int hwpss_fill(cm2_hwpss *h, const double *d_chi, hipStream_t st)
{
    const hp::Plan &p = h->plan;
    const int K = p.K;
    if (int rc = h->state.fill(p, K, st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_cos, sizeof(double) * (size_t)p.ns));
    CM2_HIP(cm2::dev_malloc(&h->d_sin, sizeof(double) * (size_t)p.ns));
    k_hwpss_tables<<<grid_for(p.ns), kBlock, 0, st>>>(p.ns, d_chi, h->d_cos, h->d_sin);
    CM2_LAUNCH_OK();
    DevTemp<double> gp;                                // the Gram sums of every segment: create time only
    CM2_HIP(gp.alloc((size_t)(p.nsegs * K * K)));
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        const dim3 grid((unsigned)p.nsegs, (unsigned)K);
        k_hwpss_gram<H><<<grid, hp::kThreads, 0, st>>>(h->dev(), h->d_pix, h->d_cos, h->d_sin, gp.p);
    });
    CM2_LAUNCH_OK();
    k_hwpss_factor<<<dim3((unsigned)p.nunits), 64, 0, st>>>(h->dev(), K, CM2_HWPSS_TAU, gp, h->state.d_factor,
                                                            h->state.d_skip);
    CM2_LAUNCH_OK();
    return h->state.tally(p, st);
}

}  // namespace

extern "C" int cm2_hwpss_create(cm2_hwpss **out, int64_t ns, int ndet, int64_t nchunks, const int64_t *h_edges,
                                const double *d_chi, const int32_t *d_pix, int nharm, void *stream)
{
    const char *who = "cm2_hwpss_create";
    CM2_CHECK(out, "%s: null output handle", who);
    CM2_CHECK(h_edges && d_chi && d_pix, "%s: null array", who);
    cm2_hwpss *h = new cm2_hwpss();
    const hp::Status ps = hp::make_plan(&h->plan, ns, ndet, nchunks, h_edges, nharm);
    if (ps != hp::kOk) {
        delete h;
        CM2_CHECK(ps != hp::kBadHarm, "%s: nharm=%d outside [1, %d]", who, nharm, hp::kMaxHarm);
        return cf::check_create_status(who, ps, hp::kBadSize, ns, ndet, nchunks);
    }
    h->d_pix = d_pix;
    const int rc = hwpss_fill(h, d_chi, as_stream(stream));
    if (rc) {
        cm2_hwpss_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_hwpss_info(const cm2_hwpss *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_hwpss_info: null argument");
    h_info[0] = h->plan.ns;
    h_info[1] = h->plan.ndet;
    h_info[2] = h->plan.nchunks;
    h_info[3] = h->plan.nharm;
    h_info[4] = h->state.nmark[0];
    h_info[5] = h->state.nmark[1];
    h_info[6] = h->state.nmark[2];
    h_info[7] = hp::kSeg;
    h_info[8] = h->plan.nsegs;
    return 0;
}

namespace {

int hwpss_fit_into(cm2_hwpss *h, const double *d_in, double *d_coeff, hipStream_t st)
{
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        k_hwpss_sums<H><<<dim3((unsigned)h->plan.nsegs), hp::kThreads, 0, st>>>(
            h->dev(), h->state.d_skip, h->d_pix, d_in, h->d_cos, h->d_sin, h->state.d_partial);
    });
    CM2_LAUNCH_OK();
    k_hwpss_solve<<<dim3((unsigned)h->plan.nunits), 64, 0, st>>>(h->dev(), h->plan.K, h->state.d_skip,
                                                                  h->state.d_factor, h->state.d_partial, d_coeff);
    CM2_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" int cm2_hwpss_fit(cm2_hwpss *h, const double *d_in, double *d_coeff, void *stream)
{
    CM2_CHECK(h, "cm2_hwpss_fit: null handle");
    CM2_CHECK(d_in && d_coeff, "cm2_hwpss_fit: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_coeff, h->plan.nunits * h->plan.K),
              "cm2_hwpss_fit: the coefficients must not alias the input");
    return hwpss_fit_into(h, d_in, d_coeff, as_stream(stream));
}

extern "C" int cm2_hwpss_apply(cm2_hwpss *h, const double *d_in, double *d_out, void *stream)
{
    CM2_CHECK(h, "cm2_hwpss_apply: null handle");
    CM2_CHECK(d_in && d_out, "cm2_hwpss_apply: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_out, h->plan.nt),
              "cm2_hwpss_apply: output must not alias the input");
    hipStream_t st = as_stream(stream);
    if (int rc = hwpss_fit_into(h, d_in, h->state.d_coeff, st)) return rc;
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        k_hwpss_subtract<H><<<dim3((unsigned)h->plan.nsegs), hp::kThreads, 0, st>>>(
            h->dev(), h->state.d_skip, h->state.d_coeff, h->d_pix, d_in, h->d_cos, h->d_sin, d_out);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_hwpss_tables(const cm2_hwpss *h, double *d_cos, double *d_sin, void *stream)
{
    CM2_CHECK(h, "cm2_hwpss_tables: null handle");
    CM2_CHECK(d_cos && d_sin, "cm2_hwpss_tables: null array");
    CM2_CHECK(!ranges_overlap(d_cos, h->plan.ns, d_sin, h->plan.ns), "cm2_hwpss_tables: the two outputs overlap");
    hipStream_t st = as_stream(stream);
    const size_t bytes = sizeof(double) * (size_t)h->plan.ns;
    CM2_HIP(hipMemcpyAsync(d_cos, h->d_cos, bytes, hipMemcpyDeviceToDevice, st));
    CM2_HIP(hipMemcpyAsync(d_sin, h->d_sin, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}
