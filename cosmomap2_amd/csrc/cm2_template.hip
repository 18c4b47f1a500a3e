// cm2_template.hip -- the template filter (TemplateFilterLO), see include/cosmomap2.h (f2i): per (detector, chunk)
// unit, fit and remove K time-domain templates given by the caller (housekeeping channels, the air mass, a
// scan-synchronous template sampled in time), shared by all detectors, on the unflagged samples.
// cm2_chunkfit.h has the order of every sum, the factor, the solve and the rule of a skipped unit (tau =
// CM2_TEMPLATE_TAU; m is an integer count, k_template_count); cm2_template_policy.h has the detector tiles.
//
// Templates of a sample, from the table tab[J][ns] of the handle: with the constant T_0 = 1 and T_j = tab[j - 1]
// (the caller's template minus its chunk mean, k_template_centre); without it T_j = tab[j], as given.
//
// What is new against cm2_hwpss.hip is where the templates come from: K doubles per sample from memory, the same for
// every detector.  A workgroup therefore takes one segment of Dt = det_tile(K) consecutive detectors: a thread loads
// the K template values of a sample once and the value and the flag of that sample for each detector, and keeps
// Dt x K accumulators (32 doubles at most).  The table costs 8 K / Dt bytes per detector sample and pass from L2
// instead of 8 K.  Workgroups run tiles fastest, so that those in flight together read the same lines of the table.
//
// The sums are formed per detector and do not depend on the tile (segment sums of T_j v in k_template_sums<K, false>,
// of T_i T_j in k_template_sums<K, true>).
//
// Centring (k_template_centre, once, with the constant only): one workgroup per (template, chunk).  Thread t adds the
// finite values x(q), q = t, t + 256, ... of the whole chunk in ascending order, starting from 0, and counts them;
// lanes and waves as in steps 2 and 3 of the sum order; mu = sum / count (0 when none is finite); tab(q) = x(q) - mu
// for every q.
// Subtract (k_template_subtract): p = c_0 T_0, then p += c_j T_j for j = 1..K-1 (c_0 T_0 = c_0 exactly where T_0 = 1);
// out = v - p on an unflagged sample, 0 on a flagged one and on every sample of a skipped unit.
#include "cm2_chunkfit.h"
#include "cm2_template_policy.h"

using namespace cm2;
namespace tp = cm2::tmpl;
namespace cf = cm2::chunkfit;

namespace {

struct PlanDev : cf::GeomDev {
    int64_t ntiles;
    int cst;                                           // 1 with the constant: T_0 = 1 and row j of the table is T_{j+1}
};

template <int K>
__device__ __forceinline__ void load_templates(const PlanDev &p, const double *__restrict__ tab, int64_t t,
                                               double (&T)[K])
{
    T[0] = p.cst ? 1.0 : tab[t];
#pragma unroll
    for (int j = 1; j < K; ++j) T[j] = tab[(int64_t)(j - p.cst) * p.ns + t];
}

// mu of (chunk c, template j) = blockIdx.(x, y), subtracted in place
__global__ __launch_bounds__(tp::kThreads) void k_template_centre(PlanDev p, double *__restrict__ tab)
{
    __shared__ double wsum[4], wcnt[4];
    __shared__ double mean;
    double *row = tab + (int64_t)blockIdx.y * p.ns;
    const int64_t a = p.edges[blockIdx.x], b = p.edges[blockIdx.x + 1];
    double acc = 0.0, cnt = 0.0;
    for (int64_t t = a + threadIdx.x; t < b; t += tp::kThreads) {
        const double x = row[t];
        if (isfinite(x)) {
            acc += x;
            cnt += 1.0;
        }
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);                               // integers below 2^40: exact
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        wsum[w] = acc;
        wcnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        const double n = ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
        mean = n > 0.0 ? s / n : 0.0;
    }
    __syncthreads();
    const double mu = mean;
    for (int64_t t = a + threadIdx.x; t < b; t += tp::kThreads) row[t] = row[t] - mu;
}

// cnt[segment] = its unflagged samples, one workgroup per (detector, row segment)
__global__ __launch_bounds__(tp::kThreads) void k_template_count(PlanDev p, const int32_t *__restrict__ pix,
                                                                 int32_t *__restrict__ cnt)
{
    __shared__ int wn[4];
    const int64_t b = blockIdx.x;
    const cf::SegPos s = cf::seg_pos(p, b);
    int n = 0;
    for (int64_t t = s.t0 + threadIdx.x; t < s.t1; t += tp::kThreads) n += pix[s.base + t] >= 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) wn[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) cnt[b] = wn[0] + wn[1] + wn[2] + wn[3];
}

// The segment sums of one workgroup's tile.  GRAM: row `row` of the Gram sums, dst[((k segs_per_det + r) K + row) K + j]
// = sum over the unflagged samples of T_j T_row; else dst[(k segs_per_det + r) K + j] = sum of T_j v, and the
// detectors whose unit is skipped are left out (their sums are never read).
template <int K, bool GRAM>
__global__ __launch_bounds__(tp::kThreads, 2) void k_template_sums(PlanDev p, const uint8_t *__restrict__ skip,
                                                                   const int32_t *__restrict__ pix,
                                                                   const double *__restrict__ v,
                                                                   const double *__restrict__ tab,
                                                                   double *__restrict__ dst)
{
    constexpr int Dt = tp::det_tile(K);
    __shared__ double wsum[Dt][4][K];
    const int64_t w = blockIdx.x;
    const cf::RowSeg s = cf::row_segment(p, w / p.ntiles);
    const int64_t k0 = (w - s.r * p.ntiles) * Dt;
    const int row = GRAM ? (int)blockIdx.y : 0;
    bool live[Dt];
    bool any = false;
#pragma unroll
    for (int d = 0; d < Dt; ++d) {
        live[d] = k0 + d < p.ndet && (GRAM || !skip[(k0 + d) * p.nchunks + s.c]);
        any = any || live[d];
    }
    if (!any) return;
    double acc[Dt][K];
#pragma unroll
    for (int d = 0; d < Dt; ++d)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[d][j] = 0.0;
#pragma unroll 2
    for (int u = 0; u < tp::kPer; ++u) {
        const int64_t t = s.t0 + threadIdx.x + (int64_t)u * tp::kThreads;
        if (t < s.t1) {
            double T[K];
            load_templates<K>(p, tab, t, T);
            double tr = 0.0;
            if (GRAM) tr = (row == 0 && p.cst) ? 1.0 : tab[(int64_t)(row - p.cst) * p.ns + t];
#pragma unroll
            for (int d = 0; d < Dt; ++d) {
                if (live[d]) {                         // the same in every lane
                    const int64_t at = (k0 + d) * p.ns + t;
                    const int32_t px = pix[at];
                    const double x = GRAM ? tr : v[at];
                    if (px >= 0) {
#pragma unroll
                        for (int j = 0; j < K; ++j) acc[d][j] += T[j] * x;
                    }
                }
            }
        }
    }
    // steps 2 and 3 of the sum order, detector by detector
#pragma unroll
    for (int d = 0; d < Dt; ++d)
        if (live[d]) cf::wave_sums<K>(acc[d], wsum[d]);
    __syncthreads();
    for (int e = threadIdx.x; e < Dt * K; e += tp::kThreads) {
        const int d = e / K, j = e - d * K;
        if (k0 + d < p.ndet && (GRAM || !skip[(k0 + d) * p.nchunks + s.c])) {
            const int64_t seg = (k0 + d) * p.segs_per_det + s.r;
            const double x = cf::waves_sum<K>(wsum[d], j);
            if (GRAM) dst[(seg * K + row) * K + j] = x;
            else dst[seg * K + j] = x;
        }
    }
}

// one workgroup of 64 threads per unit: adds the counts and the Gram sums of its segments, factorises, marks
__global__ __launch_bounds__(64) void k_template_factor(PlanDev p, int K, double tau, const int32_t *__restrict__ cnt,
                                                         const double *__restrict__ gp, double *__restrict__ factor,
                                                         uint8_t *__restrict__ skip)
{
    cf::factor_unit<tp::kMaxK>(p, K, tau, gp, factor, skip, [&](const double *, const cf::UnitSegs &u) {
        int64_t m = 0;
        for (int64_t g = 0; g < u.n; ++g) m += cnt[u.first + g];
        return m;
    });
}

__global__ __launch_bounds__(64) void k_template_solve(PlanDev p, int K, const uint8_t *__restrict__ skip,
                                                        const double *__restrict__ factor,
                                                        const double *__restrict__ partial, double *__restrict__ coeff)
{
    cf::solve_unit<tp::kMaxK>(p, K, skip, factor, partial, coeff);
}

// the coefficients of the tile's units go through LDS once per workgroup, the templates are loaded once per sample
template <int K>
__global__ __launch_bounds__(tp::kThreads, 2) void k_template_subtract(PlanDev p, const uint8_t *__restrict__ skip,
                                                                       const double *__restrict__ coeff,
                                                                       const int32_t *__restrict__ pix,
                                                                       const double *__restrict__ v,
                                                                       const double *__restrict__ tab,
                                                                       double *__restrict__ out)
{
    constexpr int Dt = tp::det_tile(K);
    __shared__ double cs[Dt][K];
    __shared__ int gone[Dt];                           // 0 fit, 1 skipped unit (zeros), 2 no such detector
    const int64_t w = blockIdx.x;
    const cf::RowSeg s = cf::row_segment(p, w / p.ntiles);
    const int64_t k0 = (w - s.r * p.ntiles) * Dt;
    for (int e = threadIdx.x; e < Dt * K; e += tp::kThreads) {
        const int d = e / K, j = e - d * K;
        const bool in = k0 + d < p.ndet;
        cs[d][j] = in ? coeff[((k0 + d) * p.nchunks + s.c) * K + j] : 0.0;
        if (j == 0) gone[d] = in ? (skip[(k0 + d) * p.nchunks + s.c] ? 1 : 0) : 2;
    }
    __syncthreads();
    int state[Dt];
#pragma unroll
    for (int d = 0; d < Dt; ++d) state[d] = __builtin_amdgcn_readfirstlane(gone[d]);      // the same in every lane
#pragma unroll 2
    for (int u = 0; u < tp::kPer; ++u) {
        const int64_t t = s.t0 + threadIdx.x + (int64_t)u * tp::kThreads;
        if (t < s.t1) {
            double T[K];
            load_templates<K>(p, tab, t, T);
#pragma unroll
            for (int d = 0; d < Dt; ++d) {
                const int g = state[d];
                if (g == 2) continue;
                const int64_t at = (k0 + d) * p.ns + t;
                double o = 0.0;
                if (g == 0) {
                    const int32_t px = pix[at];
                    const double x = v[at];
                    if (px >= 0) {
                        double pr = cs[d][0] * T[0];
#pragma unroll
                        for (int j = 1; j < K; ++j) pr += cs[d][j] * T[j];
                        o = x - pr;
                    }
                }
                out[at] = o;
            }
        }
    }
}

}  // namespace

struct cm2_template {
    tp::Plan plan;
    const int32_t *d_pix = nullptr;       // borrowed
    cf::State state;
    double *d_tab = nullptr;
    PlanDev dev() const { return PlanDev{state.dev(plan), plan.ntiles, plan.add_constant}; }
};

extern "C" int cm2_template_destroy(cm2_template *h)
{
    if (!h) return 0;
    h->state.release();
    dev_release(h->d_tab);
    delete h;
    return 0;
}

namespace {

int template_fill(cm2_template *h, const double *d_templates, hipStream_t st)
{
    const tp::Plan &p = h->plan;
    const int K = p.K;
    const size_t ntab = (size_t)p.J * (size_t)p.ns;
    if (int rc = h->state.fill(p, K, st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_tab, sizeof(double) * (ntab ? ntab : 1)));
    if (ntab) CM2_HIP(hipMemcpyAsync(h->d_tab, d_templates, sizeof(double) * ntab, hipMemcpyDeviceToDevice, st));
    if (p.add_constant && p.J > 0) {
        k_template_centre<<<dim3((unsigned)p.nchunks, (unsigned)p.J), tp::kThreads, 0, st>>>(h->dev(), h->d_tab);
        CM2_LAUNCH_OK();
    }
    DevTemp<int32_t> cnt;                              // create time only: the counts and the Gram sums of every segment
    DevTemp<double> gp;
    CM2_HIP(cnt.alloc((size_t)p.nsegs));
    CM2_HIP(gp.alloc((size_t)(p.nsegs * K * K)));
    k_template_count<<<dim3((unsigned)p.nsegs), tp::kThreads, 0, st>>>(h->dev(), h->d_pix, cnt.p);
    CM2_LAUNCH_OK();
    dispatch_int<1, tp::kMaxK>(K, [&](auto KC) {
        const dim3 grid((unsigned)p.ngroups, (unsigned)K);
        k_template_sums<KC, true><<<grid, tp::kThreads, 0, st>>>(h->dev(), nullptr, h->d_pix, nullptr, h->d_tab, gp.p);
    });
    CM2_LAUNCH_OK();
    k_template_factor<<<dim3((unsigned)p.nunits), 64, 0, st>>>(h->dev(), K, CM2_TEMPLATE_TAU, cnt, gp,
                                                                h->state.d_factor, h->state.d_skip);
    CM2_LAUNCH_OK();
    return h->state.tally(p, st);
}

}  // namespace

extern "C" int cm2_template_create(cm2_template **out, int64_t ns, int ndet, int64_t nchunks, const int64_t *h_edges,
                                   int ntemplates, const double *d_templates, int add_constant, const int32_t *d_pix,
                                   void *stream)
{
    const char *who = "cm2_template_create";
    CM2_CHECK(out, "%s: null output handle", who);
    CM2_CHECK(h_edges && d_pix && (d_templates || ntemplates <= 0), "%s: null array", who);
    cm2_template *h = new cm2_template();
    const tp::Status ps = tp::make_plan(&h->plan, ns, ndet, nchunks, h_edges, ntemplates, add_constant);
    if (ps != tp::kOk) {
        delete h;
        CM2_CHECK(ps != tp::kBadCount, "%s: ntemplates=%d must be >= 0", who, ntemplates);
        CM2_CHECK(ps != tp::kBadConstant, "%s: add_constant=%d must be 0 or 1", who, add_constant);
        CM2_CHECK(ps != tp::kBadK, "%s: K = ntemplates + add_constant = %d + %d outside [1, %d]", who, ntemplates,
                  add_constant, tp::kMaxK);
        return cf::check_create_status(who, ps, tp::kBadSize, ns, ndet, nchunks);
    }
    h->d_pix = d_pix;
    const int rc = template_fill(h, d_templates, as_stream(stream));
    if (rc) {
        cm2_template_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_template_info(const cm2_template *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_template_info: null argument");
    h_info[0] = h->plan.ns;
    h_info[1] = h->plan.ndet;
    h_info[2] = h->plan.nchunks;
    h_info[3] = h->plan.K;
    h_info[4] = h->plan.add_constant;
    h_info[5] = h->state.nmark[0];
    h_info[6] = h->state.nmark[1];
    h_info[7] = h->state.nmark[2];
    h_info[8] = tp::kSeg;
    h_info[9] = h->plan.nsegs;
    return 0;
}

namespace {

int template_fit_into(cm2_template *h, const double *d_in, double *d_coeff, hipStream_t st)
{
    dispatch_int<1, tp::kMaxK>(h->plan.K, [&](auto KC) {
        k_template_sums<KC, false><<<dim3((unsigned)h->plan.ngroups), tp::kThreads, 0, st>>>(
            h->dev(), h->state.d_skip, h->d_pix, d_in, h->d_tab, h->state.d_partial);
    });
    CM2_LAUNCH_OK();
    k_template_solve<<<dim3((unsigned)h->plan.nunits), 64, 0, st>>>(h->dev(), h->plan.K, h->state.d_skip,
                                                                     h->state.d_factor, h->state.d_partial, d_coeff);
    CM2_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" int cm2_template_fit(cm2_template *h, const double *d_in, double *d_coeff, void *stream)
{
    CM2_CHECK(h, "cm2_template_fit: null handle");
    CM2_CHECK(d_in && d_coeff, "cm2_template_fit: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_coeff, h->plan.nunits * h->plan.K),
              "cm2_template_fit: the coefficients must not alias the input");
    return template_fit_into(h, d_in, d_coeff, as_stream(stream));
}

extern "C" int cm2_template_apply(cm2_template *h, const double *d_in, double *d_out, void *stream)
{
    CM2_CHECK(h, "cm2_template_apply: null handle");
    CM2_CHECK(d_in && d_out, "cm2_template_apply: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_out, h->plan.nt),
              "cm2_template_apply: output must not alias the input");
    hipStream_t st = as_stream(stream);
    if (int rc = template_fit_into(h, d_in, h->state.d_coeff, st)) return rc;
    dispatch_int<1, tp::kMaxK>(h->plan.K, [&](auto KC) {
        k_template_subtract<KC><<<dim3((unsigned)h->plan.ngroups), tp::kThreads, 0, st>>>(
            h->dev(), h->state.d_skip, h->state.d_coeff, h->d_pix, d_in, h->d_tab, d_out);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_template_status(const cm2_template *h, uint8_t *d_status, void *stream)
{
    CM2_CHECK(h, "cm2_template_status: null handle");
    CM2_CHECK(d_status, "cm2_template_status: null array");
    CM2_HIP(hipMemcpyAsync(d_status, h->state.d_skip, (size_t)h->plan.nunits, hipMemcpyDeviceToDevice,
                           as_stream(stream)));
    return 0;
}

extern "C" int cm2_template_tables(const cm2_template *h, double *d_tables, void *stream)
{
    CM2_CHECK(h, "cm2_template_tables: null handle");
    const size_t ntab = (size_t)h->plan.J * (size_t)h->plan.ns;
    CM2_CHECK(d_tables || !ntab, "cm2_template_tables: null array");
    if (ntab)
        CM2_HIP(hipMemcpyAsync(d_tables, h->d_tab, sizeof(double) * ntab, hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}
