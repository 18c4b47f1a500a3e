// cm2_hwpss.hip -- the HWP-synchronous signal filter (HWPSSFilterLO), see include/cosmomap2.h (f2c): per (detector,
// chunk) unit, fit and remove the harmonics 1, cos(n chi), sin(n chi), n = 1..H, of the plate angle chi on the
// unflagged samples.  cm2_hwpss_policy.h has the segment plan.
//
// Templates of a sample, from the two tables c1 = cos chi, s1 = sin chi (device sincos, once at create time):
//   T_0 = 1, T_1 = c1, T_2 = s1,  T_{2n-1} = T_{2n-3} c1 - T_{2n-2} s1,  T_{2n} = T_{2n-2} c1 + T_{2n-3} s1   (n >= 2)
// every product and every sum rounded on its own (the unit is compiled with -ffp-contract=off).
//
// The order of every sum (segment sums of T_j v in k_hwpss_sums, of T_i T_j in k_hwpss_gram):
//   1. thread t of the segment's workgroup: acc = 0, then acc += T_j(q) v(q) for its unflagged samples
//      q = t, t + 256, ... in ascending order (kPer = 16 at most);
//   2. the 64 lanes of a wave: x += shfl_down(x, off) for off = 32, 16, 8, 4, 2, 1; lane 0 holds the wave's sum;
//   3. the segment's sum is ((w0 + w1) + w2) + w3 of its four waves;
//   4. a unit's sum is 0 + its segments' sums in ascending segment order (k_hwpss_solve, k_hwpss_factor).
// There is no floating-point atomic: two applications give the same bits.
//
// Factor (k_hwpss_factor, once) and solve (k_hwpss_solve): cm2_fit.h has them and the order of their operations;
// the unit is skipped when a pivot fails with tau = CM2_HWPSS_TAU (or when G_00 = m < K).
// Subtract (k_hwpss_subtract): p = c_0, then p += c_{2n-1} T_{2n-1}, p += c_{2n} T_{2n} for n = 1..H; out = v - p on
// an unflagged sample, 0 on a flagged one and on every sample of a skipped unit.
#include "cm2_common.h"
#include "cm2_hwpss_policy.h"

using namespace cm2;
namespace hp = cm2::hwpss;

namespace {

struct PlanDev {
    int64_t ns, nchunks, segs_per_det;
    const int64_t *edges, *seg_first;
    const int32_t *seg_chunk;
};

struct SegPos {
    int64_t t0, t1;      // samples [t0, t1) of the row
    int64_t base;        // first sample of the row in the stream
    int64_t unit;
};

__device__ __forceinline__ SegPos seg_pos(const PlanDev &p, int64_t b)
{
    SegPos s;
    const int64_t det = b / p.segs_per_det, r = b - det * p.segs_per_det;
    const int64_t c = p.seg_chunk[r];
    s.t0 = p.edges[c] + (r - p.seg_first[c]) * hp::kSeg;
    const int64_t e = p.edges[c + 1];
    s.t1 = s.t0 + hp::kSeg < e ? s.t0 + hp::kSeg : e;
    s.base = det * p.ns;
    s.unit = det * p.nchunks + c;
    return s;
}

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

// steps 2 and 3 of the sum order for the K accumulators of a thread; threads 0..K-1 write the segment's sums
template <int K>
__device__ __forceinline__ void segment_reduce(double (&acc)[K], double *__restrict__ dst)
{
    __shared__ double wsum[4][K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double s = wave_sum(acc[j]);
        if (lane == 0) wsum[w][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        dst[j] = ((wsum[0][j] + wsum[1][j]) + wsum[2][j]) + wsum[3][j];
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
// skip = 0 fitted, 1 fewer than K unflagged samples, 2 a pivot at or below tau G_jj
__global__ __launch_bounds__(64) void k_hwpss_factor(PlanDev p, int K, double tau, const double *__restrict__ gp,
                                                      double *__restrict__ factor, uint8_t *__restrict__ skip)
{
    __shared__ double G[hp::kMaxK * hp::kMaxK];
    const int64_t unit = blockIdx.x;
    const int64_t det = unit / p.nchunks, c = unit - det * p.nchunks;
    const int64_t first = det * p.segs_per_det + p.seg_first[c];
    const int64_t nseg = p.seg_first[c + 1] - p.seg_first[c];
    const int KK = K * K;
    for (int e = threadIdx.x; e < KK; e += 64) {
        double sum = 0.0;
        for (int64_t g = 0; g < nseg; ++g) sum += gp[(first + g) * KK + e];
        G[e] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *L = factor + unit * hp::packed(K);
    int mark = G[0] < (double)K ? 1 : 0;               // G_00 = the number of unflagged samples, exact
    const fit::RowMajor rows{G, K};
    if (mark == 0 && fit::factor(K, rows, tau)) mark = 2;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) L[hp::packed_at(i, j)] = mark ? 0.0 : G[i * K + j];
    skip[unit] = (uint8_t)mark;
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

// one workgroup of 64 threads per unit: lane j adds the segments' sums of template j, thread 0 solves
__global__ __launch_bounds__(64) void k_hwpss_solve(PlanDev p, int K, const uint8_t *__restrict__ skip,
                                                     const double *__restrict__ factor,
                                                     const double *__restrict__ partial, double *__restrict__ coeff)
{
    __shared__ double y[hp::kMaxK];
    __shared__ double L[hp::kMaxK * (hp::kMaxK + 1) / 2];
    const int64_t unit = blockIdx.x;
    const int j = threadIdx.x;
    if (skip[unit]) {
        if (j < K) coeff[unit * K + j] = 0.0;
        return;
    }
    const int64_t det = unit / p.nchunks, c = unit - det * p.nchunks;
    const int64_t first = det * p.segs_per_det + p.seg_first[c];
    const int64_t nseg = p.seg_first[c + 1] - p.seg_first[c];
    for (int e = j; e < hp::packed(K); e += 64) L[e] = factor[unit * hp::packed(K) + e];
    if (j < K) {
        double sum = 0.0;
#pragma unroll 8
        for (int64_t g = 0; g < nseg; ++g) sum += partial[(first + g) * K + j];
        y[j] = sum;
    }
    __syncthreads();
    if (j != 0) return;
    fit::solve(K, L, y);
    for (int i = 0; i < K; ++i) coeff[unit * K + i] = y[i];
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
    int64_t *d_edges = nullptr, *d_seg_first = nullptr;
    int32_t *d_seg_chunk = nullptr;
    double *d_cos = nullptr, *d_sin = nullptr, *d_factor = nullptr, *d_partial = nullptr, *d_coeff = nullptr;
    uint8_t *d_skip = nullptr;
    int64_t nmark[3] = {0, 0, 0};
    PlanDev dev() const
    {
        return PlanDev{plan.ns, plan.nchunks, plan.segs_per_det, d_edges, d_seg_first, d_seg_chunk};
    }
};

extern "C" int cm2_hwpss_destroy(cm2_hwpss *h)
{
    if (!h) return 0;
    dev_release(h->d_edges, h->d_seg_first, h->d_seg_chunk, h->d_cos, h->d_sin, h->d_factor, h->d_partial,
                h->d_coeff, h->d_skip);
    delete h;
    return 0;
}

namespace {

int hwpss_fill(cm2_hwpss *h, const double *d_chi, hipStream_t st)
{
    const hp::Plan &p = h->plan;
    const int K = p.K;
    if (int rc = dev_put(&h->d_edges, p.edges.data(), p.edges.size(), st)) return rc;
    if (int rc = dev_put(&h->d_seg_first, p.seg_first.data(), p.seg_first.size(), st)) return rc;
    if (int rc = dev_put(&h->d_seg_chunk, p.seg_chunk.data(), p.seg_chunk.size(), st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_cos, sizeof(double) * (size_t)p.ns));
    CM2_HIP(cm2::dev_malloc(&h->d_sin, sizeof(double) * (size_t)p.ns));
    CM2_HIP(cm2::dev_malloc(&h->d_factor, sizeof(double) * (size_t)(p.nunits * hp::packed(K))));
    CM2_HIP(cm2::dev_malloc(&h->d_partial, sizeof(double) * (size_t)(p.nsegs * K)));
    CM2_HIP(cm2::dev_malloc(&h->d_coeff, sizeof(double) * (size_t)(p.nunits * K)));
    CM2_HIP(cm2::dev_malloc(&h->d_skip, (size_t)p.nunits));
    k_hwpss_tables<<<grid_for(p.ns), kBlock, 0, st>>>(p.ns, d_chi, h->d_cos, h->d_sin);
    CM2_LAUNCH_OK();
    DevTemp<double> gp;                                // the Gram sums of every segment: create time only
    CM2_HIP(gp.alloc((size_t)(p.nsegs * K * K)));
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        const dim3 grid((unsigned)p.nsegs, (unsigned)K);
        k_hwpss_gram<H><<<grid, hp::kThreads, 0, st>>>(h->dev(), h->d_pix, h->d_cos, h->d_sin, gp.p);
    });
    CM2_LAUNCH_OK();
    k_hwpss_factor<<<dim3((unsigned)p.nunits), 64, 0, st>>>(h->dev(), K, CM2_HWPSS_TAU, gp, h->d_factor, h->d_skip);
    CM2_LAUNCH_OK();
    std::vector<uint8_t> marks((size_t)p.nunits);
    CM2_HIP(cm2::download(marks.data(), h->d_skip, marks.size(), st));
    CM2_HIP(hipStreamSynchronize(st));
    for (uint8_t m : marks) h->nmark[m < 3 ? m : 0]++;
    return 0;
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
        CM2_CHECK(ps != hp::kBadSize, "%s: ns=%lld, ndet=%d, nchunks=%lld must all be >= 1", who, (long long)ns, ndet,
                  (long long)nchunks);
        CM2_CHECK(ps != hp::kBadEdges, "%s: the %lld chunk edges must ascend strictly from 0 to ns=%lld", who,
                  (long long)nchunks + 1, (long long)ns);
        CM2_CHECK(false, "%s: ns=%lld x ndet=%d with %lld chunks overflows the index types", who, (long long)ns, ndet,
                  (long long)nchunks);
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
    h_info[4] = h->nmark[0];
    h_info[5] = h->nmark[1];
    h_info[6] = h->nmark[2];
    h_info[7] = hp::kSeg;
    h_info[8] = h->plan.nsegs;
    return 0;
}

namespace {

int hwpss_fit_into(cm2_hwpss *h, const double *d_in, double *d_coeff, hipStream_t st)
{
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        k_hwpss_sums<H><<<dim3((unsigned)h->plan.nsegs), hp::kThreads, 0, st>>>(h->dev(), h->d_skip, h->d_pix, d_in,
                                                                                 h->d_cos, h->d_sin, h->d_partial);
    });
    CM2_LAUNCH_OK();
    k_hwpss_solve<<<dim3((unsigned)h->plan.nunits), 64, 0, st>>>(h->dev(), h->plan.K, h->d_skip, h->d_factor,
                                                                  h->d_partial, d_coeff);
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
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_out, h->plan.nt), "cm2_hwpss_apply: output must not alias the input");
    hipStream_t st = as_stream(stream);
    if (int rc = hwpss_fit_into(h, d_in, h->d_coeff, st)) return rc;
    dispatch_int<1, hp::kMaxHarm>(h->plan.nharm, [&](auto H) {
        k_hwpss_subtract<H><<<dim3((unsigned)h->plan.nsegs), hp::kThreads, 0, st>>>(
            h->dev(), h->d_skip, h->d_coeff, h->d_pix, d_in, h->d_cos, h->d_sin, d_out);
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
