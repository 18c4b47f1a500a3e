// cm2_chunkfit.h -- the per-chunk fit of the HWPSS filter (cm2_hwpss.hip) and the template filter (cm2_template.hip),
// written once: per (detector, chunk) unit, fit and remove K templates T_0..T_{K-1} on the unflagged samples.  The two
// filters differ in where T_j of a sample comes from and in how a workgroup's detectors are chosen; their kernels form
// the sums of a thread and subtract, and use what is here for the rest.  cm2_chunkfit_policy.h has the segment plan;
// the host helpers of the two handles are at the end.
//
// The order of every sum (segment sums of T_j v for the right-hand sides, of T_i T_j for the Gram matrices), per
// detector (the units are compiled with -ffp-contract=off: every product and every sum is rounded on its own):
//   1. thread t of the segment's workgroup: acc = 0, then acc += T_j(q) v(q) for its unflagged samples
//      q = t, t + 256, ... in ascending order (kPer = 16 at most);
//   2. the 64 lanes of a wave: x += shfl_down(x, off) for off = 32, 16, 8, 4, 2, 1; lane 0 holds the wave's sum;
//   3. the segment's sum is ((w0 + w1) + w2) + w3 of its four waves;
//   4. a unit's sum is 0 + its segments' sums in ascending segment order (factor_unit, solve_unit).
// There is no floating-point atomic: two applications give the same bits.
//
// Factor (factor_unit, once per handle) and solve (solve_unit): cm2_fit.h has them and the order of their operations.
// A unit is skipped, its coefficients and its output 0, when it has m < K unflagged samples (kFew) or when a pivot
// fails with the filter's tau (kPivot); the caller says what m is.
#pragma once
#include "cm2_common.h"
#include "cm2_chunkfit_policy.h"

#include <vector>

namespace cm2 {
namespace chunkfit {

// the geometry of a plan as the kernels see it
struct GeomDev {
    int64_t ns, ndet, nchunks, segs_per_det;
    const int64_t *edges, *seg_first;
    const int32_t *seg_chunk;
};

struct RowSeg {
    int64_t t0, t1;      // samples [t0, t1) of the row
    int64_t r, c;        // row segment, chunk
};

__device__ __forceinline__ RowSeg row_segment(const GeomDev &p, int64_t r)
{
    RowSeg s;
    s.r = r;
    s.c = p.seg_chunk[r];
    s.t0 = p.edges[s.c] + (r - p.seg_first[s.c]) * kSeg;
    const int64_t e = p.edges[s.c + 1];
    s.t1 = s.t0 + kSeg < e ? s.t0 + kSeg : e;
    return s;
}

struct SegPos {
    int64_t t0, t1;      // samples [t0, t1) of the row
    int64_t base;        // first sample of the row in the stream
    int64_t unit;
};

// segment b = det segs_per_det + r of the whole stream
__device__ __forceinline__ SegPos seg_pos(const GeomDev &p, int64_t b)
{
    const int64_t det = b / p.segs_per_det;
    const RowSeg s = row_segment(p, b - det * p.segs_per_det);
    return SegPos{s.t0, s.t1, det * p.ns, det * p.nchunks + s.c};
}

// step 2 of the sum order for the K accumulators of one detector: wsum[w][j] (LDS) = the sum of wave w.  A barrier
// stands between this and step 3, waves_sum: the segment's sum of accumulator j.  A tile calls both once per detector
template <int K>
__device__ __forceinline__ void wave_sums(const double (&acc)[K], double (&wsum)[4][K])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double x = wave_sum(acc[j]);
        if (lane == 0) wsum[w][j] = x;
    }
}
template <int K>
__device__ __forceinline__ double waves_sum(const double (&wsum)[4][K], int j)
{
    return ((wsum[0][j] + wsum[1][j]) + wsum[2][j]) + wsum[3][j];
}

// steps 2 and 3 for one detector: threads 0..K-1 write the segment's sums to dst[0..K-1]
template <int K>
__device__ __forceinline__ void segment_reduce(const double (&acc)[K], double *__restrict__ dst)
{
    __shared__ double wsum[4][K];
    wave_sums<K>(acc, wsum);
    __syncthreads();
    if (threadIdx.x < K) dst[threadIdx.x] = waves_sum<K>(wsum, threadIdx.x);
}

// the segments first .. first + n - 1 of a unit
struct UnitSegs {
    int64_t first, n;
};

__device__ __forceinline__ UnitSegs unit_segments(const GeomDev &p, int64_t unit)
{
    const int64_t det = unit / p.nchunks, c = unit - det * p.nchunks;
    return UnitSegs{det * p.segs_per_det + p.seg_first[c], p.seg_first[c + 1] - p.seg_first[c]};
}

// the body of a factor kernel, one workgroup of 64 threads per unit: adds the Gram sums of the unit's segments (step
// 4); thread 0 factorises, marks the unit with m = count(G, u) unflagged samples and stores its packed factor (zeros
// for a skipped unit).  MAXK: the filter's largest K
template <int MAXK, class Count>
__device__ __forceinline__ void factor_unit(const GeomDev &p, int K, double tau, const double *__restrict__ gp,
                                            double *__restrict__ factor, uint8_t *__restrict__ skip, Count &&count)
{
    __shared__ double G[MAXK * MAXK];
    const int64_t unit = blockIdx.x;
    const UnitSegs u = unit_segments(p, unit);
    const int KK = K * K;
    for (int e = threadIdx.x; e < KK; e += 64) {
        double sum = 0.0;
        for (int64_t g = 0; g < u.n; ++g) sum += gp[(u.first + g) * KK + e];
        G[e] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *L = factor + unit * packed(K);
    int mark = count(G, u) < K ? kFew : kFitted;
    const fit::RowMajor rows{G, K};
    if (mark == kFitted && fit::factor(K, rows, tau)) mark = kPivot;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) L[packed_at(i, j)] = mark ? 0.0 : G[i * K + j];
    skip[unit] = (uint8_t)mark;
}

// the body of a solve kernel, one workgroup of 64 threads per unit: lane j adds the segments' sums of template j
// (step 4), thread 0 solves.  MAXK: the filter's largest K
template <int MAXK>
__device__ __forceinline__ void solve_unit(const GeomDev &p, int K, const uint8_t *__restrict__ skip,
                                           const double *__restrict__ factor, const double *__restrict__ partial,
                                           double *__restrict__ coeff)
{
    __shared__ double y[MAXK];
    __shared__ double L[MAXK * (MAXK + 1) / 2];
    const int64_t unit = blockIdx.x;
    const int j = threadIdx.x;
    if (skip[unit]) {
        if (j < K) coeff[unit * K + j] = 0.0;
        return;
    }
    const UnitSegs u = unit_segments(p, unit);
    for (int e = j; e < packed(K); e += 64) L[e] = factor[unit * packed(K) + e];
    if (j < K) {
        double sum = 0.0;
#pragma unroll 8
        for (int64_t g = 0; g < u.n; ++g) sum += partial[(u.first + g) * K + j];
        y[j] = sum;
    }
    __syncthreads();
    if (j != 0) return;
    fit::solve(K, L, y);
    for (int i = 0; i < K; ++i) coeff[unit * K + i] = y[i];
}

// ------------------------------------------------------------------ host side ----
// what both handles own on the device: the three tables of the plan, the factors, the segment sums of the last fit,
// the coefficients of the last apply and the marks, with the tally of the marks
struct State {
    int64_t *d_edges = nullptr, *d_seg_first = nullptr;
    int32_t *d_seg_chunk = nullptr;
    double *d_factor = nullptr, *d_partial = nullptr, *d_coeff = nullptr;
    uint8_t *d_skip = nullptr;
    int64_t nmark[3] = {0, 0, 0};

    GeomDev dev(const Geometry &p) const
    {
        return GeomDev{p.ns, p.ndet, p.nchunks, p.segs_per_det, d_edges, d_seg_first, d_seg_chunk};
    }
    int fill(const Geometry &p, int K, hipStream_t st)
    {
        if (int rc = dev_put(&d_edges, p.edges.data(), p.edges.size(), st)) return rc;
        if (int rc = dev_put(&d_seg_first, p.seg_first.data(), p.seg_first.size(), st)) return rc;
        if (int rc = dev_put(&d_seg_chunk, p.seg_chunk.data(), p.seg_chunk.size(), st)) return rc;
        CM2_HIP(cm2::dev_malloc(&d_factor, sizeof(double) * (size_t)(p.nunits * packed(K))));
        CM2_HIP(cm2::dev_malloc(&d_partial, sizeof(double) * (size_t)(p.nsegs * K)));
        CM2_HIP(cm2::dev_malloc(&d_coeff, sizeof(double) * (size_t)(p.nunits * K)));
        CM2_HIP(cm2::dev_malloc(&d_skip, (size_t)p.nunits));
        return 0;
    }
    // after the factor kernel: nmark[c] = the units of class c
    int tally(const Geometry &p, hipStream_t st)
    {
        std::vector<uint8_t> marks((size_t)p.nunits);
        CM2_HIP(cm2::download(marks.data(), d_skip, marks.size(), st));
        CM2_HIP(hipStreamSynchronize(st));
        for (uint8_t m : marks) nmark[m < 3 ? m : 0]++;
        return 0;
    }
    void release() { dev_release(d_edges, d_seg_first, d_seg_chunk, d_factor, d_partial, d_coeff, d_skip); }
};

// the refusals of a create that both filters word alike.  ps is the Status of either policy and bad_size its kBadSize:
// kBadEdges and kTooLarge follow it in both (the policy headers assert it)
inline int check_create_status(const char *who, int ps, int bad_size, int64_t ns, int ndet, int64_t nchunks)
{
    CM2_CHECK(ps != bad_size, "%s: ns=%lld, ndet=%d, nchunks=%lld must all be >= 1", who, (long long)ns, ndet,
              (long long)nchunks);
    CM2_CHECK(ps != bad_size + 1, "%s: the %lld chunk edges must ascend strictly from 0 to ns=%lld", who,
              (long long)nchunks + 1, (long long)ns);
    CM2_CHECK(ps != bad_size + 2, "%s: ns=%lld x ndet=%d with %lld chunks overflows the index types", who,
              (long long)ns, ndet, (long long)nchunks);
    return 0;
}

}  // namespace chunkfit
}  // namespace cm2
