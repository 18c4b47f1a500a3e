// cm2_pca.hip -- the PCA filter (PCAFilterLO), see include/cosmomap2.h (f2g): the detector-detector covariance of
// every (chunk, group) unit on the fp64 MFMA, and the per-sample fit and removal of K modes that differ from chunk
// to chunk.  cm2_pca_policy.h has the accepted arguments, the work-item and slab tables and the LDS layout.
//
// Covariance (k_pca_cov): a workgroup owns one work item = (unit, tile pair (a, b <= a), segment).  It walks its
// segment in steps of kStep samples.  Per step the 256 threads read the two 128-row slabs from HBM along time (16
// consecutive lanes on 16 consecutive samples of one row, masked and padded with +0.0 on the way in) and stage them
// in LDS as [row][kPitch]; with kPitch = 18 the 8-byte operand reads of a half-wave (16 rows x 2 samples) fall on 64
// different banks.  The loads of step s + 1 are issued before the MFMAs of step s.  Wave (wr, wc) of the 2 x 2 waves
// holds the 64 x 64 block (wr, wc) of the tile in 4 x 4 accumulators of v_mfma_f64_16x16x4_f64 across the whole
// segment: operand A[m][k] = row-slab detector 16 ta + m at sample 4 q + k, B[k][n] = column-slab detector 16 tb + n
// at the same sample, q ascending.  A diagonal pair stages one slab and its wave (0, 1) does nothing (the upper
// triangle is the mirror); 16 x 16 results that hold no stored entry (beyond the group, or above the diagonal) are
// skipped and stay 0.  The partials go to the workspace, no atomics.
// k_pca_cov_final: one thread per stored entry (a, b); it adds the partials of the segments of entry
// (max(a, b), min(a, b)) in ascending segment order, starting from segment 0's, so both mirrors get the same bits.
//
// Apply, fit and class: the unit of cm2_modefit.h (shared with the common-mode filter) with Phi = the modes of the
// sample's chunk; a workgroup is one slab of the policy's table, so the chunk and with it Phi_c[k, :] is the same for
// the whole workgroup.  The order of every operation is the one written in cm2_modefit.h (steps 1 to 3), compiled
// with -ffp-contract=off.
#include <vector>

#include "cm2_modefit.h"
#include "cm2_pca_policy.h"

using namespace cm2;
namespace pp = cm2::pca;
namespace mf = cm2::modefit;

typedef double double4_t __attribute__((ext_vector_type(4)));
static_assert(pp::kSegment == CM2_PCA_SEGMENT && pp::kMaxK == CM2_PCA_MAX_K, "the header states the policy's constants");

namespace {

// ------------------------------------------------------------------------ covariance ----
constexpr int kRowsPerThread = pp::kTile / (pp::kThreads / pp::kStep);      // 8
constexpr int kRowStride = pp::kThreads / pp::kStep;                        // 16
constexpr int kSub = pp::kWaveTile / pp::kMfma;                             // 4

// the samples [i, i + 1) of the rows r0 + 16 j of a slab whose first detector is det0: 0 past the group or the
// segment, 0 where flagged
__device__ __forceinline__ void cov_fetch(const double *__restrict__ v, const int32_t *__restrict__ flags, int64_t ns,
                                          int64_t det0, int rows, int r0, int64_t i, bool live,
                                          double (&p)[kRowsPerThread])
{
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
        const int r = r0 + kRowStride * j;
        double x = 0.0;
        if (live && r < rows) {
            const int64_t at = (det0 + r) * ns + i;
            x = v[at];
            if (flags && flags[at] < 0) x = 0.0;
        }
        p[j] = x;
    }
}

__global__ __launch_bounds__(pp::kThreads) void k_pca_cov(const pp::CovItem *__restrict__ items, int64_t ns,
                                                           const double *__restrict__ v,
                                                           const int32_t *__restrict__ flags,
                                                           double *__restrict__ work)
{
    __shared__ double lds[2 * pp::kTile * pp::kPitch];
    const pp::CovItem it = items[blockIdx.x];
    const bool diag = it.row0 == it.col0;
    const int t = threadIdx.x, col = t % pp::kStep, r0 = t / pp::kStep;
    const int lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
    const int boff = diag ? 0 : pp::kTile * pp::kPitch;
    // the 16 x 16 results of this wave that hold a stored entry: block (a, b) needs rows and columns inside the group
    // and, on the diagonal of a diagonal pair, b <= a (the upper triangle is the mirror); wave (0, 1) of a diagonal
    // pair has none.  Wave-uniform, so a skipped block costs a branch, and a group of ten detectors one MFMA a quad.
    const int na = (it.rows - wr * pp::kWaveTile + pp::kMfma - 1) / pp::kMfma;
    const int nb = (it.cols - wc * pp::kWaveTile + pp::kMfma - 1) / pp::kMfma;
    const bool lower = diag && wr == wc;
    const bool idle = (diag && wc > wr) || na <= 0 || nb <= 0;
    double4_t acc[kSub][kSub];
#pragma unroll
    for (int a = 0; a < kSub; ++a)
#pragma unroll
        for (int b = 0; b < kSub; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int steps = (it.len + pp::kStep - 1) / pp::kStep;
    double pa[kRowsPerThread], pb[kRowsPerThread];
    cov_fetch(v, flags, ns, it.row0, it.rows, r0, it.first + col, col < it.len, pa);
    if (!diag) cov_fetch(v, flags, ns, it.col0, it.cols, r0, it.first + col, col < it.len, pb);
    for (int s = 0; s < steps; ++s) {
        __syncthreads();                                     // the MFMAs of the step before have read the slabs
#pragma unroll
        for (int j = 0; j < kRowsPerThread; ++j) {
            lds[pp::lds_at(r0 + kRowStride * j, col)] = pa[j];
            if (!diag) lds[boff + pp::lds_at(r0 + kRowStride * j, col)] = pb[j];
        }
        __syncthreads();
        if (s + 1 < steps) {
            const int k = (s + 1) * pp::kStep + col;
            cov_fetch(v, flags, ns, it.row0, it.rows, r0, it.first + k, k < it.len, pa);
            if (!diag) cov_fetch(v, flags, ns, it.col0, it.cols, r0, it.first + k, k < it.len, pb);
        }
        if (!idle) {
#pragma unroll
            for (int q = 0; q < pp::kStep / pp::kMfmaK; ++q) {
                double av[kSub], bv[kSub];
                const int k = pp::kMfmaK * q + (lane >> 4);
#pragma unroll
                for (int a = 0; a < kSub; ++a)
                    av[a] = lds[pp::lds_at(wr * pp::kWaveTile + a * pp::kMfma + (lane & 15), k)];
#pragma unroll
                for (int b = 0; b < kSub; ++b)
                    bv[b] = lds[boff + pp::lds_at(wc * pp::kWaveTile + b * pp::kMfma + (lane & 15), k)];
#pragma unroll
                for (int a = 0; a < kSub; ++a)
#pragma unroll
                    for (int b = 0; b < kSub; ++b)
                        if (a < na && b < nb && !(lower && b > a))
                            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
        }
    }
    // result register j of lane l is D[row (l >> 4) + 4 j][column l & 15]
#pragma unroll
    for (int a = 0; a < kSub; ++a)
#pragma unroll
        for (int b = 0; b < kSub; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = wr * pp::kWaveTile + a * pp::kMfma + (lane >> 4) + 4 * j;
                const int c = wc * pp::kWaveTile + b * pp::kMfma + (lane & 15);
                if (r < it.rows && c < it.cols) work[it.part + (int64_t)r * it.cols + c] = acc[a][b][j];
            }
}

// sq[g] = sum_{g' < g} n_g'^2 (ngroups + 1 entries)
__global__ __launch_bounds__(pp::kThreads) void k_pca_cov_final(int64_t total, int64_t per_chunk, int ngroups,
                                                                 const int64_t *__restrict__ sq,
                                                                 const pp::CovUnit *__restrict__ units,
                                                                 const pp::CovItem *__restrict__ items,
                                                                 const double *__restrict__ work,
                                                                 double *__restrict__ cov)
{
    const int64_t e = (int64_t)blockIdx.x * pp::kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t c = e / per_chunk, r = e - c * per_chunk;
    int lo = 0, hi = ngroups;                                // the group with sq[g] <= r < sq[g + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (sq[mid] <= r) lo = mid; else hi = mid;
    }
    const pp::CovUnit u = units[c * ngroups + lo];
    const int64_t local = r - sq[lo];
    int a = (int)(local / u.n), b = (int)(local - (int64_t)a * u.n);
    if (a < b) {
        const int x = a;
        a = b;
        b = x;
    }
    const int ta = a / pp::kTile, tb = b / pp::kTile;
    const int64_t first = u.first_item + ((int64_t)ta * (ta + 1) / 2 + tb) * u.nseg;
    const int64_t in_tile = (int64_t)(a - ta * pp::kTile) * items[first].cols + (b - tb * pp::kTile);
    double sum = work[items[first].part + in_tile];
    for (int s = 1; s < u.nseg; ++s) sum += work[items[first + s].part + in_tile];
    cov[e] = sum;
}

// ------------------------------------------------------------- apply, fit and class ----
struct Shape {
    int64_t ns, ndet, nslabs;
    const pp::Slab *slabs;          // [nslabs], device
    const int32_t *gedges;          // [ngroups + 1], device
    const double *modes;            // [nchunks][ndet][K], device
    const int32_t *pix;             // [ndet ns], device, borrowed
};

// the unit of this thread: its slab gives the sample and the chunk, the chunk the modes
template <int K>
__device__ __forceinline__ mf::Frame my_unit(const Shape &s)
{
    mf::Frame u;
    u.ns = s.ns;
    u.g = (int64_t)blockIdx.x / s.nslabs;
    const pp::Slab sl = s.slabs[(int64_t)blockIdx.x - u.g * s.nslabs];
    u.i = (int)threadIdx.x < sl.len ? sl.first + threadIdx.x : -1;      // past the slab's end: not the next slab's
    u.k0 = s.gedges[u.g];
    u.k1 = s.gedges[u.g + 1];
    u.phi = s.modes + (int64_t)sl.chunk * s.ndet * K;
    u.pix = s.pix;
    u.live = u.i >= 0;
    return u;
}

// the bodies, and why v and out are not __restrict__: cm2_modefit.h
template <int K>
__global__ __launch_bounds__(pp::kThreads) void k_pca_apply(Shape s, double tau, const double *v, double *out)
{
    mf::apply<K>(my_unit<K>(s), tau, v, out);
}

template <int K>
__global__ __launch_bounds__(pp::kThreads) void k_pca_fit(Shape s, double tau, const double *__restrict__ v,
                                                           double *__restrict__ coeff)
{
    mf::coefficients<K>(my_unit<K>(s), tau, v, coeff);
}

template <int K>
__global__ __launch_bounds__(pp::kThreads) void k_pca_class(Shape s, double tau, uint8_t *__restrict__ status,
                                                             unsigned long long *__restrict__ counts)
{
    mf::classify<K>([&] { return my_unit<K>(s); }, tau, status, counts);
}

}  // namespace

struct cm2_pca {
    pp::Plan plan;
    int64_t ns = 0, ndet = 0, ngroups = 0, nchunks = 0;
    int K = 0;
    bool modes_set = false;
    const int32_t *d_pix = nullptr;        // borrowed
    int32_t *d_gedges = nullptr;
    int64_t *d_sq = nullptr;
    pp::CovItem *d_items = nullptr;
    pp::CovUnit *d_units = nullptr;
    pp::Slab *d_slabs = nullptr;
    double *d_work = nullptr;
    double *d_modes = nullptr;
    uint8_t *d_status = nullptr;
    unsigned long long *d_counts = nullptr;
    int64_t nclass[4] = {0, 0, 0, 0};
    Shape shape() const { return Shape{ns, ndet, plan.slabs, d_slabs, d_gedges, d_modes, d_pix}; }
};

extern "C" int cm2_pca_destroy(cm2_pca *h)
{
    if (!h) return 0;
    dev_release(h->d_gedges, h->d_sq, h->d_items, h->d_units, h->d_slabs, h->d_work, h->d_modes, h->d_status,
                h->d_counts);
    delete h;
    return 0;
}

namespace {

int pca_fill(cm2_pca *h, const int64_t *gedges, const int64_t *cedges, hipStream_t st)
{
    std::vector<int32_t> e((size_t)h->ngroups + 1);
    std::vector<int64_t> sq((size_t)h->ngroups + 1, 0);
    for (size_t g = 0; g < e.size(); ++g) e[g] = (int32_t)gedges[g];
    for (int64_t g = 0; g < h->ngroups; ++g) sq[g + 1] = sq[g] + (gedges[g + 1] - gedges[g]) * (gedges[g + 1] - gedges[g]);
    std::vector<pp::CovItem> items;
    std::vector<pp::CovUnit> units;
    std::vector<pp::Slab> slabs;
    pp::cov_table(h->ngroups, gedges, h->nchunks, cedges, &items, &units);
    pp::slab_table(h->nchunks, cedges, &slabs);
    CM2_CHECK((int64_t)items.size() == h->plan.items && (int64_t)slabs.size() == h->plan.slabs &&
                  (int64_t)units.size() == h->plan.cov_units,
              "cm2_pca_create: the tables do not have the planned sizes");
    if (int rc = dev_put(&h->d_gedges, e.data(), e.size(), st)) return rc;
    if (int rc = dev_put(&h->d_sq, sq.data(), sq.size(), st)) return rc;
    if (int rc = dev_put(&h->d_items, items.data(), items.size(), st)) return rc;
    if (int rc = dev_put(&h->d_units, units.data(), units.size(), st)) return rc;
    if (int rc = dev_put(&h->d_slabs, slabs.data(), slabs.size(), st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_work, sizeof(double) * (size_t)h->plan.work_doubles));
    CM2_HIP(cm2::dev_malloc(&h->d_modes, sizeof(double) * (size_t)(h->nchunks * h->ndet * h->K)));
    CM2_HIP(cm2::dev_malloc(&h->d_status, (size_t)h->plan.units));
    CM2_HIP(cm2::dev_malloc(&h->d_counts, 4 * sizeof(unsigned long long)));
    CM2_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" int cm2_pca_create(cm2_pca **out, int64_t ns, int ndet, int ngroups, const int64_t *h_group_edges,
                              int64_t nchunks, const int64_t *h_chunk_edges, int K, const int32_t *d_pix, void *stream)
{
    const char *who = "cm2_pca_create";
    CM2_CHECK(out, "%s: null output handle", who);
    CM2_CHECK(h_group_edges && h_chunk_edges && d_pix, "%s: null array", who);
    pp::Plan p;
    const pp::Status ps = pp::check(&p, ns, ndet, ngroups, h_group_edges, nchunks, h_chunk_edges, K);
    if (int rc = mf::check_create_status(who, ps, ndet, ngroups, K)) return rc;
    CM2_CHECK(ps != pp::kBadSize, "%s: ns=%lld, ndet=%d, ngroups=%d, nchunks=%lld must all be >= 1", who,
              (long long)ns, ndet, ngroups, (long long)nchunks);
    CM2_CHECK(ps != pp::kBadChunks, "%s: the %lld chunk edges must ascend strictly from 0 to ns=%lld", who,
              (long long)nchunks + 1, (long long)ns);
    CM2_CHECK(ps == pp::kOk, "%s: ns=%lld x ndet=%d in %d groups and %lld chunks overflows the index types or a grid",
              who, (long long)ns, ndet, ngroups, (long long)nchunks);
    cm2_pca *h = new cm2_pca();
    h->plan = p;
    h->ns = ns;
    h->ndet = ndet;
    h->ngroups = ngroups;
    h->nchunks = nchunks;
    h->K = K;
    h->d_pix = d_pix;
    const int rc = pca_fill(h, h_group_edges, h_chunk_edges, as_stream(stream));
    if (rc) {
        cm2_pca_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_pca_info(const cm2_pca *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_pca_info: null argument");
    h_info[0] = h->ns;
    h_info[1] = h->ndet;
    h_info[2] = h->ngroups;
    h_info[3] = h->nchunks;
    h_info[4] = h->K;
    h_info[5] = h->plan.cov_doubles;
    h_info[6] = h->plan.work_doubles;
    h_info[7] = h->plan.items;
    h_info[8] = h->modes_set ? 1 : 0;
    for (int c = 0; c < 4; ++c) h_info[9 + c] = h->nclass[c];
    return 0;
}

extern "C" int64_t cm2_pca_cov_doubles(const cm2_pca *h) { return h ? h->plan.cov_doubles : -1; }

extern "C" int cm2_pca_cov(cm2_pca *h, const double *d_in, const int32_t *d_flags, double *d_cov, void *stream)
{
    CM2_CHECK(h, "cm2_pca_cov: null handle");
    CM2_CHECK(d_in && d_cov, "cm2_pca_cov: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_cov, h->plan.cov_doubles),
              "cm2_pca_cov: the covariance must not alias the input");
    CM2_CHECK(!bytes_overlap(d_flags, (uint64_t)h->plan.nt * sizeof(int32_t), d_cov,
                             (uint64_t)h->plan.cov_doubles * sizeof(double)),
              "cm2_pca_cov: the covariance must not alias the flags");
    hipStream_t st = as_stream(stream);
    k_pca_cov<<<dim3((unsigned)h->plan.items), pp::kThreads, 0, st>>>(h->d_items, h->ns, d_in, d_flags, h->d_work);
    CM2_LAUNCH_OK();
    k_pca_cov_final<<<dim3((unsigned)h->plan.final_blocks), pp::kThreads, 0, st>>>(
        h->plan.cov_doubles, h->plan.cov_per_chunk, (int)h->ngroups, h->d_sq, h->d_units, h->d_items, h->d_work, d_cov);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_pca_set_modes(cm2_pca *h, const double *d_modes, void *stream)
{
    CM2_CHECK(h, "cm2_pca_set_modes: null handle");
    CM2_CHECK(d_modes, "cm2_pca_set_modes: null modes");
    CM2_CHECK(pp::modes_allowed(h->plan.min_group, h->K),
              "cm2_pca_set_modes: every group needs at least K + 1 = %d detectors, the smallest has %lld", h->K + 1,
              (long long)h->plan.min_group);
    hipStream_t st = as_stream(stream);
    CM2_HIP(hipMemcpyAsync(h->d_modes, d_modes, sizeof(double) * (size_t)(h->nchunks * h->ndet * h->K),
                           hipMemcpyDeviceToDevice, st));
    auto launch_class = [&](auto K) {
        k_pca_class<K><<<dim3((unsigned)h->plan.blocks), pp::kThreads, 0, st>>>(h->shape(), CM2_PCA_TAU, h->d_status,
                                                                                h->d_counts);
    };
    if (int rc = mf::count_classes(h->K, launch_class, h->d_counts, st, h->nclass)) return rc;
    h->modes_set = true;
    return 0;
}

extern "C" int cm2_pca_apply(cm2_pca *h, const double *d_in, double *d_out, void *stream)
{
    CM2_CHECK(h, "cm2_pca_apply: null handle");
    CM2_CHECK(d_in && d_out, "cm2_pca_apply: null vector");
    CM2_CHECK(h->modes_set, "cm2_pca_apply: no modes are set (cm2_pca_set_modes)");
    CM2_CHECK(mf::apply_ok(d_in, d_out, h->plan.nt),
              "cm2_pca_apply: the output must be the input itself or not overlap it");
    dispatch_int<1, pp::kMaxK>(h->K, [&](auto K) {
        k_pca_apply<K><<<dim3((unsigned)h->plan.blocks), pp::kThreads, 0, as_stream(stream)>>>(h->shape(), CM2_PCA_TAU,
                                                                                               d_in, d_out);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_pca_fit(cm2_pca *h, const double *d_in, double *d_coeff, void *stream)
{
    CM2_CHECK(h, "cm2_pca_fit: null handle");
    CM2_CHECK(d_in && d_coeff, "cm2_pca_fit: null vector");
    CM2_CHECK(h->modes_set, "cm2_pca_fit: no modes are set (cm2_pca_set_modes)");
    CM2_CHECK(!ranges_overlap(d_in, h->plan.nt, d_coeff, h->plan.units * h->K),
              "cm2_pca_fit: the coefficients must not alias the input");
    dispatch_int<1, pp::kMaxK>(h->K, [&](auto K) {
        k_pca_fit<K><<<dim3((unsigned)h->plan.blocks), pp::kThreads, 0, as_stream(stream)>>>(h->shape(), CM2_PCA_TAU,
                                                                                             d_in, d_coeff);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_pca_status(const cm2_pca *h, uint8_t *d_status)
{
    CM2_CHECK(h && d_status, "cm2_pca_status: null argument");
    CM2_CHECK(h->modes_set, "cm2_pca_status: no modes are set (cm2_pca_set_modes)");
    return mf::copy_status(d_status, h->d_status, h->plan.units);
}
