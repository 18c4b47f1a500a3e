// cm2_offsets.hip -- destriping: the baseline-offset templates F and F^T on the GPU.
//
// The correlated noise of a time stream is modelled as one constant per stretch ("baseline") of L samples inside a
// noise block (cm2_offsets_policy.h has the arithmetic).  With valid = (pix >= 0) and w_b the white-noise weight of
// block b:
//   (F a)_t   = a_j(t) on the valid samples, 0 on the flagged ones            k_offsets_expand, k_offsets_to_tiles
//   (F^T y)_j = sum over the valid samples of baseline j of y_t               k_offsets_sum,    k_offsets_from_tiles
//   d0 - F a  = d_t - a_j(t) on the valid samples, 0 on the flagged ones      k_offsets_residual
// each optionally times w_b, applied ONCE per output (F^T factors it out of the sum).
//
// The summation order of F^T is fixed by (nt, blocks, L) alone and has no floating-point atomics.  A workgroup owns
// a window of 8192 consecutive time samples (counted from t = 0) in LDS, flagged slots zero.  window_sums():
//   1. thread c sums the chunk [32 c, 32 c + 32) serially, piece by piece (piece = chunk x baseline); a baseline
//      inside the chunk is finished there;
//   2. the pieces left open at the chunk ends go through a segmented inclusive scan over the 256 chunks (8 steps,
//      a piece adds the partial sum d chunks back while no baseline starts in between), so a segment's chunk
//      pieces are added in a fixed tree that depends on the segment's first chunk and length only;
//   3. the chunk in which a segment ends adds its own first piece to the scan's carry.
// A segment that is a whole baseline is written (times w_b) to the output; one of a baseline that crosses a window
// boundary goes to the window's head / tail slot of the side buffer and k_offsets_combine adds a baseline's slots in
// ascending window order.  The time-order and the tile-order form differ only in how the window reaches LDS, so
// they give the same bits.
//
// Tile-order forms work on the plan's windowed permutation lists (cm2_perm_window.h): to tiles, a thread takes its list
// entries (k, q), finds the baseline of sample t0 + q and stores w_b a_j at tile position k; from tiles, the window
// is gathered as k_perm_windows<true> does.  A stream shorter than one window has no lists: the time-order kernel
// and the plan's per-sample permutation serve.
#include "cm2_common.h"
#include "cm2_offsets_policy.h"
#include "cm2_perm_window.h"

#include <cmath>
#include <vector>

using namespace cm2;
namespace of = cm2::offsets;

static_assert(of::kWin == kPermWin && of::kChunks == kPermT, "the windows are the tile plan's permutation windows");

namespace {

constexpr size_t kSumLds = sizeof(double) * (of::kWinPadded + of::kChunks) + sizeof(int) * of::kChunks;

// the block table as the kernels read it
struct Table {
    const int64_t *off;     // [nb+1] first sample of every block
    const int64_t *j0;      // [nb+1] first baseline of every block
    const double *w;        // [nb] weights, nullptr: 1
    int64_t nb, L, nt;
};

__device__ __forceinline__ void emit(const Table &T, int64_t t0, int64_t w, const of::Baseline &s, double total,
                                     double *__restrict__ out, double *__restrict__ side)
{
    const of::Target tg = of::segment_target(s.start, s.end, t0);
    if (tg == of::kDirect) out[s.j] = T.w ? T.w[s.b] * total : total;
    else side[of::side_slot(w, tg)] = total;
}

// The per-baseline sums of window w, whose span samples lie in win (padded, flagged slots zero).  sv / sf: 256
// doubles / ints of LDS.  Called by all 256 threads; win must be complete (the caller has synchronised).
__device__ __forceinline__ void window_sums(const Table &T, int64_t w, int span, const double *win, double *sv,
                                            int *sf, double *__restrict__ out, double *__restrict__ side)
{
    const int c = threadIdx.x, a = c * of::kChunk;
    const int64_t t0 = w * of::kWin;
    double open = 0.0, first = 0.0;     // the piece left open at the chunk's end; the first piece when it ends here
    int fresh = 1;                      // the open piece starts in this chunk (or there is none)
    bool pending = false;               // the first piece continues a segment of earlier chunks and ends here
    of::Baseline ps = {0, 0, 0, 0};
    if (a < span) {
        const int end = a + of::kChunk < span ? a + of::kChunk : span;
        of::Baseline s = of::baseline_of(T.off, T.j0, T.nb, T.L, t0 + a);
        bool cont = a > 0 && s.start < t0 + a;
        int pos = a;
        while (true) {
            const int64_t e = s.end - t0;
            const int stop = e < (int64_t)end ? (int)e : end;
            double acc = 0.0;
            for (int i = pos; i < stop; ++i) acc += win[of::pad(i)];
            const bool closes = e <= (int64_t)end || end == span;
            if (cont) {
                if (closes) { pending = true; first = acc; ps = s; }
                else { open = acc; fresh = 0; }
            } else {
                if (closes) emit(T, t0, w, s, acc, out, side);
                else open = acc;
            }
            cont = false;
            pos = stop;
            if (pos >= end) break;
            s = of::next_baseline(T.off, T.j0, T.L, s);
        }
    }
    sv[c] = open;
    sf[c] = fresh;
    __syncthreads();
    for (int d = 1; d < of::kChunks; d <<= 1) {
        const bool take = c >= d && !sf[c];
        double v = 0.0;
        int f = 0;
        if (take) { v = sv[c - d]; f = sf[c - d]; }
        __syncthreads();
        if (take) { sv[c] = v + sv[c]; sf[c] = f; }
        __syncthreads();
    }
    if (pending) emit(T, t0, w, ps, sv[c - 1] + first, out, side);
}

// nvalid[j] += valid samples of every (32-sample run x baseline): integer atomics, once per handle
__global__ __launch_bounds__(256) void k_offsets_count(Table T, const int32_t *__restrict__ pix,
                                                        unsigned long long *__restrict__ nvalid)
{
    const int64_t nrun = (T.nt + of::kChunk - 1) / of::kChunk, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrun; r += stride) {
        int64_t pos = r * of::kChunk;
        const int64_t end = pos + of::kChunk < T.nt ? pos + of::kChunk : T.nt;
        of::Baseline s = of::baseline_of(T.off, T.j0, T.nb, T.L, pos);
        while (true) {
            const int64_t stop = s.end < end ? s.end : end;
            unsigned long long n = 0;
            for (int64_t i = pos; i < stop; ++i) n += pix[i] >= 0 ? 1u : 0u;
            if (n) atomicAdd(&nvalid[s.j], n);
            pos = stop;
            if (pos >= end) break;
            s = of::next_baseline(T.off, T.j0, T.L, s);
        }
    }
}

// wsum[j] = w_b nvalid[j]: one multiplication
__global__ __launch_bounds__(256) void k_offsets_wsum(Table T, int64_t na, const int64_t *__restrict__ nvalid,
                                                       double *__restrict__ wsum)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < na; j += stride) {
        const double n = (double)nvalid[j];
        wsum[j] = T.w ? T.w[of::block_of_baseline(T.j0, T.nb, j)] * n : n;
    }
}

// RES = false: out_t = [w_b] a_j(t);  RES = true: out_t = [w_b] (d_t - a_j(t)), a == nullptr: [w_b] d_t; 0 on the
// flagged samples.  A select: what d holds at a flagged sample is loaded and dropped.  out may be d.  A workgroup
// walks a window, a thread keeps the block of its last sample.
template <bool RES>
__device__ __forceinline__ void offsets_time(const Table &T, int64_t nwin, const int32_t *__restrict__ pix,
                                             const double *d, const double *__restrict__ a, double *out)
{
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * of::kWin;
    const int span = (int)window_span(T.nt, t0);
    if ((int)threadIdx.x >= span) return;
    int64_t b = of::block_of(T.off, T.nb, t0 + threadIdx.x);
    for (int i = threadIdx.x; i < span; i += kPermT) {
        const int64_t t = t0 + i;
        while (t >= T.off[b + 1]) ++b;
        double v = RES ? d[t] : 0.0;
        if (a) {
            const double aj = a[of::baseline_in_block(T.off, T.j0, b, T.L, t).j];
            v = RES ? v - aj : aj;
        }
        if (T.w) v = T.w[b] * v;
        out[t] = pix[t] >= 0 ? v : 0.0;
    }
}

__global__ __launch_bounds__(kPermT) void k_offsets_expand(Table T, int64_t nwin, const int32_t *__restrict__ pix,
                                                            const double *__restrict__ a, double *__restrict__ out)
{
    offsets_time<false>(T, nwin, pix, nullptr, a, out);
}

__global__ __launch_bounds__(kPermT) void k_offsets_residual(Table T, int64_t nwin, const int32_t *__restrict__ pix,
                                                              const double *d, const double *__restrict__ a,
                                                              double *out)
{
    offsets_time<true>(T, nwin, pix, d, a, out);
}

__global__ __launch_bounds__(kPermT) void k_offsets_sum(Table T, int64_t nwin, const int32_t *__restrict__ pix,
                                                         const double *__restrict__ y, double *__restrict__ out,
                                                         double *__restrict__ side)
{
    extern __shared__ double lds_sum[];
    double *win = lds_sum, *sv = lds_sum + of::kWinPadded;
    int *sf = reinterpret_cast<int *>(sv + of::kChunks);
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * of::kWin;
    const int span = (int)window_span(T.nt, t0);
    for (int i = threadIdx.x; i < span; i += kPermT) {
        const double v = y[t0 + i];
        win[of::pad(i)] = pix[t0 + i] >= 0 ? v : 0.0;
    }
    __syncthreads();
    window_sums(T, w, span, win, sv, sf, out, side);
}

__global__ __launch_bounds__(kPermT) void k_offsets_from_tiles(Table T, int64_t nwin,
                                                                const uint32_t *__restrict__ lst_k,
                                                                const uint16_t *__restrict__ lst_q,
                                                                const double *__restrict__ tb,
                                                                double *__restrict__ out, double *__restrict__ side)
{
    extern __shared__ double lds_sum[];
    double *win = lds_sum, *sv = lds_sum + of::kWinPadded;
    int *sf = reinterpret_cast<int *>(sv + of::kChunks);
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * of::kWin;
    const int span = (int)window_span(T.nt, t0);
    const int t = threadIdx.x;
    WindowEntries e;
    e.load(lst_k, lst_q, w);
    double vv[kPermPer];
    e.gather(tb, vv);
    for (int i = t; i < span; i += kPermT) win[of::pad(i)] = 0.0;      // flagged samples count as 0
    __syncthreads();
    // (not through each_valid: with the span guard inside a callable the compiler commutes the 32 compares and the
    // kernel no longer is the instruction stream it was)
#pragma unroll
    for (int u = 0; u < kPermPer; ++u)
        if (e.k[u] != kInvalidSample && (int)e.q[u] < span) win[of::pad(e.q[u])] = vv[u];
    __syncthreads();
    window_sums(T, w, span, win, sv, sf, out, side);
}

// tb[k] = [w_b] a_j(t0 + q) for the list entries (k, q) of the window; a is gathered (cache-resident)
__global__ __launch_bounds__(kPermT) void k_offsets_to_tiles(Table T, int64_t nwin,
                                                              const uint32_t *__restrict__ lst_k,
                                                              const uint16_t *__restrict__ lst_q,
                                                              const double *__restrict__ a, double *__restrict__ tb)
{
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * of::kWin, base = w * of::kWin;
    const int t = threadIdx.x;
    const int64_t b0 = of::block_of(T.off, T.nb, t0);
#pragma unroll 4
    for (int u = 0; u < kPermPer; ++u) {
        const uint32_t k = lst_k[base + t + u * kPermT];
        const int64_t ts = t0 + lst_q[base + t + u * kPermT];
        if (k == kInvalidSample || ts >= T.nt) continue;
        int64_t b = b0;
        while (ts >= T.off[b + 1]) ++b;
        const double aj = a[of::baseline_in_block(T.off, T.j0, b, T.L, ts).j];
        tb[k] = T.w ? T.w[b] * aj : aj;
    }
}

// One thread per window boundary: the baseline that crosses it and started in the window before is finished here,
// its slots added in ascending window order
__global__ __launch_bounds__(256) void k_offsets_combine(Table T, int64_t nwin, const double *__restrict__ side,
                                                          double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwin; w += stride) {
        of::Baseline s;
        if (!of::combines_at(T.off, T.j0, T.nb, T.L, w, &s)) continue;
        double acc = side[of::side_slot(w - 1, of::kTail)];
        for (int64_t v = w; v * of::kWin < s.end; ++v) acc += side[of::side_slot(v, of::kHead)];
        out[s.j] = T.w ? T.w[s.b] * acc : acc;
    }
}

// first[0] = the smallest sample whose flag differs between the tile plan (tb_dst == kInvalidSample) and pix
__global__ __launch_bounds__(256) void k_offsets_compare(int64_t nt, const int32_t *__restrict__ pix,
                                                          const uint32_t *__restrict__ tb_dst,
                                                          uint32_t *__restrict__ first)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    flag_mismatch((int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride, nt, pix, tb_dst, first,
                  [](const int32_t *__restrict__ p, int64_t i) { return p[i] < 0; });
}

}  // namespace

struct cm2_offsets {
    int64_t nt = 0, nb = 0, L = 0, Lc = 0, na = 0, nwin = 0, nvalid = 0;
    const int32_t *d_pix = nullptr;   // the caller's pixel stream (kept alive and unchanged by the caller)
    bool weighted = false;
    int64_t *d_off = nullptr;         // [nb+1]
    int64_t *d_j0 = nullptr;          // [nb+1]
    double *d_w = nullptr;            // [nb] (handles made with weights)
    int64_t *d_nvalid = nullptr;      // [na]
    double *d_wsum = nullptr;         // [na]
    double *d_side = nullptr;         // [2 nwin] head / tail slots of F^T
    // cm2_offsets_prepare_tiles
    uint64_t tiles_plan = 0;          // plan id (0: not prepared)
    bool windows = false;             // the plan has windowed permutation lists
    double *d_time = nullptr;         // [nt] time-order scratch of the tile forms of a plan without lists
};

static Table table_of(const cm2_offsets *f, bool weighted)
{
    return Table{f->d_off, f->d_j0, weighted ? f->d_w : nullptr, f->nb, f->Lc, f->nt};
}

extern "C" int cm2_offsets_destroy(cm2_offsets *f)
{
    if (!f) return 0;
    cm2::dev_release(f->d_off, f->d_j0, f->d_w, f->d_nvalid, f->d_wsum, f->d_side, f->d_time);
    delete f;
    return 0;
}

static int offsets_build(cm2_offsets *f, const std::vector<int64_t> &off, const std::vector<int64_t> &j0,
                         const double *h_w, hipStream_t stream)
{
    CM2_HIP(cm2::dev_malloc(&f->d_off, sizeof(int64_t) * (f->nb + 1)));
    CM2_HIP(cm2::dev_malloc(&f->d_j0, sizeof(int64_t) * (f->nb + 1)));
    CM2_HIP(cm2::upload(f->d_off, off.data(), sizeof(int64_t) * (f->nb + 1), stream));
    CM2_HIP(cm2::upload(f->d_j0, j0.data(), sizeof(int64_t) * (f->nb + 1), stream));
    if (h_w) {
        CM2_HIP(cm2::dev_malloc(&f->d_w, sizeof(double) * f->nb));
        CM2_HIP(cm2::upload(f->d_w, h_w, sizeof(double) * f->nb, stream));
    }
    CM2_HIP(cm2::dev_malloc(&f->d_nvalid, sizeof(int64_t) * f->na));
    CM2_HIP(cm2::dev_malloc(&f->d_wsum, sizeof(double) * f->na));
    CM2_HIP(cm2::dev_malloc(&f->d_side, sizeof(double) * of::side_slots(f->nwin)));
    CM2_HIP(hipMemsetAsync(f->d_nvalid, 0, sizeof(int64_t) * f->na, stream));
    CM2_HIP(hipMemsetAsync(f->d_side, 0, sizeof(double) * of::side_slots(f->nwin), stream));
    const Table T = table_of(f, true);
    k_offsets_count<<<grid_for((f->nt + of::kChunk - 1) / of::kChunk), kBlock, 0, stream>>>(
        T, f->d_pix, reinterpret_cast<unsigned long long *>(f->d_nvalid));
    CM2_LAUNCH_OK();
    k_offsets_wsum<<<grid_for(f->na), kBlock, 0, stream>>>(T, f->na, f->d_nvalid, f->d_wsum);
    CM2_LAUNCH_OK();
    std::vector<int64_t> h(f->na);
    CM2_HIP(cm2::download(h.data(), f->d_nvalid, sizeof(int64_t) * f->na, stream));
    f->nvalid = 0;
    for (int64_t n : h) f->nvalid += n;
    return 0;
}

extern "C" int cm2_offsets_create(cm2_offsets **out, const int32_t *d_pix, int64_t nt, const int64_t *h_sizes,
                                  int64_t nblocks, int64_t baseline_length, const double *h_weights, void *stream_)
{
    CM2_CHECK(out && d_pix && h_sizes, "cm2_offsets_create: NULL argument");
    *out = nullptr;
    CM2_CHECK(nt >= 1, "cm2_offsets_create: nt=%lld < 1", (long long)nt);
    CM2_CHECK(nt < (int64_t)0xFFFFFFFFLL, "cm2_offsets_create: nt=%lld does not fit the 32-bit sample index",
              (long long)nt);
    CM2_CHECK(nblocks >= 1 && nblocks <= nt, "cm2_offsets_create: nblocks=%lld outside [1, nt]", (long long)nblocks);
    CM2_CHECK(baseline_length >= 1, "cm2_offsets_create: baseline_length=%lld < 1", (long long)baseline_length);
    const int64_t Lc = baseline_length < nt ? baseline_length : nt;    // no baseline is longer than the stream
    std::vector<int64_t> off(nblocks + 1, 0), j0(nblocks + 1, 0);
    for (int64_t b = 0; b < nblocks; ++b) {
        CM2_CHECK(h_sizes[b] > 0, "cm2_offsets_create: block %lld has non-positive size %lld", (long long)b,
                  (long long)h_sizes[b]);
        CM2_CHECK(h_sizes[b] <= nt - off[b], "cm2_offsets_create: the blocks add up to more than nt=%lld samples",
                  (long long)nt);
        off[b + 1] = off[b] + h_sizes[b];
        j0[b + 1] = j0[b] + of::baselines_in(h_sizes[b], Lc);
        CM2_CHECK(!h_weights || (std::isfinite(h_weights[b]) && h_weights[b] > 0.0),
                  "cm2_offsets_create: the weight of block %lld is %g, not positive and finite", (long long)b,
                  h_weights ? h_weights[b] : 0.0);
    }
    CM2_CHECK(off[nblocks] == nt, "cm2_offsets_create: the blocks add up to %lld samples, nt=%lld",
              (long long)off[nblocks], (long long)nt);
    CM2_CHECK(j0[nblocks] < ((int64_t)1 << 31), "cm2_offsets_create: %lld baselines do not fit the 31-bit baseline "
              "index", (long long)j0[nblocks]);
    cm2_offsets *f = new cm2_offsets();
    f->nt = nt;
    f->nb = nblocks;
    f->L = baseline_length;
    f->Lc = Lc;
    f->na = j0[nblocks];
    f->nwin = (nt + of::kWin - 1) / of::kWin;
    f->d_pix = d_pix;
    f->weighted = h_weights != nullptr;
    if (int rc = offsets_build(f, off, j0, h_weights, as_stream(stream_))) {
        cm2_offsets_destroy(f);
        return rc;
    }
    *out = f;
    return 0;
}

extern "C" int cm2_offsets_info(const cm2_offsets *f, int64_t *h_info)
{
    CM2_CHECK(f && h_info, "cm2_offsets_info: NULL argument");
    h_info[0] = f->nt;
    h_info[1] = f->nb;
    h_info[2] = f->L;
    h_info[3] = f->na;
    h_info[4] = f->nvalid;
    h_info[5] = f->nwin;
    h_info[6] = f->tiles_plan ? (f->windows ? 1 : 2) : 0;     // tile forms: 0 not prepared, 1 windows, 2 per sample
    h_info[7] = (int64_t)kSumLds;
    return 0;
}

extern "C" int cm2_offsets_counts(const cm2_offsets *f, int64_t *h_nvalid, double *h_wsum, void *stream_)
{
    CM2_CHECK(f, "cm2_offsets_counts: NULL argument");
    if (h_nvalid) CM2_HIP(cm2::download(h_nvalid, f->d_nvalid, sizeof(int64_t) * f->na, as_stream(stream_)));
    if (h_wsum) CM2_HIP(cm2::download(h_wsum, f->d_wsum, sizeof(double) * f->na, as_stream(stream_)));
    return 0;
}

static int check_weighted(int weighted, const char *who)
{
    CM2_CHECK(weighted == 0 || weighted == 1, "%s: weighted=%d (0 or 1)", who, weighted);
    return 0;
}

extern "C" int cm2_offsets_expand(const cm2_offsets *f, const double *d_a, int weighted, double *d_out, void *stream_)
{
    CM2_CHECK(f && d_a && d_out, "cm2_offsets_expand: NULL argument");
    if (int rc = check_weighted(weighted, "cm2_offsets_expand")) return rc;
    CM2_CHECK(d_out != d_a, "cm2_offsets_expand: d_out must not be d_a");
    k_offsets_expand<<<window_grid(f->nwin), kPermT, 0, as_stream(stream_)>>>(table_of(f, weighted != 0), f->nwin,
                                                                               f->d_pix, d_a, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_offsets_residual(const cm2_offsets *f, const double *d_d, const double *d_a, int weighted,
                                    double *d_out, void *stream_)
{
    CM2_CHECK(f && d_d && d_out, "cm2_offsets_residual: NULL argument");
    if (int rc = check_weighted(weighted, "cm2_offsets_residual")) return rc;
    CM2_CHECK(d_out != d_a, "cm2_offsets_residual: d_out must not be d_a");
    k_offsets_residual<<<window_grid(f->nwin), kPermT, 0, as_stream(stream_)>>>(
        table_of(f, weighted != 0), f->nwin, f->d_pix, d_d, d_a, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

static int offsets_combine(const cm2_offsets *f, const Table &T, double *d_out, hipStream_t stream)
{
    if (f->nwin < 2) return 0;
    k_offsets_combine<<<grid_for(f->nwin - 1), kBlock, 0, stream>>>(T, f->nwin, f->d_side, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_offsets_sum(cm2_offsets *f, const double *d_y, int weighted, double *d_out, void *stream_)
{
    CM2_CHECK(f && d_y && d_out, "cm2_offsets_sum: NULL argument");
    if (int rc = check_weighted(weighted, "cm2_offsets_sum")) return rc;
    CM2_CHECK(d_out != d_y, "cm2_offsets_sum: d_out must not be d_y");
    hipStream_t stream = as_stream(stream_);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds((const void *)k_offsets_sum, kSumLds, granted));
    const Table T = table_of(f, weighted != 0);
    k_offsets_sum<<<window_grid(f->nwin), kPermT, kSumLds, stream>>>(T, f->nwin, f->d_pix, d_y, d_out, f->d_side);
    CM2_LAUNCH_OK();
    return offsets_combine(f, T, d_out, stream);
}

// ------------------------------------------------------------------------ on a tile plan ------
extern "C" int cm2_offsets_prepare_tiles(cm2_offsets *f, const cm2_tiles *tiles, void *stream_)
{
    CM2_CHECK(f && tiles, "cm2_offsets_prepare_tiles: NULL argument");
    if (f->tiles_plan == tiles->plan_id) return 0;
    CM2_CHECK(tiles->nt == f->nt, "cm2_offsets_prepare_tiles: the tile plan has nt=%lld samples, the offsets nt=%lld",
              (long long)tiles->nt, (long long)f->nt);
    CM2_CHECK(tiles->nvalid == f->nvalid, "cm2_offsets_prepare_tiles: the tile plan has %lld valid samples of %lld, "
              "the offsets count %lld: not the same pointing", (long long)tiles->nvalid, (long long)f->nt,
              (long long)f->nvalid);
    hipStream_t stream = as_stream(stream_);
    uint32_t first = 0;
    auto compare = [&](uint32_t *d_first) {
        k_offsets_compare<<<grid_for(f->nt), kBlock, 0, stream>>>(f->nt, f->d_pix, tiles->d_tb_dst, d_first);
    };
    if (int rc = cm2::first_flag_mismatch(stream, compare, &first)) return rc;
    CM2_CHECK(first == kInvalidSample, "cm2_offsets_prepare_tiles: both have %lld valid samples, but sample %u is "
              "flagged in one and valid in the other: not the same pointing", (long long)f->nvalid, first);
    bool windows = false;
    if (int rc = cm2::perm_lists(tiles, stream, &windows)) return rc;
    f->tiles_plan = 0;
    if (!windows && !f->d_time) CM2_HIP(cm2::dev_malloc(&f->d_time, sizeof(double) * f->nt));
    f->windows = windows;
    f->tiles_plan = tiles->plan_id;
    return 0;
}

static int offsets_check_tiles(const cm2_offsets *f, const cm2_tiles *tiles, const char *who)
{
    CM2_CHECK(f->tiles_plan == tiles->plan_id, "%s: cm2_offsets_prepare_tiles has not been called for this tile "
              "plan", who);
    CM2_CHECK(f->windows ? (tiles->nperm_win == f->nwin && tiles->d_perm_k && tiles->d_perm_q) : f->d_time != nullptr,
              "%s: the plan's window lists do not fit the offsets' windows", who);
    return 0;
}

extern "C" int cm2_offsets_to_tiles(const cm2_offsets *f, const cm2_tiles *tiles, const double *d_a, int weighted,
                                    double *d_tb, void *stream_)
{
    CM2_CHECK(f && tiles && d_a && (d_tb || tiles->nvalid == 0), "cm2_offsets_to_tiles: NULL argument");
    if (int rc = check_weighted(weighted, "cm2_offsets_to_tiles")) return rc;
    if (int rc = offsets_check_tiles(f, tiles, "cm2_offsets_to_tiles")) return rc;
    if (!f->windows) {
        if (int rc = cm2_offsets_expand(f, d_a, weighted, f->d_time, stream_)) return rc;
        return cm2_tod_time_to_tiles(tiles, f->d_time, d_tb, stream_);
    }
    k_offsets_to_tiles<<<window_grid(f->nwin), kPermT, 0, as_stream(stream_)>>>(
        table_of(f, weighted != 0), f->nwin, tiles->d_perm_k, tiles->d_perm_q, d_a, d_tb);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_offsets_from_tiles(cm2_offsets *f, const cm2_tiles *tiles, const double *d_tb, int weighted,
                                      double *d_out, void *stream_)
{
    CM2_CHECK(f && tiles && d_out && (d_tb || tiles->nvalid == 0), "cm2_offsets_from_tiles: NULL argument");
    if (int rc = check_weighted(weighted, "cm2_offsets_from_tiles")) return rc;
    if (int rc = offsets_check_tiles(f, tiles, "cm2_offsets_from_tiles")) return rc;
    if (!f->windows) {
        if (int rc = cm2_tod_tiles_to_time(tiles, d_tb, f->d_time, stream_)) return rc;
        return cm2_offsets_sum(f, f->d_time, weighted, d_out, stream_);
    }
    hipStream_t stream = as_stream(stream_);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds((const void *)k_offsets_from_tiles, kSumLds, granted));
    const Table T = table_of(f, weighted != 0);
    k_offsets_from_tiles<<<window_grid(f->nwin), kPermT, kSumLds, stream>>>(T, f->nwin, tiles->d_perm_k,
                                                                             tiles->d_perm_q, d_tb, d_out, f->d_side);
    CM2_LAUNCH_OK();
    return offsets_combine(f, T, d_out, stream);
}
