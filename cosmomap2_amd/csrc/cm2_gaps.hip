// cm2_gaps.hip -- the flagged samples of a time stream: their index, and the kernels that fill them.
//
// The reference flags a sample with pix = -1 (flagging_subscan, utilities/IOfiles.py:142-152; bad pixels,
// process_ces.py:403-418); P and P^T skip such samples, the Toeplitz N^-1 (ToeplitzLO.mult,
// interfaces/linearoperators.py:582-595) does not.  With G the flagged samples, V the valid ones and Q = N^-1:
//
//   constrained fill   x_G = n_G + y,   Q_GG y = (Q u)_G,   u = 0 on G, n - d on V   (n = 0: the conditional mean
//                      -Q_GG^-1 Q_GV d_V, after which (Q d_filled)_V is the Schur complement applied to d_V)
//   linear fill        a straight line across every run between the mean levels of its two edges
//
// A cm2_gaps handle owns the index (ascending positions of the flagged samples, the table of runs cut at the
// block boundaries), the compact Jacobi vector 1 / a_0(block) and two nt-sized buffers: the scatter target, zero
// on V for its whole life, and the output of N^-1.  One application of Q_GG (cm2_gaps_normal_apply) is
// k_gap_scatter (ng writes), cm2_noise_apply, k_gap_gather (ng reads): the positions are ascending and the runs
// long, so a wave's 64 positions fall in a few cache lines and both kernels move 8-byte words at close to the rate
// of a contiguous copy.
//
// The gap-aware normal operator A_e = [P E]^T N^-1 [P E] (E = one unknown per flagged sample) on a tile plan goes
// through the time order, because a tile-order stream has no slot for a flagged sample:
//   k_P_tiles -> k_gap_perm_windows<true> (tile -> time order, g merged in) -> time-order N^-1
//             -> k_gap_perm_windows<false> (time -> tile order, g read out) -> fixed-order P^T
// The two permutations are the plan's windowed ones (cm2_tiles.hip) with the flagged samples of a window, the
// contiguous compact range [c_w, c_{w+1}), written into / read out of the LDS window beside the valid ones.
#include "cm2_common.h"
#include "cm2_perm_window.h"
#include "cm2_stream.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <vector>

using namespace cm2;

namespace {

// 1 where sample i is flagged (cm2_stream.h has the two kinds of flags)
template <int KIND>
struct FlagAt {
    const void *flags;
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return stream::flagged<KIND>(flags, i) ? 1u : 0u;
    }
};

// 1 where the j-th flagged sample starts a run: the first one, one whose predecessor in time is valid, or the
// first sample of a block
struct RunStartAt {
    const uint32_t *pos;
    const int64_t *off;
    int64_t nb;
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t j) const
    {
        if (j == 0) return 1u;
        const uint32_t t = pos[j];
        if (pos[j - 1] + 1u != t) return 1u;
        return off[stream::locate(off, nb, (int64_t)t)] == (int64_t)t ? 1u : 0u;
    }
};

// the run of the j-th flagged sample: the r with j0[r] <= j < j0[r + 1]
__device__ __forceinline__ int64_t run_of(const uint32_t *__restrict__ j0, int64_t nruns, uint32_t j)
{
    int64_t lo = 0, hi = nruns;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (j0[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// run r: start[r] = position of its first sample, blk[r] = its block
__global__ __launch_bounds__(256) void k_gap_runs(int64_t nruns, const uint32_t *__restrict__ pos,
                                                   const uint32_t *__restrict__ j0, const int64_t *__restrict__ off,
                                                   int64_t nb, uint32_t *__restrict__ start, int32_t *__restrict__ blk)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nruns; r += stride) {
        const uint32_t t = pos[j0[r]];
        start[r] = t;
        blk[r] = (int32_t)stream::locate(off, nb, (int64_t)t);
    }
}

// jac[j] = inva0[block of the j-th flagged sample]
__global__ __launch_bounds__(256) void k_gap_jacobi(int64_t ng, int64_t nruns, const uint32_t *__restrict__ j0,
                                                     const int32_t *__restrict__ blk,
                                                     const double *__restrict__ inva0, double *__restrict__ jac)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += stride)
        jac[j] = inva0[blk[run_of(j0, nruns, (uint32_t)j)]];
}

// compact <- stream
__global__ __launch_bounds__(256) void k_gap_gather(int64_t ng, const uint32_t *__restrict__ pos,
                                                     const double *__restrict__ s, double *__restrict__ c)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += stride) c[j] = s[pos[j]];
}

// stream <- compact, the ng positions only
__global__ __launch_bounds__(256) void k_gap_scatter(int64_t ng, const uint32_t *__restrict__ pos,
                                                      const double *__restrict__ c, double *__restrict__ s)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += stride) s[pos[j]] = c[j];
}

// u_i = 0 where flagged, n_i - d_i elsewhere (n == nullptr: n = 0).  A select: what d holds at a flagged sample
// (a NaN, say) is loaded and dropped, never multiplied by a mask.
template <int KIND>
__global__ __launch_bounds__(256) void k_gap_masked_diff(int64_t nt, const void *__restrict__ flags,
                                                          const double *__restrict__ n, const double *__restrict__ d,
                                                          double *__restrict__ u)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const double diff = (n ? n[i] : 0.0) - d[i];
        u[i] = stream::flagged<KIND>(flags, i) ? 0.0 : diff;
    }
}

// out_i = d_i on the valid samples, bit for bit; the flagged ones are left to k_gap_finish / k_gap_interp
template <int KIND>
__global__ __launch_bounds__(256) void k_gap_copy_valid(int64_t nt, const void *__restrict__ flags,
                                                         const double *__restrict__ d, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride)
        if (!stream::flagged<KIND>(flags, i)) out[i] = d[i];
}

// out at the j-th flagged sample = n there + y_j (n == nullptr: y_j)
__global__ __launch_bounds__(256) void k_gap_finish(int64_t ng, const uint32_t *__restrict__ pos,
                                                     const double *__restrict__ n, const double *__restrict__ y,
                                                     double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += stride) {
        const uint32_t t = pos[j];
        out[t] = n ? n[t] + y[j] : y[j];
    }
}

// One thread per run [s, s + len) of block [b0, b1): L = mean of the valid samples among the nedge before s inside
// the block, R = the same after the run, each summed in time order; a side without a valid sample takes the
// other side's level, 0 when both have none.  lr[2 r] = L, lr[2 r + 1] = R.
template <int KIND>
__global__ __launch_bounds__(256) void k_gap_edges(int64_t nruns, const uint32_t *__restrict__ start,
                                                    const uint32_t *__restrict__ j0, const int32_t *__restrict__ blk,
                                                    const int64_t *__restrict__ off, const void *__restrict__ flags,
                                                    const double *__restrict__ d, int64_t nedge,
                                                    double *__restrict__ lr)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nruns; r += stride) {
        const int64_t s = start[r], e = s + (int64_t)(j0[r + 1] - j0[r]);
        const int64_t b0 = off[blk[r]], b1 = off[blk[r] + 1];
        const int64_t lo = s - nedge > b0 ? s - nedge : b0, hi = e + nedge < b1 ? e + nedge : b1;
        double sl = 0.0, sr = 0.0;
        int64_t nl = 0, nr = 0;
        for (int64_t i = lo; i < s; ++i)
            if (!stream::flagged<KIND>(flags, i)) { sl += d[i]; ++nl; }
        for (int64_t i = e; i < hi; ++i)
            if (!stream::flagged<KIND>(flags, i)) { sr += d[i]; ++nr; }
        double L = nl ? sl / (double)nl : 0.0, R = nr ? sr / (double)nr : 0.0;
        if (!nl) L = R;
        if (!nr) R = L;
        lr[2 * r] = L;
        lr[2 * r + 1] = R;
    }
}

// One thread per flagged sample: sample s + k of a run of len samples becomes L + (R - L) (k + 1) / (len + 1)
__global__ __launch_bounds__(256) void k_gap_interp(int64_t ng, int64_t nruns, const uint32_t *__restrict__ pos,
                                                     const uint32_t *__restrict__ j0, const double *__restrict__ lr,
                                                     double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += stride) {
        const int64_t r = run_of(j0, nruns, (uint32_t)j);
        const double L = lr[2 * r], R = lr[2 * r + 1];
        const double k1 = (double)((uint32_t)j - j0[r] + 1u), len1 = (double)(j0[r + 1] - j0[r] + 1u);
        out[pos[j]] = L + ((R - L) * k1) / len1;
    }
}

// first[0] = the smallest sample whose flag differs between the tile plan (tb_dst == kInvalidSample) and the flags
template <int KIND>
__global__ __launch_bounds__(256) void k_gap_compare(int64_t nt, const void *__restrict__ flags,
                                                      const uint32_t *__restrict__ tb_dst,
                                                      uint32_t *__restrict__ first)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    flag_mismatch((int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride, nt, flags, tb_dst, first,
                  [](const void *__restrict__ f, int64_t i) { return stream::flagged<KIND>(f, i); });
}

// cw[w] = number of flagged samples before window w (lower_bound of w kPermWin in pos), w = 0 .. nwin
__global__ __launch_bounds__(256) void k_gap_window_table(int64_t nwin, int64_t ng, const uint32_t *__restrict__ pos,
                                                           uint32_t *__restrict__ cw)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= nwin; w += stride) {
        const int64_t t0 = w * kPermWin;
        int64_t lo = 0, hi = ng;                       // pos[j] < t0 for j < lo, pos[j] >= t0 for j >= hi
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)pos[mid] < t0) lo = mid + 1; else hi = mid;
        }
        cw[w] = (uint32_t)lo;
    }
}

// k_perm_windows (cm2_tiles.hip; the pieces: cm2_perm_window.h) with the flagged samples merged in.  TO_TIME: out[t] = in[tile position of t] on
// the valid samples and gc[c] at the c-th flagged one -- every slot of a window below its span is one or the
// other, so nothing is zero-filled (slots from span up are never read).  To tiles: out[tile position] = in[t] and
// gc[c] = in[pos[c]].  The flagged samples of window w are pos[cw[w] .. cw[w + 1]), read coalesced.
template <bool TO_TIME>
__global__ __launch_bounds__(kPermT) void k_gap_perm_windows(int64_t nt, int64_t nwin,
                                                              const uint32_t *__restrict__ lst_k,
                                                              const uint16_t *__restrict__ lst_q,
                                                              const uint32_t *__restrict__ pos,
                                                              const uint32_t *__restrict__ cw,
                                                              const double *__restrict__ in, double *__restrict__ out,
                                                              const double *__restrict__ gc_in,
                                                              double *__restrict__ gc_out)
{
    __shared__ double win[kPermWin];
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * kPermWin;
    const int span = (int)window_span(nt, t0);
    const int t = threadIdx.x;
    const uint32_t c0 = cw[w], c1 = cw[w + 1];
    WindowEntries e;
    e.load(lst_k, lst_q, w);
    if (TO_TIME) {
        double vv[kPermPer];
        e.gather(in, vv);
        e.each_valid([&](int u, uint32_t, uint16_t q) { win[q] = vv[u]; });
        for (uint32_t c = c0 + t; c < c1; c += kPermT) win[(int64_t)pos[c] - t0] = gc_in[c];
        __syncthreads();
        for (int j = t; j < span; j += kPermT) out[t0 + j] = win[j];
    } else {
        for (int j = t; j < span; j += kPermT) win[j] = in[t0 + j];
        __syncthreads();
        e.each_valid([&](int, uint32_t k, uint16_t q) { out[k] = win[q]; });
        for (uint32_t c = c0 + t; c < c1; c += kPermT) gc_out[c] = win[(int64_t)pos[c] - t0];
    }
}

}  // namespace

struct cm2_gaps {
    int64_t nt = 0, nb = 0, ng = 0, nruns = 0, longest = 0;
    int kind = 0;                     // 0: int32 flags (negative = flagged), 1: bytes (non-zero = flagged)
    const void *d_flags = nullptr;    // the caller's flags (kept alive and unchanged by the caller)
    int64_t *d_off = nullptr;         // [nb+1] block offsets
    uint32_t *d_pos = nullptr;        // [ng] positions of the flagged samples, ascending
    uint32_t *d_run_j0 = nullptr;     // [nruns+1] index into d_pos of each run's first sample; [nruns] = ng
    uint32_t *d_run_start = nullptr;  // [nruns] position of each run's first sample
    int32_t *d_run_blk = nullptr;     // [nruns] its block
    double *d_run_lr = nullptr;       // [2 nruns] edge levels of the linear fill
    double *d_jac = nullptr;          // [ng] 1 / a_0 of each flagged sample's block (handles made with h_a0)
    double *d_scatter = nullptr;      // [nt] scatter target: zero on the valid samples     (handles made with h_a0)
    double *d_work = nullptr;         // [nt] N^-1 of it                                     (handles made with h_a0)
    // cm2_gaps_prepare_tiles: the tile plan whose flagged samples were found equal to the handle's, and for its
    // windowed permutations the table of the windows' compact ranges
    uint64_t tiles_plan = 0;          // plan id (0: not prepared)
    int64_t nwin = 0;                 // windows of the table (0: the plan keeps the per-sample permutations)
    uint32_t *d_win_c = nullptr;      // [nwin+1] flagged samples before every window; [nwin] = ng
    std::vector<uint32_t> h_run_j0, h_run_start;
    std::vector<int32_t> h_run_blk;
};

extern "C" int cm2_gaps_destroy(cm2_gaps *g)
{
    if (!g) return 0;
    void *ptrs[] = {g->d_off, g->d_pos, g->d_run_j0, g->d_run_start, g->d_run_blk, g->d_run_lr, g->d_jac,
                    g->d_scatter, g->d_work, g->d_win_c};
    for (void *q : ptrs)
        if (q) (void)cm2::dev_free(q);
    delete g;
    return 0;
}

// ng and d_pos from the flags: a hipCUB sum of the flags, then a select of the sample numbers
template <int KIND>
static int gaps_positions(cm2_gaps *g, hipStream_t stream)
{
    using Count = hipcub::CountingInputIterator<uint32_t>;
    hipcub::TransformInputIterator<uint32_t, FlagAt<KIND>, Count> flag_it(Count(0u), FlagAt<KIND>{g->d_flags});
    DevTemp<uint32_t> d_count;
    DevTemp<char> d_temp;
    CM2_HIP(d_count.alloc(1));
    size_t tb = 0;
    CM2_HIP(hipcub::DeviceReduce::Sum(nullptr, tb, flag_it, d_count.p, g->nt, stream));
    CM2_HIP(d_temp.alloc(tb + 16));
    CM2_HIP(hipcub::DeviceReduce::Sum(d_temp.p, tb, flag_it, d_count.p, g->nt, stream));
    uint32_t ng = 0;
    CM2_HIP(cm2::download(&ng, d_count.p, sizeof(ng), stream));
    g->ng = ng;
    if (!ng) return 0;
    CM2_HIP(cm2::dev_malloc(&g->d_pos, sizeof(uint32_t) * g->ng));
    d_temp.release();
    CM2_HIP(hipcub::DeviceSelect::Flagged(nullptr, tb, Count(0u), flag_it, g->d_pos, d_count.p, g->nt, stream));
    CM2_HIP(d_temp.alloc(tb + 16));
    CM2_HIP(hipcub::DeviceSelect::Flagged(d_temp.p, tb, Count(0u), flag_it, g->d_pos, d_count.p, g->nt, stream));
    CM2_HIP(hipStreamSynchronize(stream));          // d_temp goes out of scope
    return 0;
}

// the run table from d_pos: the same sum and select over the run starts
static int gaps_runs(cm2_gaps *g, hipStream_t stream)
{
    using Count = hipcub::CountingInputIterator<uint32_t>;
    hipcub::TransformInputIterator<uint32_t, RunStartAt, Count> start_it(Count(0u),
                                                                           RunStartAt{g->d_pos, g->d_off, g->nb});
    DevTemp<uint32_t> d_count;
    DevTemp<char> d_temp;
    CM2_HIP(d_count.alloc(1));
    size_t tb = 0;
    CM2_HIP(hipcub::DeviceReduce::Sum(nullptr, tb, start_it, d_count.p, g->ng, stream));
    CM2_HIP(d_temp.alloc(tb + 16));
    CM2_HIP(hipcub::DeviceReduce::Sum(d_temp.p, tb, start_it, d_count.p, g->ng, stream));
    uint32_t nruns = 0;
    CM2_HIP(cm2::download(&nruns, d_count.p, sizeof(nruns), stream));
    g->nruns = nruns;
    CM2_HIP(cm2::dev_malloc(&g->d_run_j0, sizeof(uint32_t) * (g->nruns + 1)));
    CM2_HIP(cm2::dev_malloc(&g->d_run_start, sizeof(uint32_t) * g->nruns));
    CM2_HIP(cm2::dev_malloc(&g->d_run_blk, sizeof(int32_t) * g->nruns));
    CM2_HIP(cm2::dev_malloc(&g->d_run_lr, sizeof(double) * 2 * g->nruns));
    d_temp.release();
    CM2_HIP(hipcub::DeviceSelect::Flagged(nullptr, tb, Count(0u), start_it, g->d_run_j0, d_count.p, g->ng, stream));
    CM2_HIP(d_temp.alloc(tb + 16));
    CM2_HIP(hipcub::DeviceSelect::Flagged(d_temp.p, tb, Count(0u), start_it, g->d_run_j0, d_count.p, g->ng, stream));
    const uint32_t ng32 = (uint32_t)g->ng;
    CM2_HIP(cm2::upload(g->d_run_j0 + g->nruns, &ng32, sizeof(ng32), stream));
    k_gap_runs<<<grid_for(g->nruns), kBlock, 0, stream>>>(g->nruns, g->d_pos, g->d_run_j0, g->d_off, g->nb,
                                                           g->d_run_start, g->d_run_blk);
    CM2_LAUNCH_OK();
    g->h_run_j0.resize(g->nruns + 1);
    g->h_run_start.resize(g->nruns);
    g->h_run_blk.resize(g->nruns);
    CM2_HIP(cm2::download(g->h_run_j0.data(), g->d_run_j0, sizeof(uint32_t) * (g->nruns + 1), stream));
    CM2_HIP(cm2::download(g->h_run_start.data(), g->d_run_start, sizeof(uint32_t) * g->nruns, stream));
    CM2_HIP(cm2::download(g->h_run_blk.data(), g->d_run_blk, sizeof(int32_t) * g->nruns, stream));
    for (int64_t r = 0; r < g->nruns; ++r) {
        const int64_t len = (int64_t)g->h_run_j0[r + 1] - (int64_t)g->h_run_j0[r];
        if (len > g->longest) g->longest = len;
    }
    return 0;
}

static int gaps_build(cm2_gaps *g, const int64_t *h_sizes, const double *h_a0, hipStream_t stream)
{
    std::vector<int64_t> off(g->nb + 1, 0);
    for (int64_t b = 0; b < g->nb; ++b) {
        CM2_CHECK(h_sizes[b] > 0, "cm2_gaps_create: block %lld has non-positive size %lld", (long long)b,
                  (long long)h_sizes[b]);
        CM2_CHECK(h_sizes[b] <= g->nt - off[b], "cm2_gaps_create: the blocks add up to more than nt=%lld samples",
                  (long long)g->nt);
        off[b + 1] = off[b] + h_sizes[b];
    }
    CM2_CHECK(off[g->nb] == g->nt, "cm2_gaps_create: the blocks add up to %lld samples, nt=%lld",
              (long long)off[g->nb], (long long)g->nt);
    CM2_HIP(cm2::dev_malloc(&g->d_off, sizeof(int64_t) * (g->nb + 1)));
    CM2_HIP(cm2::upload(g->d_off, off.data(), sizeof(int64_t) * (g->nb + 1), stream));
    if (int rc = g->kind == 0 ? gaps_positions<0>(g, stream) : gaps_positions<1>(g, stream)) return rc;
    if (g->ng)
        if (int rc = gaps_runs(g, stream)) return rc;
    if (!h_a0) return 0;
    std::vector<double> inva0(g->nb);
    for (int64_t b = 0; b < g->nb; ++b) {
        CM2_CHECK(std::isfinite(h_a0[b]) && h_a0[b] > 0.0, "cm2_gaps_create: a_0 of block %lld is %g, not positive",
                  (long long)b, h_a0[b]);
        inva0[b] = 1.0 / h_a0[b];
    }
    CM2_HIP(cm2::dev_malloc(&g->d_scatter, sizeof(double) * g->nt));
    CM2_HIP(cm2::dev_malloc(&g->d_work, sizeof(double) * g->nt));
    CM2_HIP(hipMemsetAsync(g->d_scatter, 0, sizeof(double) * g->nt, stream));
    if (g->ng) {
        DevTemp<double> d_inva0;
        CM2_HIP(d_inva0.alloc(g->nb));
        CM2_HIP(cm2::upload(d_inva0.p, inva0.data(), sizeof(double) * g->nb, stream));
        CM2_HIP(cm2::dev_malloc(&g->d_jac, sizeof(double) * g->ng));
        k_gap_jacobi<<<grid_for(g->ng), kBlock, 0, stream>>>(g->ng, g->nruns, g->d_run_j0, g->d_run_blk, d_inva0.p,
                                                             g->d_jac);
        CM2_LAUNCH_OK();
        CM2_HIP(hipStreamSynchronize(stream));      // d_inva0 goes out of scope
    }
    CM2_HIP(hipStreamSynchronize(stream));
    return 0;
}

extern "C" int cm2_gaps_create(cm2_gaps **out, const void *d_flags, int flag_kind, int64_t nt, const int64_t *h_sizes,
                               int64_t nblocks, const double *h_a0, void *stream_)
{
    CM2_CHECK(out && d_flags && h_sizes, "cm2_gaps_create: NULL argument");
    *out = nullptr;
    CM2_CHECK(flag_kind == 0 || flag_kind == 1, "cm2_gaps_create: flag_kind=%d (0 = int32 pixel ids, 1 = bytes)",
              flag_kind);
    CM2_CHECK(nt >= 1, "cm2_gaps_create: nt=%lld < 1", (long long)nt);
    CM2_CHECK(nt < (int64_t)0xFFFFFFFFLL, "cm2_gaps_create: nt=%lld does not fit the 32-bit sample index",
              (long long)nt);
    CM2_CHECK(nblocks >= 1 && nblocks <= nt, "cm2_gaps_create: nblocks=%lld outside [1, nt]", (long long)nblocks);
    cm2_gaps *g = new cm2_gaps();
    g->nt = nt;
    g->nb = nblocks;
    g->kind = flag_kind;
    g->d_flags = d_flags;
    if (int rc = gaps_build(g, h_sizes, h_a0, as_stream(stream_))) {
        cm2_gaps_destroy(g);
        return rc;
    }
    *out = g;
    return 0;
}

extern "C" int cm2_gaps_info(const cm2_gaps *g, int64_t *h_info)
{
    CM2_CHECK(g && h_info, "cm2_gaps_info: NULL argument");
    h_info[0] = g->nt;
    h_info[1] = g->ng;
    h_info[2] = g->nruns;
    h_info[3] = g->longest;
    h_info[4] = g->d_scatter ? (int64_t)(2 * sizeof(double) * g->nt) : 0;
    return 0;
}

extern "C" int cm2_gaps_index(const cm2_gaps *g, uint32_t *h_pos, int64_t *h_runs, void *stream_)
{
    CM2_CHECK(g, "cm2_gaps_index: NULL argument");
    if (h_pos && g->ng) CM2_HIP(cm2::download(h_pos, g->d_pos, sizeof(uint32_t) * g->ng, as_stream(stream_)));
    if (h_runs)
        for (int64_t r = 0; r < g->nruns; ++r) {
            h_runs[3 * r] = g->h_run_start[r];
            h_runs[3 * r + 1] = (int64_t)g->h_run_j0[r + 1] - (int64_t)g->h_run_j0[r];
            h_runs[3 * r + 2] = g->h_run_blk[r];
        }
    return 0;
}

extern "C" int cm2_gaps_gather(const cm2_gaps *g, const double *d_stream, double *d_compact, void *stream_)
{
    CM2_CHECK(g, "cm2_gaps_gather: NULL argument");
    if (!g->ng) return 0;
    CM2_CHECK(d_stream && d_compact, "cm2_gaps_gather: NULL argument");
    k_gap_gather<<<grid_for(g->ng), kBlock, 0, as_stream(stream_)>>>(g->ng, g->d_pos, d_stream, d_compact);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_gaps_scatter(const cm2_gaps *g, const double *d_compact, double *d_stream, void *stream_)
{
    CM2_CHECK(g, "cm2_gaps_scatter: NULL argument");
    if (!g->ng) return 0;
    CM2_CHECK(d_stream && d_compact, "cm2_gaps_scatter: NULL argument");
    k_gap_scatter<<<grid_for(g->ng), kBlock, 0, as_stream(stream_)>>>(g->ng, g->d_pos, d_compact, d_stream);
    CM2_LAUNCH_OK();
    return 0;
}

// the operator must act on the same nt samples in the same number of blocks
static int gaps_check_noise(const cm2_gaps *g, cm2_noise *noise, const char *who)
{
    CM2_CHECK(g->d_scatter, "%s: the handle was made without a_0 and has no buffers", who);
    int64_t op[6] = {0, 0, 0, 0, 0, 0};
    if (int rc = cm2_noise_info(noise, op)) return rc;
    CM2_CHECK(op[0] == g->nt && op[1] == g->nb, "%s: the noise operator has %lld samples in %lld blocks, the gaps "
              "%lld in %lld", who, (long long)op[0], (long long)op[1], (long long)g->nt, (long long)g->nb);
    return 0;
}

extern "C" int cm2_gaps_normal_apply(cm2_gaps *g, cm2_noise *noise, const double *d_y, double *d_out, void *stream_)
{
    CM2_CHECK(g && noise, "cm2_gaps_normal_apply: NULL argument");
    if (int rc = gaps_check_noise(g, noise, "cm2_gaps_normal_apply")) return rc;
    if (!g->ng) return 0;
    CM2_CHECK(d_y && d_out, "cm2_gaps_normal_apply: NULL argument");
    if (int rc = cm2_gaps_scatter(g, d_y, g->d_scatter, stream_)) return rc;
    if (int rc = cm2_noise_apply(noise, g->d_scatter, g->d_work, stream_)) return rc;
    return cm2_gaps_gather(g, g->d_work, d_out, stream_);
}

extern "C" int cm2_gaps_precond_apply(const cm2_gaps *g, const double *d_r, double *d_z, void *stream_)
{
    CM2_CHECK(g, "cm2_gaps_precond_apply: NULL argument");
    if (!g->ng) return 0;
    CM2_CHECK(g->d_jac, "cm2_gaps_precond_apply: the handle was made without a_0");
    return cm2_xmy(g->ng, g->d_jac, d_r, d_z, stream_);
}

extern "C" int cm2_gaps_masked_diff(const cm2_gaps *g, const double *d_n, const double *d_d, double *d_u,
                                    void *stream_)
{
    CM2_CHECK(g && d_d && d_u, "cm2_gaps_masked_diff: NULL argument");
    CM2_CHECK(d_u != d_d && d_u != d_n, "cm2_gaps_masked_diff: d_u must not be one of the inputs");
    hipStream_t stream = as_stream(stream_);
    if (g->kind == 0)
        k_gap_masked_diff<0><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, d_n, d_d, d_u);
    else
        k_gap_masked_diff<1><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, d_n, d_d, d_u);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_gaps_rhs(cm2_gaps *g, cm2_noise *noise, const double *d_n, const double *d_d, double *d_u,
                            double *d_b, void *stream_)
{
    CM2_CHECK(g && noise, "cm2_gaps_rhs: NULL argument");
    if (int rc = gaps_check_noise(g, noise, "cm2_gaps_rhs")) return rc;
    if (!g->ng) return 0;
    CM2_CHECK(d_b, "cm2_gaps_rhs: NULL argument");
    if (int rc = cm2_gaps_masked_diff(g, d_n, d_d, d_u, stream_)) return rc;
    if (int rc = cm2_noise_apply(noise, d_u, g->d_work, stream_)) return rc;
    return cm2_gaps_gather(g, g->d_work, d_b, stream_);
}

static int gaps_copy_valid(const cm2_gaps *g, const double *d_d, double *d_out, hipStream_t stream)
{
    if (d_out == d_d) return 0;
    if (g->kind == 0)
        k_gap_copy_valid<0><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, d_d, d_out);
    else
        k_gap_copy_valid<1><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, d_d, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_gaps_finish(const cm2_gaps *g, const double *d_d, const double *d_n, const double *d_y,
                               double *d_out, void *stream_)
{
    CM2_CHECK(g && d_d && d_out, "cm2_gaps_finish: NULL argument");
    CM2_CHECK(d_out != d_n, "cm2_gaps_finish: d_out must not be d_n");
    hipStream_t stream = as_stream(stream_);
    if (int rc = gaps_copy_valid(g, d_d, d_out, stream)) return rc;
    if (!g->ng) return 0;
    CM2_CHECK(d_y, "cm2_gaps_finish: NULL argument");
    k_gap_finish<<<grid_for(g->ng), kBlock, 0, stream>>>(g->ng, g->d_pos, d_n, d_y, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_gaps_fill_linear(const cm2_gaps *g, const double *d_d, double *d_out, int64_t nedge, void *stream_)
{
    CM2_CHECK(g && d_d && d_out, "cm2_gaps_fill_linear: NULL argument");
    CM2_CHECK(nedge >= 1, "cm2_gaps_fill_linear: nedge=%lld < 1", (long long)nedge);
    if (nedge > g->nt) nedge = g->nt;               // no window reaches further, and s - nedge, e + nedge cannot wrap
    hipStream_t stream = as_stream(stream_);
    if (int rc = gaps_copy_valid(g, d_d, d_out, stream)) return rc;
    if (!g->ng) return 0;
    if (g->kind == 0)
        k_gap_edges<0><<<grid_for(g->nruns, kWave), kWave, 0, stream>>>(g->nruns, g->d_run_start, g->d_run_j0,
                                                                         g->d_run_blk, g->d_off, g->d_flags, d_d,
                                                                         nedge, g->d_run_lr);
    else
        k_gap_edges<1><<<grid_for(g->nruns, kWave), kWave, 0, stream>>>(g->nruns, g->d_run_start, g->d_run_j0,
                                                                         g->d_run_blk, g->d_off, g->d_flags, d_d,
                                                                         nedge, g->d_run_lr);
    CM2_LAUNCH_OK();
    k_gap_interp<<<grid_for(g->ng), kBlock, 0, stream>>>(g->ng, g->nruns, g->d_pos, g->d_run_j0, g->d_run_lr, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

// ------------------------------------------------- the gap-aware normal operator on a tile plan ------
extern "C" int cm2_gaps_prepare_tiles(cm2_gaps *g, const cm2_tiles *tiles, void *stream_)
{
    CM2_CHECK(g && tiles, "cm2_gaps_prepare_tiles: NULL argument");
    if (g->tiles_plan == tiles->plan_id) return 0;
    CM2_CHECK(tiles->nt == g->nt, "cm2_gaps_prepare_tiles: the tile plan has nt=%lld samples, the gaps nt=%lld",
              (long long)tiles->nt, (long long)g->nt);
    CM2_CHECK(tiles->nvalid + g->ng == g->nt, "cm2_gaps_prepare_tiles: the tile plan has %lld valid samples of "
              "%lld, the gaps flag %lld: not the same pointing", (long long)tiles->nvalid, (long long)g->nt,
              (long long)g->ng);
    hipStream_t stream = as_stream(stream_);
    uint32_t first = 0;
    auto compare = [&](uint32_t *d_first) {
        if (g->kind == 0)
            k_gap_compare<0><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, tiles->d_tb_dst, d_first);
        else
            k_gap_compare<1><<<grid_for(g->nt), kBlock, 0, stream>>>(g->nt, g->d_flags, tiles->d_tb_dst, d_first);
    };
    if (int rc = cm2::first_flag_mismatch(stream, compare, &first)) return rc;
    CM2_CHECK(first == kInvalidSample, "cm2_gaps_prepare_tiles: both flag %lld samples, but sample %u is flagged in "
              "one and valid in the other: not the same pointing", (long long)g->ng, first);
    bool windows = false;
    if (int rc = cm2::perm_lists(tiles, stream, &windows)) return rc;
    g->tiles_plan = 0;
    cm2::dev_release(g->d_win_c);
    g->nwin = 0;
    if (windows) {
        const int64_t nwin = tiles->nperm_win;
        CM2_HIP(cm2::dev_malloc(&g->d_win_c, sizeof(uint32_t) * (nwin + 1)));
        k_gap_window_table<<<grid_for(nwin + 1), kBlock, 0, stream>>>(nwin, g->ng, g->d_pos, g->d_win_c);
        CM2_LAUNCH_OK();
        CM2_HIP(hipStreamSynchronize(stream));
        g->nwin = nwin;
    }
    g->tiles_plan = tiles->plan_id;
    return 0;
}

extern "C" int cm2_gaps_window_table(const cm2_gaps *g, int64_t *h_nwin, uint32_t *h_table, void *stream_)
{
    CM2_CHECK(g && h_nwin, "cm2_gaps_window_table: NULL argument");
    *h_nwin = g->nwin;
    if (h_table && g->nwin)
        CM2_HIP(cm2::download(h_table, g->d_win_c, sizeof(uint32_t) * (g->nwin + 1), as_stream(stream_)));
    return 0;
}

static int gaps_check_tiles(const cm2_gaps *g, const cm2_tiles *tiles, const char *who)
{
    CM2_CHECK(g->tiles_plan == tiles->plan_id, "%s: cm2_gaps_prepare_tiles has not been called for this tile plan",
              who);
    CM2_CHECK(g->nwin == 0 || (g->nwin == tiles->nperm_win && tiles->d_perm_k && tiles->d_perm_q && g->d_win_c),
              "%s: the window table does not belong to the plan's lists", who);
    return 0;
}

extern "C" int cm2_gaps_tiles_to_time(const cm2_gaps *g, const cm2_tiles *tiles, const double *d_tb,
                                      const double *d_compact, double *d_time, void *stream_)
{
    CM2_CHECK(g && tiles && d_time && (d_tb || tiles->nvalid == 0) && (d_compact || g->ng == 0),
              "cm2_gaps_tiles_to_time: NULL argument");
    if (int rc = gaps_check_tiles(g, tiles, "cm2_gaps_tiles_to_time")) return rc;
    if (!g->nwin) {
        if (int rc = cm2_tod_tiles_to_time(tiles, d_tb, d_time, stream_)) return rc;
        return cm2_gaps_scatter(g, d_compact, d_time, stream_);
    }
    k_gap_perm_windows<true><<<window_grid(g->nwin), kPermT, 0, as_stream(stream_)>>>(
        g->nt, g->nwin, tiles->d_perm_k, tiles->d_perm_q, g->d_pos, g->d_win_c, d_tb, d_time, d_compact, nullptr);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_gaps_time_to_tiles(const cm2_gaps *g, const cm2_tiles *tiles, const double *d_time, double *d_tb,
                                      double *d_compact_out, void *stream_)
{
    CM2_CHECK(g && tiles && d_time && (d_tb || tiles->nvalid == 0) && (d_compact_out || g->ng == 0),
              "cm2_gaps_time_to_tiles: NULL argument");
    if (int rc = gaps_check_tiles(g, tiles, "cm2_gaps_time_to_tiles")) return rc;
    if (!g->nwin) {
        if (int rc = cm2_gaps_gather(g, d_time, d_compact_out, stream_)) return rc;
        return cm2_tod_time_to_tiles(tiles, d_time, d_tb, stream_);
    }
    k_gap_perm_windows<false><<<window_grid(g->nwin), kPermT, 0, as_stream(stream_)>>>(
        g->nt, g->nwin, tiles->d_perm_k, tiles->d_perm_q, g->d_pos, g->d_win_c, d_time, d_tb, nullptr,
        d_compact_out);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_PtNP_gaps_apply(const cm2_tiles *tiles, cm2_noise *noise, const cm2_gaps *g, const double *d_z,
                                   double *d_out, double *d_tb, double *d_time1, double *d_time2, void *stream_)
{
    CM2_CHECK(tiles && noise && g && d_z && d_out && d_tb && d_time1 && d_time2, "cm2_PtNP_gaps_apply: NULL argument");
    CM2_CHECK(d_time1 != d_time2 && d_z != d_out, "cm2_PtNP_gaps_apply: d_time1 / d_time2 and d_z / d_out must differ");
    if (int rc = gaps_check_tiles(g, tiles, "cm2_PtNP_gaps_apply")) return rc;
    int64_t op[6] = {0, 0, 0, 0, 0, 0};
    if (int rc = cm2_noise_info(noise, op)) return rc;
    CM2_CHECK(op[0] == g->nt && op[1] == g->nb && op[2] > 0, "cm2_PtNP_gaps_apply: the noise operator has %lld "
              "samples in %lld blocks (lambda %lld), the gaps %lld in %lld", (long long)op[0], (long long)op[1],
              (long long)op[2], (long long)g->nt, (long long)g->nb);
    const int64_t nmap = (int64_t)tiles->pol * tiles->npix;
    if (int rc = cm2_P_tiles_apply(tiles, d_z, d_tb, stream_)) return rc;
    if (int rc = cm2_gaps_tiles_to_time(g, tiles, d_tb, d_z + nmap, d_time1, stream_)) return rc;
    if (int rc = cm2_noise_apply(noise, d_time1, d_time2, stream_)) return rc;
    if (int rc = cm2_gaps_time_to_tiles(g, tiles, d_time2, d_tb, d_out + nmap, stream_)) return rc;
    return cm2_Pt_tiles_apply(tiles, d_tb, d_out, stream_);
}
