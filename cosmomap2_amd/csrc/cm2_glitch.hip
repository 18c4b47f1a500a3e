// cm2_glitch.hip -- glitch flags from the time streams, see include/cosmomap2.h (f2e): a running median per noise
// block, the robust scale of its residual by an exact rank selection, the threshold and the grown hits.
// cm2_glitch_policy.h has the accepted arguments, the tiers, the layout of threads over blocks and the digit split;
// cm2_stream.h how a kernel sees the stream, its flags and its blocks.
//
// Everything here is an order statistic, a comparison or an integer count: no floating-point sum whose order could
// matter, no floating-point atomic, no cross-lane operation on doubles.  The only arithmetic on doubles is
//   med = 0.5 v_lo + 0.5 v_hi (m even),  r = d - med,  sigma = 1.4826 s,  thr = nsigma sigma,
// each operation rounded on its own (the unit is compiled with -ffp-contract=off).
//
// k_glitch_median.  One thread walks one run of kRun consecutive outputs of a block and keeps the window of the
// current output as sorted keys: in registers (tiers 0-3, the sweeps fully unrolled over the tier's slots), or the
// first 96 in registers and the rest in LDS laid out [slot][thread] (tier 4; all lanes of a wave touch the same
// slot, so consecutive lanes hit consecutive banks).  A position outside the block and an unusable sample enter as the key +inf, m counts the real keys.  One
// step removes the departing key a (by value: the first slot that equals it) and inserts the arriving key b in ONE
// ascending sweep without a data-dependent branch: with v the sorted slots, u_j = v_j before the slot that held a and
// v_{j+1} from it on (u_last = +inf), and
//     new_j = max(u_{j-1}, min(u_j, b)),   u_{-1} = -inf,
// which costs one read and one write per slot.  The window of the first output is built by the same step from slots
// full of +inf (W steps that remove a +inf), W^2 / kRun slot visits per output on top of the W of the walk.
// Comparisons and selects only, never fmin / fmax: the keys keep their bits.
//
// k_glitch_hist / k_glitch_pick.  kDigits passes over the stream, most significant digit first.  A workgroup takes
// one tile of one block, counts in an LDS histogram the digit of the usable samples whose key matches the prefix
// fixed so far, and adds its non-empty bins to the block's histogram with integer atomics; k_glitch_pick then walks
// each block's histogram to the bin that holds the wanted rank, appends the digit to the prefix, reduces the rank
// and clears the histogram.  The sum of the first pass's bins is m_b.  A sample with r != 0 is usable by definition
// 3 (an unusable one has r = 0), so d is read only where r = 0 and neither flags nor prev decide.
//
// k_glitch_classify.  A workgroup takes one tile, stages one byte per sample of the tile and of its grow-wide halo
// (cut at the block) in LDS -- the class where the sample alone decides it, a hit mark, or 0 -- and then resolves
// the 0s to NEAR or CLEAN from the hit marks within grow.  Classes are tallied in LDS and added to counts[b][5] with
// integer atomics.
#include "cm2_common.h"
#include "cm2_glitch_policy.h"
#include "cm2_stream.h"

using namespace cm2;
using namespace cm2::stream;
namespace gp = cm2::glitch;

namespace {

constexpr uint64_t kAbsMask = 0x7FFFFFFFFFFFFFFFull;
constexpr uint8_t kHitMark = 0x80;         // staged byte of a hit (no class has this value)

// the selection's state of one block
struct Pick {
    unsigned long long prefix;             // the digits fixed so far
    long long rank;                        // the wanted rank among the samples that match the prefix
    long long m;                           // usable samples of the block
};

__device__ __forceinline__ double pos_inf() { return __longlong_as_double((long long)kExpMask); }
__device__ __forceinline__ bool carried_at(const Stream &s, int64_t i)
{
    if (!s.prev) return false;
    const uint8_t p = s.prev[i];
    return p == gp::kHit || p == gp::kNear;
}

// definition 1; *x = d_i
__device__ __forceinline__ bool usable_at(const Stream &s, int64_t i, double *x)
{
    *x = s.d[i];
    return !flagged_at(s, i) && finite_bits(*x) && !carried_at(s, i);
}

// the key of position p for the window of a block [lo, hi): d_p where usable, +inf elsewhere; *use = 1 for a real key
__device__ __forceinline__ double key_at(const Stream &s, int64_t p, int64_t lo, int64_t hi, int *use)
{
    *use = 0;
    if (p < lo || p >= hi) return pos_inf();
    double x;
    const bool u = usable_at(s, p, &x);
    *use = u ? 1 : 0;
    return u ? x : pos_inf();
}

// The sorted keys of one thread: the first RS slots in registers, every index a compile-time constant after unrolling;
// RS = SLOTS for tiers 0-3.  Tier 4 keeps the slots RS .. n - 1 of the n = W it was asked for in LDS, slot RS + j of
// this thread at col[j * THREADS].
template <int SLOTS, int RS, int THREADS>
struct Keys {
    static constexpr bool kLds = RS < SLOTS;
    double v[RS];
    double *col;
    int n;

    __device__ __forceinline__ void fill_inf()
    {
#pragma unroll
        for (int j = 0; j < RS; ++j) v[j] = pos_inf();
        if constexpr (kLds)
            for (int j = 0; j < n - RS; ++j) col[j * THREADS] = pos_inf();
    }

    // remove one key equal to a, insert b (the header of this file has the recurrence)
    __device__ __forceinline__ void step(double a, double b)
    {
        bool found = false;
        double below = -pos_inf(), cur = v[0];
#pragma unroll
        for (int j = 0; j < RS; ++j) {
            double next = pos_inf();
            if (j + 1 < RS) next = v[j + 1];
            else if constexpr (kLds) next = col[0];
            found = found || cur == a;
            const double u = found ? next : cur;
            const double lower = b < u ? b : u;
            v[j] = below > lower ? below : lower;
            below = u;
            cur = next;
        }
        if constexpr (kLds) {
            // kAhead slots a trip: their reads are issued together, before the first write of the trip
            constexpr int kAhead = 8;
            const int nl = n - RS;
            for (int j0 = 0; j0 < nl; j0 += kAhead) {
                double ahead[kAhead];
#pragma unroll
                for (int k = 0; k < kAhead; ++k)
                    ahead[k] = j0 + k + 1 < nl ? col[(j0 + k + 1) * THREADS] : pos_inf();
#pragma unroll
                for (int k = 0; k < kAhead; ++k) {
                    const double next = ahead[k];
                    found = found || cur == a;
                    const double u = found ? next : cur;
                    const double lower = b < u ? b : u;
                    if (j0 + k < nl) col[(j0 + k) * THREADS] = below > lower ? below : lower;
                    below = u;
                    cur = next;
                }
            }
        }
    }

    // the keys of rank lo and hi (0 <= lo <= hi < slots in use)
    __device__ __forceinline__ void pick(int lo, int hi, double *vlo, double *vhi) const
    {
        double x = v[0], y = v[0];
#pragma unroll
        for (int j = 1; j < RS; ++j) {
            x = j == lo ? v[j] : x;
            y = j == hi ? v[j] : y;
        }
        if constexpr (kLds) {
            if (lo >= RS) x = col[(lo - RS) * THREADS];
            if (hi >= RS) y = col[(hi - RS) * THREADS];
        }
        *vlo = x;
        *vhi = y;
    }
};

// A thread's keys arrive, leave and are subtracted at three positions of the stream, each kRun samples away from its
// neighbour lane's: read lane by lane, every load of a wave would touch 64 cache lines for 8 bytes each.  So the
// workgroup moves them in chunks of kChunk steps through LDS: stage[c][row][j] is the key of position
// first_row + off_c + j, loaded with consecutive threads on consecutive samples (kChunk doubles = 64 bytes a row), and
// the residuals go back the same way.  A row is padded to kChunk + 1 doubles: lane L reads its row at a stride of 18
// banks, which spreads a half-wave over all 64.
template <int SLOTS, int RS, int THREADS>
__global__ __launch_bounds__(THREADS) void k_glitch_median(Blocks t, int h, int64_t runs, Stream s,
                                                           double *__restrict__ r)
{
    constexpr int kChunk = gp::kChunk, kRows = THREADS / kChunk;
    static_assert(THREADS % kChunk == 0 && gp::kRun % kChunk == 0, "whole chunks");
    extern __shared__ double lds[];
    __shared__ double stage[3][THREADS][kChunk + 1];
    __shared__ int64_t row_first[THREADS], row_end[THREADS], row_lo[THREADS], row_hi[THREADS];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * THREADS + tid;
    {
        gp::Span sp;                               // a thread without a run: an empty span, every key +inf
        int64_t lo = 0, hi = 0;
        if (g < runs) {
            sp = gp::run_span(t.off, t.unit_start, t.nblocks, g);
            lo = t.off[sp.block];
            hi = t.off[sp.block + 1];
        }
        row_first[tid] = sp.first;
        row_end[tid] = sp.end;
        row_lo[tid] = lo;
        row_hi[tid] = hi;
    }
    // stage[c][row][j] = the key of position first_row + off + j, for every row of the workgroup
    auto load = [&](int c, int64_t off) {
        const int col = tid % kChunk;
#pragma unroll
        for (int row = tid / kChunk; row < THREADS; row += kRows) {
            int use;
            stage[c][row][col] = key_at(s, row_first[row] + off + col, row_lo[row], row_hi[row], &use);
        }
    };
    Keys<SLOTS, RS, THREADS> keys;
    keys.col = lds + tid;
    keys.n = 2 * h + 1;
    keys.fill_inf();
    const int W = 2 * h + 1;
    const double inf = pos_inf();
    int m = 0;
    __syncthreads();
    // the window of the sample before the first output: positions first - h - 1 .. first + h - 1, W keys
    for (int s0 = 0; s0 < W; s0 += kChunk) {
        load(0, (int64_t)(s0 - h - 1));
        __syncthreads();
        for (int j = 0; j < kChunk && s0 + j < W; ++j) {
            const double b = stage[0][tid][j];
            m += b != inf;
            keys.step(inf, b);
        }
        __syncthreads();
    }
    for (int k0 = 0; k0 < gp::kRun; k0 += kChunk) {
        load(0, (int64_t)(k0 + h));                // arriving
        load(1, (int64_t)k0);                      // the output's own
        load(2, (int64_t)(k0 - h - 1));            // departing
        __syncthreads();
        for (int j = 0; j < kChunk; ++j) {
            const double b = stage[0][tid][j], x = stage[1][tid][j], a = stage[2][tid][j];
            m += (b != inf) - (a != inf);
            keys.step(a, b);
            const int jlo = m > 0 ? (m - 1) / 2 : 0, jhi = m / 2;
            double vlo, vhi;
            keys.pick(jlo, jhi, &vlo, &vhi);
            const double med = (m & 1) ? vlo : 0.5 * vlo + 0.5 * vhi;
            stage[1][tid][j] = x != inf ? x - med : 0.0;       // (a usable sample is finite: +inf is no real key)
        }
        __syncthreads();
        const int col = tid % kChunk;
#pragma unroll
        for (int row = tid / kChunk; row < THREADS; row += kRows) {
            const int64_t p = row_first[row] + k0 + col;
            if (p < row_end[row]) r[p] = stage[1][row][col];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(gp::kTileThreads) void k_glitch_hist(Blocks t, int pass, Stream s,
                                                                  const double *__restrict__ r,
                                                                  const Pick *__restrict__ state,
                                                                  unsigned int *__restrict__ hist)
{
    __shared__ unsigned int bins[gp::kMaxBins];
    const gp::Span sp = gp::tile_span(t.off, t.unit_start, t.nblocks, (int64_t)blockIdx.x);
    const int nbins = gp::digit_bins(pass), shift = gp::digit_shift(pass);
    for (int j = threadIdx.x; j < nbins; j += gp::kTileThreads) bins[j] = 0u;
    __syncthreads();
    const unsigned long long mask = gp::prefix_mask(pass), prefix = pass ? state[sp.block].prefix : 0ull;
    for (int64_t i = sp.first + threadIdx.x; i < sp.end; i += gp::kTileThreads) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(r[i]) & kAbsMask;
        bool u = !flagged_at(s, i) && !carried_at(s, i);
        if (u && key == 0ull) u = finite_bits(s.d[i]);          // r = 0: usable or not, only d can tell
        if (u && (key & mask) == prefix) atomicAdd(&bins[(unsigned)(key >> shift) & (unsigned)(nbins - 1)], 1u);
    }
    __syncthreads();
    unsigned int *mine = hist + (size_t)sp.block * gp::kMaxBins;
    for (int j = threadIdx.x; j < nbins; j += gp::kTileThreads)
        if (bins[j]) atomicAdd(&mine[j], bins[j]);
}

// one workgroup per block: the bin that holds the wanted rank
__global__ __launch_bounds__(gp::kTileThreads) void k_glitch_pick(int pass, int W, double to_sigma,
                                                                  unsigned int *__restrict__ hist,
                                                                  Pick *__restrict__ state,
                                                                  double *__restrict__ sigma)
{
    __shared__ unsigned long long part[gp::kTileThreads];
    const int64_t b = blockIdx.x;
    unsigned int *mine = hist + (size_t)b * gp::kMaxBins;
    const int nbins = gp::digit_bins(pass), per = nbins / gp::kTileThreads;
    unsigned long long sum = 0;
    for (int k = 0; k < per; ++k) sum += mine[threadIdx.x * per + k];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        Pick p;
        if (pass == 0) {
            unsigned long long m = 0;
            for (int k = 0; k < gp::kTileThreads; ++k) m += part[k];
            p.prefix = 0ull;
            p.m = (long long)m;
            p.rank = m ? (long long)((m - 1) / 2) : 0;
        } else {
            p = state[b];
        }
        if (p.m > 0) {
            unsigned long long below = 0;
            int seg = 0;
            while (seg < gp::kTileThreads - 1 && below + part[seg] <= (unsigned long long)p.rank) below += part[seg++];
            int bin = seg * per;
            while (bin < seg * per + per - 1 && below + mine[bin] <= (unsigned long long)p.rank) below += mine[bin++];
            p.prefix |= (unsigned long long)bin << gp::digit_shift(pass);
            p.rank -= (long long)below;
        }
        state[b] = p;
        if (pass == gp::kDigits - 1)
            sigma[b] = p.m < W ? pos_inf() : to_sigma * __longlong_as_double((long long)p.prefix);
    }
    __syncthreads();
    for (int k = 0; k < per; ++k) mine[threadIdx.x * per + k] = 0u;
}

__global__ __launch_bounds__(gp::kTileThreads) void k_glitch_classify(Blocks t, Stream s, const double *__restrict__ r,
                                                                      const double *__restrict__ sigma, double nsigma,
                                                                      int grow, uint8_t *__restrict__ cls,
                                                                      unsigned long long *__restrict__ counts)
{
    __shared__ uint8_t stage[gp::kTile + 2 * gp::kMaxGrow];
    __shared__ unsigned int tally[gp::kClasses];
    const gp::Span sp = gp::tile_span(t.off, t.unit_start, t.nblocks, (int64_t)blockIdx.x);
    const int64_t lo = t.off[sp.block], hi = t.off[sp.block + 1];
    const double thr = nsigma * sigma[sp.block];
    if (threadIdx.x < gp::kClasses) tally[threadIdx.x] = 0u;
    // stage[p - base] for the samples p of [from, to): the tile and its halo, cut at the block
    const int64_t base = sp.first - grow;
    const int64_t from = base > lo ? base : lo, to = sp.end + grow < hi ? sp.end + grow : hi;
    for (int64_t p = from + threadIdx.x; p < to; p += gp::kTileThreads) {
        const double x = s.d[p];
        uint8_t c = 0;
        if (flagged_at(s, p)) c = gp::kInput;
        else if (!finite_bits(x)) c = gp::kNonfinite;
        else if (carried_at(s, p)) c = s.prev[p];
        else if (fabs(r[p]) > thr) c = kHitMark;
        stage[p - base] = c;
    }
    __syncthreads();
    for (int64_t i = sp.first + threadIdx.x; i < sp.end; i += gp::kTileThreads) {
        uint8_t c = stage[i - base];
        if (c == kHitMark) {
            c = gp::kHit;
        } else if (c == 0) {
            const int64_t a = i - grow > lo ? i - grow : lo, b = i + grow < hi - 1 ? i + grow : hi - 1;
            bool near = false;
            for (int64_t j = a; j <= b; ++j) near = near || stage[j - base] == kHitMark;      // (j = i holds a 0)
            c = near ? gp::kNear : gp::kClean;
        }
        cls[i] = c;
        atomicAdd(&tally[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < gp::kClasses && tally[threadIdx.x])
        atomicAdd(&counts[(size_t)sp.block * gp::kClasses + threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_glitch_apply_pix(int64_t nt, const uint8_t *__restrict__ cls,
                                                             int32_t *__restrict__ pix)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kBlock)
        if (cls[i]) pix[i] = -1;
}

}  // namespace

struct cm2_glitch {
    gp::Launch launch;
    BlockTables tables;                    // the blocks in runs (view 0) and in tiles (view 1)
    unsigned int *d_hist = nullptr;
    Pick *d_state = nullptr;
    int64_t bytes = 0;
    Blocks runs() const { return tables.view(0); }
    Blocks tiles() const { return tables.view(1); }
};

extern "C" int cm2_glitch_destroy(cm2_glitch *h)
{
    if (!h) return 0;
    dev_release(h->d_hist, h->d_state);
    delete h;
    return 0;
}

namespace {

int glitch_fill(cm2_glitch *h, const int64_t *sizes, hipStream_t st)
{
    const size_t nb = (size_t)h->launch.nblocks;
    if (int rc = h->tables.fill(sizes, h->launch.nblocks, {gp::kRun, gp::kTile}, st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_hist, (size_t)h->launch.hist_bytes));
    CM2_HIP(cm2::dev_malloc(&h->d_state, sizeof(Pick) * nb));
    CM2_HIP(hipMemsetAsync(h->d_hist, 0, (size_t)h->launch.hist_bytes, st));
    CM2_HIP(hipMemsetAsync(h->d_state, 0, sizeof(Pick) * nb, st));
    CM2_HIP(hipStreamSynchronize(st));
    h->bytes = h->tables.bytes() + (int64_t)(sizeof(Pick) * nb) + h->launch.hist_bytes;
    return 0;
}

// the checks the stream-sized calls share
int glitch_stream(const char *who, const cm2_glitch *h, const double *d_in, const void *d_flags, int flag_kind,
                  Stream *s, const uint8_t *d_prev)
{
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_in, "%s: null input", who);
    if (int rc = check_flag_kind_status(who, d_flags != nullptr, flag_kind)) return rc;
    *s = Stream{d_in, d_flags, flag_kind, d_prev};
    return 0;
}

template <int TIER>
int launch_median(const cm2_glitch *h, const Stream &s, double *d_r, hipStream_t st)
{
    constexpr int kSlots = gp::tier_slots(TIER), kThreads = gp::tier_threads(TIER);
    constexpr int kRegSlots = gp::tier_register_slots(TIER);
    auto kernel = k_glitch_median<kSlots, kRegSlots, kThreads>;
    if (kRegSlots < kSlots) {
        static size_t granted[64] = {0};
        CM2_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (size_t)h->launch.lds_bytes, granted));
    }
    kernel<<<dim3((unsigned)h->launch.median_blocks), kThreads, (size_t)h->launch.lds_bytes, st>>>(
        h->runs(), h->launch.h, h->launch.runs, s, d_r);
    CM2_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" int cm2_glitch_create(cm2_glitch **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int half_width,
                                 void *stream)
{
    const char *who = "cm2_glitch_create";
    CM2_CHECK(out, "%s: null output handle", who);
    gp::Launch l;
    const gp::Status ps = gp::check_create(&l, nt, h_sizes, nblocks, half_width);
    if (int rc = check_create_status(who, ps, nt, nblocks, "half_width", half_width, gp::kMaxHalfWidth,
                                     "the histograms")) return rc;
    cm2_glitch *h = new cm2_glitch();
    h->launch = l;
    const int rc = glitch_fill(h, h_sizes, as_stream(stream));
    if (rc) {
        cm2_glitch_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_glitch_info(const cm2_glitch *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_glitch_info: null argument");
    h_info[0] = h->launch.nt;
    h_info[1] = h->launch.nblocks;
    h_info[2] = h->launch.h;
    h_info[3] = gp::kRun;
    h_info[4] = h->launch.tier;
    h_info[5] = h->bytes;
    return 0;
}

extern "C" int cm2_glitch_residual(cm2_glitch *h, const double *d_in, const void *d_flags, int flag_kind,
                                   const uint8_t *d_prev, double *d_r, void *stream)
{
    const char *who = "cm2_glitch_residual";
    Stream s;
    if (int rc = glitch_stream(who, h, d_in, d_flags, flag_kind, &s, d_prev)) return rc;
    CM2_CHECK(d_r, "%s: null output", who);
    CM2_CHECK(!ranges_overlap(d_in, h->launch.nt, d_r, h->launch.nt), "%s: the residual must not overlap the input",
              who);
    switch (h->launch.tier) {
    case 0: return launch_median<0>(h, s, d_r, as_stream(stream));
    case 1: return launch_median<1>(h, s, d_r, as_stream(stream));
    case 2: return launch_median<2>(h, s, d_r, as_stream(stream));
    case 3: return launch_median<3>(h, s, d_r, as_stream(stream));
    default: return launch_median<4>(h, s, d_r, as_stream(stream));
    }
}

extern "C" int cm2_glitch_scale(cm2_glitch *h, const double *d_in, const double *d_r, const void *d_flags,
                                int flag_kind, const uint8_t *d_prev, double *d_sigma, void *stream)
{
    const char *who = "cm2_glitch_scale";
    Stream s;
    if (int rc = glitch_stream(who, h, d_in, d_flags, flag_kind, &s, d_prev)) return rc;
    CM2_CHECK(d_r && d_sigma, "%s: null residual or output", who);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks;
    CM2_CHECK(!bytes_overlap(d_sigma, 8 * nb, d_in, 8 * nt) && !bytes_overlap(d_sigma, 8 * nb, d_r, 8 * nt),
              "%s: sigma must not overlap the input or the residual", who);
    hipStream_t st = as_stream(stream);
    CM2_HIP(hipMemsetAsync(h->d_hist, 0, (size_t)h->launch.hist_bytes, st));
    for (int pass = 0; pass < gp::kDigits; ++pass) {
        k_glitch_hist<<<dim3((unsigned)h->launch.tiles), gp::kTileThreads, 0, st>>>(h->tiles(), pass, s, d_r,
                                                                                     h->d_state, h->d_hist);
        CM2_LAUNCH_OK();
        k_glitch_pick<<<dim3((unsigned)h->launch.nblocks), gp::kTileThreads, 0, st>>>(
            pass, 2 * h->launch.h + 1, CM2_GLITCH_MAD_TO_SIGMA, h->d_hist, h->d_state, d_sigma);
        CM2_LAUNCH_OK();
    }
    return 0;
}

extern "C" int cm2_glitch_classify(cm2_glitch *h, const double *d_in, const double *d_r, const void *d_flags,
                                   int flag_kind, const uint8_t *d_prev, const double *d_sigma, double nsigma, int grow,
                                   uint8_t *d_class, int64_t *d_counts, void *stream)
{
    const char *who = "cm2_glitch_classify";
    Stream s;
    if (int rc = glitch_stream(who, h, d_in, d_flags, flag_kind, &s, d_prev)) return rc;
    CM2_CHECK(d_r && d_sigma && d_class && d_counts, "%s: null residual, sigma or output", who);
    const gp::Status ps = gp::check_classify(nsigma, grow);
    CM2_CHECK(ps != gp::kBadNsigma, "%s: nsigma=%g must be finite and > 0", who, nsigma);
    CM2_CHECK(ps == gp::kOk, "%s: grow=%d outside [0, %d]", who, grow, gp::kMaxGrow);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks;
    const Range cls = {d_class, nt}, counts = {d_counts, 40 * nb}, in = {d_in, 8 * nt}, r = {d_r, 8 * nt},
                sigma = {d_sigma, 8 * nb};
    // a workgroup reads prev in the halo of its tile, where a neighbour may already have written: never in place
    if (int rc = check_disjoint(who, {cls}, {{d_prev, nt}}, "%s: the classes must not overlap prev (the halo of a tile "
                                "reads prev where another workgroup writes)")) return rc;
    if (int rc = check_disjoint(who, {cls}, {in, r, sigma, counts, {d_flags, flag_kind == 0 ? 4 * nt : nt}},
                                "%s: the classes must not overlap an input or the counts")) return rc;
    if (int rc = check_disjoint(who, {counts}, {in, r, sigma}, "%s: the counts must not overlap an input")) return rc;
    hipStream_t st = as_stream(stream);
    CM2_HIP(hipMemsetAsync(d_counts, 0, (size_t)(40 * nb), st));
    k_glitch_classify<<<dim3((unsigned)h->launch.tiles), gp::kTileThreads, 0, st>>>(
        h->tiles(), s, d_r, d_sigma, nsigma, grow, d_class, reinterpret_cast<unsigned long long *>(d_counts));
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_glitch_apply_pix(int64_t nt, const uint8_t *d_class, int32_t *d_pix, void *stream)
{
    const char *who = "cm2_glitch_apply_pix";
    CM2_CHECK(nt >= 1 && nt < (((int64_t)1 << 32) - 1), "%s: nt=%lld outside [1, 2^32 - 1)", who, (long long)nt);
    CM2_CHECK(d_class && d_pix, "%s: null array", who);
    CM2_CHECK(!bytes_overlap(d_class, (uint64_t)nt, d_pix, 4 * (uint64_t)nt), "%s: the classes overlap pix", who);
    k_glitch_apply_pix<<<grid_for(nt), kBlock, 0, as_stream(stream)>>>(nt, d_class, d_pix);
    CM2_LAUNCH_OK();
    return 0;
}
