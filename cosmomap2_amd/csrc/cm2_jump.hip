// cm2_jump.hip -- baseline jumps of the time streams, see include/cosmomap2.h (f2f): the step statistic t of every
// position from two window means, its robust scale (the selection of cm2_glitch), the jumps as the local maxima of |t|
// beyond the threshold, their accumulated offsets, and the corrected stream with its classes.
// cm2_jump_policy.h has the accepted arguments, the tiles and what a tile of the statistic kernel holds in LDS;
// cm2_stream.h how a kernel sees the stream, its flags and its blocks.
//
// The floating-point operations are the ones of the definition, each rounded on its own (the unit is compiled with
// -ffp-contract=off): the w additions of a window sum in ascending sample order from +0.0, two divisions and one
// subtraction per position, nsigma sigma, the chain of the offsets, d - s.  No floating-point atomic, no cross-lane
// operation on doubles; the counts are integers.
//
// k_jump_stat.  A workgroup takes one tile [first, end) of one block and stages in LDS the samples from first - w on,
// an unusable sample and a position outside the block as +0.0 (x + +0.0 has the bits of x for every x a sum that
// started from +0.0 can hold, so the sums need no branch), and the running count C of the usable ones, n_j =
// C[j + w] - C[j].  Thread t then forms the sums of the starts t, t + 256, ... side by side: kStarts independent chains
// of additions, every LDS read of a wave 64 consecutive doubles.  R_i is L_{i+w}: every sum is formed once per tile
// and parked in LDS for the positions that need it as L and as R.
//
// k_jump_peaks.  |t| of the tile and of w positions on either side in LDS, -1 where the position is not evaluable or
// outside the block (no |t| is below 0, so such a position is neither a candidate nor a rival).  A candidate looks at
// its 2 w neighbours; candidates are few.  One mark byte per position, the jumps of the tile added to njumps[b].
// hipCUB's DeviceSelect::Flagged makes the ascending table of positions from the marks, through an output iterator
// that drops what lies beyond the caller's capacity.
//
// k_jump_offsets.  One thread per block: its slice of the table by two bisections, the heights a = t[p] and the chain
// s_m = s_{m-1} + a_m.
//
// k_jump_correct.  A workgroup takes one tile and bisects the table once for the entries within radius of it; a
// sample then bisects that short range (empty for nearly every tile) for m(i): the entry before gives the offset and
// whether the sample is a jump, the entries on either side whether one lies within radius.
#include <iterator>

#include <hipcub/hipcub.hpp>

#include "cm2_common.h"
#include "cm2_jump_policy.h"
#include "cm2_stream.h"

using namespace cm2;
using namespace cm2::stream;
namespace jp = cm2::jump;

namespace {

// rule 1; *x = d_i
__device__ __forceinline__ bool usable_at(const Stream &s, int64_t i, double *x)
{
    *x = s.d[i];
    return !flagged_at(s, i) && finite_bits(*x) && !(s.prev && s.prev[i] != 0);
}

__global__ __launch_bounds__(jp::kTileThreads) void k_jump_stat(Blocks tb, int w, int min_count, Stream s,
                                                                 double *__restrict__ t, uint8_t *__restrict__ noeval)
{
    extern __shared__ double lds[];
    __shared__ unsigned int wave_total[jp::kTileThreads / kWave];
    const int nvals = jp::stat_values(w), tid = threadIdx.x;
    double *vals = lds, *S = lds + nvals;
    uint16_t *C = reinterpret_cast<uint16_t *>(S + jp::stat_starts());        // C[v] = usable among vals[0, v)
    const jp::Span sp = jp::tile_span(tb.off, tb.unit_start, tb.nblocks, (int64_t)blockIdx.x);
    const int64_t lo = tb.off[sp.block], hi = tb.off[sp.block + 1];
    const int len = (int)(sp.end - sp.first);
    const int64_t base = sp.first - w;                                        // the sample of vals[0]
    const int need = len + 2 * w;                                             // values the tile's sums read (one less)
    for (int v = tid; v < nvals; v += jp::kTileThreads) {
        const int64_t p = base + v;
        double x = 0.0;
        bool u = false;
        if (v < need && p >= lo && p < hi) u = usable_at(s, p, &x);
        vals[v] = u ? x : 0.0;
        C[v + 1] = u ? 1 : 0;
    }
    if (tid == 0) C[0] = 0;
    __syncthreads();
    // the running count: a thread's own stretch, the stretches of a wave by integer shuffles, the four waves
    {
        const int per = (nvals + jp::kTileThreads - 1) / jp::kTileThreads;
        const int v0 = tid * per < nvals ? tid * per : nvals, v1 = v0 + per < nvals ? v0 + per : nvals;
        unsigned int run = 0;
        for (int v = v0; v < v1; ++v) {
            run += C[v + 1];
            C[v + 1] = (uint16_t)run;
        }
        unsigned int incl = run;
        const int lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned int up = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += up;
        }
        if (lane == kWave - 1) wave_total[wave] = incl;
        __syncthreads();
        unsigned int before = incl - run;
        for (int k = 0; k < wave; ++k) before += wave_total[k];
        for (int v = v0; v < v1; ++v) C[v + 1] = (uint16_t)(C[v + 1] + before);
    }
    // rule 2: the sums of the starts base + tid + 256 m, side by side
    const int nstarts = len + w;
    const int rounds = (nstarts + jp::kTileThreads - 1) / jp::kTileThreads;
    double acc[jp::kStarts];
#pragma unroll
    for (int m = 0; m < jp::kStarts; ++m) acc[m] = 0.0;
    for (int k = 0; k < w; ++k) {
#pragma unroll
        for (int m = 0; m < jp::kStarts; ++m)
            if (m < rounds) acc[m] = acc[m] + vals[m * jp::kTileThreads + tid + k];
    }
#pragma unroll
    for (int m = 0; m < jp::kStarts; ++m)
        if (m < rounds) S[m * jp::kTileThreads + tid] = acc[m];
    __syncthreads();
    // rule 3: position first + q has L = S[q] (the start q samples after base) and R = S[q + w]
    for (int q = tid; q < len; q += jp::kTileThreads) {
        const int64_t p = sp.first + q;
        bool ev = p - w >= lo && p + w <= hi;
        const int nL = (int)C[q + w] - (int)C[q], nR = (int)C[q + 2 * w] - (int)C[q + w];
        double x = 0.0;
        if (ev && nL >= min_count && nR >= min_count) {
            x = S[q + w] / (double)nR - S[q] / (double)nL;
            ev = finite_bits(x);
        } else {
            ev = false;
        }
        t[p] = ev ? x : 0.0;
        noeval[p] = ev ? 0 : 1;
    }
}

__global__ __launch_bounds__(jp::kTileThreads) void k_jump_peaks(Blocks tb, int w, const double *__restrict__ t,
                                                                  const uint8_t *__restrict__ noeval,
                                                                  const double *__restrict__ sigma, double nsigma,
                                                                  uint8_t *__restrict__ mark,
                                                                  unsigned long long *__restrict__ njumps)
{
    __shared__ double a[jp::kTile + 2 * jp::kMaxWindow];
    __shared__ unsigned int tally;
    const jp::Span sp = jp::tile_span(tb.off, tb.unit_start, tb.nblocks, (int64_t)blockIdx.x);
    const int64_t lo = tb.off[sp.block], hi = tb.off[sp.block + 1];
    const int len = (int)(sp.end - sp.first);
    const int64_t base = sp.first - w;
    const double thr = nsigma * sigma[sp.block];                              // rule 5, one multiplication
    if (threadIdx.x == 0) tally = 0u;
    for (int v = threadIdx.x; v < len + 2 * w; v += jp::kTileThreads) {
        const int64_t p = base + v;
        a[v] = p >= lo && p < hi && !noeval[p] ? fabs(t[p]) : -1.0;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < len; q += jp::kTileThreads) {
        const double c = a[q + w];
        bool jump = c > thr;
        if (jump) {
            for (int j = 1; j <= w; ++j)                                      // rule 6: an equal one before p wins
                jump = jump && !(a[q + w - j] >= c) && !(a[q + w + j] > c);
            if (jump) atomicAdd(&tally, 1u);
        }
        mark[sp.first + q] = jump ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0 && tally) atomicAdd(&njumps[sp.block], (unsigned long long)tally);
}

// the entries of the table that exist: the jumps found, or the capacity
__device__ __forceinline__ int64_t table_size(const int64_t *total, int64_t capacity)
{
    return *total < capacity ? *total : capacity;
}

__global__ __launch_bounds__(kBlock) void k_jump_offsets(const int64_t *__restrict__ off, int64_t nblocks,
                                                         const int64_t *__restrict__ pos,
                                                         const int64_t *__restrict__ total, int64_t capacity,
                                                         const double *__restrict__ t, double *__restrict__ heights,
                                                         double *__restrict__ offsets)
{
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = table_size(total, capacity);
    if (b >= nblocks || n == 0) return;
    const int64_t k0 = jp::table_lower(pos, n, off[b]), k1 = jp::table_lower(pos, n, off[b + 1]);
    double sum = 0.0;
    for (int64_t k = k0; k < k1; ++k) {                                       // rule 8: s_m = s_{m-1} + a_m
        const double height = t[pos[k]];
        sum = sum + height;
        heights[k] = height;
        offsets[k] = sum;
    }
}

__global__ __launch_bounds__(jp::kTileThreads) void k_jump_correct(Blocks tb, const double *d_in,
                                                                    const uint8_t *__restrict__ prev,
                                                                    const int64_t *__restrict__ pos,
                                                                    const double *__restrict__ offsets,
                                                                    const int64_t *__restrict__ total,
                                                                    int64_t capacity, int radius, double *d_out,
                                                                    uint8_t *__restrict__ cls,
                                                                    unsigned long long *__restrict__ counts)
{
    __shared__ int64_t range[2];
    __shared__ unsigned int tally[jp::kCounts];
    const jp::Span sp = jp::tile_span(tb.off, tb.unit_start, tb.nblocks, (int64_t)blockIdx.x);
    const int64_t lo = tb.off[sp.block], hi = tb.off[sp.block + 1], n = table_size(total, capacity);
    if (threadIdx.x < jp::kCounts) tally[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        // the entries within radius of the tile, cut at the block
        const int64_t from = sp.first - radius > lo ? sp.first - radius : lo;
        const int64_t to = sp.end + radius < hi ? sp.end + radius : hi;
        range[0] = jp::table_lower(pos, n, from);
        range[1] = jp::table_lower(pos, n, to);
    }
    __syncthreads();
    const int64_t k0 = range[0], k1 = range[1];
    for (int64_t i = sp.first + threadIdx.x; i < sp.end; i += jp::kTileThreads) {
        const int64_t k = k0 + jp::table_upper(pos + k0, k1 - k0, i);        // entries <= i; the entry k is beyond i
        const bool before = k > 0 && pos[k - 1] >= lo;                        // a jump of this block at or before i
        const double s = before ? offsets[k - 1] : 0.0;
        const bool at = before && pos[k - 1] == i;
        const int64_t kl = at ? k - 2 : k - 1;                                // the nearest jump before i
        const bool near = (kl >= 0 && pos[kl] >= lo && i - pos[kl] <= radius) ||
                          (k < n && pos[k] < hi && pos[k] - i <= radius);
        const uint8_t pv = prev ? prev[i] : 0;
        const uint8_t c = at ? jp::kAt : near ? jp::kNear : jp::kClean;
        d_out[i] = d_in[i] - s;
        cls[i] = pv ? pv : c;
        if (!pv) atomicAdd(&tally[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < jp::kCounts && tally[threadIdx.x])
        atomicAdd(&counts[(size_t)sp.block * jp::kCounts + threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// writes pos[i] for i < capacity and drops the rest: the select reports the true count and stays inside the table
struct CappedOut {
    using iterator_category = std::random_access_iterator_tag;
    using value_type = int64_t;
    using difference_type = std::ptrdiff_t;
    using pointer = int64_t *;
    struct Slot {
        int64_t *q;
        __host__ __device__ Slot &operator=(int64_t v)
        {
            if (q) *q = v;
            return *this;
        }
    };
    using reference = Slot;
    int64_t *pos;
    int64_t capacity, at;
    __host__ __device__ Slot operator[](difference_type i) const
    {
        return Slot{at + i < capacity ? pos + at + i : nullptr};
    }
    __host__ __device__ Slot operator*() const { return (*this)[0]; }
    __host__ __device__ CappedOut operator+(difference_type i) const { return CappedOut{pos, capacity, at + i}; }
};

// the ascending table of the marked positions; d_temp = NULL: only *temp_bytes
hipError_t select_marked(void *d_temp, size_t *temp_bytes, const uint8_t *d_mark, int64_t nt, int64_t *d_pos,
                         int64_t capacity, int64_t *d_total, hipStream_t st)
{
    return hipcub::DeviceSelect::Flagged(d_temp, *temp_bytes, hipcub::CountingInputIterator<int64_t>(0), d_mark,
                                         CappedOut{d_pos, capacity, 0}, d_total, nt, st);
}

}  // namespace

struct cm2_jump {
    jp::Launch launch;
    BlockTables tables;                    // the blocks in tiles
    uint8_t *d_mark = nullptr;             // [nt] the jumps of the last cm2_jump_find
    char *d_temp = nullptr;                // the select's
    size_t temp_bytes = 0;
    cm2_glitch *scale = nullptr;           // half-width 1: its selection gives the scale of t
    int64_t bytes = 0;
    Blocks tiles() const { return tables.view(0); }
};

extern "C" int cm2_jump_destroy(cm2_jump *h)
{
    if (!h) return 0;
    cm2_glitch_destroy(h->scale);
    dev_release(h->d_mark, h->d_temp);
    delete h;
    return 0;
}

namespace {

int jump_fill(cm2_jump *h, const int64_t *sizes, void *stream)
{
    hipStream_t st = as_stream(stream);
    const size_t nt = (size_t)h->launch.nt;
    if (int rc = h->tables.fill(sizes, h->launch.nblocks, {jp::kTile}, st)) return rc;
    CM2_HIP(cm2::dev_malloc(&h->d_mark, nt));
    CM2_HIP(select_marked(nullptr, &h->temp_bytes, h->d_mark, h->launch.nt, nullptr, 1, nullptr, st));
    CM2_HIP(cm2::dev_malloc(&h->d_temp, h->temp_bytes + 16));
    if (int rc = cm2_glitch_create(&h->scale, h->launch.nt, sizes, h->launch.nblocks, 1, stream)) return rc;
    int64_t ginfo[6];
    if (int rc = cm2_glitch_info(h->scale, ginfo)) return rc;
    h->bytes = h->tables.bytes() + (int64_t)(nt + h->temp_bytes + 16) + ginfo[5];
    return 0;
}

}  // namespace

extern "C" int cm2_jump_create(cm2_jump **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int half_window,
                               void *stream)
{
    const char *who = "cm2_jump_create";
    CM2_CHECK(out, "%s: null output handle", who);
    jp::Launch l;
    const jp::Status ps = jp::check_create(&l, nt, h_sizes, nblocks, half_window);
    if (int rc = check_create_status(who, ps, nt, nblocks, "half_window", half_window, jp::kMaxWindow,
                                     "the scale's histograms")) return rc;
    cm2_jump *h = new cm2_jump();
    h->launch = l;
    const int rc = jump_fill(h, h_sizes, stream);
    if (rc) {
        cm2_jump_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_jump_info(const cm2_jump *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_jump_info: null argument");
    h_info[0] = h->launch.nt;
    h_info[1] = h->launch.nblocks;
    h_info[2] = h->launch.w;
    h_info[3] = jp::kTile;
    h_info[4] = h->launch.lds_bytes;
    h_info[5] = h->bytes;
    return 0;
}

extern "C" int cm2_jump_stat(cm2_jump *h, const double *d_in, const void *d_flags, int flag_kind,
                             const uint8_t *d_prev, int min_count, double *d_t, uint8_t *d_noeval, void *stream)
{
    const char *who = "cm2_jump_stat";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_in && d_t && d_noeval, "%s: null input or output", who);
    if (int rc = check_flag_kind_status(who, d_flags != nullptr, flag_kind)) return rc;
    CM2_CHECK(jp::check_stat(h->launch.w, d_flags != nullptr, flag_kind, min_count) == jp::kOk,
              "%s: min_count=%d outside [1, half_window=%d]", who, min_count, h->launch.w);
    const uint64_t nt = (uint64_t)h->launch.nt;
    const Range in = {d_in, 8 * nt}, flags = {d_flags, flag_kind == 0 ? 4 * nt : nt}, prev = {d_prev, nt},
                noeval = {d_noeval, nt};
    if (int rc = check_disjoint(who, {{d_t, 8 * nt}}, {in, flags, prev, noeval},
                                "%s: t must not overlap an input or noeval")) return rc;
    if (int rc = check_disjoint(who, {noeval}, {in, flags, prev}, "%s: noeval must not overlap an input")) return rc;
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(k_jump_stat), (size_t)h->launch.lds_bytes, granted));
    k_jump_stat<<<dim3((unsigned)h->launch.tiles), jp::kTileThreads, (size_t)h->launch.lds_bytes, as_stream(stream)>>>(
        h->tiles(), h->launch.w, min_count, Stream{d_in, d_flags, flag_kind, d_prev}, d_t, d_noeval);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_jump_scale(cm2_jump *h, const double *d_t, const uint8_t *d_noeval, double *d_sigma, void *stream)
{
    const char *who = "cm2_jump_scale";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_t && d_noeval && d_sigma, "%s: null input or output", who);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks;
    CM2_CHECK(!bytes_overlap(d_sigma, 8 * nb, d_t, 8 * nt) && !bytes_overlap(d_sigma, 8 * nb, d_noeval, nt),
              "%s: sigma must not overlap t or noeval", who);
    // definition 4 of f2e with d = r = t, the noeval bytes as flags and W = 3
    return cm2_glitch_scale(h->scale, d_t, d_t, d_noeval, 1, nullptr, d_sigma, stream);
}

extern "C" int cm2_jump_find(cm2_jump *h, const double *d_t, const uint8_t *d_noeval, const double *d_sigma,
                             double nsigma, int64_t capacity, int64_t *d_pos, double *d_heights, double *d_offsets,
                             int64_t *d_njumps, void *stream)
{
    const char *who = "cm2_jump_find";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_t && d_noeval && d_sigma && d_pos && d_heights && d_offsets && d_njumps, "%s: null input or output",
              who);
    const jp::Status ps = jp::check_find(nsigma, capacity);
    CM2_CHECK(ps != jp::kBadNsigma, "%s: nsigma=%g must be finite and > 0", who, nsigma);
    CM2_CHECK(ps == jp::kOk, "%s: capacity=%lld < 1", who, (long long)capacity);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks;
    const uint64_t cap = 8 * (uint64_t)(capacity < h->launch.nt ? capacity : h->launch.nt);   // bytes a table can take
    if (int rc = check_disjoint(who, {{d_pos, cap}, {d_heights, cap}, {d_offsets, cap}, {d_njumps, 8 * (nb + 1)}},
                                {{d_t, 8 * nt}, {d_noeval, nt}, {d_sigma, 8 * nb}}, "%s: an output overlaps an input",
                                "%s: two outputs overlap")) return rc;
    hipStream_t st = as_stream(stream);
    CM2_HIP(hipMemsetAsync(d_njumps, 0, (size_t)(8 * (nb + 1)), st));
    k_jump_peaks<<<dim3((unsigned)h->launch.tiles), jp::kTileThreads, 0, st>>>(
        h->tiles(), h->launch.w, d_t, d_noeval, d_sigma, nsigma, h->d_mark,
        reinterpret_cast<unsigned long long *>(d_njumps));
    CM2_LAUNCH_OK();
    size_t temp_bytes = h->temp_bytes;
    CM2_HIP(select_marked(h->d_temp, &temp_bytes, h->d_mark, h->launch.nt, d_pos, capacity, d_njumps + nb, st));
    k_jump_offsets<<<dim3((unsigned)((nb + kBlock - 1) / kBlock)), kBlock, 0, st>>>(
        h->tables.d_off, h->launch.nblocks, d_pos, d_njumps + nb, capacity, d_t, d_heights, d_offsets);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_jump_correct(cm2_jump *h, const double *d_in, const uint8_t *d_prev, const int64_t *d_pos,
                                const double *d_offsets, const int64_t *d_njumps, int64_t capacity, int radius,
                                double *d_out, uint8_t *d_class, int64_t *d_counts, void *stream)
{
    const char *who = "cm2_jump_correct";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_in && d_pos && d_offsets && d_njumps && d_out && d_class && d_counts, "%s: null input or output", who);
    const jp::Status ps = jp::check_correct(radius, capacity);
    CM2_CHECK(ps != jp::kBadRadius, "%s: radius=%d outside [0, %d]", who, radius, jp::kMaxRadius);
    CM2_CHECK(ps == jp::kOk, "%s: capacity=%lld < 1", who, (long long)capacity);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks;
    const uint64_t cap = 8 * (uint64_t)(capacity < h->launch.nt ? capacity : h->launch.nt);
    // d_out may be d_in itself: a sample is read and written by one thread
    const Range table = {d_pos, cap}, offsets = {d_offsets, cap}, njumps = {d_njumps, 8 * (nb + 1)};
    if (int rc = check_disjoint(who, {{d_out, 8 * nt}, {d_class, nt}, {d_counts, 8 * jp::kCounts * nb}},
                                {{d_in, 8 * nt}, {d_prev, nt}, table, offsets, njumps},
                                "%s: an output overlaps an input (only d_out may be d_in itself)",
                                "%s: two outputs overlap", 0, 0)) return rc;
    hipStream_t st = as_stream(stream);
    CM2_HIP(hipMemsetAsync(d_counts, 0, (size_t)(8 * jp::kCounts * nb), st));
    k_jump_correct<<<dim3((unsigned)h->launch.tiles), jp::kTileThreads, 0, st>>>(
        h->tiles(), d_in, d_prev, d_pos, d_offsets, d_njumps + nb, capacity, radius, d_out, d_class,
        reinterpret_cast<unsigned long long *>(d_counts));
    CM2_LAUNCH_OK();
    return 0;
}
