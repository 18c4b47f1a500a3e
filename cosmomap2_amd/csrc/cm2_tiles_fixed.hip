// cm2_tiles_fixed.hip -- P^T on the tile-bucketed order with every pixel's terms added IN TIME
// ORDER starting from 0, exactly like the reference's serial scatter loop
// (interfaces/linearoperators.py:394-400, :452-458, :509-516): no atomics, bitwise reproducible
// from run to run, and bit-identical to the serial loop when the plan keeps cos and sin
// (CM2_TILE_ANGLES=full; the default half-angle storage rebuilds them to 3.4e-16).
//
// ONE workgroup owns a tile from its first sample to its last: the tile's accumulators stay in
// LDS for the whole bucket and are written out once with plain stores.  The bucket is walked
// slice by slice (S consecutive TB samples = S consecutive-in-time samples of this tile).  At
// plan time the samples of a slice are sorted by (pixel, time) and packed into GROUPS of four
// list entries such that a group holds whole runs (run = the slice's samples of one pixel):
//
//   entry  = pl word (pixel in tile, sign of cos) | offset in the slice << 16 | level << 28
//   group  = 4 entries + their 4 half angles (or cos, sin), padded with null entries
//   thread t of the workgroup owns group t of the slice: it reads its 16 + 32 bytes with
//   three 16-byte loads straight into registers -- two slices ahead of the one it reduces --,
//   picks the 4 TOD values out of the slice staged in LDS, and adds its entries to the pixels' LDS
//   accumulators one after the other (ds_add_f64: adds of one thread to one address happen in
//   program order).  A pixel is touched by one thread per pass and the slices follow each other
//   in time, so each sum is the reference's, term by term.
//
// Runs of 5..60 samples are cut into pieces of 4 in consecutive groups of ONE wave (the packer pads
// so that a run never straddles a multiple of 64 groups), piece p carrying level p: every wave
// makes one pass per level (the slice's highest level is known at plan time); the LDS executes a
// wave's instructions in issue order, so the pieces are added in order without a barrier between
// the passes (round 2 had one per level: dense tiles, 5-6 hits per pixel and slice, paid 2-3 of
// them per slice).  Longer runs (a pixel hit
// > 60 times inside one slice: hot pixels) are kept out of the groups and walked by one thread
// each from a separate list.
//
// HBM per sample: 8 B TOD + ~1.14 x 12 B of list (padding of the groups) = ~21.7 B, every load
// 16 B per lane and coalesced.  What the kernel had to get right to stream at HBM speed
// (measured, 1e8 samples, nside 256: 0.37 ms with the reduction switched off, 0.45 ms with it):
//   * no register spill in the slice loop: a scratch reload is a VMEM operation, and waiting for
//     it (vmcnt counts in order) drains every prefetched load issued before it;
//   * unconditional loads (clamped indices) and a scheduling barrier per slice, so that the
//     compiler waits with s_waitcnt vmcnt(N > 0) for the oldest slice only;
//   * LDS adds instead of a load / add / store chain per run (12 of 24 LDS operations less per
//     thread and slice, and no dependent round trip).
#include "cm2_fx_lists.h"

#include <algorithm>
#include <cstring>
#include <mutex>

using namespace cm2;

namespace {

// (kFxT threads, the entry word, meta and the null entry: cm2_fx_lists.h, shared with the list builders.  The fields
// are taken apart with its shifts and masks in place: as accessor functions they cost every instance of
// k_Pt_tiles_fixed two more v_cndmask.)
constexpr int kFxDepth = 2;             // slices fetched ahead of the one being reduced
// Hot pixels.  A run longer than `chunk_min` entries inside one slice (a pixel that takes a large
// share of a tile's samples: a stare at a source, a tile that is one pixel) is not walked term by
// term by one thread -- 1536 dependent additions per slice while 511 threads wait -- but cut into
// chunks of kFxChunk consecutive entries: one thread per chunk sums its terms in time order in
// registers, the chunk sums of a run are added in time order by one thread, and the result joins
// the pixel's accumulator.  The chunk boundaries and both orders are fixed by the plan, so the
// result is reproducible bit for bit and independent of the hit map; it differs from the serial
// sum by the rounding of a regrouped sum (~1e-16 relative per level).  cm2_tiles_set_pt_order(t, 2)
// / CM2_PT_ORDER=exact keep the pure time order for every run.
constexpr int kFxChunk = 32;
constexpr int kFxChunkMinDefault = 256;
constexpr int kFxMaxChunks = policy::kFxChunkSums;    // (128) per slice: S / kFxChunk + long runs <= 64 + 8

// ------------------------------------------------------------------- fused form -----
// The ranges of the hot tiles (a one-pixel tile of very many samples is reduced by ranges of kHotChunk samples)
// used to be two more launches behind the main one (k_Pt_hot: 306 workgroups for a 5e6-sample pixel, 22 us;
// k_hot_combine, 7 us).  They are work items at the END of the main launch's grid now, and the last range of a
// tile to finish adds the tile's range sums.  Who is last depends on the dispatch; WHAT is added and in which
// order does not (range after range, as k_hot_combine did): the same bits, whoever does it.  Measured at C4
// with 5 % of the samples on one pixel (profiles/r05_pt_fused.md): P^T 0.402-0.411 against 0.440-0.449 ms.
// The copies of SPLIT tiles stay with k_parts_combine: adding them in the main launch as well (the tile's last
// part to finish reads the other parts' copies) was built and measured -- P^T of the uneven hit map 0.438-0.446
// against 0.423-0.428 ms: one workgroup reading k copies at the tail of the launch loses to a short, wide
// kernel -- and removed.
// Hand-off between workgroups inside a launch (cdna_hip_programming.md, Guideline 16, counter form with
// write-through payload): the producer stores its three sums sc1 (no release fence: a release writes back the
// XCD's whole L2), drains them, ONE lane does a relaxed agent-scope fetch_add on the tile's counter; the
// workgroup that draws the last ticket: agent-scope acquire fence by one lane, drain, barrier, then plain loads
// of the others' sums.  The counters are zeroed by a memset in front of every launch (fx_launch_inst).
struct FxFused {
    unsigned int *count;            // [nhot] arrival counters
    const int64_t *hot_range;       // [ranges][2] first / one-past-last TB position
    const int *hot_range_tile;      // [ranges] index in hot_tiles
    const int64_t *hot_tiles;       // [nhot][3] first pixel, first range, ranges
    double *hot_partial;            // [ranges][3]
    const uint16_t *pl;             // TB-order streams of the plan (hot ranges read them directly)
    const double *a_tb, *b_tb;
};

constexpr int kHotChunk = 16384, kHotT = 1024;          // samples per range, (virtual) threads per range
// (1024 threads: 306 workgroups of 256 left the chip with one wave per SIMD, 45 us for 5e6 samples)

// a handed-off double: WRITE-THROUGH (sc1) store, so that the producer needs no release fence
__device__ __forceinline__ void fx_publish(double *p, double x)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), __builtin_bit_cast(unsigned long long, x),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool fx_last_arriver(unsigned int *counter, unsigned int expected, int *lds_flag, int tid)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every storing wave drains its (sc1) stores
    __syncthreads();
    if (tid == 0) {
        const unsigned int old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (old + 1u == expected) ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *lds_flag = last;
    }
    __syncthreads();
    return *lds_flag != 0;
}

// One range of a hot tile (kHotChunk consecutive samples of ONE pixel) by one workgroup of kFxT = 512
// threads doing the work of k_Pt_hot's 1024: thread t is the virtual threads t and t + 512, each adding the
// terms at positions vt, vt + 1024, ... of the range in that order; the 1024 sums are combined by the same
// halving tree.  Then the last range of the tile adds the tile's range sums in time order (k_hot_combine).
// (The term, the tree and the tail are written out here and in k_Pt_hot / k_hot_combine: each was tried as a shared
// __forceinline__ helper and changed the instruction stream of some instance, profiles/fx_split_ab.md.)
template <int POL, bool HALF>
__device__ __forceinline__ void fx_hot_item(const FxFused &z, int64_t c, const double *__restrict__ v_tb,
                                            double *__restrict__ out, double *sm, int tid)
{
    double *red = sm;                                        // [3][kHotT]
    const int64_t k0 = z.hot_range[2 * c], k1 = z.hot_range[2 * c + 1];
    double sv[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
    constexpr int U = 4;
    for (int64_t kk = k0 + tid; kk < k1; kk += (int64_t)U * kHotT) {
        double v[2][U], a[2][U], b2[2][U];
        uint16_t w[2][U];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = kk + (int64_t)hh * kFxT + (int64_t)u * kHotT;
                const int64_t kc = k < k1 ? k : k1 - 1;
                v[hh][u] = v_tb[kc];
                a[hh][u] = POL > 1 ? z.a_tb[kc] : 0.0;
                b2[hh][u] = (POL > 1 && !HALF) ? z.b_tb[kc] : 0.0;
                w[hh][u] = (POL > 1 && HALF) ? z.pl[kc] : (uint16_t)0;
            }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kk + (int64_t)hh * kFxT + (int64_t)u * kHotT >= k1) continue;
                sv[hh] += v[hh][u];
                if (POL > 1) {
                    double cc, ss;
                    if (HALF) {
                        const double h = a[hh][u], h2 = h * h, inv = 1.0 / (1.0 + h2);
                        cc = (1.0 - h2) * inv;
                        ss = (h + h) * inv;
                        if (w[hh][u] & 0x8000u) cc = -cc;
                    } else {
                        cc = a[hh][u];
                        ss = b2[hh][u];
                    }
                    s1[hh] += v[hh][u] * cc;
                    s2[hh] += v[hh][u] * ss;
                }
            }
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        red[tid + hh * kFxT] = sv[hh];
        red[kHotT + tid + hh * kFxT] = s1[hh];
        red[2 * kHotT + tid + hh * kFxT] = s2[hh];
    }
    __syncthreads();
    for (int h = kHotT / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            red[tid] += red[tid + h];
            red[kHotT + tid] += red[kHotT + tid + h];
            red[2 * kHotT + tid] += red[2 * kHotT + tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        fx_publish(z.hot_partial + 3 * c, red[0]);
        fx_publish(z.hot_partial + 3 * c + 1, red[kHotT]);
        fx_publish(z.hot_partial + 3 * c + 2, red[2 * kHotT]);
    }
    const int h = z.hot_range_tile[c];
    const int64_t p0 = z.hot_tiles[3 * h], c0 = z.hot_tiles[3 * h + 1], nc = z.hot_tiles[3 * h + 2];
    int *flag = reinterpret_cast<int *>(red + 3 * kHotT);
    if (!fx_last_arriver(z.count + h, (unsigned int)nc, flag, tid)) return;
    // the tile's range sums in time order (k_hot_combine): staged 256 ranges at a time, one thread adds
    double *st = red;
    double tv = 0.0, t1 = 0.0, t2 = 0.0;
    for (int64_t base = 0; base < nc; base += 256) {
        const int64_t n = nc - base < 256 ? nc - base : 256;
        for (int64_t i = tid; i < 3 * n; i += kFxT) st[i] = z.hot_partial[3 * (c0 + base) + i];
        __syncthreads();
        if (tid == 0)
            for (int64_t q = 0; q < n; ++q) {
                tv += st[3 * q];
                t1 += st[3 * q + 1];
                t2 += st[3 * q + 2];
            }
        __syncthreads();
    }
    if (tid != 0) return;
    if (POL == 1) {
        out[p0] = tv;
    } else if (POL == 2) {
        out[2 * p0] = t1;
        out[2 * p0 + 1] = t2;
    } else {
        out[3 * p0] = tv;
        out[3 * p0 + 1] = t1;
        out[3 * p0 + 2] = t2;
    }
}

// ------------------------------------------------------------------- kernel --------
template <int POL, bool HALF, int VPT>
__global__ __launch_bounds__(kFxT, 4) void k_Pt_tiles_fixed(
    int tp, const int64_t *__restrict__ tile_p0, int tile0, const uint2 *__restrict__ sk,
    const int64_t *__restrict__ slice0, const uint2 *__restrict__ meta,
    const uint4 *__restrict__ gent, const double2 *__restrict__ ga,
    const double2 *__restrict__ gb, const uint2 *__restrict__ trun,
    const uint32_t *__restrict__ tent, const double *__restrict__ ta,
    const double *__restrict__ tb, const double *__restrict__ v_tb, double *__restrict__ out,
    uint32_t chunk_min, const uint8_t *__restrict__ hot, const int4 *__restrict__ parts,
    int part0, double *__restrict__ scratch, const FxFused *__restrict__ fz, int nmain, int64_t hot_c0)
{
    constexpr int D = kFxDepth;
    constexpr bool ANG = POL > 1, TWO = POL > 1 && !HALF;
    constexpr uint32_t QM = fx_pixel_mask(HALF);
    extern __shared__ double sm[];
    double *tile = sm;                                   // tp * POL accumulators
    // the slice's TOD values, TB order, in one of TWO buffers (slice j in buffer j & 1): a wave that
    // is ahead stages the next slice while another still gathers from this one, so a slice costs ONE
    // workgroup barrier (behind the staging; it also completes every wave's LDS adds of the slice
    // before, which keeps the slices' adds to one pixel in time order)
    double *vbuf0 = sm + (int64_t)tp * POL;              // VPT * kFxT values
    double *vbuf1 = vbuf0 + VPT * kFxT;
    double *part = vbuf1 + VPT * kFxT;                   // 3 x kFxMaxChunks chunk sums of hot runs
    const int tid = threadIdx.x;
    if (fz && (int)blockIdx.x >= nmain) {                // fused form: the ranges of the hot tiles come last
        fx_hot_item<POL, HALF>(*fz, hot_c0 + ((int)blockIdx.x - nmain), v_tb, out, sm, tid);
        return;
    }
    // the workgroup's work: a whole tile, or (plans with parts) some consecutive slices of one, summed
    // into a scratch copy of the tile that k_parts_combine adds to the other parts' copies
    int b = tile0 + (int)blockIdx.x, nsl = 0;
    int64_t s0 = 0;
    double *o_part = nullptr;
    if (parts) {
        const int4 pd = parts[part0 + (int)blockIdx.x];
        b = pd.x;
        nsl = pd.y;
        s0 = pd.z;
        if (pd.w >= 0) o_part = scratch + (int64_t)pd.w * ((int64_t)tp * POL);
    }
    if (hot && hot[b]) return;                           // reduced by k_Pt_hot (many workgroups)
    const int64_t p0 = tile_p0[b];
    const int64_t np = tile_p0[b + 1] - p0;
    const int nvals = (int)(np * POL);
    for (int i = tid; i < nvals; i += kFxT) tile[i] = 0.0;
    if (!parts) {
        s0 = slice0[b];
        nsl = (int)(slice0[b + 1] - s0);
    }

    // register ring: slice j lives in slot j % D from the moment slice j - D has been staged.
    // All loads are unconditional (indices clamped) and kept together per slice, so that the
    // compiler counts outstanding loads (s_waitcnt vmcnt(N)) instead of draining them.
    double pv[D][VPT];
    uint4 pe[D];
    double2 pa[D][2], pb[D][2];
    uint2 pm[D][2];                                      // meta of slice j and j + 1
    // {first group, first tail run} of the NEXT slice to fetch and of its successor: loaded one
    // fetch ahead, so that the group addresses never wait for them
    // ... and {first TB address, samples} of it
    uint2 nx0 = meta[s0], nx1 = meta[s0 + (nsl > 0 ? 1 : 0)], nk = sk[s0];
    auto fetch = [&](int slot, int j) {
        const int64_t kb = (int64_t)nk.x;
        const int len = (int)nk.y;
        const uint2 m0 = nx0, m1 = nx1;
        pm[slot][0] = m0;
        pm[slot][1] = m1;
        {
            const int jn = j + 1 < nsl ? j + 1 : nsl - 1;
            nx0 = meta[s0 + jn];
            nx1 = meta[s0 + jn + 1];
            nk = sk[s0 + jn];
        }
        const uint32_t G = m1.x - m0.x;
        const int64_t g = (int64_t)m0.x + ((uint32_t)tid < G ? tid : 0);
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            const int i = tid + u * kFxT;
            pv[slot][u] = v_tb[kb + (i < len ? i : len - 1)];
        }
        pe[slot] = gent[g];
        if (ANG) {
            pa[slot][0] = ga[2 * g];
            pa[slot][1] = ga[2 * g + 1];
        }
        if (TWO) {
            pb[slot][0] = gb[2 * g];
            pb[slot][1] = gb[2 * g + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    // terms of one list entry: (v, v cos, v sin)
    auto terms = [&](uint32_t w, double a, double bsin, double v, double &t1, double &t2) {
        if (POL == 1) return;
        double cc, ss;
        if (HALF) {
            const double h2 = a * a, inv = 1.0 / (1.0 + h2);
            cc = (1.0 - h2) * inv;
            ss = (a + a) * inv;
            if (w & 0x8000u) cc = -cc;
        } else {
            cc = a;
            ss = bsin;
        }
        t1 = v * cc;
        t2 = v * ss;
    };
    // tile[pixel] += term with the LDS adder (ds_add_f64, nothing returned): the same IEEE addition
    // the serial loop performs on its accumulator, and the adds one thread issues to one address
    // are performed in program order -- so a run is summed term after term without a register
    // round trip.  Within a pass no two threads touch the same pixel.
    auto tile_add = [&](int q, double v, double t1, double t2) {
        if (POL == 1) {
            atomicAdd(&tile[q], v);
        } else if (POL == 2) {
            atomicAdd(&tile[2 * q], t1);
            atomicAdd(&tile[2 * q + 1], t2);
        } else {
            atomicAdd(&tile[3 * q], v);
            atomicAdd(&tile[3 * q + 1], t1);
            atomicAdd(&tile[3 * q + 2], t2);
        }
    };
    // one group: its entries added to the tile accumulators in list (= time) order
    auto reduce_group = [&](const uint32_t (&w)[4], const double (&v)[4], const double (&t1)[4],
                            const double (&t2)[4]) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (w[m] != kFxNull) tile_add((int)(w[m] & QM), v[m], t1[m], t2[m]);
    };

    if (nsl > 0) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd) fetch(dd, dd);
    }
    for (int jj = 0; jj < nsl; jj += D) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
            const int j = jj + dd;
            if (j >= nsl) break;
            double *vbuf = dd ? vbuf1 : vbuf0;               // (kFxDepth = 2: slot dd = j & 1)
            // ---- stage the slice's TOD values (into the buffer slice j - 2 used: every wave left
            //      that slice before it arrived at slice j - 1's barrier; j = 0: the barrier below
            //      also covers the zeroing of the tile) ----
#pragma unroll
            for (int u = 0; u < VPT; ++u) vbuf[tid + u * kFxT] = pv[dd][u];
            const uint2 m0 = pm[dd][0], m1 = pm[dd][1];
            uint32_t w[4] = {pe[dd].x, pe[dd].y, pe[dd].z, pe[dd].w};
            double a[4] = {0.0, 0.0, 0.0, 0.0}, bs[4] = {0.0, 0.0, 0.0, 0.0};
            if (ANG) {
                a[0] = pa[dd][0].x; a[1] = pa[dd][0].y; a[2] = pa[dd][1].x; a[3] = pa[dd][1].y;
            }
            if (TWO) {
                bs[0] = pb[dd][0].x; bs[1] = pb[dd][0].y; bs[2] = pb[dd][1].x; bs[3] = pb[dd][1].y;
            }
            __syncthreads();
            fetch(dd, j + D);
            const uint32_t G = m1.x - m0.x, ntail = (m1.y & kFxRunMask) - (m0.y & kFxRunMask);
            const int maxlevel = (int)(m0.y >> kFxLevelShift);     // highest level in this slice (plan time)
            for (uint32_t g0 = 0; g0 < G || g0 == 0; g0 += kFxT) {
                const bool mine = g0 + tid < G;
                if (g0 > 0) {                             // more groups than threads: direct loads
                    const int64_t g = (int64_t)m0.x + (mine ? g0 + tid : 0);
                    const uint4 e = gent[g];
                    w[0] = e.x; w[1] = e.y; w[2] = e.z; w[3] = e.w;
                    if (ANG) {
                        const double2 x0 = ga[2 * g], x1 = ga[2 * g + 1];
                        a[0] = x0.x; a[1] = x0.y; a[2] = x1.x; a[3] = x1.y;
                    }
                    if (TWO) {
                        const double2 x0 = gb[2 * g], x1 = gb[2 * g + 1];
                        bs[0] = x0.x; bs[1] = x0.y; bs[2] = x1.x; bs[3] = x1.y;
                    }
                }
                if (!mine) w[0] = w[1] = w[2] = w[3] = kFxNull;
                double v[4], t1[4], t2[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t off = (w[m] >> kFxOffsetShift) & kFxOffsetMask;
                    v[m] = vbuf[w[m] != kFxNull ? off : 0];
                    t1[m] = t2[m] = 0.0;
                    terms(w[m], a[m], bs[m], v[m], t1[m], t2[m]);
                }
                const int level = mine ? (int)((w[0] >> kFxLevelShift) & kFxLevelMask) : 0;
                if (g0 == 0 && ntail > 0) {
                    const int64_t tr0 = (int64_t)(m0.y & kFxRunMask);
                    // runs too long for the groups: one thread walks a whole run ...
                    for (uint32_t r = tid; r < ntail; r += kFxT) {
                        const uint2 r0 = trun[tr0 + r], r1 = trun[tr0 + r + 1];
                        if (r1.x - r0.x > chunk_min) continue;
                        const int q = (int)r0.y;
                        for (uint32_t e = r0.x; e < r1.x; ++e) {
                            const uint32_t we = tent[e];
                            const double ve = vbuf[(we >> kFxOffsetShift) & kFxOffsetMask];
                            double u1 = 0.0, u2 = 0.0;
                            terms(we, ANG ? ta[e] : 0.0, TWO ? tb[e] : 0.0, ve, u1, u2);
                            tile_add(q, ve, u1, u2);
                        }
                    }
                    // ... unless it is a hot run: chunk sums by one thread per chunk (the walk over
                    // the runs is the same for every thread: trun is read uniformly), then the
                    // chunk sums of a run added in time order by the thread of its first chunk
                    int cbase = 0, my_first = -1, my_n = 0, my_q = 0;
                    for (uint32_t r = 0; r < ntail; ++r) {
                        const uint2 r0 = trun[tr0 + r], r1 = trun[tr0 + r + 1];
                        const uint32_t len = r1.x - r0.x;
                        if (len <= chunk_min) continue;
                        const int nch = (int)((len + kFxChunk - 1) / kFxChunk);
                        const int c = tid - cbase;
                        if (c >= 0 && c < nch && tid < kFxMaxChunks) {
                            const uint32_t e0 = r0.x + (uint32_t)c * kFxChunk;
                            const uint32_t e1 = e0 + kFxChunk < r1.x ? e0 + kFxChunk : r1.x;
                            double sv = 0.0, s1 = 0.0, s2 = 0.0;
                            for (uint32_t e = e0; e < e1; ++e) {
                                const uint32_t we = tent[e];
                                const double ve = vbuf[(we >> kFxOffsetShift) & kFxOffsetMask];
                                double u1 = 0.0, u2 = 0.0;
                                terms(we, ANG ? ta[e] : 0.0, TWO ? tb[e] : 0.0, ve, u1, u2);
                                sv += ve;
                                s1 += u1;
                                s2 += u2;
                            }
                            part[tid] = sv;
                            part[kFxMaxChunks + tid] = s1;
                            part[2 * kFxMaxChunks + tid] = s2;
                            if (c == 0) {
                                my_first = tid;
                                my_n = nch;
                                my_q = (int)r0.y;
                            }
                        }
                        cbase += nch;
                    }
                    if (cbase > 0) {                      // (uniform: some run of this slice is hot)
                        __syncthreads();
                        if (my_first >= 0) {
                            double sv = part[my_first], s1 = part[kFxMaxChunks + my_first],
                                   s2 = part[2 * kFxMaxChunks + my_first];
                            for (int k = 1; k < my_n; ++k) {
                                sv += part[my_first + k];
                                s1 += part[kFxMaxChunks + my_first + k];
                                s2 += part[2 * kFxMaxChunks + my_first + k];
                            }
                            tile_add(my_q, sv, s1, s2);
                        }
                    }
                }
                // one pass per level: piece p of a long run is added after piece p - 1.  The pieces
                // of a run are groups of one wave (k_fx_pack), and the LDS executes a wave's
                // instructions in issue order, so the passes need no barrier between them; the
                // next slice's staging barrier separates this slice's adds from the next slice's.
                for (int p = 0; p <= maxlevel; ++p)
                    if (mine && level == p) reduce_group(w, v, t1, t2);
                if (g0 + kFxT < G) __syncthreads();          // (a further round of groups of this slice)
            }
        }
    }
    __syncthreads();
    double *o = o_part ? o_part : out + p0 * POL;
    for (int i = tid; i < nvals; i += kFxT) o[i] = tile[i];
}

// the copies of a split tile added in time order (part after part), written to the map
__global__ __launch_bounds__(256) void k_parts_combine(const int64_t *__restrict__ multi, int64_t m0,
                                                        int64_t stride, const double *__restrict__ scratch,
                                                        double *__restrict__ out)
{
    const int64_t *m = multi + 4 * (m0 + blockIdx.x);
    const int64_t o = m[0], nvals = m[1], slot = m[2], k = m[3];
    const int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x;       // one value per thread: the launch is short
    if (i >= nvals) return;
    double acc = scratch[slot * stride + i];
    for (int64_t j = 1; j < k; ++j) acc += scratch[(slot + j) * stride + i];
    out[o + i] = acc;
}

// ------------------------------------------------------------------- hot tiles ------
// A tile that is one pixel with very many samples: its bucket is cut into ranges of kHotChunk
// consecutive samples; one workgroup per range, thread t adding the terms at positions t, t + 1024,
// ... of the range in that order, the 1024 thread sums combined by a fixed halving tree; k_hot_combine
// then adds the range sums of a tile in time order and writes the pixel.  Every boundary and every
// order depends on the bucket's length only: reproducible bit for bit, independent of the rest of
// the hit map; a regrouping of the serial sum, ~1e-16 relative per level away from it.
constexpr int64_t kHotMin = policy::kHotTileMin;                // samples that make a one-pixel tile hot
static_assert(kHotMin == 2 * kHotChunk, "hot tiles: at least two ranges");

template <int POL, bool HALF>
__global__ __launch_bounds__(kHotT) void k_Pt_hot(const int64_t *__restrict__ range, int64_t c0,
                                                   const uint16_t *__restrict__ pl,
                                                   const double *__restrict__ a_tb,
                                                   const double *__restrict__ b_tb,
                                                   const double *__restrict__ v_tb,
                                                   double *__restrict__ partial)
{
    __shared__ double red[3][kHotT];
    const int64_t c = c0 + blockIdx.x;
    const int64_t k0 = range[2 * c], k1 = range[2 * c + 1];
    const int t = threadIdx.x;
    double sv = 0.0, s1 = 0.0, s2 = 0.0;
    // (four positions' loads in flight at a time; the terms are added in the order of the positions)
    constexpr int U = 4;
    for (int64_t kk = k0 + t; kk < k1; kk += (int64_t)U * kHotT) {
        double v[U], a[U], b2[U];
        uint16_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = kk + (int64_t)u * kHotT;
            const int64_t kc = k < k1 ? k : k1 - 1;
            v[u] = v_tb[kc];
            a[u] = POL > 1 ? a_tb[kc] : 0.0;
            b2[u] = (POL > 1 && !HALF) ? b_tb[kc] : 0.0;
            w[u] = (POL > 1 && HALF) ? pl[kc] : (uint16_t)0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kk + (int64_t)u * kHotT >= k1) break;
            sv += v[u];
            if (POL > 1) {
                double cc, ss;
                if (HALF) {
                    const double h = a[u], h2 = h * h, inv = 1.0 / (1.0 + h2);
                    cc = (1.0 - h2) * inv;
                    ss = (h + h) * inv;
                    if (w[u] & 0x8000u) cc = -cc;
                } else {
                    cc = a[u];
                    ss = b2[u];
                }
                s1 += v[u] * cc;
                s2 += v[u] * ss;
            }
        }
    }
    red[0][t] = sv;
    red[1][t] = s1;
    red[2][t] = s2;
    __syncthreads();
    for (int h = kHotT / 2; h >= 1; h >>= 1) {
        if (t < h) {
            red[0][t] += red[0][t + h];
            red[1][t] += red[1][t + h];
            red[2][t] += red[2][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[3 * c] = red[0][0];
        partial[3 * c + 1] = red[1][0];
        partial[3 * c + 2] = red[2][0];
    }
}

// One workgroup per hot tile: the range sums are staged in LDS 256 ranges at a time (coalesced loads: one
// thread walking them in HBM paid a memory round trip every few terms -- 305 ranges for 5e6 samples), and
// thread 0 adds them in time order.
template <int POL>
__global__ __launch_bounds__(256) void k_hot_combine(const int64_t *__restrict__ tiles, int64_t h0,
                                                      const double *__restrict__ partial,
                                                      double *__restrict__ out)
{
    __shared__ double st[3 * 256];
    const int64_t h = h0 + blockIdx.x;
    const int64_t p0 = tiles[3 * h], c0 = tiles[3 * h + 1], nc = tiles[3 * h + 2];
    double sv = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t base = 0; base < nc; base += 256) {
        const int64_t n = nc - base < 256 ? nc - base : 256;
        for (int64_t i = threadIdx.x; i < 3 * n; i += 256) st[i] = partial[3 * (c0 + base) + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int64_t c = 0; c < n; ++c) {               // range sums in time order
                sv += st[3 * c];
                s1 += st[3 * c + 1];
                s2 += st[3 * c + 2];
            }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (POL == 1) {
        out[p0] = sv;
    } else if (POL == 2) {
        out[2 * p0] = s1;
        out[2 * p0 + 1] = s2;
    } else {
        out[3 * p0] = sv;
        out[3 * p0 + 1] = s1;
        out[3 * p0 + 2] = s2;
    }
}

// one-pixel tiles with at least kHotMin samples, their sample ranges and the scratch of range sums
int hot_plan(cm2_tiles *t, hipStream_t st)
{
    FxHot &hot = t->hot;
    hot.reset();
    const policy::HotRanges h = policy::hot_ranges(t->tile_p0, t->tile_off, kHotChunk);
    const std::vector<int64_t> &range = h.range, &tiles = h.tiles;
    hot.tile = h.hot_tile;
    hot.chunk0 = h.hot_chunk0;
    if (hot.tile.empty()) return 0;
    CM2_HIP(cm2::dev_malloc(&hot.d_flag, h.flag.size()));
    CM2_HIP(cm2::dev_malloc(&hot.d_range, sizeof(int64_t) * range.size()));
    CM2_HIP(cm2::dev_malloc(&hot.d_tiles, sizeof(int64_t) * tiles.size()));
    CM2_HIP(cm2::dev_malloc(&hot.d_partial, sizeof(double) * 3 * (range.size() / 2)));
    CM2_HIP(cm2::upload(hot.d_flag, h.flag.data(), h.flag.size(), st));
    CM2_HIP(cm2::upload(hot.d_range, range.data(), sizeof(int64_t) * range.size(), st));
    CM2_HIP(cm2::upload(hot.d_tiles, tiles.data(), sizeof(int64_t) * tiles.size(), st));
    CM2_HIP(cm2::dev_malloc(&hot.d_range_tile, sizeof(int) * h.range_tile.size()));
    CM2_HIP(cm2::upload(hot.d_range_tile, h.range_tile.data(), sizeof(int) * h.range_tile.size(), st));
    CM2_HIP(hipStreamSynchronize(st));
    return 0;
}

template <int POL, bool HALF>
int hot_launch(const cm2_tiles *t, const double *d_tod_tb, double *d_out, int64_t tile_lo,
               int64_t tile_hi, hipStream_t stream)
{
    const FxHot &hot = t->hot;
    const policy::IndexRange h = policy::tiles_in_range(hot.tile, tile_lo, tile_hi);
    if (h.hi <= h.lo) return 0;
    const int64_t c0 = hot.chunk0[(size_t)h.lo], c1 = hot.chunk0[(size_t)h.hi];
    k_Pt_hot<POL, HALF><<<(unsigned)(c1 - c0), kHotT, 0, stream>>>(
        hot.d_range, c0, t->d_pl, HALF ? t->d_half : t->d_cos, t->d_sin, d_tod_tb, hot.d_partial);
    CM2_LAUNCH_OK();
    k_hot_combine<POL><<<(unsigned)(h.hi - h.lo), 256, 0, stream>>>(hot.d_tiles, h.lo, hot.d_partial, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

// ------------------------------------------------------------------- parts ----------
// Shares the slices of heavy tiles out to several workgroups (see cm2_tiles.h): the part length and the
// parts of every tile are policy::choose_parts' (CM2_PT_PARTS=0 keeps one workgroup per tile,
// CM2_PT_PARTS=<samples> fixes the target); here they become the plan's part lists and scratch.
int parts_plan(cm2_tiles *t, hipStream_t st)
{
    FxParts &pp = t->parts;
    if (!t->pt_split || t->fx.nslices == 0) return 0;
    const std::vector<int64_t> slice0 = policy::slices(t->tile_off, t->fx.S).slice0;
    // (two workgroups per CU of the simulated machine when their LDS fits twice, policy::fx_max_slice)
    const int slots = policy::fx_workgroups_per_cu(t->tp, t->pol, t->fx.S) * policy::kSimCUs;
    std::vector<int64_t> load((size_t)t->ntiles, 0), nslices((size_t)t->ntiles, 0);
    for (int64_t b = 0; b < t->ntiles; ++b) {
        nslices[(size_t)b] = slice0[(size_t)b + 1] - slice0[(size_t)b];
        if (!fx_hot_tile(t, b)) load[(size_t)b] = t->tile_count[(size_t)b];
    }
    const policy::PartsChoice choice = policy::choose_parts(load, nslices, t->fx.S, slots, t->sw.pt_parts);
    if (choice.target == 0) return 0;
    // the parts in tile order (= dispatch order), their scratch slots (split tiles only)
    std::vector<int4> parts;
    std::vector<int64_t> multi;
    pp.tile_part0.assign((size_t)t->ntiles + 1, 0);
    int64_t slot = 0;
    for (int64_t b = 0; b < t->ntiles; ++b) {
        pp.tile_part0[(size_t)b] = (int64_t)parts.size();
        const int64_t s0 = slice0[(size_t)b], ns = nslices[(size_t)b], k = choice.parts[(size_t)b];
        if (k > 1) {
            pp.multi_tile.push_back(b);
            multi.push_back(t->tile_p0[(size_t)b] * t->pol);
            multi.push_back((t->tile_p0[(size_t)b + 1] - t->tile_p0[(size_t)b]) * t->pol);
            multi.push_back(slot);
            multi.push_back(k);
        }
        for (int64_t j = 0; j < k; ++j) {
            const int64_t a = s0 + policy::part_slice(ns, j, k), e = s0 + policy::part_slice(ns, j + 1, k);
            parts.push_back(make_int4((int)b, (int)(e - a), (int)a, k > 1 ? (int)(slot + j) : -1));
        }
        if (k > 1) slot += k;
    }
    pp.tile_part0[(size_t)t->ntiles] = (int64_t)parts.size();
    if (pp.multi_tile.empty()) {                            // nothing to split after all
        pp.tile_part0.clear();
        return 0;
    }
    pp.nparts = (int64_t)parts.size();
    pp.slots = slot;
    pp.makespan = choice.makespan;
    CM2_HIP(cm2::dev_malloc(&pp.d_parts, sizeof(int4) * parts.size()));
    CM2_HIP(cm2::dev_malloc(&pp.d_multi, sizeof(int64_t) * multi.size()));
    CM2_HIP(cm2::dev_malloc(&pp.d_buf, sizeof(double) * (size_t)slot * (size_t)t->tp * (size_t)t->pol));
    CM2_HIP(cm2::upload(pp.d_parts, parts.data(), sizeof(int4) * parts.size(), st));
    CM2_HIP(cm2::upload(pp.d_multi, multi.data(), sizeof(int64_t) * multi.size(), st));
    CM2_HIP(hipStreamSynchronize(st));
    return 0;
}

// The device-side description of the fused form (FxFused) and its arrival counters, after hot_plan: one
// counter per hot tile, in a block of their own padded to 16 bytes (zeroed by one memset in front of every
// launch).  CM2_PT_FUSE=0 keeps the separate kernels.
int fused_plan(cm2_tiles *t, hipStream_t st)
{
    FxHot &hot = t->hot;
    if (!t->sw.pt_fuse) return 0;
    const size_t nhot = hot.tile.size();
    if (nhot == 0) return 0;
    hot.count_bytes = (sizeof(unsigned int) * nhot + 15) / 16 * 16;
    CM2_HIP(cm2::dev_malloc(&hot.d_count, hot.count_bytes));
    FxFused z;
    memset(&z, 0, sizeof(z));
    z.count = hot.d_count;
    z.hot_range = hot.d_range;
    z.hot_range_tile = hot.d_range_tile;
    z.hot_tiles = hot.d_tiles;
    z.hot_partial = hot.d_partial;
    z.pl = t->d_pl;
    z.a_tb = t->d_half ? t->d_half : t->d_cos;
    z.b_tb = t->d_sin;
    FxFused *dz = nullptr;
    CM2_HIP(cm2::dev_malloc(&dz, sizeof(FxFused)));
    hot.d_fused = dz;
    CM2_HIP(cm2::upload(dz, &z, sizeof(FxFused), st));
    CM2_HIP(hipStreamSynchronize(st));
    return 0;
}

template <int POL, bool HALF, int VPT>
int fx_launch_inst(const cm2_tiles *t, const double *d_tod_tb, double *d_out, int64_t tile_lo,
                   int64_t tile_hi, hipStream_t stream)
{
    const FxLists &f = t->fx;
    const FxParts &pp = t->parts;
    const FxHot &hot = t->hot;
    // plans with parts (and not the exact order): the workgroups are the parts of the tiles in range, in
    // tile (= address) order; then the copies of the split tiles are added up
    const bool parts = pp.d_parts && t->pt_fixed != 2;
    const int64_t q0 = parts ? pp.tile_part0[(size_t)tile_lo] : tile_lo;
    const int64_t q1 = parts ? pp.tile_part0[(size_t)tile_hi] : tile_hi;
    // fused form: the hot tiles' ranges inside [tile_lo, tile_hi) are further workgroups of this launch
    const bool fused = hot.d_fused && t->pt_fixed != 2;
    int64_t hc0 = 0, hc1 = 0;
    if (fused && hot.d_flag) {
        const policy::IndexRange h = policy::tiles_in_range(hot.tile, tile_lo, tile_hi);
        hc0 = hot.chunk0[(size_t)h.lo];
        hc1 = hot.chunk0[(size_t)h.hi];
    }
    size_t lds = policy::fx_lds_bytes(t->tp, t->pol, f.S);
    if (hc1 > hc0 && lds < sizeof(double) * (3 * (size_t)kHotT + 2)) lds = sizeof(double) * (3 * (size_t)kHotT + 2);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds((const void *)k_Pt_tiles_fixed<POL, HALF, VPT>, lds, granted));
    if (fused) CM2_HIP(hipMemsetAsync(hot.d_count, 0, hot.count_bytes, stream));
    k_Pt_tiles_fixed<POL, HALF, VPT><<<(int)(q1 - q0 + hc1 - hc0), kFxT, lds, stream>>>(
        t->tp, t->d_tile_p0, (int)tile_lo, f.d_sk, f.d_slice0, f.d_meta,
        f.d_gent, reinterpret_cast<const double2 *>(f.d_ga),
        reinterpret_cast<const double2 *>(f.d_gb), f.d_trun, f.d_tent, f.d_ta,
        f.d_tb, d_tod_tb, d_out,
        t->pt_fixed == 2 ? 0xFFFFFFFFu : (uint32_t)kFxChunkMinDefault,
        t->pt_fixed == 2 ? nullptr : hot.d_flag, parts ? pp.d_parts : nullptr, (int)q0, pp.d_buf,
        fused ? static_cast<const FxFused *>(hot.d_fused) : nullptr, (int)(q1 - q0), hc0);
    CM2_LAUNCH_OK();
    if (parts) {
        const policy::IndexRange m = policy::tiles_in_range(pp.multi_tile, tile_lo, tile_hi);
        if (m.hi > m.lo) {
            const dim3 cgrid((unsigned)(m.hi - m.lo), (unsigned)(((int64_t)t->tp * t->pol + 255) / 256));
            k_parts_combine<<<cgrid, 256, 0, stream>>>(pp.d_multi, m.lo, (int64_t)t->tp * t->pol, pp.d_buf, d_out);
            CM2_LAUNCH_OK();
        }
    }
    if (t->pt_fixed != 2 && hot.d_flag && !fused)
        return hot_launch<POL, HALF>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    return 0;
}

template <int POL, bool HALF>
int fx_launch_vpt(const cm2_tiles *t, const double *d_tod_tb, double *d_out, int64_t tile_lo,
                  int64_t tile_hi, hipStream_t stream)
{
    const int vpt = (t->fx.S + kFxT - 1) / kFxT;
    if (vpt <= 2) return fx_launch_inst<POL, HALF, 2>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    if (vpt == 3) return fx_launch_inst<POL, HALF, 3>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    return fx_launch_inst<POL, HALF, 4>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
}

}  // namespace

namespace cm2 {

void fx_free(cm2_tiles *t)
{
    t->fx.reset();
    t->parts.reset();
    t->hot.reset();
}

int fx_parts_info(const cm2_tiles *t, int64_t *h_info)
{
    const FxParts &pp = t->parts;
    h_info[0] = pp.d_parts ? pp.nparts : t->ntiles;
    h_info[1] = (int64_t)pp.multi_tile.size();
    h_info[2] = (int64_t)sizeof(double) * (pp.slots * t->tp * t->pol + (t->hot.chunk0.empty() ? 0 : 3 * t->hot.chunk0.back()));
    h_info[3] = (int64_t)(1000.0 * pp.makespan + 0.5);
    return 0;
}

int64_t fx_designed_bytes(const cm2_tiles *t)
{
    if (!t || !t->fx.S) return 0;
    const int64_t per_group = 16 + (t->pol > 1 ? (t->half ? 32 : 64) : 0);
    return 8 * t->nvalid + per_group * t->fx.ngroups + 8 * t->fx.nslices;
}

// plan of the fixed-order P^T, built on first use.  Slice length: a slice should fill most of
// the workgroup's 512 groups but rarely more; the number of groups per sample depends on how
// often a pixel is hit twice inside a slice, so it is measured: a count on a sample of the slices with S = 1536
// gives the groups per slice, S is then set for ~0.92 x 512 groups and the plan built, and rebuilt while the
// built lists ask for another length (policy::tune_slice; CM2_PT_SLICE = samples fixes S).
int fx_plan(const cm2_tiles *tc, hipStream_t st, bool *use)
{
    cm2_tiles *t = const_cast<cm2_tiles *>(tc);
    *use = false;
    if (!t->pt_fixed) return 0;
    // The lists are normally built by cm2_tiles_prepare_pt right after the plan (the Python layer
    // and the C demos call it): an application then allocates nothing and is safe to capture or
    // to issue from several host threads.  A plan that was not prepared builds them here, under
    // a lock (two threads applying P^T on one plan would otherwise both build).
    static std::mutex build_lock;
    std::lock_guard<std::mutex> hold(build_lock);
    if (t->fx_failed) {
        set_error("the fixed-order P^T lists of this tile plan could not be built (earlier error); "
                  "cm2_tiles_set_pt_order(t, 0) selects the atomic form");
        return CM2_ERR_HIP;
    }
    auto build = [&]() -> int {
        if (t->fx.S == 0) {
            // (4 staged values per thread at most.  Two workgroups per CU need <= 79 KB each: a 2048-pixel
            // IQU tile (48 KB) with four staged values per thread in two buffers (32 KB) would leave ONE
            // workgroup per CU (C5: P^T 0.53 -> 0.64 ms); the slice is kept short enough for two whenever
            // some slice length allows it.)
            if (policy::fx_tile_fills_lds(t->tp, t->pol)) {  // the tile alone fills LDS: atomics
                t->pt_fixed = 0;
                return 0;
            }
            int S = 0;
            const int rc = policy::tune_slice(
                t->sw.pt_slice, policy::fx_max_slice(t->tp, t->pol), kFxT, !t->sw.fx_serial,
                [&](int s, double &mean, double &over) { return fx_count_sample(t, s, st, &mean, &over); },
                [&](int s, double &mean, double &over) {
                    fx_free(t);
                    return fx_build_lists(t, s, st, &mean, &over);
                },
                &S);
            if (rc) return rc;
        }
        if (!t->hot.d_flag && t->hot.chunk0.empty()) {
            if (int rc = hot_plan(t, st)) return rc;
            if (int rc = parts_plan(t, st)) return rc;
            if (int rc = fused_plan(t, st)) return rc;
        }
        *use = true;
        return 0;
    };
    const int rc = build();
    if (rc) {
        t->fx.S = 0;
        // running out of device memory is transient: the failure is not remembered, so that the call may be made
        // again after the host has freed memory (cosmomap2_amd/_hip.py does that once; a build starts from scratch)
        if (rc != CM2_ERR_OUT_OF_MEMORY) t->fx_failed = 1;
    }
    return rc;
}

int fx_launch(const cm2_tiles *t, const double *d_tod_tb, double *d_out, int64_t tile_lo,
              int64_t tile_hi, hipStream_t stream)
{
    if (tile_hi <= tile_lo) return 0;
    if (t->pol == 1) return fx_launch_vpt<1, false>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    if (t->pol == 2)
        return t->half ? fx_launch_vpt<2, true>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream)
                       : fx_launch_vpt<2, false>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    return t->half ? fx_launch_vpt<3, true>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream)
                   : fx_launch_vpt<3, false>(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
}

}  // namespace cm2
