// cm2_tiles.hip -- tile-bucketed ("TB") TOD order and the LDS-staged pointing kernels
// that work on it.  This is the throughput path of the P^T N^-1 P chain when N has
// off-diagonal terms (so that a time-ordered TOD must exist between P and P^T).
//
// Why: with uniformly random pointing a time-ordered gather P x touches a random 24-B
// map record per sample and a pixel-major P^T touches a random 8-B TOD entry per sample;
// both pay a whole cache line for a few useful bytes (measured 2.0 ms each at 1e8
// samples / nside 256, i.e. 1.4 TB/s algorithmic).  Bucketing the samples by pixel TILE
// (TP pixels, tile map slice = TP*pol*8 B staged in LDS) makes every HBM access of the
// two pointing kernels a coalesced stream:
//
//   TB order   = stable partition of the valid samples by tile (time order inside a tile)
//   pl_tb u16  = pixel index inside the tile,  cos_tb / sin_tb f64     (static, built once)
//   tb_dst u32 = position of time sample t in TB order (0xFFFFFFFF for flagged samples)
//
//   P    : stage the tile of x in LDS, stream the bucket, write d_tb      26 B read + 8 B write
//   P^T  : stream the bucket, ds_add_f64 into the LDS tile, flush tile    26+8 B read
//   time<->TB permutation: time-order-driven; because the partition is stable every tile
//          is a sequential stream, so the scattered 8-B accesses combine in L2
//          (each workgroup owns one contiguous time range).                20 B / sample
//
// P on TB order evaluates the reference's per-sample expression; with both angle arrays
// (CM2_TILE_ANGLES=full) it is bit-identical to the reference loop, in the default half-angle
// storage cos / sin are rebuilt to 3.4e-16 absolute, so P agrees to rounding.
// P^T has two forms.  The default (k_Pt_tiles_fixed, CM2_PT_ORDER=fixed) adds the terms of every
// pixel IN TIME ORDER starting from 0, exactly like the reference's serial loop, with no
// atomics: bitwise reproducible from run to run and, with CM2_TILE_ANGLES=full, bit-identical to
// the serial loop.  CM2_PT_ORDER=atomic selects k_Pt_tiles (LDS + global fp64 atomics): the same
// set of terms per pixel in an unspecified order, equal to rounding, not reproducible.
//
// Reference loops replaced: interfaces/linearoperators.py:483-489 (mult_iqu) and :509-516
// (rmult_iqu) and their I / QU variants.
#include "cm2_perm_window.h"

#include <hipcub/hipcub.hpp>
#include <cstring>
#include <type_traits>

using namespace cm2;

static uint64_t next_plan_id()
{
    static uint64_t counter = 0;
    return ++counter;
}

// ------------------------------------------------------------------ build -------
// tile of pixel p: uniform tiles of tp pixels, or (p0 != nullptr) the tile whose pixel range
// [p0[b], p0[b + 1]) holds p -- tiles of equal sample count for uneven hit maps
__device__ __forceinline__ uint32_t tile_of(int32_t p, int tp, const int64_t *__restrict__ p0,
                                            uint32_t ntiles)
{
    if (p0 == nullptr) return (uint32_t)(p / tp);
    uint32_t lo = 0, hi = ntiles;                        // largest b with p0[b] <= p
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p0[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_tile_keys(const int32_t *__restrict__ pix, int64_t nt,
                                                    int tp, const int64_t *__restrict__ p0,
                                                    uint32_t ntiles, int64_t npix,
                                                    uint32_t *__restrict__ keys,
                                                    uint32_t *__restrict__ vals,
                                                    unsigned int *__restrict__ bad)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const int32_t p = pix[i];
        if (p < -1 || p >= npix) b = 1;                  // same rule as cm2_pointing_create
        keys[i] = (p < 0 || p >= npix) ? ntiles : tile_of(p, tp, p0, ntiles);
        vals[i] = (uint32_t)i;
    }
    if (b) atomicOr(bad, 1u);
}

// hits of every pixel (flagged / out-of-range samples skipped): input of the balanced tiling.
// A pixel that holds a large share of the samples (5e6 hits on one address: 50 ms of serialised
// global atomics) is counted in LDS: every workgroup keeps a direct-mapped table of 1024 pixels,
// first come first served; a sample whose slot belongs to its pixel is an LDS add, the others go to
// memory as before, and the table is flushed with one global add per slot.  Counts are integers:
// the result does not depend on which path a sample took.
__global__ __launch_bounds__(256) void k_pix_hist(const int32_t *__restrict__ pix, int64_t nt,
                                                   int64_t npix, unsigned int *__restrict__ hits)
{
    __shared__ unsigned int key[1024], cnt[1024];
    for (int i = threadIdx.x; i < 1024; i += 256) {
        key[i] = 0xFFFFFFFFu;
        cnt[i] = 0;
    }
    __syncthreads();
    const int64_t span = (nt + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * span, i1 = i0 + span < nt ? i0 + span : nt;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int32_t p = pix[i];
        if (p < 0 || p >= npix) continue;
        const unsigned int slot = ((unsigned int)p * 2654435761u) >> 22;
        const unsigned int old = atomicCAS(&key[slot], 0xFFFFFFFFu, (unsigned int)p);
        if (old == 0xFFFFFFFFu || old == (unsigned int)p) atomicAdd(&cnt[slot], 1u);
        else atomicAdd(&hits[p], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += 256)
        if (cnt[i]) atomicAdd(&hits[key[i]], cnt[i]);
}

__global__ __launch_bounds__(256) void k_tile_bounds(const uint32_t *__restrict__ keys, int64_t nt,
                                                      int64_t ntiles, int64_t *__restrict__ off)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > ntiles) return;
    int64_t lo = 0, hi = nt;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < (uint32_t)b) lo = mid + 1; else hi = mid;
    }
    off[b] = lo;
}

// ---- stable partition by tile without a sort ("multisplit") -----------------------------------
// Every wave owns kSplitChunk consecutive time samples.  Pass 1 (k_tile_rank): per sample its tile
// and its rank among the EARLIER samples of the same tile in the chunk -- 64 samples at a time:
// rank inside the row by comparing with every lower lane, plus the tile's running count in a
// wave-private LDS histogram (read by all lanes of the row, advanced by the last lane of each
// tile) -- and the chunk's count of every tile, stored tile-major.  One exclusive scan over the
// tile-major counts IS the tile order: base[tile][chunk] = first address of that chunk's samples
// of that tile.  Pass 2 (k_tile_place): address = base[tile][chunk] + rank.  The addresses are
// those of a stable sort by tile; nothing here depends on the order in which waves run.
constexpr int kSplitChunk = 8192;                        // samples per wave (rank fits 16 bits)
constexpr int64_t kSplitMaxTiles = 8192;                 // 4 wave histograms of u16 in 64 KB of LDS

__global__ __launch_bounds__(256) void k_tile_rank(const int32_t *__restrict__ pix, int64_t nt, int tp,
                                                    const int64_t *__restrict__ p0, uint32_t ntiles,
                                                    int64_t npix, int64_t nchunks,
                                                    uint32_t *__restrict__ packed,
                                                    uint32_t *__restrict__ cnt_t,
                                                    unsigned int *__restrict__ bad)
{
    extern __shared__ uint16_t hist_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t *hist = hist_all + (size_t)wave * ntiles;
    for (uint32_t b = lane; b < ntiles; b += 64) hist[b] = 0;
    const int64_t c = (int64_t)blockIdx.x * 4 + wave;
    if (c >= nchunks) return;
    const int64_t i0 = c * kSplitChunk, i1 = i0 + kSplitChunk < nt ? i0 + kSplitChunk : nt;
    unsigned int b_ = 0;
    for (int64_t i = i0; i < i1; i += 64) {
        const int64_t idx = i + lane;
        const bool in = idx < i1;
        const int32_t p = in ? pix[idx] : -1;
        if (p < -1 || p >= npix) b_ = 1;                 // same rule as cm2_pointing_create
        const bool valid = p >= 0 && p < npix;
        const int tile = valid ? (int)tile_of(p, tp, p0, ntiles) : -1;
        int rank = 0, same = 0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const int tj = __builtin_amdgcn_readlane(tile, j);
            const int eq = tj == tile ? 1 : 0;
            same += eq;
            rank += j < lane ? eq : 0;
        }
        if (valid) {
            const uint32_t r = (uint32_t)hist[tile] + (uint32_t)rank;
            packed[idx] = ((uint32_t)tile << 16) | r;
            if (rank == same - 1) hist[tile] = (uint16_t)(r + 1);
        } else if (in) {
            packed[idx] = 0xFFFFFFFFu;
        }
    }
    for (uint32_t b = lane; b < ntiles; b += 64) cnt_t[b * nchunks + c] = hist[b];
    if (b_) atomicOr(bad, 1u);
}

// off[b] = first address of tile b (b <= ntiles: the last one is the number of valid samples)
__global__ __launch_bounds__(256) void k_tile_offsets(const uint32_t *__restrict__ base, int64_t nchunks,
                                                       int64_t ntiles, int64_t *__restrict__ off)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= ntiles) off[b] = base[b * nchunks];
}

template <int POL, bool HALF>
__global__ __launch_bounds__(256) void k_tile_place(
    int64_t nt, int tp, const int64_t *__restrict__ p0,
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ base,
    const int32_t *__restrict__ pix, const double *__restrict__ c, const double *__restrict__ s,
    uint32_t *__restrict__ tb_dst, uint16_t *__restrict__ pl, double *__restrict__ ctb,
    double *__restrict__ stb)
{
    const int64_t nchunks = (nt + kSplitChunk - 1) / kSplitChunk;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const uint32_t pk = packed[i];
        if (pk == 0xFFFFFFFFu) {
            tb_dst[i] = kInvalidSample;                  // flagged samples sort behind every tile
            continue;
        }
        const int64_t tile = pk >> 16;
        const uint32_t k = base[tile * nchunks + i / kSplitChunk] + (pk & 0xFFFFu);
        tb_dst[i] = k;
        const int32_t px = pix[i];
        uint16_t w = p0 ? (uint16_t)(px - p0[tile]) : (uint16_t)(px - (int32_t)tile * tp);
        if (POL > 1) {
            if (HALF) {
                const double cv = c[i], sv = s[i];
                if (cv < 0.0) {
                    w |= 0x8000;
                    ctb[k] = sv / (1.0 - cv);
                } else {
                    ctb[k] = sv / (1.0 + cv);
                }
            } else {
                ctb[k] = c[i];
                stb[k] = s[i];
            }
        }
        pl[k] = w;
    }
}

// k_tile_place with the chunk's samples staged in LDS by address: one workgroup per chunk of
// kSplitChunk samples.  The chunk's samples of tile b occupy the addresses base[b][chunk] ..; in LDS
// they get the slots lbase[b] .. (lbase = scan of the chunk's per-tile counts), so that consecutive
// slots are consecutive addresses inside a run and the 2-byte words and half angles leave in pieces
// of 16 entries per tile instead of one scattered store per sample (4.9 -> 2 ms at C4).  Used for the
// one-array forms (pol = 1, half angles): 8192 doubles + 2 x 8192 words + two tables per tile.
template <int POL>
__global__ __launch_bounds__(256) void k_tile_place_staged(
    int64_t nt, int tp, const int64_t *__restrict__ p0, int ntiles,
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ base,
    const int32_t *__restrict__ pix, const double *__restrict__ c, const double *__restrict__ s,
    uint32_t *__restrict__ tb_dst, uint16_t *__restrict__ pl, double *__restrict__ ctb)
{
    extern __shared__ double sm_p[];
    double *hs = sm_p;                                              // [kSplitChunk] half angles by slot
    uint32_t *gbase = reinterpret_cast<uint32_t *>(hs + (POL > 1 ? kSplitChunk : 0));   // [ntiles]
    uint32_t *lbase = gbase + ntiles;                               // [ntiles + 1]
    uint16_t *ws = reinterpret_cast<uint16_t *>(lbase + ntiles + 1);   // [kSplitChunk] pl words by slot
    uint16_t *ts = ws + kSplitChunk;                                // [kSplitChunk] tile of the slot
    __shared__ uint32_t wsum[4];
    const int64_t ch = blockIdx.x, nchunks = gridDim.x;
    const int64_t i0 = ch * kSplitChunk, i1 = i0 + kSplitChunk < nt ? i0 + kSplitChunk : nt;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // per-tile counts of the chunk (next word of the tile-major scan minus this one), scanned
    const int per = (ntiles + 255) / 256;
    uint32_t mine = 0;
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) {
        const int64_t ci = b * nchunks + ch;
        const uint32_t g0 = base[ci], g1 = base[ci + 1];
        gbase[b] = g0;
        lbase[b] = g1 - g0;
        mine += g1 - g0;
    }
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) {
        const uint32_t cnt = lbase[b];
        lbase[b] = before;
        before += cnt;
    }
    if (t == 0) lbase[ntiles] = total;
    __syncthreads();
    // (one workgroup per CU: four samples per thread in flight at a time)
    for (int64_t ib = i0 + t; ib < i1; ib += 4 * 256) {
        uint32_t pk[4];
        int32_t px[4];
        double cv[4], sv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = ib + 256 * u;
            const bool in = i < i1;
            pk[u] = in ? packed[i] : 0xFFFFFFFFu;
            px[u] = in ? pix[i] : 0;
            if (POL > 1) {
                cv[u] = in ? c[i] : 1.0;
                sv[u] = in ? s[i] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = ib + 256 * u;
            if (i >= i1) continue;
            if (pk[u] == 0xFFFFFFFFu) {
                tb_dst[i] = kInvalidSample;
                continue;
            }
            const uint32_t tile = pk[u] >> 16, r = pk[u] & 0xFFFFu;
            tb_dst[i] = gbase[tile] + r;
            const uint32_t slot = lbase[tile] + r;
            uint16_t w = p0 ? (uint16_t)(px[u] - p0[tile]) : (uint16_t)(px[u] - (int32_t)tile * tp);
            if (POL > 1) {
                if (cv[u] < 0.0) {
                    w |= 0x8000;
                    hs[slot] = sv[u] / (1.0 - cv[u]);
                } else {
                    hs[slot] = sv[u] / (1.0 + cv[u]);
                }
            }
            ws[slot] = w;
            ts[slot] = (uint16_t)tile;
        }
    }
    __syncthreads();
    for (uint32_t j = t; j < total; j += 256) {
        const uint32_t tile = ts[j];
        const uint32_t k = gbase[tile] + (j - lbase[tile]);
        pl[k] = ws[j];
        if (POL > 1) ctb[k] = hs[j];
    }
}

// 1 if some (cos, sin) pair is not on the unit circle to rounding: then the half-angle form
// would change the operator and the full arrays are kept
__global__ __launch_bounds__(256) void k_unit_circle(int64_t nt, const double *__restrict__ c,
                                                      const double *__restrict__ s,
                                                      unsigned int *__restrict__ off_circle)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const double r = c[i] * c[i] + s[i] * s[i] - 1.0;
        if (!(fabs(r) <= 1e-14)) bad = 1;
    }
    if (bad) atomicOr(off_circle, 1u);
}

template <int POL, bool HALF>
__global__ __launch_bounds__(256) void k_tile_fill(
    int64_t nt, int64_t nvalid, int tp, const int64_t *__restrict__ p0, uint32_t ntiles,
    const uint32_t *__restrict__ tb_src,
    const int32_t *__restrict__ pix, const double *__restrict__ c, const double *__restrict__ s,
    uint32_t *__restrict__ tb_dst, uint16_t *__restrict__ pl, double *__restrict__ ctb,
    double *__restrict__ stb)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nt; k += stride) {
        const uint32_t t = tb_src[k];
        if (k < nvalid) {
            tb_dst[t] = (uint32_t)k;
            const int32_t px = pix[t];
            uint16_t w = p0 ? (uint16_t)(px - p0[tile_of(px, tp, p0, ntiles)]) : (uint16_t)(px % tp);
            if (POL > 1) {
                if (HALF) {
                    const double cv = c[t], sv = s[t];
                    if (cv < 0.0) {
                        w |= 0x8000;
                        ctb[k] = sv / (1.0 - cv);
                    } else {
                        ctb[k] = sv / (1.0 + cv);
                    }
                } else {
                    ctb[k] = c[t];
                    stb[k] = s[t];
                }
            }
            pl[k] = w;
        } else {
            tb_dst[t] = kInvalidSample;      // flagged samples sort behind every tile
        }
    }
}

// (pixel in tile, cos, sin) of TB sample k in either storage form
template <int POL, bool HALF>
__device__ __forceinline__ void tile_sample(const uint16_t *__restrict__ pl,
                                            const double *__restrict__ c,
                                            const double *__restrict__ s, int64_t k, int &q,
                                            double &cc, double &ss)
{
    const uint16_t w = pl[k];
    if (POL == 1) {
        q = w;
        cc = ss = 0.0;
    } else if (HALF) {
        q = w & 0x7FFF;
        const double h = c[k], h2 = h * h, inv = 1.0 / (1.0 + h2);
        cc = (1.0 - h2) * inv;
        ss = (h + h) * inv;
        if (w & 0x8000) cc = -cc;
    } else {
        q = w;
        cc = c[k];
        ss = s[k];
    }
}

// workgroup size of the two tile kernels: 1024 threads for the gather (0.355 vs 0.38 ms at
// 1e8 samples), 512 for the scatter (no difference)
constexpr int kPBlock = 1024, kPtBlock = 512;

// ------------------------------------------------------------------ P (TB) ------
// one workgroup per work item = (tile, addresses [k0, k1) of its bucket): the tile of x is staged
// once, the item's samples are streamed
template <int POL, bool HALF>
__global__ __launch_bounds__(1024) void k_P_tiles(
    const int64_t *__restrict__ tile_p0, const int32_t *__restrict__ item_tile,
    const int64_t *__restrict__ item_k0, const int64_t *__restrict__ item_k1,
    const uint16_t *__restrict__ pl, const double *__restrict__ c, const double *__restrict__ s,
    const double *__restrict__ x, double *__restrict__ d_tb)
{
    extern __shared__ double tile[];                    // tp*POL doubles
    const int b = item_tile[blockIdx.x];
    const int64_t p0 = tile_p0[b];
    const int64_t np = tile_p0[b + 1] - p0;
    const int64_t nvals = np * POL;
    const double *xs = x + p0 * POL;
    for (int64_t i = threadIdx.x; i < nvals; i += blockDim.x) tile[i] = xs[i];
    __syncthreads();
    const int64_t k0 = item_k0[blockIdx.x], k1 = item_k1[blockIdx.x];
    for (int64_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
        int q;
        double cc, ss;
        tile_sample<POL, HALF>(pl, c, s, k, q, cc, ss);
        double r = 0.0;
        if (POL == 1) {
            r += tile[q];
        } else if (POL == 2) {
            r += tile[2 * q] * cc + tile[2 * q + 1] * ss;
        } else {
            r += tile[3 * q] + tile[3 * q + 1] * cc + tile[3 * q + 2] * ss;
        }
        d_tb[k] = r;
    }
}

// ---------------------------------------------------------------- P^T (TB) ------
// (launched with kPtBlock threads.  The strides are compile-time constants: with blockDim.x the
// compiler kept a 64-bit address per unrolled load in VGPRs, 80 instead of 38 at pol = 3)
template <int POL, bool HALF>
__global__ __launch_bounds__(kPtBlock) void k_Pt_tiles(
    const int64_t *__restrict__ tile_p0, const int32_t *__restrict__ item_tile,
    const int64_t *__restrict__ item_k0, const int64_t *__restrict__ item_k1,
    const uint16_t *__restrict__ pl, const double *__restrict__ c, const double *__restrict__ s,
    const double *__restrict__ v_tb, double *__restrict__ out)
{
    extern __shared__ double tile[];                    // tp*POL accumulators
    const int b = item_tile[blockIdx.x];
    const int64_t p0 = tile_p0[b];
    const int64_t np = tile_p0[b + 1] - p0;
    const int64_t nvals = np * POL;
    for (int64_t i = threadIdx.x; i < nvals; i += kPtBlock) tile[i] = 0.0;
    __syncthreads();
    const int64_t k1 = item_k1[blockIdx.x];
    constexpr int U = 4;                     // independent loads in flight per thread
    int64_t k = item_k0[blockIdx.x] + threadIdx.x;
    for (; k + (U - 1) * kPtBlock < k1; k += U * kPtBlock) {
        int q[U];
        double v[U], cc[U], ss[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = k + u * kPtBlock;
            v[u] = v_tb[kk];
            tile_sample<POL, HALF>(pl, c, s, kk, q[u], cc[u], ss[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (POL == 1) {
                atomicAdd(&tile[q[u]], v[u]);
            } else if (POL == 2) {
                atomicAdd(&tile[2 * q[u]], v[u] * cc[u]);
                atomicAdd(&tile[2 * q[u] + 1], v[u] * ss[u]);
            } else {
                atomicAdd(&tile[3 * q[u]], v[u]);
                atomicAdd(&tile[3 * q[u] + 1], v[u] * cc[u]);
                atomicAdd(&tile[3 * q[u] + 2], v[u] * ss[u]);
            }
        }
    }
    for (; k < k1; k += kPtBlock) {
        int q;
        double c1, s1;
        tile_sample<POL, HALF>(pl, c, s, k, q, c1, s1);
        const double v = v_tb[k];
        if (POL == 1) {
            atomicAdd(&tile[q], v);
        } else if (POL == 2) {
            atomicAdd(&tile[2 * q], v * c1);
            atomicAdd(&tile[2 * q + 1], v * s1);
        } else {
            atomicAdd(&tile[3 * q], v);
            atomicAdd(&tile[3 * q + 1], v * c1);
            atomicAdd(&tile[3 * q + 2], v * s1);
        }
    }
    __syncthreads();
    double *o = out + p0 * POL;
    for (int64_t i = threadIdx.x; i < nvals; i += kPtBlock) atomicAdd(&o[i], tile[i]);
}

// ------------------------------------------------------- time <-> TB order ------
// each workgroup owns ONE contiguous time range, so that the K sequential tile streams
// it touches stay in its XCD's L2 until their lines are complete
__global__ __launch_bounds__(1024) void k_time_to_tiles(int64_t nt, int64_t chunk,
                                                         const uint32_t *__restrict__ tb_dst,
                                                         const double *__restrict__ in,
                                                         double *__restrict__ out_tb)
{
    const int64_t t0 = (int64_t)blockIdx.x * chunk;
    int64_t t1 = t0 + chunk;
    if (t1 > nt) t1 = nt;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) {
        const uint32_t k = tb_dst[t];
        if (k != kInvalidSample) out_tb[k] = in[t];
    }
}

__global__ __launch_bounds__(1024) void k_tiles_to_time(int64_t nt, int64_t chunk,
                                                         const uint32_t *__restrict__ tb_dst,
                                                         const double *__restrict__ in_tb,
                                                         double *__restrict__ out)
{
    const int64_t t0 = (int64_t)blockIdx.x * chunk;
    int64_t t1 = t0 + chunk;
    if (t1 > nt) t1 = nt;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) {
        const uint32_t k = tb_dst[t];
        out[t] = (k != kInvalidSample) ? in_tb[k] : 0.0;
    }
}

// Windowed forms of the two permutations.  A per-sample scatter / gather between the orders
// moves 8-byte fragments (a window's samples of one tile are ~20 contiguous entries) and the
// caches write lines back before they are complete: 3.2 GB of HBM writes for 0.8 GB of
// payload.  Here a workgroup owns kPermWin consecutive time samples, reaches their TB
// positions through a list sorted by address (one contiguous run per tile) and stages the
// window in LDS, so that both sides of the copy are streams: 6 + 8 + 8 bytes per sample.
// (the list format and the pieces the kernel is made of: cm2_perm_window.h, shared with cm2_gaps.hip,
// cm2_offsets.hip and cm2_filter.hip)

template <bool TO_TIME>
__global__ __launch_bounds__(kPermT) void k_perm_windows(int64_t nt, int64_t nwin,
                                                          const uint32_t *__restrict__ lst_k,
                                                          const uint16_t *__restrict__ lst_q,
                                                          const double *__restrict__ in,
                                                          double *__restrict__ out)
{
    __shared__ double win[kPermWin];
    const int64_t w = window_of_workgroup(nwin);
    if (w >= nwin) return;
    const int64_t t0 = w * kPermWin;
    const int span = (int)window_span(nt, t0);
    const int t = threadIdx.x;
    WindowEntries e;
    e.load(lst_k, lst_q, w);
    if (TO_TIME) {
        double vv[kPermPer];
        e.gather(in, vv);
        for (int j = t; j < span; j += kPermT) win[j] = 0.0;      // flagged samples read as 0
        __syncthreads();
        e.each_valid([&](int u, uint32_t, uint16_t q) { win[q] = vv[u]; });
        __syncthreads();
        for (int j = t; j < span; j += kPermT) out[t0 + j] = win[j];
    } else {
        for (int j = t; j < span; j += kPermT) win[j] = in[t0 + j];
        __syncthreads();
        e.each_valid([&](int, uint32_t k, uint16_t q) { out[k] = win[q]; });
    }
}

__global__ __launch_bounds__(256) void k_perm_keys(int64_t nt, int64_t nwin,
                                                    const uint32_t *__restrict__ tb_dst,
                                                    uint64_t *__restrict__ keys,
                                                    uint16_t *__restrict__ vals)
{
    const int64_t total = nwin * kPermWin;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t k = g < nt ? tb_dst[g] : kInvalidSample;
        keys[g] = ((uint64_t)(g / kPermWin) << 32) | (uint64_t)k;
        vals[g] = (uint16_t)(g % kPermWin);
    }
}

__global__ __launch_bounds__(256) void k_perm_unpack(int64_t total, const uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ lst_k)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride)
        lst_k[g] = (uint32_t)(keys[g] & 0xFFFFFFFFull);
}


// ------------------------------------------------------------------ C ABI -------
// f(std::integral_constant<int, POL>, std::bool_constant<HALF>) for the storage form of the plan: pol 1,
// pol 2 and 3 with half or full angles (the five instances of the <POL, HALF> kernels)
template <typename F>
static int with_pol_half(const cm2_tiles *t, F &&f)
{
    using std::integral_constant;
    if (t->pol == 1) return f(integral_constant<int, 1>{}, std::false_type{});
    if (t->pol == 2)
        return t->half ? f(integral_constant<int, 2>{}, std::true_type{}) : f(integral_constant<int, 2>{}, std::false_type{});
    return t->half ? f(integral_constant<int, 3>{}, std::true_type{}) : f(integral_constant<int, 3>{}, std::false_type{});
}

extern "C" int cm2_tiles_destroy(cm2_tiles *t)
{
    if (!t) return 0;
    void *ptrs[] = {t->d_tb_dst, t->d_pl, t->d_cos, t->d_sin, t->d_half, t->d_item_tile, t->d_item_k0,
                    t->d_item_k1, t->d_perm_k, t->d_perm_q, t->d_tile_off, t->d_tile_p0};
    for (void *q : ptrs)
        if (q) (void)cm2::dev_free(q);
    cm2::fx_free(t);
    delete t;
    return 0;
}

// The one place where the environment steers a tile plan (the values: PlanSwitches, cm2_tiles.h).
static PlanSwitches read_plan_switches()
{
    PlanSwitches sw;
    auto is = [](const char *e, const char *v) { return e && strcmp(e, v) == 0; };
    if (const char *e = getenv("CM2_PT_ORDER")) sw.pt_order = is(e, "atomic") ? 0 : (is(e, "exact") ? 2 : 1);
    sw.tile_sort = is(getenv("CM2_TILE_BUILD"), "sort");
    if (const char *e = getenv("CM2_TILE_BALANCE"))
        sw.balance = is(e, "parts") ? policy::Balance::parts
                                    : (is(e, "cut") || atoi(e) != 0 ? policy::Balance::cut : policy::Balance::off);
    sw.full_angles = is(getenv("CM2_TILE_ANGLES"), "full");
    sw.fx_serial = is(getenv("CM2_FX_BUILD"), "serial");
    if (const char *e = getenv("CM2_PT_SLICE")) sw.pt_slice = atoi(e);
    if (const char *e = getenv("CM2_PT_PARTS")) sw.pt_parts = atoi(e);
    if (const char *e = getenv("CM2_PT_FUSE")) sw.pt_fuse = atoi(e) != 0;
    return sw;
}

// Stable partition of the samples by tile.  Default: the multisplit above (k_tile_rank, one scan,
// k_tile_place).  With more tiles than its LDS histograms hold, or CM2_TILE_BUILD=sort: a radix sort of
// (tile, time) pairs and a gather (k_tile_fill).  Same addresses either way.  Owns the temporaries of both
// paths: run() partitions by the plan's current tiles (again after a re-cut), place() writes the plan's
// per-sample arrays from what the last run left.
struct Partition {
    cm2_tiles *t;
    const int32_t *d_pix;
    hipStream_t stream;
    int64_t nchunks;                                           // chunks of kSplitChunk samples
    DevTemp<uint32_t> keys_in, keys_out, vals_in, tb_src;      // sort path
    DevTemp<uint32_t> packed, cnt_t;                           // multisplit: tile << 16 | rank; counts -> bases
    DevTemp<int64_t> d_off;
    DevTemp<char> d_temp;
    DevTemp<unsigned int> d_bad;                               // a pixel index outside [-1, npix) was seen
    std::vector<int64_t> off;                                  // first address of every tile
    bool sorted = false;                                       // which path the last run took

    int sort(const int64_t *d_p0)
    {
        const int64_t nt = t->nt;
        if (!keys_in.p) {
            CM2_HIP(keys_in.alloc(nt));
            CM2_HIP(keys_out.alloc(nt));
            CM2_HIP(vals_in.alloc(nt));
            CM2_HIP(tb_src.alloc(nt));
        }
        k_tile_keys<<<grid_for(nt), kBlock, 0, stream>>>(d_pix, nt, t->tp, d_p0, (uint32_t)t->ntiles, t->npix,
                                                         keys_in, vals_in, d_bad);
        CM2_LAUNCH_OK();
        int end_bit = 1;
        while (((int64_t)1 << end_bit) <= t->ntiles) ++end_bit;
        size_t tb = 0;
        CM2_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in.p, keys_out.p, vals_in.p,
                                                   tb_src.p, nt, 0, end_bit, stream));
        d_temp.release();
        CM2_HIP(d_temp.alloc(tb + 16));
        CM2_HIP(hipcub::DeviceRadixSort::SortPairs(d_temp.p, tb, keys_in.p, keys_out.p, vals_in.p,
                                                   tb_src.p, nt, 0, end_bit, stream));
        k_tile_bounds<<<(int)((t->ntiles + 1 + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
            keys_out, nt, t->ntiles, d_off);
        CM2_LAUNCH_OK();
        return 0;
    }

    int split(const int64_t *d_p0)
    {
        const int64_t ncnt = t->ntiles * nchunks + 1;          // (+1: the scan's last word = nvalid)
        if (!packed.p) CM2_HIP(packed.alloc(t->nt));
        cnt_t.release();
        CM2_HIP(cnt_t.alloc(ncnt));
        CM2_HIP(hipMemsetAsync(cnt_t.p, 0, sizeof(uint32_t) * ncnt, stream));
        const size_t lds = sizeof(uint16_t) * 4 * (size_t)t->ntiles;
        static size_t granted[64] = {0};
        CM2_HIP(ensure_dynamic_lds((const void *)k_tile_rank, lds, granted));
        k_tile_rank<<<(unsigned)((nchunks + 3) / 4), 256, lds, stream>>>(
            d_pix, t->nt, t->tp, d_p0, (uint32_t)t->ntiles, t->npix, nchunks, packed, cnt_t, d_bad);
        CM2_LAUNCH_OK();
        CM2_CHECK(ncnt < ((int64_t)1 << 31), "cm2_tiles_create: %lld tile x chunk counts", (long long)ncnt);
        size_t tb = 0;
        CM2_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt_t.p, cnt_t.p, (int)ncnt, stream));
        d_temp.release();
        CM2_HIP(d_temp.alloc(tb + 16));
        CM2_HIP(hipcub::DeviceScan::ExclusiveSum(d_temp.p, tb, cnt_t.p, cnt_t.p, (int)ncnt, stream));
        k_tile_offsets<<<(int)((t->ntiles + 1 + kBlock - 1) / kBlock), kBlock, 0, stream>>>(cnt_t, nchunks,
                                                                                            t->ntiles, d_off);
        CM2_LAUNCH_OK();
        return 0;
    }

    // d_p0: the tiles' first pixels on the device (nullptr: uniform tiles of t->tp pixels)
    int run(const int64_t *d_p0)
    {
        if (!d_bad.p) {
            CM2_HIP(d_bad.alloc(1));
            CM2_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned int), stream));
        }
        d_off.release();
        sorted = t->sw.tile_sort || t->ntiles > kSplitMaxTiles || t->ntiles * nchunks + 1 >= ((int64_t)1 << 31);
        CM2_HIP(d_off.alloc(t->ntiles + 1));
        if (int rc = sorted ? sort(d_p0) : split(d_p0)) return rc;
        off.assign((size_t)t->ntiles + 1, 0);
        CM2_HIP(cm2::download(off.data(), d_off, sizeof(int64_t) * (t->ntiles + 1), stream));
        CM2_HIP(hipStreamSynchronize(stream));
        return 0;
    }

    int place(const double *d_cos, const double *d_sin)
    {
        const int64_t nt = t->nt;
        const int64_t *d_p0 = t->balanced ? t->d_tile_p0 : nullptr;
        return with_pol_half(t, [&](auto pol_c, auto half_c) -> int {
            constexpr int POL = decltype(pol_c)::value;
            constexpr bool HALF = decltype(half_c)::value;
            if (sorted)
                k_tile_fill<POL, HALF><<<grid_for(nt), kBlock, 0, stream>>>(
                    nt, t->nvalid, t->tp, d_p0, (uint32_t)t->ntiles, tb_src, d_pix, d_cos, d_sin, t->d_tb_dst,
                    t->d_pl, HALF ? t->d_half : t->d_cos, t->d_sin);
            else if ((HALF || POL == 1) && t->ntiles <= 4096) {
                const size_t lds = (POL > 1 ? sizeof(double) * kSplitChunk : 0) +
                                   sizeof(uint32_t) * (2 * (size_t)t->ntiles + 1) + sizeof(uint16_t) * 2 * kSplitChunk;
                static size_t granted[64] = {0};
                CM2_HIP(ensure_dynamic_lds((const void *)k_tile_place_staged<POL>, lds, granted));
                k_tile_place_staged<POL><<<(unsigned)nchunks, 256, lds, stream>>>(
                    nt, t->tp, d_p0, (int)t->ntiles, packed, cnt_t, d_pix, d_cos, d_sin, t->d_tb_dst, t->d_pl,
                    t->d_half);
            } else
                k_tile_place<POL, HALF><<<grid_for(nt), kBlock, 0, stream>>>(
                    nt, t->tp, d_p0, packed, cnt_t, d_pix, d_cos, d_sin, t->d_tb_dst, t->d_pl,
                    HALF ? t->d_half : t->d_cos, t->d_sin);
            CM2_LAUNCH_OK();
            return 0;
        });
    }
};

// hits of every pixel on the host (input of the policy's re-cuts); d_hits: the caller's temporary
static int pixel_hits(const int32_t *d_pix, int64_t nt, int64_t npix, hipStream_t stream,
                      DevTemp<unsigned int> &d_hits, std::vector<unsigned int> &hits)
{
    CM2_HIP(d_hits.alloc(npix));
    CM2_HIP(hipMemsetAsync(d_hits, 0, sizeof(unsigned int) * npix, stream));
    k_pix_hist<<<grid_for(nt), kBlock, 0, stream>>>(d_pix, nt, npix, d_hits);
    CM2_LAUNCH_OK();
    hits.resize((size_t)npix);
    CM2_HIP(cm2::download(hits.data(), d_hits, sizeof(unsigned int) * npix, stream));
    CM2_HIP(hipStreamSynchronize(stream));
    return 0;
}

extern "C" int cm2_tiles_create(cm2_tiles **out, const int32_t *d_pix, const double *d_cos,
                                const double *d_sin, int64_t nt, int64_t npix, int pol,
                                int tile_pixels, int64_t slice_samples, void *stream_)
{
    CM2_CHECK(out != nullptr, "cm2_tiles_create: out is NULL");
    *out = nullptr;
    CM2_CHECK(pol == 1 || pol == 2 || pol == 3, "cm2_tiles_create: bad pol=%d", pol);
    CM2_CHECK(pol == 1 || (d_cos && d_sin), "cm2_tiles_create: cos/sin required for pol=%d", pol);
    CM2_CHECK(nt > 0 && nt < (int64_t)0xFFFFFFFF, "cm2_tiles_create: nt=%lld out of range",
              (long long)nt);
    CM2_CHECK(tile_pixels >= 64 && tile_pixels <= 65536 && tile_pixels * pol * 8 <= 160 * 1024 - 1024,
              "cm2_tiles_create: tile of %d pixels does not fit LDS / uint16", tile_pixels);
    CM2_CHECK(slice_samples >= 256, "cm2_tiles_create: slice too short");
    hipStream_t stream = as_stream(stream_);
    cm2_tiles *t = new cm2_tiles();
    struct Guard { cm2_tiles *t; ~Guard() { if (t) cm2_tiles_destroy(t); } } guard{t};
    t->nt = nt; t->npix = npix; t->pol = pol; t->tp = tile_pixels;
    t->plan_id = next_plan_id();
    t->sw = read_plan_switches();
    // order of the per-pixel sums of P^T: fixed (time order, reproducible; default), exact or atomic
    t->pt_fixed = t->sw.pt_order;
    if (cm2::exact_order_setting() >= 0 && t->pt_fixed) t->pt_fixed = cm2::exact_order_setting() ? 2 : 1;

    // uniform tiles first: their loads decide the tiling
    t->tile_p0 = policy::uniform_tiles(npix, tile_pixels);
    t->ntiles = (int64_t)t->tile_p0.size() - 1;
    Partition part{t, d_pix, stream, (nt + kSplitChunk - 1) / kSplitChunk};
    if (int rc = part.run(nullptr)) return rc;
    unsigned int h_bad = 0;
    CM2_HIP(cm2::download(&h_bad, part.d_bad, sizeof(h_bad), nullptr));
    CM2_CHECK(h_bad == 0, "cm2_tiles_create: a pixel index is outside [-1, npix=%lld)",
              (long long)npix);
    const policy::TilingChoice choice = policy::choose_tiling(part.off, t->pt_fixed == 2, t->sw.balance);
    t->pt_split = choice.pt_split;
    DevTemp<int64_t> d_p0;
    {
        std::vector<int64_t> p0v;                           // re-cut boundaries (empty: the uniform tiles stay)
        DevTemp<unsigned int> d_hits;
        std::vector<unsigned int> hits;
        if (choice.tiling == policy::Tiling::equal_load) {
            if (int rc = pixel_hits(d_pix, nt, npix, stream, d_hits, hits)) return rc;
            p0v = policy::equal_load_tiles(hits, npix, tile_pixels, t->ntiles, part.off[(size_t)t->ntiles]);
        } else if (choice.hot_min > 0) {
            if (int rc = pixel_hits(d_pix, nt, npix, stream, d_hits, hits)) return rc;
            bool any = false;
            p0v = policy::hot_pixel_tiles(hits, npix, tile_pixels, choice.hot_min, &any);
            if (!any) p0v.clear();
        }
        // balanced = "the tiles are not the uniform grid", whichever rule re-cut them: the kernels then find a
        // pixel's tile in d_tile_p0, and only the shared cuts (policy::shared_cuts) are boundaries for sure
        t->balanced = !p0v.empty();
        if (t->balanced) {
            t->ntiles = (int64_t)p0v.size() - 1;
            t->tile_p0 = p0v;
            CM2_HIP(d_p0.alloc(p0v.size()));
            CM2_HIP(cm2::upload(d_p0.p, p0v.data(), sizeof(int64_t) * p0v.size(), nullptr));
            if (int rc = part.run(d_p0.p)) return rc;
        }
    }
    const std::vector<int64_t> &off = part.off;
    CM2_HIP(cm2::dev_malloc(&t->d_tile_p0, sizeof(int64_t) * (t->ntiles + 1)));
    CM2_HIP(cm2::upload(t->d_tile_p0, t->tile_p0.data(), sizeof(int64_t) * (t->ntiles + 1), nullptr));
    t->nvalid = off[t->ntiles];
    t->tile_count.assign((size_t)t->ntiles, 0);
    for (int64_t b = 0; b < t->ntiles; ++b) t->tile_count[(size_t)b] = off[(size_t)b + 1] - off[(size_t)b];
    t->tile_off = off;
    t->d_tile_off = part.d_off.keep();

    const int64_t nv = t->nvalid > 0 ? t->nvalid : 1;
    CM2_HIP(cm2::dev_malloc(&t->d_tb_dst, sizeof(uint32_t) * nt));
    CM2_HIP(cm2::dev_malloc(&t->d_pl, sizeof(uint16_t) * nv));
    // half-angle storage (one double per sample instead of cos and sin) when every pair lies
    // on the unit circle; CM2_TILE_ANGLES=full keeps both arrays
    t->half = false;
    if (pol > 1 && nt > 0 && tile_pixels <= 0x8000 && !t->sw.full_angles) {
        DevTemp<unsigned int> d_off_circle;
        CM2_HIP(d_off_circle.alloc(1));
        CM2_HIP(hipMemsetAsync(d_off_circle, 0, sizeof(unsigned int), stream));
        k_unit_circle<<<grid_for(nt), kBlock, 0, stream>>>(nt, d_cos, d_sin, d_off_circle);
        CM2_LAUNCH_OK();
        unsigned int h_off = 0;
        CM2_HIP(cm2::download(&h_off, d_off_circle, sizeof(h_off), stream));
        CM2_HIP(hipStreamSynchronize(stream));
        t->half = (h_off == 0);
    }
    if (pol > 1) {
        if (t->half) {
            CM2_HIP(cm2::dev_malloc(&t->d_half, sizeof(double) * nv));
        } else {
            CM2_HIP(cm2::dev_malloc(&t->d_cos, sizeof(double) * nv));
            CM2_HIP(cm2::dev_malloc(&t->d_sin, sizeof(double) * nv));
        }
    }
    if (int rc = part.place(d_cos, d_sin)) return rc;
    // work items: every tile's bucket cut into address ranges of at most slice_samples (none for an empty one)
    const policy::WorkItems items = policy::work_items(off, slice_samples);
    t->tile_item0 = items.tile_item0;
    t->nitems = (int64_t)items.tile.size();
    const int64_t ni = t->nitems > 0 ? t->nitems : 1;
    CM2_HIP(cm2::dev_malloc(&t->d_item_tile, sizeof(int32_t) * ni));
    CM2_HIP(cm2::dev_malloc(&t->d_item_k0, sizeof(int64_t) * ni));
    CM2_HIP(cm2::dev_malloc(&t->d_item_k1, sizeof(int64_t) * ni));
    if (t->nitems) {
        CM2_HIP(cm2::upload(t->d_item_tile, items.tile.data(), sizeof(int32_t) * ni, nullptr));
        CM2_HIP(cm2::upload(t->d_item_k0, items.k0.data(), sizeof(int64_t) * ni, nullptr));
        CM2_HIP(cm2::upload(t->d_item_k1, items.k1.data(), sizeof(int64_t) * ni, nullptr));
    }
    CM2_HIP(hipStreamSynchronize(stream));
    guard.t = nullptr;
    *out = t;
    return 0;
}

extern "C" int cm2_tiles_info(const cm2_tiles *t, int64_t *h_info)
{
    CM2_CHECK(t && h_info, "cm2_tiles_info: NULL argument");
    h_info[0] = t->nt; h_info[1] = t->nvalid; h_info[2] = t->tp;
    h_info[3] = t->ntiles; h_info[4] = t->nitems; h_info[5] = t->half ? 1 : 0;
    h_info[6] = t->pt_fixed; h_info[7] = (int64_t)t->plan_id;
    h_info[8] = t->fx.S; h_info[9] = cm2::fx_designed_bytes(t);
    // (the two fields of the span order removed in round 5: one span of all the chunks of kSplitChunk samples)
    h_info[10] = 1; h_info[11] = (t->nt + kSplitChunk - 1) / kSplitChunk * kSplitChunk;
    return 0;
}

extern "C" int cm2_tiles_pt_parts(const cm2_tiles *t, int64_t *h_info)
{
    CM2_CHECK(t && h_info, "cm2_tiles_pt_parts: NULL argument");
    return cm2::fx_parts_info(t, h_info);
}

extern "C" int cm2_tiles_prepare_pt(cm2_tiles *t, void *stream_)
{
    CM2_CHECK(t, "cm2_tiles_prepare_pt: NULL plan");
    bool fixed = false;
    return cm2::fx_plan(t, as_stream(stream_), &fixed);
}

extern "C" int cm2_tiles_set_pt_order(cm2_tiles *t, int fixed)
{
    CM2_CHECK(t, "cm2_tiles_set_pt_order: NULL argument");
    t->pt_fixed = fixed == 2 ? 2 : (fixed ? 1 : 0);
    return 0;
}

// Tile indices bounding `ngroups` consecutive groups of tiles whose PIXEL boundaries are the same on
// every rank of a sharded run (ranks with different hit maps may have cut their tiles differently):
// group g = tiles [h_tiles[g], h_tiles[g + 1]).  Up to 8 groups are bounded by policy::shared_cuts, the
// uniform tiling's boundaries nearest to eighths of the map.
extern "C" int cm2_tiles_group_tiles(const cm2_tiles *t, int ngroups, int64_t *h_tiles)
{
    CM2_CHECK(t && h_tiles && ngroups >= 1, "cm2_tiles_group_tiles: bad argument");
    const std::vector<int64_t> eighths = policy::shared_cuts(t->npix, t->tp);
    for (int g = 0; g <= ngroups; ++g) {
        int64_t pixel;
        if (ngroups > 8) {                     // finer than eighths: only a uniform tiling has the cuts
            CM2_CHECK(!t->balanced, "cm2_tiles_group_tiles: at most 8 groups on a balanced tiling");
            pixel = ((t->npix + t->tp - 1) / t->tp * g / ngroups) * t->tp;
            if (pixel > t->npix || g == ngroups) pixel = t->npix;
        } else {
            pixel = eighths[(size_t)((8 * g) / ngroups)];
        }
        // the tile that starts at `pixel` (every tiling has a boundary there)
        int64_t lo = 0, hi = t->ntiles;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (t->tile_p0[(size_t)mid] < pixel) lo = mid + 1; else hi = mid;
        }
        CM2_CHECK(t->tile_p0[(size_t)lo] == pixel, "cm2_tiles_group_tiles: no tile boundary at pixel %lld",
                  (long long)pixel);
        h_tiles[g] = lo;
    }
    return 0;
}

extern "C" int cm2_tiles_pixel_range(const cm2_tiles *t, int64_t tile_lo, int64_t tile_hi,
                                     int64_t *h_p0p1)
{
    CM2_CHECK(t && h_p0p1, "cm2_tiles_pixel_range: NULL argument");
    CM2_CHECK(tile_lo >= 0 && tile_lo <= tile_hi && tile_hi <= t->ntiles,
              "cm2_tiles_pixel_range: tiles [%lld, %lld) outside [0, %lld]", (long long)tile_lo,
              (long long)tile_hi, (long long)t->ntiles);
    h_p0p1[0] = t->tile_p0[(size_t)tile_lo];
    h_p0p1[1] = t->tile_p0[(size_t)tile_hi];
    return 0;
}

extern "C" int cm2_P_tiles_apply(const cm2_tiles *t, const double *d_x, double *d_tod_tb,
                                 void *stream_)
{
    CM2_CHECK(t && d_x && (d_tod_tb || t->nvalid == 0), "cm2_P_tiles_apply: NULL argument");
    if (t->nitems == 0) return 0;
    hipStream_t stream = as_stream(stream_);
    const size_t lds = sizeof(double) * t->tp * t->pol;
    return with_pol_half(t, [&](auto pol_c, auto half_c) -> int {
        constexpr int POL = decltype(pol_c)::value;
        constexpr bool HALF = decltype(half_c)::value;
        k_P_tiles<POL, HALF><<<(int)t->nitems, kPBlock, lds, stream>>>(
            t->d_tile_p0, t->d_item_tile, t->d_item_k0, t->d_item_k1, t->d_pl,
            HALF ? t->d_half : t->d_cos, t->d_sin, d_x, d_tod_tb);
        CM2_LAUNCH_OK();
        return 0;
    });
}

// the atomic P^T of the work items [i0, i1)
static int pt_tiles_atomic(const cm2_tiles *t, int64_t i0, int64_t i1, const double *d_tod_tb, double *d_out,
                           hipStream_t stream)
{
    const size_t lds = sizeof(double) * t->tp * t->pol;
    return with_pol_half(t, [&](auto pol_c, auto half_c) -> int {
        constexpr int POL = decltype(pol_c)::value;
        constexpr bool HALF = decltype(half_c)::value;
        k_Pt_tiles<POL, HALF><<<(int)(i1 - i0), kPtBlock, lds, stream>>>(
            t->d_tile_p0, t->d_item_tile + i0, t->d_item_k0 + i0, t->d_item_k1 + i0, t->d_pl,
            HALF ? t->d_half : t->d_cos, t->d_sin, d_tod_tb, d_out);
        CM2_LAUNCH_OK();
        return 0;
    });
}

extern "C" int cm2_Pt_tiles_apply(const cm2_tiles *t, const double *d_tod_tb, double *d_out,
                                  void *stream_)
{
    CM2_CHECK(t && d_out && (d_tod_tb || t->nvalid == 0), "cm2_Pt_tiles_apply: NULL argument");
    hipStream_t stream = as_stream(stream_);
    bool fixed = false;
    if (int rc = cm2::fx_plan(t, stream, &fixed)) return rc;
    if (fixed) return cm2::fx_launch(t, d_tod_tb, d_out, 0, t->ntiles, stream);
    CM2_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * t->npix * t->pol, stream));
    if (t->nitems == 0) return 0;
    return pt_tiles_atomic(t, 0, t->nitems, d_tod_tb, d_out, stream);
}

extern "C" int cm2_Pt_tiles_apply_range(const cm2_tiles *t, const double *d_tod_tb, double *d_out,
                                        int64_t tile_lo, int64_t tile_hi, void *stream_)
{
    CM2_CHECK(t && d_out && (d_tod_tb || t->nvalid == 0), "cm2_Pt_tiles_apply_range: NULL argument");
    CM2_CHECK(tile_lo >= 0 && tile_lo <= tile_hi && tile_hi <= t->ntiles,
              "cm2_Pt_tiles_apply_range: tiles [%lld, %lld) outside [0, %lld]", (long long)tile_lo,
              (long long)tile_hi, (long long)t->ntiles);
    if (tile_lo == tile_hi) return 0;
    hipStream_t stream = as_stream(stream_);
    bool fixed = false;
    if (int rc = cm2::fx_plan(t, stream, &fixed)) return rc;
    if (fixed) return cm2::fx_launch(t, d_tod_tb, d_out, tile_lo, tile_hi, stream);
    const int64_t p0 = t->tile_p0[(size_t)tile_lo], p1 = t->tile_p0[(size_t)tile_hi];
    CM2_HIP(hipMemsetAsync(d_out + p0 * t->pol, 0, sizeof(double) * (p1 - p0) * t->pol, stream));
    const int64_t i0 = t->tile_item0[(size_t)tile_lo], i1 = t->tile_item0[(size_t)tile_hi];
    if (i1 == i0) return 0;
    return pt_tiles_atomic(t, i0, i1, d_tod_tb, d_out, stream);
}

__global__ __launch_bounds__(256) void k_i32_time_to_tiles(int64_t nt,
                                                            const uint32_t *__restrict__ tb_dst,
                                                            const int32_t *__restrict__ in,
                                                            int32_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride) {
        const uint32_t k = tb_dst[t];
        if (k != kInvalidSample) out[k] = in[t];
    }
}

extern "C" int cm2_i32_time_to_tiles(const cm2_tiles *t, const int32_t *d_time, int32_t *d_tb,
                                     void *stream_)
{
    CM2_CHECK(t && (t->nt == 0 || (d_time && d_tb)), "cm2_i32_time_to_tiles: NULL argument");
    if (t->nt == 0) return 0;
    k_i32_time_to_tiles<<<grid_for(t->nt), kBlock, 0, as_stream(stream_)>>>(t->nt, t->d_tb_dst, d_time,
                                                                          d_tb);
    CM2_LAUNCH_OK();
    return 0;
}

static inline void perm_geometry(int64_t nt, int &blocks, int64_t &chunk)
{
    // one 1024-thread workgroup per CU-slot, each with a contiguous time range
    blocks = kNumCU * 2;
    chunk = (nt + blocks - 1) / blocks;
    chunk = ((chunk + 1023) / 1024) * 1024;
    blocks = (int)((nt + chunk - 1) / chunk);
    if (blocks < 1) blocks = 1;
}

// the one builder of window lists (cm2_tiles.h): keys by the caller's kernel, a radix sort over the window bits and
// the 32 address bits, the low words unpacked
int cm2::window_lists(int64_t nwin, hipStream_t st,
                      const std::function<void(uint64_t *keys, uint16_t *vals)> &fill_keys, uint32_t **lst_k,
                      uint16_t **lst_q)
{
    const int64_t total = nwin * kPermWin;
    DevTemp<uint64_t> keys_in, keys_out;
    DevTemp<uint16_t> vals_in, lq;
    DevTemp<uint32_t> lk;
    DevTemp<char> d_temp;
    CM2_HIP(keys_in.alloc(total));
    CM2_HIP(keys_out.alloc(total));
    CM2_HIP(vals_in.alloc(total));
    CM2_HIP(lk.alloc(total));
    CM2_HIP(lq.alloc(total));
    fill_keys(keys_in, vals_in);
    CM2_LAUNCH_OK();
    int end_bit = 33;
    while (((int64_t)1 << (end_bit - 32)) <= nwin && end_bit < 64) ++end_bit;
    size_t tb = 0;
    CM2_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in.p, keys_out.p, vals_in.p, lq.p, total, 0,
                                               end_bit, st));
    CM2_HIP(d_temp.alloc(tb + 16));
    CM2_HIP(hipcub::DeviceRadixSort::SortPairs(d_temp.p, tb, keys_in.p, keys_out.p, vals_in.p, lq.p, total, 0,
                                               end_bit, st));
    k_perm_unpack<<<grid_for(total), kBlock, 0, st>>>(total, keys_out, lk);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(st));
    *lst_k = lk.keep();
    *lst_q = lq.keep();
    return 0;
}

int cm2::first_flag_mismatch(hipStream_t st, const std::function<void(uint32_t *d_first)> &launch_compare,
                             uint32_t *first)
{
    DevTemp<uint32_t> d_first;
    CM2_HIP(d_first.alloc(1));
    CM2_HIP(hipMemsetAsync(d_first.p, 0xFF, sizeof(uint32_t), st));
    launch_compare(d_first);
    CM2_LAUNCH_OK();
    CM2_HIP(cm2::download(first, d_first.p, sizeof(*first), st));
    return 0;
}

// lists of the windowed permutations (a TOD shorter than one window keeps the per-sample kernels)
int cm2::perm_lists(const cm2_tiles *tc, hipStream_t st, bool *use)
{
    cm2_tiles *t = const_cast<cm2_tiles *>(tc);         // lazily built cache
    *use = false;
    if (t->nt < kPermWin) return 0;
    if (!t->d_perm_k) {
        const int64_t nwin = (t->nt + kPermWin - 1) / kPermWin;
        auto keys = [&](uint64_t *k, uint16_t *v) {
            k_perm_keys<<<grid_for(nwin * kPermWin), kBlock, 0, st>>>(t->nt, nwin, t->d_tb_dst, k, v);
        };
        if (int rc = window_lists(nwin, st, keys, &t->d_perm_k, &t->d_perm_q)) return rc;
        t->nperm_win = nwin;
    }
    *use = true;
    return 0;
}

extern "C" int cm2_tod_time_to_tiles(const cm2_tiles *t, const double *d_time, double *d_tb,
                                     void *stream_)
{
    CM2_CHECK(t && d_time && d_tb, "cm2_tod_time_to_tiles: NULL argument");
    bool windows = false;
    if (int rc = perm_lists(t, as_stream(stream_), &windows)) return rc;
    if (windows) {
        k_perm_windows<false><<<window_grid(t->nperm_win), kPermT, 0, as_stream(stream_)>>>(
            t->nt, t->nperm_win, t->d_perm_k, t->d_perm_q, d_time, d_tb);
        CM2_LAUNCH_OK();
        return 0;
    }
    int blocks;
    int64_t chunk;
    perm_geometry(t->nt, blocks, chunk);
    k_time_to_tiles<<<blocks, 1024, 0, as_stream(stream_)>>>(t->nt, chunk, t->d_tb_dst, d_time, d_tb);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_tod_tiles_to_time(const cm2_tiles *t, const double *d_tb, double *d_time,
                                     void *stream_)
{
    CM2_CHECK(t && d_time && d_tb, "cm2_tod_tiles_to_time: NULL argument");
    bool windows = false;
    if (int rc = perm_lists(t, as_stream(stream_), &windows)) return rc;
    if (windows) {
        k_perm_windows<true><<<window_grid(t->nperm_win), kPermT, 0, as_stream(stream_)>>>(
            t->nt, t->nperm_win, t->d_perm_k, t->d_perm_q, d_tb, d_time);
        CM2_LAUNCH_OK();
        return 0;
    }
    int blocks;
    int64_t chunk;
    perm_geometry(t->nt, blocks, chunk);
    k_tiles_to_time<<<blocks, 1024, 0, as_stream(stream_)>>>(t->nt, chunk, t->d_tb_dst, d_tb, d_time);
    CM2_LAUNCH_OK();
    return 0;
}
