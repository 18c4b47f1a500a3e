// cm2_os_lists.hip -- plan-time side of the overlap-save N^-1 (cm2_overlap_save.hip): the address lists through
// which k_os_real reaches a window's samples in a tile-bucketed order, in the three formats described there, written
// straight from the tile plan's offsets or from a segmented sort.  Integer kernels only.
#include "cm2_os_lists.h"

#include <hipcub/hipcub.hpp>

using namespace cm2;

namespace {

// ---- plan-time kernels ----------------------------------------------------------------------------
// entries of the lists of windows [w0, w0 + nw), PER per window, in the order they are stored:
//   list 0 / 1: window positions [0, N) / [N, 2N)        -> value = position within the half
//   list 2 (3): results [0, RLEN) ([RLEN, 2 RLEN))       -> value = position within the round
// key = address in the tile order (0xFFFFFFFF: no sample); a segmented sort then orders every list
// by address.
__global__ __launch_bounds__(256) void k_real_keys(const WinDesc *__restrict__ wins, int64_t w0, int64_t nw,
                                                   const uint32_t *__restrict__ idx, uint32_t *__restrict__ keys,
                                                   uint16_t *__restrict__ vals)
{
    const int64_t total = nw * os::PER;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const int64_t p = g / os::PER;
        const int e = (int)(g - p * os::PER);
        const WinDesc wd = wins[w0 + p];
        uint32_t k = kInvalidSample;
        int val;
        if (e < 2 * os::N) {
            val = e & (os::N - 1);
            const int64_t ts = wd.start - kHalo + e;
            if (ts >= wd.lo && ts < wd.hi) k = idx[ts];
        } else {
            const int o = e - 2 * os::N;
            val = o % os::RLEN;
            if (o < wd.len) k = idx[wd.start + o];
        }
        keys[g] = k;
        vals[g] = (uint16_t)(val | (k == kInvalidSample ? 0x8000 : 0));   // bit 15: no sample
    }
}

struct RealListOffset {
    int end;
    __host__ __device__ int operator()(int s) const
    {
        const int l = s % os::NLIST + end;
        return (s / os::NLIST) * os::PER + (l == os::NLIST ? os::PER : os::list_off(l));
    }
};

// run structure of one sorted list per workgroup: a run starts where the address is not the
// previous address + 1.  One pass over the list in pieces of 256 consecutive entries (coalesced):
// the 16-bit words get their run-start bit, the run table delta[r] = address - slot and the header
// are written.  A list has at most one run per pixel tile (a window's samples in a tile are
// consecutive addresses, and two adjacent tiles' runs can only merge), so the table stride is
// known from the tile count and no counting pass is needed; *max_runs receives the largest count.
__global__ __launch_bounds__(256) void k_real_rc(int64_t nlists, const uint32_t *__restrict__ lk, uint16_t *__restrict__ lq,
                                                 ListHdr *__restrict__ hdrs, uint32_t *__restrict__ tabs, int rmax,
                                                 uint32_t *__restrict__ max_runs)
{
    __shared__ int wsum[4], vsum[4];
    const int64_t lid = blockIdx.x;
    if (lid >= nlists) return;
    const int l = (int)(lid % os::NLIST);
    const int64_t win = lid / os::NLIST;
    const int64_t e0 = win * os::PER + os::list_off(l);
    const int len = os::list_len(l);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int runs = 0, nvalid = 0;                          // in front of the current piece (uniform)
    for (int s0 = 0; s0 < len; s0 += 256) {
        const int s = s0 + t;
        const uint32_t k = lk[e0 + s];
        const uint32_t prev = s > 0 ? lk[e0 + s - 1] : kInvalidSample;
        const bool valid = k != kInvalidSample;
        const bool flag = valid && (s == 0 || k != prev + 1u);
        const uint64_t fm = __ballot(flag), vm = __ballot(valid);
        const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
        if (lane == 0) { wsum[wave] = __popcll(fm); vsum[wave] = __popcll(vm); }
        __syncthreads();
        int wbase = 0, tot = 0, vtot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) wbase += wsum[w];
            tot += wsum[w];
            vtot += vsum[w];
        }
        __syncthreads();
        const int r = runs + wbase + below + (flag ? 1 : 0) - 1;     // run of this entry (-1: none yet)
        if (flag) {
            if (r < rmax) tabs[lid * rmax + r] = k - (uint32_t)s;
        }
        const uint16_t q = lq[e0 + s];
        lq[e0 + s] = (uint16_t)((q & 0x7FFFu) | (flag ? 0x8000u : 0u));
        // run index in front of each wave's first slot (waves own len / 4 consecutive slots)
        if (s % (len / 4) == 0) hdrs[lid].wbase[s / (len / 4)] = flag ? r - 1 : r;
        runs += tot;
        nvalid += vtot;
    }
    if (t == 0) {
        hdrs[lid].nvalid = (uint32_t)nvalid;
        hdrs[lid].nruns = (uint32_t)runs;
        atomicMax(max_runs, (uint32_t)runs);
    }
}

// the 16-bit words of every list from slot order (what the segmented sort and k_real_rc leave) to
// the stored order q_index: one workgroup per list, through LDS
__global__ __launch_bounds__(256) void k_real_qperm(int64_t nlists, uint16_t *__restrict__ lq)
{
    __shared__ uint16_t stage[os::N];
    const int64_t lid = blockIdx.x;
    if (lid >= nlists) return;
    const int l = (int)(lid % os::NLIST);
    const int64_t e0 = (lid / os::NLIST) * os::PER + os::list_off(l);
    const int len = os::list_len(l), E = len / 256;
    for (int s = threadIdx.x; s < len; s += 256) stage[q_index(s, E)] = lq[e0 + s];
    __syncthreads();
    uint32_t *dst = reinterpret_cast<uint32_t *>(lq + e0);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(stage);
    for (int i = threadIdx.x; i < len / 2; i += 256) dst[i] = src[i];
}

// ---- the lists without a sort ------------------------------------------------------------------
// The tile order is a STABLE partition of the time samples by pixel tile: the samples of one tile
// that fall into any contiguous time range have consecutive addresses, in time order.  A list
// sorted by address is therefore: tiles ascending, inside a tile address - (lowest address of the
// tile in this list).  One workgroup per list: count and lowest address per tile with LDS atomics
// (integer add / min: the result does not depend on their order), a scan over the tiles, then
//   slot(entry) = base[tile] + address - lowest[tile]
// and the entries without a sample behind the valid ones in list order.  The run table falls out
// of the same numbers: every tile with samples starts a run, delta = lowest[tile] - base[tile].
// (k_real_rc merges the runs of two adjacent tiles when their addresses happen to be contiguous;
// this kernel does not: at most one run per tile either way.)
// RC: bit 15 of a word = run start, headers and run tables written; otherwise bit 15 = no sample
// and the addresses go to lk (plain lists).
template <bool RC>
__global__ __launch_bounds__(256) void k_real_lists(const WinDesc *__restrict__ wins, int64_t nlists,
                                                    const uint32_t *__restrict__ idx, const int64_t *__restrict__ tile_off,
                                                    int ntiles, uint16_t *__restrict__ lq, uint32_t *__restrict__ lk,
                                                    ListHdr *__restrict__ hdrs, uint32_t *__restrict__ tabs, int rmax,
                                                    uint32_t *__restrict__ max_runs)
{
    constexpr int E = os::N / 256;                        // rows of 64 entries a wave handles at most
    extern __shared__ uint32_t sm_l[];
    uint32_t *toff = sm_l;                               // [ntiles + 1] first address of every tile
    uint32_t *cnt = toff + ntiles + 1;                   // [ntiles] entries, then: base slot
    uint32_t *mn = cnt + ntiles;                         // [ntiles] lowest address
    uint32_t *ridx = mn + ntiles;                        // [ntiles] run index of the tile
    uint32_t *misc = ridx + ntiles;                      // [4] waves' scan sums, [4] entries without sample, [4] wbase counts
    uint16_t *stage = reinterpret_cast<uint16_t *>(misc + 12);   // [len] the list's 16-bit words
    const int64_t lid = blockIdx.x;
    if (lid >= nlists) return;
    const int l = (int)(lid % os::NLIST);
    const int64_t win = lid / os::NLIST;
    const int64_t e0 = win * os::PER + os::list_off(l);
    const int len = os::list_len(l), quarter = len / 4, rows = quarter / 64;
    const WinDesc wd = wins[win];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int b = t; b <= ntiles; b += 256) toff[b] = (uint32_t)tile_off[b];
    for (int b = t; b < ntiles; b += 256) {
        cnt[b] = 0;
        mn[b] = 0xFFFFFFFFu;
    }
    if (t < 12) misc[t] = 0;
    __syncthreads();
    // ---- pass 1: addresses, tiles, counts ----
    uint32_t a[E];
    uint16_t tl[E];
    int ninv = 0;                                        // entries without a sample of this wave so far
    uint32_t inv_rank[E / 2];                            // (two 16-bit ranks a word)
#pragma unroll
    for (int i = 0; i < E; ++i) {
        a[i] = kInvalidSample;
        tl[i] = 0;
        if (i < rows) {
            const int e = wave * quarter + 64 * i + lane;
            if (l < 2) {
                const int64_t ts = wd.start - kHalo + (int64_t)l * os::N + e;
                if (ts >= wd.lo && ts < wd.hi) a[i] = idx[ts];
            } else {
                const int64_t o = (int64_t)(l - 2) * os::RLEN + e;
                if (o < wd.len) a[i] = idx[wd.start + o];
            }
            const bool valid = a[i] != kInvalidSample;
            if (valid) {
                int lo = 0, hi = ntiles;                 // largest b with toff[b] <= a
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (toff[mid] <= a[i]) lo = mid; else hi = mid;
                }
                tl[i] = (uint16_t)lo;
                atomicAdd(&cnt[lo], 1u);
                atomicMin(&mn[lo], a[i]);
            }
            const uint64_t im = __ballot(!valid);
            const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(im >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)im, 0u));
            const uint32_t r = (uint32_t)(ninv + below);
            if (i & 1) inv_rank[i / 2] |= r << 16; else inv_rank[i / 2] = r;
            ninv += __popcll(im);
        }
    }
    if (lane == 0) misc[4 + wave] = (uint32_t)ninv;
    __syncthreads();
    // ---- scan over the tiles: base slot and run index (packed: runs << 16 | entries) ----
    const int per = (ntiles + 255) / 256;
    uint32_t mine = 0;
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) mine += cnt[b] | (cnt[b] ? 0x10000u : 0u);
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) misc[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += misc[w];
        total += misc[w];
    }
    const int nvalid = (int)(total & 0xFFFFu), nruns = (int)(total >> 16);
    // (len <= 8192 entries and at most 2^15 tiles: both halves of the packed word are exact)
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) {
        const uint32_t c = cnt[b];
        const uint32_t base = before & 0xFFFFu, r = before >> 16;
        cnt[b] = base;
        ridx[b] = r;
        if (c) {
            if (RC) {
                if ((int)r < rmax) tabs[lid * rmax + r] = mn[b] - base;
#pragma unroll
                for (int w = 1; w < 4; ++w)
                    if ((int)base < w * quarter) atomicAdd(&misc[8 + w], 1u);
            }
            before += c | 0x10000u;
        }
    }
    int inv_before = nvalid;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) inv_before += (int)misc[4 + w];
    __syncthreads();
    // ---- pass 2: every entry to its slot ----
#pragma unroll
    for (int i = 0; i < E; ++i) {
        if (i < rows) {
            const int e = wave * quarter + 64 * i + lane;
            const bool valid = a[i] != kInvalidSample;
            int slot;
            uint16_t word = (uint16_t)e;
            if (valid) {
                const uint32_t low = mn[tl[i]];
                slot = (int)(cnt[tl[i]] + (a[i] - low));
                if (RC && a[i] == low) word |= 0x8000u;
            } else {
                slot = inv_before + (int)((inv_rank[i / 2] >> (16 * (i & 1))) & 0xFFFFu);
                if (!RC) word |= 0x8000u;
            }
            stage[q_index(slot, len / 256)] = word;
            if (!RC) lk[e0 + slot] = a[i];
        }
    }
    if (RC && t == 0) {
        ListHdr h;
        h.nvalid = (uint32_t)nvalid;
        h.nruns = (uint32_t)nruns;
        h.wbase[0] = -1;
        for (int w = 1; w < 4; ++w) h.wbase[w] = (int32_t)misc[8 + w] - 1;
        hdrs[lid] = h;
        atomicMax(max_runs, (uint32_t)nruns);
    }
    __syncthreads();
    uint32_t *dst = reinterpret_cast<uint32_t *>(lq + e0);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(stage);
    for (int i = t; i < len / 2; i += 256) dst[i] = src[i];
}

// ---- inverse lists (MODE 3 of k_os_real) ---------------------------------------------------------
// One workgroup per list (l = 0: the 2N window positions, l = 1: the HOP result positions).  Same
// arithmetic as k_real_lists over the whole (result) window: per-tile count and lowest address, scan,
// slot = base[tile] + address - lowest[tile].  Written: what cm2_overlap_save.hip describes under "inverse
// lists", and the run index in front of every wave's slots of every round.
__global__ __launch_bounds__(256) void k_real_ilists(const WinDesc *__restrict__ wins, int64_t nlists,
                                                     const uint32_t *__restrict__ idx, const int64_t *__restrict__ tile_off,
                                                     int ntiles, uint16_t *__restrict__ plist, uint32_t *__restrict__ flags,
                                                     IListHdr *__restrict__ hdrs, uint32_t *__restrict__ tabs, int rmax,
                                                     uint32_t *__restrict__ max_runs, int threads)
{
    // threads: workgroup size of the kernel that will read the lists (256: k_os_real, 512: k_os_wide);
    // it fixes the slot order of a round (slot = 64 (E wave + u) + lane, E = round / threads)
    constexpr int EMAX = 2 * os::N / 256;
    extern __shared__ uint32_t sm_i[];
    uint32_t *toff = sm_i;                               // [ntiles + 1]
    uint32_t *cnt = toff + ntiles + 1;                   // [ntiles] entries, then: base slot
    uint32_t *mn = cnt + ntiles;                         // [ntiles] lowest address
    uint32_t *misc = mn + ntiles;                        // [4] scan sums, [16] wbase counts
    uint32_t *fl = misc + 20;                            // [2 threads] run-start bits
    const int64_t lid = blockIdx.x;
    if (lid >= nlists) return;
    const int l = (int)(lid & 1);
    const int64_t win = lid >> 1;
    const int64_t e0 = win * os::PER + (l ? 2 * os::N : 0);
    const int len = l ? os::HOP : 2 * os::N;               // positions
    const int RL = l ? os::RLEN : os::N;                   // slots a round
    const int rounds = l ? os::RR : 2, rows = len / 256, E = RL / threads, nw = threads / 64;
    const WinDesc wd = wins[win];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int b = t; b <= ntiles; b += 256) toff[b] = (uint32_t)tile_off[b];
    for (int b = t; b < ntiles; b += 256) {
        cnt[b] = 0;
        mn[b] = 0xFFFFFFFFu;
    }
    if (t < 20) misc[t] = 0;
    for (int i = t; i < 2 * threads; i += 256) fl[i] = 0;
    __syncthreads();
    uint32_t a[EMAX];
    uint16_t tl[EMAX];
#pragma unroll
    for (int i = 0; i < EMAX; ++i) {
        a[i] = kInvalidSample;
        tl[i] = 0;
        if (i < rows) {
            const int e = 256 * i + t;
            if (l == 0) {
                const int64_t ts = wd.start - kHalo + e;
                if (ts >= wd.lo && ts < wd.hi) a[i] = idx[ts];
            } else {
                if (e < wd.len) a[i] = idx[wd.start + e];
            }
            if (a[i] != kInvalidSample) {
                int lo = 0, hi = ntiles;                 // largest b with toff[b] <= a
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (toff[mid] <= a[i]) lo = mid; else hi = mid;
                }
                tl[i] = (uint16_t)lo;
                atomicAdd(&cnt[lo], 1u);
                atomicMin(&mn[lo], a[i]);
            }
        }
    }
    __syncthreads();
    // scan over the tiles: base slot and run index (packed: runs << 16 | entries)
    const int per = (ntiles + 255) / 256;
    uint32_t mine = 0;
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) mine += cnt[b] | (cnt[b] ? 0x10000u : 0u);
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) misc[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += misc[w];
        total += misc[w];
    }
    const int nvalid = (int)(total & 0xFFFFu), nruns = (int)(total >> 16);
    for (int b = t * per; b < (t + 1) * per && b < ntiles; ++b) {
        const uint32_t c = cnt[b];
        const uint32_t base = before & 0xFFFFu, r = before >> 16;
        cnt[b] = base;
        if (c) {
            if ((int)r < rmax) tabs[lid * rmax + r] = mn[b] - base;
            // the run's first slot: round, then (wave, row, lane) of the kernel's slot order
            const int j = (int)base / RL, sr = (int)base % RL;
            const int wv = sr / (64 * E), rem = sr % (64 * E);
            atomicOr(&fl[threads * j + 64 * wv + (rem & 63)], 1u << (rem >> 6));
            for (int jj = 0; jj < rounds; ++jj)
                for (int w = 0; w < nw; ++w)
                    if ((int)base < jj * RL + w * (RL / nw)) atomicAdd(&misc[4 + nw * jj + w], 1u);
            before += c | 0x10000u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EMAX; ++i)
        if (i < rows) {
            const int e = 256 * i + t;
            uint16_t slot = 0xFFFFu;
            if (a[i] != kInvalidSample) slot = (uint16_t)(cnt[tl[i]] + (a[i] - mn[tl[i]]));
            plist[e0 + e] = slot;
        }
    for (int i = t; i < 2 * threads; i += 256) flags[lid * 2 * threads + i] = fl[i];
    if (t == 0) {
        IListHdr h;
        h.nvalid = (uint32_t)nvalid;
        h.nruns = (uint32_t)nruns;
        for (int k = 0; k < 16; ++k) h.wbase[k] = (int32_t)misc[4 + k] - 1;
        hdrs[lid] = h;
        atomicMax(max_runs, (uint32_t)nruns);
    }
}

}  // namespace

namespace cm2 {

// Zeroes the counter in which a builder's kernel gathers the largest run count of a list (atomicMax).
static int runs_begin(DevTemp<uint32_t> &d_max, hipStream_t stream)
{
    CM2_HIP(d_max.alloc(1));
    CM2_HIP(hipMemsetAsync(d_max.p, 0, sizeof(uint32_t), stream));
    return 0;
}
// Behind a builder's launch: reads that counter back (waits for the stream) and checks it against the table stride.
// `ls` then holds run-coded (mode 2) or inverse (3) lists: `nl` a window, each with `hdr` bytes of header and flags.
static int runs_end(const DevTemp<uint32_t> &d_max, OsLists *ls, int mode, int rmax, int nl, double hdr,
                    hipStream_t stream)
{
    uint32_t h_max = 0;
    CM2_HIP(cm2::download(&h_max, d_max.p, sizeof(uint32_t), stream));
    CM2_HIP(hipStreamSynchronize(stream));
    CM2_CHECK((int)h_max <= rmax, "fused overlap-save: a list has %u address runs, more than the %d pixel "
              "tiles allow", h_max, rmax);
    ls->rmax = rmax;
    ls->mode = mode;
    ls->bytes_per_window = 2.0 * os::PER + nl * (hdr + 4.0 * h_max);
    return 0;
}

// The lists straight from the tile plan's offsets (k_real_lists): no keys, no sort, no temporaries.
static int lists_direct(const os::WinDesc *d_wins, int64_t nwin, OsLists *ls, const OsPlanView &pv, bool rc, int rmax,
                        hipStream_t stream)
{
    const int64_t total = nwin * os::PER;
    const int64_t nlists = nwin * os::NLIST;
    CM2_HIP(cm2::dev_malloc(&ls->d_lst_q, sizeof(uint16_t) * total));
    const size_t lds = sizeof(uint32_t) * (size_t)(4 * pv.ntiles + 1 + 12) + sizeof(uint16_t) * (size_t)os::N;
    static size_t granted[64] = {0};
    DevTemp<uint32_t> d_max;
    if (int e = runs_begin(d_max, stream)) return e;
    if (rc) {
        CM2_HIP(cm2::dev_malloc(&ls->d_hdrs, sizeof(ListHdr) * nlists));
        CM2_HIP(cm2::dev_malloc(&ls->d_tabs, sizeof(uint32_t) * nlists * rmax));
    } else {
        CM2_HIP(cm2::dev_malloc(&ls->d_lst_k, sizeof(uint32_t) * total));
    }
    const auto kernel = rc ? k_real_lists<true> : k_real_lists<false>;      // (what a format does not have stays NULL)
    CM2_HIP(ensure_dynamic_lds((const void *)kernel, lds, granted));
    kernel<<<(unsigned)nlists, 256, lds, stream>>>(d_wins, nlists, pv.d_idx, pv.d_tile_off, (int)pv.ntiles, ls->d_lst_q,
                                                   ls->d_lst_k, ls->d_hdrs, ls->d_tabs, rmax, d_max);
    CM2_LAUNCH_OK();
    if (rc) return runs_end(d_max, ls, 2, rmax, os::NLIST, sizeof(ListHdr), stream);
    CM2_HIP(hipStreamSynchronize(stream));
    ls->mode = 1;
    ls->bytes_per_window = 6.0 * os::PER;
    return 0;
}

// Inverse lists (k_real_ilists): needs the tile offsets and run tables that fit LDS.
static int lists_inverse(const os::WinDesc *d_wins, int64_t nwin, OsLists *ls, const OsPlanView &pv, int rmax,
                         hipStream_t stream)
{
    const int64_t total = nwin * os::PER;
    const int64_t nlists = nwin * 2;
    CM2_HIP(cm2::dev_malloc(&ls->d_lst_q, sizeof(uint16_t) * total));
    CM2_HIP(cm2::dev_malloc(&ls->d_ihdrs, sizeof(IListHdr) * nlists));
    CM2_HIP(cm2::dev_malloc(&ls->d_iflags, sizeof(uint32_t) * nlists * 2 * kT));
    CM2_HIP(cm2::dev_malloc(&ls->d_tabs, sizeof(uint32_t) * nlists * rmax));
    DevTemp<uint32_t> d_max;
    if (int e = runs_begin(d_max, stream)) return e;
    const size_t lds = sizeof(uint32_t) * (size_t)(3 * pv.ntiles + 1 + 20 + 2 * kT);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds((const void *)k_real_ilists, lds, granted));
    k_real_ilists<<<(unsigned)nlists, 256, lds, stream>>>(d_wins, nlists, pv.d_idx, pv.d_tile_off, (int)pv.ntiles,
                                                          ls->d_lst_q, ls->d_iflags, ls->d_ihdrs, ls->d_tabs, rmax, d_max, kT);
    CM2_LAUNCH_OK();
    return runs_end(d_max, ls, 3, rmax, 2, sizeof(IListHdr) + 2048.0, stream);
}

// The lists from a segmented sort of (address, position) pairs: needs nothing but the index
// (CM2_OS_LIST_BUILD=sort, a plan without tile offsets, or more tiles than the direct builders keep in
// LDS).  rc: run-coded lists with tables of rmax words (one run per pixel tile at most: k_real_rc).
static int lists_sorted(const os::WinDesc *d_wins, int64_t nwin, OsLists *ls, const OsPlanView &pv, bool rc, int rmax,
                        int64_t sort_chunk_windows, hipStream_t stream)
{
    const int64_t total = nwin * os::PER;
    CM2_HIP(cm2::dev_malloc(&ls->d_lst_k, sizeof(uint32_t) * total));
    CM2_HIP(cm2::dev_malloc(&ls->d_lst_q, sizeof(uint16_t) * total));
    int64_t chunk_w = ((int64_t)1 << 30) / os::PER;             // hipCUB counts items in int
    if (sort_chunk_windows > 0 && sort_chunk_windows < chunk_w) chunk_w = sort_chunk_windows;
    const int64_t cw_max = nwin < chunk_w ? nwin : chunk_w;
    {
        DevTemp<uint32_t> keys_in;
        DevTemp<uint16_t> vals_in;
        DevTemp<char> d_temp;
        CM2_HIP(keys_in.alloc(cw_max * os::PER));
        CM2_HIP(vals_in.alloc(cw_max * os::PER));
        hipcub::CountingInputIterator<int> seg_id(0);
        using OffsetIt = hipcub::TransformInputIterator<int, RealListOffset, hipcub::CountingInputIterator<int>>;
        OffsetIt seg_begin(seg_id, RealListOffset{0}), seg_end(seg_id, RealListOffset{1});
        size_t tb = 0;
        CM2_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(
            nullptr, tb, keys_in.p, ls->d_lst_k, vals_in.p, ls->d_lst_q, (int)(cw_max * os::PER),
            (int)(os::NLIST * cw_max), seg_begin, seg_end, 0, 32, stream));
        CM2_HIP(d_temp.alloc(tb + 16));
        for (int64_t p0 = 0; p0 < nwin; p0 += chunk_w) {
            const int64_t nw = nwin - p0 < chunk_w ? nwin - p0 : chunk_w;
            k_real_keys<<<grid_for(nw * os::PER), kBlock, 0, stream>>>(d_wins, p0, nw, pv.d_idx, keys_in, vals_in);
            CM2_LAUNCH_OK();
            size_t tbc = tb;
            CM2_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(
                d_temp.p, tbc, keys_in.p, ls->d_lst_k + p0 * os::PER, vals_in.p, ls->d_lst_q + p0 * os::PER,
                (int)(nw * os::PER), (int)(os::NLIST * nw), seg_begin, seg_end, 0, 32, stream));
        }
        CM2_HIP(hipStreamSynchronize(stream));
    }
    ls->mode = 1;
    ls->bytes_per_window = 6.0 * os::PER;
    const int64_t nlists = nwin * os::NLIST;
    if (rc) {
        DevTemp<uint32_t> d_max;
        if (int e = runs_begin(d_max, stream)) return e;
        CM2_HIP(cm2::dev_malloc(&ls->d_hdrs, sizeof(ListHdr) * nlists));
        CM2_HIP(cm2::dev_malloc(&ls->d_tabs, sizeof(uint32_t) * nlists * rmax));
        k_real_rc<<<(unsigned)nlists, 256, 0, stream>>>(nlists, ls->d_lst_k, ls->d_lst_q, ls->d_hdrs, ls->d_tabs, rmax, d_max);
        CM2_LAUNCH_OK();
        if (int e = runs_end(d_max, ls, 2, rmax, os::NLIST, sizeof(ListHdr), stream)) return e;
        (void)cm2::dev_free(ls->d_lst_k);                     // the addresses are now in the run tables
        ls->d_lst_k = nullptr;
    }
    k_real_qperm<<<(unsigned)nlists, 256, 0, stream>>>(nlists, ls->d_lst_q);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(stream));
    return 0;
}

int os_build_lists(const os::ListChoice &c, const os::WinDesc *d_wins, int64_t nwin, OsLists *ls, const OsPlanView &pv,
                   int64_t sort_chunk_windows, hipStream_t stream)
{
    if (c.builder == os::Builder::sorted)
        return lists_sorted(d_wins, nwin, ls, pv, c.mode == 2, c.rmax, sort_chunk_windows, stream);
    if (c.builder == os::Builder::inverse) return lists_inverse(d_wins, nwin, ls, pv, c.rmax, stream);
    return lists_direct(d_wins, nwin, ls, pv, c.mode == 2, c.rmax, stream);
}

}  // namespace cm2
