// cm2_fx_lists.hip -- the plan-time builders of the fixed-order P^T lists (cm2_fx_lists.h): per slice, the samples
// sorted by (pixel, time) and packed into groups of four entries that hold whole runs, plus the lists of the runs
// too long for the groups.  Two complete builders: one workgroup per slice (k_fx_build, the default) and the serial
// pair k_fx_keys + radix sort + k_fx_pack (CM2_FX_BUILD=serial), which the tests use as an independent cross-check.
#include "cm2_fx_lists.h"

#include <hipcub/hipcub.hpp>

using namespace cm2;

namespace {

// keys of the per-slice sort: (global slice number << 16) | pixel in tile; value = list entry
__global__ __launch_bounds__(256) void k_fx_keys(int64_t nvalid, int64_t ntiles, int S, uint32_t qmask,
                                                  const int64_t *__restrict__ tile_off,
                                                  const int64_t *__restrict__ tile_slice0,
                                                  const uint16_t *__restrict__ pl,
                                                  uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nvalid; k += stride) {
        int64_t lo = 0, hi = ntiles;                      // largest b with tile_off[b] <= k
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (tile_off[mid] <= k) lo = mid; else hi = mid;
        }
        const int64_t r = k - tile_off[lo];
        const uint32_t w = pl[k];
        keys[k] = ((uint64_t)(tile_slice0[lo] + r / S) << 16) | (uint64_t)(w & qmask);
        vals[k] = w | ((uint32_t)(r % S) << kFxOffsetShift);
    }
}

// One thread per slice walks the slice's sorted entries and packs the runs into groups.
// WRITE = false: counts[4 s + {0, 1, 2, 3}] = groups, tail runs, tail entries, highest level.
// WRITE = true: the groups / tail lists are written at the offsets of the slice.
// NANG = angle arrays to carry along: 0 (pol = 1), 1 (half angle), 2 (cos and sin); a compile-time
// switch, because a run-time "if (ga)" does not keep the compiler from issuing the a_tb load.
template <bool WRITE, int NANG>
__global__ __launch_bounds__(64) void k_fx_pack(
    int64_t nslices, uint32_t qmask, const int64_t *__restrict__ slice_k0,
    const uint32_t *__restrict__ ent, const double *__restrict__ a_tb,
    const double *__restrict__ b_tb, uint32_t *__restrict__ counts,
    const uint2 *__restrict__ meta, const uint32_t *__restrict__ tent_off,
    uint32_t *__restrict__ gent, double *__restrict__ ga, double *__restrict__ gb,
    uint2 *__restrict__ trun, uint32_t *__restrict__ tent, double *__restrict__ ta,
    double *__restrict__ tb)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslices) return;
    const int64_t k0 = slice_k0[s];
    const int len = (int)(slice_k0[s + 1] - k0);
    int64_t g = WRITE ? (int64_t)meta[s].x : 0;
    uint32_t ntr = 0, nte = 0, ng = 0, maxlev = 0;
    int fill = 0;
    auto put = [&](int slot, uint32_t w, uint32_t level) {
        if (!WRITE) return;
        const int64_t at = 4 * g + slot;
        gent[at] = w | (level << kFxLevelShift);
        const int64_t src = k0 + (int64_t)((w >> kFxOffsetShift) & kFxOffsetMask);
        if (NANG >= 1) ga[at] = a_tb[src];
        if (NANG == 2) gb[at] = b_tb[src];
    };
    auto close = [&]() {
        if (WRITE)
            for (int slot = fill; slot < 4; ++slot) {
                gent[4 * g + slot] = kFxNull;
                if (NANG >= 1) ga[4 * g + slot] = 0.0;
                if (NANG == 2) gb[4 * g + slot] = 0.0;
            }
        ++g;
        ++ng;
        fill = 0;
    };
    int i = 0;
    while (i < len) {
        const uint32_t q = ent[k0 + i] & qmask;
        int L = 1;
        while (i + L < len && (ent[k0 + i + L] & qmask) == q) ++L;
        if (L > 4 * (kFxMaxLevel + 1)) {
            if (WRITE) {
                const uint32_t e0 = tent_off[s] + nte;
                trun[(int64_t)(meta[s].y & kFxRunMask) + ntr] = make_uint2(e0, q);
                for (int m = 0; m < L; ++m) {
                    const uint32_t w = ent[k0 + i + m];
                    tent[e0 + m] = w;
                    const int64_t src = k0 + (int64_t)((w >> kFxOffsetShift) & kFxOffsetMask);
                    if (NANG >= 1) ta[e0 + m] = a_tb[src];
                    if (NANG == 2) tb[e0 + m] = b_tb[src];
                }
            }
            ++ntr;
            nte += (uint32_t)L;
        } else if (L <= 4) {
            if (fill + L > 4) close();
            for (int m = 0; m < L; ++m) put(fill + m, ent[k0 + i + m], 0);
            fill += L;
            if (fill == 4) close();
        } else {
            if (fill > 0) close();
            if ((uint32_t)((L - 1) / 4) > maxlev) maxlev = (uint32_t)((L - 1) / 4);
            // all pieces of a run inside ONE wave (64 consecutive groups of the slice): the kernel
            // orders the pieces by the program order of that wave's LDS adds, not by barriers
            while ((int)(ng % 64u) + (L + 3) / 4 > 64) close();
            for (int m = 0; m < L; ++m) {
                put(fill, ent[k0 + i + m], (uint32_t)(m / 4));
                if (++fill == 4) close();
            }
            if (fill > 0) close();
        }
        i += L;
    }
    if (fill > 0) close();
    if (!WRITE) {
        counts[4 * s] = ng;
        counts[4 * s + 1] = ntr;
        counts[4 * s + 2] = nte;
        counts[4 * s + 3] = maxlev;
    }
}

// ---- the same lists built by one workgroup per slice ------------------------------------------------
// k_fx_keys + a global radix sort + one THREAD per slice walking ~1500 sorted entries (k_fx_pack) cost
// 14 ms at C4.  k_fx_build does the whole slice in LDS: a bitonic sort of (pixel, position) keys, the
// runs from a flag scan, and a packing that needs no walk: runs are placed by CLASS with ranks from a
// scan --
//   runs of 5 .. 60 entries ("long") first, each in ceil(L / 4) consecutive groups with levels 0, 1, ..;
//     rows of 64 groups (= one wave of the P^T kernel): with R = 64 - (groups of the slice's longest run)
//     + 1, run i with u_i = groups of the long runs before it goes to row u_i / R at offset u_i - (u of
//     the row's first run) <= R - 1, so it ends inside the row;
//   then the runs of 4, the runs of 3 (slot 3 takes a single), the runs of 2 in pairs (an odd one out
//     takes two singles), the remaining singles four to a group.
// What the P^T kernel needs holds as before: a run's entries are in time order, the pieces of a long
// run are consecutive groups of one wave, a pixel appears in one run per slice.  The sums per pixel
// are the same sums in the same order as with k_fx_pack's lists; only the packing differs (a few
// per cent fewer groups: k_fx_pack closes a group when the next run does not fit).
// Pass 1 (WRITE = false) sorts, stores the sorted keys in ent and counts; pass 2 reads ent and writes.
constexpr int kFbT = 256, kFbMaxS = 4 * kFxT, kFbPer = kFbMaxS / kFbT;
constexpr int kFbMaxGroups = 1280;       // 2048 entries: <= 0.4 groups an entry (runs of 5) x 64 / 50

__device__ __forceinline__ uint64_t fb_exscan(uint64_t v, uint64_t *tmp, uint64_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    uint64_t before = inc - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < kFbT / 64; ++w) {
        if (w < wave) before += tmp[w];
        total += tmp[w];
    }
    __syncthreads();
    return before;
}

template <bool WRITE, int NANG>
__global__ __launch_bounds__(kFbT) void k_fx_build(
    int64_t nslices, uint32_t qmask, const int64_t *__restrict__ slice_k0, int k0_stride,
    const uint16_t *__restrict__ pl, uint32_t *__restrict__ ent, const double *__restrict__ a_tb,
    const double *__restrict__ b_tb, uint32_t *__restrict__ counts, const uint2 *__restrict__ meta,
    const uint32_t *__restrict__ tent_off, uint32_t *__restrict__ gent, double *__restrict__ ga,
    double *__restrict__ gb, uint2 *__restrict__ trun, uint32_t *__restrict__ tent,
    double *__restrict__ ta, double *__restrict__ tb, unsigned int *__restrict__ overflow)
{
    __shared__ uint32_t keys[kFbMaxS];
    __shared__ uint16_t rs[kFbMaxS + 1];
    __shared__ uint64_t tmp[kFbT / 64];
    __shared__ uint32_t rowfirst[64];
    __shared__ uint32_t misc[2];
    __shared__ uint32_t tails[2 * (kFbMaxS / (4 * (kFxMaxLevel + 1)) + 2)];   // (first sorted entry, first tail entry) per tail run
    __shared__ uint32_t stage[WRITE ? 4 * kFbMaxGroups : 4];
    const int64_t s = blockIdx.x;
    if (s >= nslices) return;
    const int t = threadIdx.x;
    // (k0_stride = 1: slice s = [slice_k0[s], slice_k0[s + 1]); 2: a list of (first, end) pairs)
    const int64_t k0 = slice_k0[s * k0_stride];
    const int len = (int)(slice_k0[s * k0_stride + 1] - k0);
    if (!WRITE) {
        int NS = 64;
        while (NS < len) NS <<= 1;
        for (int i = t; i < NS; i += kFbT) {
            uint32_t key = 0xFFFFFFFFu;
            if (i < len) {
                const uint32_t w = pl[k0 + i];
                key = ((w & qmask) << 12) | ((uint32_t)i << 1) | ((w & ~qmask & 0xFFFFu) ? 1u : 0u);
            }
            keys[i] = key;
        }
        __syncthreads();
        for (int k = 2; k <= NS; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < NS / 2; i += kFbT) {
                    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                    const uint32_t a = keys[lo], b = keys[hi];
                    const bool asc = (lo & k) == 0;
                    if ((a > b) == asc) {
                        keys[lo] = b;
                        keys[hi] = a;
                    }
                }
                __syncthreads();
            }
        for (int i = t; i < len; i += kFbT) ent[k0 + i] = keys[i];
    } else {
        for (int i = t; i < len; i += kFbT) keys[i] = ent[k0 + i];
        __syncthreads();
    }
    // ---- runs: rs[r] = first sorted entry of run r ----
    int nst = 0;
    bool st[kFbPer];
#pragma unroll
    for (int u = 0; u < kFbPer; ++u) {
        const int j = kFbPer * t + u;
        st[u] = j < len && (j == 0 || (keys[j] >> 12) != (keys[j - 1] >> 12));
        nst += st[u] ? 1 : 0;
    }
    uint64_t tot = 0;
    int r0 = (int)fb_exscan((uint64_t)nst, tmp, tot);
    const int nruns = (int)tot;
#pragma unroll
    for (int u = 0; u < kFbPer; ++u)
        if (st[u]) rs[r0++] = (uint16_t)(kFbPer * t + u);
    if (t == 0) {
        rs[nruns] = (uint16_t)len;
        misc[0] = 0;
        misc[1] = 0;
    }
    if (t < 64) rowfirst[t] = 0xFFFFFFFFu;
    __syncthreads();
    // ---- classes and ranks: A = singles | pairs << 12 | triples << 24 | fours << 36,
    //      B = long groups | tail runs << 12 | tail entries << 24 ----
    uint64_t sumA = 0, sumB = 0;
    int L[kFbPer];
#pragma unroll
    for (int u = 0; u < kFbPer; ++u) {
        const int r = kFbPer * t + u;
        L[u] = r < nruns ? (int)rs[r + 1] - (int)rs[r] : 0;
        if (L[u] == 0) continue;
        if (L[u] <= 4) sumA += (uint64_t)1 << (12 * (L[u] - 1));
        else if (L[u] <= 4 * (kFxMaxLevel + 1)) sumB += (uint64_t)((L[u] + 3) / 4);
        else sumB += ((uint64_t)1 << 12) | ((uint64_t)L[u] << 24);
    }
    uint64_t totA = 0, totB = 0;
    uint64_t exA = fb_exscan(sumA, tmp, totA);
    uint64_t exB = fb_exscan(sumB, tmp, totB);
    const int n1 = (int)(totA & 0xFFF), n2 = (int)((totA >> 12) & 0xFFF), n3 = (int)((totA >> 24) & 0xFFF),
              n4 = (int)((totA >> 36) & 0xFFF);
    const int ntr = (int)((totB >> 12) & 0xFFF), nte = (int)(totB >> 24);
    // rows of the long runs: the row length leaves room for the slice's longest run
#pragma unroll
    for (int u = 0; u < kFbPer; ++u)
        if (L[u] > 4 && L[u] <= 4 * (kFxMaxLevel + 1)) atomicMax(&misc[1], (uint32_t)((L[u] - 1) / 4));
    __syncthreads();
    const uint32_t row_len = 64u - misc[1];              // (longest run: misc[1] + 1 groups)
    {
        uint64_t b = exB;
#pragma unroll
        for (int u = 0; u < kFbPer; ++u) {
            if (L[u] > 4 && L[u] <= 4 * (kFxMaxLevel + 1)) {
                const uint32_t uu = (uint32_t)(b & 0xFFF);
                atomicMin(&rowfirst[uu / row_len], uu);
                b += (uint64_t)((L[u] + 3) / 4);
            } else if (L[u] > 4 * (kFxMaxLevel + 1)) {
                b += ((uint64_t)1 << 12) | ((uint64_t)L[u] << 24);
            }
        }
    }
    __syncthreads();
    int pos[kFbPer];
    {
        uint64_t b = exB;
#pragma unroll
        for (int u = 0; u < kFbPer; ++u) {
            pos[u] = 0;
            if (L[u] > 4 && L[u] <= 4 * (kFxMaxLevel + 1)) {
                const uint32_t uu = (uint32_t)(b & 0xFFF), row = uu / row_len;
                pos[u] = (int)(64 * row + uu - rowfirst[row]);
                atomicMax(&misc[0], (uint32_t)(pos[u] + (L[u] + 3) / 4));
                b += (uint64_t)((L[u] + 3) / 4);
            } else if (L[u] > 4 * (kFxMaxLevel + 1)) {
                b += ((uint64_t)1 << 12) | ((uint64_t)L[u] << 24);
            }
        }
    }
    __syncthreads();
    const int GL = (int)misc[0], maxlev = (int)misc[1];
    const int odd2 = n2 & 1;
    const int s1 = n1 > n3 ? n1 - n3 : 0;
    const int x2 = odd2 ? (s1 < 2 ? s1 : 2) : 0;
    const int ng = GL + n4 + n3 + (n2 + 1) / 2 + (s1 - x2 + 3) / 4;
    if (!WRITE) {
        if (t == 0) {
            counts[4 * s] = (uint32_t)ng;
            counts[4 * s + 1] = (uint32_t)ntr;
            counts[4 * s + 2] = (uint32_t)nte;
            counts[4 * s + 3] = (uint32_t)maxlev;
        }
        return;
    }
    if (ng > kFbMaxGroups) {                              // (cannot happen for S <= 2048; never write past the stage)
        if (t == 0) atomicOr(overflow, 1u);
        return;
    }
    for (int i = t; i < 4 * ng; i += kFbT) stage[i] = kFxNull;
    __syncthreads();
    const int64_t g_base = (int64_t)meta[s].x;
    const int64_t tr_base = (int64_t)(meta[s].y & kFxRunMask);
    const uint32_t te_base = tent_off[s];
    {
        uint64_t a = exA, b = exB;
        const int G4 = GL, G3 = GL + n4, G2 = G3 + n3, G1 = G2 + (n2 + 1) / 2;
#pragma unroll
        for (int u = 0; u < kFbPer; ++u) {
            if (L[u] == 0) continue;
            const int j0 = (int)rs[kFbPer * t + u];
            auto value = [&](int m) {
                const uint32_t key = keys[j0 + m];
                return (key >> 12) | ((key & 1u) << 15) | (((key >> 1) & 0x7FFu) << kFxOffsetShift);
            };
            if (L[u] == 1) {
                const int sr = (int)(a & 0xFFF);
                int g, slot;
                if (sr < n3) {
                    g = G3 + sr;
                    slot = 3;
                } else if (sr - n3 < x2) {
                    g = G2 + n2 / 2;
                    slot = 2 + (sr - n3);
                } else {
                    const int q = sr - n3 - x2;
                    g = G1 + q / 4;
                    slot = q % 4;
                }
                stage[4 * g + slot] = value(0);
                a += 1;
            } else if (L[u] == 2) {
                const int r2 = (int)((a >> 12) & 0xFFF);
                const int g = G2 + r2 / 2, slot = (r2 & 1) * 2;
                stage[4 * g + slot] = value(0);
                stage[4 * g + slot + 1] = value(1);
                a += (uint64_t)1 << 12;
            } else if (L[u] == 3) {
                const int g = G3 + (int)((a >> 24) & 0xFFF);
                for (int m = 0; m < 3; ++m) stage[4 * g + m] = value(m);
                a += (uint64_t)1 << 24;
            } else if (L[u] == 4) {
                const int g = G4 + (int)((a >> 36) & 0xFFF);
                for (int m = 0; m < 4; ++m) stage[4 * g + m] = value(m);
                a += (uint64_t)1 << 36;
            } else if (L[u] <= 4 * (kFxMaxLevel + 1)) {
                for (int m = 0; m < L[u]; ++m)
                    stage[4 * pos[u] + m] = value(m) | ((uint32_t)(m / 4) << kFxLevelShift);
                b += (uint64_t)((L[u] + 3) / 4);
            } else {
                const int tr = (int)((b >> 12) & 0xFFF);
                const uint32_t e0 = te_base + (uint32_t)(b >> 24);
                trun[tr_base + tr] = make_uint2(e0, keys[j0] >> 12);
                tails[2 * tr] = (uint32_t)j0 | ((uint32_t)L[u] << 16);
                tails[2 * tr + 1] = e0;
                b += ((uint64_t)1 << 12) | ((uint64_t)L[u] << 24);
            }
        }
    }
    __syncthreads();
    // the runs kept out of the groups: their entries, in time order
    for (int tr = 0; tr < ntr; ++tr) {
        const int j0 = (int)(tails[2 * tr] & 0xFFFFu), Lr = (int)(tails[2 * tr] >> 16);
        const uint32_t e0 = tails[2 * tr + 1];
        for (int m = t; m < Lr; m += kFbT) {
            const uint32_t key = keys[j0 + m];
            const uint32_t w = (key >> 12) | ((key & 1u) << 15) | (((key >> 1) & 0x7FFu) << kFxOffsetShift);
            tent[e0 + m] = w;
            const int64_t src = k0 + (int64_t)((w >> kFxOffsetShift) & kFxOffsetMask);
            if (NANG >= 1) ta[e0 + m] = a_tb[src];
            if (NANG == 2) tb[e0 + m] = b_tb[src];
        }
    }
    for (int i = t; i < 4 * ng; i += kFbT) {
        const uint32_t w = stage[i];
        gent[4 * g_base + i] = w;
        const int64_t src = k0 + (int64_t)((w >> kFxOffsetShift) & kFxOffsetMask);
        if (NANG >= 1) ga[4 * g_base + i] = w == kFxNull ? 0.0 : a_tb[src];
        if (NANG == 2) gb[4 * g_base + i] = w == kFxNull ? 0.0 : b_tb[src];
    }
}

// One pass of a builder over n slices: the counting pass (WRITE = false: the counts, and the sorted entries in
// `ent`) or the writing pass into the plan's lists.  serial: k_fx_pack on the radix-sorted entries, slices as a cut
// list (slice s = [cuts[s], cuts[s + 1])); otherwise k_fx_build, slices as (first, end) pairs.
struct FxPass {
    int64_t n;
    const int64_t *d_pairs, *d_cuts;
    uint32_t *ent, *counts;
    const uint32_t *tent_off;
    unsigned int *overflow;
};
template <bool WRITE, int NANG>
void fx_pass(const cm2_tiles *t, bool serial, const FxPass &w, hipStream_t st)
{
    const FxLists &f = t->fx;
    const uint32_t qmask = fx_pixel_mask(t->half);
    const double *a_tb = t->half ? t->d_half : t->d_cos, *b_tb = t->half ? nullptr : t->d_sin;
    uint32_t *gent = reinterpret_cast<uint32_t *>(f.d_gent);
    if (serial)
        k_fx_pack<WRITE, NANG><<<(int)((w.n + 63) / 64), 64, 0, st>>>(
            w.n, qmask, w.d_cuts, w.ent, a_tb, b_tb, w.counts, f.d_meta, w.tent_off, gent, f.d_ga, f.d_gb, f.d_trun,
            f.d_tent, f.d_ta, f.d_tb);
    else
        k_fx_build<WRITE, NANG><<<(unsigned)w.n, kFbT, 0, st>>>(
            w.n, qmask, w.d_pairs, 2, t->d_pl, w.ent, a_tb, b_tb, w.counts, f.d_meta, w.tent_off, gent, f.d_ga, f.d_gb,
            f.d_trun, f.d_tent, f.d_ta, f.d_tb, w.overflow);
}

}  // namespace

namespace cm2 {

int fx_count_sample(const cm2_tiles *t, int S, hipStream_t st, double *mean_groups, double *over)
{
    *mean_groups = 0.0;
    *over = 0.0;
    std::vector<int64_t> pairs;
    const policy::Slices sl_all = policy::slices(t->tile_off, S);
    const std::vector<int64_t> &slice0 = sl_all.slice0, &all = sl_all.pairs;
    int64_t seen = 0;
    for (int64_t b = 0; b < t->ntiles; ++b) {
        if (fx_hot_tile(t, b)) continue;
        for (int64_t sl = slice0[(size_t)b]; sl < slice0[(size_t)b + 1]; ++sl) {
            const int64_t k = all[(size_t)(2 * sl)], e = all[(size_t)(2 * sl + 1)];
            if (e - k != S) continue;                    // (full slices only)
            if (seen++ % 8 == 0) {
                pairs.push_back(k);
                pairs.push_back(e);
            }
        }
    }
    const int64_t np = (int64_t)pairs.size() / 2;
    if (np == 0) return 0;
    DevTemp<int64_t> d_pairs;
    DevTemp<uint32_t> ent, d_counts;
    DevTemp<unsigned int> d_overflow;
    CM2_HIP(d_pairs.alloc(pairs.size()));
    CM2_HIP(cm2::upload(d_pairs, pairs.data(), sizeof(int64_t) * pairs.size(), st));
    CM2_HIP(ent.alloc(t->nvalid));
    CM2_HIP(d_counts.alloc(4 * np));
    CM2_HIP(d_overflow.alloc(1));
    fx_pass<false, 0>(t, false, FxPass{np, d_pairs, nullptr, ent, d_counts, nullptr, d_overflow}, st);
    CM2_LAUNCH_OK();
    std::vector<uint32_t> counts((size_t)(4 * np));
    CM2_HIP(cm2::download(counts.data(), d_counts, sizeof(uint32_t) * counts.size(), st));
    CM2_HIP(hipStreamSynchronize(st));
    double gsum = 0.0;
    int64_t nover = 0;
    for (int64_t i = 0; i < np; ++i) {
        gsum += counts[(size_t)(4 * i)];
        if (counts[(size_t)(4 * i)] > (uint32_t)kFxT) ++nover;
    }
    *mean_groups = gsum / (double)np;
    *over = (double)nover / (double)np;
    return 0;
}

int fx_build_lists(cm2_tiles *t, int S, hipStream_t st, double *mean_groups, double *over)
{
    // (k_fx_build sorts a slice in LDS; policy::fx_max_slice allows no longer one)
    CM2_CHECK(S <= kFbMaxS, "cm2_tiles: a slice of %d samples is longer than the %d the list builder holds", S, kFbMaxS);
    FxLists &f = t->fx;
    const int64_t nv = t->nvalid;
    policy::Slices sl = policy::slices(t->tile_off, S);
    const std::vector<int64_t> &slice0 = sl.slice0;
    const std::vector<int64_t> &k0 = sl.pairs;       // k0: (first address, end) of every slice
    const int64_t nslices = slice0[(size_t)t->ntiles];
    CM2_CHECK(nslices < ((int64_t)1 << 31), "cm2_tiles: too many slices");
    {
        std::vector<uint2> sk((size_t)nslices + 1, make_uint2(0, 0));
        for (int64_t i = 0; i < nslices; ++i)
            sk[(size_t)i] = make_uint2((uint32_t)k0[(size_t)(2 * i)], (uint32_t)(k0[(size_t)(2 * i + 1)] - k0[(size_t)(2 * i)]));
        CM2_HIP(cm2::dev_malloc(&f.d_sk, sizeof(uint2) * sk.size()));
        CM2_HIP(cm2::upload(f.d_sk, sk.data(), sizeof(uint2) * sk.size(), st));
        CM2_HIP(hipStreamSynchronize(st));           // (sk is a local)
    }
    CM2_HIP(cm2::dev_malloc(&f.d_slice0, sizeof(int64_t) * slice0.size()));
    CM2_HIP(cm2::upload(f.d_slice0, slice0.data(), sizeof(int64_t) * slice0.size(), st));
    *mean_groups = 0.0;
    *over = 0.0;
    int64_t ngroups = 0;
    if (nv > 0) {
        DevTemp<int64_t> d_k0;
        DevTemp<uint64_t> keys_in, keys_out;
        DevTemp<uint32_t> vals_in, ent, d_counts, d_tent_off;
        DevTemp<unsigned int> d_overflow;
        DevTemp<char> d_temp;
        CM2_HIP(d_k0.alloc(k0.size()));
        CM2_HIP(cm2::upload(d_k0, k0.data(), sizeof(int64_t) * k0.size(), st));
        // one workgroup per slice (k_fx_build) unless CM2_FX_BUILD=serial asks for the radix sort and
        // the one-thread-per-slice packer (k_fx_pack): other lists, the same sums
        const bool serial = t->sw.fx_serial;
        // (k_fx_pack, the serial builder of the global order, reads the slices as a cut list: slice s =
        //  [cut[s], cut[s + 1]))
        DevTemp<int64_t> d_k0s;
        std::vector<int64_t> cuts;
        if (serial) {
            for (int64_t i = 0; i < nslices; ++i) cuts.push_back(k0[(size_t)(2 * i)]);
            cuts.push_back(nv);
            CM2_HIP(d_k0s.alloc(cuts.size()));
            CM2_HIP(cm2::upload(d_k0s, cuts.data(), sizeof(int64_t) * cuts.size(), st));
        }
        CM2_HIP(ent.alloc(nv));
        CM2_HIP(d_counts.alloc(4 * nslices));
        CM2_HIP(d_overflow.alloc(1));
        CM2_HIP(hipMemsetAsync(d_overflow.p, 0, sizeof(unsigned int), st));
        if (serial) {
            CM2_HIP(keys_in.alloc(nv));
            CM2_HIP(keys_out.alloc(nv));
            CM2_HIP(vals_in.alloc(nv));
            k_fx_keys<<<grid_for(nv), kBlock, 0, st>>>(nv, t->ntiles, S, fx_pixel_mask(t->half), t->d_tile_off,
                                                      f.d_slice0, t->d_pl, keys_in, vals_in);
            CM2_LAUNCH_OK();
            int end_bit = 17;
            while (((int64_t)1 << (end_bit - 16)) <= nslices && end_bit < 64) ++end_bit;
            size_t tb = 0;
            CM2_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in.p, keys_out.p, vals_in.p,
                                                       ent.p, nv, 0, end_bit, st));
            CM2_HIP(d_temp.alloc(tb + 16));
            CM2_HIP(hipcub::DeviceRadixSort::SortPairs(d_temp.p, tb, keys_in.p, keys_out.p, vals_in.p,
                                                       ent.p, nv, 0, end_bit, st));
        }
        FxPass pass{nslices, d_k0, d_k0s, ent, d_counts, nullptr, d_overflow};
        fx_pass<false, 0>(t, serial, pass, st);
        CM2_LAUNCH_OK();
        std::vector<uint32_t> counts((size_t)(4 * nslices));
        CM2_HIP(cm2::download(counts.data(), d_counts, sizeof(uint32_t) * counts.size(), st));
        CM2_HIP(hipStreamSynchronize(st));
        std::vector<uint8_t> hot((size_t)t->ntiles, 0);
        for (int64_t b = 0; b < t->ntiles; ++b) hot[(size_t)b] = fx_hot_tile(t, b) ? 1 : 0;
        const policy::FxOffsets off = policy::fx_offsets(counts, sl, hot, S, kFxT, kFxLevelShift);
        CM2_CHECK(off.fits, "cm2_tiles: fixed-order lists exceed their offsets");
        ngroups = off.ngroups;
        *mean_groups = off.mean_groups;
        *over = off.over;
        // (+1 group: a slice without groups at the very end still loads "its" group 0)
        const int64_t ng1 = ngroups + 1, nt1 = off.ntent ? off.ntent : 1;
        static_assert(sizeof(uint2) == 2 * sizeof(uint32_t), "meta is uploaded as pairs of words");
        CM2_HIP(cm2::dev_malloc(&f.d_meta, sizeof(uint32_t) * off.meta.size()));
        CM2_HIP(cm2::upload(f.d_meta, off.meta.data(), sizeof(uint32_t) * off.meta.size(), st));
        CM2_HIP(d_tent_off.alloc(off.tent_off.size()));
        CM2_HIP(cm2::upload(d_tent_off, off.tent_off.data(), sizeof(uint32_t) * off.tent_off.size(), st));
        CM2_HIP(cm2::dev_malloc(&f.d_gent, sizeof(uint4) * ng1));
        CM2_HIP(cm2::dev_malloc(&f.d_trun, sizeof(uint2) * (off.ntrun + 1)));
        CM2_HIP(cm2::dev_malloc(&f.d_tent, sizeof(uint32_t) * nt1));
        if (t->pol > 1) {
            CM2_HIP(cm2::dev_malloc(&f.d_ga, sizeof(double) * 4 * ng1));
            CM2_HIP(cm2::dev_malloc(&f.d_ta, sizeof(double) * nt1));
            if (!t->half) {
                CM2_HIP(cm2::dev_malloc(&f.d_gb, sizeof(double) * 4 * ng1));
                CM2_HIP(cm2::dev_malloc(&f.d_tb, sizeof(double) * nt1));
            }
        }
        const uint2 last = make_uint2((uint32_t)off.ntent, 0);
        CM2_HIP(cm2::upload(f.d_trun + off.ntrun, &last, sizeof(uint2), st));
        pass.tent_off = d_tent_off;
        if (t->pol == 1) fx_pass<true, 0>(t, serial, pass, st);
        else if (t->half) fx_pass<true, 1>(t, serial, pass, st);
        else fx_pass<true, 2>(t, serial, pass, st);
        CM2_LAUNCH_OK();
        unsigned int h_over = 0;
        CM2_HIP(cm2::download(&h_over, d_overflow.p, sizeof(h_over), st));
        CM2_HIP(hipStreamSynchronize(st));
        CM2_CHECK(h_over == 0, "cm2_tiles: a slice of %d samples packs into more than %d groups", S,
                  kFbMaxGroups);
    } else {
        const std::vector<uint2> meta((size_t)nslices + 1, make_uint2(0, 0));
        CM2_HIP(cm2::dev_malloc(&f.d_meta, sizeof(uint2) * meta.size()));
        CM2_HIP(cm2::upload(f.d_meta, meta.data(), sizeof(uint2) * meta.size(), st));
        CM2_HIP(cm2::dev_malloc(&f.d_gent, sizeof(uint4)));
        CM2_HIP(cm2::dev_malloc(&f.d_trun, sizeof(uint2)));
        CM2_HIP(cm2::dev_malloc(&f.d_tent, sizeof(uint32_t)));
        CM2_HIP(hipStreamSynchronize(st));
    }
    f.S = S;
    f.ngroups = ngroups;
    f.nslices = nslices;
    return 0;
}

}  // namespace cm2
