// cm2_plan_policy.h -- the host decisions of the tile plan and of its fixed-order P^T lists: where the pixel tiles
// are cut, how a bucket is cut into slices, work items and hot ranges, how the slices of heavy tiles are shared
// out to workgroups, and for the fixed-order lists the LDS budget, the list offsets from the per-slice counts and the
// tuning of the slice length.  Plain C++17 on host vectors: no device, no plan object, no environment, no hidden state -- a
// rule can be changed here and its plan looked at on a CPU (tests/test_plan_policy_cpu.py).  Tile cuts and part
// boundaries fix the order in which a pixel's terms are added, hence the bits: integer types, floating-point
// expressions and tie rules are part of the result.  cm2_tiles.hip, cm2_tiles_fixed.hip and cm2_fx_lists.hip turn
// these answers into device data.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cm2 {
namespace policy {

constexpr int64_t kHotTileMin = 32768;   // samples that make a one-pixel tile a hot tile (cm2_tiles_fixed.hip)

// ------------------------------------------------------------------ tiles -------
// Cuts every rank of a sharded run has in common, whatever its own hit map: the group boundaries of
// cm2_tiles_group_tiles (the pieces of the map that are all-reduced while the next piece is back-projected) -- the
// uniform tiling's tile boundaries nearest to eighths of the map, a function of npix and tile_pixels alone.  [9],
// from 0 to npix.
inline std::vector<int64_t> shared_cuts(int64_t npix, int tile_pixels)
{
    const int64_t ntu = (npix + tile_pixels - 1) / tile_pixels;
    std::vector<int64_t> cut(9);
    for (int c = 0; c <= 8; ++c) {
        cut[(size_t)c] = (ntu * c / 8) * tile_pixels;
        if (cut[(size_t)c] > npix || c == 8) cut[(size_t)c] = npix;
    }
    return cut;
}

// first pixel of every tile of tile_pixels pixels, [ntiles + 1]
inline std::vector<int64_t> uniform_tiles(int64_t npix, int tile_pixels)
{
    const int64_t ntiles = (npix + tile_pixels - 1) / tile_pixels;
    std::vector<int64_t> p0((size_t)ntiles + 1, 0);
    for (int64_t b = 0; b <= ntiles; ++b) p0[(size_t)b] = b * tile_pixels < npix ? b * tile_pixels : npix;
    return p0;
}

// The equal-load cut.  The fixed-order P^T keeps 512 workgroups resident (two per CU): tiles of equal load finish in
// whole rounds of 512, so 737 tiles cost as much as 1024.  The width limit makes a sparse region take more tiles than
// its load asks for; the target load is therefore lowered (mult = 1, 2, 3, 4 times the uniform count `base_tiles`)
// until the cut fits mult x the uniform count, with 2 % slack so that rounding does not spill one more tile; a tile
// ends when the next pixel would exceed the target, the width tile_pixels or a shared cut (a single pixel heavier
// than the target is a tile of its own).  A uniform count that is no multiple of 512 keeps mult = 1.
// *mult_used: the multiple the cut was made for.
inline std::vector<int64_t> equal_load_tiles(const std::vector<unsigned int> &hits, int64_t npix, int tile_pixels,
                                             int64_t base_tiles, int64_t nvalid, int *mult_used = nullptr)
{
    const std::vector<int64_t> forced = shared_cuts(npix, tile_pixels);
    std::vector<int64_t> p0v;
    for (int mult = 1;; ++mult) {
        const int64_t target = (int64_t)(1.02 * (double)nvalid / (double)(base_tiles * mult)) + 1;
        int fc = 1;
        p0v.assign(1, 0);
        int64_t acc = 0, start = 0;
        for (int64_t p = 0; p < npix; ++p) {
            const int64_t h = hits[(size_t)p];
            while (fc < 8 && forced[(size_t)fc] < p) ++fc;
            const bool at_cut = fc < 8 && forced[(size_t)fc] == p;
            if (p > start && (acc + h > target || p - start >= tile_pixels || at_cut)) {
                p0v.push_back(p);
                start = p;
                acc = 0;
            }
            acc += h;
        }
        p0v.push_back(npix);
        if (mult_used) *mult_used = mult;
        if ((int64_t)p0v.size() - 1 <= base_tiles * mult || base_tiles % 512 != 0 || mult == 4) break;
    }
    return p0v;
}

// uniform tiles, but every pixel with at least hot_min hits is a tile of its own (the hot-tile path of the
// fixed-order P^T takes it); *any = some pixel is that heavy (otherwise these are the uniform tiles)
inline std::vector<int64_t> hot_pixel_tiles(const std::vector<unsigned int> &hits, int64_t npix, int tile_pixels,
                                            int64_t hot_min, bool *any)
{
    std::vector<int64_t> p0v(1, 0);
    *any = false;
    for (int64_t p = 1; p < npix; ++p) {
        const bool hot_here = (int64_t)hits[(size_t)p] >= hot_min, hot_before = (int64_t)hits[(size_t)p - 1] >= hot_min;
        if (p % tile_pixels == 0 || hot_here || hot_before) p0v.push_back(p);
        *any = *any || hot_here || hot_before;
    }
    p0v.push_back(npix);
    return p0v;
}

// The fixed-order P^T gives every tile to ONE workgroup: a hit map that is far from uniform (half of the samples on a
// tenth of the sky: 0.47 -> 1.7 ms) would leave most of the chip waiting for the heaviest tiles.  When some uniform
// tile holds over 25 % more than the mean, the pixel ranges can be re-cut to equal sample counts (equal_load: width
// <= tile_pixels, every pixel still summed by one workgroup in time order, so results do not change by a bit).
// Round 4: by default such a hit map keeps the uniform tile width instead, and the fixed-order P^T shares the slices
// of its heavy tiles out to several workgroups (uniform_parts, pt_split; cm2_tiles.h, "PARTS"): narrow dense tiles
// see many hits per pixel and slice (runs of 5-8 list entries in two level passes) and halve the address runs of the
// overlap-save kernel.  Only a pixel heavy enough for the hot-tile path is cut out as a tile of its own.
enum class Tiling { uniform, equal_load, uniform_parts };
// CM2_TILE_BALANCE: off = uniform tiles, one workgroup each; cut = the equal-load cut (also chosen when the exact
// summation order is asked for: it does not change a bit); parts = split even when the hit map is even; automatic =
// by the hit map (switch not set)
enum class Balance { automatic, off, cut, parts };
struct TilingChoice {
    Tiling tiling = Tiling::uniform;
    bool pt_split = false;               // the fixed-order P^T may share a tile's slices out to parts
    int64_t hot_min = 0;                 // > 0: pixels with so many hits become tiles (hot_pixel_tiles);
                                         // 0: no tile holds enough samples for one
};
// tile_off: first address of every uniform tile, [ntiles + 1]
inline TilingChoice choose_tiling(const std::vector<int64_t> &tile_off, bool exact_order, Balance sw)
{
    const int64_t ntiles = (int64_t)tile_off.size() - 1, nvalid = tile_off[(size_t)ntiles];
    int64_t nmax = 0;
    for (int64_t b = 0; b < ntiles; ++b)
        if (tile_off[(size_t)b + 1] - tile_off[(size_t)b] > nmax) nmax = tile_off[(size_t)b + 1] - tile_off[(size_t)b];
    const double mean_load = (double)nvalid / (double)(ntiles > 0 ? ntiles : 1);
    const bool uneven = ntiles >= 64 && nvalid >= (1 << 20) && (double)nmax > 1.25 * mean_load;
    const bool some = nvalid > 0;
    TilingChoice c;
    if (sw == Balance::automatic) c.tiling = !uneven ? Tiling::uniform : (exact_order ? Tiling::equal_load : Tiling::uniform_parts);
    else if (sw == Balance::parts && some) c.tiling = Tiling::uniform_parts;
    else if (sw == Balance::cut && some) c.tiling = Tiling::equal_load;
    c.pt_split = c.tiling == Tiling::uniform_parts;
    const int64_t hot_min = (int64_t)(0.5 * mean_load) > kHotTileMin ? (int64_t)(0.5 * mean_load) : kHotTileMin;
    if (c.pt_split && nmax >= hot_min) c.hot_min = hot_min;      // (otherwise no pixel can be that heavy)
    return c;
}

// ------------------------------------------------- slices, work items, hot ranges -------
// The slices of a plan for the slice length S, as (first address, end) pairs in the order the kernel walks them: tile
// after tile, a tile's bucket [tile_off[b], tile_off[b + 1]) cut into pieces of S with a shorter last one (none for
// an empty bucket).  slice0[b] = first slice of tile b.
struct Slices {
    std::vector<int64_t> slice0, pairs;
};
inline Slices slices(const std::vector<int64_t> &tile_off, int64_t S)
{
    const int64_t ntiles = (int64_t)tile_off.size() - 1;
    Slices r;
    r.slice0.assign((size_t)ntiles + 1, 0);
    for (int64_t b = 0; b < ntiles; ++b) {
        r.slice0[(size_t)b] = (int64_t)r.pairs.size() / 2;
        const int64_t a1 = tile_off[(size_t)b + 1];
        for (int64_t k = tile_off[(size_t)b]; k < a1; k += S) {
            r.pairs.push_back(k);
            r.pairs.push_back(k + S < a1 ? k + S : a1);
        }
    }
    r.slice0[(size_t)ntiles] = (int64_t)r.pairs.size() / 2;
    return r;
}

// work items of k_P_tiles / k_Pt_tiles: the same cut with the plan's slice_samples, as the arrays the kernels read
// (tile, first address, end of every item; tile_item0[b] = first item of tile b)
struct WorkItems {
    std::vector<int64_t> tile_item0, k0, k1;
    std::vector<int32_t> tile;
};
inline WorkItems work_items(const std::vector<int64_t> &tile_off, int64_t slice_samples)
{
    Slices s = slices(tile_off, slice_samples);
    WorkItems w;
    for (size_t b = 0; b + 1 < s.slice0.size(); ++b)
        for (int64_t i = s.slice0[b]; i < s.slice0[b + 1]; ++i) {
            w.tile.push_back((int32_t)b);
            w.k0.push_back(s.pairs[(size_t)(2 * i)]);
            w.k1.push_back(s.pairs[(size_t)(2 * i + 1)]);
        }
    w.tile_item0 = std::move(s.slice0);
    return w;
}

// slice length wanted after a build (or an estimate) with S samples gave mean_groups groups per full slice and a
// fraction `over` of slices with more groups than the `threads` of a workgroup: a slice should fill ~0.92 of the
// threads but rarely more; multiples of 64 in [256, smax]
inline int wanted_slice(int S, double mean_groups, double over, int smax, int threads)
{
    int want = (int)(0.92 * threads * S / mean_groups) / 64 * 64;
    if (over > 0.10) want = want < S * 7 / 8 ? want : S * 7 / 8 / 64 * 64;
    if (want > smax) want = smax;
    if (want < 256) want = 256;
    return want;
}

// The tuning of the slice length.  A rebuild is not worth it when the wanted length is within 1/16 of the built one
// and few slices overflow, or when nothing would change.
inline bool slice_settled(int S, int want, double over)
{
    const bool close_enough = want >= S * 15 / 16 && want <= S * 17 / 16 && over <= 0.10;
    return close_enough || want == S;
}
constexpr int kSliceFirst = 1536;        // slice length of the first count
constexpr int kSliceRebuilds = 3;        // rebuilds after the first build, at most
// The slice lengths a plan tries, in order, the last one being the plan's.  build(S, mean, over) builds the lists for
// S and answers the groups per full slice and the fraction of slices with more groups than threads; count(S, mean,
// over) answers the same from a sample of the slices without building (sample_first = false: not asked, the serial
// builders).  Both return non-zero on failure, which ends the tuning with that code.  forced (CM2_PT_SLICE) in [64,
// 4 x threads] fixes the length, clamped to smax.  *S_out: the last length built.
template <typename Count, typename Build>
inline int tune_slice(int forced, int smax, int threads, bool sample_first, Count count, Build build, int *S_out)
{
    double mean = 0.0, over = 0.0;
    int &S = *S_out;
    if (forced >= 64 && forced <= 4 * threads) return build(S = forced < smax ? forced : smax, mean, over);
    S = kSliceFirst < smax ? kSliceFirst : smax;
    if (sample_first) {                                     // first guess from a sample of the slices
        if (int rc = count(S, mean, over)) return rc;
        if (mean > 0.0) S = wanted_slice(S, mean, over, smax, threads);
    }
    if (int rc = build(S, mean, over)) return rc;
    for (int iter = 0; iter < kSliceRebuilds && mean > 0.0; ++iter) {
        const int want = wanted_slice(S, mean, over, smax, threads);
        if (slice_settled(S, want, over)) break;
        S = want;
        if (int rc = build(S, mean, over)) return rc;
    }
    return 0;
}

// ------------------------------------------------------- fixed-order lists: LDS, offsets -------
constexpr int kFxThreads = 512;          // threads of k_Pt_tiles_fixed = groups of a slice handled in one round
constexpr int kFxChunkSums = 128;        // chunk sums of hot runs a slice may hold, x 3 doubles
// A CU has 160 KB of LDS.  What a workgroup may ask for so that
constexpr size_t kLdsTwoPerCU = 79 * 1024;     // ... two workgroups are resident on a CU,
constexpr size_t kLdsOnePerCU = 159 * 1024;    // ... one is.
// LDS of k_Pt_tiles_fixed for slices of S samples: the tile's accumulators, two buffers of the slice's values (at
// least two values a thread) and the chunk sums
inline size_t fx_lds_bytes(int tp, int pol, int S)
{
    int vpt = (S + kFxThreads - 1) / kFxThreads;
    vpt = vpt <= 2 ? 2 : vpt;
    return sizeof(double) * ((size_t)tp * pol + 2 * (size_t)vpt * kFxThreads + 3 * (size_t)kFxChunkSums);
}
// longest slice the kernel can stage beside the tile: 4 values a thread at most, and short enough for
// two workgroups per CU whenever some slice length allows that
inline int fx_max_slice(int tp, int pol)
{
    int smax = 4 * kFxThreads;
    {
        int s2 = smax;
        while (s2 > 2 * kFxThreads && fx_lds_bytes(tp, pol, s2) > kLdsTwoPerCU) s2 -= kFxThreads;
        if (fx_lds_bytes(tp, pol, s2) <= kLdsTwoPerCU) smax = s2;
    }
    while (smax > 256 && fx_lds_bytes(tp, pol, smax) > kLdsOnePerCU) smax -= 256;
    return smax;
}
// not even the shortest slice fits beside the tile: the plan uses the atomic P^T
inline bool fx_tile_fills_lds(int tp, int pol) { return fx_lds_bytes(tp, pol, fx_max_slice(tp, pol)) > kLdsOnePerCU; }
// workgroups of k_Pt_tiles_fixed a CU holds at the slice length S
inline int fx_workgroups_per_cu(int tp, int pol, int S) { return fx_lds_bytes(tp, pol, S) <= kLdsTwoPerCU ? 2 : 1; }

// Where every slice's lists begin, from the builders' counting pass.  counts[4 s + {0, 1, 2, 3}] = groups, tail runs,
// tail entries and highest level of slice s (the slices of policy::slices, `sl`).  meta[2 s] = first group, meta[2 s
// + 1] = first tail run | highest level << level_shift, tent_off[s] = first tail entry; entry [nslices] closes the
// lists with the totals.  fits = the offsets hold them: groups and tail entries in 32 bits, tail runs below the level
// field.  mean_groups: groups per full slice (S samples); over: fraction of slices with more groups than `threads`;
// both over the tiles that are not `hot` ([ntiles], 1 = left to the hot-tile path).
struct FxOffsets {
    std::vector<uint32_t> meta, tent_off;
    int64_t ngroups = 0, ntrun = 0, ntent = 0;
    bool fits = false;
    double mean_groups = 0.0, over = 0.0;
};
inline FxOffsets fx_offsets(const std::vector<uint32_t> &counts, const Slices &sl, const std::vector<uint8_t> &hot,
                            int64_t S, int threads, int level_shift)
{
    const int64_t ntiles = (int64_t)sl.slice0.size() - 1, nslices = sl.slice0[(size_t)ntiles];
    FxOffsets r;
    r.meta.assign(2 * ((size_t)nslices + 1), 0);
    r.tent_off.assign((size_t)nslices + 1, 0);
    for (int64_t s = 0; s < nslices; ++s) {
        r.meta[(size_t)(2 * s)] = (uint32_t)r.ngroups;
        r.meta[(size_t)(2 * s + 1)] = (uint32_t)r.ntrun | (counts[(size_t)(4 * s + 3)] << level_shift);
        r.tent_off[(size_t)s] = (uint32_t)r.ntent;
        r.ngroups += counts[(size_t)(4 * s)];
        r.ntrun += counts[(size_t)(4 * s + 1)];
        r.ntent += counts[(size_t)(4 * s + 2)];
    }
    int64_t nfull = 0, nover = 0, ncounted = 0;
    double gsum = 0.0;
    for (int64_t b = 0; b < ntiles; ++b) {
        if (hot[(size_t)b]) continue;
        for (int64_t s = sl.slice0[(size_t)b]; s < sl.slice0[(size_t)b + 1]; ++s) {
            ++ncounted;
            if (counts[(size_t)(4 * s)] > (uint32_t)threads) ++nover;
            if (sl.pairs[(size_t)(2 * s + 1)] - sl.pairs[(size_t)(2 * s)] == S) {
                ++nfull;
                gsum += counts[(size_t)(4 * s)];
            }
        }
    }
    r.meta[(size_t)(2 * nslices)] = (uint32_t)r.ngroups;
    r.meta[(size_t)(2 * nslices + 1)] = (uint32_t)r.ntrun;
    r.tent_off[(size_t)nslices] = (uint32_t)r.ntent;
    r.fits = r.ngroups < ((int64_t)1 << 32) && r.ntent < ((int64_t)1 << 32) && r.ntrun < ((int64_t)1 << level_shift);
    r.mean_groups = nfull ? gsum / (double)nfull : 0.0;
    r.over = ncounted ? (double)nover / (double)ncounted : 0.0;
    return r;
}

// the index range [lo, hi) of the entries of the ascending tile list `asc` that lie in [tile_lo, tile_hi)
struct IndexRange {
    int64_t lo, hi;
};
inline IndexRange tiles_in_range(const std::vector<int64_t> &asc, int64_t tile_lo, int64_t tile_hi)
{
    IndexRange r{0, (int64_t)asc.size()};
    while (r.lo < r.hi && asc[(size_t)r.lo] < tile_lo) ++r.lo;
    while (r.hi > r.lo && asc[(size_t)r.hi - 1] >= tile_hi) --r.hi;
    return r;
}

// a tile that k_Pt_hot takes over: ONE pixel with at least kHotTileMin samples
inline bool is_hot_tile(int64_t pixels, int64_t samples) { return pixels == 1 && samples >= kHotTileMin; }

// the hot tiles of a plan and their sample ranges in time order: `chunk` consecutive samples of the bucket each
struct HotRanges {
    std::vector<uint8_t> flag;           // [ntiles] 1 = hot
    std::vector<int64_t> range;          // [ranges][2] first / one-past-last address
    std::vector<int64_t> tiles;          // [nhot][3] first pixel, first range, range count
    std::vector<int> range_tile;         // [ranges] index of the range's tile in `tiles`
    std::vector<int64_t> hot_tile, hot_chunk0;   // tile index, first range of every hot tile (+ total)
};
inline HotRanges hot_ranges(const std::vector<int64_t> &tile_p0, const std::vector<int64_t> &tile_off, int64_t chunk)
{
    const int64_t ntiles = (int64_t)tile_off.size() - 1;
    HotRanges r;
    r.flag.assign((size_t)ntiles, 0);
    r.hot_chunk0.assign(1, 0);
    for (int64_t b = 0; b < ntiles; ++b) {
        const int64_t a0 = tile_off[(size_t)b], a1 = tile_off[(size_t)b + 1];
        if (!is_hot_tile(tile_p0[(size_t)b + 1] - tile_p0[(size_t)b], a1 - a0)) continue;
        r.flag[(size_t)b] = 1;
        const int64_t c0 = (int64_t)r.range.size() / 2;
        for (int64_t k = a0; k < a1; k += chunk) {
            r.range.push_back(k);
            r.range.push_back(k + chunk < a1 ? k + chunk : a1);
        }
        r.tiles.push_back(tile_p0[(size_t)b]);
        r.tiles.push_back(c0);
        r.tiles.push_back((int64_t)r.range.size() / 2 - c0);
        r.range_tile.resize(r.range.size() / 2, (int)r.hot_tile.size());
        r.hot_tile.push_back(b);
        r.hot_chunk0.push_back((int64_t)r.range.size() / 2);
    }
    return r;
}

// ------------------------------------------------------------------ parts -------
// The simulated machine is the MI355X this library is written for, NOT the live device: part boundaries change the
// order in which a pixel's terms are added, and cm2_tiles.h promises that they depend on the plan only -- the same
// bits on any partition mode or device count.
constexpr int kSimCUs = 256;
// One workgroup alone cannot use more than about 1.5 x its share of the full chip (measured at C4 size: a slice takes
// 3.7 us with 512 workgroups resident, 2.5 us with 51).
constexpr double kSimMaxRate = 1.5;
constexpr double kSimItemCost = 4096.0;  // samples' worth of zeroing and writing the tile copy

// Finish time of `items` (samples each, in dispatch order) over the ideal (total / slots).  `slots` workgroups are
// resident and take the next item as one finishes; the kernel is bandwidth bound, so the resident workgroups share
// the chip's rate equally -- up to kSimMaxRate, which is what makes a few items left over at the end expensive.
inline double parts_makespan(const std::vector<int64_t> &items, int slots)
{
    std::vector<double> heap;                               // min-heap: finish "virtual time" of the active items
    auto cmp = [](double a, double b2) { return a > b2; };
    double V = 0.0, T = 0.0, total = 0.0;                   // virtual time (work done per active item), real time
    size_t next = 0;
    auto rate = [&]() {
        const double fair = (double)slots / (double)(heap.empty() ? 1 : heap.size());
        return fair < kSimMaxRate ? fair : kSimMaxRate;
    };
    for (; next < items.size() && (int)heap.size() < slots; ++next) {
        heap.push_back((double)items[next] + kSimItemCost);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    for (int64_t x : items) total += (double)x + kSimItemCost;
    while (!heap.empty()) {
        const double vf = heap.front();
        T += (vf - V) / rate();
        V = vf;
        std::pop_heap(heap.begin(), heap.end(), cmp);
        heap.pop_back();
        if (next < items.size()) {
            heap.push_back(V + (double)items[next++] + kSimItemCost);
            std::push_heap(heap.begin(), heap.end(), cmp);
        }
    }
    return total > 0.0 ? T * (double)slots / total : 1.0;
}

// parts of a tile of `load` samples in `nslices` slices for the part length `target`: a tile of more than 1.1 x
// target is cut into ceil(load / target) parts, never more parts than slices
inline int64_t parts_of(int64_t load, int64_t nslices, int64_t target)
{
    if (load * 10 <= target * 11 || nslices <= 1) return 1;
    const int64_t k = (load + target - 1) / target;
    return k < nslices ? k : nslices;
}
// part j of k takes the slices [part_slice(ns, j, k), part_slice(ns, j + 1, k)) of the tile's ns: equal slice counts
inline int64_t part_slice(int64_t nslices, int64_t j, int64_t k) { return nslices * j / k; }

// Shares the slices of heavy tiles out to several workgroups (see cm2_tiles.h).  The part length is chosen by
// simulation, for targets between 1.25 and 0.2 of the mean load per resident workgroup; the target with the earliest
// simulated finish wins (fewer parts on a tie).  Parts are dispatched in tile order, i.e. by ascending address:
// dispatched by descending load instead (which scatters the workgroups' streams over the buffers) the same parts took
// 0.45 instead of 0.42 ms at C4 size (profiles/r04_uneven_parts.md).  forced (CM2_PT_PARTS): 0 keeps one workgroup
// per tile, > 0 fixes the target, < 0 chooses.  load[b]: samples of tile b (0 for a hot tile).
struct PartsChoice {
    int64_t target = 0;                  // 0: one workgroup per tile
    std::vector<int64_t> parts;          // [ntiles] parts of every tile
    double makespan = 0.0;               // simulated finish time / ideal of the chosen parts
};
inline PartsChoice choose_parts(const std::vector<int64_t> &load, const std::vector<int64_t> &nslices, int fx_S,
                                int slots, int forced)
{
    PartsChoice c;
    c.parts.assign(load.size(), 1);
    int64_t total = 0;
    for (int64_t x : load) total += x;
    if (forced == 0 || total == 0) return c;
    auto items_for = [&](int64_t target, std::vector<int64_t> &items) {
        items.clear();
        for (size_t b = 0; b < load.size(); ++b) {
            if (load[b] == 0) continue;
            const int64_t k = parts_of(load[b], nslices[b], target);
            for (int64_t j = 0; j < k; ++j) items.push_back(load[b] / k);
        }
    };
    const double per_slot = (double)total / (double)slots;
    int64_t best_target = 0;
    double best = 1e30;
    size_t best_items = 0;
    std::vector<int64_t> items;
    if (forced > 0) {
        best_target = forced;
        items_for(best_target, items);
        best = parts_makespan(items, slots);
    } else {
        // one workgroup per tile is kept unless some split finishes at least 5 % earlier; among the
        // splits the earliest finish, and the fewest parts within 1 % of it
        items_for(INT64_MAX / 16, items);
        const double whole = parts_makespan(items, slots);
        for (int step = 0; step <= 42; ++step) {
            const int64_t target = (int64_t)(per_slot * (1.25 - 0.025 * step)) + 1;
            if (target < 4 * fx_S) break;                   // (parts of a few slices only: not worth a copy)
            items_for(target, items);
            const double mk = parts_makespan(items, slots);
            if (mk < best - 0.01 || (mk < best + 0.01 && items.size() < best_items)) {
                best = mk;
                best_target = target;
                best_items = items.size();
            }
        }
        if (best > 0.95 * whole) best_target = 0;
    }
    if (best_target == 0) return c;
    c.target = best_target;
    c.makespan = best;
    for (size_t b = 0; b < load.size(); ++b)
        if (load[b]) c.parts[b] = parts_of(load[b], nslices[b], best_target);
    return c;
}

}  // namespace policy
}  // namespace cm2
