// cm2_tiles.h -- the tile-bucketed pointing plan.  Written by cm2_tiles.hip (plan, P, atomic P^T,
// permutations), cm2_tiles_fixed.hip (fixed-order P^T) and cm2_fx_lists.hip (its list builders); read by
// the units that work on a TOD in the plan's order: cm2_gaps.hip, cm2_noise.hip and cm2_filter.hip
// (index, offsets, counts and the plan's id)
#pragma once
#include "cm2_pixindex.h"
#include "cm2_plan_policy.h"

#include <functional>
#include <vector>

namespace cm2 {
// The switches that steer a tile plan and its fixed-order P^T lists.  Read from the environment ONCE,
// by cm2_tiles_create (read_plan_switches, cm2_tiles.hip), and kept in the plan: lists that are
// built later (cm2_tiles_prepare_pt, the first P^T) follow the switches of the plan's creation.
struct PlanSwitches {
    int pt_order = 1;            // CM2_PT_ORDER: atomic = 0, exact = 2, fixed or anything else = 1 (default)
    bool tile_sort = false;      // CM2_TILE_BUILD=sort: radix sort + gather instead of the multisplit
    policy::Balance balance = policy::Balance::automatic;   // CM2_TILE_BALANCE: parts | cut or a non-zero
                                 // number = cut | anything else (0) = off; not set = automatic
    bool full_angles = false;    // CM2_TILE_ANGLES=full: cos and sin arrays, no half-angle storage
    bool fx_serial = false;      // CM2_FX_BUILD=serial: the reference builders of the lists (global tile order only)
    int pt_slice = 0;            // CM2_PT_SLICE=<samples in [64, 2048]>: fixes the slice length (0: tuned)
    int pt_parts = -1;           // CM2_PT_PARTS: 0 = one workgroup per tile, <samples> fixes the part length (-1: chosen)
    bool pt_fuse = true;         // CM2_PT_FUSE=0 (or no number): hot ranges and part copies in kernels of their own
};

// The state of the fixed-order P^T in three parts, each the owner of its device buffers: reset() (and the
// destructor) frees them, so that no table of pointers has to be kept in step with the fields.

// fixed-order P^T (cm2_tiles_fixed.hip), built on first use: every tile bucket is cut into
// slices of S consecutive TB samples; per slice the samples sorted by (pixel, time) are
// packed into groups of 4 list entries that hold whole runs (= samples of one pixel).  The formats of the
// entry word and of meta: cm2_fx_lists.h.
struct FxLists : NoCopy {
    int S = 0;
    int64_t *d_slice0 = nullptr;     // [ntiles+1] first slice of every tile
    uint2 *d_sk = nullptr;           // [nslices+1] {first TB position, samples} of every slice
    uint2 *d_meta = nullptr;         // [nslices+1] {first group, first tail run | max level << 28}
    uint4 *d_gent = nullptr;         // [ngroups] 4 entries: pl word | offset in slice << 16 | level << 28
    double *d_ga = nullptr, *d_gb = nullptr;   // [4 ngroups] half angle (or cos, sin)
    uint2 *d_trun = nullptr;         // [ntail runs + 1] {first tail entry, pixel in tile}
    uint32_t *d_tent = nullptr;      // [ntail entries] entries of the runs kept out of the groups
    double *d_ta = nullptr, *d_tb = nullptr;
    int64_t ngroups = 0, nslices = 0;
    ~FxLists() { reset(); }
    void reset()
    {
        dev_release(d_slice0, d_sk, d_meta, d_gent, d_ga, d_gb, d_trun, d_tent, d_ta, d_tb);
        S = 0;
        ngroups = nslices = 0;
    }
};

// PARTS of the fixed-order P^T (round 4, cm2_tiles_fixed.hip): on a hit map that is far from
// uniform the tiles keep their width (only a pixel heavy enough for the hot-tile path becomes a
// tile of its own) and the SLICES of a heavy tile are shared out to several workgroups, each
// summing its consecutive slices in time order into its own copy of the tile; k_parts_combine adds
// the copies in time order.  Part boundaries depend on the plan only: reproducible bit for bit;
// a regrouped sum, ~1e-16 relative away from the serial one.  cm2_tiles::pt_split = the plan may do this
// (set at create: unbalanced hit map, neither the equal-load cut nor the exact order asked for).
struct FxParts : NoCopy {
    std::vector<int64_t> tile_part0;    // [ntiles+1] first part of every tile (empty: no parts)
    std::vector<int64_t> multi_tile;    // tiles with more than one part, ascending
    int4 *d_parts = nullptr;            // [nparts] {tile, slices, first slice, scratch slot or -1}
    int64_t *d_multi = nullptr;         // [nmulti][4] offset in the map, values, first scratch slot, parts
    double *d_buf = nullptr;            // [scratch slots][tp * pol]
    int64_t nparts = 0, slots = 0;
    double makespan = 0.0;              // simulated finish time / ideal, 2 workgroups per CU
    ~FxParts() { reset(); }
    void reset()
    {
        dev_release(d_parts, d_multi, d_buf);
        tile_part0.clear();
        multi_tile.clear();
        nparts = slots = 0;
        makespan = 0.0;
    }
};

// hot tiles of the fixed-order P^T: a tile that is ONE pixel with very many samples (a stare at
// a source; the balanced tiling makes such a pixel a tile of its own) is reduced by many
// workgroups, each summing a fixed range of kHotChunk consecutive samples of the bucket, and
// the range sums are added in time order (cm2_tiles_fixed.hip)
struct FxHot : NoCopy {
    std::vector<int64_t> tile, chunk0;       // tile index, first chunk of every hot tile (+ total)
    uint8_t *d_flag = nullptr;               // [ntiles]
    int64_t *d_range = nullptr;              // [chunks][2] first / one-past-last TB position
    int64_t *d_tiles = nullptr;              // [nhot][3] first pixel, first chunk, chunk count
    double *d_partial = nullptr;             // [chunks][3]
    // FUSED form (round 5): the ranges of a hot tile are work items at the end of the main launch and their
    // sums are added up by the last range to finish (cm2_tiles_fixed.hip, FxFused)
    void *d_fused = nullptr;                 // FxFused (device copy)
    int *d_range_tile = nullptr;             // [chunks] index of the range's tile in d_tiles
    unsigned int *d_count = nullptr;         // [nhot] arrival counters, zeroed before every launch
    size_t count_bytes = 0;
    ~FxHot() { reset(); }
    void reset()
    {
        dev_release(d_flag, d_range, d_tiles, d_partial, d_fused, d_range_tile, d_count);
        tile.clear();
        chunk0.clear();
        count_bytes = 0;
    }
};
}  // namespace cm2

struct cm2_tiles {
    cm2::PlanSwitches sw;
    int64_t nt = 0, npix = 0, nvalid = 0;
    int pol = 0;
    int tp = 0;                  // pixels per tile (the largest width when the tiles are balanced)
    bool balanced = false;       // the tiles are not the uniform grid: boundaries are read from tile_p0
    std::vector<int64_t> tile_p0;   // [ntiles+1] first pixel of every tile (host)
    int64_t *d_tile_p0 = nullptr;
    int64_t ntiles = 0, nitems = 0;
    // tile b's bucket = the addresses [tile_off[b], tile_off[b + 1])
    std::vector<int64_t> tile_off;  // [ntiles+1] first address of every tile (host)
    int64_t *d_tile_off = nullptr;
    uint32_t *d_tb_dst = nullptr;   // [nt]
    uint16_t *d_pl = nullptr;       // [nvalid]
    double *d_cos = nullptr, *d_sin = nullptr;   // [nvalid]  (full-angle mode)
    // half-angle mode: ONE double per sample, h = sin / (1 + |cos|) (= tan of half the angle
    // folded into [-1, 1]) and the sign of cos in bit 15 of d_pl; cos = +-(1 - h^2)/(1 + h^2),
    // sin = 2h/(1 + h^2) are rebuilt in the kernels (absolute error <= 3.4e-16): 8 bytes less per
    // sample in each of the two tile kernels
    bool half = false;
    double *d_half = nullptr;                    // [nvalid]
    // work items of k_P_tiles / k_Pt_tiles: tile and the addresses [k0, k1) of its bucket (a bucket
    // longer than the slice length is cut into several items)
    int32_t *d_item_tile = nullptr; // [nitems]
    int64_t *d_item_k0 = nullptr;   // [nitems]
    int64_t *d_item_k1 = nullptr;
    std::vector<int64_t> tile_item0;   // [ntiles+1] first work item of every tile (host)
    // address-sorted lists of the windowed permutations (built on first use): for every window
    // of kPermWin consecutive time samples, its samples' TB positions in ascending order and
    // their offsets in the window
    uint32_t *d_perm_k = nullptr;
    uint16_t *d_perm_q = nullptr;
    int64_t nperm_win = 0;
    // identity of this plan for the caches other objects key on it (noise / filter lists): a
    // device address can be reused by a later plan, a plan id cannot
    uint64_t plan_id = 0;
    // fixed-order P^T (cm2_tiles_fixed.hip), built on first use: lists, hot tiles and parts below
    int pt_fixed = 1;
    int fx_failed = 0;       // a build of the fixed-order lists failed: not retried on every apply
    std::vector<int64_t> tile_count;    // [ntiles] valid samples of every tile (host)
    bool pt_split = false;   // the plan may share a heavy tile's slices out to parts (FxParts)
    cm2::FxLists fx;
    cm2::FxParts parts;
    cm2::FxHot hot;
};

namespace cm2 {
int fx_plan(const cm2_tiles *t, hipStream_t st, bool *use);
int fx_launch(const cm2_tiles *t, const double *d_tod_tb, double *d_out, int64_t tile_lo,
              int64_t tile_hi, hipStream_t stream);
void fx_free(cm2_tiles *t);
int64_t fx_designed_bytes(const cm2_tiles *t);
int fx_parts_info(const cm2_tiles *t, int64_t *h_info);   // cm2_tiles_pt_parts

// Windowed exchange between time and tile order: a workgroup of kPermT threads owns kPermWin consecutive time
// samples and reaches their tile-order positions through an address-sorted list.  The list format and the device
// pieces that read it: cm2_perm_window.h.  perm_lists builds the plan's lists d_perm_k / d_perm_q on first use
// (allocates, synchronises); *use = false for a TOD shorter than one window, which keeps the per-sample kernels.
constexpr int kPermWin = 8192, kPermT = 256, kPermPer = kPermWin / kPermT;
int perm_lists(const cm2_tiles *t, hipStream_t st, bool *use);

// The builder of window lists (cm2_tiles.hip).  fill_keys launches the caller's kernel that writes, for every slot
// g < nwin kPermWin, keys[g] = (window << 32) | tile-order position (kInvalidSample: none) and vals[g] = offset in
// the window; the slots are sorted by key and come back as *lst_k (the keys' low words) and *lst_q, which the caller
// owns.  Synchronises; on failure nothing is left allocated.
int window_lists(int64_t nwin, hipStream_t st, const std::function<void(uint64_t *keys, uint16_t *vals)> &fill_keys,
                 uint32_t **lst_k, uint16_t **lst_q);

// "Does this handle flag the same samples as the plan?"  launch_compare launches the caller's kernel around
// flag_mismatch (cm2_perm_window.h) on the word it is given; *first = the smallest sample whose flag differs,
// kInvalidSample when there is none.
int first_flag_mismatch(hipStream_t st, const std::function<void(uint32_t *d_first)> &launch_compare, uint32_t *first);
}  // namespace cm2

