// cm2_fx_lists.h -- internal to the fixed-order P^T: what its plan-time list builders (cm2_fx_lists.hip) write and
// its kernel (k_Pt_tiles_fixed, cm2_tiles_fixed.hip) reads, and the builders' two entry points.
#pragma once
#include "cm2_tiles.h"

namespace cm2 {

constexpr int kFxT = policy::kFxThreads;        // threads = groups per slice handled in one round
constexpr int kFxMaxLevel = 14;                 // pieces of 4: runs up to 60 samples go into groups
constexpr uint32_t kFxNull = 0xFFFFFFFFu;       // an empty slot of a group

// pixel-in-tile bits of a pl word: bit 15 is the sign of cos when the plan stores half angles
constexpr uint32_t fx_pixel_mask(bool half) { return half ? 0x7FFFu : 0xFFFFu; }

// A list entry: pl word (pixel in tile, sign of cos) | offset in the slice << 16 | level << 28.  The offset has 12
// bits (slices of up to 4 kFxT = 2048 samples); piece p of a run cut into pieces of 4 carries level p.
constexpr int kFxOffsetShift = 16, kFxLevelShift = 28;
constexpr uint32_t kFxOffsetMask = 0xFFFu, kFxLevelMask = 15u;
static_assert(kFxMaxLevel <= (int)kFxLevelMask && 4 * kFxT <= (int)kFxOffsetMask + 1, "entry word: level and offset fit");

// meta of a slice: .x = first group, .y = first tail run | highest level of the slice << 28 (the level field of the
// entry word: policy::fx_offsets packs it with kFxLevelShift)
constexpr uint32_t kFxRunMask = (1u << kFxLevelShift) - 1;      // .y & kFxRunMask, .y >> kFxLevelShift

// a tile that k_Pt_hot takes over (hot_plan): its slices do not count when the slice length is tuned
inline bool fx_hot_tile(const cm2_tiles *t, int64_t b)
{
    return policy::is_hot_tile(t->tile_p0[(size_t)b + 1] - t->tile_p0[(size_t)b], t->tile_count[(size_t)b]);
}

// groups per full slice of S samples and the fraction of slices with more groups than threads,
// from every 8th full slice (k_fx_build's counting pass on ~12 % of the samples): the slice length
// is chosen from this before anything is allocated or written
int fx_count_sample(const cm2_tiles *t, int S, hipStream_t st, double *mean_groups, double *over);

// Fills t->fx (empty on entry) for slices of S samples, with one workgroup per slice or, for the plan's fx_serial
// switch, the radix sort and the one-thread-per-slice packer: other lists, the same sums.  *mean_groups = average
// groups per full slice, *over = fraction of slices with more groups than threads.  Launches on st and waits for it.
int fx_build_lists(cm2_tiles *t, int S, hipStream_t st, double *mean_groups, double *over);

}  // namespace cm2
