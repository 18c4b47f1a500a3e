// cm2_glitch_policy.h -- the device-free arithmetic of the glitch flagger (cm2_glitch.hip): which arguments are
// accepted, which tier a half-width takes and what it costs in registers or LDS, how threads and workgroups are laid
// over the noise blocks, and the digit split of the rank selection.  Plain C++: tests/test_glitch_cpu.py compiles it
// with the host compiler and checks it against Python.
//
// cm2_stream_policy.h has the blocks, the units they are cut into and the checks every stage shares; its names are
// reachable as cm2::glitch:: too.  The median walks *runs*, units of kRun samples, one per thread; the selection and
// the classes take *tiles*, one per workgroup: a workgroup sees one block only, and its LDS histogram and class tally
// belong to that block.
#pragma once
#include <cstdint>

#include "cm2_stream_policy.h"

namespace cm2 {
namespace glitch {

using namespace stream;

constexpr int kMaxHalfWidth = 64;          // 1 <= h <= 64, the window is W = 2 h + 1 <= 129 samples
constexpr int kMaxGrow = 64;
constexpr int kRun = 64;                   // consecutive outputs of one thread of the median kernel
constexpr int kChunk = 8;                  // steps whose keys the median kernel stages through LDS at a time
constexpr int kTileThreads = 256;
constexpr int kClasses = 5;

// the classes of a sample (CM2_GLITCH_* of include/cosmomap2.h)
enum Class { kClean = 0, kInput = 1, kNonfinite = 2, kHit = 3, kNear = 4 };

// the codes of this stage beside the shared ones
constexpr Status kBadHalfWidth = kBadWindow;       // h outside [1, 64]
constexpr Status kBadGrow = Status(7);             // outside [0, 64]

// ---- tiers of the half-width ------------------------------------------------------------------------------------
// Tiers 0-3 keep the window of a thread in registers, kSlots doubles in fully unrolled sweeps (a smaller window is
// padded with +inf keys); tier 4 keeps the first 96 keys of the window it was asked for in registers and the other
// W - 96 in LDS, [slot][thread].
constexpr int kTiers = 5;
constexpr int tier_of(int h) { return h <= 8 ? 0 : h <= 16 ? 1 : h <= 32 ? 2 : h <= 48 ? 3 : 4; }
constexpr int tier_max_h(int tier) { return tier == 0 ? 8 : tier == 1 ? 16 : tier == 2 ? 32 : tier == 3 ? 48 : 64; }
constexpr int tier_slots(int tier) { return 2 * tier_max_h(tier) + 1; }
constexpr bool tier_in_registers(int tier) { return tier < 4; }
constexpr int tier_threads(int) { return 64; }      // one wave: a barrier costs nothing, LDS is granted per wave
// slots of a thread that live in registers
constexpr int tier_register_slots(int tier) { return tier_in_registers(tier) ? tier_slots(tier) : 96; }
// 32-bit registers the keys of one thread take
constexpr int tier_key_registers(int tier) { return 2 * tier_register_slots(tier); }
// LDS of one workgroup that every tier takes: three staged chunks of keys and four positions per row
constexpr int64_t stage_lds_bytes(int tier)
{
    return (int64_t)tier_threads(tier) * (3 * (kChunk + 1) * (int64_t)sizeof(double) + 4 * (int64_t)sizeof(int64_t));
}
// dynamic LDS of one workgroup on top of that
constexpr int64_t tier_lds_bytes(int tier, int h)
{
    return tier_in_registers(tier) ? 0
        : (int64_t)(2 * h + 1 - tier_register_slots(tier)) * tier_threads(tier) * (int64_t)sizeof(double);
}

// ---- the digit split of the selection ---------------------------------------------------------------------------
// The key of a usable sample is the bit pattern of |r|, 63 bits (the sign bit is 0); non-negative doubles order as
// unsigned integers.  Pass p fixes the bits [digit_shift(p), digit_shift(p) + digit_bits(p)), most significant first.
constexpr int kDigits = 6;
constexpr int kMaxBins = 2048;             // bins of one block's histogram (the widest digit)
constexpr int digit_bits(int p) { return p == 0 ? 8 : 11; }
constexpr int digit_shift(int p) { return p == 0 ? 55 : 11 * (5 - p); }
constexpr int digit_bins(int p) { return 1 << digit_bits(p); }
// the bits fixed before pass p
constexpr uint64_t prefix_mask(int p)
{
    return p == 0 ? 0 : (~(uint64_t)0 << (digit_shift(p) + digit_bits(p))) & ~((uint64_t)1 << 63);
}

// ---- layout -----------------------------------------------------------------------------------------------------
constexpr int64_t runs_of(int64_t size) { return units_of(size, kRun); }
constexpr int64_t workgroups_for(int64_t units, int threads) { return (units + threads - 1) / threads; }

// run g of the stream
constexpr Span run_span(const int64_t *off, const int64_t *run_start, int64_t nblocks, int64_t g)
{
    return unit_span(off, run_start, nblocks, kRun, g);
}

struct Launch {
    int64_t nt = 0, nblocks = 0, runs = 0, tiles = 0;
    int h = 0, tier = 0, threads = 0;
    int64_t median_blocks = 0, lds_bytes = 0, hist_bytes = 0;
};

// fills *l; anything but kOk leaves it unspecified
inline Status check_create(Launch *l, int64_t nt, const int64_t *sizes, int64_t nblocks, int half_width)
{
    const Status st = check_blocks(nt, sizes, nblocks, half_width >= 1 && half_width <= kMaxHalfWidth);
    if (st != kOk) return st;
    l->nt = nt;
    l->nblocks = nblocks;
    l->runs = total_units(sizes, nblocks, kRun);
    l->tiles = total_units(sizes, nblocks, kTile);
    l->h = half_width;
    l->tier = tier_of(half_width);
    l->threads = tier_threads(l->tier);
    l->median_blocks = workgroups_for(l->runs, l->threads);
    l->lds_bytes = tier_lds_bytes(l->tier, half_width);
    l->hist_bytes = nblocks * kMaxBins * (int64_t)sizeof(uint32_t);
    return kOk;
}

inline Status check_classify(double nsigma, int grow)
{
    if (check_nsigma(nsigma) != kOk) return kBadNsigma;
    if (grow < 0 || grow > kMaxGrow) return kBadGrow;
    return kOk;
}

}  // namespace glitch
}  // namespace cm2
