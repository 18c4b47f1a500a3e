// cm2_glitch_policy.h -- the device-free arithmetic of the glitch flagger (cm2_glitch.hip): which arguments are
// accepted, which tier a half-width takes and what it costs in registers or LDS, how threads and workgroups are laid
// over the noise blocks, and the digit split of the rank selection.  Plain C++: tests/test_glitch_cpu.py compiles it
// with the host compiler and checks it against Python.
//
// The stream is nblocks noise blocks one after the other, block b the samples [off[b], off[b + 1]).
//
// Median.  A *run* is kRun consecutive samples of one block (the last run of a block may be shorter); block b has
// runs_of(size_b) of them and the runs of the stream are numbered block after block, run_start[b] the first of block
// b.  Global thread g (workgroup w, thread t: g = w threads + t) walks run g: no thread crosses a block, every sample
// belongs to exactly one run, and blocks of any size pack the threads densely.
//
// Selection and classes.  A *tile* is kTile consecutive samples of one block (the last may be shorter), numbered the
// same way with tile_start[b]; workgroup w takes tile w.  One workgroup therefore sees one block only, and its LDS
// histogram and class tally belong to that block.
#pragma once
#include <cstdint>

namespace cm2 {
namespace glitch {

constexpr int kMaxHalfWidth = 64;          // 1 <= h <= 64, the window is W = 2 h + 1 <= 129 samples
constexpr int kMaxGrow = 64;
constexpr int kRun = 64;                   // consecutive outputs of one thread of the median kernel
constexpr int kChunk = 8;                  // steps whose keys the median kernel stages through LDS at a time
constexpr int kTile = 2048;                // samples of one workgroup of the histogram and class kernels
constexpr int kTileThreads = 256;
constexpr int kClasses = 5;

// the classes of a sample (CM2_GLITCH_* of include/cosmomap2.h)
enum Class { kClean = 0, kInput = 1, kNonfinite = 2, kHit = 3, kNear = 4 };

enum Status {
    kOk = 0,
    kBadSize = 1,          // nt < 1, nblocks < 1 or no sizes
    kBadBlocks = 2,        // a size < 1, or the sizes do not add up to nt
    kBadHalfWidth = 3,     // h outside [1, 64]
    kTooLarge = 4,         // nt >= 2^32 - 1 (the limit of cm2_gaps)
    kTooManyBlocks = 5,    // nblocks > kMaxBlocks: the histograms would pass 2 GB
    kBadNsigma = 6,        // not finite or <= 0
    kBadGrow = 7,          // outside [0, 64]
    kBadFlagKind = 8       // flags given with a kind other than 0 or 1
};

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

constexpr int64_t kMaxBlocks = (int64_t)1 << 18;          // 2^18 x 2048 x 4 bytes = 2 GB of histograms

// ---- layout -----------------------------------------------------------------------------------------------------
constexpr int64_t runs_of(int64_t size) { return (size + kRun - 1) / kRun; }
constexpr int64_t tiles_of(int64_t size) { return (size + kTile - 1) / kTile; }
constexpr int64_t workgroups_for(int64_t units, int threads) { return (units + threads - 1) / threads; }

// the block of unit u: the largest b in [0, nblocks) with start[b] <= u; start[0] = 0 and start ascends strictly
// (every block has at least one sample).  (constexpr: callable from device code as well)
constexpr int64_t locate(const int64_t *start, int64_t nblocks, int64_t u)
{
    int64_t lo = 0, hi = nblocks;              // start[lo] <= u < start[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

struct Span {
    int64_t block = 0, first = 0, end = 0;     // the samples [first, end) of the stream, all of one block
};

// run g of the stream
constexpr Span run_span(const int64_t *off, const int64_t *run_start, int64_t nblocks, int64_t g)
{
    Span s;
    s.block = locate(run_start, nblocks, g);
    s.first = off[s.block] + (g - run_start[s.block]) * kRun;
    s.end = s.first + kRun < off[s.block + 1] ? s.first + kRun : off[s.block + 1];
    return s;
}

// tile w of the stream
constexpr Span tile_span(const int64_t *off, const int64_t *tile_start, int64_t nblocks, int64_t w)
{
    Span s;
    s.block = locate(tile_start, nblocks, w);
    s.first = off[s.block] + (w - tile_start[s.block]) * kTile;
    s.end = s.first + kTile < off[s.block + 1] ? s.first + kTile : off[s.block + 1];
    return s;
}

struct Launch {
    int64_t nt = 0, nblocks = 0, runs = 0, tiles = 0;
    int h = 0, tier = 0, threads = 0;
    int64_t median_blocks = 0, lds_bytes = 0, hist_bytes = 0;
};

// fills *l; anything but kOk leaves it unspecified.  nt < 2^32 - 1 keeps the run and tile counts (grid dimensions)
// below 2^31 and every count of a histogram in 32 bits.
inline Status check_create(Launch *l, int64_t nt, const int64_t *sizes, int64_t nblocks, int half_width)
{
    if (nt < 1 || nblocks < 1 || !sizes) return kBadSize;
    if (half_width < 1 || half_width > kMaxHalfWidth) return kBadHalfWidth;
    if (nt >= (((int64_t)1 << 32) - 1)) return kTooLarge;
    if (nblocks > nt) return kBadBlocks;
    int64_t sum = 0, runs = 0, tiles = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (sizes[b] < 1 || sizes[b] > nt - sum) return kBadBlocks;
        sum += sizes[b];
        runs += runs_of(sizes[b]);
        tiles += tiles_of(sizes[b]);
    }
    if (sum != nt) return kBadBlocks;
    if (nblocks > kMaxBlocks) return kTooManyBlocks;
    l->nt = nt;
    l->nblocks = nblocks;
    l->runs = runs;
    l->tiles = tiles;
    l->h = half_width;
    l->tier = tier_of(half_width);
    l->threads = tier_threads(l->tier);
    l->median_blocks = workgroups_for(runs, l->threads);
    l->lds_bytes = tier_lds_bytes(l->tier, half_width);
    l->hist_bytes = nblocks * kMaxBins * (int64_t)sizeof(uint32_t);
    return kOk;
}

inline Status check_flag_kind(bool have_flags, int kind)
{
    return have_flags && kind != 0 && kind != 1 ? kBadFlagKind : kOk;
}

inline Status check_classify(double nsigma, int grow)
{
    if (!(nsigma > 0.0) || !(nsigma <= 1.7976931348623157e308)) return kBadNsigma;
    if (grow < 0 || grow > kMaxGrow) return kBadGrow;
    return kOk;
}

}  // namespace glitch
}  // namespace cm2
