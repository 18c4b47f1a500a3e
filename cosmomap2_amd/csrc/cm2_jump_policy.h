// cm2_jump_policy.h -- the device-free arithmetic of the jump corrector (cm2_jump.hip): which arguments are accepted,
// how workgroups are laid over the noise blocks, and what one tile of the statistic kernel holds in LDS.  Plain C++:
// tests/test_jump_cpu.py compiles it with the host compiler and checks it against Python.
//
// cm2_stream_policy.h has the blocks, their tiles of kTile samples and the checks every stage shares; its names are
// reachable as cm2::jump:: too.  Workgroup g takes tile g in every kernel, so one workgroup sees one block only.
//
// Statistic.  The t of the positions [first, end) of a tile needs the window sums S_j of the starts j = first - w ..
// end - 1 (R_i = S_i, L_i = S_{i-w}), and those the samples first - w .. end + w - 2.  A workgroup stages
// stat_values(w) masked values (kStarts x kTileThreads starts, each w samples long), the running count of the usable
// ones among them, and the stat_starts() sums.
#pragma once
#include <cstdint>

#include "cm2_stream_policy.h"

namespace cm2 {
namespace jump {

using namespace stream;

constexpr int kMaxWindow = 256;            // 1 <= w <= 256, the half-window: w samples on either side of a position
constexpr int kMaxRadius = 256;
constexpr int kTileThreads = 256;
constexpr int kCounts = 3;                 // counts[b][CLEAN, AT, NEAR]
constexpr int64_t kLdsLimit = 64 * 1024;   // of one workgroup

// the classes a pass adds (CM2_JUMP_* of include/cosmomap2.h)
enum Class { kClean = 0, kAt = 1, kNear = 2 };

// the codes of this stage beside the shared ones (kBadWindow: w outside [1, 256])
constexpr Status kBadRadius = Status(7);           // outside [0, 256]
constexpr Status kBadMinCount = Status(9);         // outside [1, w]
constexpr Status kBadCapacity = Status(10);        // < 1

// ---- one tile of the statistic kernel -----------------------------------------------------------------------------
// window starts a thread sums, all at once (independent chains of additions): ceil((kTile + kMaxWindow) / threads)
constexpr int kStarts = (kTile + kMaxWindow + kTileThreads - 1) / kTileThreads;
constexpr int stat_starts() { return kStarts * kTileThreads; }
// staged values: the last start reads w - 1 samples beyond itself
constexpr int stat_values(int w) { return stat_starts() + w; }
// values (8 bytes), sums (8 bytes), running usable counts (2 bytes, one more than the values, rounded up to 8 bytes)
constexpr int64_t stat_lds_bytes(int w)
{
    return (int64_t)stat_values(w) * 8 + (int64_t)stat_starts() * 8 + (((int64_t)stat_values(w) + 1) * 2 + 7) / 8 * 8;
}
// |t| of a tile and its halo of w on either side, the peaks kernel
constexpr int64_t peaks_lds_bytes() { return (int64_t)(kTile + 2 * kMaxWindow) * 8; }

static_assert(kStarts * kTileThreads >= kTile + kMaxWindow, "every start of a tile has a thread");
static_assert(stat_values(kMaxWindow) < 65536, "the running counts fit 16 bits");
static_assert(stat_lds_bytes(kMaxWindow) <= kLdsLimit && peaks_lds_bytes() <= kLdsLimit, "one workgroup's LDS");

struct Launch {
    int64_t nt = 0, nblocks = 0, tiles = 0;
    int w = 0;
    int64_t lds_bytes = 0;
};

// fills *l; anything but kOk leaves it unspecified
inline Status check_create(Launch *l, int64_t nt, const int64_t *sizes, int64_t nblocks, int half_window)
{
    const Status st = check_blocks(nt, sizes, nblocks, half_window >= 1 && half_window <= kMaxWindow);
    if (st != kOk) return st;
    l->nt = nt;
    l->nblocks = nblocks;
    l->tiles = total_units(sizes, nblocks, kTile);
    l->w = half_window;
    l->lds_bytes = stat_lds_bytes(half_window);
    return kOk;
}

inline Status check_stat(int w, bool have_flags, int kind, int min_count)
{
    if (check_flag_kind(have_flags, kind) != kOk) return kBadFlagKind;
    if (min_count < 1 || min_count > w) return kBadMinCount;
    return kOk;
}

inline Status check_find(double nsigma, int64_t capacity)
{
    if (check_nsigma(nsigma) != kOk) return kBadNsigma;
    if (capacity < 1) return kBadCapacity;
    return kOk;
}

inline Status check_correct(int radius, int64_t capacity)
{
    if (radius < 0 || radius > kMaxRadius) return kBadRadius;
    if (capacity < 1) return kBadCapacity;
    return kOk;
}

// entries of the ascending table pos[0, n) that are < x (lower) or <= x (upper)
constexpr int64_t table_lower(const int64_t *pos, int64_t n, int64_t x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
constexpr int64_t table_upper(const int64_t *pos, int64_t n, int64_t x) { return table_lower(pos, n, x + 1); }

}  // namespace jump
}  // namespace cm2
