// cm2_os_policy.h -- the geometry and the host decisions of the overlap-save N^-1: how a block is cut into windows,
// which list format and builder a tile plan gets, buffer-descriptor or flat addressing, the kernel's LDS size.
// Plain C++17, no device, no environment, no state (tests/test_os_policy_cpu.py); the .hip files restate none of it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cm2::os {

// one workgroup: kT threads x kPts complex points in registers = one real window of W samples
constexpr int kT = 256;                 // threads per workgroup
constexpr int kPts = 32;                // complex points per thread
constexpr int kHalo = 2048;             // window halo on both sides (>= lambda - 1)
constexpr int N = kT * kPts;            // complex points (8192)
constexpr int W = 2 * N;                // window samples
constexpr int HOP = W - 2 * kHalo;      // outputs per window (12288)
constexpr int RR = 2;                   // result rounds through the LDS buffer
constexpr int RSLOTS = (kPts - 8) / RR; // register slots per round (m = 4 + j RSLOTS ...)
constexpr int RLEN = 512 * RSLOTS;      // outputs per round
constexpr int NLIST = 2 + RR;           // lists per window: two window halves, results
constexpr int PER = 2 * N + HOP;        // list entries per window
constexpr int LDSD = N + N / 32;        // doubles of the exchange buffer
constexpr int list_off(int l) { return l <= 2 ? l * N : 2 * N + (l - 2) * RLEN; }
constexpr int list_len(int l) { return l < 2 ? N : RLEN; }

struct WinDesc {              // one workgroup's work: HOP (or fewer) outputs of one noise block
    int64_t start, len, lo, hi;
    int32_t blk, pad;
};

// the windows of the noise blocks [off[b], off[b + 1]): HOP outputs each, the last of a block what is left
inline std::vector<WinDesc> windows(const std::vector<int64_t> &off)
{
    std::vector<WinDesc> wins;
    for (size_t b = 0; b + 1 < off.size(); ++b)
        for (int64_t s0 = off[b]; s0 < off[b + 1]; s0 += HOP)
            wins.push_back({s0, off[b + 1] - s0 < HOP ? off[b + 1] - s0 : HOP, off[b], off[b + 1], (int32_t)b, 0});
    return wins;
}

// run-table words per list: one run per pixel tile at most (k_real_rc / k_real_lists); 0 tiles = unknown
inline int rmax(int64_t ntiles)
{
    const int64_t bound = ntiles > 0 && ntiles < N ? ntiles : N;
    return (int)((bound + 63) / 64 * 64);              // (64 at least: bound >= 1)
}

// The two run tables of a list pair live in LDS beside the exchange buffer: run-coded and inverse lists up to
// kTabRows table words per thread (2048 runs a list), plain lists beyond that.
constexpr int kTabRows = 8;
inline bool table_fits(int rmax_) { return rmax_ <= kTabRows * kT; }

// List format (1 plain, 2 run-coded, 3 inverse) and builder of a tile plan.  `want_lists`: CM2_OS_LISTS = auto (0)
// | plain (1) | rc (2) | inv (3).  Auto: lists cut by time (2) keep the pick / place side cheap and win while a half
// window's address runs are long (512 tiles at C4: 16 entries); from ~768 tiles up the longer runs and whole sectors
// of the lists cut by address (3) win: C5's 1536 tiles 1.24 -> 1.05 ms, the balanced tiling of an uneven hit map
// (1015 tiles) 0.92 -> 0.87 ms, 512 tiles 0.76 -> 0.79 ms (profiles/r03_inverse_lists.md).  The direct builders
// keep per-tile counters in LDS and need the tile offsets; everything else goes through the segmented sort
// (`build_sort`: CM2_OS_LIST_BUILD=sort), which never yields inverse lists.
enum class Builder { sorted, direct, inverse };
struct ListChoice { Builder builder; int mode, rmax; };
inline ListChoice choose_lists(int want_lists, bool build_sort, bool has_tile_off, int64_t ntiles)
{
    const int want = want_lists ? want_lists : (ntiles >= 768 ? 3 : 2);
    const bool direct = !build_sort && has_tile_off && ntiles > 0 && ntiles <= 4096;
    const int r = rmax(ntiles);
    const Builder b = !direct ? Builder::sorted : (want == 3 && table_fits(r) ? Builder::inverse : Builder::direct);
    return {b, b == Builder::inverse ? 3 : (want >= 2 && table_fits(r) ? 2 : 1), r};
}

// Bytes of the descriptors over the tile-order buffers of `nvalid` doubles; 0: flat (4 GB up, unknown, CM2_OS_FLAT)
inline uint32_t descriptor_bytes(int64_t nvalid, bool flat)
{
    return nvalid > 0 && nvalid * 8 < (int64_t)0xFFFFFFF0u && !flat ? (uint32_t)(nvalid * 8) : 0u;
}

// dynamic LDS of k_os_real: exchange plane, the two run tables of a list pair, 2 KB for the lower slots of the
// eight self-paired threads of the half-plane pairing
inline size_t kernel_lds_bytes(int mode, int rmax_)
{
    return sizeof(double) * (size_t)LDSD + (mode >= 2 ? sizeof(uint32_t) * 2 * (size_t)rmax_ : 0) + 2048;
}

}  // namespace cm2::os
