// cm2_os_lists.h -- internal to the overlap-save N^-1: the address lists of an (operator, tile plan) pair as
// k_os_real (cm2_overlap_save.hip) reads them and the plan-time builders (cm2_os_lists.hip) write them.
#pragma once
#include "cm2_os_policy.h"
#include "cm2_overlap_save.h"

namespace cm2 {

using os::kT, os::kPts, os::kHalo, os::kTabRows, os::WinDesc;      // (spelled without the prefix in both units)

struct ListHdr {              // one run-coded list
    uint32_t nvalid;          // entries with a sample (they come first: invalid keys sort last)
    uint32_t nruns;
    int32_t wbase[4];         // run index in front of each wave's first slot (-1: none)
    uint32_t pad[2];
};

struct IListHdr {             // one inverse list
    uint32_t nvalid, nruns;
    int32_t wbase[16];        // [round][wave] (4 or 8 waves a workgroup): run index in front of the wave's
                              // first slot of the round
};

// Slot of entry u of this thread in a list of E entries per thread: every wave owns a contiguous
// range of the list, a wave instruction covers 64 consecutive slots.
template <int E>
__device__ __forceinline__ int slot_of(int t, int u) { return 64 * (E * (t >> 6) + u) + (t & 63); }

// Where the 16-bit word of slot s of a list with E entries per thread is STORED: the words of a
// thread's entries 4i .. 4i+3 share one 8-byte word, word (E/4 wave + i) 64 + lane of the list, so a
// thread fetches its E words with E/4 coalesced 8-byte loads into E/2 registers (one 2-byte load and
// one register per entry before round 4: the 24-32 list words held across the last transform pass
// were what pushed the kernel over 256 VGPRs).  The plan-time kernels write through this map.
__host__ __device__ inline int q_index(int s, int E)
{
    const int row = s >> 6, lane = s & 63, w = row / E, u = row % E;
    return (((E / 4) * w + (u >> 2)) * 64 + lane) * 4 + (u & 3);
}

// The address lists of one (noise operator, tile plan) pair, over the operator's windows.  Owned by a
// shared_ptr: an application holds a reference while it launches, so a concurrent eviction cannot free
// lists that a launch is about to use (dev_free waits for the device before a block can be handed out
// again).
struct OsLists {
    uint64_t plan_id = 0;
    int mode = 0;                        // 1 plain, 2 run-coded (cut by time), 3 inverse (cut by address)
    uint32_t *d_lst_k = nullptr;         // mode 1: addresses
    uint16_t *d_lst_q = nullptr;         // modes 1, 2: position of every slot; mode 3: slot of every position
    ListHdr *d_hdrs = nullptr;           // mode 2
    uint32_t *d_tabs = nullptr;          // modes 2, 3: run tables
    IListHdr *d_ihdrs = nullptr;         // mode 3
    uint32_t *d_iflags = nullptr;        // mode 3: run-start bits, [list][round][thread]
    int rmax = 0;
    double bytes_per_window = 0.0;
    ~OsLists()
    {
        void *ptrs[] = {d_lst_k, d_lst_q, d_hdrs, d_tabs, d_ihdrs, d_iflags};
        for (void *q : ptrs)
            if (q) (void)cm2::dev_free(q);
    }
};

// Fills `ls` for the `nwin` windows `d_wins` of an operator and the tile plan `pv` with the builder, the format and
// the run-table stride of `c` (os::choose_lists); launches on `stream` and waits for it.
// sort_chunk_windows: CM2_OS_LIST_CHUNK_PAIRS (test hook: sort in several chunks; 0 = as many as hipCUB takes)
int os_build_lists(const os::ListChoice &c, const os::WinDesc *d_wins, int64_t nwin, OsLists *ls, const OsPlanView &pv,
                   int64_t sort_chunk_windows, hipStream_t stream);

}  // namespace cm2
