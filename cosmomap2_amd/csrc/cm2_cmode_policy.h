// cm2_cmode_policy.h -- the device-free arithmetic of the common-mode filter (cm2_cmode.hip): which arguments are
// accepted and how the (group, time sample) units are laid over workgroups.  Plain C++: tests/test_cmode_cpu.py
// compiles it with the host compiler and checks it against Python.
//
// The stream is ndet rows of ns samples.  Group g is the detectors [edges[g], edges[g + 1]),
// 0 = edges[0] < ... < edges[ngroups] = ndet; unit (g, i) = sample i of group g has the index g ns + i.  One thread
// per unit, kThreads threads a workgroup; a workgroup never crosses a group: group g owns the workgroups
// [g B, (g + 1) B) with B = blocks_per_group(ns), and thread t of workgroup w takes the sample
// (w - g B) kThreads + t of its group, or nothing when that is >= ns.
#pragma once
#include <cstdint>

#include "cm2_modefit_policy.h"

namespace cm2 {
namespace cmode {

// the workgroup, the largest K, the classes of a unit, the status codes and apply_ok: shared with the PCA filter
using modefit::kThreads;
using modefit::kMaxK;
using modefit::Class, modefit::kFitted, modefit::kEmpty, modefit::kFew, modefit::kPivot;
using modefit::Status, modefit::kOk, modefit::kBadK, modefit::kBadSize, modefit::kBadEdges, modefit::kTooLarge;
using modefit::packed;
using modefit::packed_at;
using modefit::apply_ok;
constexpr int64_t blocks_per_group(int64_t ns) { return (ns + kThreads - 1) / kThreads; }

struct Launch {
    int64_t blocks_per_group = 0, blocks = 0, units = 0, nt = 0;
};

// fills *l; anything but kOk leaves it unspecified.  Beyond the shared limits, the workgroup count (a grid dimension)
// stays below 2^31.
inline Status check(Launch *l, int64_t ns, int64_t ndet, int64_t ngroups, const int64_t *edges, int K)
{
    const Status shared = modefit::check(ns, ndet, ngroups, edges, K);
    if (shared != kOk) return shared;
    const int64_t lim = (int64_t)1 << 31;
    const int64_t b = blocks_per_group(ns);
    if (ngroups > (lim - 1) / b) return kTooLarge;
    l->blocks_per_group = b;
    l->blocks = b * ngroups;
    l->units = ngroups * ns;
    l->nt = ndet * ns;
    return kOk;
}

// workgroup w -> its group and the first sample of the group it covers
inline void block_position(const Launch &l, int64_t w, int64_t *group, int64_t *first)
{
    *group = w / l.blocks_per_group;
    *first = (w - *group * l.blocks_per_group) * kThreads;
}

}  // namespace cmode
}  // namespace cm2
