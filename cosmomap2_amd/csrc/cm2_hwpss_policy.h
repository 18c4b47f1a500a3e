// cm2_hwpss_policy.h -- the device-free arithmetic of the HWP-synchronous signal filter (cm2_hwpss.hip): the number
// of harmonics and of templates.  Chunks, units, segments and the plan's geometry are those of cm2_chunkfit_policy.h.
// Plain C++: tests/test_hwpss_cpu.py compiles it with the host compiler and checks it against Python.
#pragma once
#include "cm2_chunkfit_policy.h"

namespace cm2 {
namespace hwpss {

using namespace chunkfit;

constexpr int kMaxHarm = 8;
constexpr int kMaxK = 2 * kMaxHarm + 1;

// (constexpr: callable from device code as well)
constexpr int templates(int nharm) { return 2 * nharm + 1; }

enum Status { kOk = 0, kBadHarm = 1, kBadSize = 2, kBadEdges = 3, kTooLarge = 4 };
static_assert(kBadEdges == kBadSize + 1 && kTooLarge == kBadSize + 2, "the shared refusals, in the shared order");

struct Plan : chunkfit::Geometry {
    int nharm = 0, K = 0;
};

// fills *p; anything but kOk leaves it unspecified
inline Status make_plan(Plan *p, int64_t ns, int64_t ndet, int64_t nchunks, const int64_t *edges, int nharm)
{
    if (nharm < 1 || nharm > kMaxHarm) return kBadHarm;
    p->nharm = nharm;
    p->K = templates(nharm);
    const int bad = make_geometry(p, ns, ndet, nchunks, edges);
    return bad ? (Status)(bad + (kBadSize - kGeomSize)) : kOk;
}

}  // namespace hwpss
}  // namespace cm2
