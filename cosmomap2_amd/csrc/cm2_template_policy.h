// cm2_template_policy.h -- the device-free arithmetic of the template filter (cm2_template.hip): the template count
// and how detectors are grouped into the tiles that share one read of the template table.  Chunks, units, segments and
// the plan's geometry are those of cm2_chunkfit_policy.h.  Plain C++: tests/test_template_cpu.py compiles it with the
// host compiler and checks it against Python.
//
// A workgroup of kThreads threads takes row segment r of the det_tile(K) consecutive detectors of one tile: thread t
// takes the samples t, t + kThreads, ... of the segment, kPer of them at most, loads their K template values once and
// uses them for every detector of the tile.  Workgroup w works on tile w % ntiles of row segment w / ntiles: tiles run
// fastest, so that the workgroups in flight together read the same lines of the table.  The tile is a grouping of the
// work only: every sum is formed per detector, in the order cm2_chunkfit.h states, and does not depend on it.
#pragma once
#include "cm2_chunkfit_policy.h"

namespace cm2 {
namespace tmpl {

using namespace chunkfit;     // kFitted, kFew, kPivot: the class of a unit, cm2_template_status

constexpr int kMaxK = 16;                  // CM2_TEMPLATE_MAX_K

// (constexpr: callable from device code as well)
// detectors of a tile: a thread holds det_tile(K) K accumulators, 32 doubles (64 VGPRs) at most.  Measured
// (profiles/template_filter.md): larger tiles read less of the table and lose more to occupancy than that saves.
constexpr int det_tile(int K) { return K <= 2 ? 4 : 2; }

enum Status { kOk = 0, kBadCount = 1, kBadConstant = 2, kBadK = 3, kBadSize = 4, kBadEdges = 5, kTooLarge = 6 };
static_assert(kBadEdges == kBadSize + 1 && kTooLarge == kBadSize + 2, "the shared refusals, in the shared order");

struct Plan : chunkfit::Geometry {
    int J = 0, K = 0, add_constant = 0, Dt = 0;
    int64_t ntiles = 0, ngroups = 0;
};

// fills *p; anything but kOk leaves it unspecified.  The workgroup count (a grid dimension) stays below 2^31 with
// the segment count.
inline Status make_plan(Plan *p, int64_t ns, int64_t ndet, int64_t nchunks, const int64_t *edges, int ntemplates,
                        int add_constant)
{
    if (ntemplates < 0) return kBadCount;
    if (add_constant != 0 && add_constant != 1) return kBadConstant;
    if (ntemplates > kMaxK || ntemplates + add_constant < 1 || ntemplates + add_constant > kMaxK) return kBadK;
    const int bad = make_geometry(p, ns, ndet, nchunks, edges);
    if (bad) return (Status)(bad + (kBadSize - kGeomSize));
    p->J = ntemplates;
    p->add_constant = add_constant;
    p->K = ntemplates + add_constant;
    p->Dt = det_tile(p->K);
    p->ntiles = (ndet + p->Dt - 1) / p->Dt;
    p->ngroups = p->ntiles * p->segs_per_det;          // workgroups of a pass: <= nsegs < 2^31
    return kOk;
}

// the work of workgroup w: row segment *r of the detectors [*k0, *k1)
inline void group_range(const Plan &p, int64_t w, int64_t *r, int64_t *k0, int64_t *k1)
{
    *r = w / p.ntiles;
    *k0 = (w - *r * p.ntiles) * p.Dt;
    *k1 = *k0 + p.Dt < p.ndet ? *k0 + p.Dt : p.ndet;
}

}  // namespace tmpl
}  // namespace cm2
