// cm2_template_policy.h -- the device-free arithmetic of the template filter (cm2_template.hip): the template count,
// how the (detector, chunk) units are cut into segments, and how detectors are grouped into the tiles that share one
// read of the template table.  Plain C++: tests/test_template_cpu.py compiles it with the host compiler and checks it
// against Python.
//
// Units, chunks and segments are those of cm2_hwpss_policy.h: the stream is ndet rows of ns samples, chunk c is
// [edges[c], edges[c + 1]) of every row, unit (k, c) has the index k nchunks + c, a chunk of n samples is cut into
// ceil(n / kSeg) segments that never cross a chunk edge, numbered chunk by chunk along a row (seg_first, seg_chunk);
// segment r of detector k has the global index k segs_per_det + r.
//
// A workgroup of kThreads threads takes row segment r of the det_tile(K) consecutive detectors of one tile: thread t
// takes the samples t, t + kThreads, ... of the segment, kPer of them at most, loads their K template values once and
// uses them for every detector of the tile.  Workgroup w works on tile w % ntiles of row segment w / ntiles: tiles run
// fastest, so that the workgroups in flight together read the same lines of the table.  The tile is a grouping of the
// work only: every sum is formed per detector, in the order cm2_template.hip states, and does not depend on it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cm2_fit.h"

namespace cm2 {
namespace tmpl {

constexpr int kSeg = 4096;                 // samples of a segment
constexpr int kThreads = 256;              // threads of a segment's workgroup
constexpr int kPer = kSeg / kThreads;      // samples a thread sums serially
constexpr int kMaxK = 16;                  // CM2_TEMPLATE_MAX_K

// (constexpr: callable from device code as well)
// detectors of a tile: a thread holds det_tile(K) K accumulators, 32 doubles (64 VGPRs) at most.  Measured
// (profiles/template_filter.md): larger tiles read less of the table and lose more to occupancy than that saves.
constexpr int det_tile(int K) { return K <= 2 ? 4 : 2; }
constexpr int64_t segments_in(int64_t n) { return (n + kSeg - 1) / kSeg; }
using fit::packed;          // doubles of a lower-triangular factor
using fit::packed_at;       // L_ij, j <= i

enum Status { kOk = 0, kBadCount = 1, kBadConstant = 2, kBadK = 3, kBadSize = 4, kBadEdges = 5, kTooLarge = 6 };
enum Mark { kFitted = 0, kFew = 1, kPivot = 2 };       // the class of a unit: cm2_template_status

struct Plan {
    int64_t ns = 0, ndet = 0, nchunks = 0, nt = 0;
    int J = 0, K = 0, add_constant = 0, Dt = 0;
    int64_t segs_per_det = 0, nsegs = 0, nunits = 0, ntiles = 0, ngroups = 0;
    std::vector<int64_t> edges, seg_first;
    std::vector<int32_t> seg_chunk;
};

// fills *p; anything but kOk leaves it unspecified.  The limits keep every index below 2^63, the segment count and
// the workgroup count (grid dimensions) and the chunk count (an int32 table entry) below 2^31.
inline Status make_plan(Plan *p, int64_t ns, int64_t ndet, int64_t nchunks, const int64_t *edges, int ntemplates,
                        int add_constant)
{
    if (ntemplates < 0) return kBadCount;
    if (add_constant != 0 && add_constant != 1) return kBadConstant;
    if (ntemplates > kMaxK || ntemplates + add_constant < 1 || ntemplates + add_constant > kMaxK) return kBadK;
    if (ns < 1 || ndet < 1 || nchunks < 1 || !edges) return kBadSize;
    if (!fit::edges_ok(edges, nchunks, ns)) return kBadEdges;
    const int64_t lim = (int64_t)1 << 31;
    if (ns >= ((int64_t)1 << 40) || ndet >= lim || nchunks >= lim) return kTooLarge;
    if (ndet > (((int64_t)1 << 46) / ns)) return kTooLarge;
    p->ns = ns;
    p->ndet = ndet;
    p->nchunks = nchunks;
    p->nt = ns * ndet;
    p->J = ntemplates;
    p->add_constant = add_constant;
    p->K = ntemplates + add_constant;
    p->Dt = det_tile(p->K);
    p->edges.assign(edges, edges + nchunks + 1);
    p->seg_first.assign((std::size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        p->seg_first[(std::size_t)c + 1] = p->seg_first[(std::size_t)c] + segments_in(edges[c + 1] - edges[c]);
    p->segs_per_det = p->seg_first[(std::size_t)nchunks];
    if (p->segs_per_det >= lim || ndet > (lim - 1) / p->segs_per_det) return kTooLarge;
    if (ndet > (lim - 1) / nchunks) return kTooLarge;
    p->nsegs = ndet * p->segs_per_det;
    p->nunits = ndet * nchunks;
    p->ntiles = (ndet + p->Dt - 1) / p->Dt;
    p->ngroups = p->ntiles * p->segs_per_det;          // workgroups of a pass: <= nsegs < 2^31
    p->seg_chunk.assign((std::size_t)p->segs_per_det, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        for (int64_t r = p->seg_first[(std::size_t)c]; r < p->seg_first[(std::size_t)c + 1]; ++r)
            p->seg_chunk[(std::size_t)r] = (int32_t)c;
    return kOk;
}

// samples [*t0, *t1) of the row that row segment r covers
inline void segment_range(const Plan &p, int64_t r, int64_t *t0, int64_t *t1)
{
    const int64_t c = p.seg_chunk[(std::size_t)r];
    *t0 = p.edges[(std::size_t)c] + (r - p.seg_first[(std::size_t)c]) * kSeg;
    *t1 = *t0 + kSeg < p.edges[(std::size_t)c + 1] ? *t0 + kSeg : p.edges[(std::size_t)c + 1];
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
