// cm2_chunkfit_policy.h -- what the per-chunk fit filters, the HWPSS filter (cm2_hwpss_policy.h) and the template
// filter (cm2_template_policy.h), agree on: how the (detector, chunk) units are cut into segments, which unit a
// segment belongs to, the classes of a unit and the limits of the sizes.  Plain C++ with no GPU header; the two policy
// headers pull these names in with `using namespace`; tests/test_chunkfit_cpu.py compiles it with the host compiler.
//
// The stream is ndet rows of ns samples.  Chunk c is [edges[c], edges[c + 1]) of every row, 0 = edges[0] < ... <
// edges[nchunks] = ns; unit (k, c) = chunk c of detector k has the index k nchunks + c.  A chunk of n samples is cut
// into ceil(n / kSeg) segments of kSeg samples, the last one may be shorter; segments never cross a chunk edge.  The
// segments of one row are numbered chunk by chunk: seg_first[c] is the first one of chunk c, seg_first[nchunks] =
// segs_per_det, seg_chunk[r] the chunk of row segment r.  Segment r of detector k has the global index
// k segs_per_det + r.  A workgroup of kThreads threads works on one row segment (of one detector, or of the
// detectors of a tile): thread t takes the samples t, t + kThreads, ... of the segment, kPer of them at most.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cm2_fit.h"

namespace cm2 {
namespace chunkfit {

constexpr int kSeg = 4096;                 // samples of a segment
constexpr int kThreads = 256;              // threads of a segment's workgroup
constexpr int kPer = kSeg / kThreads;      // samples a thread sums serially

// (constexpr: callable from device code as well)
constexpr int64_t segments_in(int64_t n) { return (n + kSeg - 1) / kSeg; }
using fit::packed;          // doubles of a lower-triangular factor
using fit::packed_at;       // L_ij, j <= i

// the class of a unit: fitted, skipped for fewer than K unflagged samples, skipped for a failed pivot
enum Mark { kFitted = 0, kFew = 1, kPivot = 2 };

// what make_geometry refuses, in this order.  A filter's own Status has its own refusals first and then these three
// in the same order (kBadSize, kBadEdges, kTooLarge): kBadSize - kGeomSize is the shift
enum GeomStatus { kGeomOk = 0, kGeomSize = 1, kGeomEdges = 2, kGeomLimit = 3 };

struct Geometry {
    int64_t ns = 0, ndet = 0, nchunks = 0, nt = 0;
    int64_t segs_per_det = 0, nsegs = 0, nunits = 0;
    std::vector<int64_t> edges, seg_first;
    std::vector<int32_t> seg_chunk;
};

// fills *p; anything but kGeomOk leaves it unspecified.  The limits keep every index below 2^63, the segment count
// (a grid dimension) and the chunk count (an int32 table entry) below 2^31.
inline GeomStatus make_geometry(Geometry *p, int64_t ns, int64_t ndet, int64_t nchunks, const int64_t *edges)
{
    if (ns < 1 || ndet < 1 || nchunks < 1 || !edges) return kGeomSize;
    if (!fit::edges_ok(edges, nchunks, ns)) return kGeomEdges;
    const int64_t lim = (int64_t)1 << 31;
    if (ns >= ((int64_t)1 << 40) || ndet >= lim || nchunks >= lim) return kGeomLimit;
    if (ndet > (((int64_t)1 << 46) / ns)) return kGeomLimit;
    p->ns = ns;
    p->ndet = ndet;
    p->nchunks = nchunks;
    p->nt = ns * ndet;
    p->edges.assign(edges, edges + nchunks + 1);
    p->seg_first.assign((std::size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        p->seg_first[(std::size_t)c + 1] = p->seg_first[(std::size_t)c] + segments_in(edges[c + 1] - edges[c]);
    p->segs_per_det = p->seg_first[(std::size_t)nchunks];
    if (p->segs_per_det >= lim || ndet > (lim - 1) / p->segs_per_det) return kGeomLimit;
    if (ndet > (lim - 1) / nchunks) return kGeomLimit;
    p->nsegs = ndet * p->segs_per_det;
    p->nunits = ndet * nchunks;
    p->seg_chunk.assign((std::size_t)p->segs_per_det, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        for (int64_t r = p->seg_first[(std::size_t)c]; r < p->seg_first[(std::size_t)c + 1]; ++r)
            p->seg_chunk[(std::size_t)r] = (int32_t)c;
    return kGeomOk;
}

// samples [*t0, *t1) of the row that row segment r covers
inline void segment_range(const Geometry &p, int64_t r, int64_t *t0, int64_t *t1)
{
    const int64_t c = p.seg_chunk[(std::size_t)r];
    *t0 = p.edges[(std::size_t)c] + (r - p.seg_first[(std::size_t)c]) * kSeg;
    *t1 = *t0 + kSeg < p.edges[(std::size_t)c + 1] ? *t0 + kSeg : p.edges[(std::size_t)c + 1];
}

}  // namespace chunkfit
}  // namespace cm2
