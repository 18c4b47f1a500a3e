// cm2_hwpss_policy.h -- the device-free arithmetic of the HWP-synchronous signal filter (cm2_hwpss.hip): how the
// (detector, chunk) units are cut into segments and which unit a segment belongs to.  Plain C++:
// tests/test_hwpss_cpu.py compiles it with the host compiler and checks it against Python.
//
// The stream is ndet rows of ns samples.  Chunk c is [edges[c], edges[c + 1]) of every row, 0 = edges[0] < ... <
// edges[nchunks] = ns; unit (k, c) = chunk c of detector k has the index k nchunks + c.  A chunk of n samples is cut
// into ceil(n / kSeg) segments of kSeg samples, the last one may be shorter; segments never cross a chunk edge.  The
// segments of one row are numbered chunk by chunk: seg_first[c] is the first one of chunk c, seg_first[nchunks] =
// segs_per_det, seg_chunk[r] the chunk of row segment r.  Segment r of detector k has the global index
// k segs_per_det + r and is the work of one workgroup of kThreads threads: thread t takes the samples
// t, t + kThreads, ... of its segment, kPer of them at most.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cm2_fit.h"

namespace cm2 {
namespace hwpss {

constexpr int kSeg = 4096;                 // samples of a segment
constexpr int kThreads = 256;              // threads of a segment's workgroup
constexpr int kPer = kSeg / kThreads;      // samples a thread sums serially
constexpr int kMaxHarm = 8;
constexpr int kMaxK = 2 * kMaxHarm + 1;

// (constexpr: callable from device code as well)
constexpr int templates(int nharm) { return 2 * nharm + 1; }
constexpr int64_t segments_in(int64_t n) { return (n + kSeg - 1) / kSeg; }
using fit::packed;          // doubles of a lower-triangular factor
using fit::packed_at;       // L_ij, j <= i

enum Status { kOk = 0, kBadHarm = 1, kBadSize = 2, kBadEdges = 3, kTooLarge = 4 };

struct Plan {
    int64_t ns = 0, ndet = 0, nchunks = 0, nt = 0;
    int nharm = 0, K = 0;
    int64_t segs_per_det = 0, nsegs = 0, nunits = 0;
    std::vector<int64_t> edges, seg_first;
    std::vector<int32_t> seg_chunk;
};

// fills *p; anything but kOk leaves it unspecified.  The limits keep every index below 2^63, the segment count
// (a grid dimension) and the chunk count (an int32 table entry) below 2^31.
inline Status make_plan(Plan *p, int64_t ns, int64_t ndet, int64_t nchunks, const int64_t *edges, int nharm)
{
    if (nharm < 1 || nharm > kMaxHarm) return kBadHarm;
    if (ns < 1 || ndet < 1 || nchunks < 1 || !edges) return kBadSize;
    if (!fit::edges_ok(edges, nchunks, ns)) return kBadEdges;
    const int64_t lim = (int64_t)1 << 31;
    if (ns >= ((int64_t)1 << 40) || ndet >= lim || nchunks >= lim) return kTooLarge;
    if (ndet > (((int64_t)1 << 46) / ns)) return kTooLarge;
    p->ns = ns;
    p->ndet = ndet;
    p->nchunks = nchunks;
    p->nt = ns * ndet;
    p->nharm = nharm;
    p->K = templates(nharm);
    p->edges.assign(edges, edges + nchunks + 1);
    p->seg_first.assign((std::size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        p->seg_first[(std::size_t)c + 1] = p->seg_first[(std::size_t)c] + segments_in(edges[c + 1] - edges[c]);
    p->segs_per_det = p->seg_first[(std::size_t)nchunks];
    if (p->segs_per_det >= lim || ndet > (lim - 1) / p->segs_per_det) return kTooLarge;
    if (ndet > (lim - 1) / nchunks) return kTooLarge;
    p->nsegs = ndet * p->segs_per_det;
    p->nunits = ndet * nchunks;
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

}  // namespace hwpss
}  // namespace cm2
