// cm2_pca_policy.h -- the device-free arithmetic of the PCA filter (cm2_pca.hip): which arguments are accepted, how
// the covariance of every (chunk, group) unit is cut into work items and how the (group, time sample) units of the
// apply are laid over workgroups.  Plain C++: tests/test_pca_cpu.py compiles it with the host compiler and checks it
// against a brute-force enumeration in Python.
//
// The stream is ndet rows of ns samples.  Group g is the detectors [gedges[g], gedges[g + 1]), chunk c the samples
// [cedges[c], cedges[c + 1]).  Covariance unit u = c G + g holds n_g^2 doubles at c sum_g n_g^2 + sum_{g' < g} n_g'^2.
//
// Covariance: the n x n lower triangle of a unit is cut into kTile x kTile tiles, tile pair (a, b), b <= a, with the
// index a (a + 1) / 2 + b; the chunk into segments of kSegment samples counted from the chunk's own start (the last
// one shorter).  One work item = one workgroup = (unit, tile pair, segment); items are ordered by unit, then pair,
// then segment, so the segments of a pair are neighbours.  An item writes its rows x cols partial sums (rows, cols
// <= kTile: the tile cut at the group's end), row-major, at `part` of the workspace.
//
// Apply: a slab is at most kThreads consecutive samples of one chunk; slabs are ordered by chunk, then by sample, and
// never cross a chunk edge.  Workgroup w takes slab w % nslabs of group w / nslabs; thread t takes sample first + t.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cm2_modefit_policy.h"

namespace cm2 {
namespace pca {

// the workgroup (of every kernel here), the largest K, the classes of a unit and apply_ok: shared with cm2_cmode
using modefit::kThreads;
using modefit::kMaxK;
using modefit::Class, modefit::kFitted, modefit::kEmpty, modefit::kFew, modefit::kPivot;
using modefit::packed;
using modefit::packed_at;
using modefit::apply_ok;

constexpr int kMfma = 16;                  // rows and columns of one v_mfma_f64_16x16x4_f64 result
constexpr int kMfmaK = 4;                  // samples one instruction contracts
constexpr int kTile = 128;                 // rows and columns of a workgroup tile: 2 x 2 waves of 64 x 64
constexpr int kWaveTile = 64;              // rows and columns of a wave's accumulators: 4 x 4 MFMA results
constexpr int kStep = 16;                  // samples staged in LDS at a time
constexpr int kPitch = 18;                 // doubles between the rows of a staged slab (kStep + 2)
constexpr int kSegment = 4096;             // samples of a segment

enum Status { kOk = 0, kBadK = 1, kBadSize = 2, kBadEdges = 3, kBadChunks = 4, kTooLarge = 5 };

static_assert(kBadK == (int)modefit::kBadK && kBadSize == (int)modefit::kBadSize &&
                  kBadEdges == (int)modefit::kBadEdges, "the shared refusals keep their codes");

// LDS of a covariance workgroup: two staged slabs (row tile, column tile) of kTile rows
constexpr size_t lds_bytes() { return (size_t)2 * kTile * kPitch * sizeof(double); }
static_assert(lds_bytes() <= 64 * 1024, "the staged slabs must fit the static LDS of a workgroup");
// kPitch = 2 x odd: the 16 rows of a half-wave start on 16 different even doubles mod 32, its 2 samples fill the pairs
static_assert(kPitch % 4 == 2 && kPitch >= kStep, "row pitch: 16 rows x 2 samples of a half-wave fill the 64 banks");
static_assert(kStep % kMfmaK == 0 && kSegment % kStep == 0 && kTile == 2 * kWaveTile && kWaveTile % kMfma == 0, "");
static_assert(kThreads == kStep * (kTile / 8), "a thread stages 8 rows of one sample column");

// where operand (row r of the slab, sample k of the step) lies in a staged slab, in doubles; bank(r, k) is the first
// of its two 4-byte banks under the 64-bank rule of an 8-byte LDS read
constexpr int lds_at(int r, int k) { return r * kPitch + k; }
constexpr int lds_bank(int r, int k) { return (2 * lds_at(r, k)) % 64; }

constexpr int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
constexpr int64_t pairs_of(int64_t n) { return tiles_of(n) * (tiles_of(n) + 1) / 2; }
constexpr int64_t segments_of(int64_t len) { return (len + kSegment - 1) / kSegment; }
constexpr int64_t slabs_of(int64_t len) { return (len + kThreads - 1) / kThreads; }

struct CovItem {
    int64_t row0, col0;       // first detector of the row tile and of the column tile (col0 <= row0)
    int64_t first;            // first sample
    int64_t part;             // where its rows x cols partial sums start in the workspace, in doubles
    int32_t len;              // samples, 1..kSegment
    int32_t rows, cols;       // detectors of the two tiles inside the group, 1..kTile
    int32_t unit;
};

struct CovUnit {
    int64_t first_item;       // its items are [first_item, first_item + pairs nseg)
    int64_t at;               // where its n x n doubles start in the output
    int32_t n, nseg;
};

struct Slab {
    int64_t first;            // first sample
    int32_t len;              // samples, 1..kThreads
    int32_t chunk;
};

struct Plan {
    int64_t nt = 0, units = 0;                   // samples; (group, sample) units of the apply
    int64_t cov_units = 0, cov_per_chunk = 0, cov_doubles = 0;
    int64_t items = 0, work_doubles = 0;
    int64_t slabs = 0, blocks = 0;               // slabs of one group; workgroups of an apply
    int64_t final_blocks = 0;
    int64_t min_group = 0;                       // detectors of the smallest group
};

// the covariance is defined for any group; modes can be set (and so applied) only when every group has at least
// K + 1 detectors: K modes on K detectors would remove everything
constexpr bool modes_allowed(int64_t min_group, int K) { return min_group >= (int64_t)K + 1; }

// fills *p; anything but kOk leaves it unspecified.  The limits keep every sample index (ndet ns <= 2^46), every
// coefficient index and every covariance and workspace index below 2^63, and every grid below 2^31 workgroups.
inline Status check(Plan *p, int64_t ns, int64_t ndet, int64_t ngroups, const int64_t *gedges, int64_t nchunks,
                    const int64_t *cedges, int K)
{
    // the shared refusals in their places: a chunk count below 1 is a size, bad chunk edges come before the limits
    const modefit::Status shared = modefit::check(ns, ndet, ngroups, gedges, K);
    if (shared == modefit::kBadK) return kBadK;
    if (shared == modefit::kBadSize || nchunks < 1 || !cedges) return kBadSize;
    if (shared == modefit::kBadEdges) return kBadEdges;
    if (!fit::edges_ok(cedges, nchunks, ns)) return kBadChunks;
    if (shared != modefit::kOk) return kTooLarge;
    const int64_t lim = (int64_t)1 << 31;
    // ndet <= 2^23 keeps sum n^2 <= ndet^2 below 2^46; nchunks times that and the items stay below 2^62
    if (ndet > ((int64_t)1 << 23) || nchunks > ((int64_t)1 << 16)) return kTooLarge;
    int64_t per_chunk = 0, pairs = 0, part = 0, smallest = ndet;
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t n = gedges[g + 1] - gedges[g];
        smallest = n < smallest ? n : smallest;
        per_chunk += n * n;
        pairs += pairs_of(n);
        // the partials of one segment of this group: the tiles of the lower triangle, cut at the group's end
        const int64_t T = tiles_of(n), last = n - (T - 1) * kTile;
        part += (T - 1) * T / 2 * kTile * kTile + (T - 1) * last * kTile + last * last;
    }
    int64_t segs = 0, slabs = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        segs += segments_of(cedges[c + 1] - cedges[c]);
        slabs += slabs_of(cedges[c + 1] - cedges[c]);
    }
    if (pairs > (lim - 1) / segs) return kTooLarge;
    if (ngroups > (lim - 1) / slabs) return kTooLarge;
    const int64_t cov = per_chunk * nchunks;
    if ((cov + kThreads - 1) / kThreads >= lim) return kTooLarge;
    p->nt = ndet * ns;
    p->units = ngroups * ns;
    p->cov_units = nchunks * ngroups;
    p->cov_per_chunk = per_chunk;
    p->cov_doubles = cov;
    p->items = pairs * segs;
    p->work_doubles = part * segs;
    p->slabs = slabs;
    p->blocks = slabs * ngroups;
    p->final_blocks = (cov + kThreads - 1) / kThreads;
    p->min_group = smallest;
    return kOk;
}

// the work items and the units of the covariance, in their order; arguments that check() accepted
inline void cov_table(int64_t ngroups, const int64_t *gedges, int64_t nchunks, const int64_t *cedges,
                      std::vector<CovItem> *items, std::vector<CovUnit> *units)
{
    items->clear();
    units->clear();
    int64_t per_chunk = 0;
    for (int64_t g = 0; g < ngroups; ++g) per_chunk += (gedges[g + 1] - gedges[g]) * (gedges[g + 1] - gedges[g]);
    int64_t part = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t len = cedges[c + 1] - cedges[c], nseg = segments_of(len);
        int64_t at = c * per_chunk;
        for (int64_t g = 0; g < ngroups; ++g) {
            const int64_t n = gedges[g + 1] - gedges[g], T = tiles_of(n);
            units->push_back(CovUnit{(int64_t)items->size(), at, (int32_t)n, (int32_t)nseg});
            at += n * n;
            for (int64_t a = 0; a < T; ++a)
                for (int64_t b = 0; b <= a; ++b)
                    for (int64_t s = 0; s < nseg; ++s) {
                        CovItem it;
                        it.row0 = gedges[g] + a * kTile;
                        it.col0 = gedges[g] + b * kTile;
                        it.first = cedges[c] + s * kSegment;
                        it.part = part;
                        it.len = (int32_t)(len - s * kSegment < kSegment ? len - s * kSegment : kSegment);
                        it.rows = (int32_t)(n - a * kTile < kTile ? n - a * kTile : kTile);
                        it.cols = (int32_t)(n - b * kTile < kTile ? n - b * kTile : kTile);
                        it.unit = (int32_t)(c * ngroups + g);
                        part += (int64_t)it.rows * it.cols;
                        items->push_back(it);
                    }
        }
    }
}

// the slabs of one group, in their order
inline void slab_table(int64_t nchunks, const int64_t *cedges, std::vector<Slab> *slabs)
{
    slabs->clear();
    for (int64_t c = 0; c < nchunks; ++c)
        for (int64_t i = cedges[c]; i < cedges[c + 1]; i += kThreads) {
            const int64_t left = cedges[c + 1] - i;
            slabs->push_back(Slab{i, (int32_t)(left < kThreads ? left : kThreads), (int32_t)c});
        }
}

}  // namespace pca
}  // namespace cm2
