// cm2_modefit_policy.h -- what the common-mode filter (cm2_cmode_policy.h) and the PCA filter (cm2_pca_policy.h)
// agree on: the size of a workgroup, the largest K, the classes of a (group, time sample) unit, the rule for an
// apply's output and the limits of the arguments they share.  Plain C++ with no GPU header; the two policy headers
// pull these names in with `using`, and their tests compile them with the host compiler.
#pragma once
#include <cstdint>

#include "cm2_fit.h"

namespace cm2 {
namespace modefit {

constexpr int kThreads = 256;              // threads of a workgroup = units of a workgroup (four waves)
constexpr int kMaxK = 10;                  // templates or modes per detector

// the classes of a unit, as cm2_cmode_status and cm2_pca_status report them
enum Class { kFitted = 0, kEmpty = 1, kFew = 2, kPivot = 3 };

// (constexpr: callable from device code as well)
using fit::packed;          // doubles of the lower triangle
using fit::packed_at;       // entry (i, j), j <= i

enum Status { kOk = 0, kBadK = 1, kBadSize = 2, kBadEdges = 3, kTooLarge = 4 };

// ns samples of ndet detectors in ngroups groups, K templates.  The limits keep every sample index (ndet ns <= 2^46)
// and every coefficient index (ngroups K ns <= 10 x 2^46) below 2^63.
inline Status check(int64_t ns, int64_t ndet, int64_t ngroups, const int64_t *edges, int K)
{
    if (K < 1 || K > kMaxK) return kBadK;
    if (ns < 1 || ndet < 1 || ngroups < 1 || !edges) return kBadSize;
    if (!fit::edges_ok(edges, ngroups, ndet)) return kBadEdges;
    if (ndet >= (int64_t)1 << 31) return kTooLarge;
    if (ndet > (((int64_t)1 << 46) / ns)) return kTooLarge;
    return kOk;
}

// do the doubles a[0, na) and b[0, nb) share a byte?  (addresses as integers: no GPU header here)
inline bool overlap(uint64_t a, int64_t na, uint64_t b, int64_t nb)
{
    return a < b + (uint64_t)nb * sizeof(double) && b < a + (uint64_t)na * sizeof(double);
}
// apply: the output is the input itself or shares nothing with it
inline bool apply_ok(uint64_t in, uint64_t out, int64_t nt) { return in == out || !overlap(in, nt, out, nt); }

}  // namespace modefit
}  // namespace cm2
