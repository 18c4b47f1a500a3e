// cm2_demod_policy.h -- the device-free arithmetic of the demodulator (cm2_demod.hip): which arguments are accepted,
// how the input units and the outputs are laid over the noise blocks, and what one unit holds in LDS.  Plain C++:
// tests/test_demod_cpu.py compiles it with the host compiler and checks it against Python.
//
// cm2_stream_policy.h has the blocks, their units and the checks every stage shares; its names are reachable as
// cm2::demod:: too.  Workgroup g takes unit g, so one workgroup sees one block only.
//
// Units.  Output j of a block is centred on sample j D of it and reads the samples j D - c .. j D + c, c = (L - 1) / 2.
// A unit is unit_len(D) = floor(2048 / D) D input samples: it starts on an output centre and owns the
// outputs_per_unit(D) = floor(2048 / D) outputs centred in it (the last unit of a block fewer: ceil(len / D)).  The
// outputs of block b start at the prefix of m_b = ceil(n_b / D), which is the unit table of unit length D.
//
// LDS.  The windows of a unit's outputs cover staged(D, L) = (outputs - 1) D + L <= 2048 - D + L <= 3072 consecutive
// samples, the halo of c on either side included.  A workgroup stages them once: the masked d (8 bytes), with a carrier
// d cos and d sin (8 bytes each), and one usable byte.  Thread t owns the outputs t, t + 256, ... of the unit and reads
// slot (t + 256 m) D + k at tap k: a stride of D doubles, which for D = 8, 16, 32, 64 would put 8, 16, 32, 32 lanes of a
// half-wave on one bank pair.  So sample v sits in slot v + v / 32 (one double of padding per 32): at k = 0 the 32
// lanes of a half-wave then fall on 32 different bank pairs for D = 1, 2, 4, 8, 16, 32 and on 16 for D = 64.
//     D = 64, L = 1025, carrier:  staged 3009, slots 3103:  3 x 24 824 + 3 104 = 77 576 bytes
//     D = 1,  L = 1025, carrier:  staged 3072, slots 3167:  3 x 25 336 + 3 168 = 79 176 bytes   (the largest)
// Two workgroups of the largest need 158 352 of the 163 840 bytes of a CU: two fit, at every (D, L).  The taps are not
// in LDS (8 200 bytes more would leave one workgroup per CU): tap k is the same for every lane, a scalar load.
// Outputs per thread: rounds(D) = ceil(outputs_per_unit(D) / 256) = 8, 4, 3, 2 for D = 1, 2, 3, 4, then 2 up to D = 7
// and 1 from D = 8 on; a thread keeps 3 or 5 chains (T, W and the count; Q, U) per output, at most 8 x 5 of them.
#pragma once
#include <cmath>
#include <cstdint>

#include "cm2_stream_policy.h"

namespace cm2 {
namespace demod {

using namespace stream;

constexpr int kMaxFactor = 64;             // 1 <= D <= 64
constexpr int kMaxTaps = 1025;             // 1 <= L <= 1025, odd
constexpr int kThreads = 256;
constexpr int kMaxUnit = 2048;             // input samples of one workgroup, at most
constexpr int kRounds = 8;                 // outputs of one thread, at most
constexpr int kCounts = 3;                 // counts[b][FULL, PARTIAL, REJECTED]
constexpr int64_t kLdsLimit = 80 * 1024;   // of one workgroup: two a CU

// the classes of an output (CM2_DEMOD_* of include/cosmomap2.h)
enum Class { kFull = 0, kPartial = 1, kRejected = 2 };

// the codes of this stage beside the shared ones
constexpr Status kBadFactor = Status(11);          // outside [1, 64]
constexpr Status kBadTaps = Status(12);            // no taps, an even number of them or more than 1025
constexpr Status kBadTapValue = Status(13);        // a tap that is not finite
constexpr Status kBadTapSum = Status(14);          // Wfull not finite or <= 0
constexpr Status kBadMinWeight = Status(15);       // outside (0, 1]
constexpr Status kBadDropFrom = Status(16);        // neither 1 nor 2

// ---- one unit ---------------------------------------------------------------------------------------------------
constexpr int outputs_per_unit(int D) { return kMaxUnit / D; }
constexpr int unit_len(int D) { return outputs_per_unit(D) * D; }
constexpr int rounds(int D) { return (outputs_per_unit(D) + kThreads - 1) / kThreads; }
// samples the windows of nout outputs cover
constexpr int staged(int nout, int D, int L) { return (nout - 1) * D + L; }
// where sample v of them sits, and the slots they take
constexpr int slot(int v) { return v + (v >> 5); }
constexpr int slots(int n) { return slot(n - 1) + 1; }
// one workgroup of a full unit: 1 or 3 planes of doubles and the usable bytes, rounded up to 8 bytes
constexpr int64_t lds_bytes(int D, int L, bool carrier)
{
    const int64_t n = slots(staged(outputs_per_unit(D), D, L));
    return n * 8 * (carrier ? 3 : 1) + (n + 7) / 8 * 8;
}
// outputs of a block, or of the last unit of one, of len samples
constexpr int64_t outputs_of(int64_t len, int D) { return units_of(len, D); }

static_assert(rounds(1) == kRounds && rounds(kMaxFactor) == 1, "a thread has at most kRounds outputs");
static_assert(staged(outputs_per_unit(1), 1, kMaxTaps) == 3072, "the largest stage");
static_assert(lds_bytes(1, kMaxTaps, true) == 79176 && 2 * lds_bytes(1, kMaxTaps, true) <= 160 * 1024 &&
              lds_bytes(1, kMaxTaps, true) <= kLdsLimit, "two workgroups a CU");

struct Launch {
    int64_t nt = 0, nblocks = 0, units = 0, M = 0;
    int D = 0, L = 0, c = 0, unit = 0, per_unit = 0, rounds = 0;
    int64_t lds_carrier = 0, lds_plain = 0;
    double wfull = 0.0;
};

// Wfull: the taps added from 0.0 in ascending k
inline double tap_sum(const double *taps, int ntaps)
{
    double w = 0.0;
    for (int k = 0; k < ntaps; ++k) w = w + taps[k];
    return w;
}

// fills *l; anything but kOk leaves it unspecified.  The order of the tests: the sizes given, the factor, the 32-bit
// limit, the blocks and their number (check_blocks), then the taps.
inline Status check_create(Launch *l, int64_t nt, const int64_t *sizes, int64_t nblocks, int factor, const double *taps,
                           int ntaps)
{
    if (nt < 1 || nblocks < 1 || !sizes) return kBadSize;
    if (factor < 1 || factor > kMaxFactor) return kBadFactor;
    const Status st = check_blocks(nt, sizes, nblocks, true);
    if (st != kOk) return st;
    if (!taps || ntaps < 1 || ntaps > kMaxTaps || ntaps % 2 == 0) return kBadTaps;
    for (int k = 0; k < ntaps; ++k)
        if (!std::isfinite(taps[k])) return kBadTapValue;
    const double w = tap_sum(taps, ntaps);
    if (!(std::isfinite(w) && w > 0.0)) return kBadTapSum;
    l->nt = nt;
    l->nblocks = nblocks;
    l->D = factor;
    l->L = ntaps;
    l->c = (ntaps - 1) / 2;
    l->unit = unit_len(factor);
    l->per_unit = outputs_per_unit(factor);
    l->rounds = rounds(factor);
    l->units = total_units(sizes, nblocks, l->unit);
    l->M = total_units(sizes, nblocks, factor);
    l->lds_carrier = lds_bytes(factor, ntaps, true);
    l->lds_plain = lds_bytes(factor, ntaps, false);
    l->wfull = w;
    return kOk;
}

inline Status check_run(bool have_flags, int kind, double min_weight)
{
    if (check_flag_kind(have_flags, kind) != kOk) return kBadFlagKind;
    if (!(min_weight > 0.0 && min_weight <= 1.0)) return kBadMinWeight;      // (a NaN fails the first)
    return kOk;
}

inline Status check_pick(int drop_from) { return drop_from == 1 || drop_from == 2 ? kOk : kBadDropFrom; }

// the class of an output: included of its L terms, and whether its weight passed the test
constexpr int class_of(int included, int L, bool weight_ok)
{
    return included == L ? kFull : weight_ok ? kPartial : kRejected;
}

}  // namespace demod
}  // namespace cm2
