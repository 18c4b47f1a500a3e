// cm2_stream.h -- the device side of cm2_stream_policy.h for the stages over the noise blocks of a time stream: how a
// kernel sees the stream and its flags, the prefix tables of the blocks on the device and their owner, and the
// refusals of a create and of overlapping arrays, worded once.
#pragma once
#include <initializer_list>
#include <vector>

#include "cm2_common.h"
#include "cm2_stream_policy.h"

namespace cm2 {
namespace stream {

constexpr uint64_t kExpMask = 0x7FF0000000000000ull;

// the flag of sample i: KIND 0 = int32 (the pixel ids), flagged when negative; KIND 1 = bytes, flagged when non-zero
template <int KIND>
__host__ __device__ __forceinline__ bool flagged(const void *__restrict__ flags, int64_t i)
{
    if (KIND == 0) return static_cast<const int32_t *>(flags)[i] < 0;
    return static_cast<const uint8_t *>(flags)[i] != 0;
}

// A sample is usable when it is not flagged, finite and not carried from an earlier pass; what "carried" means is the
// stage's (its usable_at).
struct Stream {
    const double *d;
    const void *flags;                     // NULL: nothing flagged
    int kind;                              // the KIND of flagged()
    const uint8_t *prev;                   // NULL: no earlier pass
};

__device__ __forceinline__ bool finite_bits(double x)
{
    return ((unsigned long long)__double_as_longlong(x) & kExpMask) != kExpMask;
}
__device__ __forceinline__ bool flagged_at(const Stream &s, int64_t i)
{
    if (!s.flags) return false;
    return s.kind == 0 ? flagged<0>(s.flags, i) : flagged<1>(s.flags, i);
}

// the blocks of a stream cut into units of one length, as a kernel takes them
struct Blocks {
    const int64_t *off;                    // [nblocks + 1] first sample of a block
    const int64_t *unit_start;             // [nblocks + 1] first unit of a block
    int64_t nblocks;
};

// owns the prefix tables on the device: off, and one unit_start per unit length asked for
struct BlockTables : NoCopy {
    int64_t *d_off = nullptr;
    std::vector<int64_t *> d_unit_start;   // in the order of the unit lengths given to fill()
    int64_t nblocks = 0;

    ~BlockTables() { reset(); }
    void reset()
    {
        dev_release(d_off);
        for (int64_t *&p : d_unit_start) dev_release(p);
        d_unit_start.clear();
    }
    // sizes that check_blocks accepted; returns when the tables are on the device
    int fill(const int64_t *sizes, int64_t nb, std::initializer_list<int64_t> unit_lens, hipStream_t st)
    {
        reset();
        nblocks = nb;
        std::vector<int64_t> start((size_t)nb + 1, 0);
        for (int64_t b = 0; b < nb; ++b) start[b + 1] = start[b] + sizes[b];
        if (int rc = dev_put(&d_off, start.data(), start.size(), st)) return rc;
        for (int64_t len : unit_lens) {
            for (int64_t b = 0; b < nb; ++b) start[b + 1] = start[b] + units_of(sizes[b], len);
            d_unit_start.push_back(nullptr);
            if (int rc = dev_put(&d_unit_start.back(), start.data(), start.size(), st)) return rc;
        }
        return 0;
    }
    int64_t bytes() const { return (int64_t)((1 + d_unit_start.size()) * (size_t)(nblocks + 1) * sizeof(int64_t)); }
    Blocks view(size_t k) const { return Blocks{d_off, d_unit_start[k], nblocks}; }
};

// The refusals of a stage's create for the status of its check_create, in the order check_blocks tests.  window_name
// and max_window word the stage's window argument, histograms whose limit kMaxBlocks is.
inline int check_create_status(const char *who, Status ps, int64_t nt, int64_t nblocks, const char *window_name,
                               int window, int max_window, const char *histograms)
{
    CM2_CHECK(ps != kBadSize, "%s: nt=%lld and nblocks=%lld must be >= 1 and the sizes given", who, (long long)nt,
              (long long)nblocks);
    CM2_CHECK(ps != kBadWindow, "%s: %s=%d outside [1, %d]", who, window_name, window, max_window);
    CM2_CHECK(ps != kTooLarge, "%s: nt=%lld does not fit the 32-bit sample counts (nt < 2^32 - 1)", who,
              (long long)nt);
    CM2_CHECK(ps != kBadBlocks, "%s: the %lld block sizes must be positive and add up to nt=%lld", who,
              (long long)nblocks, (long long)nt);
    CM2_CHECK(ps == kOk, "%s: %lld blocks are more than the %lld %s allow", who, (long long)nblocks,
              (long long)kMaxBlocks, histograms);
    return 0;
}

// flag_kind as check_flag_kind takes it
inline int check_flag_kind_status(const char *who, bool have_flags, int flag_kind)
{
    CM2_CHECK(check_flag_kind(have_flags, flag_kind) == kOk,
              "%s: flag_kind=%d is neither 0 (int32, flagged when negative) nor 1 (bytes, flagged when non-zero)", who,
              flag_kind);
    return 0;
}

// disjoint() as a refusal: on_input / on_output are the messages (one "%s" each, for who) of an output that overlaps
// an input / another output
template <size_t NOUT, size_t NIN>
inline int check_disjoint(const char *who, const Range (&outs)[NOUT], const Range (&ins)[NIN], const char *on_input,
                          const char *on_output = nullptr, int alias_out = -1, int alias_in = -1)
{
    const Overlap o = disjoint(outs, (int)NOUT, ins, (int)NIN, alias_out, alias_in);
    CM2_CHECK(o != kOutputOnInput, on_input, who);
    CM2_CHECK(o == kDisjoint, on_output ? on_output : on_input, who);
    return 0;
}

}  // namespace stream
}  // namespace cm2
