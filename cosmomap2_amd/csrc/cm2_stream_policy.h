// cm2_stream_policy.h -- what the stages over the noise blocks of a time stream agree on (cm2_glitch, cm2_jump; the
// bisection also cm2_gaps, cm2_offsets, cm2_noise_model): how blocks are cut into units and workgroups laid over them,
// which block sizes and flag kinds are accepted, and which arrays of a call may share memory.  Plain C++: the stage
// policy headers include it, tests/test_glitch_cpu.py and tests/test_jump_cpu.py compile it with the host compiler.
//
// The stream is nblocks noise blocks one after the other, block b the samples [off[b], off[b + 1]).  A *unit* is
// unit_len consecutive samples of one block (the last unit of a block may be shorter); block b has units_of(size_b,
// unit_len) of them and the units of the stream are numbered block after block, unit_start[b] the first of block b.
// Thread or workgroup g takes unit g: no unit crosses a block, every sample belongs to exactly one unit, and blocks of
// any size pack the units densely.  A *tile* is the unit of kTile samples that one workgroup takes.
#pragma once
#include <cstdint>

namespace cm2 {
namespace stream {

constexpr int kTile = 2048;                               // samples of one workgroup
constexpr int64_t kMaxBlocks = (int64_t)1 << 18;          // 2^18 x 2048 x 4 bytes = 2 GB of histograms (cm2_glitch)

// the codes the stages share; a stage adds its own (7, 9, ...) as constants of this type
enum Status : int {
    kOk = 0,
    kBadSize = 1,          // nt < 1, nblocks < 1 or no sizes
    kBadBlocks = 2,        // a size < 1, or the sizes do not add up to nt
    kBadWindow = 3,        // the stage's window (half-width, half-window) outside its range
    kTooLarge = 4,         // nt >= 2^32 - 1 (the limit of cm2_gaps)
    kTooManyBlocks = 5,    // nblocks > kMaxBlocks
    kBadNsigma = 6,        // not finite or <= 0
    kBadFlagKind = 8       // flags given with a kind other than 0 or 1
};

// ---- layout -----------------------------------------------------------------------------------------------------
constexpr int64_t units_of(int64_t size, int64_t unit_len) { return (size + unit_len - 1) / unit_len; }
constexpr int64_t tiles_of(int64_t size) { return units_of(size, kTile); }

// the block of unit u: the largest b in [0, nblocks) with start[b] <= u; start[0] = 0 and start ascends strictly
// (every block has at least one sample).  (constexpr: callable from device code as well)
constexpr int64_t locate(const int64_t *start, int64_t nblocks, int64_t u)
{
    int64_t lo = 0, hi = nblocks;              // start[lo] <= u < start[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

struct Span {
    int64_t block = 0, first = 0, end = 0;     // the samples [first, end) of the stream, all of one block
};

// unit g of the stream
constexpr Span unit_span(const int64_t *off, const int64_t *unit_start, int64_t nblocks, int64_t unit_len, int64_t g)
{
    Span s;
    s.block = locate(unit_start, nblocks, g);
    s.first = off[s.block] + (g - unit_start[s.block]) * unit_len;
    s.end = s.first + unit_len < off[s.block + 1] ? s.first + unit_len : off[s.block + 1];
    return s;
}

// tile w of the stream
constexpr Span tile_span(const int64_t *off, const int64_t *tile_start, int64_t nblocks, int64_t w)
{
    return unit_span(off, tile_start, nblocks, kTile, w);
}

// ---- accepted arguments -----------------------------------------------------------------------------------------
// The block sizes of a create: given, positive and adding up to nt, nt < 2^32 - 1 (which keeps the unit counts, grid
// dimensions, below 2^31 and every count of a histogram in 32 bits), at most kMaxBlocks blocks.  window_ok is the
// stage's verdict on its own window argument; it is looked at after the sizes are known to be given and before
// anything else, so an input with two faults gets the code it always got.
inline Status check_blocks(int64_t nt, const int64_t *sizes, int64_t nblocks, bool window_ok)
{
    if (nt < 1 || nblocks < 1 || !sizes) return kBadSize;
    if (!window_ok) return kBadWindow;
    if (nt >= (((int64_t)1 << 32) - 1)) return kTooLarge;
    if (nblocks > nt) return kBadBlocks;
    int64_t sum = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (sizes[b] < 1 || sizes[b] > nt - sum) return kBadBlocks;
        sum += sizes[b];
    }
    if (sum != nt) return kBadBlocks;
    if (nblocks > kMaxBlocks) return kTooManyBlocks;
    return kOk;
}

// units of the whole stream (sizes that check_blocks accepted)
inline int64_t total_units(const int64_t *sizes, int64_t nblocks, int64_t unit_len)
{
    int64_t n = 0;
    for (int64_t b = 0; b < nblocks; ++b) n += units_of(sizes[b], unit_len);
    return n;
}

inline Status check_flag_kind(bool have_flags, int kind)
{
    return have_flags && kind != 0 && kind != 1 ? kBadFlagKind : kOk;
}

inline Status check_nsigma(double nsigma)
{
    return nsigma > 0.0 && nsigma <= 1.7976931348623157e308 ? kOk : kBadNsigma;      // (a NaN fails the first)
}

// ---- arrays that must not share memory --------------------------------------------------------------------------
struct Range {
    const void *p;         // NULL: an array the caller left out, it overlaps nothing
    uint64_t bytes;
};

inline bool overlap(const Range &a, const Range &b)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}

enum Overlap { kDisjoint = 0, kOutputOnInput = 1, kOutputOnOutput = 2 };

// Does an output share a byte with an input or with another output?  The outputs are taken in order, each against
// every input and then against the outputs after it, and the first pair that overlaps is the answer.  The pair
// (outs[alias_out], ins[alias_in]) may be one and the same pointer -- a kernel whose threads each read and write
// their own samples runs in place -- but may not overlap in any other way; -1: no such pair.
inline Overlap disjoint(const Range *outs, int nout, const Range *ins, int nin, int alias_out = -1, int alias_in = -1)
{
    for (int a = 0; a < nout; ++a) {
        for (int b = 0; b < nin; ++b) {
            const bool same = a == alias_out && b == alias_in && outs[a].p == ins[b].p;
            if (!same && overlap(outs[a], ins[b])) return kOutputOnInput;
        }
        for (int b = a + 1; b < nout; ++b)
            if (overlap(outs[a], outs[b])) return kOutputOnOutput;
    }
    return kDisjoint;
}

}  // namespace stream
}  // namespace cm2
