// cm2_fourier_policy.h -- the device-free arithmetic of the Fourier filter (cm2_fourier.hip): which arguments are
// accepted, the transform length of a block, how the blocks are grouped by length and how many rows one rocFFT batch
// of a length holds.  Plain C++: tests/test_fourier_cpu.py compiles it with the host compiler and checks it against
// Python.
//
// cm2_stream_policy.h has the blocks and the checks every stage shares; its names are reachable as cm2::fourier:: too.
//
// Lengths.  Block b of n samples is transformed at L = fft_length(n, pad): the smallest even integer >= max(2, n + pad)
// whose prime factors all lie in {2, 3, 5, 7}, L <= 2^28.  Blocks of one L form a *group* and share a plan; at most
// kMaxLengths groups.
//
// Rows.  One row of a batch is one block: L doubles and L/2 + 1 double2, row_bytes(L) = 8 L + 16 (L/2 + 1).  A batch
// of a group starts at first_batch(L, blocks, max_work_bytes) rows: at most kBatchSamples / L (as the Welch PSD sizes
// its batch), at most what max_work_bytes holds, at most the blocks of the group, at least one.  The work buffer the
// library asks for counts against max_work_bytes too: batch_fits() is the test, the batch is halved until it passes,
// and a single row that fails it is refused with the bytes it needs.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "cm2_stream_policy.h"

namespace cm2 {
namespace fourier {

using namespace stream;

constexpr int kThreads = 256;
constexpr int kSegment = 4096;                              // samples of a row one workgroup packs or unpacks
constexpr int kMaxOrder = 16;                               // 1 <= p, q <= 16
constexpr int kMaxNotch = 16;                               // J <= 16
constexpr int kMaxEndMean = 1024;                           // 1 <= end_mean <= 1024
constexpr int kMaxLengths = 8;                              // distinct L of one handle
constexpr int64_t kMaxLength = (int64_t)1 << 28;            // L <= 2^28
constexpr int64_t kBatchSamples = (int64_t)1 << 24;         // rows of a batch * L, at most (128 MB of input)
constexpr int64_t kDefaultWorkBytes = (int64_t)512 << 20;

enum Mode { kDeconvolve = 0, kConvolve = 1 };
enum Detrend { kNone = 0, kEnds = 1 };
enum TableKind { kNoTable = 0, kRealTable = 1, kComplexTable = 2 };

// the codes of this stage beside the shared ones (the demodulator's end at 16)
constexpr Status kBadRate = Status(17);            // fs not finite or <= 0
constexpr Status kBadMode = Status(18);            // mode or conjugate other than 0 or 1
constexpr Status kBadTau = Status(19);             // a time constant that is negative or not finite
constexpr Status kBadCut = Status(20);             // a cut-off that is negative or not finite, an order outside [1, 16]
constexpr Status kBadNotch = Status(21);           // more than 16, no list, f0 not finite, w not finite or <= 0
constexpr Status kBadTable = Status(22);           // kind outside 0..2, Rn < 2, no values, per_block other than 0 or 1
constexpr Status kBadTableValue = Status(23);      // a table value that is not finite
constexpr Status kBadDetrend = Status(24);         // detrend other than 0 or 1, end_mean outside [1, 1024]
constexpr Status kBadPad = Status(25);             // pad < 0, or a block whose L would exceed 2^28
constexpr Status kTooManyLengths = Status(26);     // more than 8 distinct L
constexpr Status kRowTooLarge = Status(27);        // one row and its plan do not fit max_work_bytes

// ---- lengths ------------------------------------------------------------------------------------------------------
constexpr bool smooth7(int64_t v)
{
    for (int p : {2, 3, 5, 7})
        while (v % p == 0) v /= p;
    return v == 1;
}

// 0: no such L <= kMaxLength (or n < 1, pad < 0)
constexpr int64_t fft_length(int64_t n, int64_t pad)
{
    if (n < 1 || pad < 0 || n > kMaxLength || pad > kMaxLength) return 0;
    int64_t L = n + pad < 2 ? 2 : n + pad;
    L += L & 1;
    for (; L <= kMaxLength; L += 2)
        if (smooth7(L)) return L;
    return 0;
}

static_assert(fft_length(1, 0) == 2 && fft_length(3, 0) == 4 && fft_length(1000, 24) == 1024 &&
              fft_length(4097, 1024) == 5184, "the lengths the definition names");

// ---- rows and batches ---------------------------------------------------------------------------------------------
constexpr int64_t row_bytes(int64_t L) { return 8 * L + 16 * (L / 2 + 1); }
constexpr int64_t segments(int64_t len) { return units_of(len, kSegment); }

constexpr int64_t first_batch(int64_t L, int64_t blocks, int64_t max_work_bytes)
{
    int64_t batch = kBatchSamples / L;
    if (batch * row_bytes(L) > max_work_bytes) batch = max_work_bytes / row_bytes(L);
    if (batch > blocks) batch = blocks;
    return batch < 1 ? 1 : batch;
}
constexpr bool batch_fits(int64_t L, int64_t batch, int64_t plan_bytes, int64_t max_work_bytes)
{
    return batch * row_bytes(L) + plan_bytes <= max_work_bytes;
}
constexpr int64_t batches(int64_t blocks, int64_t batch) { return units_of(blocks, batch); }

// ---- the accepted arguments ---------------------------------------------------------------------------------------
// what the response needs, as the kernels take it by value
struct Response {
    double fs = 0.0, f_lp = 0.0, f_hp = 0.0;
    int mode = 0, p = 1, q = 1, nnotch = 0, conjugate = 0;
    int table_kind = 0, table_per_block = 0;
    int64_t Rn = 0;
    double notch[2 * kMaxNotch] = {0.0};           // (f0_j, w_j)
};

struct Group {
    int64_t L = 0, blocks = 0, batch = 0;          // batch is set by the create (first_batch, then halved)
};

struct Launch {
    int64_t nt = 0, nblocks = 0, pad = 0;
    int detrend = 0, end_mean = 0;
    Response resp;
    std::vector<Group> groups;                     // in the order their first block appears
    std::vector<int32_t> group_of;                 // [nblocks]
};

inline bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// fills *l (the batches are left 0); anything but kOk leaves it unspecified.  The order of the tests: the sizes given,
// the 32-bit limit, the blocks and their number (check_blocks), the rate, mode and conjugate, the time constants, the
// cut-offs, the notches, the table, the trend, the padding and the lengths.
inline Status check_create(Launch *l, int64_t nt, const int64_t *sizes, int64_t nblocks, double fs, const double *tau,
                           int mode, double f_lp, int p, double f_hp, int q, const double *notch, int nnotch,
                           const double *table, int64_t Rn, int table_kind, int table_per_block, int detrend,
                           int end_mean, int64_t pad, int conjugate)
{
    const Status st = check_blocks(nt, sizes, nblocks, true);
    if (st != kOk) return st;
    if (!(std::isfinite(fs) && fs > 0.0)) return kBadRate;
    if ((mode != kDeconvolve && mode != kConvolve) || (conjugate != 0 && conjugate != 1)) return kBadMode;
    if (tau)
        for (int64_t b = 0; b < nblocks; ++b)
            if (!finite_nonneg(tau[b])) return kBadTau;
    if (!finite_nonneg(f_lp) || !finite_nonneg(f_hp) || p < 1 || p > kMaxOrder || q < 1 || q > kMaxOrder)
        return kBadCut;
    if (nnotch < 0 || nnotch > kMaxNotch || (nnotch > 0 && !notch)) return kBadNotch;
    for (int j = 0; j < nnotch; ++j)
        if (!std::isfinite(notch[2 * j]) || !(std::isfinite(notch[2 * j + 1]) && notch[2 * j + 1] > 0.0))
            return kBadNotch;
    if (table_kind < kNoTable || table_kind > kComplexTable) return kBadTable;
    if (table_kind != kNoTable) {
        if (!table || Rn < 2 || Rn > kMaxLength || (table_per_block != 0 && table_per_block != 1)) return kBadTable;
        const int64_t count = (table_per_block ? nblocks : 1) * Rn * (table_kind == kComplexTable ? 2 : 1);
        for (int64_t i = 0; i < count; ++i)
            if (!std::isfinite(table[i])) return kBadTableValue;
    }
    if ((detrend != kNone && detrend != kEnds) || end_mean < 1 || end_mean > kMaxEndMean) return kBadDetrend;
    if (pad < 0) return kBadPad;
    l->nt = nt;
    l->nblocks = nblocks;
    l->pad = pad;
    l->detrend = detrend;
    l->end_mean = end_mean;
    Response &r = l->resp;
    r = Response();
    r.fs = fs;
    r.f_lp = f_lp;
    r.f_hp = f_hp;
    r.mode = mode;
    r.p = p;
    r.q = q;
    r.nnotch = nnotch;
    r.conjugate = conjugate;
    r.table_kind = table_kind;
    r.table_per_block = table_kind != kNoTable ? table_per_block : 0;
    r.Rn = table_kind != kNoTable ? Rn : 0;
    for (int j = 0; j < 2 * nnotch; ++j) r.notch[j] = notch[j];
    l->groups.clear();
    l->group_of.assign((size_t)nblocks, 0);
    int64_t last_n = 0, last_L = 0;                // consecutive blocks of one size are the common case
    for (int64_t b = 0; b < nblocks; ++b) {
        if (sizes[b] != last_n) {
            last_n = sizes[b];
            last_L = fft_length(last_n, pad);
        }
        if (last_L == 0) return kBadPad;
        size_t g = 0;
        while (g < l->groups.size() && l->groups[g].L != last_L) ++g;
        if (g == l->groups.size()) {
            if (g == (size_t)kMaxLengths) return kTooManyLengths;
            l->groups.push_back(Group{last_L, 0, 0});
        }
        l->groups[g].blocks += 1;
        l->group_of[(size_t)b] = (int32_t)g;
    }
    return kOk;
}

}  // namespace fourier
}  // namespace cm2
