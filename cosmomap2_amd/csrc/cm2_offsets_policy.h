// cm2_offsets_policy.h -- the device-free arithmetic of the baseline-offset templates (cm2_offsets.hip): the
// baseline of a sample, the baselines that meet a permutation window, where a (window x baseline) segment's sum
// goes.  Plain C++: tests/test_destriper_cpu.py compiles it with the host compiler and checks it against NumPy.
//
// The stream has noise blocks [off[b], off[b + 1]); block b is cut into K_b = ceil(n_b / L) baselines of L samples,
// the last one of a block may be shorter.  Baseline (b, k) has the global index j = j0[b] + k, j0[b] = sum of K_b'
// over b' < b, na = j0[nb].  Baselines never cross a block boundary.
//
// F^T sums a baseline window by window (windows of kWin samples counted from t = 0): a segment = window x baseline.
// A baseline inside one window is finished there; one that starts before its window's first sample leaves the
// segment's sum in the window's HEAD slot, one that starts in the window and ends after it in the TAIL slot, and
// the combine kernel adds a baseline's slots in ascending window order: tail[w0], head[w0 + 1], ..., head[w1].
#pragma once
#include <cstdint>

#include "cm2_stream_policy.h"

#if defined(__HIPCC__)
#define CM2_OFF_HD __host__ __device__ __forceinline__
#else
#define CM2_OFF_HD inline
#endif

namespace cm2 {
namespace offsets {

constexpr int kWin = 8192;            // samples of a window (= kPermWin of the tile plan)
constexpr int kChunk = 32;            // consecutive samples one thread sums serially
constexpr int kChunks = kWin / kChunk;                 // = threads of a window's workgroup
constexpr int kWinPadded = kWin + kWin / kChunk;       // LDS doubles of a window: one pad word per chunk

// LDS position of window sample q: a thread walks its chunk with stride 1, a wave's 64 chunks start 33 doubles
// apart and fall into different banks
CM2_OFF_HD int pad(int q) { return q + (q >> 5); }

CM2_OFF_HD int64_t baselines_in(int64_t n, int64_t L) { return (n + L - 1) / L; }

// block of sample t: the b with off[b] <= t < off[b + 1]
CM2_OFF_HD int64_t block_of(const int64_t *off, int64_t nb, int64_t t) { return stream::locate(off, nb, t); }

// block of baseline j: the b with j0[b] <= j < j0[b + 1]
CM2_OFF_HD int64_t block_of_baseline(const int64_t *j0, int64_t nb, int64_t j) { return stream::locate(j0, nb, j); }

struct Baseline {
    int64_t j;              // global index
    int64_t start, end;     // samples [start, end)
    int64_t b;              // block
};

// the baseline of sample t, which lies in block b
CM2_OFF_HD Baseline baseline_in_block(const int64_t *off, const int64_t *j0, int64_t b, int64_t L, int64_t t)
{
    Baseline s;
    const int64_t r = t - off[b];
    // nt < 2^32: the quotient of two 32-bit numbers
    const int64_t k = (int64_t)((uint32_t)r / (uint32_t)L);
    s.j = j0[b] + k;
    s.start = off[b] + k * L;
    s.end = s.start + L < off[b + 1] ? s.start + L : off[b + 1];
    s.b = b;
    return s;
}

CM2_OFF_HD Baseline baseline_of(const int64_t *off, const int64_t *j0, int64_t nb, int64_t L, int64_t t)
{
    return baseline_in_block(off, j0, block_of(off, nb, t), L, t);
}

// the baseline after s (s is not the last one)
CM2_OFF_HD Baseline next_baseline(const int64_t *off, const int64_t *j0, int64_t L, const Baseline &s)
{
    Baseline n;
    n.b = s.end == off[s.b + 1] ? s.b + 1 : s.b;
    n.j = s.j + 1;
    n.start = s.end;
    n.end = n.start + L < off[n.b + 1] ? n.start + L : off[n.b + 1];
    return n;
}

// the baselines that meet window w: [*first, *last] (window w holds a sample: w kWin < nt)
CM2_OFF_HD void window_baselines(const int64_t *off, const int64_t *j0, int64_t nb, int64_t L, int64_t nt, int64_t w,
                                 int64_t *first, int64_t *last)
{
    const int64_t t0 = w * kWin, t1 = (t0 + kWin < nt ? t0 + kWin : nt) - 1;
    *first = baseline_of(off, j0, nb, L, t0).j;
    *last = baseline_of(off, j0, nb, L, t1).j;
}

// where the sum of the segment (window starting at t0) x (baseline [start, end)) goes
enum Target { kDirect = 0, kHead = 1, kTail = 2 };
CM2_OFF_HD Target segment_target(int64_t start, int64_t end, int64_t t0)
{
    if (start < t0) return kHead;
    if (end > t0 + kWin) return kTail;
    return kDirect;
}

// side buffer: two slots a window
CM2_OFF_HD int64_t side_slots(int64_t nwin) { return 2 * nwin; }
CM2_OFF_HD int64_t side_slot(int64_t w, Target tg) { return 2 * w + (tg == kTail ? 1 : 0); }

// The window boundary t = w kWin (1 <= w < nwin) is where the combine kernel finishes a baseline, when that baseline
// crosses the boundary and started in window w - 1; *s = that baseline.
CM2_OFF_HD bool combines_at(const int64_t *off, const int64_t *j0, int64_t nb, int64_t L, int64_t w, Baseline *s)
{
    const int64_t t = w * kWin;
    *s = baseline_of(off, j0, nb, L, t);
    return s->start < t && s->start >= t - kWin;
}

}  // namespace offsets
}  // namespace cm2
