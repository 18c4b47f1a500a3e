// cm2_perm_window.h -- the device side of the windowed exchange between time order and tile order, shared by the
// kernels that run on window lists: k_perm_windows (cm2_tiles.hip), k_gap_perm_windows (cm2_gaps.hip),
// k_offsets_from_tiles / k_offsets_to_tiles (cm2_offsets.hip) and k_filter_windows (cm2_filter.hip).
//
// A workgroup of kPermT threads owns a window of kPermWin consecutive time samples and reaches their tile-order
// positions through kPermWin list entries (k, q), sorted by k: k = position in the tile order (kInvalidSample: the
// slot has no sample, or a flagged one), q = offset in the window.  Thread t holds the entries t + u kPermT,
// u < kPermPer, so that a wave reads consecutive entries and, the list being sorted, nearby addresses.  Windows are
// dealt round-robin to the 8 XCDs by the hardware; window_of_workgroup() undoes that, so that consecutive windows
// share an XCD's L2.  The lists are built by cm2::window_lists (cm2_tiles.h).
#pragma once
#include "cm2_tiles.h"

namespace cm2 {

// grid of a window kernel: a multiple of the 8 XCDs (workgroups past the last window return at once)
static inline int window_grid(int64_t nwin) { return (int)(((nwin + 7) / 8) * 8); }

// window of the workgroup: consecutive windows go to the same XCD (I: the kernel's type of nwin)
template <class I>
__device__ __forceinline__ I window_of_workgroup(I nwin)
{
    const int per_xcd = (int)((nwin + 7) / 8);
    return (I)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
}

// samples of the window that starts at t0 = w kPermWin in a stream of nt samples (the kernels narrow it to int)
__device__ __forceinline__ int64_t window_span(int64_t nt, int64_t t0)
{
    return (nt - t0 < kPermWin) ? nt - t0 : kPermWin;
}

// one thread's entries of window w, kept in registers between the gather and the scatter
struct WindowEntries {
    uint32_t k[kPermPer];
    uint16_t q[kPermPer];

    __device__ __forceinline__ void load(const uint32_t *__restrict__ lst_k, const uint16_t *__restrict__ lst_q,
                                         int64_t w)
    {
        const int64_t base = w * kPermWin;
        const int t = threadIdx.x;
#pragma unroll
        for (int u = 0; u < kPermPer; ++u) {
            k[u] = lst_k[base + t + u * kPermT];
            q[u] = lst_q[base + t + u * kPermT];
        }
    }

    // vv[u] = the tile-order value of entry u, 0 where it has none: all loads in flight at once
    __device__ __forceinline__ void gather(const double *__restrict__ src, double (&vv)[kPermPer]) const
    {
#pragma unroll
        for (int u = 0; u < kPermPer; ++u) vv[u] = (k[u] != kInvalidSample) ? src[k[u]] : 0.0;
    }

    // f(u, k, q) for the entries that have a sample.  A callable that stores through pointers of two types takes
    // them by value (k_filter_windows): captured by reference they cost the kernel its instruction order.
    template <class F>
    __device__ __forceinline__ void each_valid(F f) const
    {
#pragma unroll
        for (int u = 0; u < kPermPer; ++u)
            if (k[u] != kInvalidSample) f(u, k[u], q[u]);
    }
};

// first[0] = the smallest sample whose flag differs between the tile plan (tb_dst == kInvalidSample) and
// flagged(flags, i); the body of the compare kernels that cm2::first_flag_mismatch (cm2_tiles.h) launches.  The
// kernel passes its own grid-stride start and step: blockDim read in the __global__ function is the plain
// group-size load, read in an inlined function it is not.
template <class T, class Flagged>
__device__ __forceinline__ void flag_mismatch(int64_t i0, int64_t stride, int64_t nt, const T *__restrict__ flags,
                                              const uint32_t *__restrict__ tb_dst, uint32_t *__restrict__ first,
                                              Flagged flagged)
{
    for (int64_t i = i0; i < nt; i += stride)
        if ((tb_dst[i] == kInvalidSample) != flagged(flags, i)) atomicMin(first, (uint32_t)i);
}

}  // namespace cm2
