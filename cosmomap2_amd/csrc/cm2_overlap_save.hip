// cm2_overlap_save.hip -- banded-Toeplitz N^-1 by overlap-save, ONE REAL WINDOW per workgroup.
//
// Reference semantics: ToeplitzLO.mult, interfaces/linearoperators.py:582-595 (symmetric band,
// ZERO boundary at both ends of every block), dispatched per block as interfaces/blkop.py:195-206.
//
// One workgroup (256 threads x 32 complex points in registers, LDS only as the exchange buffer between
// the radix-32 / 16 / 16 passes: 66 KB, two workgroups per CU) transforms one real window of 2N =
// 16384 samples as a complex signal of N = 8192 points
//
//     z[a] = x[2a] + i x[2a+1],   Z = FFT_N(z),
//     Z'[k] = alpha_k Z[k] + i beta_k conj(Z[N-k]),   z' = IFFT_N(Z') = y[2a] + i y[2a+1]
//
// with two real tables per noise block, alpha = (S - D sin(pi k/N)) / N, beta = D cos(pi k/N) / N,
// S, D = (H[k] +- H[k+N]) / 2 and H the band's real, even spectrum on 2N points: no untangling pass;
// the partner bin N-k lives in ONE other thread (k' = N-k is (263 - t, 31 - m) in the digit-reversed
// register layout), so the pairing costs one more plane exchange.  12288 outputs per window (halo
// 2048 >= lambda - 1 on both sides: overlap 1.33).
//
// On the tile-bucketed order the window is reached through address-sorted lists, in one of three
// formats:
//   plain : a 4-byte address and a 2-byte position per entry (plans with more than 2048 tiles);
//   RC    : run-coded -- a window's samples in one pixel tile are consecutive addresses, so a list is
//           a few hundred runs: per entry 2 bytes (position, bit 15 = "a run starts here"), per run
//           one 4-byte word delta = address - slot, staged in LDS; entry s of run r has address
//           delta[r] + s, r from a ballot and a population count.  2.0 + 4 / run length bytes per
//           entry instead of 6.  Two window halves and two result rounds, each sorted by address;
//   inverse : one address-sorted order per window (and per result window), cut by ADDRESS into rounds.
// History (profiles/r03_*): the segment-pair kernel of rounds 1-2 (cm2_fft.hip,
// A + iB packing: 0.89-0.95 ms at C4), a 16-point / four-workgroups-per-CU variant of this kernel
// (1.00-1.06 ms) and a 512-thread x 16-point variant of the same window (1.28 ms) all lost to this one
// (0.75-0.80 ms) and were removed in round 4.
// The geometry and the host's decisions are in cm2_os_policy.h, the lists' structures and their plan-time
// builders in cm2_os_lists.h / cm2_os_lists.hip.  This translation unit is compiled with FMA contraction
// ON (results are not promised bit for bit: every element is held to c 2^-53 B_i, B_i = A1 ||window||_2 / sqrt(W)
// against an extended-precision band sum, tests/_noise_ref.py and tests/test_gpu_noise_kernels.py).
#include "cm2_os_lists.h"

#include <cstring>
#include <memory>
#include <mutex>

using namespace cm2;

namespace {

constexpr double kCos32[32] = {1.0, 0.9807852804032304, 0.9238795325112867, 0.8314696123025452, 0.7071067811865476, 0.5555702330196022, 0.3826834323650898, 0.19509032201612828, 0.0, -0.19509032201612828, -0.3826834323650898, -0.5555702330196022, -0.7071067811865476, -0.8314696123025452, -0.9238795325112867, -0.9807852804032304, -1.0, -0.9807852804032304, -0.9238795325112867, -0.8314696123025452, -0.7071067811865476, -0.5555702330196022, -0.3826834323650898, -0.19509032201612828, 0.0, 0.19509032201612828, 0.3826834323650898, 0.5555702330196022, 0.7071067811865476, 0.8314696123025452, 0.9238795325112867, 0.9807852804032304};
constexpr double kSin32[32] = {0.0, 0.19509032201612828, 0.3826834323650898, 0.5555702330196022, 0.7071067811865476, 0.8314696123025452, 0.9238795325112867, 0.9807852804032304, 1.0, 0.9807852804032304, 0.9238795325112867, 0.8314696123025452, 0.7071067811865476, 0.5555702330196022, 0.3826834323650898, 0.19509032201612828, 0.0, -0.19509032201612828, -0.3826834323650898, -0.5555702330196022, -0.7071067811865476, -0.8314696123025452, -0.9238795325112867, -0.9807852804032304, -1.0, -0.9807852804032304, -0.9238795325112867, -0.8314696123025452, -0.7071067811865476, -0.5555702330196022, -0.3826834323650898, -0.19509032201612828};

__host__ __device__ constexpr int ilog2(int r) { return r <= 1 ? 0 : 1 + ilog2(r >> 1); }

template <int R>
__host__ __device__ constexpr int brev(int m)
{
    int out = 0;
    for (int b = 0; b < ilog2(R); ++b) out |= ((m >> b) & 1) << (ilog2(R) - 1 - b);
    return out;
}

// What was measured and dropped (each was a compile-time switch of this source until round 4; the
// numbers are in profiles/r03_os_knob_builds.jsonl and DESIGN.md section 3.1): (alpha, beta) in
// batches of 8 bins requested in front of the last forward pass, both window halves' gathers in
// flight together, both result rounds' lists requested up front, the second inverse-list round's
// gathers behind the first round's staging, wave priorities, non-temporal gathers and result stores.
// Kept: non-temporal LIST loads (a list is read once).
template <class T> __device__ __forceinline__ T ld_list(const T *p) { return __builtin_nontemporal_load(p); }


// Diagnostic build only (-DCM2_OS_STAMPS, never in the shipped library): every workgroup records
// s_memtime at its phase boundaries into a buffer of 8 words per window (profiles/scripts/
// os_stamps.py).  Every lane stores: a branch at a phase boundary splits the kernel's one basic
// block and costs the register allocator 70-150 spilled VGPRs, which would time a different kernel.
// TIMING-ONLY builds (wrong results, never shipped; profiles/r05_os_memory_vs_compute.md): -DCM2_OS_TIMING=1 compiles
// the transforms, their LDS exchanges and the pairing out -- what is left is the window's memory side (lists, run
// tables, gathers, staging, result lists, stores) exactly as the kernel issues it.
#ifndef CM2_OS_TIMING
#define CM2_OS_TIMING 0
#endif
#if CM2_OS_TIMING & 1
#define OS_XF(...) do { } while (0)
#else
#define OS_XF(...) do { __VA_ARGS__; } while (0)
#endif

#ifdef CM2_OS_STAMPS
static unsigned long long *g_os_stamps_host = nullptr;      // set by cm2_os_debug_stamps
static unsigned long long *os_stamp_buf()                   // never NULL: a dummy when none is wanted
{
    static unsigned long long *dummy = nullptr;
    if (g_os_stamps_host) return g_os_stamps_host;
    if (!dummy && cm2::dev_malloc(&dummy, sizeof(unsigned long long) * 8 * (1 << 20)) != hipSuccess) abort();
    return dummy;
}
#define OS_STAMP_PARAM , unsigned long long *__restrict__ stamps
#define OS_STAMP_ARG , os_stamp_buf()
#define OS_STAMP(i) (stamps[(int64_t)win * 8 + (i)] = __builtin_amdgcn_s_memtime())
#else
#define OS_STAMP_PARAM
#define OS_STAMP_ARG
#define OS_STAMP(i) do { } while (0)
#endif

// ---- register layouts, as in cm2_fft.hip ----------------------------------------------------
//   P1: a = t + 256 m                      radix-32 pass over stride 256     (n = N)
//   P2: a = (16 (m>>4) + (t>>4)) 256 + (t&15) + 16 (m&15)      radix-16 over stride 16 (n = 256)
//   P3: a = 32 t + m                         radix-16 on contiguous points
// padded LDS index padi(a) = a + (a >> 5) split into a per-thread base and a compile-time offset
template <int L>
__device__ __forceinline__ int reg_base(int t)
{
    if (L == 1) return t + (t >> 5);
    if (L == 2) return (t >> 4) * 264 + (t & 15);
    return 33 * t;
}
template <int L>
__host__ __device__ constexpr int reg_off(int m)
{
    return L == 1 ? 264 * m : (L == 2 ? 4224 * (m >> 4) + 16 * (m & 15) + ((m & 15) >> 1) : m);
}
// where slot m of the array sits after in-place butterflies (dft_sub leaves output m of a radix-R
// block at index brev<R>(m)): PERM = 0 natural, 32 one radix-32 block, 16 radix-16 blocks
template <int PERM>
__host__ __device__ constexpr int reg_slot(int m)
{
    return PERM == 32 ? brev<32>(m) : (PERM == 16 ? 16 * (m >> 4) + brev<16>(m & 15) : m);
}

template <int FROM, int TO, int PERM>
__device__ __forceinline__ void reg_exchange(double (&a)[kPts], double *__restrict__ buf, int t)
{
    double *__restrict__ wp = buf + reg_base<FROM>(t);
    const double *__restrict__ rp = buf + reg_base<TO>(t);
#pragma unroll
    for (int m = 0; m < kPts; ++m) wp[reg_off<FROM>(m)] = a[reg_slot<PERM>(m)];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kPts; ++m) a[m] = rp[reg_off<TO>(m)];
    __syncthreads();
}

// in-place decimation-in-frequency butterflies on the sub-block [OFF, OFF + R)
template <int R, int OFF>
__device__ __forceinline__ void dft_sub(double (&re)[kPts], double (&im)[kPts])
{
#pragma unroll
    for (int h = R / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const int a = OFF + blk + i, b = a + h;
                const int tw = i * (32 / (2 * h));
                const double ar = re[a], ai = im[a], br = re[b], bi = im[b];
                re[a] = ar + br;
                im[a] = ai + bi;
                const double dr = ar - br, di = ai - bi;
                if (tw == 0) {
                    re[b] = dr;
                    im[b] = di;
                } else if (tw == 8) {
                    re[b] = di;
                    im[b] = -dr;
                } else {
                    const double c = kCos32[tw], s = kSin32[tw];
                    re[b] = dr * c + di * s;
                    im[b] = di * c - dr * s;
                }
            }
        }
    }
}

// decimation-in-time counterpart: input m at index brev<R>(m), output natural
template <int R, int OFF>
__device__ __forceinline__ void dit_sub(double (&re)[kPts], double (&im)[kPts])
{
#pragma unroll
    for (int h = 1; h <= R / 2; h <<= 1) {
#pragma unroll
        for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const int a = OFF + blk + i, b = a + h;
                const int tw = i * (32 / (2 * h));
                double tr, ti;
                if (tw == 0) {
                    tr = re[b];
                    ti = im[b];
                } else if (tw == 8) {
                    tr = im[b];
                    ti = -re[b];
                } else {
                    const double c = kCos32[tw], s = kSin32[tw];
                    tr = re[b] * c + im[b] * s;
                    ti = im[b] * c - re[b] * s;
                }
                const double ar = re[a], ai = im[a];
                re[a] = ar + tr;
                im[a] = ai + ti;
                re[b] = ar - tr;
                im[b] = ai - ti;
            }
        }
    }
}

// forward pass on a block: butterfly, then output m (at index brev(m)) times w1^m
template <int R, int OFF>
__device__ __forceinline__ void reg_fwd(double (&xr)[kPts], double (&xi)[kPts], double2 w1)
{
    dft_sub<R, OFF>(xr, xi);
    double cr = 1.0, ci = 0.0;
#pragma unroll
    for (int m = 1; m < R; ++m) {
        const double nr = cr * w1.x - ci * w1.y;
        ci = cr * w1.y + ci * w1.x;
        cr = nr;
        const int i = OFF + brev<R>(m);
        const double tr = xr[i] * cr - xi[i] * ci;
        xi[i] = xr[i] * ci + xi[i] * cr;
        xr[i] = tr;
    }
}

// inverse pass on a block: input m (natural index) times conj(w1^m), then the inverse butterfly
// (swap . forward . swap); output m ends at index brev(m)
template <int R, int OFF>
__device__ __forceinline__ void reg_inv(double (&xr)[kPts], double (&xi)[kPts], double2 w1)
{
    double cr = 1.0, ci = 0.0;
#pragma unroll
    for (int m = 1; m < R; ++m) {
        const double nr = cr * w1.x - ci * w1.y;
        ci = cr * w1.y + ci * w1.x;
        cr = nr;
        const int i = OFF + m;
        const double tr = xr[i] * cr + xi[i] * ci;
        xi[i] = xi[i] * cr - xr[i] * ci;
        xr[i] = tr;
    }
    dft_sub<R, OFF>(xi, xr);
}

typedef unsigned int v2u_t __attribute__((ext_vector_type(2)));
// this thread's E list words, two per register
template <int E>
__device__ __forceinline__ void q_request(const uint16_t *q, int t, uint32_t (&qq)[E / 2])
{
    asm volatile("" : "+v"(t));               // (the lane's list offset is recomputed per list, not kept: see tab_dma)
    const v2u_t *p = reinterpret_cast<const v2u_t *>(q) + (E / 4) * 64 * (t >> 6) + (t & 63);
#pragma unroll
    for (int i = 0; i < E / 4; ++i) {
        const v2u_t v = __builtin_nontemporal_load(p + 64 * i);
        qq[2 * i] = v.x;
        qq[2 * i + 1] = v.y;
    }
}
template <int E2>
__device__ __forceinline__ uint32_t q_word(const uint32_t (&qq)[E2], int u) { return (qq[u >> 1] >> (16 * (u & 1))) & 0xFFFFu; }

struct ListArgs {
    const uint32_t *k;        // plain: addresses of this list
    const uint16_t *q;        // plain / RC: positions of this list
    const ListHdr *hdr;       // RC
    const uint32_t *tab;      // RC: run table of this list in global memory
};

// RC: the run table of a list (rmax words, a multiple of 64; the table is read up to its ALLOCATED
// length, so the request does not wait for the list header) goes from global memory straight into
// LDS (global_load_lds_dword: lane l of a wave writes word l behind the wave-uniform LDS base in M0):
// no VGPR holds a table word.  The data is in LDS once the issuing wave's vmcnt has drained; the
// __syncthreads() that publishes it to the other waves waits for that (the compiler puts
// s_waitcnt vmcnt(0) in front of the barrier).
// At most kTabRows requests per wave (rmax <= 256 kTabRows), unrolled behind wave-uniform tests: with a
// loop of unknown length the compiler cannot count the requests in flight and every later wait for
// an OLDER load becomes s_waitcnt vmcnt(0), i.e. a wait for the table and the list words as well.
__device__ __forceinline__ void tab_dma(const uint32_t *gtab, uint32_t *tab_lds, int rmax, int wave_, int t)
{
    // (the wave index passes through an empty asm statement at every call: the eight wave-uniform tests below
    //  are then scalar compares made where they are used -- shared between the window lists at the top of the
    //  kernel and the result lists at its end they were eight 64-bit masks kept across the whole transform,
    //  16 SGPRs spilled to VGPR lanes in the default instantiation)
    int wave = wave_;
    asm volatile("" : "+s"(wave));
    // (and the thread index through a "+v": the lane's 64-bit table offset is recomputed at every call -- three
    //  VALU instructions -- instead of being kept, or spilled, from the window lists to the result lists)
    asm volatile("" : "+v"(t));
    const uint32_t *g = gtab + 64 * wave + (t & 63);
#pragma unroll
    for (int i = 0; i < kTabRows; ++i)
        if (64 * wave + kT * i < rmax)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + kT * i),
                                             (__attribute__((address_space(3))) void *)(tab_lds + 64 * wave + kT * i),
                                             4, 0, 0);
}

// RC / inverse lists: addresses of the E slots s0 + 64 u from the run table in LDS.  The run of a slot = the runs in
// front of the wave's first slot (wbase) + the run starts up to the slot, from a ballot and a population count;
// starts(u): a run starts at this thread's entry u.
template <int E, class F>
__device__ __forceinline__ void run_decode(F starts, const uint32_t *__restrict__ tab_lds, int wbase, uint32_t nvalid,
                                           uint32_t s0, uint32_t (&kk)[E])
{
    int rb = wbase;
    // slot of entry u = s0 + 64 u; s0 passes through an empty asm statement so that the E slot
    // numbers are recomputed here (one add each) instead of being kept live from list to list
    asm volatile("" : "+v"(s0));
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const bool flag = starts(u);
        const uint64_t mask = __ballot(flag);
        const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        int r = rb + below + (flag ? 1 : 0);
        rb += __popcll(mask);
        r = r < 0 ? 0 : r;
        const uint32_t s = s0 + 64u * (uint32_t)u;
        const uint32_t a = tab_lds[r] + s;           // read for every entry: no branch, no wait per entry
        kk[u] = s < nvalid ? a : kInvalidSample;
    }
}
// RC: the flag is bit 15 of an entry's 16-bit word
template <int E>
__device__ __forceinline__ void rc_decode(const uint32_t (&qq)[E / 2], const uint32_t *__restrict__ tab_lds,
                                          int wbase, uint32_t nvalid, int t, uint32_t (&kk)[E])
{
    run_decode<E>([&](int u) { return (qq[u >> 1] & (0x8000u << (16 * (u & 1)))) != 0u; }, tab_lds, wbase, nvalid,
                  (uint32_t)slot_of<E>(t, 0), kk);
}

// ---- inverse lists (MODE 3) ----------------------------------------------------------------------
// The lists above are cut by TIME (two window halves, two result rounds), each sorted by address: a
// tile's samples of one window are consecutive addresses, but a half window holds only half of them
// (runs of 16 entries = 128 bytes at C4, 12 = 96 bytes on the result side), and every run ends in
// partly used 64-byte sectors.  An inverse list keeps ONE address-sorted order per window (and one per
// result window) and cuts it by ADDRESS: round j moves slots [j R, (j + 1) R) -- whole runs of 32
// (24) entries -- linearly through the LDS buffer, and every thread picks (or places) its own points
// by slot number: the list stored per POSITION is its slot (u16, 0xFFFF = no sample), read in
// register order.  The slot -> address direction needs only the run table and one bit per slot (a
// run starts here), kept transposed: bit u of word [round][thread] belongs to the thread's u-th slot
// of that round.

// this thread's E slots of the round that starts at list slot `soff`: the flag is bit u of the round's flag word
template <int E>
__device__ __forceinline__ void idecode(uint32_t fw, const uint32_t *__restrict__ tab_lds, int wbase,
                                        uint32_t nvalid, uint32_t soff, int t, uint32_t (&kk)[E])
{
    run_decode<E>([&](int u) { return ((fw >> u) & 1u) != 0u; }, tab_lds, wbase, nvalid,
                  soff + (uint32_t)slot_of<E>(t, 0), kk);
}

// ---- the partner exchange and the spectrum product: pairing by HALF PLANES (round 5) ------------------
// Z'[k] = alpha Z[k] + i beta conj(Z[N-k]):  re' = alpha re + beta pim,  im' = alpha im + beta pre.
// Frequency (e, d3) of a thread sits in register slot 16 e + brev16(d3), P3 index m = 16 e + d3.
// Rounds 3-4 published the real plane, read the partner's 32 real parts into registers (64 VGPRs), published the
// imaginary plane and walked the bins with ONE batch of four (alpha, beta) pairs in flight: eight dependent table
// loads a window, seven of them exposed (19 k of the window's 109 k clocks).  Here a thread publishes only its
// UPPER slots (P3 index 16..31), both parts, in the one plane buffer -- real part at 33 t + 16 + j, imaginary
// part at 33 t + j -- and the holder of the LOWER slot of a bin pair (k, N - k) computes BOTH outputs: it has
// Z[k] in registers, reads Z[N-k] from the partner's published slots, writes Z'[N-k] back to the same two words
// (no other thread touches them), and the partner reads its new upper slots back behind one barrier.  No partner
// array in registers: the coefficients travel in TWO batches of eight bin pairs (16 double2 = the partner
// array's 64 registers), the first requested in front of the publication: one exposed round trip instead of
// seven; three barriers instead of four; the same LDS reads, 32 more LDS writes per thread.  (All 32 double2 at
// once, into the upper slots' registers that are dead between publication and read-back, was tried: the
// register allocator spills 100 VGPRs.)  Five same-box alternations of bench.py: N^-1 0.673 against 0.696 ms
// (every pair), step 1.378 against 1.390 (four of five pairs); profiles/r05_os_half_plane_pairing_ab.jsonl.
//   t >= 8: (t, m < 16) pairs with (263 - t, 31 - m): lower <-> upper.
//   t <  8 (frequency digit d1 = 0: 8 threads of wave 0): lower slots pair with LOWER slots (thread 8 - t, slot
//   15 - m; thread 0 with itself, slot 16 - m; bins 0 and N/2 with themselves) and upper with upper (thread
//   7 - t, slot 47 - m).  They also publish their lower slots (xbuf: 2 x 8 x 16 doubles behind the run tables),
//   compute their own 32 bins from the published ORIGINALS (nobody writes to their slots: the partners of
//   threads >= 8 are threads 8..255) with the same two batches of loads -- their "partner" coefficients are their
//   own upper bins' -- and skip the read-back.
template <int BP>                   // BP: bin pairs per coefficient batch (8; 4 where registers are shortest)
__device__ __forceinline__ void partner_filter_half(double (&zr)[kPts], double (&zi)[kPts], double *__restrict__ buf,
                                                    double *__restrict__ xbuf, int t, const double2 *__restrict__ ab_own,
                                                    const double2 *__restrict__ ab_blk)
{
    constexpr int H = kPts / 2;
    double *__restrict__ wp = buf + reg_base<3>(t);                  // 33 t
    const bool special = t < 8;
    // the coefficients of bin 31 - m: the partner's (general case) or this thread's own upper bin (special case)
    // -- ONE load sequence serves both cases
    const double2 *__restrict__ ab_prt = ab_blk + (special ? t : 263 - t);
    double2 ca[BP], cb[BP];
    auto request = [&](int m0) {
        // The OFFSET passes through an empty asm statement: the loads have no other dependency and would otherwise
        // all be hoisted to one place.  The pointer itself must keep its provenance: a laundered pointer is loaded
        // from with FLAT instructions, and one pending flat load turns every later wait into s_waitcnt vmcnt(0)
        // lgkmcnt(0) (flat loads may return out of order).
        int o = m0 * kT;
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            ca[i] = ab_own[o + i * kT];
            cb[i] = ab_prt[(kPts - 1) * kT - o - i * kT];
        }
    };
    request(0);                               // arrives behind the publication and its barrier
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < H; ++j) {
        wp[H + j] = zr[reg_slot<16>(H + j)];
        wp[j] = zi[reg_slot<16>(H + j)];
    }
    if (special) {
#pragma unroll
        for (int j = 0; j < H; ++j) {
            xbuf[t * H + j] = zr[reg_slot<16>(j)];
            xbuf[(8 + t) * H + j] = zi[reg_slot<16>(j)];
        }
    }
    __syncthreads();
    if (!special) {
        double *__restrict__ pp = buf + 33 * (263 - t) + 31;             // partner slot 31 - m: re at pp[-m], im at pp[-16 - m]
#pragma unroll
        for (int m0 = 0; m0 < H; m0 += BP) {
            if (m0 > 0) request(m0);
#pragma unroll
            for (int i0 = 0; i0 < BP; i0 += 4) {
                double pre[4], pim[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    pre[i] = pp[-(m0 + i0 + i)];
                    pim[i] = pp[-H - (m0 + i0 + i)];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + i0 + i, sl = reg_slot<16>(m);
                    const double a = ca[i0 + i].x, b = ca[i0 + i].y, ap = cb[i0 + i].x, bp = cb[i0 + i].y;
                    const double nr = a * zr[sl] + b * pim[i];
                    const double ni = a * zi[sl] + b * pre[i];
                    const double qr = ap * pre[i] + bp * zi[sl];         // Z'[N-k] = alpha' Z[N-k] + i beta' conj(Z[k])
                    const double qi = ap * pim[i] + bp * zr[sl];
                    zr[sl] = nr;
                    zi[sl] = ni;
                    pp[-m] = qr;
                    pp[-H - m] = qi;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // the eight threads whose partner bins sit in the same half: every own bin from published originals
        // (lower bin m with ca, upper bin 31 - m with cb: the same two batches of loads as the other threads)
        const int tl = t == 0 ? 0 : 8 - t;                               // lower slots' partner thread
        const double *__restrict__ up = buf + 33 * (7 - t) + 47;         // upper: re at up[-m], im at up[-m - 16]
#pragma unroll
        for (int m0 = 0; m0 < H; m0 += BP) {
            if (m0 > 0) request(m0);
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const int m = m0 + i, sl = reg_slot<16>(m);
                const int ms = t == 0 ? (m == 0 ? 0 : H - m) : H - 1 - m;
                const double pre_ = xbuf[tl * H + ms], pim_ = xbuf[(8 + tl) * H + ms];
                const double nr = ca[i].x * zr[sl] + ca[i].y * pim_;
                const double ni = ca[i].x * zi[sl] + ca[i].y * pre_;
                zr[sl] = nr;
                zi[sl] = ni;
                const int mu = kPts - 1 - m, su = reg_slot<16>(mu);       // the upper bin 31 - m
                const double ure = up[-mu], uim = up[-mu - H];
                // (its own upper originals are read back from the slots it published, so that the upper registers
                //  are dead from the publication on for every lane of the wave: liveness is per register)
                zr[su] = cb[i].x * wp[mu] + cb[i].y * uim;
                zi[su] = cb[i].x * wp[mu - H] + cb[i].y * ure;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    if (!special) {
#pragma unroll
        for (int j = 0; j < H; ++j) {
            zr[reg_slot<16>(H + j)] = wp[H + j];
            zi[reg_slot<16>(H + j)] = wp[j];
        }
    }
    __syncthreads();
}

// ---- the transform's phases around the pairing ---------------------------------------------------
// forward: radix 32 and radix 16 with their twiddles and exchanges (the last radix-16 butterflies follow in the kernel)
__device__ __forceinline__ void forward_passes(double (&zr)[kPts], double (&zi)[kPts], double *buf, int t,
                                               const double2 *Wtw)
{
    const double2 w_a = Wtw[t];                      // n = N:   exp(-2 pi i t / N)
    const double2 w_b = Wtw[kPts * (t & 15)];        // n = 256: exp(-2 pi i (t & 15) / 256)
    reg_fwd<kPts, 0>(zr, zi, w_a);
    reg_exchange<1, 2, kPts>(zr, buf, t);
    reg_exchange<1, 2, kPts>(zi, buf, t);
    reg_fwd<16, 0>(zr, zi, w_b);
    reg_fwd<16, 16>(zr, zi, w_b);
    reg_exchange<2, 3, 16>(zr, buf, t);
    reg_exchange<2, 3, 16>(zi, buf, t);
}

// the middle and the last inverse pass; result slot m ends at index brev<32>(m)
__device__ __forceinline__ void inverse_tail(double (&zr)[kPts], double (&zi)[kPts], double *buf, int t, double2 w_bi,
                                             double2 w_ai)
{
    reg_inv<16, 0>(zr, zi, w_bi);
    reg_inv<16, 16>(zr, zi, w_bi);
    reg_exchange<2, 1, 16>(zr, buf, t);
    reg_exchange<2, 1, 16>(zi, buf, t);
    reg_inv<kPts, 0>(zr, zi, w_ai);
}

// MODE 0: time order; 1: plain lists; 2: run-coded lists; 3: inverse lists.
// BUF: the TOD buffers are addressed through buffer descriptors of `nbytes` bytes -- an entry
// without a sample carries the address 0xFFFFFFFF, whose byte offset lies outside the descriptor:
// such a load returns 0 and such a store is dropped by the hardware, so the gathers need no
// address clamp and no zeroing select and the result stores no branch (48 exec-masked blocks in
// the flat form).  Flat addressing is kept for buffers of 4 GB and more.
// Phases: load the window, forward passes, pairing, first inverse pass and exchange, request the result lists,
// inverse tail, store.  What is still written out in place changed an instruction stream or spilled as a helper.
template <int MODE, bool BUF>
__global__ __launch_bounds__(kT, 2) void k_os_real(
    const WinDesc *__restrict__ wins, int nwin, const double2 *__restrict__ Wtw, const double2 *Wtw_inv,
    const double2 *__restrict__ AB, const uint32_t *__restrict__ lst_k, const uint16_t *__restrict__ lst_q,
    const ListHdr *__restrict__ hdrs, const uint32_t *__restrict__ tabs, int rmax, const double *__restrict__ v,
    double *__restrict__ out, uint32_t nbytes, const IListHdr *__restrict__ ihdrs,
    const uint32_t *__restrict__ iflags OS_STAMP_PARAM)
{
    constexpr int N = os::N, H = kPts / 2;
    constexpr int ER = os::RLEN / kT;                // result entries (slots) per thread and round
    __amdgpu_buffer_rsrc_t v_rs, o_rs;
    if constexpr (BUF) {
        v_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(v), 0, (int)nbytes, 0x00020000);
        o_rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)nbytes, 0x00020000);
    }
    // sample at tile-order address k (0xFFFFFFFF: none)
    auto gather = [&](uint32_t k) -> double {
        if constexpr (BUF) {
            const v2u_t r = __builtin_amdgcn_raw_buffer_load_b64(v_rs, k * 8u, 0, 0);
            return __builtin_bit_cast(double, r);
        } else {
            return v[k != kInvalidSample ? k : 0u];
        }
    };
    auto keep = [&](uint32_t k, double x) -> double {        // value staged for entry k
        if constexpr (BUF) return x;
        return k != kInvalidSample ? x : 0.0;
    };
    extern __shared__ double buf[];
    uint32_t *__restrict__ tab_lds = reinterpret_cast<uint32_t *>(buf + os::LDSD);   // RC: 2 x rmax words
    const int t = threadIdx.x;
    const int per_xcd = (nwin + 7) / 8;
    const int win = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (win >= nwin) return;
    const WinDesc wd = wins[win];
    const int64_t w0 = wd.start - kHalo;            // time of window position 0
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform: an SGPR, the header words become scalar loads
    OS_STAMP(0);

    auto list_args = [&](int l) {
        ListArgs la;
        const int64_t e0 = (int64_t)win * os::PER + os::list_off(l);
        // (no null tests: the launcher hands every MODE the arrays it reads -- a test made here is a 64-bit
        //  mask the compiler keeps from the first use of a list to the last, across the whole transform)
        la.k = nullptr, la.q = nullptr, la.hdr = nullptr, la.tab = nullptr;
        if constexpr (MODE == 1) la.k = lst_k + e0;
        if constexpr (MODE == 1 || MODE == 2) la.q = lst_q + e0;
        if constexpr (MODE == 2) {
            la.hdr = hdrs + ((int64_t)win * os::NLIST + l);
            la.tab = tabs + ((int64_t)win * os::NLIST + l) * rmax;
        }
        return la;
    };

    double zr[kPts], zi[kPts];
    // ---- load the window, one half (N positions) at a time through the LDS buffer --------------
    // (one branch per list format and the LDS -> register read of a half written out three times: as lambdas or
    //  helpers they move the register allocation of this 251-256 VGPR kernel into scratch)
    if constexpr (MODE == 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double vv[kPts];
#pragma unroll
            for (int u = 0; u < kPts; ++u) {
                const int64_t ts = w0 + (int64_t)h * N + t + u * kT;
                vv[u] = (ts >= wd.lo && ts < wd.hi) ? v[ts] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kPts; ++u) buf[t + u * kT] = vv[u];
            __syncthreads();
            const double2 *__restrict__ sp = reinterpret_cast<const double2 *>(buf) + t;
#pragma unroll
            for (int m = 0; m < H; ++m) {
                const double2 p = sp[256 * m];
                zr[h * H + m] = p.x;
                zi[h * H + m] = p.y;
            }
            __syncthreads();
        }
    } else if constexpr (MODE == 3) {
        // inverse lists: two rounds of N slots of the window's address-sorted order.  Header, run
        // table, flag words and this thread's slot numbers are requested together (the table is
        // read up to its allocated length: no dependency on the run count).
        const IListHdr *__restrict__ h0 = ihdrs + (int64_t)win * 2;
        const uint32_t *__restrict__ pl = reinterpret_cast<const uint32_t *>(lst_q + (int64_t)win * os::PER);
        uint32_t fw[2], pp[kPts];
        tab_dma(tabs + ((int64_t)win * 2) * rmax, tab_lds, rmax, wave, t);
        fw[0] = iflags[((int64_t)win * 2) * 512 + t];
        fw[1] = iflags[((int64_t)win * 2) * 512 + 256 + t];
        const uint32_t nv = h0->nvalid;
        const int wb0 = h0->wbase[wave], wb1 = h0->wbase[4 + wave];
#pragma unroll
        for (int m = 0; m < kPts; ++m) pp[m] = pl[t + kT * m];
        __syncthreads();
        // both rounds' gathers are issued before anything is staged: 2 x 32 loads in flight per thread
        // while the transform's registers are not live yet
        double va[kPts], vb[kPts];
        {
            uint32_t kk[kPts];
            idecode<kPts>(fw[0], tab_lds, wb0, nv, 0u, t, kk);
#pragma unroll
            for (int u = 0; u < kPts; ++u) va[u] = keep(kk[u], gather(kk[u]));
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            uint32_t kk[kPts];
            idecode<kPts>(fw[1], tab_lds, wb1, nv, (uint32_t)N, t, kk);
#pragma unroll
            for (int u = 0; u < kPts; ++u) vb[u] = keep(kk[u], gather(kk[u]));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int u = 0; u < kPts; ++u) buf[slot_of<kPts>(t, u)] = j ? vb[u] : va[u];
            if (j == 1) {
                // the slot numbers again (L2): 32 registers not held across the first round's picks
                int tj = t;
                asm volatile("" : "+v"(tj));
#pragma unroll
                for (int m = 0; m < kPts; ++m) pp[m] = pl[tj + kT * m];
            }
            __syncthreads();
            // a point outside this round reads word 0 (one address for all such lanes: no bank conflict)
#pragma unroll
            for (int m = 0; m < kPts; ++m) {
                const uint32_t lo = (pp[m] & 0xFFFFu) - (uint32_t)(j * N), hi = (pp[m] >> 16) - (uint32_t)(j * N);
                const bool inl = lo < (uint32_t)N, inh = hi < (uint32_t)N;
                const double x = buf[inl ? lo : 0u], y = buf[inh ? hi : 0u];
                if (j == 0) {
                    zr[m] = inl ? x : 0.0;
                    zi[m] = inh ? y : 0.0;
                } else {
                    zr[m] = inl ? x : zr[m];
                    zi[m] = inh ? y : zi[m];
                }
            }
            __syncthreads();
        }
    } else {                                             // plain and run-coded lists: one list per window half
        const ListArgs l0 = list_args(0), l1 = list_args(1);
        uint32_t qa[kPts / 2], qb[kPts / 2], ka[kPts], kb[kPts];
        uint32_t nva = 0, nvb = 0;
        int wba = -1, wbb = -1;
        if constexpr (MODE == 2) {
            nva = l0.hdr->nvalid;
            nvb = l1.hdr->nvalid;
            wba = l0.hdr->wbase[wave];
            wbb = l1.hdr->wbase[wave];
            tab_dma(l0.tab, tab_lds, rmax, wave, t);
            tab_dma(l1.tab, tab_lds + rmax, rmax, wave, t);
        }
        q_request<kPts>(l0.q, t, qa);
        if constexpr (MODE == 1) {
#pragma unroll
            for (int u = 0; u < kPts; ++u) ka[u] = ld_list(l0.k + slot_of<kPts>(t, u));
        }
        q_request<kPts>(l1.q, t, qb);
        if constexpr (MODE == 1) {
#pragma unroll
            for (int u = 0; u < kPts; ++u) kb[u] = ld_list(l1.k + slot_of<kPts>(t, u));
        }
        if constexpr (MODE == 2) {
            __syncthreads();
            OS_STAMP(6);                             // (diagnostic build: lists and run tables have arrived)
            rc_decode<kPts>(qa, tab_lds, wba, nva, t, ka);
        }
        __builtin_amdgcn_sched_barrier(0);
        // Both halves' gathers are in flight together (2 x 32 loads per thread: the transform's registers
        // are not live yet), half a is staged while half b is still on its way: two dependent round
        // trips (lists, gathers) instead of three.  Five same-box alternations of bench.py: step 1.478
        // against 1.507 ms (-1.9 %, every pair); one noisy pair had hidden it earlier in the round.
        double va[kPts], vv[kPts];
        if constexpr (MODE == 2) rc_decode<kPts>(qb, tab_lds + rmax, wbb, nvb, t, kb);
#pragma unroll
        for (int u = 0; u < kPts; ++u) va[u] = gather(ka[u]);
#pragma unroll
        for (int u = 0; u < kPts; ++u) vv[u] = gather(kb[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kPts; ++u) buf[q_word(qa, u) & 0x7FFFu] = keep(ka[u], va[u]);
        OS_STAMP(7);                                 // (diagnostic build: the first half's gathers have arrived)
        __syncthreads();
        const double2 *__restrict__ sp = reinterpret_cast<const double2 *>(buf) + t;
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const double2 p = sp[256 * m];
            zr[m] = p.x;
            zi[m] = p.y;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kPts; ++u) buf[q_word(qb, u) & 0x7FFFu] = keep(kb[u], vv[u]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const double2 p = sp[256 * m];
            zr[H + m] = p.x;
            zi[H + m] = p.y;
        }
        __syncthreads();
    }

    OS_STAMP(1);
    OS_XF(forward_passes(zr, zi, buf, t, Wtw));
    // (the last butterflies stay here, behind this address: inside forward_passes they cost three instances scratch)
    const double2 *ab = AB + (int64_t)wd.blk * N + t;
    OS_XF(dft_sub<16, 0>(zr, zi));
    OS_XF(dft_sub<16, 16>(zr, zi));
    OS_STAMP(2);
    // ---- pairing with bin N-k and the spectrum product ----
    // (plain lists with flat addressing -- more than 2048 pixel tiles AND buffers of 4 GB and more -- hold 32
    //  address words beside the transform: batches of four bin pairs there, or three VGPRs spill)
    OS_XF(partner_filter_half<(MODE == 1 && !BUF) ? 4 : 8>(zr, zi, buf, reinterpret_cast<double *>(tab_lds + 2 * rmax),
                                                           t, ab, AB + (int64_t)wd.blk * N));
    (void)ab;
    OS_STAMP(3);
    // ---- inverse: radix 16 (decimation in time on the bit-reversed data), radix 16, radix 32 ----
    OS_XF(dit_sub<16, 0>(zi, zr));
    OS_XF(dit_sub<16, 16>(zi, zr));
    // the inverse passes read their twiddles again (through a second pointer to the same table,
    // so that nothing of the forward passes stays live across the pairing step)
    const double2 w_bi = Wtw_inv[kPts * (t & 15)], w_ai = Wtw_inv[t];
    OS_XF(reg_exchange<3, 2, 0>(zr, buf, t));
    OS_XF(reg_exchange<3, 2, 0>(zi, buf, t));
    // The result lists of round 0 are requested HERE, in front of the middle inverse pass: a run table
    // travels by LDS-DMA, and while one is in flight every workgroup barrier waits for it (s_waitcnt
    // vmcnt(0) in front of s_barrier) -- so the request is issued right behind a barrier, with the
    // longest barrier-free stretch of arithmetic (the two radix-16 blocks) to hide behind; the 16-bit
    // words are in registers by the end of the last pass.  Both twiddles are made to arrive first
    // (requested two exchanges ago): a wait for a load OLDER than the table requests would be emitted as
    // s_waitcnt vmcnt(0) too -- the compiler does not count LDS-DMA requests behind wave-uniform
    // branches -- and would wait for the lists as well.
    asm volatile("" : : "v"(w_bi.x), "v"(w_bi.y), "v"(w_ai.x), "v"(w_ai.y));
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MODE == 3) {
        // ---- inverse result list: rounds of RLEN slots of the result window's address-sorted order ----
        constexpr int NP = kPts - 8;                     // points with results
        // (the list number passes through an empty asm statement -- an offset, not a pointer, see
        // partner_filter_half: the requests below have no other dependency and would be hoisted to the top)
        int l1 = 1;
        asm volatile("" : "+s"(l1));
        const IListHdr *h1 = ihdrs + (int64_t)win * 2 + l1;
        const uint32_t *tg = tabs + ((int64_t)win * 2 + l1) * rmax;
        const uint32_t *fg = iflags + ((int64_t)win * 2 + l1) * 512 + t;
        const uint32_t nv1 = h1->nvalid;
        uint32_t fr[os::RR], rp[NP];
        const uint32_t *rl = reinterpret_cast<const uint32_t *>(lst_q + (int64_t)win * os::PER + 2 * N);
        tab_dma(tg, tab_lds + rmax, rmax, wave, t);            // published by the barriers of the next exchange
#pragma unroll
        for (int j = 0; j < os::RR; ++j) fr[j] = fg[256 * j];
        // the slot numbers of this thread's results, in registers by the end of the last pass
        int t0 = t;
        asm volatile("" : "+v"(t0));
#pragma unroll
        for (int m = 0; m < NP; ++m) rp[m] = rl[t0 + kT * m];
        __builtin_amdgcn_sched_barrier(0);
        OS_XF(inverse_tail(zr, zi, buf, t, w_bi, w_ai));
        OS_STAMP(4);
#pragma unroll
        for (int j = 0; j < os::RR; ++j) {
            if (j > 0) {
                __syncthreads();                         // the previous round's reads are done
                int tj = t;                              // (the slot numbers again, from L2)
                asm volatile("" : "+v"(tj));
#pragma unroll
                for (int m = 0; m < NP; ++m) rp[m] = rl[tj + kT * m];
            }
            // y[2 (t + 256 m)] = zr, y[.. + 1] = zi for m in [4, 28): each value to its slot of this
            // round, the others to a spare word behind the stage (no branch)
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const uint32_t lo = (rp[m] & 0xFFFFu) - (uint32_t)(j * os::RLEN), hi = (rp[m] >> 16) - (uint32_t)(j * os::RLEN);
                buf[lo < (uint32_t)os::RLEN ? lo : (uint32_t)N] = zr[brev<kPts>(m + 4)];
                buf[hi < (uint32_t)os::RLEN ? hi : (uint32_t)N + 1u] = zi[brev<kPts>(m + 4)];
            }
            __syncthreads();
            uint32_t ks[ER];
            idecode<ER>(fr[j], tab_lds + rmax, h1->wbase[4 * j + wave], nv1, (uint32_t)(j * os::RLEN), t, ks);
            double rv[ER];
#pragma unroll
            for (int u = 0; u < ER; ++u) rv[u] = buf[slot_of<ER>(t, u)];
            // (the store loop is written out in both branches: as one helper it changes <3, true>'s stream)
#pragma unroll
            for (int u = 0; u < ER; ++u) {
                if constexpr (BUF) {
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_t, rv[u]), o_rs, ks[u] * 8u, 0, 0);
                } else {
                    if (ks[u] != kInvalidSample) out[ks[u]] = rv[u];
                }
            }
        }
    } else {
        uint32_t qs[ER / 2], ks[ER];
        uint32_t nvs = 0;
        int wbs = -1;
        auto request_results = [&](int j, auto &qq, uint32_t &nv, int &wb, uint32_t *tdst) {
            if constexpr (MODE != 0) {
                // (the list number passes through an empty asm statement: an offset, not a pointer, see
                // partner_filter_half; the list's addresses stay wave-uniform and its header words scalar loads)
                int lj = 2 + j;
                asm volatile("" : "+s"(lj));
                const ListArgs ls = list_args(lj);
                if constexpr (MODE == 2) {
                    nv = ls.hdr->nvalid;
                    wb = ls.hdr->wbase[wave];
                    tab_dma(ls.tab, tdst, rmax, wave, t);
                }
                q_request<ER>(ls.q, t, qq);      // (plain lists: the addresses are fetched behind the last pass, see below)
            }
        };
        // EARLY: the second result round's lists are requested behind the first round's staging barrier, so
        // that they travel while the first round's results are stored (the barrier in front of the second
        // round waits for the stores and the lists together: one round trip less per window).  Five
        // same-box alternations of bench.py: step 1.407 against 1.446 ms (-2.7 %).  Not for plain lists
        // with flat addressing (the 12 list words more spill 22 VGPRs there).
        constexpr bool EARLY = MODE == 2 || (MODE == 1 && BUF);
        uint32_t qs1[ER / 2];
        uint32_t nv1 = 0;
        int wb1 = -1;
        request_results(0, qs, nvs, wbs, tab_lds);   // (its run table: published by the barriers of the next exchange)
        __builtin_amdgcn_sched_barrier(0);
        OS_XF(inverse_tail(zr, zi, buf, t, w_bi, w_ai));
        // ---- store: y[2 (t + 256 m)] = zr, y[.. + 1] = zi for m in [4, 28), RSLOTS slots a round --
        OS_STAMP(4);
#pragma unroll
        for (int j = 0; j < os::RR; ++j) {
            const uint32_t *tabj = tab_lds + (EARLY && j > 0 ? rmax : 0);
            if (j > 0) {
                __syncthreads();                         // the previous round's reads are done (EARLY: and round j's table is in)
                if constexpr (EARLY) {
#pragma unroll
                    for (int i = 0; i < ER / 2; ++i) qs[i] = qs1[i];
                    nvs = nv1;
                    wbs = wb1;
                } else {
                    request_results(j, qs, nvs, wbs, tab_lds);
                    if constexpr (MODE == 2) __syncthreads();
                }
            }
            if constexpr (MODE == 2) rc_decode<ER>(qs, tabj, wbs, nvs, t, ks);
            double2 *__restrict__ sp = reinterpret_cast<double2 *>(buf) + t;
#pragma unroll
            for (int mm = 0; mm < os::RSLOTS; ++mm) {
                const int m = 4 + j * os::RSLOTS + mm;
                sp[256 * mm] = make_double2(zr[brev<kPts>(m)], zi[brev<kPts>(m)]);
            }
            if constexpr (MODE == 1) {
                // plain lists: 24 address words held across the radix-32 pass do not fit beside its 128 data
                // registers (20 spilled VGPRs in the flat form); they are requested here instead
                const ListArgs ls = list_args(2 + j);
#pragma unroll
                for (int u = 0; u < ER; ++u) ks[u] = ld_list(ls.k + slot_of<ER>(t, u));
            }
            __syncthreads();
            if constexpr (EARLY)
                if (j + 1 < os::RR) request_results(j + 1, qs1, nv1, wb1, tab_lds + rmax);
            if constexpr (MODE == 0) {
#pragma unroll
                for (int u = 0; u < ER; ++u) {
                    const int e = t + u * kT;
                    const int64_t o = (int64_t)j * os::RLEN + e;
                    if (o < wd.len) out[wd.start + o] = buf[e];
                }
            } else {
                double rv[ER];
#pragma unroll
                for (int u = 0; u < ER; ++u) rv[u] = buf[q_word(qs, u) & 0x7FFFu];
#pragma unroll
                for (int u = 0; u < ER; ++u) {
                    if constexpr (BUF) {
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_t, rv[u]), o_rs, ks[u] * 8u, 0, 0);
                    } else {
                        if (ks[u] != kInvalidSample) out[ks[u]] = rv[u];
                    }
                }
            }
        }
    }
    OS_STAMP(5);
}

// W[t] = exp(-2 pi i t / N)
__global__ void k_real_twiddles(int N, double2 *__restrict__ W)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) W[t] = make_double2(cospi(2.0 * t / N), -sinpi(2.0 * t / N));
}

// ct[m] = cos(pi m / N), m = 0..N
__global__ void k_real_cos_table(int N, double *__restrict__ ct)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m <= N) ct[m] = cospi((double)m / (double)N);
}

// H[b][k] = a0 + 2 sum_{j>=1} a_j cos(2 pi j k / (2N)),  k = 0..N  (real, even: symmetric band).
// The cosines come from the table ct staged in LDS (cos(pi m / N) for m = j k mod 2N, folded to
// m <= N by the cosine's symmetry) instead of one cospi per term: the sum over j is the same sum in
// the same order (j = lambda - 1 down to 1).  One workgroup: kSpecK bins of one block.
constexpr int kSpecK = 1024;                             // bins per workgroup (4 per thread)
__global__ __launch_bounds__(256) void k_real_spectrum(int nb, int64_t lambda, int N,
                                                        const double *__restrict__ bands,
                                                        const double *__restrict__ ct_g,
                                                        double *__restrict__ Hs)
{
    extern __shared__ double ct[];                       // N + 1 cosines
    constexpr int PER = kSpecK / 256;
    const int chunks = (N + 1 + kSpecK - 1) / kSpecK;
    const int b = blockIdx.x / chunks, c = blockIdx.x % chunks;
    for (int m = threadIdx.x; m <= N; m += 256) ct[m] = ct_g[m];
    __syncthreads();
    const double *band = bands + (int64_t)b * lambda;
    const int mask = 2 * N - 1;                          // N is a power of two
    int k[PER], m[PER];
    double acc[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        k[u] = c * kSpecK + u * 256 + (int)threadIdx.x;
        m[u] = (int)(((lambda - 1) * (int64_t)k[u]) & mask);
        acc[u] = 0.0;
    }
    for (int64_t j = lambda - 1; j >= 1; --j) {
        const double a = band[j];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int f = m[u] <= N ? m[u] : 2 * N - m[u];
            acc[u] += a * ct[f];
            m[u] = (m[u] - k[u]) & mask;
        }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u)
        if (k[u] <= N) Hs[(int64_t)b * (N + 1) + k[u]] = band[0] + 2.0 * acc[u];
}

// AB[b][a] = (alpha_k, beta_k), a = d1 256 + d2 16 + d3 the P3 position holding k = d1 + kPts d2 + 16 kPts d3
__global__ __launch_bounds__(256) void k_real_alpha_beta(int nb, const double *__restrict__ Hs, double2 *__restrict__ AB)
{
    constexpr int N = os::N;
    const int64_t total = (int64_t)nb * N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t b = e / N;
        const int a = (int)(e - b * N);
        const int d1 = a / 256, d2 = (a / 16) % 16, d3 = a % 16;
        const int k = d1 + kPts * d2 + 16 * kPts * d3;
        const double *h = Hs + b * (N + 1);
        const double hk = h[k], hp = h[N - k];          // H[k + N] = H[N - k]
        const double S = 0.5 * (hk + hp), Dd = 0.5 * (hk - hp);
        const double th = (double)k / (double)N;
        // stored [m][t] (a = kPts t + m): the 256 threads read bin m of all of them in one contiguous
        // 4 KB piece -- [t][m] order made every lane of a load touch another cache line
        const int t = a / kPts, m = a % kPts;
        AB[b * N + (int64_t)m * kT + t] = make_double2((S - Dd * sinpi(th)) / (double)N,
                                                        (Dd * cospi(th)) / (double)N);
    }
}

}  // namespace

namespace cm2 {

constexpr size_t kListCache = 3;         // tile plans whose lists one operator keeps (most recent first)

struct FusedOS {
    int64_t nwin = 0;
    WinDesc *d_wins = nullptr;
    double2 *d_AB = nullptr;
    double2 *d_W = nullptr;
    // switches, read ONCE when the operator is created (never on the application path):
    int want_lists = 0;                  // CM2_OS_LISTS = auto (0) | plain (1) | rc (2) | inv (3)
    bool build_sort = false;             // CM2_OS_LIST_BUILD = sort: lists from a segmented sort
    bool flat = false;                   // CM2_OS_FLAT: flat addressing although the buffers are < 4 GB
    int64_t sort_chunk_windows = 0;      // CM2_OS_LIST_CHUNK_PAIRS (test hook: sort in several chunks)
    std::mutex mu;                       // guards `cache`; list builds run under it
    std::vector<std::shared_ptr<OsLists>> cache;
};

void fused_os_destroy(FusedOS *f)
{
    if (!f) return;
    f->cache.clear();
    void *ptrs[] = {f->d_wins, f->d_AB, f->d_W};
    for (void *q : ptrs)
        if (q) (void)cm2::dev_free(q);
    delete f;
}

bool fused_os_supported(int64_t lambda) { return lambda >= 1 && lambda - 1 <= kHalo; }

int64_t fused_os_length(const FusedOS *f) { return f ? os::N : 0; }

int fused_os_create(FusedOS **out, const double *d_bands, int64_t lambda, const std::vector<int64_t> &off,
                    hipStream_t stream)
{
    CM2_CHECK(out != nullptr, "fused_os_create: out is NULL");
    *out = nullptr;
    CM2_CHECK(fused_os_supported(lambda), "fused overlap-save supports lambda <= 2049, got %lld",
              (long long)lambda);
    FusedOS *f = new FusedOS();
    struct Guard { FusedOS *f; ~Guard() { if (f) fused_os_destroy(f); } } guard{f};
    if (const char *e = getenv("CM2_OS_LISTS")) {
        if (!strcmp(e, "plain")) f->want_lists = 1;
        else if (!strcmp(e, "rc")) f->want_lists = 2;
        else if (!strcmp(e, "inv")) f->want_lists = 3;
    }
    if (const char *e = getenv("CM2_OS_LIST_BUILD")) f->build_sort = strcmp(e, "sort") == 0;
    f->flat = getenv("CM2_OS_FLAT") != nullptr;
    if (const char *e = getenv("CM2_OS_LIST_CHUNK_PAIRS")) f->sort_chunk_windows = atoll(e);
    const int64_t nb = (int64_t)off.size() - 1;
    const std::vector<WinDesc> wins = os::windows(off);
    f->nwin = (int64_t)wins.size();
    CM2_CHECK(f->nwin * 4 < ((int64_t)1 << 31), "fused overlap-save: too many windows (%lld)", (long long)f->nwin);
    CM2_HIP(cm2::dev_malloc(&f->d_wins, sizeof(WinDesc) * (wins.size() ? wins.size() : 1)));
    if (!wins.empty())
        CM2_HIP(cm2::upload(f->d_wins, wins.data(), sizeof(WinDesc) * wins.size(), nullptr));
    CM2_HIP(cm2::dev_malloc(&f->d_AB, sizeof(double2) * (nb > 0 ? nb : 1) * os::N));
    if (nb > 0) {
        DevTemp<double> Hs;
        CM2_HIP(Hs.alloc(nb * (os::N + 1)));
        DevTemp<double> ct;
        CM2_HIP(ct.alloc(os::N + 1));
        k_real_cos_table<<<(os::N + 256) / 256, 256, 0, stream>>>(os::N, ct);
        CM2_LAUNCH_OK();
        const size_t ct_lds = sizeof(double) * (os::N + 1);
        static size_t ct_granted[64] = {0};
        CM2_HIP(ensure_dynamic_lds((const void *)k_real_spectrum, ct_lds, ct_granted));
        const int chunks = (os::N + 1 + kSpecK - 1) / kSpecK;
        k_real_spectrum<<<(int)nb * chunks, 256, ct_lds, stream>>>((int)nb, lambda, os::N, d_bands, ct, Hs);
        CM2_LAUNCH_OK();
        k_real_alpha_beta<<<grid_for(nb * os::N), kBlock, 0, stream>>>((int)nb, Hs, f->d_AB);
        CM2_LAUNCH_OK();
        CM2_HIP(hipStreamSynchronize(stream));
    }
    CM2_HIP(cm2::dev_malloc(&f->d_W, sizeof(double2) * os::N));
    k_real_twiddles<<<(os::N + 255) / 256, 256, 0, stream>>>(os::N, f->d_W);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(stream));
    guard.f = nullptr;
    *out = f;
    return 0;
}

template <int MODE, bool BUF>
static int os_launch_t(const FusedOS *f, const OsLists *ls, const double *d_v, double *d_out, uint32_t nbytes,
                       hipStream_t stream)
{
    const int rmax = ls ? ls->rmax : 0;
    const size_t lds = os::kernel_lds_bytes(MODE, rmax);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds((const void *)k_os_real<MODE, BUF>, lds, granted));
    if (f->nwin == 0) return 0;
    const int grid = (int)(((f->nwin + 7) / 8) * 8);       // whole rounds over the 8 XCDs
    k_os_real<MODE, BUF><<<grid, kT, lds, stream>>>(
        f->d_wins, (int)f->nwin, f->d_W, f->d_W, f->d_AB, ls ? ls->d_lst_k : nullptr, ls ? ls->d_lst_q : nullptr,
        ls ? ls->d_hdrs : nullptr, ls ? ls->d_tabs : nullptr, rmax, d_v, d_out, nbytes, ls ? ls->d_ihdrs : nullptr,
        ls ? ls->d_iflags : nullptr OS_STAMP_ARG);
    CM2_LAUNCH_OK();
    return 0;
}

// The kernel instance for a list format, a run-table size and a buffer size.  Buffers below 4 GB are
// addressed through buffer descriptors (BUF), larger ones (or CM2_OS_FLAT) with flat addresses.
static int os_launch(const FusedOS *f, const OsLists *ls, int64_t nvalid, const double *d_v, double *d_out,
                     hipStream_t stream)
{
    if (f->nwin == 0) return 0;
    const uint32_t nbytes = os::descriptor_bytes(nvalid, f->flat);          // 0: flat addressing
    static constexpr decltype(&os_launch_t<1, false>) launch[3][2] = {{os_launch_t<1, false>, os_launch_t<1, true>},
                                                                      {os_launch_t<2, false>, os_launch_t<2, true>},
                                                                      {os_launch_t<3, false>, os_launch_t<3, true>}};
    if (ls->mode == 1 || ((ls->mode == 2 || ls->mode == 3) && os::table_fits(ls->rmax)))
        return launch[ls->mode - 1][nbytes != 0u](f, ls, d_v, d_out, nbytes, stream);
    set_error("fused overlap-save: run table of %d words per list does not fit the kernel", ls->rmax);
    return CM2_ERR_ARGUMENT;
}

int fused_os_apply(const FusedOS *f, const double *d_v, double *d_out, hipStream_t stream)
{
    return os_launch_t<0, false>(f, nullptr, d_v, d_out, 0, stream);
}

// The lists of `f` for the tile plan `pv`, from the operator's cache or built now (under the
// operator's mutex: two host threads that meet here build once); format and builder: os::choose_lists.
static int os_lists_for(FusedOS *f, const OsPlanView &pv, hipStream_t stream, std::shared_ptr<OsLists> *out)
{
    std::lock_guard<std::mutex> lock(f->mu);
    for (size_t i = 0; i < f->cache.size(); ++i)
        if (f->cache[i]->plan_id == pv.plan_id) {
            std::shared_ptr<OsLists> hit = f->cache[i];
            f->cache.erase(f->cache.begin() + (long)i);
            f->cache.insert(f->cache.begin(), hit);
            *out = hit;
            return 0;
        }
    const os::ListChoice c = os::choose_lists(f->want_lists, f->build_sort, pv.d_tile_off != nullptr, pv.ntiles);
    std::shared_ptr<OsLists> ls = std::make_shared<OsLists>();
    ls->plan_id = pv.plan_id;
    CM2_CHECK(f->nwin * os::NLIST < ((int64_t)1 << 31), "fused overlap-save: too many lists (%lld)",
              (long long)(f->nwin * os::NLIST));
    if (f->nwin == 0) {
        ls->mode = 1;
    } else if (int rc = os_build_lists(c, f->d_wins, f->nwin, ls.get(), pv, f->sort_chunk_windows, stream)) {
        return rc;                                           // (ls frees what it holds)
    }
    f->cache.insert(f->cache.begin(), ls);
    while (f->cache.size() > kListCache) f->cache.pop_back();
    *out = ls;
    return 0;
}

int fused_os_prepare_indexed(FusedOS *f, const OsPlanView &pv, hipStream_t stream)
{
    std::shared_ptr<OsLists> ls;
    return os_lists_for(f, pv, stream, &ls);
}

int fused_os_apply_indexed(FusedOS *f, const OsPlanView &pv, const double *d_v, double *d_out, hipStream_t stream)
{
    std::shared_ptr<OsLists> ls;
    if (int rc = os_lists_for(f, pv, stream, &ls)) return rc;
    return os_launch(f, ls.get(), pv.nvalid, d_v, d_out, stream);
}

// (see cm2_overlap_save.h) the bytes: lists + gathered window + results
double fused_os_tile_info(const FusedOS *f_, int *kernel)
{
    FusedOS *f = const_cast<FusedOS *>(f_);
    std::shared_ptr<OsLists> ls;
    if (f) {
        std::lock_guard<std::mutex> lock(f->mu);
        if (!f->cache.empty()) ls = f->cache.front();
    }
    if (kernel) {
        kernel[0] = f ? os::kPts : 0;
        kernel[1] = ls ? ls->mode : 0;
    }
    if (!f) return 0.0;
    const double hop = (double)os::HOP, win = (double)os::W;
    const double lists = ls && ls->bytes_per_window > 0 ? ls->bytes_per_window : 6.0 * (win + hop);
    return (lists + 8.0 * win + 8.0 * hop) / hop;
}

#ifdef CM2_OS_STAMPS
extern "C" int cm2_os_debug_stamps(unsigned long long *d_buf)
{
    g_os_stamps_host = d_buf;
    return 0;
}
#endif

}  // namespace cm2
