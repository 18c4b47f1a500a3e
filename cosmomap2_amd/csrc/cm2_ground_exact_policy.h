// cm2_ground_exact_policy.h -- the device-free arithmetic of the order-independent ground-bin sums
// (cm2_ground_exact.hip; include/cosmomap2.h states the contract).  Plain C++: tests/test_ground_exact_cpu.py
// compiles it with the host compiler and checks it against big-integer arithmetic.
//
// A sample v of a call whose largest counted |v| has the biased exponent field E (e = E - 1023, so every counted
// |v| < 2^(e+1)) is cut into three signed 32-bit limbs of trunc(v 2^(95-e)); the limbs of a bin are added as 64-bit
// integers in any order, and the bin's integer S = L0 2^64 + L1 2^32 + L2 is rounded to fp64 once.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CM2_GS_HD __host__ __device__ __forceinline__
#else
#define CM2_GS_HD inline
#endif

namespace cm2 {
namespace gsum {

constexpr int kLdsBins = 2048;                      // the LDS route holds 3 x 8 x nbins bytes per workgroup
constexpr uint64_t kAbsMask = 0x7FFFFFFFFFFFFFFFull;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kNanBits = 0x7FF8000000000000ull;
constexpr int64_t kMaxSamples = (int64_t)1 << 31;   // below it no limb accumulator reaches 2^63

enum Kind { kZero = 0, kFinite = 1, kPoisoned = 2 };

CM2_GS_HD uint64_t abs_bits(double v)
{
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u & kAbsMask;
}

CM2_GS_HD double from_bits(uint64_t u)
{
    double v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

// what the scale word M (the largest abs_bits of a counted sample) says about the call
CM2_GS_HD Kind kind_of(uint64_t M) { return M == 0 ? kZero : (M >= kInfBits ? kPoisoned : kFinite); }
CM2_GS_HD int exponent_of(uint64_t M) { return (int)(M >> 52) - 1023; }

// l[0] 2^64 + l[1] 2^32 + l[2] = trunc(v 2^(95-e)) for |v| < 2^(e+1): every step is exact in fp64 (scalings by
// powers of two, subtractions of a truncation); a v so small that v 2^(31-e) is subnormal gives three zeros either way
CM2_GS_HD void limbs(double v, int e, int64_t l[3])
{
    const double y0 = ldexp(v, 31 - e);
    const double t0 = trunc(y0);
    const double y1 = ldexp(y0 - t0, 32);
    const double t1 = trunc(y1);
    const double t2 = trunc(ldexp(y1 - t1, 32));
    l[0] = (int64_t)t0;
    l[1] = (int64_t)t1;
    l[2] = (int64_t)t2;
}

// S 2^(e-95), S = L0 2^64 + L1 2^32 + L2 (|S| < 2^127), rounded to nearest, ties to even; S == 0 gives +0.0
CM2_GS_HD double round_sum(int64_t L0, int64_t L1, int64_t L2, int e)
{
    typedef unsigned __int128 u128;
    const u128 s = ((u128)(uint64_t)L0 << 64) + (((u128)(__int128)L1) << 32) + (u128)(__int128)L2;   // mod 2^128
    const bool neg = (uint64_t)(s >> 64) >> 63;
    const u128 mag = neg ? (u128)0 - s : s;
    const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
    if (hi == 0 && lo == 0) return 0.0;
    const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
    int shift = 0;
    uint64_t mant = lo;
    if (top > 52) {
        shift = top - 52;
        mant = (uint64_t)(mag >> shift);
        const u128 rem = mag & (((u128)1 << shift) - 1), half = (u128)1 << (shift - 1);
        if (rem > half || (rem == half && (mant & 1))) ++mant;      // 2^53 at the most: still exact
    }
    const double r = ldexp((double)mant, shift + e - 95);
    return neg ? -r : r;
}

}  // namespace gsum
}  // namespace cm2
