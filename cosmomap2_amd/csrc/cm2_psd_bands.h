// cm2_psd_bands.h -- from a Welch PSD to the first row of a banded-Toeplitz block, the part that the inverse-noise
// band and the colouring band (cm2_noise_model.hip) and the offset prior (cm2_offset_prior.hip) share, written once.
//
// What S is: one row P_k (k = 0 .. L/2, L = nperseg) of the one-sided PSD of a block gives the two-sided spectrum
//   S_k = P_k fs / m_k,   m_k = 1 at the Nyquist bin k = L/2 and 2 elsewhere,   S_0 := S_1
// so bin 0 of the PSD (the mean, which detrending removes) is never read.  Only spectrum_at knows m_k and S_0 := S_1.
//
// Which bin is refused: k_bands_spectrum<G> stores G(S) and reports the first (block, bin) whose S the policy G does
// not accept, the smallest flat index b * nfreq + k of a bin that was read (one integer atomicMin); spectrum<G> runs
// it and words the refusal, before anything but its own output is written.
//
// The cosine sums: tab[m] = cos(2 pi m / N) (k_bands_cos_table; N a power of two), and every sum over it is cos_sum,
// whose order the test references (tests/_noise_model_ref.py, tests/_offset_prior_ref.py) count their error bounds
// from; both units are compiled with -ffp-contract=off, so every product and sum is rounded on its own.
#pragma once
#include "cm2_common.h"

#include <cmath>

namespace cm2 {
namespace psd {

constexpr int64_t kMinL = 256, kMaxL = 65536;           // nperseg

inline bool pow2_in_range(int64_t L) { return L >= kMinL && L <= kMaxL && (L & (L - 1)) == 0; }

// smallest power of two >= v (v >= 1)
inline int64_t pow2_at_least(int64_t v)
{
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline unsigned blocks_for(int64_t count) { return (unsigned)((count + kBlock - 1) / kBlock); }

#define CM2_CHECK_NPERSEG(who, nperseg)                                                                       \
    CM2_CHECK(cm2::psd::pow2_in_range(nperseg), "%s: nperseg=%lld is not a power of two in [%lld, %lld]", who, \
              (long long)(nperseg), (long long)cm2::psd::kMinL, (long long)cm2::psd::kMaxL)

// what every PSD -> band entry point refuses the same way
inline int check_args(const char *who, const double *d_psd, const double *d_bands, int64_t nb, int64_t nperseg,
                      double fsample)
{
    CM2_CHECK(d_psd && d_bands, "%s: NULL argument", who);
    CM2_CHECK(nb >= 1, "%s: nb=%lld < 1", who, (long long)nb);
    CM2_CHECK_NPERSEG(who, nperseg);
    CM2_CHECK(fsample > 0.0 && std::isfinite(fsample), "%s: fsample=%g is not positive", who, fsample);
    return 0;
}

// The policies G of the spectrum step: what is stored for a bin, which S is refused, and the words of the refusal.
//   kInverse   1/S      S must be positive and finite, and not so small that 1/S overflows
//   kSqrt      sqrt(S)  zero is allowed; S must not be negative
//   kIdentity  S        S must be positive and finite
constexpr int kInverse = 0, kSqrt = 1, kIdentity = 2;
constexpr const char *kRefused[] = {"not positive and finite", "negative or not finite", "not positive and finite"};
constexpr const char *kProduct[] = {"inverse-noise band", "colouring band", "offset prior"};

// S_k of the statement at the top, and the bin kk of the PSD that it was read from
__device__ __forceinline__ double spectrum_at(const double *__restrict__ psd, int64_t b, int64_t k, int64_t nfreq,
                                              double fs, int64_t &kk)
{
    kk = k == 0 ? 1 : k;
    const double m = (kk == nfreq - 1) ? 1.0 : 2.0;
    return psd[b * nfreq + kk] * fs / m;
}

// sum_{k = first}^{end - 1} term(k) tab[phase_k]: serial and ascending in one accumulator from 0.0, the angle reduced
// in integers, phase_first = phase and phase_{k+1} = (phase_k + step) & mask, before the table sees it
template <class Term>
__device__ __forceinline__ double cos_sum(Term term, const double *__restrict__ tab, int64_t first, int64_t end,
                                          int64_t phase, int64_t step, int64_t mask)
{
    double acc = 0.0;
    for (int64_t k = first; k < end; ++k, phase = (phase + step) & mask) acc += term(k) * tab[phase];
    return acc;
}

namespace {                         // (kernels of a header and what launches them: one copy per translation unit)

// out[b][k] = G(S_k); *bad = the smallest b * nfreq + kk of a refused bin
template <int G>
__global__ __launch_bounds__(256) void k_bands_spectrum(const double *__restrict__ psd, int64_t nb, int64_t nfreq,
                                                         double fs, double *__restrict__ out,
                                                         unsigned long long *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * nfreq) return;
    const int64_t b = i / nfreq, k = i - b * nfreq;
    int64_t kk;
    const double S = spectrum_at(psd, b, k, nfreq, fs, kk);
    const double g = G == kInverse ? 1.0 / S : G == kSqrt ? sqrt(S) : S;
    const bool refused = G == kSqrt ? !(S >= 0.0) || !isfinite(S) : !(S > 0.0) || !isfinite(S) || !isfinite(g);
    if (refused) atomicMin(bad, (unsigned long long)(b * nfreq + kk));
    out[i] = g;
}

// tab[m] = cos(2 pi m / N), m < N (2m/N is exact: N is a power of two)
__global__ __launch_bounds__(256) void k_bands_cos_table(int64_t N, double *__restrict__ tab)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < N) tab[m] = cospi((double)(2 * m) / (double)N);
}

// d_out[nb][nfreq] = G(S) of the PSD d_psd[nb][nfreq]; a refused bin is a CM2_ERR_ARGUMENT naming block, bin and value
template <int G>
int spectrum(const double *d_psd, int64_t nb, int64_t nfreq, double fs, double *d_out, hipStream_t stream)
{
    DevTemp<unsigned long long> bad;
    CM2_HIP(bad.alloc(1));
    CM2_HIP(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), stream));
    k_bands_spectrum<G><<<blocks_for(nb * nfreq), kBlock, 0, stream>>>(d_psd, nb, nfreq, fs, d_out, bad);
    CM2_LAUNCH_OK();
    unsigned long long h_bad = 0;
    CM2_HIP(cm2::read_back(&h_bad, bad, sizeof(h_bad), stream));
    if (h_bad != ~0ULL) {
        double v = 0.0;
        CM2_HIP(cm2::read_back(&v, d_psd + h_bad, sizeof(v), stream));
        CM2_CHECK(false, "PSD of block %lld is %s at bin %lld (value %g): no %s can be built from it",
                  (long long)(h_bad / (unsigned long long)nfreq), kRefused[G], (long long)(h_bad % nfreq), v,
                  kProduct[G]);
    }
    return 0;
}

}  // namespace

}  // namespace psd
}  // namespace cm2
