// cm2_offset_prior.hip -- the destriper's noise model from a PSD: one white weight per noise block and the
// banded-Toeplitz prior C_a^-1 on the baseline offsets (interfaces/destriper.py solves with both).
//
// The third PSD -> band path beside cm2_noise_bands_from_psd (G = 1/S) and cm2_noise_filter_from_psd
// (G = sqrt(S)) of cm2_noise_model.hip; cm2_psd_bands.h has what the three share.  Per block, from one row P_k
// (k = 0 .. n/2, n = nperseg) of the Welch PSD, with the baseline length L:
//
//   spectrum<kIdentity> S_k as cm2_psd_bands.h states it; the first (block, bin) whose S is not positive and finite
//                      is refused
//   k_oprior_white     sigma^2 = (4/n) sum_{k = n/4}^{n/2 - 1} S_k: the white level, when the caller gives none
//   k_oprior_terms     W_k = m_k R_k D_k, R_k = max(S_k - sigma^2, 0) the correlated part,
//                      D_k = sin^2(L w_k / 2) / (L^2 sin^2(w_k / 2)), w_k = 2 pi k / n, D_0 = 1: the transfer
//                      function of the mean over L samples
//   k_oprior_q         q_j = (1/n) sum_k W_k cos(w_k L j), j < K = (n/2 + 1) / L: the covariance of two baseline
//                      means j baselines apart, (1/L^2) sum_{|s| < L} (L - |s|) r_{|jL + s|} with r = irfft(R, n),
//                      in closed form (no lag beyond n/2 is used); stored with its Bartlett taper,
//                      q~_j = (1 - j/K) q_j
//   k_oprior_invert    Q_i = q~_0 + 2 sum_{j = 1}^{K-1} q~_j cos(2 pi i j / M), i = 0 .. M/2, M the smallest power
//                      of two >= 2K: the offsets' spectrum, a Fejer-smoothed non-negative symbol;
//                      H_i = 1 / max(Q_i, floor sigma^2 / L)  (sigma^2 / L: the white variance of a baseline mean)
//   k_oprior_band      band_i = (1 - i/lambda) (1/M) sum_{k = 0}^{M/2} m'_k H_k cos(2 pi i k / M), i < lambda <= M/2
//                      (m' like m, on M): the second Bartlett taper makes every block SPD.
//
// One thread per output, every sum in increasing index order in one accumulator (the cosine sums are cos_sum of
// cm2_psd_bands.h), no atomics on doubles: a block processed alone gives the bits of the same block processed inside
// a group.  The angles are reduced in integers ((k L j) mod n, (k L) mod n, (i j) mod M) before cospi / sinpi see
// them.
#include "cm2_psd_bands.h"

#include <cmath>
#include <vector>

using namespace cm2;
using namespace cm2::psd;

namespace {

// one thread per block: the upper half of the band, in increasing k
__global__ __launch_bounds__(256) void k_oprior_white(const double *__restrict__ S, int64_t nb, int64_t n,
                                                       double *__restrict__ sigma2)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const double *s = S + b * (n / 2 + 1);
    double acc = 0.0;
    for (int64_t k = n / 4; k < n / 2; ++k) acc += s[k];
    sigma2[b] = (4.0 / (double)n) * acc;
}

__global__ __launch_bounds__(256) void k_oprior_terms(const double *__restrict__ S, const double *__restrict__ sigma2,
                                                       int64_t nb, int64_t n, int64_t L, double *__restrict__ W)
{
    const int64_t nfreq = n / 2 + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * nfreq) return;
    const int64_t b = i / nfreq, k = i - b * nfreq;
    double D = 1.0;
    if (k > 0) {
        int64_t a = (k * L) & (n - 1);                   // sin^2 has the period pi: (k L) mod n, folded to [0, n/2]
        if (a > n / 2) a = n - a;
        const double sn = sinpi((double)a / (double)n), sd = sinpi((double)k / (double)n);
        D = (sn * sn) / (((double)L * (double)L) * (sd * sd));
    }
    const double m = (k == 0 || k == nfreq - 1) ? 1.0 : 2.0;
    const double r = S[i] - sigma2[b];
    W[i] = (m * (r > 0.0 ? r : 0.0)) * D;
}

// one thread per (block, j < K)
__global__ __launch_bounds__(256) void k_oprior_q(const double *__restrict__ W, const double *__restrict__ tab,
                                                   int64_t nb, int64_t n, int64_t L, int64_t K,
                                                   double *__restrict__ qt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * K) return;
    const int64_t b = i / K, j = i - b * K;
    const int64_t nfreq = n / 2 + 1, mask = n - 1;
    const double *w = W + b * nfreq;
    const double acc = cos_sum([=](int64_t k) { return w[k]; }, tab, 0, nfreq, 0, (L * j) & mask, mask);
    qt[i] = (1.0 - (double)j / (double)K) * (acc / (double)n);
}

// one thread per (block, i <= M/2)
__global__ __launch_bounds__(256) void k_oprior_invert(const double *__restrict__ qt, const double *__restrict__ tab,
                                                        const double *__restrict__ sigma2, int64_t nb, int64_t K,
                                                        int64_t M, int64_t L, double floor, double *__restrict__ H)
{
    const int64_t nh = M / 2 + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * nh) return;
    const int64_t b = t / nh, i = t - b * nh;
    const int64_t mask = M - 1;
    const double *q = qt + b * K;
    const double acc = cos_sum([=](int64_t j) { return q[j]; }, tab, 1, K, i, i, mask);             // (i j) mod M
    const double Q = q[0] + 2.0 * acc;
    const double f = floor * sigma2[b] / (double)L;
    H[t] = 1.0 / (Q > f ? Q : f);
}

// one thread per (block, i < lambda)
__global__ __launch_bounds__(256) void k_oprior_band(const double *__restrict__ H, const double *__restrict__ tab,
                                                      int64_t nb, int64_t M, int64_t lambda,
                                                      double *__restrict__ bands)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * lambda) return;
    const int64_t b = t / lambda, i = t - b * lambda;
    const int64_t nh = M / 2 + 1, mask = M - 1;
    const double *h = H + b * nh;
    const auto term = [=](int64_t k) { return ((k == 0 || k == nh - 1) ? 1.0 : 2.0) * h[k]; };        // m'_k H_k
    const double acc = cos_sum(term, tab, 0, nh, 0, i, mask);                                       // (i k) mod M
    bands[t] = (1.0 - (double)i / (double)lambda) * (acc / (double)M);
}

}  // namespace

extern "C" int cm2_offset_prior_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                                         int64_t baseline_length, int64_t lambda, const double *h_sigma2_in,
                                         double floor, double *d_bands, double *h_sigma2_out, void *stream_)
{
    const char *who = "cm2_offset_prior_from_psd";
    if (int rc = check_args(who, d_psd, d_bands, nb, nperseg, fsample)) return rc;
    CM2_CHECK(baseline_length >= 1, "%s: baseline_length=%lld < 1", who, (long long)baseline_length);
    const int64_t n = nperseg, nfreq = n / 2 + 1, L = baseline_length;
    const int64_t K = nfreq / L;
    if (K < 2) {                                          // two baseline lags need n/2 + 1 >= 2L
        const int64_t need = L <= kMaxL ? pow2_at_least(4 * L - 2) : 2 * kMaxL;
        CM2_CHECK(need > kMaxL, "%s: nperseg=%lld holds %lld lag(s) of baselines of %lld samples, two are needed: "
                  "the smallest nperseg that would do is %lld", who, (long long)n, (long long)K, (long long)L,
                  (long long)need);
        CM2_CHECK(false, "%s: baselines of %lld samples are too long for any nperseg up to %lld (two lags need "
                  "nperseg/2 + 1 >= 2 baseline_length)", who, (long long)L, (long long)kMaxL);
    }
    const int64_t M = pow2_at_least(2 * K), nh = M / 2 + 1;
    CM2_CHECK(lambda >= 1 && lambda <= M / 2, "%s: lambda=%lld outside [1, M/2 = %lld] (K = %lld baseline lags, "
              "M = %lld)", who, (long long)lambda, (long long)(M / 2), (long long)K, (long long)M);
    CM2_CHECK(floor > 0.0 && floor <= 1.0, "%s: floor=%g outside (0, 1]", who, floor);
    if (h_sigma2_in)
        for (int64_t b = 0; b < nb; ++b)
            CM2_CHECK(h_sigma2_in[b] > 0.0 && std::isfinite(h_sigma2_in[b]),
                      "%s: sigma2 of block %lld is %g, not positive and finite", who, (long long)b, h_sigma2_in[b]);
    hipStream_t stream = as_stream(stream_);
    DevTemp<double> S, W, sigma2, tab_n, tab_m, qt, H;
    CM2_HIP(S.alloc(nb * nfreq));
    CM2_HIP(W.alloc(nb * nfreq));
    CM2_HIP(sigma2.alloc(nb));
    CM2_HIP(tab_n.alloc(n));
    CM2_HIP(tab_m.alloc(M));
    CM2_HIP(qt.alloc(nb * K));
    CM2_HIP(H.alloc(nb * nh));
    if (int rc = spectrum<kIdentity>(d_psd, nb, nfreq, fsample, S, stream)) return rc;
    std::vector<double> h_sigma2(nb);
    if (h_sigma2_in) {
        CM2_HIP(cm2::upload(sigma2, h_sigma2_in, sizeof(double) * nb, stream));
        for (int64_t b = 0; b < nb; ++b) h_sigma2[b] = h_sigma2_in[b];
    } else {
        k_oprior_white<<<blocks_for(nb), kBlock, 0, stream>>>(S, nb, n, sigma2);
        CM2_LAUNCH_OK();
        CM2_HIP(cm2::read_back(h_sigma2.data(), sigma2, sizeof(double) * nb, stream));
        for (int64_t b = 0; b < nb; ++b)                  // (every S is positive and finite: only an overflow)
            CM2_CHECK(h_sigma2[b] > 0.0 && std::isfinite(h_sigma2[b]),
                      "white level of block %lld is %g, not positive and finite: no offset prior can be built from "
                      "it", (long long)b, h_sigma2[b]);
    }
    k_oprior_terms<<<blocks_for(nb * nfreq), kBlock, 0, stream>>>(S, sigma2, nb, n, L, W);
    CM2_LAUNCH_OK();
    k_bands_cos_table<<<blocks_for(n), kBlock, 0, stream>>>(n, tab_n);
    CM2_LAUNCH_OK();
    k_bands_cos_table<<<blocks_for(M), kBlock, 0, stream>>>(M, tab_m);
    CM2_LAUNCH_OK();
    k_oprior_q<<<blocks_for(nb * K), kBlock, 0, stream>>>(W, tab_n, nb, n, L, K, qt);
    CM2_LAUNCH_OK();
    k_oprior_invert<<<blocks_for(nb * nh), kBlock, 0, stream>>>(qt, tab_m, sigma2, nb, K, M, L, floor, H);
    CM2_LAUNCH_OK();
    k_oprior_band<<<blocks_for(nb * lambda), kBlock, 0, stream>>>(H, tab_m, nb, M, lambda, d_bands);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(stream));      // (the temporaries go back to the cache on return)
    if (h_sigma2_out)
        for (int64_t b = 0; b < nb; ++b) h_sigma2_out[b] = h_sigma2[b];
    return 0;
}
