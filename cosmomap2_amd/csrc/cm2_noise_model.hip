// cm2_noise_model.hip -- estimating the banded-Toeplitz inverse noise N^-1 from the time streams.
//
// The reference has no estimator: its BlockLO / ToeplitzLO (interfaces/linearoperators.py:560-697, product
// at :582-595) only define what a band means, y_k = a0 v_k + sum_{i>=1} a_i (v_{k+i} + v_{k-i}).  Two steps:
//
//   cm2_psd_welch            Welch PSD per noise block, exactly scipy.signal.welch(x_b, fs, window='hann',
//                            nperseg=L, noverlap=L/2, detrend='constant'|False, scaling='density',
//                            average='mean'): segments of L samples every L/2 inside each block (a tail
//                            that does not fill a segment is ignored), periodic Hann window, one-sided
//                            |X|^2 summed in segment order.
//   cm2_noise_bands_from_psd PSD -> first row of an SPD inverse-noise band: S of cm2_psd_bands.h,
//                            G = 1/S, c_j = irfft(G, L)[j] as a fixed-order cosine sum, Bartlett taper
//                            a_j = (1 - j/lambda) c_j.  The symbol of the band is G smoothed by the Fejer
//                            kernel (>= 0), so every block is SPD by construction.
//   cm2_noise_filter_from_psd the same with G = sqrt(S): the band g of the symmetric FIR filter that colours
//                            white noise to the spectrum |g^|^2, g^ = sqrt(S) smoothed by the Fejer kernel
//                            (cm2_noise_sim.hip applies it).
//
// The Welch path runs over batches of a FIXED number of segments (set at cm2_psd_create from nperseg and the
// workspace cap; the last batch is padded with zero segments), so a segment's rocFFT transform is the same
// whichever segments share its batch, and the per-bin sums run in segment order across batch boundaries:
// a block estimated alone gives the bits of the same block estimated inside a group.
#include "cm2_psd_bands.h"
#include "cm2_rocfft.h"
#include "cm2_stream_policy.h"

#include <cmath>
#include <vector>

using namespace cm2;
using namespace cm2::psd;

namespace {

constexpr int64_t kBatchSamples = int64_t(1) << 24;     // segments per batch * L, at most (128 MB of input)

// One workgroup per segment of the batch: gather the L samples of segment g = first + blockIdx.x, subtract
// their mean (detrend = 1: every thread sums its samples j = t, t+256, ... in order, then the fixed tree of
// block_sum_256), multiply by the window.  Segments past the last one of the TOD are written as zeros.
__global__ __launch_bounds__(256) void k_psd_pack(const double *__restrict__ tod, const int64_t *__restrict__ off,
                                                   const int64_t *__restrict__ seg_off, int64_t nb, int64_t nseg,
                                                   int64_t first, int64_t L, int detrend,
                                                   const double *__restrict__ win, double *__restrict__ X)
{
    __shared__ double lds4[4];
    const int64_t g = first + blockIdx.x;
    double *x = X + (int64_t)blockIdx.x * L;
    if (g >= nseg) {
        for (int64_t j = threadIdx.x; j < L; j += blockDim.x) x[j] = 0.0;
        return;
    }
    const int64_t b = stream::locate(seg_off, nb, g);       // segments are numbered block after block
    const double *src = tod + off[b] + (g - seg_off[b]) * (L / 2);
    double mean = 0.0;
    if (detrend) {
        double s = 0.0;
        for (int64_t j = threadIdx.x; j < L; j += blockDim.x) s += src[j];
        s = block_sum_256(s, lds4);
        if (threadIdx.x == 0) lds4[0] = s / (double)L;
        __syncthreads();
        mean = lds4[0];
    }
    for (int64_t j = threadIdx.x; j < L; j += blockDim.x) x[j] = (src[j] - mean) * win[j];
}

// One thread per (block, bin) of the blocks that have segments in this batch: adds |X_s(k)|^2 of those
// segments, in segment order, to the running sum kept in psd.
__global__ __launch_bounds__(256) void k_psd_accumulate(const double2 *__restrict__ F, const int64_t *__restrict__ seg_off,
                                                         int64_t b_lo, int64_t nblk, int64_t nfreq, int64_t first,
                                                         int64_t batch, double *__restrict__ psd)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblk * nfreq) return;
    const int64_t b = b_lo + i / nfreq, k = i - (i / nfreq) * nfreq;
    const int64_t s0 = seg_off[b] > first ? seg_off[b] : first;
    const int64_t s1 = seg_off[b + 1] < first + batch ? seg_off[b + 1] : first + batch;
    double acc = psd[b * nfreq + k];
    const double2 *f = F + (s0 - first) * nfreq + k;
#pragma unroll 8
    for (int64_t s = s0; s < s1; ++s, f += nfreq) {
        const double2 v = *f;
        acc += v.x * v.x + v.y * v.y;
    }
    psd[b * nfreq + k] = acc;
}

// psd[b][k] *= m_k / (K_b fs sum w^2), m_k = 1 at k = 0 and k = L/2, 2 otherwise
__global__ __launch_bounds__(256) void k_psd_finish(const int64_t *__restrict__ seg_off, int64_t nb, int64_t nfreq,
                                                     double fs, double wsum2, double *__restrict__ psd)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * nfreq) return;
    const int64_t b = i / nfreq, k = i - b * nfreq;
    const double m = (k == 0 || k == nfreq - 1) ? 1.0 : 2.0;
    psd[i] = psd[i] * (m / ((double)(seg_off[b + 1] - seg_off[b]) * fs * wsum2));
}

// One thread per (block, lag j < lambda):
//   c_j = (G_0 + (-1)^j G_{L/2} + 2 sum_{k=1}^{L/2-1} G_k cos(2 pi j k / L)) / L     (= numpy.fft.irfft(G, L)[j])
//   a_j = (1 - j/lambda) c_j
// with the sum over k in increasing order.
__global__ __launch_bounds__(256) void k_bands_lags(const double *__restrict__ G, const double *__restrict__ tab,
                                                     int64_t nb, int64_t L, int64_t lambda, double *__restrict__ bands)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * lambda) return;
    const int64_t b = i / lambda, j = i - b * lambda;
    const int64_t nfreq = L / 2 + 1, mask = L - 1;
    const double *g = G + b * nfreq;
    const double acc = cos_sum([=](int64_t k) { return g[k]; }, tab, 1, nfreq - 1, j, j, mask);   // (j k) mod L
    const double nyq = (j & 1) ? -g[nfreq - 1] : g[nfreq - 1];
    const double c = (g[0] + nyq + 2.0 * acc) / (double)L;
    bands[i] = (1.0 - (double)j / (double)lambda) * c;
}

}  // namespace

struct cm2_psd {
    int64_t L = 0, nfreq = 0, batch = 0;
    int detrend = 1;
    double wsum2 = 0.0;           // sum of w_j^2
    double *d_win = nullptr;      // [L] periodic Hann window
    double *d_X = nullptr;        // [batch][L] windowed segments
    double2 *d_F = nullptr;       // [batch][L/2+1] their transforms
    cm2::RealFft fft;             // forward transform of `batch` segments
    ~cm2_psd() { dev_release(d_win, d_X, d_F); }
};

extern "C" int cm2_psd_destroy(cm2_psd *p)
{
    delete p;
    return 0;
}

static int psd_build(cm2_psd *p, int64_t max_work_bytes, hipStream_t stream)
{
    const int64_t L = p->L;
    const int64_t per_seg = (int64_t)(sizeof(double) * L + sizeof(double2) * p->nfreq);
    int64_t batch = kBatchSamples / L;
    if (batch * per_seg > max_work_bytes) batch = max_work_bytes / per_seg;
    if (batch < 1) batch = 1;
    // the rocFFT work buffer counts against the cap too: halve the batch until it fits (or is one segment)
    for (;;) {
        if (int rc = p->fft.plan(L, batch, false)) return rc;
        if (batch == 1 || batch * per_seg + (int64_t)p->fft.work_bytes <= max_work_bytes) break;
        batch /= 2;
    }
    p->batch = batch;
    std::vector<double> w(L);
    double s2 = 0.0;
    for (int64_t j = 0; j < L; ++j) {
        w[j] = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)j / (double)L);
        s2 += w[j] * w[j];
    }
    p->wsum2 = s2;
    CM2_HIP(cm2::dev_malloc(&p->d_win, sizeof(double) * L));
    CM2_HIP(cm2::upload(p->d_win, w.data(), sizeof(double) * L, stream));
    CM2_HIP(cm2::dev_malloc(&p->d_X, sizeof(double) * L * batch));
    CM2_HIP(cm2::dev_malloc(&p->d_F, sizeof(double2) * p->nfreq * batch));
    return p->fft.bind();
}

extern "C" int cm2_psd_create(cm2_psd **out, int64_t nperseg, int detrend, int64_t max_work_bytes, void *stream_)
{
    CM2_CHECK(out, "cm2_psd_create: NULL argument");
    *out = nullptr;
    CM2_CHECK_NPERSEG("cm2_psd_create", nperseg);
    CM2_CHECK(detrend == 0 || detrend == 1, "cm2_psd_create: detrend=%d (0 = none, 1 = constant)", detrend);
    if (max_work_bytes <= 0) max_work_bytes = int64_t(512) << 20;
    cm2_psd *p = new cm2_psd();
    p->L = nperseg;
    p->nfreq = nperseg / 2 + 1;
    p->detrend = detrend;
    if (int rc = psd_build(p, max_work_bytes, as_stream(stream_))) {
        cm2_psd_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int cm2_psd_info(const cm2_psd *p, int64_t *h_info)
{
    CM2_CHECK(p && h_info, "cm2_psd_info: NULL argument");
    h_info[0] = p->L;
    h_info[1] = p->batch;
    h_info[2] = (int64_t)(sizeof(double) * p->L * p->batch + sizeof(double2) * p->nfreq * p->batch +
                          p->fft.work_bytes);
    return 0;
}

extern "C" int cm2_psd_welch(cm2_psd *p, const double *d_tod, const int64_t *h_sizes, int64_t nb, double fsample,
                             double *d_psd, void *stream_)
{
    CM2_CHECK(p && d_tod && h_sizes && d_psd, "cm2_psd_welch: NULL argument");
    CM2_CHECK(nb >= 1, "cm2_psd_welch: nb=%lld < 1", (long long)nb);
    CM2_CHECK(fsample > 0.0 && std::isfinite(fsample), "cm2_psd_welch: fsample=%g is not positive", fsample);
    hipStream_t stream = as_stream(stream_);
    const int64_t L = p->L, half = L / 2, nfreq = p->nfreq, batch = p->batch;
    std::vector<int64_t> off(nb + 1, 0), seg_off(nb + 1, 0);
    for (int64_t b = 0; b < nb; ++b) {
        CM2_CHECK(h_sizes[b] >= L, "cm2_psd_welch: block %lld has %lld samples, fewer than nperseg=%lld",
                  (long long)b, (long long)h_sizes[b], (long long)L);
        off[b + 1] = off[b] + h_sizes[b];
        seg_off[b + 1] = seg_off[b] + (h_sizes[b] - L) / half + 1;
    }
    const int64_t nseg = seg_off[nb];
    DevTemp<int64_t> d_off, d_seg_off;
    CM2_HIP(d_off.alloc(nb + 1));
    CM2_HIP(d_seg_off.alloc(nb + 1));
    CM2_HIP(cm2::upload(d_off, off.data(), sizeof(int64_t) * (nb + 1), stream));
    CM2_HIP(cm2::upload(d_seg_off, seg_off.data(), sizeof(int64_t) * (nb + 1), stream));
    CM2_HIP(hipMemsetAsync(d_psd, 0, sizeof(double) * nb * nfreq, stream));
    if (int rc = p->fft.set_stream(stream)) return rc;
    int64_t b_lo = 0;
    for (int64_t first = 0; first < nseg; first += batch) {
        k_psd_pack<<<(unsigned)batch, kBlock, 0, stream>>>(d_tod, d_off, d_seg_off, nb, nseg, first, L, p->detrend,
                                                           p->d_win, p->d_X);
        CM2_LAUNCH_OK();
        if (int rc = p->fft.forward(p->d_X, p->d_F)) return rc;
        // blocks with segments in [first, first + batch)
        while (seg_off[b_lo + 1] <= first) ++b_lo;
        int64_t b_hi = b_lo;
        while (b_hi + 1 < nb && seg_off[b_hi + 1] < first + batch) ++b_hi;
        const int64_t nblk = b_hi - b_lo + 1;
        k_psd_accumulate<<<(unsigned)((nblk * nfreq + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
            p->d_F, d_seg_off, b_lo, nblk, nfreq, first, batch, d_psd);
        CM2_LAUNCH_OK();
    }
    k_psd_finish<<<(unsigned)((nb * nfreq + kBlock - 1) / kBlock), kBlock, 0, stream>>>(d_seg_off, nb, nfreq, fsample,
                                                                                        p->wsum2, d_psd);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(stream));      // (d_off / d_seg_off go back to the cache on return)
    return 0;
}

// PSD -> band with G = 1/S (kInverse) or G = sqrt(S) (kSqrt): the two entry points below
template <int G>
static int bands_from_psd(const char *who, const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                          int64_t lambda, double *d_bands, void *stream_)
{
    if (int rc = check_args(who, d_psd, d_bands, nb, nperseg, fsample)) return rc;
    CM2_CHECK(lambda >= 1 && lambda <= nperseg / 2, "%s: lambda=%lld outside [1, %lld]", who,
              (long long)lambda, (long long)(nperseg / 2));
    hipStream_t stream = as_stream(stream_);
    const int64_t L = nperseg, nfreq = L / 2 + 1;
    DevTemp<double> Gk, tab;
    CM2_HIP(Gk.alloc(nb * nfreq));
    CM2_HIP(tab.alloc(L));
    if (int rc = spectrum<G>(d_psd, nb, nfreq, fsample, Gk, stream)) return rc;
    k_bands_cos_table<<<blocks_for(L), kBlock, 0, stream>>>(L, tab);
    CM2_LAUNCH_OK();
    k_bands_lags<<<blocks_for(nb * lambda), kBlock, 0, stream>>>(Gk, tab, nb, L, lambda, d_bands);
    CM2_LAUNCH_OK();
    CM2_HIP(hipStreamSynchronize(stream));      // (Gk, tab go back to the cache on return)
    return 0;
}

extern "C" int cm2_noise_bands_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                                        int64_t lambda, double *d_bands, void *stream_)
{
    return bands_from_psd<kInverse>("cm2_noise_bands_from_psd", d_psd, nb, nperseg, fsample, lambda, d_bands, stream_);
}

extern "C" int cm2_noise_filter_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                                         int64_t lambda, double *d_bands, void *stream_)
{
    return bands_from_psd<kSqrt>("cm2_noise_filter_from_psd", d_psd, nb, nperseg, fsample, lambda, d_bands, stream_);
}
