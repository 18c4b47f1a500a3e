// cm2_noise.hip -- the inverse noise operator N^-1 on the TOD stream.
//
// Reference code replaced:
//   BlockLO / build_blocks            interfaces/linearoperators.py:655-690
//   blk_matvec (per-block dispatch)   interfaces/blkop.py:178-208
//   ToeplitzLO.mult                   interfaces/linearoperators.py:582-595
//
// Two block kinds, both block-diagonal over `nblocks` stationary intervals:
//   * constant diagonal  t_b * I                       (offdiag=False)
//   * symmetric banded Toeplitz with first row a_b[0..lambda-1], ZERO boundary at
//     both ends of every block (the reference is not circulant, :592-593)
//
// Toeplitz is applied
//   DIRECT  : y_k = a0 v_k + sum_i a_i v_{k+i} + a_i v_{k-i} in the reference's term
//             order (bit-exact; O(n*lambda), used for short bands), or
//   FFT     : overlap-save with rocFFT fp64 R2C/C2R of length L: each segment carries
//             hop = L - 2(lambda-1) new samples plus a halo of lambda-1 on both sides,
//             zero outside its block; spectrum of the band is real (symmetric kernel)
//             and is evaluated in closed form H_k = (a0 + 2 sum_j a_j cos(2 pi j k/L))/L.
// Algorithmic traffic 16 B/sample (read v, write y); the rocFFT route moves
// ~7x that through HBM (pack, 2 FFTs, spectrum multiply, unpack) -- see DESIGN.md.
#include "cm2_overlap_save.h"
#include "cm2_rocfft.h"
#include "cm2_tiles.h"

#include <cstdlib>
#include <mutex>
#include <vector>

using namespace cm2;

// one work item of the tiled direct Toeplitz kernel
struct DirTile {
    int64_t start;      // first output sample
    int32_t len, blk;
};

// The state of a Toeplitz operator in three parts, one per route of application, each the owner of what it
// holds: reset() (and the destructor) frees it.  An operator fills the part of its method at creation.

// DIRECT, LDS-tiled: the work list of k_toeplitz_direct_tiled (empty for a band too long for the LDS, which
// the plain loop serves)
struct DirRoute : NoCopy {
    size_t lds = 0;                  // dynamic LDS of the tiled kernel for this band
    DirTile *d_tiles = nullptr;
    int64_t ntiles = 0;
    ~DirRoute() { reset(); }
    void reset()
    {
        dev_release(d_tiles);
        ntiles = 0;
        lds = 0;
    }
};

// FFT: overlap-save through rocFFT, all segments in one batch
struct FftRoute : NoCopy {
    int64_t nseg = 0, nfreq = 0;
    int64_t *d_seg = nullptr;    // [nseg*4]: out_start, out_len, blk_lo, blk_hi
    int32_t *d_seg_blk = nullptr;
    double *d_X = nullptr;       // [nseg][L]
    double2 *d_F = nullptr;      // [nseg][L/2+1]
    double *d_H = nullptr;       // [nb][L/2+1] real spectra, 1/L folded in
    RealFft fft;                 // forward and inverse of nseg segments, one info, one work buffer
    ~FftRoute() { reset(); }
    void reset()
    {
        dev_release(d_seg, d_seg_blk, d_X, d_F, d_H);
        fft.reset();
        nseg = nfreq = 0;
    }
};

// FUSED: the register-FFT overlap-save kernel (cm2_overlap_save.hip).  Set at creation for method
// CM2_TOEPLITZ_FUSED; for AUTO -> DIRECT / FFT operators built on first application on a tile order.
struct FusedRoute : NoCopy {
    FusedOS *os = nullptr;
    ~FusedRoute() { reset(); }
    void reset()
    {
        if (os) fused_os_destroy(os);
        os = nullptr;
    }
};

struct cm2_noise : NoCopy {
    int64_t nt = 0, nb = 0, lambda = 0;
    int method = 0;
    bool equal_sizes = true;
    int64_t bsize = 0;
    int64_t *d_off = nullptr;    // [nb+1] block offsets
    double *d_t = nullptr;       // [nb] diagonal values  | [nb*lambda] bands
    int64_t L = 0, hop = 0, halo = 0;   // overlap-save geometry (FFT and FUSED)
    DirRoute dir;
    FftRoute fft;
    FusedRoute fused;
    bool auto_method = false;        // the caller left the choice to the library
    std::vector<int64_t> h_off;      // block offsets (host)
    std::mutex mu;                   // lazy creation of `fused.os`
    ~cm2_noise() { dev_release(d_off, d_t); }
};

__device__ __forceinline__ int find_block(const int64_t *__restrict__ off, int nb, int64_t k,
                                          bool equal, int64_t bsize)
{
    if (equal) return (int)(k / bsize);
    int lo = 0, hi = nb;              // largest b with off[b] <= k
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------- diagonal -------
__global__ __launch_bounds__(256) void k_diag_apply(int64_t nt, int nb, bool equal, int64_t bsize,
                                                     const int64_t *__restrict__ off,
                                                     const double *__restrict__ t,
                                                     const double *__restrict__ v,
                                                     double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nt; k += stride) {
        const int b = find_block(off, nb, k, equal, bsize);
        out[k] = v ? t[b] * v[k] : t[b];     // lp.DiagonalOperator: diag * x
    }
}

// --------------------------------------------------- Toeplitz, direct ---------
// Term order of the NumPy loop linearoperators.py:587-593:
//   a0 v_k, then for i = 1..lambda-1:  + a_i v_{k+i} (y[:-i]+=temp[i:]),  + a_i v_{k-i}
__global__ __launch_bounds__(256) void k_toeplitz_direct(int64_t nt, int nb, bool equal,
                                                          int64_t bsize, int64_t lambda,
                                                          const int64_t *__restrict__ off,
                                                          const double *__restrict__ bands,
                                                          const double *__restrict__ v,
                                                          double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nt; k += stride) {
        const int b = find_block(off, nb, k, equal, bsize);
        const int64_t lo = off[b], hi = off[b + 1];
        const double *a = bands + (int64_t)b * lambda;
        double acc = a[0] * v[k];
        for (int64_t i = 1; i < lambda; ++i) {
            if (k + i < hi) acc += a[i] * v[k + i];
            if (k - i >= lo) acc += a[i] * v[k - i];
        }
        out[k] = acc;
    }
}

// LDS-tiled form of the same sum.  A workgroup owns kDirTile consecutive outputs of one block,
// stages them with a halo of lambda-1 samples on both sides (zeros outside the block: adding
// a_i * 0 leaves every partial sum unchanged, so the boundary tests of the loop above are not
// needed) and each thread forms kDirPer outputs, 256 apart, with the reference's term order.
// 2(lambda-1) LDS reads per output instead of as many cache accesses.
constexpr int kDirTile = 2048, kDirT = 256, kDirPer = kDirTile / kDirT;

__global__ __launch_bounds__(kDirT) void k_toeplitz_direct_tiled(const DirTile *__restrict__ tiles,
                                                                  int64_t lambda,
                                                                  const int64_t *__restrict__ off,
                                                                  const double *__restrict__ bands,
                                                                  const double *__restrict__ v,
                                                                  double *__restrict__ out)
{
    extern __shared__ double dir_lds[];                 // kDirTile + 2 (lambda - 1) doubles
    const DirTile tl = tiles[blockIdx.x];
    const int64_t lo = off[tl.blk], hi = off[tl.blk + 1];
    const int halo = (int)(lambda - 1), span = kDirTile + 2 * halo;
    const int64_t w0 = tl.start - halo;
    for (int j = threadIdx.x; j < span; j += kDirT) {
        const int64_t ts = w0 + j;
        dir_lds[j] = (ts >= lo && ts < hi && j < tl.len + 2 * halo) ? v[ts] : 0.0;
    }
    __syncthreads();
    const double *a = bands + (int64_t)tl.blk * lambda;
    const double *c = dir_lds + halo + threadIdx.x;     // c[256 u] = v at this thread's output u
    double acc[kDirPer];
#pragma unroll
    for (int u = 0; u < kDirPer; ++u) acc[u] = a[0] * c[kDirT * u];
    for (int i = 1; i < (int)lambda; ++i) {
        const double ai = a[i];
#pragma unroll
        for (int u = 0; u < kDirPer; ++u) {
            acc[u] += ai * c[kDirT * u + i];
            acc[u] += ai * c[kDirT * u - i];
        }
    }
#pragma unroll
    for (int u = 0; u < kDirPer; ++u) {
        const int j = threadIdx.x + kDirT * u;
        if (j < tl.len) out[tl.start + j] = acc[u];
    }
}

// --------------------------------------------------- Toeplitz, overlap-save ---
// H[b][k] = (a0 + 2 sum_{j>=1} a_j cos(2 pi (j k mod L) / L)) / L
__global__ __launch_bounds__(256) void k_spectrum(int nb, int64_t lambda, int64_t L, int64_t nfreq,
                                                   const double *__restrict__ bands,
                                                   double *__restrict__ H)
{
    const int64_t total = (int64_t)nb * nfreq;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t b = e / nfreq, k = e % nfreq;
        const double *a = bands + b * lambda;
        double acc = 0.0;
        for (int64_t j = lambda - 1; j >= 1; --j) {       // small terms first
            const int64_t m = (j * k) % L;
            acc += a[j] * cospi(2.0 * (double)m / (double)L);
        }
        H[e] = (a[0] + 2.0 * acc) / (double)L;
    }
}

__global__ __launch_bounds__(256) void k_pack(int64_t L, int64_t halo,
                                               const int64_t *__restrict__ seg,
                                               const double *__restrict__ v,
                                               double *__restrict__ X)
{
    const int64_t s = blockIdx.y;
    const int64_t out_start = seg[4 * s], lo = seg[4 * s + 2], hi = seg[4 * s + 3];
    double *x = X + s * L;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < L;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = out_start - halo + j;
        x[j] = (src >= lo && src < hi) ? v[src] : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_spec_mul(int64_t nfreq, const int32_t *__restrict__ seg_blk,
                                                   const double *__restrict__ H,
                                                   double2 *__restrict__ F)
{
    const int64_t s = blockIdx.y;
    const double *h = H + (int64_t)seg_blk[s] * nfreq;
    double2 *f = F + s * nfreq;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nfreq;
         k += (int64_t)gridDim.x * blockDim.x) {
        double2 z = f[k];
        const double hk = h[k];
        z.x *= hk;
        z.y *= hk;
        f[k] = z;
    }
}

__global__ __launch_bounds__(256) void k_unpack(int64_t L, int64_t halo,
                                                 const int64_t *__restrict__ seg,
                                                 const double *__restrict__ X,
                                                 double *__restrict__ out)
{
    const int64_t s = blockIdx.y;
    const int64_t out_start = seg[4 * s], out_len = seg[4 * s + 1];
    const double *x = X + s * L + halo;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < out_len;
         j += (int64_t)gridDim.x * blockDim.x)
        out[out_start + j] = x[j];
}

// ------------------------------------------------------------------ C ABI ------
// block offsets on the host and the device, the values (diagonal entries or bands) on the device
static int noise_common(cm2_noise *n, const double *h_vals, int64_t per_block, const int64_t *h_sizes,
                        int64_t nb)
{
    CM2_CHECK(nb >= 1, "noise operator needs at least one block (nblocks=%lld)", (long long)nb);
    std::vector<int64_t> &off = n->h_off;
    off.assign(nb + 1, 0);
    n->equal_sizes = true;
    for (int64_t b = 0; b < nb; ++b) {
        CM2_CHECK(h_sizes[b] > 0, "block %lld has non-positive size %lld", (long long)b,
                  (long long)h_sizes[b]);
        off[b + 1] = off[b] + h_sizes[b];
        if (h_sizes[b] != h_sizes[0]) n->equal_sizes = false;
    }
    n->nb = nb;
    n->nt = off[nb];
    n->bsize = h_sizes[0];
    CM2_HIP(cm2::dev_malloc(&n->d_off, sizeof(int64_t) * (nb + 1)));
    CM2_HIP(cm2::upload(n->d_off, off.data(), sizeof(int64_t) * (nb + 1), nullptr));
    CM2_HIP(cm2::dev_malloc(&n->d_t, sizeof(double) * nb * per_block));
    CM2_HIP(cm2::upload(n->d_t, h_vals, sizeof(double) * nb * per_block, nullptr));
    return 0;
}

static int64_t pick_fft_length(int64_t halo, int64_t max_block)
{
    if (const char *e = getenv("CM2_FFT_LEN")) {
        const int64_t v = atoll(e);
        if (v > 2 * halo + 1) return v;
    }
    int64_t L = 256;
    while (L < 8 * halo) L <<= 1;                 // hop >= 3/4 L
    int64_t need = 1;                             // but never longer than one padded block
    while (need < max_block + 2 * halo) need <<= 1;
    if (need < L) L = need;
    if (L < 2 * halo + 2) L = 2 * (2 * halo + 2);
    return L;
}

// a band too long for the LDS of the tiled direct kernel (or an empty TOD) takes the plain loop
static bool dir_plain_loop(size_t lds, int64_t nt) { return lds > 150 * 1024 || nt == 0; }

// DIRECT: the work list of the tiled kernel, kDirTile outputs of one block per workgroup
static int dir_build(cm2_noise *n)
{
    DirRoute &d = n->dir;
    d.lds = sizeof(double) * (size_t)(kDirTile + 2 * (n->lambda - 1));
    if (dir_plain_loop(d.lds, n->nt)) return 0;
    const std::vector<int64_t> &off = n->h_off;
    std::vector<DirTile> tl;
    for (int64_t b = 0; b < n->nb; ++b)
        for (int64_t s0 = off[(size_t)b]; s0 < off[(size_t)b + 1]; s0 += kDirTile) {
            DirTile t;
            t.start = s0;
            t.len = (int32_t)(off[(size_t)b + 1] - s0 < kDirTile ? off[(size_t)b + 1] - s0 : kDirTile);
            t.blk = (int32_t)b;
            tl.push_back(t);
        }
    CM2_HIP(cm2::dev_malloc(&d.d_tiles, sizeof(DirTile) * tl.size()));
    CM2_HIP(cm2::upload(d.d_tiles, tl.data(), sizeof(DirTile) * tl.size(), nullptr));
    d.ntiles = (int64_t)tl.size();
    return 0;
}

// FFT: segments, spectra of the bands and the rocFFT plans
static int fft_build(cm2_noise *n, hipStream_t stream)
{
    FftRoute &f = n->fft;
    const std::vector<int64_t> &off = n->h_off;
    int64_t max_block = 0;
    for (int64_t b = 0; b < n->nb; ++b)
        max_block = off[b + 1] - off[b] > max_block ? off[b + 1] - off[b] : max_block;
    n->halo = n->lambda - 1;
    n->L = pick_fft_length(n->halo, max_block);
    n->hop = n->L - 2 * n->halo;
    f.nfreq = n->L / 2 + 1;
    std::vector<int64_t> seg;
    std::vector<int32_t> seg_blk;
    for (int64_t b = 0; b < n->nb; ++b) {
        for (int64_t s0 = off[b]; s0 < off[b + 1]; s0 += n->hop) {
            const int64_t len = (off[b + 1] - s0 < n->hop) ? off[b + 1] - s0 : n->hop;
            seg.push_back(s0);
            seg.push_back(len);
            seg.push_back(off[b]);
            seg.push_back(off[b + 1]);
            seg_blk.push_back((int32_t)b);
        }
    }
    f.nseg = (int64_t)seg_blk.size();
    CM2_CHECK(f.nseg < 65536LL * 32768LL, "too many FFT segments (%lld)", (long long)f.nseg);
    CM2_HIP(cm2::dev_malloc(&f.d_seg, sizeof(int64_t) * seg.size()));
    CM2_HIP(cm2::dev_malloc(&f.d_seg_blk, sizeof(int32_t) * seg_blk.size()));
    CM2_HIP(cm2::upload(f.d_seg, seg.data(), sizeof(int64_t) * seg.size(), nullptr));
    CM2_HIP(cm2::upload(f.d_seg_blk, seg_blk.data(), sizeof(int32_t) * seg_blk.size(), nullptr));
    CM2_HIP(cm2::dev_malloc(&f.d_X, sizeof(double) * f.nseg * n->L));
    CM2_HIP(cm2::dev_malloc(&f.d_F, sizeof(double2) * f.nseg * f.nfreq));
    CM2_HIP(cm2::dev_malloc(&f.d_H, sizeof(double) * n->nb * f.nfreq));
    k_spectrum<<<grid_for(n->nb * f.nfreq), kBlock, 0, stream>>>((int)n->nb, n->lambda, n->L, f.nfreq,
                                                                 n->d_t, f.d_H);
    CM2_LAUNCH_OK();
    if (int rc = f.fft.plan(n->L, f.nseg, true)) return rc;
    if (int rc = f.fft.bind()) return rc;
    CM2_HIP(hipStreamSynchronize(stream));
    return 0;
}

// The one build path of both kinds of operator (lambda = 0: constant diagonal).  It may return from any
// line: the caller destroys the operator, which frees what was built so far.
static int noise_build(cm2_noise *n, const double *h_vals, int64_t lambda, const int64_t *h_sizes,
                       int64_t nblocks, int method, hipStream_t stream)
{
    if (int rc = noise_common(n, h_vals, lambda ? lambda : 1, h_sizes, nblocks)) return rc;
    n->lambda = lambda;
    if (lambda == 0) return 0;
    n->auto_method = (method == CM2_TOEPLITZ_AUTO);
    if (method == CM2_TOEPLITZ_AUTO)
        method = (lambda <= 32) ? CM2_TOEPLITZ_DIRECT
                                : (cm2::fused_os_supported(lambda) ? CM2_TOEPLITZ_FUSED
                                                                   : CM2_TOEPLITZ_FFT);
    n->method = method;
    if (method == CM2_TOEPLITZ_DIRECT) return dir_build(n);
    if (method == CM2_TOEPLITZ_FFT) return fft_build(n, stream);
    if (int rc = cm2::fused_os_create(&n->fused.os, n->d_t, lambda, n->h_off, stream)) return rc;
    n->L = cm2::fused_os_length(n->fused.os);
    n->halo = lambda - 1;
    n->hop = n->L - 2 * n->halo;
    return 0;
}

// new, build, and on failure destroy: nothing between `new` and the hand-over to *out returns early
static int noise_create(cm2_noise **out, const double *h_vals, int64_t lambda, const int64_t *h_sizes,
                        int64_t nblocks, int method, hipStream_t stream)
{
    cm2_noise *n = new cm2_noise();
    const int rc = noise_build(n, h_vals, lambda, h_sizes, nblocks, method, stream);
    if (rc) {
        cm2_noise_destroy(n);
        return rc;
    }
    *out = n;
    return 0;
}

extern "C" int cm2_noise_destroy(cm2_noise *n)
{
    delete n;                // every part frees what it owns
    return 0;
}

extern "C" int cm2_noise_create_diag(cm2_noise **out, const double *h_t, const int64_t *h_sizes,
                                     int64_t nblocks)
{
    CM2_CHECK(out && h_t && h_sizes, "cm2_noise_create_diag: NULL argument");
    *out = nullptr;
    return noise_create(out, h_t, 0, h_sizes, nblocks, 0, nullptr);
}

extern "C" int cm2_noise_create_toeplitz(cm2_noise **out, const double *h_bands, int64_t lambda,
                                         const int64_t *h_sizes, int64_t nblocks, int method,
                                         void *stream_)
{
    CM2_CHECK(out && h_bands && h_sizes, "cm2_noise_create_toeplitz: NULL argument");
    CM2_CHECK(lambda >= 1, "cm2_noise_create_toeplitz: band length lambda=%lld < 1", (long long)lambda);
    CM2_CHECK(method >= 0 && method <= 3, "cm2_noise_create_toeplitz: bad method %d", method);
    *out = nullptr;
    return noise_create(out, h_bands, lambda, h_sizes, nblocks, method, as_stream(stream_));
}

extern "C" int cm2_noise_info(const cm2_noise *n, int64_t *h_info)
{
    CM2_CHECK(n && h_info, "cm2_noise_info: NULL argument");
    h_info[0] = n->nt; h_info[1] = n->nb; h_info[2] = n->lambda;
    h_info[3] = n->method; h_info[4] = n->L;
    h_info[5] = (n->lambda > 0 && (n->method == CM2_TOEPLITZ_FUSED ||
                                    (n->auto_method && cm2::fused_os_supported(n->lambda)))) ? 1 : 0;
    return 0;
}

extern "C" int cm2_noise_tile_kernel_info(const cm2_noise *n, int64_t *h_info, double *h_bytes_per_sample)
{
    CM2_CHECK(n && h_info && h_bytes_per_sample, "cm2_noise_tile_kernel_info: NULL argument");
    int kernel[2] = {0, 0};
    *h_bytes_per_sample = cm2::fused_os_tile_info(n->fused.os, kernel);
    h_info[0] = kernel[0];
    h_info[1] = kernel[1];
    h_info[2] = 512 * (int64_t)kernel[0];                 // window samples
    h_info[3] = 0;                                        // (reserved: cosmomap2.h)
    return 0;
}

extern "C" int cm2_noise_expand_diag(const cm2_noise *n, double *d_w, void *stream_)
{
    CM2_CHECK(n && d_w, "cm2_noise_expand_diag: NULL argument");
    CM2_CHECK(n->lambda == 0, "cm2_noise_expand_diag: operator has off-diagonal terms");
    k_diag_apply<<<grid_for(n->nt), kBlock, 0, as_stream(stream_)>>>(
        n->nt, (int)n->nb, n->equal_sizes, n->bsize, n->d_off, n->d_t, nullptr, d_w);
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_noise_apply(cm2_noise *n, const double *d_v, double *d_out, void *stream_)
{
    CM2_CHECK(n && d_v && d_out, "cm2_noise_apply: NULL argument");
    CM2_CHECK(d_v != d_out, "cm2_noise_apply: in-place application is not supported");
    hipStream_t stream = as_stream(stream_);
    if (n->lambda == 0) {
        k_diag_apply<<<grid_for(n->nt), kBlock, 0, stream>>>(n->nt, (int)n->nb, n->equal_sizes,
                                                             n->bsize, n->d_off, n->d_t, d_v, d_out);
        CM2_LAUNCH_OK();
        return 0;
    }
    if (n->method == CM2_TOEPLITZ_DIRECT) {
        const DirRoute &d = n->dir;
        if (dir_plain_loop(d.lds, n->nt)) {             // very long bands: the plain loop
            k_toeplitz_direct<<<grid_for(n->nt), kBlock, 0, stream>>>(
                n->nt, (int)n->nb, n->equal_sizes, n->bsize, n->lambda, n->d_off, n->d_t, d_v, d_out);
            CM2_LAUNCH_OK();
            return 0;
        }
        if (d.lds > 64 * 1024) {
            static size_t granted[64] = {0};
            CM2_HIP(ensure_dynamic_lds((const void *)k_toeplitz_direct_tiled, d.lds, granted));
        }
        if (d.ntiles)
            k_toeplitz_direct_tiled<<<(unsigned)d.ntiles, kDirT, d.lds, stream>>>(
                d.d_tiles, n->lambda, n->d_off, n->d_t, d_v, d_out);
        CM2_LAUNCH_OK();
        return 0;
    }
    if (n->method == CM2_TOEPLITZ_FUSED) return cm2::fused_os_apply(n->fused.os, d_v, d_out, stream);
    // overlap-save: pack -> R2C -> spectrum multiply -> C2R -> unpack
    FftRoute &f = n->fft;
    const int gx_L = (int)((n->L + kBlock * 4 - 1) / (kBlock * 4));
    const int64_t per_launch = 65535;             // gridDim.y limit
    for (int64_t s0 = 0; s0 < f.nseg; s0 += per_launch) {
        const int ny = (int)((f.nseg - s0 < per_launch) ? f.nseg - s0 : per_launch);
        k_pack<<<dim3(gx_L, ny), kBlock, 0, stream>>>(n->L, n->halo, f.d_seg + 4 * s0, d_v,
                                                      f.d_X + s0 * n->L);
        CM2_LAUNCH_OK();
    }
    if (int rc = f.fft.set_stream(stream)) return rc;
    if (int rc = f.fft.forward(f.d_X, f.d_F)) return rc;
    const int gx_F = (int)((f.nfreq + kBlock * 4 - 1) / (kBlock * 4));
    for (int64_t s0 = 0; s0 < f.nseg; s0 += per_launch) {
        const int ny = (int)((f.nseg - s0 < per_launch) ? f.nseg - s0 : per_launch);
        k_spec_mul<<<dim3(gx_F, ny), kBlock, 0, stream>>>(f.nfreq, f.d_seg_blk + s0, f.d_H,
                                                          f.d_F + s0 * f.nfreq);
        CM2_LAUNCH_OK();
    }
    if (int rc = f.fft.inverse(f.d_F, f.d_X)) return rc;
    const int gx_O = (int)((n->hop + kBlock * 4 - 1) / (kBlock * 4));
    for (int64_t s0 = 0; s0 < f.nseg; s0 += per_launch) {
        const int ny = (int)((f.nseg - s0 < per_launch) ? f.nseg - s0 : per_launch);
        k_unpack<<<dim3(gx_O, ny), kBlock, 0, stream>>>(n->L, n->halo, f.d_seg + 4 * s0,
                                                        f.d_X + s0 * n->L, d_out);
        CM2_LAUNCH_OK();
    }
    return 0;
}

// N^-1 applied to a TOD held in the tile-bucketed order of cm2_tiles (input and output):
// the overlap-save kernel gathers its segment through the tile index and scatters the
// result back the same way, so no time-ordered copy of the TOD is ever written.
static int noise_tiles_ready(cm2_noise *n, const cm2_tiles *tiles, const char *who, void *stream_)
{
    if (n->auto_method && n->method != CM2_TOEPLITZ_FUSED && n->lambda > 0 && cm2::fused_os_supported(n->lambda)) {
        // the method was left to the library and resolved to the direct sum (short band) for
        // the time order; on a tile order the fused overlap-save kernel is the fast one.  n->fused.os is
        // only read and written under the operator's lock on this path (application calls of several
        // host threads may meet here; the operators built with CM2_TOEPLITZ_FUSED set it at creation).
        std::lock_guard<std::mutex> lock(n->mu);
        if (!n->fused.os)
            if (int rc = cm2::fused_os_create(&n->fused.os, n->d_t, n->lambda, n->h_off, as_stream(stream_)))
                return rc;
    }
    CM2_CHECK(n->fused.os && (n->method == CM2_TOEPLITZ_FUSED || n->auto_method),
              "%s needs a Toeplitz operator built with CM2_TOEPLITZ_FUSED or CM2_TOEPLITZ_AUTO", who);
    CM2_CHECK(tiles->nt == n->nt, "noise operator has %lld samples, tile plan %lld",
              (long long)n->nt, (long long)tiles->nt);
    return 0;
}

static cm2::OsPlanView plan_view(const cm2_tiles *tiles)
{
    cm2::OsPlanView pv;
    pv.d_idx = tiles->d_tb_dst;
    pv.d_tile_off = tiles->d_tile_off;
    pv.plan_id = tiles->plan_id;
    pv.ntiles = tiles->ntiles;
    pv.nvalid = tiles->nvalid;
    return pv;
}

extern "C" int cm2_noise_prepare_tiles(cm2_noise *n, const cm2_tiles *tiles, void *stream_)
{
    CM2_CHECK(n && tiles, "cm2_noise_prepare_tiles: NULL argument");
    if (int rc = noise_tiles_ready(n, tiles, "cm2_noise_prepare_tiles", stream_)) return rc;
    return cm2::fused_os_prepare_indexed(n->fused.os, plan_view(tiles), as_stream(stream_));
}

extern "C" int cm2_noise_apply_tiles(cm2_noise *n, const cm2_tiles *tiles, const double *d_in_tb,
                                     double *d_out_tb, void *stream_)
{
    CM2_CHECK(n && tiles && d_in_tb && d_out_tb, "cm2_noise_apply_tiles: NULL argument");
    CM2_CHECK(d_in_tb != d_out_tb, "cm2_noise_apply_tiles: in-place application is not supported");
    if (int rc = noise_tiles_ready(n, tiles, "cm2_noise_apply_tiles", stream_)) return rc;
    return cm2::fused_os_apply_indexed(n->fused.os, plan_view(tiles), d_in_tb, d_out_tb, as_stream(stream_));
}

// One call for the whole tile-order chain y = P^T N^-1 P x (SURVEY 8b's fused cm2_PtNP_apply):
// k_P_tiles, the overlap-save kernel on the tile order, the fixed-order (or atomic) P^T -- three
// launches on `stream`, no allocation when the plan was prepared (cm2_tiles_prepare_pt) and the
// operator has run once on this plan.  d_tb1 / d_tb2: scratch of >= (valid samples) doubles each.
extern "C" int cm2_PtNP_tiles_apply(const cm2_tiles *tiles, cm2_noise *n, const double *d_x,
                                    double *d_y, double *d_tb1, double *d_tb2, void *stream)
{
    CM2_CHECK(tiles && n && d_x && d_y && d_tb1 && d_tb2, "cm2_PtNP_tiles_apply: NULL argument");
    CM2_CHECK(d_tb1 != d_tb2, "cm2_PtNP_tiles_apply: the two scratch buffers must differ");
    if (int rc = cm2_P_tiles_apply(tiles, d_x, d_tb1, stream)) return rc;
    if (int rc = cm2_noise_apply_tiles(n, tiles, d_tb1, d_tb2, stream)) return rc;
    return cm2_Pt_tiles_apply(tiles, d_tb2, d_y, stream);
}
