// cm2_noise_sim.hip -- noise time streams with a given spectrum, drawn on the GPU.
//
// The reference has no simulator (its tests draw noise with NumPy on the host).  Three steps, the inverse
// of cm2_noise_model.hip's time stream -> PSD -> band:
//
//   cm2_rng_fill             white noise.  The stream of (seed, realization, block) is Philox4x64-10 with key
//                            [seed, realization]; output block j = 0, 1, ... (four uint64) is the Philox function
//                            of the counter [j + 1, block, 0, 0] -- numpy.random.Philox(key=[seed, realization],
//                            counter=[0, block, 0, 0]).random_raw(), bit for bit.  uniform u = (raw >> 11) 2^-53
//                            (= numpy.random.Generator(...).random()); normal = Box-Muller over the pairs
//                            (u0, u1), (u2, u3) of a counter block: r = sqrt(-2 log(1 - u_a)),
//                            z_a = r cospi(2 u_b), z_b = r sinpi(2 u_b).  Sample i of a stream depends on
//                            (seed, realization, block, i) alone: any [first, first + n) can be asked for.
//   (cm2_noise_filter_from_psd, in cm2_noise_model.hip: PSD -> colouring band g)
//   cm2_noise_sim_draw       block b of n_b samples: w = n_b + 2 (lambda - 1) normals of the stream
//                            (seed, realization, first_block + b), y_i = sum_{|j| < lambda} g_|j| w_{i + lambda-1 + j}:
//                            the VALID part of the convolution, so every sample of the block has the
//                            autocovariance g * g (a zero-boundary Toeplitz product on n_b samples would lose
//                            variance in the first and last lambda samples).  The padded white stream goes through
//                            a cm2_noise Toeplitz operator built on the padded block sizes (method AUTO); its
//                            interior rows are the valid convolution, and k_sim_interior compacts them.
#include "cm2_common.h"

#include <cmath>
#include <vector>

using namespace cm2;

namespace {

constexpr uint64_t kPhiloxM0 = 0xD2E7470EE14C6C93ULL, kPhiloxM1 = 0xCA5A826395121157ULL;
constexpr uint64_t kPhiloxW0 = 0x9E3779B97F4A7C15ULL, kPhiloxW1 = 0xBB67AE8584CAA73BULL;
constexpr int64_t kMaxGridY = 65535;

// Philox4x64-10 of the counter [c0, c1, 0, 0] under the key [k0, k1]
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t k1, uint64_t (&r)[4])
{
    uint64_t c2 = 0, c3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t hi0 = __umul64hi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint64_t hi1 = __umul64hi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ double to_uniform(uint64_t raw) { return (double)(raw >> 11) * 0x1.0p-53; }

// r = sqrt(-2 log(1 - ua)) (1 - ua is exact and lies in (0, 1]), za = r cospi(2 ub), zb = r sinpi(2 ub)
__device__ __forceinline__ void box_muller(double ua, double ub, double &za, double &zb)
{
    const double r = sqrt(-2.0 * log(1.0 - ua));
    double s, c;
    sincospi(2.0 * ub, &s, &c);
    za = r * c;
    zb = r * s;
}

// One thread per counter block (four samples, 32 bytes: two 16-byte stores where the address allows, single
// masked stores in the counter blocks cut by `first` and `first + n` and in streams that start on an odd double),
// grid-stride over the counter blocks of a stream.  blockIdx.y counts streams:
//   poff == nullptr   the one stream (seed, realization, block0), samples [first, first + n) to out[0 .. n)
//   poff != nullptr   stream (seed, realization, block0 + blockIdx.y), samples [0, poff[y+1] - poff[y]) to
//                     out[poff[y] ...)                                     (the padded blocks of a simulator)
template <int KIND>
__global__ __launch_bounds__(256) void k_rng_fill(uint64_t seed, uint64_t realization, uint64_t block0,
                                                   const int64_t *__restrict__ poff, int64_t first, int64_t n,
                                                   double *__restrict__ out)
{
    const uint64_t blk = block0 + (uint64_t)blockIdx.y;
    double *o = out;
    int64_t len = n;
    if (poff) {
        o = out + poff[blockIdx.y];
        len = poff[blockIdx.y + 1] - poff[blockIdx.y];
    }
    const int64_t j0 = first >> 2, j1 = (first + len + 3) >> 2;          // counter blocks [j0, j1)
    const bool even = ((((uintptr_t)o >> 3) - (uint64_t)first) & 1) == 0;   // o + (4 j - first) is 16-byte aligned
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += stride) {
        uint64_t r[4];
        philox4x64_10((uint64_t)j + 1, blk, seed, realization, r);
        double z0 = to_uniform(r[0]), z1 = to_uniform(r[1]), z2 = to_uniform(r[2]), z3 = to_uniform(r[3]);
        if (KIND == 1) {
            box_muller(z0, z1, z0, z1);
            box_muller(z2, z3, z2, z3);
        }
        const int64_t i = 4 * j - first;                                 // of z0, relative to o
        if (even && i >= 0 && i + 4 <= len) {
            double2 *p = reinterpret_cast<double2 *>(o + i);
            p[0] = make_double2(z0, z1);
            p[1] = make_double2(z2, z3);
        } else {
            if (i >= 0 && i < len) o[i] = z0;
            if (i + 1 >= 0 && i + 1 < len) o[i + 1] = z1;
            if (i + 2 >= 0 && i + 2 < len) o[i + 2] = z2;
            if (i + 3 < len) o[i + 3] = z3;
        }
    }
}

// out[off[b] + i] = (add ? out[off[b] + i] : 0) + scale * ypad[poff[b] + halo + i], i < off[b+1] - off[b];
// b = blockIdx.y, grid-stride over the block.  16-byte accesses when source and destination sit on the same
// side of a 16-byte boundary (one leading and one trailing double are then moved alone), 8-byte ones otherwise.
__global__ __launch_bounds__(256) void k_sim_interior(const int64_t *__restrict__ off, const int64_t *__restrict__ poff,
                                                       int64_t halo, double scale, int add,
                                                       const double *__restrict__ ypad, double *__restrict__ out)
{
    const int64_t b = blockIdx.y;
    const double *src = ypad + poff[b] + halo;
    double *dst = out + off[b];
    const int64_t len = off[b + 1] - off[b];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 8) == 0) {
        const int64_t head = ((uintptr_t)dst & 8) ? 1 : 0;              // (len >= 1)
        const int64_t npair = (len - head) >> 1;
        const double2 *s2 = reinterpret_cast<const double2 *>(src + head);
        double2 *d2 = reinterpret_cast<double2 *>(dst + head);
        for (int64_t p = t; p < npair; p += stride) {
            const double2 v = s2[p];
            double2 o = add ? d2[p] : make_double2(0.0, 0.0);
            o.x = o.x + scale * v.x;
            o.y = o.y + scale * v.y;
            d2[p] = o;
        }
        if (t == 0) {
            if (head) dst[0] = (add ? dst[0] : 0.0) + scale * src[0];
            const int64_t last = head + 2 * npair;
            if (last < len) dst[last] = (add ? dst[last] : 0.0) + scale * src[last];
        }
    } else {
        for (int64_t i = t; i < len; i += stride) dst[i] = (add ? dst[i] : 0.0) + scale * src[i];
    }
}

// grid.x of a launch whose grid.y counts `ny` streams of at most `items` work items each
int grid_x_for(int64_t items, int64_t ny)
{
    int64_t cap = (int64_t)kNumCU * 8 / (ny < 1 ? 1 : ny);
    if (cap < 1) cap = 1;
    return grid_for(items, kBlock, (int)cap);
}

int rng_launch(int kind, uint64_t seed, uint64_t realization, uint64_t block0, const int64_t *d_poff, int64_t ny,
               int64_t max_len, int64_t first, int64_t n, double *d_out, hipStream_t stream)
{
    const dim3 grid((unsigned)grid_x_for((max_len + 6) / 4, ny), (unsigned)ny);
    if (kind == 1)
        k_rng_fill<1><<<grid, kBlock, 0, stream>>>(seed, realization, block0, d_poff, first, n, d_out);
    else
        k_rng_fill<0><<<grid, kBlock, 0, stream>>>(seed, realization, block0, d_poff, first, n, d_out);
    CM2_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" int cm2_rng_fill(int kind, uint64_t seed, uint64_t realization, uint64_t block, int64_t first, int64_t n,
                            double *d_out, void *stream_)
{
    CM2_CHECK(kind == 0 || kind == 1, "cm2_rng_fill: kind=%d (0 = uniform, 1 = normal)", kind);
    CM2_CHECK(first >= 0 && n >= 0, "cm2_rng_fill: first=%lld, n=%lld must not be negative", (long long)first,
              (long long)n);
    CM2_CHECK(first <= INT64_MAX - 8 - n, "cm2_rng_fill: first + n = %lld + %lld does not fit 63 bits",
              (long long)first, (long long)n);
    if (n == 0) return 0;
    CM2_CHECK(d_out, "cm2_rng_fill: NULL argument");
    return rng_launch(kind, seed, realization, block, nullptr, 1, n, first, n, d_out, as_stream(stream_));
}

struct cm2_noise_sim {
    int64_t nb = 0, lambda = 0, halo = 0, nt = 0, npad = 0, max_pad = 0, max_len = 0;
    uint64_t seed = 0, first_block = 0;
    cm2_noise *op = nullptr;         // Toeplitz operator with bands g on the padded blocks
    int64_t *d_off = nullptr;        // [nb+1] block offsets of the output
    int64_t *d_poff = nullptr;       // [nb+1] block offsets of the padded buffers
    double *d_w = nullptr;           // [npad] white noise
    double *d_y = nullptr;           // [npad] the operator applied to it
};

extern "C" int cm2_noise_sim_destroy(cm2_noise_sim *s)
{
    if (!s) return 0;
    if (s->op) cm2_noise_destroy(s->op);
    void *ptrs[] = {s->d_off, s->d_poff, s->d_w, s->d_y};
    for (void *q : ptrs)
        if (q) (void)cm2::dev_free(q);
    delete s;
    return 0;
}

static int sim_build(cm2_noise_sim *s, const double *h_bands, const int64_t *h_sizes, hipStream_t stream)
{
    const int64_t nb = s->nb;
    std::vector<int64_t> off(nb + 1, 0), poff(nb + 1, 0), psizes(nb);
    for (int64_t b = 0; b < nb; ++b) {
        CM2_CHECK(h_sizes[b] > 0, "cm2_noise_sim_create: block %lld has non-positive size %lld", (long long)b,
                  (long long)h_sizes[b]);
        psizes[b] = h_sizes[b] + 2 * s->halo;
        off[b + 1] = off[b] + h_sizes[b];
        poff[b + 1] = poff[b] + psizes[b];
        if (psizes[b] > s->max_pad) s->max_pad = psizes[b];
        if (h_sizes[b] > s->max_len) s->max_len = h_sizes[b];
    }
    s->nt = off[nb];
    s->npad = poff[nb];
    if (int rc = cm2_noise_create_toeplitz(&s->op, h_bands, s->lambda, psizes.data(), nb, CM2_TOEPLITZ_AUTO, stream))
        return rc;
    CM2_HIP(cm2::dev_malloc(&s->d_off, sizeof(int64_t) * (nb + 1)));
    CM2_HIP(cm2::dev_malloc(&s->d_poff, sizeof(int64_t) * (nb + 1)));
    CM2_HIP(cm2::upload(s->d_off, off.data(), sizeof(int64_t) * (nb + 1), stream));
    CM2_HIP(cm2::upload(s->d_poff, poff.data(), sizeof(int64_t) * (nb + 1), stream));
    CM2_HIP(cm2::dev_malloc(&s->d_w, sizeof(double) * s->npad));
    CM2_HIP(cm2::dev_malloc(&s->d_y, sizeof(double) * s->npad));
    return 0;
}

extern "C" int cm2_noise_sim_create(cm2_noise_sim **out, const double *h_bands, int64_t lambda, const int64_t *h_sizes,
                                    int64_t nblocks, uint64_t seed, uint64_t first_block, void *stream_)
{
    CM2_CHECK(out && h_bands && h_sizes, "cm2_noise_sim_create: NULL argument");
    *out = nullptr;
    CM2_CHECK(lambda >= 1, "cm2_noise_sim_create: band length lambda=%lld < 1", (long long)lambda);
    CM2_CHECK(nblocks >= 1, "cm2_noise_sim_create: nblocks=%lld < 1", (long long)nblocks);
    CM2_CHECK(first_block <= UINT64_MAX - (uint64_t)nblocks,
              "cm2_noise_sim_create: first_block + nblocks does not fit 64 bits");
    cm2_noise_sim *s = new cm2_noise_sim();
    s->nb = nblocks;
    s->lambda = lambda;
    s->halo = lambda - 1;
    s->seed = seed;
    s->first_block = first_block;
    if (int rc = sim_build(s, h_bands, h_sizes, as_stream(stream_))) {
        cm2_noise_sim_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

extern "C" int cm2_noise_sim_info(const cm2_noise_sim *s, int64_t *h_info)
{
    CM2_CHECK(s && h_info, "cm2_noise_sim_info: NULL argument");
    int64_t op[6] = {0, 0, 0, 0, 0, 0};
    if (int rc = cm2_noise_info(s->op, op)) return rc;
    h_info[0] = s->nt;
    h_info[1] = s->nb;
    h_info[2] = s->lambda;
    h_info[3] = s->npad;
    h_info[4] = op[3];                                    // CM2_TOEPLITZ_* of the operator
    h_info[5] = op[4];                                    // its FFT length (0: direct sum)
    h_info[6] = (int64_t)(2 * sizeof(double) * s->npad);  // bytes of the two padded buffers
    return 0;
}

extern "C" int cm2_noise_sim_draw(cm2_noise_sim *s, uint64_t realization, double scale, int add, double *d_out,
                                  void *stream_)
{
    CM2_CHECK(s && d_out, "cm2_noise_sim_draw: NULL argument");
    CM2_CHECK(add == 0 || add == 1, "cm2_noise_sim_draw: add=%d (0 = overwrite, 1 = accumulate)", add);
    CM2_CHECK(std::isfinite(scale), "cm2_noise_sim_draw: scale=%g is not finite", scale);
    hipStream_t stream = as_stream(stream_);
    for (int64_t b0 = 0; b0 < s->nb; b0 += kMaxGridY) {
        const int64_t ny = s->nb - b0 < kMaxGridY ? s->nb - b0 : kMaxGridY;
        if (int rc = rng_launch(1, s->seed, realization, s->first_block + (uint64_t)b0, s->d_poff + b0, ny, s->max_pad,
                                0, 0, s->d_w, stream))
            return rc;
    }
    if (int rc = cm2_noise_apply(s->op, s->d_w, s->d_y, stream)) return rc;
    for (int64_t b0 = 0; b0 < s->nb; b0 += kMaxGridY) {
        const int64_t ny = s->nb - b0 < kMaxGridY ? s->nb - b0 : kMaxGridY;
        const dim3 grid((unsigned)grid_x_for((s->max_len + 1) / 2, ny), (unsigned)ny);
        k_sim_interior<<<grid, kBlock, 0, stream>>>(s->d_off + b0, s->d_poff + b0, s->halo, scale, add, s->d_y, d_out);
        CM2_LAUNCH_OK();
    }
    return 0;
}
