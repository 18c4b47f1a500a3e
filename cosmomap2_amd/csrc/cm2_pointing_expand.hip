// cm2_pointing_expand.hip -- boresight quaternions + detector offsets -> HEALPix pixel and (cos 2phi, sin 2phi)
// per detector sample, written straight into the arrays that P, P^T, the tile plan and the gap index read.
//
// Quaternions are (x, y, z, w), scalar last, Hamilton product.  Per detector k and time sample i, every operation
// in IEEE double in the order written (this unit is compiled with -ffp-contract=off):
//
//   q  = (q_frame q_bore[i]) q_det[k]              the product in brackets once per time sample; without a frame
//                                                   it is q_bore[i] itself
//        (p q).x = ((pw qx + px qw) + py qz) - pz qy    (p q).y = ((pw qy - px qz) + py qw) + pz qx
//        (p q).z = ((pw qz + px qy) - py qx) + pz qw    (p q).w = ((pw qw - px qx) - py qy) - pz qz
//   n2 = ((xx + yy) + zz) + ww,  r = 1 / n2        (xx = x x, ...): the one normalisation
//   d  = R(q) z^ = ((2 (x z + w y)) r, (2 (y z - w x)) r, ((ww + zz) - (xx + yy)) r)      the line of sight
//   o  = R(q) x^ = (((ww + xx) - (yy + zz)) r, (2 (x y + w z)) r, (2 (x z - w y)) r)      the sensitive direction
//   s2 = dx dx + dy dy
//   a  = (ox (dz dx) + oy (dz dy)) - oz s2         o . (south of the local meridian) sin(theta)
//   b  = oy dx - ox dy                             o . (east) sin(theta);  s2 == 0: a = ox dz, b = oy (longitude 0)
//   den = a a + b b,  cos 2psi = (a a - b b) / den,  sin 2psi = (2 (a b)) / den;  den == 0: (1, 0)
//   with a plate angle chi[i]: (c4, s4) = sincos(4 chi[i]) once per time sample,
//        cos 2phi = c2 c4 - s2 s4,  sin 2phi = s2 c4 + c2 s4;  without: phi = psi.
//
//   pixel (Gorski et al. 2005), nside a power of two <= 8192:
//   za = |dz|,  t = atan2(dy, dx) (2/pi);  t < 0: t += 4;  t >= 4: t -= 4
//   za <= 2/3:   t1 = nside (0.5 + t), t2 = (nside dz) 0.75, jp = floor(t1 - t2), jm = floor(t1 + t2)
//        RING    ir = nside + 1 + jp - jm, kshift = 1 - (ir & 1), ip = ((jp + jm - nside + kshift + 1) / 2) mod 4 nside,
//                pix = 2 nside (nside - 1) + (ir - 1) 4 nside + ip
//        NESTED  ifp = jp / nside, ifm = jm / nside, face = ifp == ifm ? ifp | 4 : ifp < ifm ? ifp : ifm + 8,
//                ix = jm mod nside, iy = nside - (jp mod nside) - 1
//   else:        tmp = za <= 0.99 ? nside sqrt(3 (1 - za)) : (nside sqrt(s2)) sqrt(3 / (1 + za))
//                ntt = min(3, floor(t)), tp = t - ntt, jp = floor(tp tmp), jm = floor((1 - tp) tmp)
//        RING    ir = jp + jm + 1, ip = floor(t ir) mod 4 ir, pix = dz > 0 ? 2 ir (ir - 1) + ip
//                                                                         : 12 nside^2 - 2 ir (ir + 1) + ip
//        NESTED  jp, jm clamped to nside - 1; dz >= 0: face = ntt, ix = nside - jm - 1, iy = nside - jp - 1;
//                else face = ntt + 8, ix = jp, iy = jm
//        NESTED  pix = face nside^2 + (bits of ix at even, of iy at odd positions): shifts and masks, no table.
//
//   flagged: flags[i] != 0, or n2 is not a normal positive finite number (a boresight component that is not finite
//   makes it NaN or infinite, a zero boresight quaternion makes it 0): pix = -1, cos = 1, sin = 0.
//
// k_pexp<NEST, ANGLES>: one thread per time sample, blockIdx.y over chunks of kDetChunk detectors.  The thread loads its
// 32-byte boresight quaternion with two 16-byte loads, forms q_frame q_bore and sincos(4 chi) once and loops over
// the chunk; the detector quaternion of an iteration is the same for the whole wave and is read from the const
// table (scalar loads).  Consecutive lanes store consecutive samples of one detector row: per wave and detector
// 256 B of pix, 512 B of cos and of sin.  DESIGN.md 8.7 has the register figures that chose the chunk and the bounds.
#include "cm2_common.h"

#include <cfloat>
#include <cmath>

using namespace cm2;

namespace {

constexpr int kDetChunk = 8;                 // detectors per thread (tests/test_gpu_pointing_expand.py: D)
constexpr double kInvHalfPi = 0.63661977236758134308;
constexpr double kTwoThird = 2.0 / 3.0;

struct Quat { double x, y, z, w; };

__host__ __device__ __forceinline__ Quat qmul(const Quat &p, const Quat &q)
{
    Quat r;
    r.x = ((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y;
    r.y = ((p.w * q.y - p.x * q.z) + p.y * q.w) + p.z * q.x;
    r.z = ((p.w * q.z + p.x * q.y) - p.y * q.x) + p.z * q.w;
    r.w = ((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z;
    return r;
}

__host__ __device__ __forceinline__ bool unitable(const Quat &q)
{
    const double n2 = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    return n2 >= DBL_MIN && n2 < INFINITY;
}

// bits of v (< 2^16) moved to the even positions
__device__ __forceinline__ uint32_t spread_bits(uint32_t v)
{
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

template <bool NEST>
__device__ __forceinline__ int32_t healpix_pixel(double dx, double dy, double dz, double s2, int32_t nside,
                                                 int order)
{
    const double za = fabs(dz), fn = (double)nside;
    double t = atan2(dy, dx) * kInvHalfPi;
    if (t < 0.0) t += 4.0;
    if (t >= 4.0) t -= 4.0;
    int32_t pix;
    if (za <= kTwoThird) {
        const double t1 = fn * (0.5 + t), t2 = (fn * dz) * 0.75;
        const int32_t jp = (int32_t)floor(t1 - t2), jm = (int32_t)floor(t1 + t2);
        if (NEST) {
            const int32_t ifp = jp >> order, ifm = jm >> order;
            const int32_t face = ifp == ifm ? (ifp | 4) : (ifp < ifm ? ifp : ifm + 8);
            const int32_t ix = jm & (nside - 1), iy = nside - (jp & (nside - 1)) - 1;
            pix = (face << (2 * order)) + (int32_t)(spread_bits((uint32_t)ix) | (spread_bits((uint32_t)iy) << 1));
        } else {
            const int32_t ir = nside + 1 + jp - jm, kshift = 1 - (ir & 1), nl4 = 4 * nside;
            int32_t ip = (jp + jm - nside + kshift + 1) / 2;
            ip &= nl4 - 1;
            pix = 2 * nside * (nside - 1) + (ir - 1) * nl4 + ip;
        }
    } else {
        const double tmp = za <= 0.99 ? fn * sqrt(3.0 * (1.0 - za)) : (fn * sqrt(s2)) * sqrt(3.0 / (1.0 + za));
        const int32_t ntt = min(3, (int32_t)floor(t));
        const double tp = t - (double)ntt;
        int32_t jp = (int32_t)floor(tp * tmp), jm = (int32_t)floor((1.0 - tp) * tmp);
        if (NEST) {
            jp = min(jp, nside - 1);
            jm = min(jm, nside - 1);
            const int32_t face = dz >= 0.0 ? ntt : ntt + 8;
            const int32_t ix = dz >= 0.0 ? nside - jm - 1 : jp, iy = dz >= 0.0 ? nside - jp - 1 : jm;
            pix = (face << (2 * order)) + (int32_t)(spread_bits((uint32_t)ix) | (spread_bits((uint32_t)iy) << 1));
        } else {
            const int32_t ir = jp + jm + 1;
            int32_t ip = (int32_t)floor(t * (double)ir);
            if (ip >= 4 * ir) ip -= 4 * ir;
            pix = dz > 0.0 ? 2 * ir * (ir - 1) + ip : 12 * nside * nside - 2 * ir * (ir + 1) + ip;
        }
    }
    return pix;
}

// ANGLES: 0 pixels only, 1 cos / sin of 2 psi, 2 of 2 (psi + 2 chi)
template <bool NEST, int ANGLES>
__global__ __launch_bounds__(256) void k_pexp(int64_t ns, int ndet, const double2 *__restrict__ bore,
                                               const double *__restrict__ det, Quat frame, int has_frame,
                                               const double *__restrict__ hwp, const uint8_t *__restrict__ flags,
                                               int32_t nside, int order, int32_t *__restrict__ pix,
                                               double *__restrict__ cosv, double *__restrict__ sinv)
{
    constexpr bool POL = ANGLES > 0, HWP = ANGLES == 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const double2 lo = bore[2 * i], hi = bore[2 * i + 1];
    Quat fb = {lo.x, lo.y, hi.x, hi.y};
    if (has_frame) fb = qmul(frame, fb);
    const bool flagged = flags != nullptr && flags[i] != 0;
    double c4 = 1.0, s4 = 0.0;
    if (HWP) sincos(4.0 * hwp[i], &s4, &c4);
    const int k0 = (int)blockIdx.y * kDetChunk, k1 = min(ndet, k0 + kDetChunk);
#pragma unroll 1
    for (int k = k0; k < k1; ++k) {
        const Quat qd = {det[4 * k], det[4 * k + 1], det[4 * k + 2], det[4 * k + 3]};
        const Quat q = qmul(fb, qd);
        const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, ww = q.w * q.w;
        const double n2 = ((xx + yy) + zz) + ww;
        int32_t p = -1;
        double c2 = 1.0, s2p = 0.0;
        if (!flagged && n2 >= DBL_MIN && n2 < INFINITY) {
            const double r = 1.0 / n2;
            const double dx = (2.0 * (q.x * q.z + q.w * q.y)) * r;
            const double dy = (2.0 * (q.y * q.z - q.w * q.x)) * r;
            const double dz = ((ww + zz) - (xx + yy)) * r;
            const double s2 = dx * dx + dy * dy;
            p = healpix_pixel<NEST>(dx, dy, dz, s2, nside, order);
            if (POL) {
                const double ox = ((ww + xx) - (yy + zz)) * r;
                const double oy = (2.0 * (q.x * q.y + q.w * q.z)) * r;
                const double oz = (2.0 * (q.x * q.z - q.w * q.y)) * r;
                double a = (ox * (dz * dx) + oy * (dz * dy)) - oz * s2;
                double b = oy * dx - ox * dy;
                if (s2 == 0.0) {
                    a = ox * dz;
                    b = oy;
                }
                const double aa = a * a, bb = b * b, den = aa + bb;
                if (den > 0.0) {
                    c2 = (aa - bb) / den;
                    s2p = (2.0 * (a * b)) / den;
                }
                if (HWP) {
                    const double c = c2 * c4 - s2p * s4, s = s2p * c4 + c2 * s4;
                    c2 = c;
                    s2p = s;
                }
            }
        }
        const int64_t at = (int64_t)k * ns + i;
        pix[at] = p;
        if (POL) {
            cosv[at] = c2;
            sinv[at] = s2p;
        }
    }
}

// one workgroup: status = 1 + the first detector whose quaternion cannot be normalised, 0 when all can
__global__ __launch_bounds__(256) void k_pexp_check_det(int ndet, const double *__restrict__ det,
                                                         int *__restrict__ status)
{
    __shared__ int first;
    if (threadIdx.x == 0) first = ndet;
    __syncthreads();
    int mine = ndet;
    for (int k = threadIdx.x; k < ndet; k += blockDim.x) {
        const Quat q = {det[4 * k], det[4 * k + 1], det[4 * k + 2], det[4 * k + 3]};
        if (!unitable(q) && k < mine) mine = k;
    }
    if (mine < ndet) atomicMin(&first, mine);
    __syncthreads();
    if (threadIdx.x == 0) status[0] = first < ndet ? first + 1 : 0;
}

}  // namespace

extern "C" int cm2_pointing_expand(int64_t ns, int ndet, const double *d_bore, const double *d_detquat,
                                   const double *h_frame, const double *d_hwp, const uint8_t *d_flags, int64_t nside,
                                   int nest, int32_t *d_pix, double *d_cos, double *d_sin, void *stream_)
{
    const char *who = "cm2_pointing_expand";
    CM2_CHECK(ns >= 0, "%s: ns=%lld < 0", who, (long long)ns);
    CM2_CHECK(ndet >= 1, "%s: ndet=%d < 1", who, ndet);
    CM2_CHECK((ndet + kDetChunk - 1) / kDetChunk <= 65535, "%s: ndet=%d is more than %d detectors", who, ndet,
              65535 * kDetChunk);
    CM2_CHECK(nside >= 1 && nside <= 8192 && (nside & (nside - 1)) == 0,
              "%s: nside=%lld is not a power of two in [1, 8192]", who, (long long)nside);
    CM2_CHECK((d_cos == nullptr) == (d_sin == nullptr), "%s: exactly one of d_cos / d_sin is given", who);
    CM2_CHECK(d_detquat && d_pix && (d_bore || ns == 0), "%s: NULL argument", who);
    CM2_CHECK((reinterpret_cast<uintptr_t>(d_bore) & 15) == 0, "%s: d_bore is not 16-byte aligned", who);
    CM2_CHECK((ns + kBlock - 1) / kBlock <= 0x7FFFFFFFLL, "%s: ns=%lld is too long for one launch", who,
              (long long)ns);
    Quat frame = {0.0, 0.0, 0.0, 1.0};
    if (h_frame) {
        frame = Quat{h_frame[0], h_frame[1], h_frame[2], h_frame[3]};
        CM2_CHECK(unitable(frame), "%s: the frame quaternion (%g, %g, %g, %g) cannot be normalised", who, frame.x,
                  frame.y, frame.z, frame.w);
    }
    hipStream_t stream = as_stream(stream_);
    DevTemp<int> status;
    CM2_HIP(status.alloc(1));
    k_pexp_check_det<<<1, kBlock, 0, stream>>>(ndet, d_detquat, status);
    CM2_LAUNCH_OK();
    int h_status = 0;
    CM2_HIP(cm2::read_back(&h_status, status, sizeof(h_status), stream));
    CM2_CHECK(h_status == 0, "%s: the quaternion of detector %d cannot be normalised", who, h_status - 1);
    if (ns == 0) return 0;
    int order = 0;
    while ((int64_t(1) << order) < nside) ++order;
    const dim3 grid((unsigned)((ns + kBlock - 1) / kBlock), (unsigned)((ndet + kDetChunk - 1) / kDetChunk));
    const double2 *bore = reinterpret_cast<const double2 *>(d_bore);
    const int has_frame = h_frame != nullptr;
    auto go = [&](auto kernel) {
        kernel<<<grid, kBlock, 0, stream>>>(ns, ndet, bore, d_detquat, frame, has_frame, d_hwp, d_flags, (int32_t)nside,
                                            order, d_pix, d_cos, d_sin);
    };
    const int angles = !d_cos ? 0 : d_hwp ? 2 : 1;
    switch (angles + (nest ? 3 : 0)) {
    case 0: go(k_pexp<false, 0>); break;
    case 1: go(k_pexp<false, 1>); break;
    case 2: go(k_pexp<false, 2>); break;
    case 3: go(k_pexp<true, 0>); break;
    case 4: go(k_pexp<true, 1>); break;
    default: go(k_pexp<true, 2>); break;
    }
    CM2_LAUNCH_OK();
    return 0;
}
