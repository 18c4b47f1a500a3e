// cm2_fourier.hip -- the Fourier filter of the time streams, see include/cosmomap2.h (f2j): per noise block the trend
// through the means of its ends is taken out, the block is padded with zeros to a 7-smooth even length L, transformed
// (rocFFT, cm2_rocfft.h), multiplied by H_b(f) -- time-constant (de)convolution, Butterworth low- and high-pass,
// cos^2 notches and a tabulated response -- transformed back, and Re H_b(0) times the trend is put back.
// cm2_fourier_policy.h has the accepted arguments, the lengths, the groups of blocks of one length and the rows of a
// batch; cm2_stream.h the blocks and the checks every stage shares.
//
// Per length and batch of rows (one row = one block of that length; the rows of a short last batch are zero):
//   k_fourier_pack      4096-sample segments of a row: x - l, the zero padding; 16-byte loads where the block starts on
//                       a 16-byte boundary, 16-byte stores always (L is even); a non-finite sample sets the block's
//                       word by an integer atomic OR
//   rocFFT forward      [batch][L] doubles -> [batch][L/2 + 1] double2
//   k_fourier_response  one thread per (row, bin): H_b(f_k) from the parameters (kernel arguments, tau_b and the two
//                       table entries around f_k), multiplied in place.  No array of H is ever stored.
//   rocFFT inverse      back into the rows
//   k_fourier_unpack    y / L + Re H_b(0) l, or the quiet NaN for a bad block
// k_fourier_ends runs once per apply before them, one workgroup per block of the stream: the means a, b of its ends in
// the stated order and the block's word (1 when an end sample is not finite, else 0: the word needs no memset).  The
// unit is compiled with -ffp-contract=off: every operation named in the header is rounded on its own.  No
// floating-point atomic: the same bits run to run.
#include <memory>
#include <vector>

#include "cm2_fourier_policy.h"
#include "cm2_rocfft.h"
#include "cm2_stream.h"

using namespace cm2;
using namespace cm2::stream;
namespace fr = cm2::fourier;

namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kHalfPi = 1.5707963267948966192313216916398;
constexpr unsigned long long kQuietNaN = 0x7FF8000000000000ull;

// the rows of a batch: row r is block rows[first + r] of the stream while first + r < count, else a zero row
struct Rows {
    const int32_t *rows;
    int64_t first, count, L;
};

__device__ __forceinline__ double butterworth(double ratio, int order)
{
    const double r = ratio * ratio;
    double pw = r;
    for (int i = 1; i < order; ++i) pw = pw * r;
    return 1.0 / sqrt(1.0 + pw);
}

// H_b at bin k of a transform of length L (rule 4 of the definition, in its operation order); row: the block's table
__device__ __forceinline__ double2 response_at(const fr::Response &r, double tau, const double *__restrict__ row,
                                               int64_t k, int64_t L)
{
    const double f = ((double)k * r.fs) / (double)L;
    double tre = 1.0, tim = 0.0;
    if (tau != 0.0) {
        const double u = (kTwoPi * f) * tau;
        if (r.mode == fr::kDeconvolve) {
            tim = u;
        } else {
            const double den = 1.0 + u * u;
            tre = 1.0 / den;
            tim = -u / den;
        }
    }
    double g = 1.0;
    if (r.f_lp > 0.0) g = g * butterworth(f / r.f_lp, r.p);
    if (r.f_hp > 0.0) g = g * (k == 0 ? 0.0 : butterworth(r.f_hp / f, r.q));
    for (int j = 0; j < r.nnotch; ++j) {
        const double a = fabs(f - r.notch[2 * j]) / r.notch[2 * j + 1];
        if (a < 1.0) {
            const double s = sin(kHalfPi * a);
            g = g * (s * s);
        }
    }
    double hre = tre * g, him = tim * g;
    if (r.table_kind != fr::kNoTable) {
        const double s = (f / (0.5 * r.fs)) * (double)(r.Rn - 1);
        int64_t i0 = (int64_t)s;
        if (i0 > r.Rn - 2) i0 = r.Rn - 2;
        const double t = s - (double)i0;
        if (r.table_kind == fr::kRealTable) {
            const double v = row[i0] + t * (row[i0 + 1] - row[i0]);
            hre = hre * v;
            him = him * v;
        } else {
            const double2 v0 = reinterpret_cast<const double2 *>(row)[i0];
            const double2 v1 = reinterpret_cast<const double2 *>(row)[i0 + 1];
            const double vre = v0.x + t * (v1.x - v0.x), vim = v0.y + t * (v1.y - v0.y);
            const double re = hre * vre - him * vim;
            him = hre * vim + him * vre;
            hre = re;
        }
    }
    if (r.conjugate) him = -him;
    if (k == 0 || 2 * k == L) him = 0.0;
    return make_double2(hre, him);
}

__device__ __forceinline__ const double *table_row(const fr::Response &r, const double *table, int64_t b)
{
    if (r.table_kind == fr::kNoTable) return nullptr;
    return table + (r.table_per_block ? b : 0) * r.Rn * (r.table_kind == fr::kComplexTable ? 2 : 1);
}

// the trend of a block of n samples at sample i
__device__ __forceinline__ double trend(double a, double b, int64_t i, int64_t n)
{
    return n == 1 ? a : a + ((b - a) * (double)i) / (double)(n - 1);
}

__global__ __launch_bounds__(fr::kThreads) void k_fourier_ends(const int64_t *__restrict__ off,
                                                               const double *__restrict__ d, int detrend, int end_mean,
                                                               double *__restrict__ ab, unsigned int *__restrict__ bad)
{
    __shared__ double lds4[4];
    const int64_t b = blockIdx.x, lo = off[b], n = off[b + 1] - lo;
    const int m = n < end_mean ? (int)n : end_mean;
    double sa = 0.0, sb = 0.0;
    int nonfinite = 0;
    if (detrend) {
        for (int i = threadIdx.x; i < m; i += fr::kThreads) {
            const double x = d[lo + i], y = d[lo + n - m + i];
            sa = sa + x;
            sb = sb + y;
            nonfinite |= !finite_bits(x) || !finite_bits(y);
        }
    }
    sa = block_sum_256(sa, lds4);
    sb = block_sum_256(sb, lds4);
    nonfinite = __syncthreads_or(nonfinite);
    if (threadIdx.x == 0) {
        ab[2 * b] = sa / (double)m;
        ab[2 * b + 1] = sb / (double)m;
        bad[b] = nonfinite ? 1u : 0u;
    }
}

__global__ __launch_bounds__(fr::kThreads) void k_fourier_pack(Rows rw, int64_t nseg, const int64_t *__restrict__ off,
                                                               const double *__restrict__ d, const double *__restrict__ ab,
                                                               int detrend, unsigned int *__restrict__ bad,
                                                               double *__restrict__ X)
{
    const int64_t r = (int64_t)blockIdx.x / nseg, seg = (int64_t)blockIdx.x - r * nseg;
    const bool real = rw.first + r < rw.count;
    const int64_t b = real ? rw.rows[rw.first + r] : 0;
    const int64_t lo = real ? off[b] : 0, n = real ? off[b + 1] - lo : 0;
    const double a = real && detrend ? ab[2 * b] : 0.0, e = real && detrend ? ab[2 * b + 1] : 0.0;
    const bool wide = ((reinterpret_cast<uintptr_t>(d) >> 3) + (uintptr_t)lo) % 2 == 0;
    double2 *row = reinterpret_cast<double2 *>(X + r * rw.L);
    int nonfinite = 0;
    for (int p = threadIdx.x; p < fr::kSegment / 2; p += fr::kThreads) {
        const int64_t i = seg * fr::kSegment + 2 * (int64_t)p;
        if (i >= rw.L) break;
        double2 x = make_double2(0.0, 0.0);
        if (i + 1 < n) {
            if (wide) {
                x = *reinterpret_cast<const double2 *>(d + lo + i);
            } else {
                x.x = d[lo + i];
                x.y = d[lo + i + 1];
            }
            nonfinite |= !finite_bits(x.x) || !finite_bits(x.y);
            if (detrend) {
                x.x = x.x - trend(a, e, i, n);
                x.y = x.y - trend(a, e, i + 1, n);
            }
        } else if (i < n) {
            x.x = d[lo + i];
            nonfinite |= !finite_bits(x.x);
            if (detrend) x.x = x.x - trend(a, e, i, n);
        }
        row[i / 2] = x;
    }
    if (real) {                                                               // (the same for the whole workgroup)
        nonfinite = __syncthreads_or(nonfinite);
        if (nonfinite && threadIdx.x == 0) atomicOr(&bad[b], 1u);
    }
}

__global__ __launch_bounds__(kBlock) void k_fourier_response(Rows rw, int64_t batch, int64_t nfreq, fr::Response resp,
                                                             const double *__restrict__ tau,
                                                             const double *__restrict__ table, double2 *__restrict__ F)
{
    const int64_t total = batch * nfreq;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t r = idx / nfreq, k = idx - r * nfreq;
        if (rw.first + r >= rw.count) continue;                               // a zero row stays zero
        const int64_t b = rw.rows[rw.first + r];
        const double2 h = response_at(resp, tau ? tau[b] : 0.0, table_row(resp, table, b), k, rw.L);
        const double2 x = F[idx];
        F[idx] = make_double2(x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x);
    }
}

__global__ __launch_bounds__(fr::kThreads) void k_fourier_unpack(Rows rw, int64_t nseg, const int64_t *__restrict__ off,
                                                                 const double *__restrict__ X,
                                                                 const double *__restrict__ ab, int detrend,
                                                                 const unsigned int *__restrict__ bad, fr::Response resp,
                                                                 const double *__restrict__ tau,
                                                                 const double *__restrict__ table, double *__restrict__ out)
{
    __shared__ double h0s;
    const int64_t r = (int64_t)blockIdx.x / nseg, seg = (int64_t)blockIdx.x - r * nseg;
    if (rw.first + r >= rw.count) return;
    const int64_t b = rw.rows[rw.first + r], lo = off[b], n = off[b + 1] - lo;
    if (seg * fr::kSegment >= n) return;                                      // a segment of padding only
    if (threadIdx.x == 0) h0s = detrend ? response_at(resp, tau ? tau[b] : 0.0, table_row(resp, table, b), 0, rw.L).x : 0.0;
    __syncthreads();
    const double h0 = h0s, a = detrend ? ab[2 * b] : 0.0, e = detrend ? ab[2 * b + 1] : 0.0, len = (double)rw.L;
    const bool isbad = bad[b] != 0u;
    const double qnan = __longlong_as_double((long long)kQuietNaN);
    const bool wide = ((reinterpret_cast<uintptr_t>(out) >> 3) + (uintptr_t)lo) % 2 == 0;
    const double2 *row = reinterpret_cast<const double2 *>(X + r * rw.L);
    for (int p = threadIdx.x; p < fr::kSegment / 2; p += fr::kThreads) {
        const int64_t i = seg * fr::kSegment + 2 * (int64_t)p;
        if (i >= n) break;
        const double2 y = row[i / 2];                                         // i + 1 < L: L is even
        double2 v;
        v.x = y.x / len;
        v.y = y.y / len;
        if (detrend) {
            v.x = v.x + h0 * trend(a, e, i, n);
            v.y = v.y + h0 * trend(a, e, i + 1 < n ? i + 1 : i, n);
        }
        if (isbad) v = make_double2(qnan, qnan);
        if (wide && i + 1 < n) {
            *reinterpret_cast<double2 *>(out + lo + i) = v;
        } else {
            out[lo + i] = v.x;
            if (i + 1 < n) out[lo + i + 1] = v.y;
        }
    }
}

// H_b as k_fourier_response evaluates it, for tests and for plotting
__global__ __launch_bounds__(kBlock) void k_fourier_write_response(int64_t b, int64_t L, int64_t nfreq,
                                                                   fr::Response resp, const double *__restrict__ tau,
                                                                   const double *__restrict__ table,
                                                                   double *__restrict__ H)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nfreq; k += (int64_t)gridDim.x * kBlock) {
        const double2 h = response_at(resp, tau ? tau[b] : 0.0, table_row(resp, table, b), k, L);
        H[2 * k] = h.x;                                                       // (d_H need not be 16-byte aligned)
        H[2 * k + 1] = h.y;
    }
}

struct GroupState {
    fr::Group g;
    int64_t row0 = 0;                      // its first entry in d_rows
    RealFft fft;
};

}  // namespace

struct cm2_fourier {
    fr::Launch launch;
    std::vector<std::unique_ptr<GroupState>> groups;
    int64_t *d_off = nullptr;              // [nblocks + 1]
    int32_t *d_rows = nullptr;             // [nblocks] the blocks group after group, ascending in a group
    double *d_tau = nullptr;               // [nblocks], NULL: every tau 0
    double *d_table = nullptr;
    double *d_ab = nullptr;                // [nblocks][2] the end means of the last apply
    unsigned int *d_bad = nullptr;         // [nblocks] the bad-block words of the last apply
    double *d_X = nullptr;                 // the rows, sized for the largest batch
    double2 *d_F = nullptr;                // their transforms
    int64_t row_bytes = 0, plan_bytes = 0;
    bool applied = false;
};

extern "C" int cm2_fourier_destroy(cm2_fourier *h)
{
    if (!h) return 0;
    h->groups.clear();
    dev_release(h->d_off, h->d_rows, h->d_tau, h->d_table, h->d_ab, h->d_bad, h->d_X, h->d_F);
    delete h;
    return 0;
}

namespace {

int fourier_fill(cm2_fourier *h, const int64_t *sizes, const double *tau, const double *table, int64_t max_work_bytes,
                 hipStream_t st)
{
    const char *who = "cm2_fourier_create";
    const fr::Launch &l = h->launch;
    const int64_t nb = l.nblocks;
    std::vector<int64_t> off((size_t)nb + 1, 0);
    for (int64_t b = 0; b < nb; ++b) off[b + 1] = off[b] + sizes[b];
    if (int rc = dev_put(&h->d_off, off.data(), off.size(), st)) return rc;
    std::vector<int32_t> rows((size_t)nb);
    int64_t at = 0;
    for (size_t g = 0; g < l.groups.size(); ++g) {
        h->groups.emplace_back(new GroupState());
        h->groups[g]->g = l.groups[g];
        h->groups[g]->row0 = at;
        for (int64_t b = 0; b < nb; ++b)
            if (l.group_of[(size_t)b] == (int32_t)g) rows[(size_t)at++] = (int32_t)b;
    }
    if (int rc = dev_put(&h->d_rows, rows.data(), rows.size(), st)) return rc;
    if (tau)
        if (int rc = dev_put(&h->d_tau, tau, (size_t)nb, st)) return rc;
    const fr::Response &r = l.resp;
    if (r.table_kind != fr::kNoTable) {
        const size_t count = (size_t)((r.table_per_block ? nb : 1) * r.Rn * (r.table_kind == fr::kComplexTable ? 2 : 1));
        if (int rc = dev_put(&h->d_table, table, count, st)) return rc;
    }
    CM2_HIP(dev_malloc(&h->d_ab, sizeof(double) * 2 * (size_t)nb));
    CM2_HIP(dev_malloc(&h->d_bad, sizeof(unsigned int) * (size_t)nb));
    int64_t x_bytes = 0, f_bytes = 0;
    for (auto &gs : h->groups) {
        fr::Group &g = gs->g;
        int64_t batch = fr::first_batch(g.L, g.blocks, max_work_bytes);
        for (;;) {
            if (int rc = gs->fft.plan(g.L, batch, true)) return rc;
            if (batch == 1 || fr::batch_fits(g.L, batch, (int64_t)gs->fft.work_bytes, max_work_bytes)) break;
            batch /= 2;
        }
        CM2_CHECK(fr::batch_fits(g.L, batch, (int64_t)gs->fft.work_bytes, max_work_bytes),
                  "%s: one block of L=%lld needs %lld bytes of work space (its row %lld, the plan %lld), max_work_bytes "
                  "is %lld", who, (long long)g.L, (long long)(fr::row_bytes(g.L) + (int64_t)gs->fft.work_bytes),
                  (long long)fr::row_bytes(g.L), (long long)gs->fft.work_bytes, (long long)max_work_bytes);
        g.batch = batch;
        if (int rc = gs->fft.bind()) return rc;
        h->plan_bytes += (int64_t)gs->fft.work_bytes;
        if (batch * g.L * 8 > x_bytes) x_bytes = batch * g.L * 8;
        if (batch * (g.L / 2 + 1) * 16 > f_bytes) f_bytes = batch * (g.L / 2 + 1) * 16;
    }
    CM2_HIP(dev_malloc(&h->d_X, (size_t)x_bytes));
    CM2_HIP(dev_malloc(&h->d_F, (size_t)f_bytes));
    h->row_bytes = x_bytes + f_bytes;
    CM2_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" int cm2_fourier_create(cm2_fourier **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, double fs,
                                  const double *h_tau, int mode, double f_lp, int p, double f_hp, int q,
                                  const double *h_notch, int nnotch, const double *h_table, int64_t Rn, int table_kind,
                                  int table_per_block, int detrend, int end_mean, int64_t pad, int conjugate,
                                  int64_t max_work_bytes, void *stream)
{
    const char *who = "cm2_fourier_create";
    CM2_CHECK(out, "%s: null output handle", who);
    std::unique_ptr<cm2_fourier> h(new cm2_fourier());
    const fr::Status ps = fr::check_create(&h->launch, nt, h_sizes, nblocks, fs, h_tau, mode, f_lp, p, f_hp, q, h_notch,
                                           nnotch, h_table, Rn, table_kind, table_per_block, detrend, end_mean, pad,
                                           conjugate);
    CM2_CHECK(ps != fr::kBadRate, "%s: fs=%g must be finite and > 0", who, fs);
    CM2_CHECK(ps != fr::kBadMode, "%s: mode=%d and conjugate=%d must each be 0 or 1", who, mode, conjugate);
    CM2_CHECK(ps != fr::kBadTau, "%s: every time constant must be finite and >= 0", who);
    CM2_CHECK(ps != fr::kBadCut, "%s: the cut-offs (%g, %g) must be finite and >= 0, the orders (%d, %d) in [1, %d]",
              who, f_lp, f_hp, p, q, fr::kMaxOrder);
    CM2_CHECK(ps != fr::kBadNotch, "%s: at most %d notches, each (f0 finite, width finite and > 0), got %d", who,
              fr::kMaxNotch, nnotch);
    CM2_CHECK(ps != fr::kBadTable, "%s: a response table needs kind 0, 1 or 2, Rn=%lld >= 2, its values and per_block 0 "
              "or 1", who, (long long)Rn);
    CM2_CHECK(ps != fr::kBadTableValue, "%s: a value of the response table is not finite", who);
    CM2_CHECK(ps != fr::kBadDetrend, "%s: detrend=%d must be 0 or 1 and end_mean=%d in [1, %d]", who, detrend, end_mean,
              fr::kMaxEndMean);
    CM2_CHECK(ps != fr::kBadPad, "%s: pad=%lld must be >= 0 and every transform length at most 2^28", who,
              (long long)pad);
    CM2_CHECK(ps != fr::kTooManyLengths, "%s: the blocks need more than %d distinct transform lengths", who,
              fr::kMaxLengths);
    if (int rc = check_create_status(who, ps, nt, nblocks, "window", 0, 0, "block tables")) return rc;
    if (max_work_bytes <= 0) max_work_bytes = fr::kDefaultWorkBytes;
    const int rc = fourier_fill(h.get(), h_sizes, h_tau, h_table, max_work_bytes, as_stream(stream));
    if (rc) {
        cm2_fourier_destroy(h.release());
        return rc;
    }
    *out = h.release();
    return 0;
}

extern "C" int cm2_fourier_info(const cm2_fourier *h, int64_t *h_info, void *stream)
{
    CM2_CHECK(h && h_info, "cm2_fourier_info: null argument");
    const fr::Launch &l = h->launch;
    int64_t nbad = 0;
    if (h->applied) {
        std::vector<unsigned int> bad((size_t)l.nblocks);
        CM2_HIP(download(bad.data(), h->d_bad, sizeof(unsigned int) * bad.size(), as_stream(stream)));
        for (unsigned int w : bad) nbad += w != 0u;
    }
    h_info[0] = l.nt;
    h_info[1] = l.nblocks;
    h_info[2] = (int64_t)h->groups.size();
    h_info[3] = h->row_bytes + h->plan_bytes;
    h_info[4] = nbad;
    for (int g = 0; g < fr::kMaxLengths; ++g) {
        const bool have = g < (int)h->groups.size();
        h_info[5 + g] = have ? h->groups[g]->g.L : 0;
        h_info[5 + fr::kMaxLengths + g] = have ? h->groups[g]->g.batch : 0;
        h_info[5 + 2 * fr::kMaxLengths + g] = have ? h->groups[g]->g.blocks : 0;
    }
    return 0;
}

extern "C" int cm2_fourier_apply(cm2_fourier *h, const double *d_in, double *d_out, void *stream)
{
    const char *who = "cm2_fourier_apply";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_in && d_out, "%s: null input or output", who);
    const fr::Launch &l = h->launch;
    const uint64_t bytes = 8 * (uint64_t)l.nt;
    if (int rc = check_disjoint(who, {{d_out, bytes}}, {{d_in, bytes}},
                                "%s: the output overlaps the input (it may be the input itself)", nullptr, 0, 0)) return rc;
    hipStream_t st = as_stream(stream);
    k_fourier_ends<<<dim3((unsigned)l.nblocks), fr::kThreads, 0, st>>>(h->d_off, d_in, l.detrend, l.end_mean, h->d_ab,
                                                                      h->d_bad);
    CM2_LAUNCH_OK();
    h->applied = true;
    for (auto &gs : h->groups) {
        const fr::Group &g = gs->g;
        const int64_t nfreq = g.L / 2 + 1, nseg = fr::segments(g.L);
        if (int rc = gs->fft.set_stream(st)) return rc;
        for (int64_t first = 0; first < g.blocks; first += g.batch) {
            const Rows rw = {h->d_rows + gs->row0, first, g.blocks, g.L};
            k_fourier_pack<<<dim3((unsigned)(g.batch * nseg)), fr::kThreads, 0, st>>>(rw, nseg, h->d_off, d_in, h->d_ab,
                                                                                     l.detrend, h->d_bad, h->d_X);
            CM2_LAUNCH_OK();
            if (int rc = gs->fft.forward(h->d_X, h->d_F)) return rc;
            k_fourier_response<<<dim3((unsigned)grid_for(g.batch * nfreq)), kBlock, 0, st>>>(
                rw, g.batch, nfreq, l.resp, h->d_tau, h->d_table, h->d_F);
            CM2_LAUNCH_OK();
            if (int rc = gs->fft.inverse(h->d_F, h->d_X)) return rc;
            k_fourier_unpack<<<dim3((unsigned)(g.batch * nseg)), fr::kThreads, 0, st>>>(
                rw, nseg, h->d_off, h->d_X, h->d_ab, l.detrend, h->d_bad, l.resp, h->d_tau, h->d_table, d_out);
            CM2_LAUNCH_OK();
        }
    }
    return 0;
}

extern "C" int cm2_fourier_response(const cm2_fourier *h, int64_t block, double *d_H, void *stream)
{
    const char *who = "cm2_fourier_response";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_H, "%s: null output", who);
    const fr::Launch &l = h->launch;
    CM2_CHECK(block >= 0 && block < l.nblocks, "%s: block=%lld outside [0, %lld)", who, (long long)block,
              (long long)l.nblocks);
    const int64_t L = l.groups[(size_t)l.group_of[(size_t)block]].L, nfreq = L / 2 + 1;
    k_fourier_write_response<<<dim3((unsigned)grid_for(nfreq)), kBlock, 0, as_stream(stream)>>>(
        block, L, nfreq, l.resp, h->d_tau, h->d_table, d_H);
    CM2_LAUNCH_OK();
    return 0;
}
