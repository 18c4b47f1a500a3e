// cm2_demod.hip -- lock-in demodulation and decimation of the time streams, see include/cosmomap2.h (f2h): a FIR
// low-pass of d (and, with a carrier, of d cos and d sin) cut at the block boundaries and renormalised by the weight of
// the usable taps, one output in D samples, with a class byte per output and counts per block; and the pixel of
// every output's centre sample.  cm2_demod_policy.h has the accepted arguments, the units and what a unit holds in
// LDS; cm2_stream.h how a kernel sees the stream, its flags and its blocks.
//
// The floating-point operations are the ones of the definition, each rounded on its own (the unit is compiled with
// -ffp-contract=off): d cos and d sin once per sample, then per output and tap one product and one addition per
// chain, in ascending k from +0.0, one division (and one doubling) per result.  No MFMA, no floating-point atomic, no
// cross-lane operation on doubles; the counts are integers.
//
// k_demod_fir.  A workgroup takes one unit [first, end) of one block and stages in LDS the samples from first - c on
// that the windows of its outputs cover: d, d cos and d sin, an unusable sample and a position outside the block as
// +0.0 (h 0.0 is +-0.0, and x + +-0.0 has the bits of x for every x a chain that started from +0.0 can hold, so the
// chains need no branch), and one byte that says which.  The loads are 16 bytes wide where the arrays are aligned and
// the pair lies in the block.  Thread t then walks the taps for the outputs t, t + 256, ... of the unit side by side:
// per output the chains T, (Q, U,) W and the count of included terms, all independent; a wave none of whose threads
// has an output skips the walk.  Tap k is one scalar load for the whole wave.  A unit whose every staged sample is
// usable and inside the block takes W = Wfull and class FULL for all its outputs and reads no bytes: the same bits,
// since W's chain would add the very taps Wfull added.
//
// k_demod_pick.  One thread per output: its block by bisection of the output prefix, the pixel of its centre.
#include "cm2_common.h"
#include "cm2_demod_policy.h"
#include "cm2_stream.h"

using namespace cm2;
using namespace cm2::stream;
namespace dm = cm2::demod;

namespace {

struct Carrier {
    const double *cosv, *sinv;             // NULL without a carrier
};

struct Outputs {
    double *T, *Q, *U;                     // [M]; Q and U NULL without a carrier
    uint8_t *cls;                          // [M]
    unsigned long long *counts;            // [nblocks][3]
};

// what a unit needs to know of the filter
struct Fir {
    int D, L, c, per_unit, rounds;
    double wfull, threshold;               // min_weight * Wfull, one multiplication
};

// a staged unit: the planes, its outputs, the first of them in the output streams (the unit starts on an output
// centre), and whether every staged sample is usable and inside the block
struct Unit {
    const double *sT, *sQ, *sU;
    const uint8_t *use;
    int nout;
    int64_t out0;
    bool all_usable;
};

// One output's chains.  MASKED = false: every term is included, W and the count are not formed.
template <bool CARRIER, bool MASKED>
struct Chains {
    double T = 0.0, Q = 0.0, U = 0.0, W = 0.0;
    int n = 0;
    __device__ __forceinline__ void term(const Unit &un, int v, double h)
    {
        const int s = dm::slot(v);
        T = T + h * un.sT[s];
        if (CARRIER) {
            Q = Q + h * un.sQ[s];
            U = U + h * un.sU[s];
        }
        if (MASKED) {
            const int u = un.use[s];
            W = W + (u ? h : 0.0);
            n += u;
        }
    }
};

// rule 3 for the ROUNDS outputs of a thread side by side, kTapsAtOnce taps (scalar loads) in flight
template <bool CARRIER, bool MASKED, int ROUNDS>
__device__ __forceinline__ void walk(const Unit &un, const Fir &f, const double *__restrict__ taps,
                                     Chains<CARRIER, MASKED> (&ch)[ROUNDS])
{
    constexpr int kTapsAtOnce = ROUNDS == 1 ? 8 : ROUNDS == 2 ? 4 : ROUNDS <= 4 ? 2 : 1;
    int at[ROUNDS];
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m) {
        const int q = m * dm::kThreads + (int)threadIdx.x;
        at[m] = q < un.nout ? q * f.D : 0;                                    // a thread without an output reads from 0 on
    }
    int k = 0;
    for (; k + kTapsAtOnce <= f.L; k += kTapsAtOnce) {
        double h[kTapsAtOnce];
#pragma unroll
        for (int u = 0; u < kTapsAtOnce; ++u) h[u] = taps[k + u];
#pragma unroll
        for (int u = 0; u < kTapsAtOnce; ++u)
#pragma unroll
            for (int m = 0; m < ROUNDS; ++m) ch[m].term(un, at[m] + k + u, h[u]);
    }
    for (; k < f.L; ++k) {
        const double h = taps[k];
#pragma unroll
        for (int m = 0; m < ROUNDS; ++m) ch[m].term(un, at[m] + k, h);
    }
}

// rules 4 and 5 for output q of the unit
template <bool CARRIER>
__device__ __forceinline__ void store(const Unit &un, const Fir &f, const Outputs &o, unsigned int *tally, int q,
                                      double T, double Q, double U, double W, int included)
{
    if (q >= un.nout) return;
    const bool ok = W >= f.threshold;                                         // (false for a NaN)
    const int c = dm::class_of(included, f.L, ok);
    const bool keep = c != dm::kRejected;
    o.T[un.out0 + q] = keep ? T / W : 0.0;
    if (CARRIER) {
        o.Q[un.out0 + q] = keep ? 2.0 * (Q / W) : 0.0;
        o.U[un.out0 + q] = keep ? 2.0 * (U / W) : 0.0;
    }
    o.cls[un.out0 + q] = (uint8_t)c;
    atomicAdd(&tally[c], 1u);
}

template <bool CARRIER, int ROUNDS>
__device__ __forceinline__ void finish(const Unit &un, const Fir &f, const double *__restrict__ taps, const Outputs &o,
                                       unsigned int *tally)
{
    if (un.all_usable) {                                                      // W = Wfull, all L terms included
        Chains<CARRIER, false> ch[ROUNDS];
        walk<CARRIER, false, ROUNDS>(un, f, taps, ch);
#pragma unroll
        for (int m = 0; m < ROUNDS; ++m)
            store<CARRIER>(un, f, o, tally, m * dm::kThreads + (int)threadIdx.x, ch[m].T, ch[m].Q, ch[m].U, f.wfull, f.L);
    } else {
        Chains<CARRIER, true> ch[ROUNDS];
        walk<CARRIER, true, ROUNDS>(un, f, taps, ch);
#pragma unroll
        for (int m = 0; m < ROUNDS; ++m)
            store<CARRIER>(un, f, o, tally, m * dm::kThreads + (int)threadIdx.x, ch[m].T, ch[m].Q, ch[m].U, ch[m].W,
                           ch[m].n);
    }
}

template <bool CARRIER, int KIND>
__global__ __launch_bounds__(dm::kThreads) void k_demod_fir(Blocks tb, const int64_t *__restrict__ out_start, Fir f,
                                                            const double *__restrict__ taps,
                                                            const double *__restrict__ d,
                                                            const void *__restrict__ flags, Carrier car, int wide,
                                                            Outputs o)
{
    extern __shared__ double lds[];
    __shared__ unsigned int tally[dm::kCounts];
    __shared__ int unusable;
    const int tid = threadIdx.x;
    const Span sp = unit_span(tb.off, tb.unit_start, tb.nblocks, (int64_t)f.per_unit * f.D, (int64_t)blockIdx.x);
    const int64_t lo = tb.off[sp.block], hi = tb.off[sp.block + 1];
    const int nout = (int)dm::outputs_of(sp.end - sp.first, f.D);             // outputs centred in this unit
    const int nst = dm::staged(nout, f.D, f.L), nslots = dm::slots(nst);
    const int64_t base = sp.first - f.c;                                      // the sample of staged value 0
    double *sT = lds, *sQ = lds + (CARRIER ? nslots : 0), *sU = lds + (CARRIER ? 2 * nslots : 0);
    uint8_t *use = reinterpret_cast<uint8_t *>(lds + (CARRIER ? 3 : 1) * nslots);
    if (tid < dm::kCounts) tally[tid] = 0u;
    if (tid == 0) unusable = 0;
    __syncthreads();

    // ---- stage: pairs of samples at even positions of the stream, so that an aligned array is read 16 bytes wide
    int bad = 0;
    const int64_t even = base & ~(int64_t)1;
    const int npairs = (int)((base + nst - even + 1) / 2);
    for (int p = tid; p < npairs; p += dm::kThreads) {
        const int64_t i0 = even + 2 * (int64_t)p;
        const int v0 = (int)(i0 - base);
        const bool slot0 = v0 >= 0, slot1 = v0 + 1 < nst;                     // (v0 >= -1 and v0 < nst always)
        const bool in0 = slot0 && i0 >= lo && i0 < hi, in1 = slot1 && i0 + 1 >= lo && i0 + 1 < hi;
        double x[2] = {0.0, 0.0}, cs[2] = {0.0, 0.0}, sn[2] = {0.0, 0.0};
        if (wide && in0 && in1) {
            const double2 xx = *reinterpret_cast<const double2 *>(d + i0);
            x[0] = xx.x;
            x[1] = xx.y;
            if (CARRIER) {
                const double2 cc = *reinterpret_cast<const double2 *>(car.cosv + i0);
                const double2 ss = *reinterpret_cast<const double2 *>(car.sinv + i0);
                cs[0] = cc.x;
                cs[1] = cc.y;
                sn[0] = ss.x;
                sn[1] = ss.y;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (e == 0 ? in0 : in1) {
                    x[e] = d[i0 + e];
                    if (CARRIER) {
                        cs[e] = car.cosv[i0 + e];
                        sn[e] = car.sinv[i0 + e];
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!(e == 0 ? slot0 : slot1)) continue;
            const bool in = e == 0 ? in0 : in1;
            const bool u = in && finite_bits(x[e]) && !(flags && flagged<KIND>(flags, i0 + e));
            const int s = dm::slot(v0 + e);
            sT[s] = u ? x[e] : 0.0;
            if (CARRIER) {
                sQ[s] = u ? x[e] * cs[e] : 0.0;                               // formed once per sample
                sU[s] = u ? x[e] * sn[e] : 0.0;
            }
            use[s] = u ? 1 : 0;
            bad |= u ? 0 : 1;
        }
    }
    if (bad) unusable = 1;                                                    // (every writer writes 1)
    __syncthreads();

    // ---- the chains of the outputs tid, tid + 256, ..., then results, classes and counts
    const Unit un = {sT, sQ, sU, use, nout, out_start[sp.block] + (sp.first - lo) / f.D, unusable == 0};
    // the rounds in which this wave has an output at all (the same for its 64 lanes: the first lane's id says which
    // wave it is): a wave beyond the unit's outputs -- three and a half of the four at D = 64, the tail of a block's
    // last unit at any D -- walks no tap
    const int wave_first = __builtin_amdgcn_readfirstlane(tid) & ~(kWave - 1);
    const int left = nout - wave_first;
    const int mine = left <= 0 ? 0 : (left + dm::kThreads - 1) / dm::kThreads;
    switch (mine < f.rounds ? mine : f.rounds) {
    case 0: break;
    case 1: finish<CARRIER, 1>(un, f, taps, o, tally); break;
    case 2: finish<CARRIER, 2>(un, f, taps, o, tally); break;
    case 3: finish<CARRIER, 3>(un, f, taps, o, tally); break;
    case 4: finish<CARRIER, 4>(un, f, taps, o, tally); break;
    default: finish<CARRIER, dm::kRounds>(un, f, taps, o, tally); break;
    }
    __syncthreads();
    if (tid < dm::kCounts && tally[tid])
        atomicAdd(&o.counts[(size_t)sp.block * dm::kCounts + tid], (unsigned long long)tally[tid]);
}

__global__ __launch_bounds__(kBlock) void k_demod_pick(const int64_t *__restrict__ off,
                                                       const int64_t *__restrict__ out_start, int64_t nblocks, int D,
                                                       int64_t M, const int32_t *__restrict__ pix,
                                                       const uint8_t *__restrict__ cls, int drop_from,
                                                       int32_t *__restrict__ out)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < M; q += (int64_t)gridDim.x * kBlock) {
        const int64_t b = locate(out_start, nblocks, q);
        const int32_t p = pix[off[b] + (q - out_start[b]) * D];               // the centre sample of output q
        out[q] = cls[q] >= drop_from || p < 0 ? -1 : p;
    }
}

}  // namespace

struct cm2_demod {
    dm::Launch launch;
    BlockTables tables;                    // the blocks in input units (0) and in outputs (1)
    double *d_taps = nullptr;              // [L]
    int64_t bytes = 0;
    Blocks units() const { return tables.view(0); }
    const int64_t *out_start() const { return tables.d_unit_start[1]; }
};

extern "C" int cm2_demod_destroy(cm2_demod *h)
{
    if (!h) return 0;
    dev_release(h->d_taps);
    delete h;
    return 0;
}

namespace {

int demod_fill(cm2_demod *h, const int64_t *sizes, const double *taps, void *stream)
{
    hipStream_t st = as_stream(stream);
    if (int rc = h->tables.fill(sizes, h->launch.nblocks, {(int64_t)h->launch.unit, (int64_t)h->launch.D}, st))
        return rc;
    if (int rc = dev_put(&h->d_taps, taps, (size_t)h->launch.L, st)) return rc;
    h->bytes = h->tables.bytes() + (int64_t)h->launch.L * 8;
    return 0;
}

template <bool CARRIER, int KIND>
int demod_launch(const cm2_demod *h, const Fir &f, const double *d, const void *flags, Carrier car, int wide,
                 Outputs o, hipStream_t st)
{
    const size_t lds = (size_t)(CARRIER ? h->launch.lds_carrier : h->launch.lds_plain);
    static size_t granted[64] = {0};
    CM2_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(k_demod_fir<CARRIER, KIND>), lds, granted));
    k_demod_fir<CARRIER, KIND><<<dim3((unsigned)h->launch.units), dm::kThreads, lds, st>>>(
        h->units(), h->out_start(), f, h->d_taps, d, flags, car, wide, o);
    CM2_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" int cm2_demod_create(cm2_demod **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int factor,
                                const double *h_taps, int ntaps, void *stream)
{
    const char *who = "cm2_demod_create";
    CM2_CHECK(out, "%s: null output handle", who);
    dm::Launch l;
    const dm::Status ps = dm::check_create(&l, nt, h_sizes, nblocks, factor, h_taps, ntaps);
    CM2_CHECK(ps != dm::kBadFactor, "%s: factor=%d outside [1, %d]", who, factor, dm::kMaxFactor);
    CM2_CHECK(ps != dm::kBadTaps, "%s: ntaps=%d must be odd, in [1, %d], and the taps given", who, ntaps, dm::kMaxTaps);
    CM2_CHECK(ps != dm::kBadTapValue, "%s: a tap is not finite", who);
    CM2_CHECK(ps != dm::kBadTapSum, "%s: the sum of the taps must be finite and > 0", who);
    if (int rc = check_create_status(who, ps, nt, nblocks, "factor", factor, dm::kMaxFactor, "block tables")) return rc;
    cm2_demod *h = new cm2_demod();
    h->launch = l;
    const int rc = demod_fill(h, h_sizes, h_taps, stream);
    if (rc) {
        cm2_demod_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_demod_info(const cm2_demod *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_demod_info: null argument");
    h_info[0] = h->launch.nt;
    h_info[1] = h->launch.nblocks;
    h_info[2] = h->launch.D;
    h_info[3] = h->launch.L;
    h_info[4] = h->launch.M;
    h_info[5] = h->launch.unit;
    h_info[6] = h->launch.rounds;
    h_info[7] = h->launch.lds_carrier;
    h_info[8] = h->bytes;
    return 0;
}

extern "C" int cm2_demod_run(cm2_demod *h, const double *d_in, const double *d_cos, const double *d_sin,
                             const void *d_flags, int flag_kind, double min_weight, double *d_T, double *d_Q,
                             double *d_U, uint8_t *d_class, int64_t *d_counts, void *stream)
{
    const char *who = "cm2_demod_run";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_in && d_T && d_class && d_counts, "%s: null input or output", who);
    const bool carrier = d_cos || d_sin;
    CM2_CHECK(!carrier || (d_cos && d_sin && d_Q && d_U), "%s: a carrier needs cos, sin, Q and U", who);
    CM2_CHECK(carrier || (!d_Q && !d_U), "%s: Q and U are given without a carrier", who);
    if (int rc = check_flag_kind_status(who, d_flags != nullptr, flag_kind)) return rc;
    CM2_CHECK(dm::check_run(d_flags != nullptr, flag_kind, min_weight) == dm::kOk,
              "%s: min_weight=%g outside (0, 1]", who, min_weight);
    const uint64_t nt = (uint64_t)h->launch.nt, nb = (uint64_t)h->launch.nblocks, M = (uint64_t)h->launch.M;
    if (int rc = check_disjoint(who, {{d_T, 8 * M}, {d_Q, 8 * M}, {d_U, 8 * M}, {d_class, M},
                                      {d_counts, 8 * dm::kCounts * nb}},
                                {{d_in, 8 * nt}, {d_cos, 8 * nt}, {d_sin, 8 * nt},
                                 {d_flags, flag_kind == 0 ? 4 * nt : nt}},
                                "%s: an output overlaps an input", "%s: two outputs overlap")) return rc;
    hipStream_t st = as_stream(stream);
    const dm::Launch &l = h->launch;
    const Fir f = {l.D, l.L, l.c, l.per_unit, l.rounds, l.wfull, min_weight * l.wfull};
    const Carrier car = {d_cos, d_sin};
    const Outputs o = {d_T, d_Q, d_U, d_class, reinterpret_cast<unsigned long long *>(d_counts)};
    const uintptr_t low = reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_cos) |
                          reinterpret_cast<uintptr_t>(d_sin);
    const int wide = low % 16 == 0;
    CM2_HIP(hipMemsetAsync(d_counts, 0, (size_t)(8 * dm::kCounts * nb), st));
    const int kind = d_flags ? flag_kind : 0;
    if (carrier) return kind == 0 ? demod_launch<true, 0>(h, f, d_in, d_flags, car, wide, o, st)
                                  : demod_launch<true, 1>(h, f, d_in, d_flags, car, wide, o, st);
    return kind == 0 ? demod_launch<false, 0>(h, f, d_in, d_flags, car, wide, o, st)
                     : demod_launch<false, 1>(h, f, d_in, d_flags, car, wide, o, st);
}

extern "C" int cm2_demod_pick(const cm2_demod *h, const int32_t *d_pix, const uint8_t *d_class, int drop_from,
                              int32_t *d_out, void *stream)
{
    const char *who = "cm2_demod_pick";
    CM2_CHECK(h, "%s: null handle", who);
    CM2_CHECK(d_pix && d_class && d_out, "%s: null input or output", who);
    CM2_CHECK(dm::check_pick(drop_from) == dm::kOk, "%s: drop_from=%d is neither 1 (partial) nor 2 (rejected)", who,
              drop_from);
    const uint64_t nt = (uint64_t)h->launch.nt, M = (uint64_t)h->launch.M;
    if (int rc = check_disjoint(who, {{d_out, 4 * M}}, {{d_pix, 4 * nt}, {d_class, M}},
                                "%s: the output overlaps an input")) return rc;
    k_demod_pick<<<dim3((unsigned)grid_for(h->launch.M)), kBlock, 0, as_stream(stream)>>>(
        h->tables.d_off, h->out_start(), h->launch.nblocks, h->launch.D, h->launch.M, d_pix, d_class, drop_from, d_out);
    CM2_LAUNCH_OK();
    return 0;
}
