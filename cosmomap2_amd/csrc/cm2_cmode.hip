// cm2_cmode.hip -- the common-mode filter (CommonModeFilterLO), see include/cosmomap2.h (f2d): per (group, time
// sample) unit, fit and remove K templates Phi[k, 0..K-1] across the unflagged detectors k of the group.
// cm2_cmode_policy.h has the accepted arguments and the launch arithmetic.
//
// The unit itself -- the order of every operation, the look-ahead, the aliasing rule of an apply -- is cm2_modefit.h's,
// which the PCA filter shares.  Here: where a thread finds its unit (a group owns blocks_per_group consecutive
// workgroups, consecutive lanes take consecutive samples) and the one table Phi of the handle.
#include <vector>

#include "cm2_modefit.h"
#include "cm2_cmode_policy.h"

using namespace cm2;
namespace cp = cm2::cmode;
namespace mf = cm2::modefit;

namespace {

struct Shape {
    int64_t ns, blocks_per_group;
    const int32_t *gedges;          // [ngroups + 1], device
    const double *modes;            // [ndet][K], device
    const int32_t *pix;             // [ndet ns], device, borrowed
};

__device__ __forceinline__ mf::Frame my_unit(const Shape &s)
{
    mf::Frame u;
    u.ns = s.ns;
    u.g = (int64_t)blockIdx.x / s.blocks_per_group;
    u.i = ((int64_t)blockIdx.x - u.g * s.blocks_per_group) * cp::kThreads + threadIdx.x;
    u.k0 = s.gedges[u.g];
    u.k1 = s.gedges[u.g + 1];
    u.phi = s.modes;
    u.pix = s.pix;
    u.live = u.i < s.ns;
    return u;
}

// the bodies, and why v and out are not __restrict__: cm2_modefit.h
template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_apply(Shape s, double tau, const double *v, double *out)
{
    mf::apply<K>(my_unit(s), tau, v, out);
}

template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_fit(Shape s, double tau, const double *__restrict__ v,
                                                             double *__restrict__ coeff)
{
    mf::coefficients<K>(my_unit(s), tau, v, coeff);
}

template <int K>
__global__ __launch_bounds__(cp::kThreads) void k_cmode_class(Shape s, double tau, uint8_t *__restrict__ status,
                                                               unsigned long long *__restrict__ counts)
{
    mf::classify<K>([&] { return my_unit(s); }, tau, status, counts);
}

}  // namespace

struct cm2_cmode {
    cp::Launch launch;
    int64_t ns = 0, ndet = 0, ngroups = 0;
    int K = 0;
    const int32_t *d_pix = nullptr;        // borrowed
    int32_t *d_gedges = nullptr;
    double *d_modes = nullptr;
    uint8_t *d_status = nullptr;
    int64_t nclass[4] = {0, 0, 0, 0};
    Shape shape() const { return Shape{ns, launch.blocks_per_group, d_gedges, d_modes, d_pix}; }
};

extern "C" int cm2_cmode_destroy(cm2_cmode *h)
{
    if (!h) return 0;
    dev_release(h->d_gedges, h->d_modes, h->d_status);
    delete h;
    return 0;
}

namespace {

int cmode_fill(cm2_cmode *h, const int64_t *h_edges, const double *d_modes, hipStream_t st)
{
    std::vector<int32_t> e((size_t)h->ngroups + 1);
    for (size_t g = 0; g < e.size(); ++g) e[g] = (int32_t)h_edges[g];
    if (int rc = dev_put(&h->d_gedges, e.data(), e.size(), st)) return rc;
    const size_t mbytes = sizeof(double) * (size_t)h->ndet * (size_t)h->K;
    CM2_HIP(cm2::dev_malloc(&h->d_modes, mbytes));
    CM2_HIP(hipMemcpyAsync(h->d_modes, d_modes, mbytes, hipMemcpyDeviceToDevice, st));
    CM2_HIP(cm2::dev_malloc(&h->d_status, (size_t)h->launch.units));
    DevTemp<unsigned long long> counts;
    CM2_HIP(counts.alloc(4));
    auto launch_class = [&](auto K) {
        k_cmode_class<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, st>>>(h->shape(), CM2_CMODE_TAU,
                                                                                    h->d_status, counts.p);
    };
    return mf::count_classes(h->K, launch_class, counts.p, st, h->nclass);
}

}  // namespace

extern "C" int cm2_cmode_create(cm2_cmode **out, int64_t ns, int ndet, int ngroups, const int64_t *h_group_edges,
                                int K, const double *d_modes, const int32_t *d_pix, void *stream)
{
    const char *who = "cm2_cmode_create";
    CM2_CHECK(out, "%s: null output handle", who);
    CM2_CHECK(h_group_edges && d_modes && d_pix, "%s: null array", who);
    cp::Launch l;
    const cp::Status ps = cp::check(&l, ns, ndet, ngroups, h_group_edges, K);
    if (int rc = mf::check_create_status(who, ps, ndet, ngroups, K)) return rc;
    CM2_CHECK(ps != cp::kBadSize, "%s: ns=%lld, ndet=%d, ngroups=%d must all be >= 1", who, (long long)ns, ndet,
              ngroups);
    CM2_CHECK(ps == cp::kOk, "%s: ns=%lld x ndet=%d in %d groups overflows the index types or the grid", who,
              (long long)ns, ndet, ngroups);
    cm2_cmode *h = new cm2_cmode();
    h->launch = l;
    h->ns = ns;
    h->ndet = ndet;
    h->ngroups = ngroups;
    h->K = K;
    h->d_pix = d_pix;
    const int rc = cmode_fill(h, h_group_edges, d_modes, as_stream(stream));
    if (rc) {
        cm2_cmode_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int cm2_cmode_info(const cm2_cmode *h, int64_t *h_info)
{
    CM2_CHECK(h && h_info, "cm2_cmode_info: null argument");
    h_info[0] = h->ns;
    h_info[1] = h->ndet;
    h_info[2] = h->ngroups;
    h_info[3] = h->K;
    for (int c = 0; c < 4; ++c) h_info[4 + c] = h->nclass[c];
    return 0;
}

extern "C" int cm2_cmode_apply(cm2_cmode *h, const double *d_in, double *d_out, void *stream)
{
    CM2_CHECK(h, "cm2_cmode_apply: null handle");
    CM2_CHECK(d_in && d_out, "cm2_cmode_apply: null vector");
    CM2_CHECK(mf::apply_ok(d_in, d_out, h->launch.nt),
              "cm2_cmode_apply: the output must be the input itself or not overlap it");
    dispatch_int<1, cp::kMaxK>(h->K, [&](auto K) {
        k_cmode_apply<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, as_stream(stream)>>>(
            h->shape(), CM2_CMODE_TAU, d_in, d_out);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_cmode_fit(cm2_cmode *h, const double *d_in, double *d_coeff, void *stream)
{
    CM2_CHECK(h, "cm2_cmode_fit: null handle");
    CM2_CHECK(d_in && d_coeff, "cm2_cmode_fit: null vector");
    CM2_CHECK(!ranges_overlap(d_in, h->launch.nt, d_coeff, h->launch.units * h->K),
              "cm2_cmode_fit: the coefficients must not alias the input");
    dispatch_int<1, cp::kMaxK>(h->K, [&](auto K) {
        k_cmode_fit<K><<<dim3((unsigned)h->launch.blocks), cp::kThreads, 0, as_stream(stream)>>>(
            h->shape(), CM2_CMODE_TAU, d_in, d_coeff);
    });
    CM2_LAUNCH_OK();
    return 0;
}

extern "C" int cm2_cmode_status(const cm2_cmode *h, uint8_t *d_status)
{
    CM2_CHECK(h && d_status, "cm2_cmode_status: null argument");
    return mf::copy_status(d_status, h->d_status, h->launch.units);
}
