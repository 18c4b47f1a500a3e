// cm2_rocfft.h -- the only place that talks to rocFFT: the status macro, the process-wide set-up and the
// owner of a batched 1-D fp64 real transform.  Included by cm2_noise.hip (the rocFFT overlap-save route of
// N^-1) and cm2_noise_model.hip (Welch PSD).
#pragma once
#include "cm2_common.h"

#include <rocfft/rocfft.h>

#include <mutex>

// rocFFT reports no out-of-memory status of its own: every failure of the library is CM2_ERR_HIP (only the
// allocations a unit makes itself, through CM2_HIP, can give CM2_ERR_OUT_OF_MEMORY)
#define CM2_ROCFFT(call)                                                               \
    do {                                                                               \
        rocfft_status s__ = (call);                                                    \
        if (s__ != rocfft_status_success) {                                            \
            cm2::set_error("%s failed: rocfft_status %d (%s:%d)", #call, (int)s__,     \
                           __FILE__, __LINE__);                                        \
            return CM2_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

namespace cm2 {

// rocfft_setup, once per process whichever unit comes first; every caller gets the status of that one call
inline rocfft_status fft_library_ready()
{
    static std::once_flag once;
    static rocfft_status status = rocfft_status_success;
    std::call_once(once, [] { status = rocfft_setup(); });
    return status;
}

// `batch` real transforms of length L, contiguous and out of place: in [batch][L] doubles, out [batch][L/2+1]
// double2 (forward) and back (inverse, unnormalised).  Two steps, because a caller may size its batch by the
// work buffer a plan asks for: plan() creates the plans and sets work_bytes without touching device memory of
// the library, bind() makes the execution info and allocates the work buffer both directions share.
struct RealFft : NoCopy {
    rocfft_plan fwd = nullptr, inv = nullptr;
    rocfft_execution_info info = nullptr;
    void *d_work = nullptr;
    size_t work_bytes = 0;           // the larger of the two plans' needs
    ~RealFft() { reset(); }
    void reset()
    {
        if (fwd) rocfft_plan_destroy(fwd);
        if (inv) rocfft_plan_destroy(inv);
        if (info) rocfft_execution_info_destroy(info);
        fwd = inv = nullptr;
        info = nullptr;
        dev_release(d_work);
        work_bytes = 0;
    }
    // replaces the plans held (call it again with another batch before bind())
    int plan(int64_t L, int64_t batch, bool with_inverse)
    {
        reset();
        CM2_ROCFFT(fft_library_ready());
        const size_t lengths[1] = {(size_t)L};
        CM2_ROCFFT(rocfft_plan_create(&fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                                      rocfft_precision_double, 1, lengths, (size_t)batch, nullptr));
        CM2_ROCFFT(rocfft_plan_get_work_buffer_size(fwd, &work_bytes));
        if (with_inverse) {
            size_t w = 0;
            CM2_ROCFFT(rocfft_plan_create(&inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                          rocfft_precision_double, 1, lengths, (size_t)batch, nullptr));
            CM2_ROCFFT(rocfft_plan_get_work_buffer_size(inv, &w));
            if (w > work_bytes) work_bytes = w;
        }
        return 0;
    }
    int bind()
    {
        CM2_ROCFFT(rocfft_execution_info_create(&info));
        if (work_bytes) {
            CM2_HIP(dev_malloc(&d_work, work_bytes));
            CM2_ROCFFT(rocfft_execution_info_set_work_buffer(info, d_work, work_bytes));
        }
        return 0;
    }
    int set_stream(hipStream_t stream)
    {
        CM2_ROCFFT(rocfft_execution_info_set_stream(info, stream));
        return 0;
    }
    int forward(double *in, double2 *out)
    {
        void *i[1] = {in}, *o[1] = {out};
        CM2_ROCFFT(rocfft_execute(fwd, i, o, info));
        return 0;
    }
    int inverse(double2 *in, double *out)
    {
        void *i[1] = {in}, *o[1] = {out};
        CM2_ROCFFT(rocfft_execute(inv, i, o, info));
        return 0;
    }
};

}  // namespace cm2
