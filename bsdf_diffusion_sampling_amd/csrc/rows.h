// rows.h — what every one-thread-per-row kernel of the ground-truth evaluators and its launcher share, whatever the model:
// measured.hip and measured_table.hip (through measured_dev.h), principled.hip, dielectric.hip and analytic_table.hip (through
// analytic_rows.h).  Device side: the tint, the row store, the "no ground truth" value.  Host side: the count and device checks of
// a launch and the launch itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "common.h"

// Fused multiply-adds are formed per source expression, by the front end, from here to the end of the including translation
// unit — not wherever the optimiser finds a product next to a sum (hipcc's default): that choice depends on the code around an
// inlined copy (which pairs the vectoriser packs, which of a*b + c*d becomes the fma's product), and it made a table kernel and
// its single-material kernel round the same expressions differently.  With this both compute the same bits.  Every header of a
// model (measured_dev.h, dielectric_dev.h, principled_dev.h) repeats the pragma, so that none depends on an include's position.
#pragma clang fp contract(on)

namespace rows {

struct Tint {
    float r, g, b;
};

__device__ __forceinline__ void store3(float* __restrict__ out, long long q, float a, float b, float c) {
    out[3 * q] = a; out[3 * q + 1] = b; out[3 * q + 2] = c;
}

// what a table kernel writes for a row without ground truth: the "use the proxy" value bsdfd_wf_shade reads
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// ---- host path shared by the launchers, after their own checks of the handle, descriptor or table ----
// The largest N of one launch.  The single-material calls bound the grid, the table calls the thread index.
constexpr long long kMaxRowsSingle = 0x7fffffffLL * 256;   // (N + 255) / 256 <= 0x7fffffff
constexpr long long kMaxRowsTable = 0xffffffffLL - 255;    // grid * block < 2^32

// The count and device checks of a launch, in the order every launcher keeps: N >= 0; for a call on an object bound to a device
// (`device`: where it says which, read only once N is known to be sound; `owner` names it, as in "measured handle") that this is
// the current device — a descriptor passed by value has none, and the checks do no device work; N <= max_n.
inline int launch_checks(int64_t n, long long max_n, const char* owner = nullptr, const int* device = nullptr) {
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (device) {
        int dev = -1;
        HIP_TRY(hipGetDevice(&dev));
        if (dev != *device) return bsdfd_fail_(BSDFD_EINVAL, std::string(owner) + " belongs to another device");
    }
    if ((long long)n > max_n) return bsdfd_fail_(BSDFD_EINVAL, "N too large for one launch");
    return BSDFD_OK;
}

// a launcher's optional `tint` argument (null: white), read where it becomes the kernel's Tint: at the launch, after the checks
struct TintArg {
    const float* rgb;
    operator Tint() const { return rgb ? Tint{rgb[0], rgb[1], rgb[2]} : Tint{1.0f, 1.0f, 1.0f}; }
};

// the empty call, `bad` (the first complaint about the arguments, or null), one thread per row in blocks of 256, the launch error
template <class... P, class... A>
int launch_rows(int64_t n, const char* bad, void (*kernel)(P...), void* stream, A... args) {
    if (n == 0) return BSDFD_OK;
    if (bad) return bsdfd_fail_(BSDFD_EINVAL, bad);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
    HIP_TRY(hipGetLastError());
    return BSDFD_OK;
}

}  // namespace rows
