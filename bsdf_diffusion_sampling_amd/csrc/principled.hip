// principled.hip — the analytic ground truth of the full-sphere plugin for bsdf_0..22: Mitsuba's `principled` restated.
//
// The reference's full-sphere plugin evaluates an analytic Mitsuba BSDF for its eval(), sample weight and firefly rule
// (rendering/bsdf_myresult.py:97-110); entries 0..22 of its material list (rendering/utils/bsdf_dict.py) are principled BSDFs.
// Four kernels, one row per lane, over the device functions of principled_dev.h: eval, the tail of the plugin's sample()
// (weight + firefly rule), the model's own importance sampler, and its pdf.  No tables, no handle: the material is a 64-byte
// descriptor read on the host at the call; what depends on it alone is derived there, once (analytic_host.h), and passed by value.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "analytic_host.h"
#include "bsdfd.h"
#include "common.h"
#include "measured_dev.h"
#include "principled_dev.h"

using namespace principled_dev;
using measured_dev::launch_rows;
using measured_dev::store3;
using measured_dev::Tint;
using measured_dev::TintArg;

namespace {

__device__ __forceinline__ Vec load3(const float* __restrict__ p, long long q) { return Vec{p[3 * q], p[3 * q + 1], p[3 * q + 2]}; }

// eval(): rgb_out = f |cos theta_o| * tint
__global__ __launch_bounds__(256) void principled_eval_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                              const float* __restrict__ wo, long long n, Tint tint,
                                                              float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    float f[3];
    principled_f(d, load3(wi, q), load3(wo, q), f);
    store3(out, q, f[0] * tint.r, f[1] * tint.g, f[2] * tint.b);
}

// the tail of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = f * tint / pdf_sa where
// pdf_sa > 0, firefly rule on channel x, no cosine masks
__global__ __launch_bounds__(256) void principled_weight_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ wo,
                                                                const float* __restrict__ pdf_in,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float thr, float* __restrict__ weight,
                                                                float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    float f[3];
    principled_f(d, load3(wi, q), load3(wo, q), f);
    const float pdf = pdf_in[q];
    const bool act = !active || active[q] != 0;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (act && pdf > 0.0f) { v[0] = f[0] * tint.r / pdf; v[1] = f[1] * tint.g / pdf; v[2] = f[2] * tint.b / pdf; }
    const float p = act && v[0] < thr ? pdf : 0.0f;
    const bool keep = p > 0.0f;
    pdf_out[q] = p;
    store3(weight, q, keep ? v[0] : 0.0f, keep ? v[1] : 0.0f, keep ? v[2] : 0.0f);
}

// sample(): u [N,3] = (sample2.x, sample2.y, sample1)
__global__ __launch_bounds__(256) void principled_sample_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ u,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float* __restrict__ wo_out,
                                                                float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    Vec wo{0.0f, 0.0f, 0.0f};
    float pdf = 0.0f, f[3] = {0.0f, 0.0f, 0.0f};
    if (!active || active[q] != 0) principled_sample(d, load3(wi, q), u[3 * q], u[3 * q + 1], u[3 * q + 2], wo, pdf, f);
    store3(wo_out, q, wo.x, wo.y, wo.z);
    pdf_out[q] = pdf;
    if (weight_out) {
        const bool keep = pdf > 0.0f;
        const float p = keep ? pdf : 1.0f;
        store3(weight_out, q, keep ? f[0] * tint.r / p : 0.0f, keep ? f[1] * tint.g / p : 0.0f, keep ? f[2] * tint.b / p : 0.0f);
    }
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void principled_pdf_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                             const float* __restrict__ wo,
                                                             const unsigned char* __restrict__ active, long long n,
                                                             float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf_out[q] = !active || active[q] != 0 ? principled_pdf(d, load3(wi, q), load3(wo, q)) : 0.0f;
}

// the host path of the four launchers: the descriptor's checks, then `kernel` over N rows
template <class... P, class... A>
int principled_launch(const bsdfd_principled* desc, int64_t n, bool pointers_given, void (*kernel)(P...), void* stream,
                      A... args) {
    if (!desc) return bsdfd_fail_(BSDFD_EINVAL, "null descriptor");
    if (const char* bad = descriptor_error(*desc)) return bsdfd_fail_(BSDFD_EINVAL, bad);
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (((long long)n + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "N too large for one launch");
    return launch_rows(n, pointers_given ? nullptr : "null pointer", kernel, stream, derive(*desc), args...);
}

}  // namespace

extern "C" {

int bsdfd_principled_eval(const bsdfd_principled* desc, const float* wi, const float* wo, int64_t n, const float* tint,
                          float* rgb_out, void* stream) {
    return principled_launch(desc, n, wi && wo && rgb_out, principled_eval_kernel, stream, wi, wo, (long long)n, TintArg{tint},
                             rgb_out);
}

int bsdfd_principled_sample_weight(const bsdfd_principled* desc, const float* wi, const float* wo, const float* pdf_sa,
                                   const unsigned char* active, int64_t n, const float* tint, float firefly_threshold,
                                   float* weight_out, float* pdf_out, void* stream) {
    return principled_launch(desc, n, wi && wo && pdf_sa && weight_out && pdf_out, principled_weight_kernel, stream, wi, wo,
                             pdf_sa, active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

int bsdfd_principled_sample(const bsdfd_principled* desc, const float* wi, const float* u, const unsigned char* active,
                            int64_t n, const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* stream) {
    return principled_launch(desc, n, wi && u && wo_out && pdf_out, principled_sample_kernel, stream, wi, u, active,
                             (long long)n, TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_principled_pdf(const bsdfd_principled* desc, const float* wi, const float* wo, const unsigned char* active, int64_t n,
                         float* pdf_out, void* stream) {
    return principled_launch(desc, n, wi && wo && pdf_out, principled_pdf_kernel, stream, wi, wo, active, (long long)n, pdf_out);
}

}  // extern "C"
