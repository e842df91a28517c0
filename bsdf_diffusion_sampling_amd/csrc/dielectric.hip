// dielectric.hip — the analytic ground truth of the full-sphere plugin: Mitsuba's `roughdielectric` restated (Walter et al. 2007).
//
// The reference's full-sphere plugin evaluates an analytic Mitsuba BSDF for its eval(), sample weight and firefly rule
// (rendering/bsdf_myresult.py:97-110); entries 23..25 of its material list (rendering/utils/bsdf_dict.py) are rough dielectrics.
// Four kernels, one row per lane, over the device functions of dielectric_dev.h: eval, the tail of the plugin's sample()
// (weight + firefly rule), the model's own importance sampler, and its pdf.  No tables, no handle: the material is a
// 16-byte descriptor passed by value.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "analytic_host.h"
#include "bsdfd.h"
#include "common.h"
#include "dielectric_dev.h"
#include "measured_dev.h"

using namespace dielectric_dev;
using measured_dev::launch_rows;
using measured_dev::store3;
using measured_dev::Tint;
using measured_dev::TintArg;

namespace {

__device__ __forceinline__ Vec load3(const float* __restrict__ p, long long q) { return Vec{p[3 * q], p[3 * q + 1], p[3 * q + 2]}; }

// eval(): rgb_out = f |cos theta_o| * tint
__global__ __launch_bounds__(256) void dielectric_eval_kernel(DielectricDev d, const float* __restrict__ wi,
                                                              const float* __restrict__ wo, long long n, Tint tint,
                                                              float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float f = dielectric_f(d, load3(wi, q), load3(wo, q));
    store3(out, q, f * tint.r, f * tint.g, f * tint.b);
}

// the tail of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = f * tint / pdf_sa where
// pdf_sa > 0, firefly rule on channel x, no cosine masks
__global__ __launch_bounds__(256) void dielectric_weight_kernel(DielectricDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ wo,
                                                                const float* __restrict__ pdf_in,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float thr, float* __restrict__ weight,
                                                                float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float f = dielectric_f(d, load3(wi, q), load3(wo, q));
    const float pdf = pdf_in[q];
    const bool act = !active || active[q] != 0;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (act && pdf > 0.0f) { v[0] = f * tint.r / pdf; v[1] = f * tint.g / pdf; v[2] = f * tint.b / pdf; }
    const float p = act && v[0] < thr ? pdf : 0.0f;
    const bool keep = p > 0.0f;
    pdf_out[q] = p;
    store3(weight, q, keep ? v[0] : 0.0f, keep ? v[1] : 0.0f, keep ? v[2] : 0.0f);
}

// sample(): u [N,3] = (sample2.x, sample2.y, sample1)
__global__ __launch_bounds__(256) void dielectric_sample_kernel(DielectricDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ u,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float* __restrict__ wo_out,
                                                                float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    Vec wo{0.0f, 0.0f, 0.0f};
    float pdf = 0.0f, f = 0.0f;
    if (!active || active[q] != 0) dielectric_sample(d, load3(wi, q), u[3 * q], u[3 * q + 1], u[3 * q + 2], wo, pdf, f);
    store3(wo_out, q, wo.x, wo.y, wo.z);
    pdf_out[q] = pdf;
    if (weight_out) {
        const bool keep = pdf > 0.0f;   // (f is 0 already where the lobe's side test failed)
        const float p = keep ? pdf : 1.0f;
        store3(weight_out, q, keep ? f * tint.r / p : 0.0f, keep ? f * tint.g / p : 0.0f, keep ? f * tint.b / p : 0.0f);
    }
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void dielectric_pdf_kernel(DielectricDev d, const float* __restrict__ wi,
                                                             const float* __restrict__ wo,
                                                             const unsigned char* __restrict__ active, long long n,
                                                             float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf_out[q] = !active || active[q] != 0 ? dielectric_pdf(d, load3(wi, q), load3(wo, q)) : 0.0f;
}

// the host path of the four launchers: the descriptor's checks, then `kernel` over N rows
template <class... P, class... A>
int dielectric_launch(const bsdfd_dielectric* desc, int64_t n, bool pointers_given, void (*kernel)(P...), void* stream,
                      A... args) {
    if (!desc) return bsdfd_fail_(BSDFD_EINVAL, "null descriptor");
    if (const char* bad = descriptor_error(*desc)) return bsdfd_fail_(BSDFD_EINVAL, bad);
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (((long long)n + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "N too large for one launch");
    return launch_rows(n, pointers_given ? nullptr : "null pointer", kernel, stream, derive(*desc), args...);
}

}  // namespace

extern "C" {

int bsdfd_dielectric_eval(const bsdfd_dielectric* desc, const float* wi, const float* wo, int64_t n, const float* tint,
                          float* rgb_out, void* stream) {
    return dielectric_launch(desc, n, wi && wo && rgb_out, dielectric_eval_kernel, stream, wi, wo, (long long)n, TintArg{tint},
                             rgb_out);
}

int bsdfd_dielectric_sample_weight(const bsdfd_dielectric* desc, const float* wi, const float* wo, const float* pdf_sa,
                                   const unsigned char* active, int64_t n, const float* tint, float firefly_threshold,
                                   float* weight_out, float* pdf_out, void* stream) {
    return dielectric_launch(desc, n, wi && wo && pdf_sa && weight_out && pdf_out, dielectric_weight_kernel, stream, wi, wo,
                             pdf_sa, active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

int bsdfd_dielectric_sample(const bsdfd_dielectric* desc, const float* wi, const float* u, const unsigned char* active,
                            int64_t n, const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* stream) {
    return dielectric_launch(desc, n, wi && u && wo_out && pdf_out, dielectric_sample_kernel, stream, wi, u, active,
                             (long long)n, TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_dielectric_pdf(const bsdfd_dielectric* desc, const float* wi, const float* wo, const unsigned char* active, int64_t n,
                         float* pdf_out, void* stream) {
    return dielectric_launch(desc, n, wi && wo && pdf_out, dielectric_pdf_kernel, stream, wi, wo, active, (long long)n, pdf_out);
}

}  // extern "C"
