// dielectric.hip — the analytic ground truth of the full-sphere plugin: Mitsuba's `roughdielectric` restated (Walter et al. 2007).
//
// The reference's full-sphere plugin evaluates an analytic Mitsuba BSDF for its eval(), sample weight and firefly rule
// (rendering/bsdf_myresult.py:97-110); entries 23..25 of its material list (rendering/utils/bsdf_dict.py) are rough dielectrics.
// Four kernels, one row per lane: eval, the tail of the plugin's sample() (weight + firefly rule), the model's own importance
// sampler, and its pdf.  The rows are analytic_rows.h's, shared with principled.hip and analytic_table.hip, over the device
// functions of dielectric_dev.h.  No tables, no handle: the material is a 16-byte descriptor passed by value.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "analytic_host.h"
#include "analytic_rows.h"
#include "bsdfd.h"
#include "common.h"

using namespace analytic_rows;
using rows::launch_rows;
using rows::TintArg;

namespace {

// eval(): rgb_out = f |cos theta_o| * tint
__global__ __launch_bounds__(256) void dielectric_eval_kernel(DielectricDev d, const float* __restrict__ wi,
                                                              const float* __restrict__ wo, long long n, Tint tint,
                                                              float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    eval_row(DielectricModel{d}, wi, wo, nullptr, q, tint, out, nullptr);
}

// the tail of the full-sphere plugin's sample(): weight = f * tint / pdf_sa with the firefly rule
__global__ __launch_bounds__(256) void dielectric_weight_kernel(DielectricDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ wo,
                                                                const float* __restrict__ pdf_in,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float thr, float* __restrict__ weight,
                                                                float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    weight_row(DielectricModel{d}, wi, wo, pdf_in, active, q, tint, thr, weight, pdf_out);
}

// sample(): the model's own importance sampler, one query per lane
__global__ __launch_bounds__(256) void dielectric_sample_kernel(DielectricDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ u,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float* __restrict__ wo_out,
                                                                float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    sample_row(DielectricModel{d}, wi, u, active, q, tint, wo_out, pdf_out, weight_out);
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void dielectric_pdf_kernel(DielectricDev d, const float* __restrict__ wi,
                                                             const float* __restrict__ wo,
                                                             const unsigned char* __restrict__ active, long long n,
                                                             float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf_row(DielectricModel{d}, wi, wo, active, q, pdf_out);
}

// the host path of the four launchers: the descriptor's checks, then `kernel` over N rows
template <class... P, class... A>
int dielectric_launch(const bsdfd_dielectric* desc, int64_t n, bool pointers_given, void (*kernel)(P...), void* stream,
                      A... args) {
    if (!desc) return bsdfd_fail_(BSDFD_EINVAL, "null descriptor");
    if (const char* bad = dielectric_dev::descriptor_error(*desc)) return bsdfd_fail_(BSDFD_EINVAL, bad);
    if (int rc = rows::launch_checks(n, rows::kMaxRowsSingle)) return rc;
    return launch_rows(n, pointers_given ? nullptr : "null pointer", kernel, stream, dielectric_dev::derive(*desc), args...);
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
