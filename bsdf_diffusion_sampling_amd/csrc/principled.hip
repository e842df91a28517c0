// principled.hip — the analytic ground truth of the full-sphere plugin for bsdf_0..22: Mitsuba's `principled` restated.
//
// The reference's full-sphere plugin evaluates an analytic Mitsuba BSDF for its eval(), sample weight and firefly rule
// (rendering/bsdf_myresult.py:97-110); entries 0..22 of its material list (rendering/utils/bsdf_dict.py) are principled BSDFs.
// Four kernels, one row per lane: eval, the tail of the plugin's sample() (weight + firefly rule), the model's own importance
// sampler, and its pdf.  The rows are analytic_rows.h's, shared with dielectric.hip and analytic_table.hip, over the device
// functions of principled_dev.h.  No tables, no handle: the material is a 64-byte descriptor read on the host at the call; what
// depends on it alone is derived there, once (analytic_host.h), and passed by value.
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
__global__ __launch_bounds__(256) void principled_eval_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                              const float* __restrict__ wo, long long n, Tint tint,
                                                              float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    eval_row(PrincipledModel{d}, wi, wo, nullptr, q, tint, out, nullptr);
}

// the tail of the full-sphere plugin's sample(): weight = f * tint / pdf_sa with the firefly rule
__global__ __launch_bounds__(256) void principled_weight_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ wo,
                                                                const float* __restrict__ pdf_in,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float thr, float* __restrict__ weight,
                                                                float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    weight_row(PrincipledModel{d}, wi, wo, pdf_in, active, q, tint, thr, weight, pdf_out);
}

// sample(): the model's own importance sampler, one query per lane
__global__ __launch_bounds__(256) void principled_sample_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                                const float* __restrict__ u,
                                                                const unsigned char* __restrict__ active, long long n,
                                                                Tint tint, float* __restrict__ wo_out,
                                                                float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    sample_row(PrincipledModel{d}, wi, u, active, q, tint, wo_out, pdf_out, weight_out);
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void principled_pdf_kernel(PrincipledDev d, const float* __restrict__ wi,
                                                             const float* __restrict__ wo,
                                                             const unsigned char* __restrict__ active, long long n,
                                                             float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf_row(PrincipledModel{d}, wi, wo, active, q, pdf_out);
}

// the host path of the four launchers: the descriptor's checks, then `kernel` over N rows
template <class... P, class... A>
int principled_launch(const bsdfd_principled* desc, int64_t n, bool pointers_given, void (*kernel)(P...), void* stream,
                      A... args) {
    if (!desc) return bsdfd_fail_(BSDFD_EINVAL, "null descriptor");
    if (const char* bad = principled_dev::descriptor_error(*desc)) return bsdfd_fail_(BSDFD_EINVAL, bad);
    if (int rc = rows::launch_checks(n, rows::kMaxRowsSingle)) return rc;
    return launch_rows(n, pointers_given ? nullptr : "null pointer", kernel, stream, principled_dev::derive(*desc), args...);
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
