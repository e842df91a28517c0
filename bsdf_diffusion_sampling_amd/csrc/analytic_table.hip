// analytic_table.hip — eval(), sample() and pdf() of a mixed-material wavefront in one launch: the analytic ground truth of the
// full-sphere plugin (principled.hip, dielectric.hip) behind a table of materials.  The analytic counterpart of measured_table.hip.
//
// A renderer's wavefront carries one material id per lane (bsdfd_wf_primary writes them).  Here the lanes stay in LANE order: one
// thread per row loads its id and runs the model the id names, through the same device functions (principled_dev.h,
// dielectric_dev.h) the single-material kernels run — bit for bit what they return (both headers fix where multiply-adds are
// fused).  A record is a kind, a per-material albedo and that kind's derived descriptor, formed on the host when the table is
// created (analytic_host.h: what the single-material launchers derive per call).  Rows without ground truth get a quiet NaN, the
// "use the proxy" value bsdfd_wf_shade reads.
//
// Image-coherent lanes hit the same ball, so most waves carry ONE id: those address the record with a scalar and read it through
// uniform loads, as the single-material kernels read their kernel argument; a wave with mixed ids reads per lane — the kind
// first, then that kind's fields only — and runs the bodies of the kinds it holds under divergence.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "analytic_host.h"
#include "bsdfd.h"
#include "common.h"
#include "dielectric_dev.h"
#include "measured_dev.h"
#include "principled_dev.h"

using dielectric_dev::DielectricDev;
using dielectric_dev::Vec;
using measured_dev::launch_rows;
using measured_dev::store3;
using measured_dev::Tint;
using measured_dev::TintArg;
using principled_dev::PrincipledDev;

namespace {

struct AnalyticRec {
    int kind;          // BSDFD_ANALYTIC_*
    float albedo[3];   // the material's own factor on the call's tint
    union {
        PrincipledDev principled;
        DielectricDev dielectric;
    };
};

// The two models behind one face: f |cos| per channel (the dielectric is grey), the sampler, its density.
struct PrincipledModel {
    const PrincipledDev& d;
    __device__ __forceinline__ void f(const Vec& wi, const Vec& wo, float out[3]) const { principled_dev::principled_f(d, wi, wo, out); }
    __device__ __forceinline__ float pdf(const Vec& wi, const Vec& wo) const { return principled_dev::principled_pdf(d, wi, wo); }
    __device__ __forceinline__ void sample(const Vec& wi, float u0, float u1, float u2, Vec& wo, float& pdf, float f[3]) const {
        principled_dev::principled_sample(d, wi, u0, u1, u2, wo, pdf, f);
    }
};
struct DielectricModel {
    const DielectricDev& d;
    __device__ __forceinline__ void f(const Vec& wi, const Vec& wo, float out[3]) const {
        out[0] = out[1] = out[2] = dielectric_dev::dielectric_f(d, wi, wo);
    }
    __device__ __forceinline__ float pdf(const Vec& wi, const Vec& wo) const { return dielectric_dev::dielectric_pdf(d, wi, wo); }
    __device__ __forceinline__ void sample(const Vec& wi, float u0, float u1, float u2, Vec& wo, float& pdf, float f[3]) const {
        float v = 0.0f;
        dielectric_dev::dielectric_sample(d, wi, u0, u1, u2, wo, pdf, v);
        f[0] = f[1] = f[2] = v;
    }
};

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ Vec load3(const float* __restrict__ p, long long q) { return Vec{p[3 * q], p[3 * q + 1], p[3 * q + 2]}; }

// one record: `row(model, t)` with the lane's effective tint t = tint * albedo (one fp32 product per channel, then used where the
// single-material kernels use tint), `none()` for a slot without ground truth
template <class Row, class None>
__device__ __forceinline__ void with_record(const AnalyticRec& r, Tint tint, Row row, None none) {
    const int kind = r.kind;
    if (kind == BSDFD_ANALYTIC_PRINCIPLED)
        row(PrincipledModel{r.principled}, Tint{tint.r * r.albedo[0], tint.g * r.albedo[1], tint.b * r.albedo[2]});
    else if (kind == BSDFD_ANALYTIC_DIELECTRIC)
        row(DielectricModel{r.dielectric}, Tint{tint.r * r.albedo[0], tint.g * r.albedo[1], tint.b * r.albedo[2]});
    else
        none();
}

// The row's material, once: a wave whose live lanes all carry one id (the first live lane's, held as a scalar) addresses the
// record with that scalar, any other wave per lane.  Call with the dead lanes (rows past N) already retired.
template <class Row, class None>
__device__ __forceinline__ void with_material(const AnalyticRec* __restrict__ table, int n_materials, long long id, Tint tint,
                                              Row row, None none) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)id & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)id >> 32));
    const long long first = (long long)(((unsigned long long)hi << 32) | lo);
    if (__ballot(id != first) == 0ull) {
        if (first >= 0 && first < n_materials) with_record(table[first], tint, row, none);
        else none();
    } else {
        if (id >= 0 && id < n_materials) with_record(table[id], tint, row, none);
        else none();
    }
}

// eval() of row q: f_o = f(wi, wo) |cos| * tint * albedo and, with wl, f_l likewise
__device__ __forceinline__ void eval_table_row(const AnalyticRec* __restrict__ table, int n_materials,
                                               const long long* __restrict__ material_id, const float* __restrict__ wi,
                                               const float* __restrict__ wo, const float* __restrict__ wl, long long q, Tint tint,
                                               float* __restrict__ f_o, float* __restrict__ f_l) {
    const float nan = quiet_nan();
    with_material(table, n_materials, material_id[q], tint,
                  [&](const auto& model, Tint t) {
                      float f[3];
                      model.f(load3(wi, q), load3(wo, q), f);
                      store3(f_o, q, f[0] * t.r, f[1] * t.g, f[2] * t.b);
                      if (wl) {
                          model.f(load3(wi, q), load3(wl, q), f);
                          store3(f_l, q, f[0] * t.r, f[1] * t.g, f[2] * t.b);
                      }
                  },
                  [&] { store3(f_o, q, nan, nan, nan); if (f_l) store3(f_l, q, nan, nan, nan); });
}

// The four kernels: the rows of principled.hip / dielectric.hip over either model; a row without ground truth gets NaN in
// every output (the weight kernel passes its pdf through), whatever its mask says.
__global__ __launch_bounds__(256) void analytic_eval_table_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                  const long long* __restrict__ material_id,
                                                                  const float* __restrict__ wi, const float* __restrict__ wo,
                                                                  const float* __restrict__ wl, long long n, Tint tint,
                                                                  float* __restrict__ f_o, float* __restrict__ f_l) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    eval_table_row(table, n_materials, material_id, wi, wo, wl, q, tint, f_o, f_l);
}

// ... over a row list: thread t serves row rows[t] of the N-row arrays and writes f_o / f_l there only.  Consecutive entries of one
// bucket of a sorted list share their id, so the wave-uniform path serves them as it serves image-coherent lanes.
__global__ __launch_bounds__(256) void analytic_eval_table_rows_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                       const long long* __restrict__ material_id,
                                                                       const float* __restrict__ wi, const float* __restrict__ wo,
                                                                       const float* __restrict__ wl, long long n, Tint tint,
                                                                       float* __restrict__ f_o, float* __restrict__ f_l,
                                                                       const long long* __restrict__ rows, long long n_rows) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows) return;
    const long long q = rows[t];
    if ((unsigned long long)q >= (unsigned long long)n) return;   // (a contract violation: skipped, not followed)
    eval_table_row(table, n_materials, material_id, wi, wo, wl, q, tint, f_o, f_l);
}

// the tail of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = f * tint / pdf_sa where
// pdf_sa > 0, firefly rule on channel x, no cosine masks
__global__ __launch_bounds__(256) void analytic_weight_table_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                    const long long* __restrict__ material_id,
                                                                    const float* __restrict__ wi, const float* __restrict__ wo,
                                                                    const float* __restrict__ pdf_in,
                                                                    const unsigned char* __restrict__ active, long long n,
                                                                    Tint tint, float thr, float* __restrict__ weight,
                                                                    float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float nan = quiet_nan();
    with_material(table, n_materials, material_id[q], tint,
                  [&](const auto& model, Tint t) {
                      float f[3];
                      model.f(load3(wi, q), load3(wo, q), f);
                      const float pdf = pdf_in[q];
                      const bool act = !active || active[q] != 0;
                      float v[3] = {0.0f, 0.0f, 0.0f};
                      if (act && pdf > 0.0f) { v[0] = f[0] * t.r / pdf; v[1] = f[1] * t.g / pdf; v[2] = f[2] * t.b / pdf; }
                      const float p = act && v[0] < thr ? pdf : 0.0f;
                      const bool keep = p > 0.0f;
                      pdf_out[q] = p;
                      store3(weight, q, keep ? v[0] : 0.0f, keep ? v[1] : 0.0f, keep ? v[2] : 0.0f);
                  },
                  [&] { pdf_out[q] = pdf_in[q]; store3(weight, q, nan, nan, nan); });
}

// sample(): u [N,3] = (sample2.x, sample2.y, sample1)
__global__ __launch_bounds__(256) void analytic_sample_table_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                    const long long* __restrict__ material_id,
                                                                    const float* __restrict__ wi, const float* __restrict__ u,
                                                                    const unsigned char* __restrict__ active, long long n,
                                                                    Tint tint, float* __restrict__ wo_out,
                                                                    float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float nan = quiet_nan();
    with_material(table, n_materials, material_id[q], tint,
                  [&](const auto& model, Tint t) {
                      Vec wo{0.0f, 0.0f, 0.0f};
                      float pdf = 0.0f, f[3] = {0.0f, 0.0f, 0.0f};
                      if (!active || active[q] != 0) model.sample(load3(wi, q), u[3 * q], u[3 * q + 1], u[3 * q + 2], wo, pdf, f);
                      store3(wo_out, q, wo.x, wo.y, wo.z);
                      pdf_out[q] = pdf;
                      if (weight_out) {
                          const bool keep = pdf > 0.0f;
                          const float p = keep ? pdf : 1.0f;
                          store3(weight_out, q, keep ? f[0] * t.r / p : 0.0f, keep ? f[1] * t.g / p : 0.0f,
                                 keep ? f[2] * t.b / p : 0.0f);
                      }
                  },
                  [&] { store3(wo_out, q, nan, nan, nan); pdf_out[q] = nan; if (weight_out) store3(weight_out, q, nan, nan, nan); });
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void analytic_pdf_table_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                 const long long* __restrict__ material_id,
                                                                 const float* __restrict__ wi, const float* __restrict__ wo,
                                                                 const unsigned char* __restrict__ active, long long n,
                                                                 float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    with_material(table, n_materials, material_id[q], Tint{1.0f, 1.0f, 1.0f},
                  [&](const auto& model, Tint) {
                      pdf_out[q] = !active || active[q] != 0 ? model.pdf(load3(wi, q), load3(wo, q)) : 0.0f;
                  },
                  [&] { pdf_out[q] = quiet_nan(); });
}

}  // namespace

struct bsdfd_analytic_table_ctx {
    AnalyticRec* dev;  // [n_materials] on the device
    int32_t n_materials;
    int device;
};

namespace {

int table_launch_checks(bsdfd_analytic_table t, int64_t n) {
    if (!t) return bsdfd_fail_(BSDFD_EINVAL, "null analytic table");
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != t->device) return bsdfd_fail_(BSDFD_EINVAL, "analytic table belongs to another device");
    if ((long long)n > 0xffffffffLL - 255) return bsdfd_fail_(BSDFD_EINVAL, "N too large for one launch");   // grid * block < 2^32
    return BSDFD_OK;
}

// the host path of the four launchers: `kernel` over N rows with their ids, `args` behind the table and the ids
template <class... P, class... A>
int table_launch(bsdfd_analytic_table t, int64_t n, const int64_t* material_id, const char* bad, void (*kernel)(P...),
                 void* stream, A... args) {
    if (int rc = table_launch_checks(t, n)) return rc;
    return launch_rows(n, bad, kernel, stream, static_cast<const AnalyticRec*>(t->dev), (int)t->n_materials,
                       reinterpret_cast<const long long*>(material_id), args...);
}

}  // namespace

extern "C" {

int bsdfd_analytic_table_create(const bsdfd_analytic_entry* entries, int32_t n_materials, bsdfd_analytic_table* out) {
    if (!out) return bsdfd_fail_(BSDFD_EINVAL, "null argument");
    *out = nullptr;
    if (!entries) return bsdfd_fail_(BSDFD_EINVAL, "null entry array");
    if (n_materials < 1 || n_materials > 65536) return bsdfd_fail_(BSDFD_EINVAL, "n_materials must be in [1, 65536]");
    std::vector<AnalyticRec> host((size_t)n_materials);
    bool any = false;
    for (int32_t m = 0; m < n_materials; ++m) {
        const bsdfd_analytic_entry& e = entries[m];
        AnalyticRec& r = host[(size_t)m];
        const std::string who = "analytic table entry " + std::to_string(m) + ": ";
        r = AnalyticRec{};
        r.kind = e.kind;
        const char* bad = nullptr;
        if (e.kind == BSDFD_ANALYTIC_PRINCIPLED) {
            if (!(bad = principled_dev::descriptor_error(e.desc.principled))) r.principled = principled_dev::derive(e.desc.principled);
        } else if (e.kind == BSDFD_ANALYTIC_DIELECTRIC) {
            if (!(bad = dielectric_dev::descriptor_error(e.desc.dielectric))) r.dielectric = dielectric_dev::derive(e.desc.dielectric);
        } else if (e.kind != BSDFD_ANALYTIC_NONE) {
            bad = "kind must be BSDFD_ANALYTIC_NONE, _PRINCIPLED or _DIELECTRIC";
        }
        if (bad) return bsdfd_fail_(BSDFD_EINVAL, who + bad);
        for (int k = 0; k < 3; ++k) {
            if (!(e.albedo[k] >= 0.0f && std::isfinite(e.albedo[k])))   // (false for NaN)
                return bsdfd_fail_(BSDFD_EINVAL, who + "albedo must be finite and >= 0");
            r.albedo[k] = e.albedo[k];
        }
        any = any || e.kind != BSDFD_ANALYTIC_NONE;
    }
    if (!any) return bsdfd_fail_(BSDFD_EINVAL, "an analytic table needs at least one material with ground truth");
    int devid = -1;
    HIP_TRY(hipGetDevice(&devid));
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, host.size() * sizeof(AnalyticRec)));
    const hipError_t err = hipMemcpy(p, host.data(), host.size() * sizeof(AnalyticRec), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(p);
        return bsdfd_fail_(BSDFD_EHIP, std::string("hipMemcpy of the material records: ") + hipGetErrorString(err));
    }
    *out = new bsdfd_analytic_table_ctx{static_cast<AnalyticRec*>(p), n_materials, devid};
    return BSDFD_OK;
}

void bsdfd_analytic_table_destroy(bsdfd_analytic_table t) {
    if (!t) return;
    (void)hipFree(t->dev);
    delete t;
}

int bsdfd_analytic_eval_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                              const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, void* stream) {
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o ? "null pointer" : nullptr;
    return table_launch(t, n, material_id, bad, analytic_eval_table_kernel, stream, wi, wo, wl, (long long)n, TintArg{tint},
                        f_o, f_l);
}

int bsdfd_analytic_eval_table_rows(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                                   const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, const int64_t* rows,
                                   int64_t n_rows, void* stream) {
    if (int rc = table_launch_checks(t, n)) return rc;
    if (n_rows < 0 || n_rows > n) return bsdfd_fail_(BSDFD_EINVAL, "n_rows must be in [0, N]");
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o || !rows ? "null pointer" : nullptr;
    return launch_rows(n_rows, bad, analytic_eval_table_rows_kernel, stream, static_cast<const AnalyticRec*>(t->dev),
                       (int)t->n_materials, reinterpret_cast<const long long*>(material_id), wi, wo, wl, (long long)n, TintArg{tint},
                       f_o, f_l, reinterpret_cast<const long long*>(rows), (long long)n_rows);
}

int bsdfd_analytic_sample_weight_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi,
                                       const float* wo, const float* pdf_sa, const unsigned char* active, int64_t n,
                                       const float* tint, float firefly_threshold, float* weight_out, float* pdf_out,
                                       void* stream) {
    const bool given = material_id && wi && wo && pdf_sa && weight_out && pdf_out;
    return table_launch(t, n, material_id, given ? nullptr : "null pointer", analytic_weight_table_kernel, stream, wi, wo, pdf_sa,
                        active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

int bsdfd_analytic_sample_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* u,
                                const unsigned char* active, int64_t n, const float* tint, float* wo_out, float* pdf_out,
                                float* weight_out, void* stream) {
    const bool given = material_id && wi && u && wo_out && pdf_out;
    return table_launch(t, n, material_id, given ? nullptr : "null pointer", analytic_sample_table_kernel, stream, wi, u, active,
                        (long long)n, TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_analytic_pdf_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                             const unsigned char* active, int64_t n, float* pdf_out, void* stream) {
    const bool given = material_id && wi && wo && pdf_out;
    return table_launch(t, n, material_id, given ? nullptr : "null pointer", analytic_pdf_table_kernel, stream, wi, wo, active,
                        (long long)n, pdf_out);
}

}  // extern "C"
