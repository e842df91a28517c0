// analytic_table.hip — eval(), sample() and pdf() of a mixed-material wavefront in one launch: the analytic ground truth of the
// full-sphere plugin (principled.hip, dielectric.hip) behind a table of materials.  The analytic counterpart of measured_table.hip.
//
// A renderer's wavefront carries one material id per lane (bsdfd_wf_primary writes them).  Here the lanes stay in LANE order: one
// thread per row loads its id and runs the model the id names, through the same row functions (analytic_rows.h) the
// single-material kernels run — bit for bit what they return (the models' headers fix where multiply-adds are fused).  A record
// is a kind, a per-material albedo and that kind's derived descriptor, formed on the host when the table is created
// (analytic_host.h: what the single-material launchers derive per call).  Rows without ground truth get a quiet NaN, the "use the
// proxy" value bsdfd_wf_shade reads.
//
// Image-coherent lanes hit the same ball, so most waves carry ONE id: those address the record with a scalar and read it through
// uniform loads, as the single-material kernels read their kernel argument; a wave with mixed ids reads per lane — the kind
// first, then that kind's fields only — and runs the bodies of the kinds it holds under divergence.  That pick, and the host side
// of a table of materials, are material_table.h's, shared with measured_table.hip.
//
// The table also answers for a path tracer's vertices INSIDE a ball (bsdfd_wf_sample_inside / _rows, below): there the models' own
// samplers stand in for the flow nets.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "analytic_host.h"
#include "analytic_rows.h"
#include "bounce_dev.h"
#include "bsdfd.h"
#include "common.h"
#include "material_table.h"

using namespace analytic_rows;
using rows::quiet_nan;
using rows::TintArg;

namespace {

struct AnalyticRec {
    int kind;          // BSDFD_ANALYTIC_*
    float albedo[3];   // the material's own factor on the call's tint
    union {
        PrincipledDev principled;
        DielectricDev dielectric;
    };
};

}  // namespace

struct bsdfd_analytic_table_ctx : material_table::Ctx<AnalyticRec> {
    static constexpr const char* noun = "analytic table";
};

namespace {

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

// the row's material (material_table.h: with_entry), then with_record; an id outside the table is a row without ground truth.
// Call with the dead lanes (rows past N) already retired.
template <class Row, class None>
__device__ __forceinline__ void with_material(const AnalyticRec* __restrict__ table, int n_materials, long long id, Tint tint,
                                              Row row, None none) {
    material_table::with_entry(table, n_materials, id, [](const AnalyticRec&) { return true; },
                               [&](const AnalyticRec& r) { with_record(r, tint, row, none); }, none);
}

// eval() of row q: f_o = f(wi, wo) |cos| * tint * albedo and, with wl, f_l likewise
__device__ __forceinline__ void eval_table_row(const AnalyticRec* __restrict__ table, int n_materials,
                                               const long long* __restrict__ material_id, const float* __restrict__ wi,
                                               const float* __restrict__ wo, const float* __restrict__ wl, long long q, Tint tint,
                                               float* __restrict__ f_o, float* __restrict__ f_l) {
    const float nan = quiet_nan();
    with_material(table, n_materials, material_id[q], tint,
                  [&](const auto& model, Tint t) { eval_row(model, wi, wo, wl, q, t, f_o, f_l); },
                  [&] { store3(f_o, q, nan, nan, nan); if (f_l) store3(f_l, q, nan, nan, nan); });
}

// The four kernels: the rows of analytic_rows.h, which principled.hip and dielectric.hip run too, over either model; a row
// without ground truth gets NaN in every output (the weight kernel passes its pdf through), whatever its mask says.
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
    long long q;
    if (!material_table::listed_row(rows, n_rows, n, q)) return;
    eval_table_row(table, n_materials, material_id, wi, wo, wl, q, tint, f_o, f_l);
}

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
                  [&](const auto& model, Tint t) { weight_row(model, wi, wo, pdf_in, active, q, t, thr, weight, pdf_out); },
                  [&] { pdf_out[q] = pdf_in[q]; store3(weight, q, nan, nan, nan); });
}

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
                  [&](const auto& model, Tint t) { sample_row(model, wi, u, active, q, t, wo_out, pdf_out, weight_out); },
                  [&] { store3(wo_out, q, nan, nan, nan); pdf_out[q] = nan; if (weight_out) store3(weight_out, q, nan, nan, nan); });
}

__global__ __launch_bounds__(256) void analytic_pdf_table_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                                 const long long* __restrict__ material_id,
                                                                 const float* __restrict__ wi, const float* __restrict__ wo,
                                                                 const unsigned char* __restrict__ active, long long n,
                                                                 float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    with_material(table, n_materials, material_id[q], Tint{1.0f, 1.0f, 1.0f},
                  [&](const auto& model, Tint) { pdf_row(model, wi, wo, active, q, pdf_out); },
                  [&] { pdf_out[q] = quiet_nan(); });
}

// The sampler's answer for the vertices INSIDE a ball (wi.z < 0: the transmitting bounce of bounce_dev.h got them there), where the
// flow nets have none worth keeping: the model's own importance sampler draws wo and states its density, and its density for the
// light strategy's direction wl — sample_row's and pdf_row's statements on the lane's material, with variates of the lane's own,
// u_k = (word k >> 8) 2^-24 of tagged_draw(.., "Insd", bounce), exact fp32 numbers keyed by the lane like "Roul" and "Envm".  A
// sample the model itself weights with 0 — its f |cos| is 0 in every channel: the dielectric's wo on the wrong side for the lobe that
// drew it — gets pdf_o = 0, because the bounce forms its own weight, f(wi, wo) / pdf_o, from the PAIR: pdf(wi, wo) classifies the
// pair by its sides, so for such a wo it is the other lobe's density and the pair's f is not 0; followed, those samples would count
// that lobe's directions twice (a glass ball in a white furnace came out 1.4 % too bright).  Dropped, the strategy's density for the
// directions it does contribute is the model's pdf, which is what pdf_l states for wl.  A record without ground truth gets zeros.
// Both end the path at the bounce.  Every other lane — floor, ended, outside (wi.z >= 0),
// unlisted — keeps every byte.  LIST: thread t serves lane rows[t].
template <bool LIST>
__global__ __launch_bounds__(256) void sample_inside_kernel(const AnalyticRec* __restrict__ table, int n_materials,
                                                            const long long* __restrict__ material_id, const float* __restrict__ wi,
                                                            const float* __restrict__ wl, long long n, int bounce,
                                                            unsigned long long seed, unsigned long long pass,
                                                            unsigned long long path_offset, float* __restrict__ wo_out,
                                                            float* __restrict__ pdf_o, float* __restrict__ pdf_l,
                                                            const long long* __restrict__ rows, long long n_rows) {
    long long q;
    if constexpr (LIST) {
        if (!material_table::listed_row(rows, n_rows, n, q)) return;
    } else {
        q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (q >= n) return;
    }
    const long long id = material_id[q];
    if (!(id >= 0 && id < n_materials) || !(wi[3 * q + 2] < 0.0f)) return;
    unsigned w[4];
    bounce_dev::tagged_draw(seed, pass, path_offset, q, 0x496E7364u /* "Insd" */, bounce, w);
    const float u0 = (float)(w[0] >> 8) * (1.0f / 16777216.0f), u1 = (float)(w[1] >> 8) * (1.0f / 16777216.0f),
                u2 = (float)(w[2] >> 8) * (1.0f / 16777216.0f);
    with_material(table, n_materials, id, Tint{1.0f, 1.0f, 1.0f},
                  [&](const auto& model, Tint) {
                      const Vec i = load3(wi, q);
                      Vec o{0.0f, 0.0f, 0.0f};
                      float pdf = 0.0f, f[3] = {0.0f, 0.0f, 0.0f};
                      model.sample(i, u0, u1, u2, o, pdf, f);
                      const float pl = model.pdf(i, load3(wl, q));
                      store3(wo_out, q, o.x, o.y, o.z);
                      pdf_o[q] = fmaxf(fmaxf(f[0], f[1]), f[2]) > 0.0f ? pdf : 0.0f;
                      pdf_l[q] = pl;
                  },
                  [&] { store3(wo_out, q, 0.0f, 0.0f, 0.0f); pdf_o[q] = 0.0f; pdf_l[q] = 0.0f; });
}

// the checks the two forms share, before the table's own
inline const char* sample_inside_complaint(int32_t bounce, const int64_t* material_id, const float* wi, const float* wl,
                                           const float* wo, const float* pdf_o, const float* pdf_l, bool rows_given) {
    return bounce < 0 ? "bounce must be >= 0"
           : !material_id || !wi || !wl || !wo || !pdf_o || !pdf_l || !rows_given ? "null pointer" : nullptr;
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
    return material_table::upload(host, devid, "records", out);
}

void bsdfd_analytic_table_destroy(bsdfd_analytic_table t) { material_table::destroy(t); }

int bsdfd_analytic_eval_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                              const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, void* stream) {
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o ? "null pointer" : nullptr;
    return material_table::launch(t, n, n, material_id, bad, analytic_eval_table_kernel, stream, wi, wo, wl, (long long)n,
                                  TintArg{tint}, f_o, f_l);
}

int bsdfd_analytic_eval_table_rows(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                                   const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, const int64_t* rows,
                                   int64_t n_rows, void* stream) {
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o || !rows ? "null pointer" : nullptr;
    return material_table::launch(t, n, n_rows, material_id, bad, analytic_eval_table_rows_kernel, stream, wi, wo, wl,
                                  (long long)n, TintArg{tint}, f_o, f_l, reinterpret_cast<const long long*>(rows),
                                  (long long)n_rows);
}

int bsdfd_analytic_sample_weight_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi,
                                       const float* wo, const float* pdf_sa, const unsigned char* active, int64_t n,
                                       const float* tint, float firefly_threshold, float* weight_out, float* pdf_out,
                                       void* stream) {
    const bool given = material_id && wi && wo && pdf_sa && weight_out && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", analytic_weight_table_kernel, stream, wi,
                                  wo, pdf_sa, active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

int bsdfd_analytic_sample_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* u,
                                const unsigned char* active, int64_t n, const float* tint, float* wo_out, float* pdf_out,
                                float* weight_out, void* stream) {
    const bool given = material_id && wi && u && wo_out && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", analytic_sample_table_kernel, stream, wi,
                                  u, active, (long long)n, TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_analytic_pdf_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                             const unsigned char* active, int64_t n, float* pdf_out, void* stream) {
    const bool given = material_id && wi && wo && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", analytic_pdf_table_kernel, stream, wi, wo,
                                  active, (long long)n, pdf_out);
}

int bsdfd_wf_sample_inside(bsdfd_analytic_table t, int32_t bounce, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t n,
                           const int64_t* material_id, const float* wi, const float* wl, float* wo, float* pdf_o, float* pdf_l,
                           void* stream) {
    return material_table::launch(t, n, n, material_id, sample_inside_complaint(bounce, material_id, wi, wl, wo, pdf_o, pdf_l, true),
                                  sample_inside_kernel<false>, stream, wi, wl, (long long)n, (int)bounce, (unsigned long long)seed,
                                  (unsigned long long)pass, (unsigned long long)path_offset, wo, pdf_o, pdf_l,
                                  (const long long*)nullptr, 0LL);
}

int bsdfd_wf_sample_inside_rows(bsdfd_analytic_table t, int32_t bounce, uint64_t seed, uint64_t pass, uint64_t path_offset,
                                int64_t n, const int64_t* material_id, const float* wi, const float* wl, float* wo, float* pdf_o,
                                float* pdf_l, const int64_t* rows, int64_t n_rows, void* stream) {
    return material_table::launch(t, n, n_rows, material_id,
                                  sample_inside_complaint(bounce, material_id, wi, wl, wo, pdf_o, pdf_l, rows != nullptr),
                                  sample_inside_kernel<true>, stream, wi, wl, (long long)n, (int)bounce, (unsigned long long)seed,
                                  (unsigned long long)pass, (unsigned long long)path_offset, wo, pdf_o, pdf_l,
                                  reinterpret_cast<const long long*>(rows), (long long)n_rows);
}

}  // extern "C"
