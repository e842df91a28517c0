// measured_table.hip — eval(), sample() and pdf() of a mixed-material wavefront in one launch: the RGL evaluator of measured.hip behind a
// table of materials.
//
// A renderer's wavefront carries one material id per lane (bsdfd_wf_primary writes them).  Serving eval() through
// bsdfd_measured_eval takes one launch per material on gathered slices; the evaluator is latency-bound (~60 dependent
// gathers per pair from L2-resident tables), so many small launches are its worst case.  Here the lanes stay in LANE order:
// one thread per row loads its id and evaluates the material the id names, through the same row functions (measured_dev.h)
// the single-material kernels run — bit for bit what they return (measured_dev.h fixes where multiply-adds are fused).
// Rows without ground truth get a quiet NaN, the "use the proxy" value bsdfd_wf_shade reads.
//
// Image-coherent lanes hit the same ball, so most waves carry ONE id: those take a wave-uniform path on which the descriptor
// is addressed by a scalar and travels through uniform loads, as the kernel argument of the single-material kernel does;
// waves with mixed ids load the descriptor's fields per lane.  That pick, and the host side of a table of materials, are
// material_table.h's, shared with analytic_table.hip.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "measured_dev.h"
#include "material_table.h"

using namespace measured_dev;
using material_table::with_entry;
using rows::quiet_nan;

struct bsdfd_measured_table_ctx : material_table::Ctx<MeasuredDev> {   // a slot without ground truth is all zero
    static constexpr const char* noun = "measured table";
};

namespace {

// The device array holds MeasuredDev records, read here through a mirror type whose pointers are typed as GLOBAL pointers: a
// pointer loaded from memory could point anywhere as far as the compiler knows, and the tables would be read with flat loads;
// the single-material kernels get the descriptor as a kernel argument, whose pointers are known to be global.
typedef const __attribute__((address_space(1))) float* gptr;
struct TableG {
    gptr data;
    int w, h;
};
struct MeasuredDevG {
    gptr phi_i, theta_i;
    int n_phi, n_theta;
    int isotropic, jacobian, reduction;
    float fold_x, fold_y;
    TableG ndf, sigma, vndf, rgb;
    gptr vndf_cond, vndf_marg;
    TableG lum;
    gptr lum_cond, lum_marg;
};
static_assert(sizeof(MeasuredDevG) == sizeof(MeasuredDev) && alignof(MeasuredDevG) == alignof(MeasuredDev) &&
              offsetof(MeasuredDevG, fold_y) == offsetof(MeasuredDev, fold_y) && offsetof(MeasuredDevG, rgb) == offsetof(MeasuredDev, rgb) &&
              offsetof(MeasuredDevG, vndf_marg) == offsetof(MeasuredDev, vndf_marg) && offsetof(MeasuredDevG, lum) == offsetof(MeasuredDev, lum) &&
              offsetof(MeasuredDevG, lum_marg) == offsetof(MeasuredDev, lum_marg), "MeasuredDevG mirrors MeasuredDev");

__device__ __forceinline__ Table generic(const TableG& t) { return Table{(const float*)t.data, t.w, t.h}; }
__device__ __forceinline__ MeasuredDev generic(const MeasuredDevG& s) {
    MeasuredDev m;
    m.phi_i = (const float*)s.phi_i; m.theta_i = (const float*)s.theta_i;
    m.n_phi = s.n_phi; m.n_theta = s.n_theta;
    m.isotropic = s.isotropic; m.jacobian = s.jacobian; m.reduction = s.reduction;
    m.fold_x = s.fold_x; m.fold_y = s.fold_y;
    m.ndf = generic(s.ndf); m.sigma = generic(s.sigma); m.vndf = generic(s.vndf); m.rgb = generic(s.rgb);
    m.vndf_cond = (const float*)s.vndf_cond; m.vndf_marg = (const float*)s.vndf_marg;
    m.lum = generic(s.lum); m.lum_cond = (const float*)s.lum_cond; m.lum_marg = (const float*)s.lum_marg;
    return m;
}

// slot of a material without ground truth: all zero (no tables)
__device__ __forceinline__ bool has_ground_truth(const MeasuredDevG& m) { return m.rgb.data != nullptr; }

// eval() of row q by the material its id names (material_table.h: with_entry; a slot that has_ground_truth serves the row)
__device__ __forceinline__ void eval_table_row(const MeasuredDevG* __restrict__ table, int n_materials,
                                               const long long* __restrict__ material_id, const float* __restrict__ wi,
                                               const float* __restrict__ wo, const float* __restrict__ wl, long long q, Tint tint,
                                               float* __restrict__ f_o, float* __restrict__ f_l) {
    const float nan = quiet_nan();
    with_entry(table, n_materials, material_id[q], has_ground_truth,
               [&](const MeasuredDevG& g) { eval_row(generic(g), wi, wo, wl, q, tint, f_o, f_l); },
               [&] { store3(f_o, q, nan, nan, nan); if (f_l) store3(f_l, q, nan, nan, nan); });
}

// The four kernels: the rows of measured_dev.h, which the single-material kernels (measured.hip) run too; a row without
// ground truth gets NaN in every output (the weight kernel passes its pdf through).
__global__ __launch_bounds__(256) void measured_eval_table_kernel(const MeasuredDevG* __restrict__ table, int n_materials,
                                                                  const long long* __restrict__ material_id,
                                                                  const float* __restrict__ wi,
                                                                  const float* __restrict__ wo,
                                                                  const float* __restrict__ wl, long long n, Tint tint,
                                                                  float* __restrict__ f_o, float* __restrict__ f_l) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    eval_table_row(table, n_materials, material_id, wi, wo, wl, q, tint, f_o, f_l);
}

// ... over a row list: thread t serves row rows[t] of the N-row arrays and writes f_o / f_l there only.  Consecutive entries of one
// bucket of a sorted list share their id, so the wave-uniform path serves them as it serves image-coherent lanes.
__global__ __launch_bounds__(256) void measured_eval_table_rows_kernel(const MeasuredDevG* __restrict__ table, int n_materials,
                                                                       const long long* __restrict__ material_id,
                                                                       const float* __restrict__ wi,
                                                                       const float* __restrict__ wo,
                                                                       const float* __restrict__ wl, long long n, Tint tint,
                                                                       float* __restrict__ f_o, float* __restrict__ f_l,
                                                                       const long long* __restrict__ rows, long long n_rows) {
    long long q;
    if (!material_table::listed_row(rows, n_rows, n, q)) return;
    eval_table_row(table, n_materials, material_id, wi, wo, wl, q, tint, f_o, f_l);
}

__global__ __launch_bounds__(256) void measured_weight_table_kernel(const MeasuredDevG* __restrict__ table, int n_materials,
                                                                    const long long* __restrict__ material_id,
                                                                    const float* __restrict__ wi,
                                                                    const float* __restrict__ wo,
                                                                    const float* __restrict__ pdf_in,
                                                                    const unsigned char* __restrict__ active, long long n,
                                                                    Tint tint, float thr, float* __restrict__ weight,
                                                                    float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float nan = quiet_nan();
    with_entry(table, n_materials, material_id[q], has_ground_truth,
               [&](const MeasuredDevG& g) { weight_row(generic(g), wi, wo, pdf_in, active, q, tint, thr, weight, pdf_out); },
               [&] { pdf_out[q] = pdf_in[q]; store3(weight, q, nan, nan, nan); });
}

__global__ __launch_bounds__(256) void measured_sample_table_kernel(const MeasuredDevG* __restrict__ table, int n_materials,
                                                                    const long long* __restrict__ material_id,
                                                                    const float* __restrict__ wi, const float* __restrict__ u,
                                                                    const unsigned char* __restrict__ active, long long n,
                                                                    Tint tint, float* __restrict__ wo_out,
                                                                    float* __restrict__ pdf_out,
                                                                    float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float nan = quiet_nan();
    with_entry(table, n_materials, material_id[q], has_ground_truth,
               [&](const MeasuredDevG& g) { sample_row(generic(g), wi, u, active, q, tint, wo_out, pdf_out, weight_out); },
               [&] { store3(wo_out, q, nan, nan, nan); pdf_out[q] = nan; if (weight_out) store3(weight_out, q, nan, nan, nan); });
}

__global__ __launch_bounds__(256) void measured_pdf_table_kernel(const MeasuredDevG* __restrict__ table, int n_materials,
                                                                 const long long* __restrict__ material_id,
                                                                 const float* __restrict__ wi, const float* __restrict__ wo,
                                                                 const unsigned char* __restrict__ active, long long n,
                                                                 float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    with_entry(table, n_materials, material_id[q], has_ground_truth,
               [&](const MeasuredDevG& g) { pdf_row(generic(g), wi, wo, active, q, pdf_out); }, [&] { pdf_out[q] = quiet_nan(); });
}

}  // namespace

extern "C" {

int bsdfd_measured_table_create(const bsdfd_measured_handle* handles, int32_t n_materials, bsdfd_measured_table* out) {
    if (!out) return bsdfd_fail_(BSDFD_EINVAL, "null argument");
    *out = nullptr;
    if (!handles) return bsdfd_fail_(BSDFD_EINVAL, "null handle array");
    if (n_materials < 1 || n_materials > 65536) return bsdfd_fail_(BSDFD_EINVAL, "n_materials must be in [1, 65536]");
    bool any = false;
    for (int32_t m = 0; m < n_materials; ++m) any = any || handles[m] != nullptr;
    if (!any) return bsdfd_fail_(BSDFD_EINVAL, "a measured table needs at least one material with ground truth");
    int devid = -1;
    HIP_TRY(hipGetDevice(&devid));
    std::vector<MeasuredDev> host((size_t)n_materials, MeasuredDev{});
    for (int32_t m = 0; m < n_materials; ++m) {
        if (!handles[m]) continue;
        if (handles[m]->device != devid)
            return bsdfd_fail_(BSDFD_EINVAL, "measured handle " + std::to_string(m) + " belongs to another device");
        host[(size_t)m] = handles[m]->dev;
    }
    return material_table::upload(host, devid, "descriptors", out);
}

void bsdfd_measured_table_destroy(bsdfd_measured_table t) { material_table::destroy(t); }

int bsdfd_measured_eval_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                              const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, void* stream) {
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o ? "null pointer" : nullptr;
    return material_table::launch(t, n, n, material_id, bad, measured_eval_table_kernel, stream, wi, wo, wl, (long long)n,
                                  TintArg{tint}, f_o, f_l);
}

int bsdfd_measured_eval_table_rows(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                                   const float* wl, int64_t n, const float* tint, float* f_o, float* f_l, const int64_t* rows,
                                   int64_t n_rows, void* stream) {
    const char* bad = (wl == nullptr) != (f_l == nullptr) ? "wl and f_l are both NULL or both given"
                      : !material_id || !wi || !wo || !f_o || !rows ? "null pointer" : nullptr;
    return material_table::launch(t, n, n_rows, material_id, bad, measured_eval_table_rows_kernel, stream, wi, wo, wl,
                                  (long long)n, TintArg{tint}, f_o, f_l, reinterpret_cast<const long long*>(rows),
                                  (long long)n_rows);
}

int bsdfd_measured_sample_weight_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi,
                                       const float* wo, const float* pdf_sa, const unsigned char* active, int64_t n,
                                       const float* tint, float firefly_threshold, float* weight_out, float* pdf_out,
                                       void* stream) {
    const bool given = material_id && wi && wo && pdf_sa && weight_out && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", measured_weight_table_kernel, stream, wi,
                                  wo, pdf_sa, active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

int bsdfd_measured_sample_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* u,
                                const unsigned char* active, int64_t n, const float* tint, float* wo_out, float* pdf_out,
                                float* weight_out, void* stream) {
    const bool given = material_id && wi && u && wo_out && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", measured_sample_table_kernel, stream, wi,
                                  u, active, (long long)n, TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_measured_pdf_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                             const unsigned char* active, int64_t n, float* pdf_out, void* stream) {
    const bool given = material_id && wi && wo && pdf_out;
    return material_table::launch(t, n, n, material_id, given ? nullptr : "null pointer", measured_pdf_table_kernel, stream, wi, wo,
                                  active, (long long)n, pdf_out);
}

}  // extern "C"
