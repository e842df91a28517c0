// analytic_rows.h — one row of each kernel of the analytic ground truth, over either model: principled.hip and dielectric.hip run
// these rows on their one material, analytic_table.hip on the material of the row's id.  One statement of each, inlined into all
// three, under the contraction mode the models' headers fix: what the table promises — bit for bit what the single-material
// kernels return — rests on it.  The analytic counterpart of the row functions of measured_dev.h, with their argument order.
#pragma once
#include <hip/hip_runtime.h>

#include "dielectric_dev.h"
#include "principled_dev.h"
#include "rows.h"

// multiply-adds are fused per source expression, by the front end (rows.h explains why)
#pragma clang fp contract(on)

namespace analytic_rows {

using dielectric_dev::DielectricDev;
using dielectric_dev::Vec;
using principled_dev::PrincipledDev;
using rows::store3;
using rows::Tint;

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
        float v = 0.0f;   // (0 already where the lobe's side test failed)
        dielectric_dev::dielectric_sample(d, wi, u0, u1, u2, wo, pdf, v);
        f[0] = f[1] = f[2] = v;
    }
};

__device__ __forceinline__ Vec load3(const float* __restrict__ p, long long q) { return Vec{p[3 * q], p[3 * q + 1], p[3 * q + 2]}; }

// eval(): f_o = f(wi, wo) |cos theta_o| * tint and, with a second direction wl (null: none), f_l = f(wi, wl) |cos| * tint
template <class Model>
__device__ __forceinline__ void eval_row(const Model& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                         const float* __restrict__ wl, long long q, Tint tint, float* __restrict__ f_o,
                                         float* __restrict__ f_l) {
    float f[3];
    m.f(load3(wi, q), load3(wo, q), f);
    store3(f_o, q, f[0] * tint.r, f[1] * tint.g, f[2] * tint.b);
    if (wl) {
        m.f(load3(wi, q), load3(wl, q), f);
        store3(f_l, q, f[0] * tint.r, f[1] * tint.g, f[2] * tint.b);
    }
}

// the tail of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = f * tint / pdf_sa where
// pdf_sa > 0, firefly rule on channel x, no cosine masks
template <class Model>
__device__ __forceinline__ void weight_row(const Model& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                           const float* __restrict__ pdf_in, const unsigned char* __restrict__ active,
                                           long long q, Tint tint, float thr, float* __restrict__ weight,
                                           float* __restrict__ pdf_out) {
    float f[3];
    m.f(load3(wi, q), load3(wo, q), f);
    const float pdf = pdf_in[q];
    const bool act = !active || active[q] != 0;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (act && pdf > 0.0f) { v[0] = f[0] * tint.r / pdf; v[1] = f[1] * tint.g / pdf; v[2] = f[2] * tint.b / pdf; }
    const float p = act && v[0] < thr ? pdf : 0.0f;
    const bool keep = p > 0.0f;
    pdf_out[q] = p;
    store3(weight, q, keep ? v[0] : 0.0f, keep ? v[1] : 0.0f, keep ? v[2] : 0.0f);
}

// sample(): u [N,3] = (sample2.x, sample2.y, sample1); a row with active[q] == 0 gets zeros; weight_out is optional
template <class Model>
__device__ __forceinline__ void sample_row(const Model& m, const float* __restrict__ wi, const float* __restrict__ u,
                                           const unsigned char* __restrict__ active, long long q, Tint tint,
                                           float* __restrict__ wo_out, float* __restrict__ pdf_out,
                                           float* __restrict__ weight_out) {
    Vec wo{0.0f, 0.0f, 0.0f};
    float pdf = 0.0f, f[3] = {0.0f, 0.0f, 0.0f};
    if (!active || active[q] != 0) m.sample(load3(wi, q), u[3 * q], u[3 * q + 1], u[3 * q + 2], wo, pdf, f);
    store3(wo_out, q, wo.x, wo.y, wo.z);
    pdf_out[q] = pdf;
    if (weight_out) {
        const bool keep = pdf > 0.0f;
        const float p = keep ? pdf : 1.0f;
        store3(weight_out, q, keep ? f[0] * tint.r / p : 0.0f, keep ? f[1] * tint.g / p : 0.0f, keep ? f[2] * tint.b / p : 0.0f);
    }
}

// pdf(): the density of that sampler at a given wo
template <class Model>
__device__ __forceinline__ void pdf_row(const Model& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                        const unsigned char* __restrict__ active, long long q, float* __restrict__ pdf_out) {
    pdf_out[q] = !active || active[q] != 0 ? m.pdf(load3(wi, q), load3(wo, q)) : 0.0f;
}

}  // namespace analytic_rows
