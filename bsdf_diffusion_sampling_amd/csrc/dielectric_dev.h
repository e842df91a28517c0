// dielectric_dev.h — device side of the rough-dielectric model (the kernels and entry points: dielectric.hip).
//
// Walter et al., "Microfacet Models for Refraction through Rough Surfaces" (EGSR 2007), with the choices Mitsuba's
// `roughdielectric` makes by default: Beckmann D, the rational approximation of the Smith G1, the exact unpolarised Fresnel
// term, sampling of the VISIBLE normals (Heitz & d'Eon 2014) and radiance transport (the transmitted lobe carries 1 / eta^2).
// Restated from the publications; parity-unpinned against Mitsuba.  Both sides of the surface are served.
//
// dielectric_f (eval), dielectric_pdf and dielectric_sample are shared by all four kernels, so that sample()'s pdf and weight,
// pdf() and eval() of the same pair are the same bits.  One row per lane, no memory but the row's own, no LDS, no scratch; the
// one numeric inversion (a slope of the visible-normal distribution) runs a FIXED trip count — wave-uniform control flow.
// tests/dielectric_ref.py restates this file statement for statement.
#pragma once
#include <hip/hip_runtime.h>

#include "bsdfd.h"
#include "common.h"

// multiply-adds are fused per source expression, by the front end (measured_dev.h explains why)
#pragma clang fp contract(on)

namespace dielectric_dev {

struct DielectricDev {
    float alpha, eta0, inv_eta0;
};

struct Vec {
    float x, y, z;
};
__device__ __forceinline__ float dot(const Vec& a, const Vec& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvSqrtPi = 0.56418958354775628695f;    // 1 / sqrt(pi)
constexpr float kInv2SqrtPi = 0.28209479177387814347f;   // 1 / (2 sqrt(pi))
constexpr float kSlopeLimit = 6.0f;                      // slopes are drawn from [-6, 6]: erfc(6) = 2e-17
constexpr int kBisections = 20, kNewtonSteps = 2;
constexpr float kMinHalfLen2 = 1e-12f;                   // |wi + k wo|^2 below this: rounding noise, no half vector

// the generalised half vector of a pair, flipped to m.z > 0; false where it is undefined
struct Half {
    Vec m;
    bool reflect, ok;
    float eta;   // relative index along the path: eta0 entering, 1 / eta0 leaving
};
__device__ __forceinline__ Half half_vector(const DielectricDev& d, const Vec& wi, const Vec& wo) {
    Half h;
    h.reflect = wi.z * wo.z > 0.0f;
    h.eta = wi.z > 0.0f ? d.eta0 : d.inv_eta0;
    const float k = h.reflect ? 1.0f : h.eta;
    const float hx = wi.x + wo.x * k, hy = wi.y + wo.y * k, hz = wi.z + wo.z * k;
    const float len2 = hx * hx + hy * hy + hz * hz;
    const bool ok = len2 > kMinHalfLen2;
    float inv = ok ? 1.0f / sqrtf(ok ? len2 : 1.0f) : 0.0f;
    inv = hz < 0.0f ? -inv : inv;
    h.m = Vec{hx * inv, hy * inv, hz * inv};
    h.ok = ok && h.m.z > 0.0f;
    return h;
}

__device__ __forceinline__ float beckmann_d(const DielectricDev& d, const Vec& m) {
    const float a2 = d.alpha * d.alpha;
    const float cz2 = m.z * m.z;
    const float v = expf(-(m.x * m.x + m.y * m.y) / (a2 * cz2)) / (kPi * a2 * cz2 * cz2);
    return v * m.z > 1e-20f ? v : 0.0f;
}

// Smith shadowing-masking of one direction (Walter et al., eq. 27: the rational approximation)
__device__ __forceinline__ float smith_g1(const DielectricDev& d, const Vec& v, float dot_vm) {
    const float ax = d.alpha * v.x, ay = d.alpha * v.y;
    const float xy = ax * ax + ay * ay;
    const float a = 1.0f / sqrtf(xy / (v.z * v.z));
    const float a2 = a * a;
    float g = (3.535f * a + 2.181f * a2) / (1.0f + 2.276f * a + 2.577f * a2);
    g = a >= 1.6f ? 1.0f : g;
    g = xy == 0.0f ? 1.0f : g;
    return dot_vm * v.z <= 0.0f ? 0.0f : g;
}

// exact unpolarised Fresnel reflectance from the two (absolute) cosines; 1 at grazing incidence
__device__ __forceinline__ float fresnel_of(float eta_it, float ca, float ct) {
    const float a_s = (eta_it * ct - ca) / (eta_it * ct + ca);
    const float a_p = (eta_it * ca - ct) / (eta_it * ca + ct);
    const float f = 0.5f * (a_s * a_s + a_p * a_p);
    return ca == 0.0f ? 1.0f : f;
}

// ... at the signed cosine c = wi . m, the transmitted cosine by Snell's law; also that cosine, signed, and the relative index
// eta_ti the refraction uses.  1 under total internal reflection.
__device__ __forceinline__ float fresnel(const DielectricDev& d, float c, float& cos_t, float& eta_ti) {
    const bool outside = c >= 0.0f;
    const float eta_it = outside ? d.eta0 : d.inv_eta0;
    eta_ti = outside ? d.inv_eta0 : d.eta0;
    const float ct2 = 1.0f - eta_ti * eta_ti * (1.0f - c * c);
    const float ct = sqrtf(fmaxf(ct2, 0.0f));
    cos_t = c > 0.0f ? -ct : ct;
    return fresnel_of(eta_it, fabsf(c), ct);
}

struct Terms {
    Half h;
    float dwi, dwo, D, F, s;
};
__device__ __forceinline__ Terms terms_of(const DielectricDev& d, const Vec& wi, const Vec& wo) {
    Terms t;
    t.h = half_vector(d, wi, wo);
    t.dwi = dot(wi, t.h.m);
    t.dwo = dot(wo, t.h.m);
    t.D = beckmann_d(d, t.h.m);
    float cos_t, eta_ti;
    // across the surface the generalised half vector obeys Snell's law by construction: |wo . m| IS the transmitted cosine.
    // Reading it off the pair keeps 1 - F well conditioned next to the critical angle (and reciprocal to rounding).
    t.F = t.h.reflect ? fresnel(d, t.dwi, cos_t, eta_ti)
                      : fresnel_of(t.dwi >= 0.0f ? d.eta0 : d.inv_eta0, fabsf(t.dwi), fabsf(t.dwo));
    t.s = t.dwi + t.h.eta * t.dwo;
    return t;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for inf and NaN

// f(wi, wo) |cos theta_o| (grey)
__device__ __forceinline__ float dielectric_f(const DielectricDev& d, const Vec& wi, const Vec& wo) {
    const Terms t = terms_of(d, wi, wo);
    const float G = smith_g1(d, wi, t.dwi) * smith_g1(d, wo, t.dwo);
    const float vr = t.F * t.D * G / (4.0f * fabsf(wi.z));
    const float vt = fabsf((1.0f - t.F) * t.D * G * t.dwi * t.dwo / (wi.z * (t.s * t.s)));
    const float v = t.h.reflect ? vr : vt;
    return t.h.ok && wi.z != 0.0f && wo.z != 0.0f && finite(v) ? v : 0.0f;
}

// solid-angle density of dielectric_sample: visible normals, the lobe's Fresnel share, the Jacobian of the half vector
__device__ __forceinline__ float dielectric_pdf(const DielectricDev& d, const Vec& wi, const Vec& wo) {
    const Terms t = terms_of(d, wi, wo);
    const float vis = t.D * smith_g1(d, wi, t.dwi) * fabsf(t.dwi) / fabsf(wi.z);
    const float lobe = t.h.reflect ? t.F : 1.0f - t.F;
    const float jac = t.h.reflect ? 1.0f / (4.0f * fabsf(t.dwo)) : t.h.eta * t.h.eta * fabsf(t.dwo) / (t.s * t.s);
    const float p = vis * lobe * jac;
    return t.h.ok && wi.z != 0.0f && wo.z != 0.0f && finite(p) && p > 0.0f ? p : 0.0f;
}

// C(x) = integral of the visible-slope density (ct - s st) exp(-s^2) / sqrt(pi) up to x, for the alpha = 1 surface seen from
// (st, 0, ct)
__device__ __forceinline__ float slope_cdf(float ct, float st, float x) {
    return 0.5f * ct * erfcf(-x) + st * kInv2SqrtPi * expf(-x * x);
}

// x with C(x) = u C(hi) on [-6, hi = min(ct / st, 6)]: bisections to a bracket, Newton steps clamped to it
__device__ __forceinline__ float sample_slope(float ct, float st, float u) {
    float lo = -kSlopeLimit;
    float hi = fminf(ct / st, kSlopeLimit);
    const float t = u * slope_cdf(ct, st, hi);
    for (int k = 0; k < kBisections; ++k) {
        const float mid = 0.5f * (lo + hi);
        const bool up = slope_cdf(ct, st, mid) <= t;
        lo = up ? mid : lo;
        hi = up ? hi : mid;
    }
    float x = 0.5f * (lo + hi);
    for (int k = 0; k < kNewtonSteps; ++k) {
        const float dc = (ct - x * st) * kInvSqrtPi * expf(-x * x);
        const float xn = fminf(fmaxf(x - (slope_cdf(ct, st, x) - t) / dc, lo), hi);
        x = dc > 0.0f ? xn : x;
    }
    return x;
}

// the visible normal of v = s wi (v.z > 0) at (u0, u1): stretch, draw the slopes, rotate, unstretch
__device__ __forceinline__ Vec sample_normal(const DielectricDev& d, const Vec& v, float u0, float u1) {
    float sx = d.alpha * v.x, sy = d.alpha * v.y, sz = v.z;
    float inv = 1.0f / sqrtf(sx * sx + sy * sy + sz * sz);
    sx *= inv; sy *= inv; sz *= inv;
    const float r = sqrtf(sx * sx + sy * sy);
    const bool flat = r > 0.0f;
    const float cphi = flat ? sx / r : 1.0f;
    const float sphi = flat ? sy / r : 0.0f;
    const float slope_x = sample_slope(sz, r, u0);
    const float slope_y = sample_slope(1.0f, 0.0f, u1);
    const float tx = (cphi * slope_x - sphi * slope_y) * d.alpha;
    const float ty = (sphi * slope_x + cphi * slope_y) * d.alpha;
    inv = 1.0f / sqrtf(tx * tx + ty * ty + 1.0f);
    return Vec{-tx * inv, -ty * inv, inv};
}

// sample(wi, u): wo, pdf = dielectric_pdf(wi, wo) and weight = dielectric_f(wi, wo) / pdf (untinted: f_cos is returned and
// the row divides), 0 where the pdf is 0 or wo is on the wrong side for the chosen lobe.  false (wo = 0) where wi.z == 0.
__device__ __forceinline__ bool dielectric_sample(const DielectricDev& d, const Vec& wi, float u0, float u1, float u2, Vec& wo,
                                                  float& pdf, float& f_cos) {
    wo = Vec{0.0f, 0.0f, 0.0f};
    pdf = f_cos = 0.0f;
    if (wi.z == 0.0f) return false;
    const float s = wi.z > 0.0f ? 1.0f : -1.0f;
    const Vec m = sample_normal(d, Vec{wi.x * s, wi.y * s, wi.z * s}, u0, u1);
    const float c = dot(wi, m);
    float cos_t, eta_ti;
    const float F = fresnel(d, c, cos_t, eta_ti);
    const bool reflect = u2 <= F;
    const float k = reflect ? 2.0f * c : eta_ti * c + cos_t;
    const float e = reflect ? 1.0f : eta_ti;
    wo = Vec{m.x * k - wi.x * e, m.y * k - wi.y * e, m.z * k - wi.z * e};
    pdf = dielectric_pdf(d, wi, wo);
    const bool side = reflect ? wi.z * wo.z > 0.0f : wi.z * wo.z < 0.0f;
    f_cos = side && pdf > 0.0f ? dielectric_f(d, wi, wo) : 0.0f;
    return true;
}

}  // namespace dielectric_dev
