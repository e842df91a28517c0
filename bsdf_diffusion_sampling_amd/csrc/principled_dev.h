// principled_dev.h — device side of the principled model (the kernels and entry points: principled.hip).
//
// Burley's principled BSDF ("Physically Based Shading at Disney", 2012; "Extending the Disney BRDF to a BSDF with Integrated
// Subsurface Scattering", 2015) with the choices Mitsuba's `principled` makes: four sampled lobes — diffuse (with retro-reflection,
// fake subsurface and sheen), a GTR1 clearcoat, specular transmission and specular reflection — over an anisotropic GGX
// distribution with the separable Smith G, the exact unpolarised Fresnel term mixed with Schlick terms, radiance transport.
// Visible normals are drawn with Heitz, "Sampling the GGX Distribution of Visible Normals" (JCGT 2018): closed form, no branch.
// Restated from the publications; parity-unpinned against Mitsuba.  Both sides of the surface are served.
//
// principled_f (eval), principled_pdf and principled_sample are shared by all four kernels, so that sample()'s pdf and weight,
// pdf() and eval() of the same pair are the same bits.  One row per lane, no memory but the row's own, no LDS, no scratch, no
// lane-dependent branch: every lobe's term is computed and selected under its mask, and sample() forms its four candidate
// directions, selects one and evaluates pdf / eval of that pair once.  What depends on the material alone is derived on the host
// (analytic_host.h: derive()) and arrives by value.  tests/principled_ref.py restates this file statement for statement.
#pragma once
#include <hip/hip_runtime.h>

#include "bsdfd.h"
#include "common.h"
#include "dielectric_dev.h"

// multiply-adds are fused per source expression, by the front end (measured_dev.h explains why)
#pragma clang fp contract(on)

namespace principled_dev {

using dielectric_dev::dot;
using dielectric_dev::finite;
using dielectric_dev::fresnel_of;
using dielectric_dev::kMinHalfLen2;
using dielectric_dev::kPi;
using dielectric_dev::Vec;

constexpr float kInvPi = 0.31830988618379067154f;

struct PrincipledDev {
    float base[3], sqrt_base[3], c_tint[3];
    float roughness, metallic, spec_tint, sheen, sheen_tint, flatness, clearcoat;
    float eta, inv_eta;
    float ax, ay, inv_ax, inv_ay, d_norm;    // GGX: max(1e-3, r^2 / aspect), max(1e-3, r^2 aspect); 1 / (pi ax ay)
    float a2_cc, ln_a2_cc;                   // GTR1: the clearcoat's alpha^2 and its logarithm
    float brdf, bsdf;                        // (1 - metallic)(1 - spec_trans), (1 - metallic) spec_trans
    float r0_eta;                            // ((eta - 1) / (eta + 1))^2
    float p_c, inv_sum, cum_d, cum_c;        // 0.25 clearcoat; 1 / (1 + p_c + brdf); the two constant lobe thresholds
};

struct Terms {
    Vec h;   // the generalised half vector, h.z >= 0
    bool reflect, refract, front, ok, compat_r, compat_t;
    float eta;   // relative index along the path: eta entering, 1 / eta leaving
    float dwi, dwo, F, s, D, Dcc;
};

__device__ __forceinline__ float ggx_d(const PrincipledDev& d, const Vec& h) {
    const float x = h.x * d.inv_ax, y = h.y * d.inv_ay;
    const float t = x * x + y * y + h.z * h.z;
    const float v = d.d_norm / (t * t);
    return v * h.z > 1e-20f ? v : 0.0f;
}

// the separable Smith term of one direction for the roughness pair (ax, ay)
__device__ __forceinline__ float smith_g1(const Vec& v, float dot_vh, float ax, float ay) {
    const float x = ax * v.x, y = ay * v.y;
    const float xy = x * x + y * y;
    float g = 2.0f / (1.0f + sqrtf(1.0f + xy / (v.z * v.z)));
    g = xy == 0.0f ? 1.0f : g;
    return dot_vh * v.z <= 0.0f ? 0.0f : g;
}

__device__ __forceinline__ float gtr1(const PrincipledDev& d, float hz) {
    return (d.a2_cc - 1.0f) / (kPi * d.ln_a2_cc * (1.0f + (d.a2_cc - 1.0f) * hz * hz));
}

// exact unpolarised Fresnel reflectance at the signed cosine c, the transmitted cosine by Snell's law; also that cosine, signed,
// and the relative index eta_ti the refraction uses.  1 under total internal reflection.
__device__ __forceinline__ float fresnel(const PrincipledDev& d, float c, float& cos_t, float& eta_ti) {
    const bool outside = c >= 0.0f;
    const float eta_it = outside ? d.eta : d.inv_eta;
    eta_ti = outside ? d.inv_eta : d.eta;
    const float ct2 = 1.0f - eta_ti * eta_ti * (1.0f - c * c);
    const float ct = sqrtf(fmaxf(ct2, 0.0f));
    cos_t = c > 0.0f ? -ct : ct;
    return fresnel_of(eta_it, fabsf(c), ct);
}

// Schlick's weight clamp(1 - c, 0, 1)^5.  The model takes its Schlick terms at c >= 0 only (the front side), where Mitsuba's
// two-sided statement is r0 + (1 - r0) sw(c).
__device__ __forceinline__ float sw(float c) {
    const float x = fminf(fmaxf(1.0f - c, 0.0f), 1.0f);
    const float x2 = x * x;
    return x2 * x2 * x;
}

__device__ __forceinline__ Terms terms_of(const PrincipledDev& d, const Vec& wi, const Vec& wo) {
    Terms t;
    t.reflect = wi.z * wo.z > 0.0f;
    t.refract = wi.z * wo.z < 0.0f;
    t.front = wi.z > 0.0f;
    t.eta = t.front ? d.eta : d.inv_eta;
    const float k = t.reflect ? 1.0f : t.eta;
    const float hx = wi.x + wo.x * k, hy = wi.y + wo.y * k, hz = wi.z + wo.z * k;
    const float len2 = hx * hx + hy * hy + hz * hz;
    const bool ok = len2 > kMinHalfLen2;
    float inv = ok ? 1.0f / sqrtf(ok ? len2 : 1.0f) : 0.0f;
    inv = hz < 0.0f ? -inv : inv;
    t.h = Vec{hx * inv, hy * inv, hz * inv};
    t.ok = ok && wi.z != 0.0f;
    t.dwi = dot(wi, t.h);
    t.dwo = dot(wo, t.h);
    float cos_t, eta_ti;
    // across the surface the generalised half vector obeys Snell's law by construction: |wo . h| IS the transmitted cosine
    t.F = t.reflect ? fresnel(d, t.dwi, cos_t, eta_ti)
                    : fresnel_of(t.dwi >= 0.0f ? d.eta : d.inv_eta, fabsf(t.dwi), fabsf(t.dwo));
    const float s_dwi = t.front ? t.dwi : -t.dwi, s_dwo = t.front ? t.dwo : -t.dwo;
    t.s = t.dwi + t.eta * t.dwo;
    t.D = ggx_d(d, t.h);
    t.compat_r = s_dwi > 0.0f && s_dwo > 0.0f;
    t.compat_t = s_dwi > 0.0f && s_dwo < 0.0f;
    t.Dcc = gtr1(d, t.h.z);
    return t;
}

// f(wi, wo) |cos theta_o| per channel
__device__ __forceinline__ void principled_f(const PrincipledDev& d, const Vec& wi, const Vec& wo, float out[3]) {
    const Terms t = terms_of(d, wi, wo);
    const float aci = fabsf(wi.z), aco = fabsf(wo.z);
    const float G = smith_g1(wi, t.dwi, d.ax, d.ay) * smith_g1(wo, t.dwo, d.ax, d.ay);
    const bool m_spec = t.reflect && t.compat_r && t.F > 0.0f;
    const bool m_trans = d.bsdf > 0.0f && t.refract && t.compat_t && t.F < 1.0f;
    const bool m_front = t.reflect && t.front;
    const float spec = m_spec ? t.D * G / (4.0f * aci) : 0.0f;
    const float trans = m_trans ? d.bsdf * fabsf((1.0f - t.F) * t.D * G * t.dwi * t.dwo / (wi.z * (t.s * t.s))) : 0.0f;
    const float sch = sw(fabsf(t.dwi));
    const float Gcc = smith_g1(wi, t.dwi, 0.25f, 0.25f) * smith_g1(wo, t.dwo, 0.25f, 0.25f);
    const float cc = m_front && d.clearcoat > 0.0f ? d.p_c * (0.04f + 0.96f * sch) * t.Dcc * Gcc * aco : 0.0f;
    const float Fo = sw(aco), Fi = sw(aci);
    const float f_d = (1.0f - 0.5f * Fi) * (1.0f - 0.5f * Fo);
    const float Rr = 2.0f * d.roughness * t.dwo * t.dwo;
    const float f_r = Rr * (Fo + Fi + Fo * Fi * (Rr - 1.0f));
    const float Fss = (1.0f + (0.5f * Rr - 1.0f) * Fo) * (1.0f + (0.5f * Rr - 1.0f) * Fi);
    const float f_ss = 1.25f * (Fss * (1.0f / (aco + aci) - 0.5f) + 0.5f);
    const float diff = m_front && d.brdf > 0.0f
                           ? d.brdf * aco * kInvPi * ((1.0f - d.flatness) * (f_d + f_r) + d.flatness * f_ss) : 0.0f;
    const float sheen = m_front && d.sheen > 0.0f && d.metallic < 1.0f
                            ? d.sheen * (1.0f - d.metallic) * sw(fabsf(t.dwo)) * aco : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float base = d.base[k], ctint = d.c_tint[k];
        const float r0c = ctint * d.r0_eta;
        float Fp = (1.0f - d.metallic) * (1.0f - d.spec_tint) * t.F + d.metallic * (base + (1.0f - base) * sch)
                   + (1.0f - d.metallic) * d.spec_tint * (r0c + (1.0f - r0c) * sch);
        Fp = t.front ? Fp : d.bsdf * t.F;
        const float v = Fp * spec + d.sqrt_base[k] * trans + cc + base * diff + (1.0f + (ctint - 1.0f) * d.sheen_tint) * sheen;
        out[k] = t.ok && finite(v) ? v : 0.0f;
    }
}

// solid-angle density of principled_sample: the mixture of the four lobes.  The lobe probabilities sum to a constant of the
// material (p_r + p_t = 1 whatever F is), which is why this density is exact although the sampler reuses its variates.
__device__ __forceinline__ float principled_pdf(const PrincipledDev& d, const Vec& wi, const Vec& wo) {
    const Terms t = terms_of(d, wi, wo);
    const float vis = t.D * smith_g1(wi, t.dwi, d.ax, d.ay) * fabsf(t.dwi) / fabsf(wi.z);
    const float p_t = t.front ? d.bsdf * (1.0f - t.F) * d.inv_sum : 1.0f - t.F;
    const float p_r = t.front ? (1.0f - d.bsdf * (1.0f - t.F)) * d.inv_sum : t.F;
    const float p_c = t.front ? d.p_c * d.inv_sum : 0.0f;
    const float p_d = t.front ? d.cum_d : 0.0f;
    const float jac = t.reflect ? 1.0f / (4.0f * fabsf(t.dwo)) : fabsf(t.eta * t.eta * t.dwo / (t.s * t.s));
    const float on_r = t.reflect && t.compat_r ? (p_r * vis + p_c * t.Dcc * t.h.z) * jac : 0.0f;
    const float on_t = t.refract && t.compat_t ? p_t * vis * jac : 0.0f;
    const float p = on_r + on_t + (t.reflect ? p_d * fmaxf(wo.z, 0.0f) * kInvPi : 0.0f);
    const bool live = t.ok && (t.front || d.bsdf > 0.0f);
    return live && finite(p) && p > 0.0f ? p : 0.0f;
}

// the visible normal of v = s wi (v.z > 0) at (u0, u1), with (sn, cs) = sin, cos of 2 pi u1: stretch, a point of the unit disk
// warped towards the visible half, back onto the hemisphere, unstretch (Heitz 2018, listing 1)
__device__ __forceinline__ Vec sample_normal(const PrincipledDev& d, const Vec& v, float u0, float sn, float cs) {
    float sx = d.ax * v.x, sy = d.ay * v.y, sz = v.z;
    float inv = 1.0f / sqrtf(sx * sx + sy * sy + sz * sz);
    sx *= inv; sy *= inv; sz *= inv;
    const float len2 = sx * sx + sy * sy;
    const bool flat = len2 > 0.0f;
    const float il = flat ? 1.0f / sqrtf(flat ? len2 : 1.0f) : 0.0f;
    const float t1x = flat ? -sy * il : 1.0f, t1y = flat ? sx * il : 0.0f;
    const float t2x = -sz * t1y, t2y = sz * t1x, t2z = sx * t1y - sy * t1x;   // cross(Vh, T1), T1.z = 0
    const float r = sqrtf(u0);
    const float p1 = r * cs;
    float p2 = r * sn;
    const float s = 0.5f * (1.0f + sz);
    p2 = (1.0f - s) * sqrtf(fmaxf(1.0f - p1 * p1, 0.0f)) + s * p2;
    const float p3 = sqrtf(fmaxf(1.0f - p1 * p1 - p2 * p2, 0.0f));
    const float nx = p1 * t1x + p2 * t2x + p3 * sx;
    const float ny = p1 * t1y + p2 * t2y + p3 * sy;
    const float nz = p2 * t2z + p3 * sz;
    const float mx = d.ax * nx, my = d.ay * ny, mz = fmaxf(nz, 0.0f);
    inv = 1.0f / sqrtf(mx * mx + my * my + mz * mz);
    return Vec{mx * inv, my * inv, mz * inv};
}

// sample(wi, u): wo, pdf = principled_pdf(wi, wo) and f = principled_f(wi, wo) (the row divides).  u2 picks the lobe on the
// cumulative order diffuse, clearcoat, transmission, reflection.  A failed sample — wo on the wrong side for its lobe, a normal
// that is not compatible with the pair, wi.z == 0, a back side without transmission, pdf == 0 — is all zeros.
__device__ __forceinline__ void principled_sample(const PrincipledDev& d, const Vec& wi, float u0, float u1, float u2, Vec& wo,
                                                  float& pdf, float f[3]) {
    const bool front = wi.z > 0.0f;
    const bool live = wi.z != 0.0f && (front || d.bsdf > 0.0f);
    const float s = front ? 1.0f : -1.0f;
    float sn0, cs0, sn1, cs1;   // of 2 pi u0 and 2 pi u1
    sincospif(2.0f * u0, &sn0, &cs0);
    sincospif(2.0f * u1, &sn1, &cs1);
    const Vec m = sample_normal(d, Vec{wi.x * s, wi.y * s, wi.z * s}, u0, sn1, cs1);
    const float c = dot(wi, m);
    float cos_t, eta_ti;
    const float F = fresnel(d, c, cos_t, eta_ti);
    // the clearcoat's normal from GTR1
    float cos2 = (1.0f - expf((1.0f - u1) * d.ln_a2_cc)) / (1.0f - d.a2_cc);
    cos2 = fminf(fmaxf(cos2, 0.0f), 1.0f);
    const float cth = sqrtf(cos2), sth = sqrtf(1.0f - cos2);
    const Vec mcc{sth * cs0, sth * sn0, cth};
    const float ccc = dot(wi, mcc);
    // the cosine hemisphere, always +z
    const float r = sqrtf(u0);
    // the lobe: thresholds of the cumulative order
    const float cum_d = front ? d.cum_d : 0.0f;
    const float cum_c = front ? d.cum_c : 0.0f;
    const float cum_t = cum_c + (front ? d.bsdf * (1.0f - F) * d.inv_sum : 1.0f - F);
    const bool is_d = u2 < cum_d, is_c = !is_d && u2 < cum_c, is_t = !is_d && !is_c && u2 < cum_t;
    // the candidate directions, one selected: wo = n k - wi e, or the hemisphere's point
    const Vec n = is_c ? mcc : m;
    const float k = is_c ? 2.0f * ccc : is_t ? eta_ti * c + cos_t : 2.0f * c;
    const float e = is_t ? eta_ti : 1.0f;
    Vec w{n.x * k - wi.x * e, n.y * k - wi.y * e, n.z * k - wi.z * e};
    w = is_d ? Vec{r * cs1, r * sn1, sqrtf(1.0f - u0)} : w;
    const float dn_i = s * dot(wi, n), dn_o = s * dot(w, n);
    const bool side = is_t ? wi.z * w.z < 0.0f : wi.z * w.z > 0.0f;
    const bool compat = is_d || (dn_i > 0.0f && (is_t ? dn_o < 0.0f : dn_o > 0.0f));
    bool good = live && side && compat;
    w = good ? w : Vec{0.0f, 0.0f, 0.0f};
    pdf = principled_pdf(d, wi, w);
    good = good && pdf > 0.0f;
    wo = good ? w : Vec{0.0f, 0.0f, 0.0f};
    pdf = good ? pdf : 0.0f;
    principled_f(d, wi, wo, f);
}

}  // namespace principled_dev
