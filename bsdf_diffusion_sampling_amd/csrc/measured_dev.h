// measured_dev.h — device side of the RGL measured-BSDF model (the model's host part: measured.hip), shared by the translation
// units that evaluate it: measured.hip (one material per launch) and measured_table.hip (a mixed-material wavefront in one
// launch).  Both inline the same measured_f (eval), measured_sample and measured_pdf (the file's own importance sampler), run the
// same row functions (eval_row, weight_row, sample_row, pdf_row) and compute the same bits (see the pragma below).  What a row
// kernel and its launcher need whatever the model — Tint, store3, launch_rows, the launch checks — is rows.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "rows.h"

// multiply-adds are fused per source expression, by the front end, from here to the end of the including translation unit
// (rows.h explains why): measured.hip and measured_table.hip compute the same bits
#pragma clang fp contract(on)

namespace measured_dev {

using rows::launch_rows;
using rows::store3;
using rows::Tint;
using rows::TintArg;

struct Table {        // [slices][h][w] fp32 on the device
    const float* data;
    int w, h;
};

struct MeasuredDev {
    const float* phi_i;
    const float* theta_i;
    int n_phi, n_theta;
    int isotropic, jacobian, reduction;
    float fold_x, fold_y;  // signs of (cos, sin) at the middle of the file's phi_i range: the quadrant / half-plane stored
    Table ndf, sigma, vndf, rgb;
    const float* vndf_cond;  // [n_phi][n_theta][h][w]  cumulative row integrals (patch units, normalised)
    const float* vndf_marg;  // [n_phi][n_theta][h]
    // the optional `luminance` field, the first warp of the file's own sampler (measured_sample): normalised per slice like the
    // VNDF, with the same two CDFs.  lum.data == nullptr: the file has none (lum_pdf = 1).  New members go HERE, at the end.
    Table lum;
    const float* lum_cond;  // [n_phi][n_theta][h][w]
    const float* lum_marg;  // [n_phi][n_theta][h]
};

__device__ __forceinline__ float elevation(float x, float y, float z) {  // 2 asin(|d - z| / 2)
    const float dist = sqrtf(x * x + y * y + (z - 1.0f) * (z - 1.0f));
    return 2.0f * asinf(fminf(0.5f * dist, 1.0f));
}

// interval i with vals[i] <= p < vals[i+1] (clamped) and the weight of its upper end
__device__ __forceinline__ void interval(const float* __restrict__ vals, int n, float p, int& i, float& t) {
    if (n == 1) { i = 0; t = 0.0f; return; }
    int lo = 0;
    for (int k = 1; k < n - 1; ++k) lo = vals[k] <= p ? k : lo;  // n <= a few dozen
    i = lo;
    const float a = vals[lo], b = vals[lo + 1];
    t = fminf(fmaxf((p - a) / (b - a), 0.0f), 1.0f);
}

struct Patch {
    int ix, iy;
    float fx, fy;
};
__device__ __forceinline__ Patch patch_of(float x, float y, int w, int h) {
    x *= (float)(w - 1); y *= (float)(h - 1);
    Patch p;
    p.ix = min(max((int)floorf(x), 0), w - 2);
    p.iy = min(max((int)floorf(y), 0), h - 2);
    p.fx = x - (float)p.ix; p.fy = y - (float)p.iy;
    return p;
}
__device__ __forceinline__ float bilerp(float v00, float v10, float v01, float v11, float fx, float fy) {
    return (1.0f - fy) * ((1.0f - fx) * v00 + fx * v10) + fy * ((1.0f - fx) * v01 + fx * v11);
}
__device__ __forceinline__ float eval_plain(const Table& t, float x, float y) {
    const Patch p = patch_of(x, y, t.w, t.h);
    const float* d = t.data + (size_t)p.iy * t.w + p.ix;
    return bilerp(d[0], d[1], d[t.w], d[t.w + 1], p.fx, p.fy);
}

// The fold of an anisotropic file.  Only phi_i in a half-plane (reduction 2: point symmetry) or a quadrant (reduction 4: two
// mirror planes) is stored; Mitsuba folds with mulsign_neg(v, s) = -|..|, i.e. into y <= 0 (and x <= 0), where its files keep
// phi_i.  Here the stored side is read off the file's own phi_i range (fold_x, fold_y), which is the same thing for such files
// and right for any other.  (wix, wiy) is folded in place; the caller applies the returned flips to wo (measured_sample: to
// the wo it returns).  A component on the wrong side is negated together with its partner of wo (reduction 2: both
// components, and only wiy says when).  A ZERO component of either sign is on a symmetry plane, i.e. already on the stored
// side: it flips nothing, and it takes the stored side's sign, so that atan2f answers inside [phi_i[0], phi_i[n_phi - 1]] —
// with the other sign, (-x, +0) in a file stored over [-pi, -pi/2] has the azimuth +pi, which `interval` clamps to the slice
// at -pi/2, the far end of the range.  Off the planes copysignf returns the bits the negation did.  (Reduction 2 stores both
// sides of x: a zero x is read as +0 — adding +0 changes nothing else —, so that no result depends on a zero's sign.)
struct Fold {
    bool x, y;
};
__device__ __forceinline__ Fold fold_wi(const MeasuredDev& m, float& wix, float& wiy) {
    Fold f{false, false};
    if (m.reduction >= 2) {
        f.y = wiy * m.fold_y < 0.0f;
        f.x = m.reduction == 4 ? (wix * m.fold_x < 0.0f) : f.y;
        wiy = copysignf(wiy, m.fold_y);
        wix = m.reduction == 4 ? copysignf(wix, m.fold_x) : (f.x ? -wix : wix) + 0.0f;
    }
    return f;
}

// The half vector of a folded pair at the pole of its chart.  A zero of wi carries the stored side's sign after the fold, so
// at the exact mirror direction wi.x + wo.x can come out as -0, and the azimuth of (+-0, +-0) is 0 or +-pi by the zeros' signs
// alone — half a table apart, at the one point where it means nothing.  Adding +0 reads a -0 of ANY origin (the fold's, or a
// product that underflowed off the planes) as +0 and changes no non-zero value; the azimuth differs for it only where both
// components are zero: the pole's azimuth is 0.  (my = -0 next to mx < 0 moves from -pi to +pi, which the wrap of um_y takes to
// the same 0.)  Files without a fold are not touched.
__device__ __forceinline__ void unsign_zeros(const MeasuredDev& m, float& mx, float& my) {
    if (m.reduction >= 2) { mx += 0.0f; my += 0.0f; }
}

// f(wi, wo) cos(theta_o) for one pair; false (and rgb = 0) on the lower hemispheres
__device__ __forceinline__ bool measured_f(const MeasuredDev& m, float wix, float wiy, float wiz, float wox, float woy,
                                           float woz, float rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (!(wiz > 0.0f && woz > 0.0f)) return false;
    const Fold fold = fold_wi(m, wix, wiy);
    if (fold.x) wox = -wox;
    if (fold.y) woy = -woy;
    float mx = wix + wox, my = wiy + woy, mz = wiz + woz;
    const float inv = 1.0f / fmaxf(sqrtf(mx * mx + my * my + mz * mz), 1e-30f);
    mx *= inv; my *= inv; mz *= inv;
    unsign_zeros(m, mx, my);
    const float theta_i = elevation(wix, wiy, wiz), phi_i = atan2f(wiy, wix);
    const float theta_m = elevation(mx, my, mz), phi_m = atan2f(my, mx);
    const float inv_2pi = 0.15915494309189533577f, pi = 3.14159265358979323846f;
    // unit-square coordinates: x = elevation, y = azimuth
    const float ui_x = sqrtf(theta_i * (2.0f / pi)), ui_y = (phi_i + pi) * inv_2pi;
    const float um_x = sqrtf(theta_m * (2.0f / pi));
    float um_y = ((m.isotropic ? phi_m - phi_i : phi_m) + pi) * inv_2pi;
    um_y -= floorf(um_y);

    // incident-direction parameter slices (<= 4) and their weights
    int ip, it;
    float tp, tt;
    interval(m.phi_i, m.n_phi, phi_i, ip, tp);
    interval(m.theta_i, m.n_theta, theta_i, it, tt);
    int slice[4];
    float wgt[4];
    int ns = 0;
    for (int a = 0; a < (m.n_phi > 1 ? 2 : 1); ++a)
        for (int b = 0; b < (m.n_theta > 1 ? 2 : 1); ++b) {
            slice[ns] = (ip + a) * m.n_theta + (it + b);
            wgt[ns] = (a ? tp : 1.0f - tp) * (b ? tt : 1.0f - tt);
            ++ns;
        }

    // ---- s = VNDF^-1(u_m): invert the marginal/conditional warp of the interpolated density ----
    const int vw = m.vndf.w, vh = m.vndf.h;
    const Patch pv = patch_of(um_x, um_y, vw, vh);
    float v00 = 0.f, v10 = 0.f, v01 = 0.f, v11 = 0.f, cdf0 = 0.f, cdf1 = 0.f, r0 = 0.f, r1 = 0.f, marg = 0.f;
    for (int k = 0; k < ns; ++k) {
        const size_t base = (size_t)slice[k] * vh * vw;
        const float* d = m.vndf.data + base + (size_t)pv.iy * vw + pv.ix;
        const float* c = m.vndf_cond + base + (size_t)pv.iy * vw;
        const float w = wgt[k];
        v00 += w * d[0]; v10 += w * d[1]; v01 += w * d[vw]; v11 += w * d[vw + 1];
        cdf0 += w * c[pv.ix]; cdf1 += w * c[vw + pv.ix];
        r0 += w * c[vw - 1]; r1 += w * c[2 * vw - 1];
        marg += w * m.vndf_marg[(size_t)slice[k] * vh + pv.iy];
    }
    const float c0 = (1.0f - pv.fy) * v00 + pv.fy * v01, c1 = (1.0f - pv.fy) * v10 + pv.fy * v11;
    const float part = pv.fx * (c0 + 0.5f * pv.fx * (c1 - c0));
    const float row = (1.0f - pv.fy) * r0 + pv.fy * r1;
    const float s0 = row > 0.0f ? (part + (1.0f - pv.fy) * cdf0 + pv.fy * cdf1) / row : 0.0f;
    const float s1 = pv.fy * (r0 + 0.5f * pv.fy * (r1 - r0)) + marg;

    // ---- spectral (rgb) lookup at s ----
    const int sw = m.rgb.w, sh = m.rgb.h;
    const Patch ps = patch_of(s0, s1, sw, sh);
    for (int k = 0; k < ns; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* d = m.rgb.data + (((size_t)slice[k] * 3 + c) * sh + ps.iy) * sw + ps.ix;
            rgb[c] += wgt[k] * bilerp(d[0], d[1], d[sw], d[sw + 1], ps.fx, ps.fy);
        }
    float scale = 1.0f;
    if (m.jacobian) scale = eval_plain(m.ndf, um_x, um_y) / (4.0f * eval_plain(m.sigma, ui_x, ui_y));
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] *= scale;
    return true;
}

// ---- sample() and pdf(): the importance sampler every RGL file ships (Dupuy & Jakob 2018, Mitsuba's `measured` plugin) ----------
// u -> luminance warp -> VNDF warp -> microfacet normal m -> wo = reflect(wi, m).  Both warps are the exact inverse of the
// `invert` measured_f runs: the inverse-CDF map of the bilinear density interpolated over the incident-direction slices.  One query
// per lane; the work is two bisections per warp, each probe a gather from <= 4 slices of L2-resident tables.  The searches run a
// fixed ceil(log2(n)) trip count (wave-uniform) and the slices are addressed with compile-time indices only (no scratch).

struct Slices {  // incident-direction parameter slices (ns <= 4 of them are in use) and their weights, as measured_f forms them
    int slice[4];
    float wgt[4];
    int ns;
};
__device__ __forceinline__ Slices slices_of(const MeasuredDev& m, float phi_i, float theta_i) {
    int ip, it;
    float tp, tt;
    interval(m.phi_i, m.n_phi, phi_i, ip, tp);
    interval(m.theta_i, m.n_theta, theta_i, it, tt);
    const bool two_p = m.n_phi > 1, two_t = m.n_theta > 1;
    Slices s;
    s.ns = (two_p ? 2 : 1) * (two_t ? 2 : 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // measured_f's order: phi outer, theta inner; entries k >= ns are never read
        const int a = two_t ? k >> 1 : k, b = two_t ? k & 1 : 0;
        s.slice[k] = (ip + a) * m.n_theta + (it + b);
        s.wgt[k] = (a ? tp : 1.0f - tp) * (b ? tt : 1.0f - tt);
    }
    return s;
}

struct Warp {  // a normalised table with its CDFs: [slices][h][w], [slices][h][w], [slices][h]
    const float* data;
    const float* cond;
    const float* marg;
    int w, h;
};

// t in [0, 1] with t (c0 + a t / 2) = rem, the integral of a linear segment from c0 to c0 + a.  The textbook root
// (sqrt(c0^2 + 2 a rem) - c0) / a cancels in fp32 (wo off by up to 1e-1 on the shipped file); this form does not and needs no case
// for a = 0.
__device__ __forceinline__ float solve_segment(float c0, float a, float rem) {
    const float den = c0 + sqrtf(fmaxf(c0 * c0 + 2.0f * a * rem, 0.0f));
    return den > 0.0f ? fminf(fmaxf(2.0f * rem / den, 0.0f), 1.0f) : 0.0f;
}

// (sx, sy) uniform in [0,1)^2 -> position (px, py) distributed with the interpolated density; returns that density per unit
// area of the unit square
__device__ __forceinline__ float warp_sample(const Warp& t, const Slices& sl, float sx, float sy, float& px, float& py) {
    const int w = t.w, h = t.h;
    // last vertex row whose interpolated marginal CDF is <= sy (row 0 holds 0)
    int iy = 0;
    float m_lo = 0.0f;
    for (int len = h - 1; len > 1;) {
        const int half = len >> 1, mid = iy + half;
        float c = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < sl.ns) c += sl.wgt[k] * t.marg[(size_t)sl.slice[k] * h + mid];
        const bool up = c <= sy;
        iy = up ? mid : iy;
        m_lo = up ? c : m_lo;
        len -= half;
    }
    float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < sl.ns) {
            const float* c = t.cond + ((size_t)sl.slice[k] * h + iy) * w;
            r0 += sl.wgt[k] * c[w - 1]; r1 += sl.wgt[k] * c[2 * w - 1];
        }
    const float fy = solve_segment(r0, r1 - r0, sy - m_lo);
    const float target = sx * ((1.0f - fy) * r0 + fy * r1);
    // last column whose y-interpolated conditional CDF is <= target (column 0 holds 0)
    int ix = 0;
    float c_lo = 0.0f;
    for (int len = w - 1; len > 1;) {
        const int half = len >> 1, mid = ix + half;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < sl.ns) {
                const float* c = t.cond + ((size_t)sl.slice[k] * h + iy) * w + mid;
                a0 += sl.wgt[k] * c[0]; a1 += sl.wgt[k] * c[w];
            }
        const float c = (1.0f - fy) * a0 + fy * a1;
        const bool up = c <= target;
        ix = up ? mid : ix;
        c_lo = up ? c : c_lo;
        len -= half;
    }
    float v00 = 0.f, v10 = 0.f, v01 = 0.f, v11 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < sl.ns) {
            const float* d = t.data + ((size_t)sl.slice[k] * h + iy) * w + ix;
            v00 += sl.wgt[k] * d[0]; v10 += sl.wgt[k] * d[1]; v01 += sl.wgt[k] * d[w]; v11 += sl.wgt[k] * d[w + 1];
        }
    const float c0 = (1.0f - fy) * v00 + fy * v01, c1 = (1.0f - fy) * v10 + fy * v11;
    const float fx = solve_segment(c0, c1 - c0, target - c_lo);
    px = ((float)ix + fx) / (float)(w - 1);
    py = ((float)iy + fy) / (float)(h - 1);
    return ((1.0f - fx) * c0 + fx * c1) * (float)((w - 1) * (h - 1));
}

// position -> the variates warp_sample maps to it, and the density there (measured_f's inversion, for any warp)
__device__ __forceinline__ float warp_invert(const Warp& t, const Slices& sl, float x, float y, float& s0, float& s1) {
    const int w = t.w, h = t.h;
    const Patch p = patch_of(x, y, w, h);
    float v00 = 0.f, v10 = 0.f, v01 = 0.f, v11 = 0.f, cdf0 = 0.f, cdf1 = 0.f, r0 = 0.f, r1 = 0.f, marg = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < sl.ns) {
            const size_t base = (size_t)sl.slice[k] * h * w;
            const float* d = t.data + base + (size_t)p.iy * w + p.ix;
            const float* c = t.cond + base + (size_t)p.iy * w;
            const float wk = sl.wgt[k];
            v00 += wk * d[0]; v10 += wk * d[1]; v01 += wk * d[w]; v11 += wk * d[w + 1];
            cdf0 += wk * c[p.ix]; cdf1 += wk * c[w + p.ix];
            r0 += wk * c[w - 1]; r1 += wk * c[2 * w - 1];
            marg += wk * t.marg[(size_t)sl.slice[k] * h + p.iy];
        }
    const float c0 = (1.0f - p.fy) * v00 + p.fy * v01, c1 = (1.0f - p.fy) * v10 + p.fy * v11;
    const float part = p.fx * (c0 + 0.5f * p.fx * (c1 - c0));
    const float row = (1.0f - p.fy) * r0 + p.fy * r1;
    s0 = row > 0.0f ? (part + (1.0f - p.fy) * cdf0 + p.fy * cdf1) / row : 0.0f;
    s1 = p.fy * (r0 + 0.5f * p.fy * (r1 - r0)) + marg;
    return ((1.0f - p.fx) * c0 + p.fx * c1) * (float)((w - 1) * (h - 1));
}

// density of a normalised table at a position (per unit area of the unit square)
__device__ __forceinline__ float warp_eval(const Warp& t, const Slices& sl, float x, float y) {
    const Patch p = patch_of(x, y, t.w, t.h);
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < sl.ns) {
            const float* d = t.data + ((size_t)sl.slice[k] * t.h + p.iy) * t.w + p.ix;
            v += sl.wgt[k] * bilerp(d[0], d[1], d[t.w], d[t.w + 1], p.fx, p.fy);
        }
    return v * (float)((t.w - 1) * (t.h - 1));
}

__device__ __forceinline__ Warp vndf_warp(const MeasuredDev& m) { return Warp{m.vndf.data, m.vndf_cond, m.vndf_marg, m.vndf.w, m.vndf.h}; }
__device__ __forceinline__ Warp lum_warp(const MeasuredDev& m) { return Warp{m.lum.data, m.lum_cond, m.lum_marg, m.lum.w, m.lum.h}; }

// d omega_o / d u_m: the half-vector parameterisation's area element times the reflection's 4 (m . wi)
__device__ __forceinline__ float sample_jacobian(float um_x, float sin_theta_m, float m_dot_wi) {
    const float pi = 3.14159265358979323846f;
    return fmaxf(2.0f * pi * pi * um_x * sin_theta_m, 1e-6f) * 4.0f * m_dot_wi;
}

// sample(wi, u): wo, its solid-angle pdf and weight = f cos / pdf (untinted).  false (and all outputs 0) where wi.z <= 0.
// Where wo leaves through the lower hemisphere — or the pdf is not a positive finite number, where f cos / pdf means
// nothing — pdf = weight = 0 and wo is still written as computed.
__device__ __forceinline__ bool measured_sample(const MeasuredDev& m, float wix, float wiy, float wiz, float u0, float u1,
                                                float wo[3], float& pdf, float weight[3]) {
    wo[0] = wo[1] = wo[2] = 0.0f;
    weight[0] = weight[1] = weight[2] = 0.0f;
    pdf = 0.0f;
    if (!(wiz > 0.0f)) return false;
    const Fold fold = fold_wi(m, wix, wiy);  // wo is unfolded at the end
    const float theta_i = elevation(wix, wiy, wiz), phi_i = atan2f(wiy, wix);
    const float inv_2pi = 0.15915494309189533577f, pi = 3.14159265358979323846f;
    const float ui_x = sqrtf(theta_i * (2.0f / pi)), ui_y = (phi_i + pi) * inv_2pi;
    const Slices sl = slices_of(m, phi_i, theta_i);

    float sx = u1, sy = u0, lum_pdf = 1.0f;  // Mitsuba swaps the two variates
    if (m.lum.data) {
        float px, py;
        lum_pdf = warp_sample(lum_warp(m), sl, sx, sy, px, py);
        sx = px; sy = py;
    }
    float um_x, um_y;
    const float vndf_pdf = warp_sample(vndf_warp(m), sl, sx, sy, um_x, um_y);

    const float theta_m = um_x * um_x * (0.5f * pi);
    float phi_m = (2.0f * um_y - 1.0f) * pi;
    if (m.isotropic) phi_m += phi_i;
    float st, ct, sp, cp;
    sincosf(theta_m, &st, &ct);
    sincosf(phi_m, &sp, &cp);
    const float mx = cp * st, my = sp * st, mz = ct;
    const float d = mx * wix + my * wiy + mz * wiz;
    float wox = 2.0f * d * mx - wix, woy = 2.0f * d * my - wiy;
    const float woz = 2.0f * d * mz - wiz;
    if (fold.x) wox = -wox;
    if (fold.y) woy = -woy;
    wo[0] = wox; wo[1] = woy; wo[2] = woz;

    const float p = vndf_pdf * lum_pdf / sample_jacobian(um_x, st, d);
    if (!(woz > 0.0f && p > 0.0f && p < 3.0e38f)) return true;
    // f cos at the sampled position: the spectral lookup at s, no inversion needed
    const int sw = m.rgb.w, sh = m.rgb.h;
    const Patch ps = patch_of(sx, sy, sw, sh);
    float rgb[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < sl.ns)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* t = m.rgb.data + (((size_t)sl.slice[k] * 3 + c) * sh + ps.iy) * sw + ps.ix;
                rgb[c] += sl.wgt[k] * bilerp(t[0], t[1], t[sw], t[sw + 1], ps.fx, ps.fy);
            }
    float scale = 1.0f / p;
    if (m.jacobian) scale *= eval_plain(m.ndf, um_x, um_y) / (4.0f * eval_plain(m.sigma, ui_x, ui_y));
    pdf = p;
#pragma unroll
    for (int c = 0; c < 3; ++c) weight[c] = rgb[c] * scale;
    return true;
}

// pdf(wi, wo): the solid-angle density with which measured_sample(wi, .) returns wo; 0 on the lower hemispheres
__device__ __forceinline__ float measured_pdf(const MeasuredDev& m, float wix, float wiy, float wiz, float wox, float woy,
                                              float woz) {
    if (!(wiz > 0.0f && woz > 0.0f)) return 0.0f;
    const Fold fold = fold_wi(m, wix, wiy);
    if (fold.x) wox = -wox;
    if (fold.y) woy = -woy;
    float mx = wix + wox, my = wiy + woy, mz = wiz + woz;
    const float inv = 1.0f / fmaxf(sqrtf(mx * mx + my * my + mz * mz), 1e-30f);
    mx *= inv; my *= inv; mz *= inv;
    unsign_zeros(m, mx, my);
    const float theta_i = elevation(wix, wiy, wiz), phi_i = atan2f(wiy, wix);
    const float theta_m = elevation(mx, my, mz), phi_m = atan2f(my, mx);
    const float inv_2pi = 0.15915494309189533577f, pi = 3.14159265358979323846f;
    const float um_x = sqrtf(theta_m * (2.0f / pi));
    float um_y = ((m.isotropic ? phi_m - phi_i : phi_m) + pi) * inv_2pi;
    um_y -= floorf(um_y);
    const Slices sl = slices_of(m, phi_i, theta_i);
    float s0, s1;
    const float vndf_pdf = warp_invert(vndf_warp(m), sl, um_x, um_y, s0, s1);
    const float lum_pdf = m.lum.data ? warp_eval(lum_warp(m), sl, s0, s1) : 1.0f;
    const float p = vndf_pdf * lum_pdf / sample_jacobian(um_x, sinf(theta_m), mx * wix + my * wiy + mz * wiz);
    return p > 0.0f && p < 3.0e38f ? p : 0.0f;
}

// ---- one row of each kernel: measured.hip runs them on its one material, measured_table.hip on the material of the row's id ----
// eval(): f_o = f(wi, wo) cos * tint and, with a second direction wl (null: none), f_l = f(wi, wl) cos * tint
__device__ __forceinline__ void eval_row(const MeasuredDev& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                         const float* __restrict__ wl, long long q, Tint tint, float* __restrict__ f_o,
                                         float* __restrict__ f_l) {
    float f[3];
    measured_f(m, wi[3 * q], wi[3 * q + 1], wi[3 * q + 2], wo[3 * q], wo[3 * q + 1], wo[3 * q + 2], f);
    store3(f_o, q, f[0] * tint.r, f[1] * tint.g, f[2] * tint.b);
    if (wl) {
        measured_f(m, wi[3 * q], wi[3 * q + 1], wi[3 * q + 2], wl[3 * q], wl[3 * q + 1], wl[3 * q + 2], f);
        store3(f_l, q, f[0] * tint.r, f[1] * tint.g, f[2] * tint.b);
    }
}

// The tail of the plugins' sample() in one pass (rendering/brdf_measured_disk.py:89-101,
// brdf_measured_spherical.py:97-109): value = f * albedo / pdf on active lanes with pdf > 0, firefly rule
// pdf := 0 where lum(value) >= thr, weight = value where active, pdf > 0 and cos(theta_o) > 0, else 0.
__device__ __forceinline__ void weight_row(const MeasuredDev& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                           const float* __restrict__ pdf_in, const unsigned char* __restrict__ active,
                                           long long q, Tint tint, float thr, float* __restrict__ weight,
                                           float* __restrict__ pdf_out) {
    const float wiz = wi[3 * q + 2], woz = wo[3 * q + 2];
    float f[3];
    measured_f(m, wi[3 * q], wi[3 * q + 1], wiz, wo[3 * q], wo[3 * q + 1], woz, f);
    const float pdf = pdf_in[q];
    const bool act = wiz > 0.0f && (!active || active[q] != 0);
    float v[3] = {0.f, 0.f, 0.f};
    if (act && pdf > 0.0f) {
        const float inv = 1.0f / pdf;
        v[0] = f[0] * tint.r * inv; v[1] = f[1] * tint.g * inv; v[2] = f[2] * tint.b * inv;
    }
    const float lum = 0.2126f * v[0] + 0.7152f * v[1] + 0.0722f * v[2];  // rendering/utils/mitsuba_brdf_draw.py:36-38
    const float p = lum < thr ? pdf : 0.0f;
    const bool keep = act && p > 0.0f && woz > 0.0f;
    pdf_out[q] = p;
    store3(weight, q, keep ? v[0] : 0.0f, keep ? v[1] : 0.0f, keep ? v[2] : 0.0f);
}

// sample() / pdf(), the file's own importance sampler: a row with active[q] == 0 gets zeros
__device__ __forceinline__ void sample_row(const MeasuredDev& m, const float* __restrict__ wi, const float* __restrict__ u,
                                           const unsigned char* __restrict__ active, long long q, Tint tint,
                                           float* __restrict__ wo_out, float* __restrict__ pdf_out,
                                           float* __restrict__ weight_out) {
    float wo[3] = {0.0f, 0.0f, 0.0f}, w[3] = {0.0f, 0.0f, 0.0f}, pdf = 0.0f;
    if (!active || active[q] != 0) measured_sample(m, wi[3 * q], wi[3 * q + 1], wi[3 * q + 2], u[2 * q], u[2 * q + 1], wo, pdf, w);
    wo_out[3 * q] = wo[0]; wo_out[3 * q + 1] = wo[1]; wo_out[3 * q + 2] = wo[2];
    pdf_out[q] = pdf;
    if (weight_out) { weight_out[3 * q] = w[0] * tint.r; weight_out[3 * q + 1] = w[1] * tint.g; weight_out[3 * q + 2] = w[2] * tint.b; }
}
__device__ __forceinline__ void pdf_row(const MeasuredDev& m, const float* __restrict__ wi, const float* __restrict__ wo,
                                        const unsigned char* __restrict__ active, long long q, float* __restrict__ pdf_out) {
    float pdf = 0.0f;
    if (!active || active[q] != 0) pdf = measured_pdf(m, wi[3 * q], wi[3 * q + 1], wi[3 * q + 2], wo[3 * q], wo[3 * q + 1], wo[3 * q + 2]);
    pdf_out[q] = pdf;
}

}  // namespace measured_dev

struct bsdfd_measured_ctx {
    measured_dev::MeasuredDev dev;
    std::vector<void*> allocs;
    int device;
    std::string description;
};
