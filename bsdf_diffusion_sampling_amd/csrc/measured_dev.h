// measured_dev.h — device side of the RGL measured-BSDF evaluator (the model and the host part: measured.hip), shared by
// the translation units that evaluate it: measured.hip (one material per launch) and measured_table.hip (a mixed-material
// wavefront in one launch).  Both inline the same measured_f and compute the same bits (see the pragma below).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "bsdfd.h"

// Fused multiply-adds are formed per source expression, by the front end, from here to the end of the including translation
// unit — not wherever the optimiser finds a product next to a sum (hipcc's default): that choice depends on the code around an
// inlined copy (which pairs the vectoriser packs, which of a*b + c*d becomes the fma's product), and it made the kernels of
// measured.hip and measured_table.hip round the same expressions differently.  With this both compute the same bits.
#pragma clang fp contract(on)

namespace measured_dev {

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

// f(wi, wo) cos(theta_o) for one pair; false (and rgb = 0) on the lower hemispheres
__device__ __forceinline__ bool measured_f(const MeasuredDev& m, float wix, float wiy, float wiz, float wox, float woy,
                                           float woz, float rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (!(wiz > 0.0f && woz > 0.0f)) return false;
    if (m.reduction >= 2) {
        // Symmetries of an anisotropic acquisition: only phi_i in a half-plane (reduction 2: point symmetry)
        // or a quadrant (reduction 4: two mirror planes) is stored.  Mitsuba folds with mulsign_neg(v, s) =
        // -|..|, i.e. into y <= 0 (and x <= 0), which is where its files keep phi_i; here the target is read
        // off the file's own phi_i range, which is the same thing for such files and right for any other.
        const bool fy = wiy * m.fold_y < 0.0f;
        const bool fx = m.reduction == 4 ? (wix * m.fold_x < 0.0f) : fy;
        if (fx) { wix = -wix; wox = -wox; }
        if (fy) { wiy = -wiy; woy = -woy; }
    }
    float mx = wix + wox, my = wiy + woy, mz = wiz + woz;
    const float inv = 1.0f / fmaxf(sqrtf(mx * mx + my * my + mz * mz), 1e-30f);
    mx *= inv; my *= inv; mz *= inv;
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

struct Tint {
    float r, g, b;
};

}  // namespace measured_dev

struct bsdfd_measured_ctx {
    measured_dev::MeasuredDev dev;
    std::vector<void*> allocs;
    int device;
    std::string description;
};
