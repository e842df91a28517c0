// env_dev.h — device side of the environment map's importance sampler (pathenv.hip): a piecewise-constant density over the unit
// square of env_lookup's own (u, v) parameterisation (wavefront_dev.h: u = atan2(x, -z) / 2pi wrapped, v = theta / pi), stored as
// a marginal CDF over the rows, one conditional CDF per row and the density per cell (bsdf_diffusion_sampling_amd/envmap.py builds
// them in fp64 and rounds to fp32).  What Mitsuba's `envmap` emitter does with a bilinear Hierarchical2D over luminance x
// sin(theta) (sample_direction / pdf_direction).
//
// A cell is THE one with cdf[k] <= t < cdf[k+1]: the table entries are data and a variate is an exact fp32 number, so the choice is
// an exact decision.  The searches run a fixed ceil(log2 n) trip count with a select per probe, like measured_dev.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "wavefront_dev.h"

namespace env_dev {

using wf_dev::V3;
using wf_dev::v3;

struct EnvDist {
    const float* marg;    // [h + 1]      0 ... 1
    const float* cond;    // [h][w + 1]   each row 0 ... 1
    const float* pdf_uv;  // [h][w]       density per unit area of the (u, v) square
    int w, h;
};

// the last k in [0, n) with cdf[k] <= t (cdf[0] = 0 <= t < 1 = cdf[n]: a cell of zero width is never the answer), and the
// position of t inside that cell, in [0, 1)
__device__ __forceinline__ int cdf_cell(const float* __restrict__ cdf, int n, float t, float& off) {
    int lo = 0;
    for (int len = n; len > 1;) {   // probes lo + half <= n - 1
        const int half = len >> 1, mid = lo + half;
        lo = cdf[mid] <= t ? mid : lo;
        len -= half;
    }
    const float a = cdf[lo], b = cdf[lo + 1];
    off = fminf(fmaxf((t - a) / (b - a), 0.0f), 0.99999994f);   // (a rounded quotient may reach 1: stay inside the cell)
    return lo;
}

// the density per solid angle of a direction at polar angle theta (given by its sine) in a cell of density `cell` per (u, v) area
__device__ __forceinline__ float solid_angle_pdf(float cell, float sin_theta) {
    return cell / (19.739208802178717238f * fmaxf(sin_theta, 1e-6f));   // d omega = 2 pi^2 sin(theta) du dv
}

// (t_row, t_col) uniform in [0, 1) -> world direction d (y up) and its density per solid angle; j, i: the chosen cell
__device__ __forceinline__ float env_sample(const EnvDist& e, float t_row, float t_col, V3& d, int& j, int& i) {
    float dv, du;
    j = cdf_cell(e.marg, e.h, t_row, dv);
    i = cdf_cell(e.cond + (size_t)j * (e.w + 1), e.w, t_col, du);
    // the polar angle is measured from the nearer pole: sin(pi v) next to the south pole would lose what pi v rounds away
    const float v = ((float)j + dv) / (float)e.h;
    const bool south = v > 0.5f;
    const float theta = 3.14159265358979323846f * (south ? 1.0f - v : v);
    const float phi = 6.28318530717958647692f * (((float)i + du) / (float)e.w);
    float st, ct, sp, cp;
    sincosf(theta, &st, &ct);
    ct = south ? -ct : ct;
    sincosf(phi, &sp, &cp);
    d = v3(st * sp, ct, -st * cp);
    return solid_angle_pdf(e.pdf_uv[(size_t)j * e.w + i], st);
}

// density per solid angle with which env_sample returns the unit direction d.  theta = atan2(sin, cos) with sin = |(x, z)|: the
// same angle as env_lookup's acos(y), but an fp32 direction still resolves it next to the poles
__device__ __forceinline__ float env_pdf(const EnvDist& e, V3 d) {
    float uu = atan2f(d.x, -d.z) * 0.15915494309189533577f;
    uu -= floorf(uu);
    const float st = sqrtf(d.x * d.x + d.z * d.z);
    const float vv = atan2f(st, d.y) * 0.31830988618379067154f;
    const int i = min(max((int)(uu * (float)e.w), 0), e.w - 1);
    const int j = min(max((int)(vv * (float)e.h), 0), e.h - 1);
    return solid_angle_pdf(e.pdf_uv[(size_t)j * e.w + i], st);
}

// ---- host side ----
inline int to_env_dist(const bsdfd_env_dist* s, EnvDist& e) {
    if (!s) return bsdfd_fail_(BSDFD_EINVAL, "null environment distribution");
    if (s->width <= 0 || s->height <= 0) return bsdfd_fail_(BSDFD_EINVAL, "environment distribution size must be positive");
    if (!s->marginal || !s->conditional || !s->pdf_uv) return bsdfd_fail_(BSDFD_EINVAL, "null environment distribution table");
    e.marg = s->marginal; e.cond = s->conditional; e.pdf_uv = s->pdf_uv;
    e.w = s->width; e.h = s->height;
    return BSDFD_OK;
}

}  // namespace env_dev
