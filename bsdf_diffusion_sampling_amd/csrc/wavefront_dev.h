// wavefront_dev.h — the scene model of the wavefront harness, shared by the translation units that trace it: wavefront.hip
// (primary rays, one-bounce shading), pathtrace.hip (occlusion and further bounces), pathlights.hip (point emitters) and
// pathenv.hip (importance sampling of the environment map) — the last three through bounce_dev.h, their one bounce.  They
// inline the same vector helpers, orthonormal basis, environment lookup and MIS weight, the same light sample, floor term and
// pixel mean, the same secondary ray and path continuation, and build the kernel-argument `Scene` from the same bsdfd_wf_scene.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "common.h"

namespace wf_dev {

struct V3 {
    float x, y, z;
};
__host__ __device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(float* p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// Orthonormal basis from a unit normal (Duff et al. 2017, the construction behind Mitsuba's
// coordinate_system()): s, t with (s, t, n) right-handed.
__device__ __forceinline__ void onb(V3 n, V3& s, V3& t) {
    const float sign = copysignf(1.0f, n.z);
    const float a = -1.0f / (sign + n.z);
    const float b = n.x * n.y * a;
    s = v3(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    t = v3(b, sign + n.y * n.y * a, -n.y);
}

constexpr int WF_MAX_SPHERES = 32;

struct Scene {
    V3 o, right, up, fwd;
    float tan_half_fov;
    int width, height;
    float albedo[3];
    int env_w, env_h;
    int n_sph;                       // material balls; ball k carries material k
    float sph[WF_MAX_SPHERES][4];    // centre xyz, radius
    int has_plane;                   // diffuse checkerboard ground plane y = plane_y (the matpreview scenes' floor)
    float plane_y, checker_scale, checker_c0, checker_c1;
};

// lat-long radiance map, y up: u = atan2(x, -z) / 2pi (wrapped), v = acos(y) / pi; bilinear
__device__ __forceinline__ void env_lookup(const float* __restrict__ env, int w, int h, V3 d, float out[3]) {
    float uu = atan2f(d.x, -d.z) * 0.15915494309189533577f;
    uu -= floorf(uu);
    const float vv = acosf(fminf(fmaxf(d.y, -1.0f), 1.0f)) * 0.31830988618379067154f;
    const float x = uu * (float)w - 0.5f, y = vv * (float)h - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    const float ax = x - xf, ay = y - yf;
    int x0 = (int)xf, y0 = (int)yf;
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = ((x0 % w) + w) % w; x1 = ((x1 % w) + w) % w;
    y0 = min(max(y0, 0), h - 1); y1 = min(max(y1, 0), h - 1);
    const float w00 = (1.f - ax) * (1.f - ay), w10 = ax * (1.f - ay), w01 = (1.f - ax) * ay, w11 = ax * ay;
    const float* p00 = env + ((long long)y0 * w + x0) * 3;
    const float* p10 = env + ((long long)y0 * w + x1) * 3;
    const float* p01 = env + ((long long)y1 * w + x0) * 3;
    const float* p11 = env + ((long long)y1 * w + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = w00 * p00[c] + w10 * p10[c] + w01 * p01[c] + w11 * p11[c];
}

__device__ __forceinline__ float mis_power(float pa, float pb) {  // mitsuba_helper.py:130-137
    // pa^2 / (pa^2 + pb^2), formed as 1 / (1 + (pb/pa)^2): no overflow for the 1e9+ densities of
    // near-specular lobes
    if (!(pa > 0.0f)) return 0.0f;
    const float q = pb / pa;
    return 1.0f / fmaf(q, q, 1.0f);
}

// cosine-weighted light-sample direction in the local frame, from two Philox words
__device__ __forceinline__ V3 cosine_sample(unsigned a, unsigned b) {
    const float u2 = u01_open(a), u3 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(u2);
    float sp, cp;
    sincosf(6.28318530717958647692f * u3, &sp, &cp);
    return v3(r * cp, r * sp, sqrtf(fmaxf(1.0f - u2, 0.0f)));
}

// ---- pieces of the radiance estimate at a vertex that shade_kernel and bounce_kernel share ----
// a sampler's pdf as the estimate uses it: anything but a positive finite number is 0
__device__ __forceinline__ float usable_pdf(float p) { return !(p > 0.0f) || !isfinite(p) ? 0.0f : p; }

// per-path opt-out of the ground truth: a NaN in an f array selects the proxy for that path (array scenes mix materials with
// and without a ground-truth file); so does a null array
__device__ __forceinline__ bool has_ground_truth(const float* f, long long p) { return f && f[3 * p] == f[3 * p]; }

// diffuse floor, cosine-sampled towards lw: f cos / pdf = reflectance
__device__ __forceinline__ void floor_term(const Scene& sc, const float* __restrict__ env, V3 lw, float refl, float L[3]) {
    float e[3];
    env_lookup(env, sc.env_w, sc.env_h, lw, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = refl * e[c];
}

// film[pix] += the mean over the pixel's spp paths of radiance(path, L)
template <class Radiance>
__device__ __forceinline__ void add_pixel_mean(float* __restrict__ film, long long pix, int spp, Radiance radiance) {
    float acc[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < spp; ++s) {
        float L[3];
        radiance(pix * spp + s, L);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += L[c];
    }
    const float inv = 1.0f / (float)spp;
#pragma unroll
    for (int c = 0; c < 3; ++c) film[3 * pix + c] += acc[c] * inv;
}

// ---- rays between the vertices of a path (pathtrace.hip, pathlights.hip) ----
struct Hit {
    float t;       // distance along the ray; 3e38 = nothing
    int id;        // ball index, n_sph for the floor, -1 for nothing
    V3 c;          // the winning ball's centre and radius, kept in registers by the loop: indexing sc.sph with the per-lane
    float r;       // id afterwards would turn the kernel-argument array into scratch
};

// Closest hit of the ray org + t d among the balls and the floor, the surface `own` (a material id) excepted.  `sc` is a
// kernel argument, so the loop is wave-uniform and its operands arrive through scalar loads.  Same discriminant as
// primary_kernel: R^2 - (distance of the centre from the ray)^2.
__device__ __forceinline__ Hit trace(const Scene& sc, V3 org, V3 d, int own) {
    Hit h;
    h.t = 3.0e38f; h.id = -1; h.c = v3(0.f, 0.f, 0.f); h.r = 1.0f;
    for (int k = 0; k < sc.n_sph; ++k) {
        const V3 c = v3(sc.sph[k][0], sc.sph[k][1], sc.sph[k][2]);
        const float r = sc.sph[k][3];
        const V3 oc = org - c;
        const float b = dot(oc, d);
        const V3 perp = oc - b * d;
        const float disc = r * r - dot(perp, perp);
        const float t = -b - sqrtf(fmaxf(disc, 0.0f));
        if (k != own && disc > 0.0f && t > 0.0f && t < h.t) { h.t = t; h.id = k; h.c = c; h.r = r; }
    }
    if (sc.has_plane && own != sc.n_sph && d.y < 0.0f) {
        const float t = (sc.plane_y - org.y) / d.y;
        if (t > 0.0f && t < h.t) { h.t = t; h.id = sc.n_sph; }
    }
    return h;
}

// What every geometry writes for the next vertex (xv, nv, w_in, id) of lane p: the vertex, the throughput b * thr, and its light
// sample — primary's Philox key and counter, counter word 3 advanced by the depth of the new vertex.
__device__ __forceinline__ void store_vertex(V3 xv, V3 nv, V3 w_in, long long id, V3 b, const float thr[3], unsigned long long seed,
                                             unsigned long long pass, unsigned long long path_offset, int bounce, long long p,
                                             float* __restrict__ org, float* __restrict__ nrm, float* __restrict__ wi,
                                             float* __restrict__ wl, long long* __restrict__ mat, float* __restrict__ beta) {
    const unsigned long long gp = path_offset + (unsigned long long)p;
    unsigned u[4];
    philox4x32((unsigned)seed, (unsigned)(seed >> 32), (unsigned)gp, (unsigned)(gp >> 32), (unsigned)pass,
               0x57617665u + (unsigned)(bounce + 1), u);
    st3(wl + 3 * p, cosine_sample(u[2], u[3]));
    st3(org + 3 * p, xv);
    st3(nrm + 3 * p, nv);
    st3(wi + 3 * p, w_in);
    st3(beta + 3 * p, v3(b.x * thr[0], b.y * thr[1], b.z * thr[2]));
    mat[p] = id;
}

// The path of lane p moves on to the hit `h` of the ray x + t d: the next vertex, written the way primary_kernel writes the first,
// the throughput b * thr, and the vertex' light sample.
__device__ __forceinline__ void continue_path(const Scene& sc, const Hit& h, V3 x, V3 d, V3 b, const float thr[3],
                                              unsigned long long seed, unsigned long long pass, unsigned long long path_offset,
                                              int bounce, long long p, float* __restrict__ org, float* __restrict__ nrm,
                                              float* __restrict__ wi, float* __restrict__ wl, long long* __restrict__ mat,
                                              float* __restrict__ beta) {
    V3 nv, xv, w_in;
    if (h.id < sc.n_sph) {
        const V3 oc = x - h.c;
        nv = (1.0f / h.r) * (oc + h.t * d);
        nv = (1.0f / sqrtf(dot(nv, nv))) * nv;
        V3 gs, gt;
        onb(nv, gs, gt);
        w_in = v3(-dot(d, gs), -dot(d, gt), -dot(d, nv));
        xv = h.c + h.r * nv;
    } else {
        xv = x + h.t * d;
        const int cx = (int)floorf(xv.x * sc.checker_scale), cz = (int)floorf(xv.z * sc.checker_scale);
        const float c0 = sc.checker_c0, c1 = sc.checker_c1;   // (both read: a select between the two argument loads goes per lane)
        const float refl = ((cx + cz) & 1) ? c1 : c0;
        nv = v3(0.f, 1.f, 0.f);
        w_in = v3(refl, refl, refl);
    }
    store_vertex(xv, nv, w_in, h.id, b, thr, seed, pass, path_offset, bounce, p, org, nrm, wi, wl, mat, beta);
}

// ---- host side ----
// one thread per lane in blocks of 256 on `stream`, and the launch error
template <class... P, class... A>
int launch_lanes(long long n, void (*kernel)(P...), void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
    HIP_TRY(hipGetLastError());
    return BSDFD_OK;
}

// the kernel-argument form of a bsdfd_wf_scene, validated together with the tile [row_begin, row_end) x spp
inline int to_scene(const bsdfd_wf_scene* s, int row_begin, int row_end, int spp, Scene& sc) {
    if (!s) return bsdfd_fail_(BSDFD_EINVAL, "null scene");
    if (s->width <= 0 || s->height <= 0) return bsdfd_fail_(BSDFD_EINVAL, "film size must be positive");
    if (row_begin < 0 || row_end > s->height || row_begin > row_end)
        return bsdfd_fail_(BSDFD_EINVAL, "row range outside the film");
    if (spp <= 0) return bsdfd_fail_(BSDFD_EINVAL, "spp must be positive");
    if (!(s->sphere_radius > 0.0f)) return bsdfd_fail_(BSDFD_EINVAL, "sphere radius must be positive");
    if (s->n_extra_spheres < 0 || s->n_extra_spheres > WF_MAX_SPHERES - 1)
        return bsdfd_fail_(BSDFD_EINVAL, "at most 31 extra spheres");
    sc.o = v3(s->cam_origin[0], s->cam_origin[1], s->cam_origin[2]);
    sc.right = v3(s->cam_right[0], s->cam_right[1], s->cam_right[2]);
    sc.up = v3(s->cam_up[0], s->cam_up[1], s->cam_up[2]);
    sc.fwd = v3(s->cam_forward[0], s->cam_forward[1], s->cam_forward[2]);
    sc.tan_half_fov = s->tan_half_fov;
    sc.width = s->width; sc.height = s->height;
    for (int c = 0; c < 3; ++c) sc.albedo[c] = s->albedo[c];
    sc.env_w = s->env_width; sc.env_h = s->env_height;
    sc.n_sph = 1 + s->n_extra_spheres;
    for (int c = 0; c < 3; ++c) sc.sph[0][c] = s->sphere_center[c];
    sc.sph[0][3] = s->sphere_radius;
    for (int k = 0; k < s->n_extra_spheres; ++k) {
        if (!(s->extra_spheres[k][3] > 0.0f)) return bsdfd_fail_(BSDFD_EINVAL, "sphere radius must be positive");
        for (int c = 0; c < 4; ++c) sc.sph[k + 1][c] = s->extra_spheres[k][c];
    }
    sc.has_plane = s->has_plane ? 1 : 0;
    sc.plane_y = s->plane_y; sc.checker_scale = s->checker_scale;
    sc.checker_c0 = s->checker_color0; sc.checker_c1 = s->checker_color1;
    return BSDFD_OK;
}

// scene + environment + lane count of a launch over N paths (no tile: the path kernels take N and a path offset)
inline int path_scene(const bsdfd_wf_scene* s, const float* env, long long n, Scene& sc) {
    if (int rc = to_scene(s, 0, 0, 1, sc)) return rc;
    if (sc.env_w <= 0 || sc.env_h <= 0) return bsdfd_fail_(BSDFD_EINVAL, "environment map size must be positive");
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "negative path count");
    if (n > 0 && !env) return bsdfd_fail_(BSDFD_EINVAL, "null environment map");
    if ((n + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "wavefront too large for one launch");
    return BSDFD_OK;
}

}  // namespace wf_dev
