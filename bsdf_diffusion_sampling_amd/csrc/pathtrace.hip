// pathtrace.hip — occlusion and further bounces for the array scene of the wavefront harness (wavefront.hip).
//
// The reference renders its array scenes with Mitsuba's `path` integrator at unbounded depth
// (matpreview/disney_bsdf_array*_envmap.xml: max_depth = -1): the balls shadow the floor and each other, and every
// further vertex calls the plugin's sample() / pdf() again.  The geometry is at most 32 analytic spheres and one plane,
// so the secondary rays are traced here by the same brute-force loop primary_kernel runs; the path state lives in
// lane-ordered arrays between the sampler calls:
//
//   path_begin : dir, nrm, material of bsdfd_wf_primary -> org (world position of the first vertex), beta = 1,
//                rad = env(dir) for a miss, 0 otherwise
//   bounce     : + wo, pdf(wo), pdf(wl) [, f(wo), f(wl)] of the sampler for the vertices that carry a material
//                -> rad += beta * (MIS estimate of the environment seen from the vertex); the path moves to the vertex its
//                BSDF sample hits (org, nrm, wi, material, beta, a fresh light sample wl) or ends (material = n_balls + 1,
//                the "miss" id: the next bucketing sorts it behind the materials and it costs no flow evaluation)
//   resolve    : film += mean over spp of rad
//
// Only the environment emits here (point emitters: pathlights.hip, whose bounce_lit_kernel stands in for bounce_kernel), so a
// BSDF sample that hits geometry adds nothing and a light sample that hits geometry is shadowed.  A ray skips the surface it
// starts on (known from the material id; a sphere is convex, a plane flat): there is no epsilon offset.  One path per lane; a
// lane whose path has ended returns after reading its id.  Streaming kernels: ~125 B read and ~90 B written per live path, a
// few hundred flops.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "common.h"
#include "wavefront_dev.h"

namespace {

using namespace wf_dev;

__global__ __launch_bounds__(256) void path_begin_kernel(Scene sc, const float* __restrict__ env, long long n,
                                                         const float* __restrict__ dir, const float* __restrict__ nrm,
                                                         const long long* __restrict__ mat, float* __restrict__ org,
                                                         float* __restrict__ beta, float* __restrict__ rad) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long m = mat[p];
    V3 o = v3(0.f, 0.f, 0.f);
    float L[3] = {0.f, 0.f, 0.f};
    if (m >= 0 && m < sc.n_sph) {
        V3 c = v3(0.f, 0.f, 0.f);
        float r = 0.0f;
        for (int k = 0; k < sc.n_sph; ++k)   // wave-uniform loop, per-lane select: no per-lane index into sc.sph
            if (m == k) { c = v3(sc.sph[k][0], sc.sph[k][1], sc.sph[k][2]); r = sc.sph[k][3]; }
        o = c + r * ld3(nrm + 3 * p);
    } else if (m == sc.n_sph) {
        const V3 d = ld3(dir + 3 * p);
        o = sc.o + ((sc.plane_y - sc.o.y) / d.y) * d;   // the ray/plane point primary_kernel took the checker colour at
    } else {
        env_lookup(env, sc.env_w, sc.env_h, ld3(dir + 3 * p), L);   // the camera sees the environment
    }
    st3(org + 3 * p, o);
    st3(beta + 3 * p, v3(1.f, 1.f, 1.f));
    st3(rad + 3 * p, v3(L[0], L[1], L[2]));
}

__global__ __launch_bounds__(256) void bounce_kernel(Scene sc, const float* __restrict__ env, int bounce, int last,
                                                     int occlusion, unsigned long long seed, unsigned long long pass,
                                                     unsigned long long path_offset, long long n, float* __restrict__ org,
                                                     float* __restrict__ nrm, float* __restrict__ wi, float* __restrict__ wl,
                                                     long long* __restrict__ mat, float* __restrict__ beta,
                                                     float* __restrict__ rad, const float* __restrict__ wo,
                                                     const float* __restrict__ pdf_o, const float* __restrict__ pdf_l,
                                                     const float* __restrict__ f_o, const float* __restrict__ f_l) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long m = mat[p];
    if (m < 0 || m > sc.n_sph) return;   // the path has ended
    const float inv_pi = 0.31830988618379067154f;
    const V3 nn = ld3(nrm + 3 * p), x = ld3(org + 3 * p);
    V3 fs, ft;
    onb(nn, fs, ft);
    const V3 l = ld3(wl + 3 * p);
    const V3 lw = l.x * fs + l.y * ft + l.z * nn;
    float L[3] = {0.f, 0.f, 0.f};   // the vertex' estimate, before the throughput
    float thr[3] = {1.f, 1.f, 1.f};  // throughput factor of the continuing direction
    V3 d = lw;                       // ... that direction
    Hit h;
    h.t = 3.0e38f; h.id = -1; h.c = v3(0.f, 0.f, 0.f); h.r = 1.0f;
    bool go = false;                 // the path continues at `h`
    if (m == sc.n_sph) {
        // diffuse floor, cosine-sampled: f cos / pdf = reflectance (in the wi slot); the one direction serves both purposes
        const float refl = wi[3 * p];
        if (occlusion) h = trace(sc, x, lw, (int)m);
        if (h.id < 0) {
            floor_term(sc, env, lw, refl, L);
        } else {
            go = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = refl;
        }
    } else {
        // the two strategies of shade_kernel, same expressions in the same order: a copy, because the shared form of these two
        // terms rounded differently (the compiler fuses and packs their multiply-adds by the code around them)
        const bool gt_o = has_ground_truth(f_o, p), gt_l = has_ground_truth(f_l, p);
        const V3 o = ld3(wo + 3 * p);
        const float pb = usable_pdf(pdf_o[p]);
        if (pb > 0.0f && (!occlusion || o.z > 0.0f)) {   // (a direction below the surface is blocked by the ball itself)
            d = o.x * fs + o.y * ft + o.z * nn;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = gt_o ? f_o[3 * p + c] / pb : sc.albedo[c];
            if (occlusion) h = trace(sc, x, d, (int)m);
            if (h.id < 0) {
                const float w = mis_power(pb, fmaxf(o.z, 0.0f) * inv_pi);
                float e[3];
                env_lookup(env, sc.env_w, sc.env_h, d, e);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * e[c] * (gt_o ? f_o[3 * p + c] / pb : sc.albedo[c]);
            } else {
                go = true;   // only the environment emits: nothing to add for this strategy
            }
        }
        // light-sampled direction (cosine hemisphere, pdf cos/pi): f cos / pdf_light, unless something is in the way
        const float pl = l.z * inv_pi;
        const float pbl = usable_pdf(pdf_l[p]);
        if (pl > 0.0f && (pbl > 0.0f || gt_l) && !(occlusion && trace(sc, x, lw, (int)m).id >= 0)) {
            const float w = mis_power(pl, pbl) / pl;
            float e[3];
            env_lookup(env, sc.env_w, sc.env_h, lw, e);
#pragma unroll
            for (int c = 0; c < 3; ++c) L[c] += w * e[c] * (gt_l ? f_l[3 * p + c] : sc.albedo[c] * pbl);
        }
    }
    const V3 b = ld3(beta + 3 * p);
    const V3 r0 = ld3(rad + 3 * p);
    st3(rad + 3 * p, v3(r0.x + b.x * L[0], r0.y + b.y * L[1], r0.z + b.z * L[2]));
    if (!go || last) {
        mat[p] = sc.n_sph + 1;
        return;
    }
    continue_path(sc, h, x, d, b, thr, seed, pass, path_offset, bounce, p, org, nrm, wi, wl, mat, beta);
}

__global__ __launch_bounds__(256) void resolve_kernel(long long npix, int spp, const float* __restrict__ rad,
                                                      float* __restrict__ film) {
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    add_pixel_mean(film, pix, spp, [&](long long p, float L[3]) { L[0] = rad[3 * p]; L[1] = rad[3 * p + 1]; L[2] = rad[3 * p + 2]; });
}

}  // namespace

extern "C" {

int bsdfd_wf_path_begin(const bsdfd_wf_scene* scene, const float* env, int64_t N, const float* dir, const float* nrm,
                        const int64_t* material, float* org, float* beta, float* rad, void* stream) {
    Scene sc;
    if (int rc = path_scene(scene, env, N, sc)) return rc;
    if (N == 0) return BSDFD_OK;
    if (!dir || !nrm || !material || !org || !beta || !rad) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, path_begin_kernel, stream, sc, env, (long long)N, dir, nrm, reinterpret_cast<const long long*>(material),
                        org, beta, rad);
}

int bsdfd_wf_bounce(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                    uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                    float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                    const float* pdf_l, const float* f_o, const float* f_l, void* stream) {
    Scene sc;
    if (int rc = path_scene(scene, env, N, sc)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if ((f_o == nullptr) != (f_l == nullptr)) return bsdfd_fail_(BSDFD_EINVAL, "f_o and f_l are both NULL or both given");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !wl || !material || !beta || !rad || !wo || !pdf_o || !pdf_l)
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, bounce_kernel, stream, sc, env, (int)bounce, last ? 1 : 0, occlusion ? 1 : 0, (unsigned long long)seed,
                        (unsigned long long)pass, (unsigned long long)path_offset, (long long)N, org, nrm, wi, wl,
                        reinterpret_cast<long long*>(material), beta, rad, wo, pdf_o, pdf_l, f_o, f_l);
}

int bsdfd_wf_resolve(const bsdfd_wf_scene* scene, int32_t row_begin, int32_t row_end, int32_t spp, const float* rad,
                     float* film, void* stream) {
    Scene sc;
    if (int rc = to_scene(scene, row_begin, row_end, spp, sc)) return rc;
    const long long npix = (long long)(row_end - row_begin) * sc.width;
    if (npix == 0) return BSDFD_OK;
    if (!rad || !film) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(npix, resolve_kernel, stream, npix, (int)spp, rad, film);
}

}  // extern "C"
