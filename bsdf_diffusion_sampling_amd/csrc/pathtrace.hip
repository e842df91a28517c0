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
//   (bounce)   : bounce.hip — per depth, with the sampler's answers for the vertices that carry a material; an ended path gets
//                material = n_balls + 1, the "miss" id: the next bucketing sorts it behind the materials and it costs no flow
//                evaluation
//   resolve    : film += mean over spp of rad
//
// A ray skips the surface it starts on (known from the material id; a sphere is convex, a plane flat): there is no epsilon
// offset.  One path per lane.
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
