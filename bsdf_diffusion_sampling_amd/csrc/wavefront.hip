// wavefront.hip — the two streaming kernels of the wavefront harness.
//
// The reference renders through Mitsuba 3 (`mi.render(scene, spp=4, seed)` in a 128..256-pass loop,
// rendering/brdf_measured_disk.py:146-155), which calls the plugin's sample()/pdf() once per
// wavefront; its own helper restates the primary-ray generation (pixel index -> film position +
// jitter -> sensor ray, rendering/utils/mitsuba_helper.py:59-127) and the power-heuristic MIS
// weight (:130-137).  Mitsuba is not part of this build, so the harness drives the SAME plugin
// entry points from a minimal scene of its own: pinhole camera, one analytic sphere carrying the
// material (the "material ball" of matpreview/*.xml), a lat-long environment map, one bounce,
// BSDF sampling + cosine-hemisphere light sampling combined with the power heuristic — one
// sample() and one pdf() call per path per pass, as config 5 describes.
//
//   primary : pixel (row, col), sample s  ->  wi (local), wl (local light-sample direction),
//             world normal, world ray direction            [HBM-bound: 48 B written per path]
//   shade   : + wo, pdf(wo), pdf(wl) from the sampler      ->  film += mean over spp of the MIS estimate
//                                                          [HBM-bound: 80 B read per path]
// Both are a few dozen flops per path; they are written as plain coalesced streaming kernels.
// Path index inside a tile of rows [row_begin, row_end): ((row - row_begin) * width + col) * spp + s;
// the Philox counter is the GLOBAL path index (row * width + col) * spp + s, so an image does not
// depend on how its rows are split over GPUs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "common.h"
#include "wavefront_dev.h"

namespace {

using namespace wf_dev;

__global__ __launch_bounds__(256) void primary_kernel(Scene sc, int row_begin, int row_end, int spp,
                                                      unsigned long long seed, unsigned long long pass,
                                                      float* __restrict__ wi, float* __restrict__ wl,
                                                      float* __restrict__ nrm, float* __restrict__ dir,
                                                      long long* __restrict__ mat) {
    const long long n = (long long)(row_end - row_begin) * sc.width * spp;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long pix_local = p / spp;
    const int s = (int)(p - pix_local * spp);
    const int row = row_begin + (int)(pix_local / sc.width);
    const int col = (int)(pix_local % sc.width);
    const unsigned long long gp = ((unsigned long long)row * sc.width + col) * (unsigned long long)spp + s;
    unsigned u[4];
    philox4x32((unsigned)seed, (unsigned)(seed >> 32), (unsigned)gp, (unsigned)(gp >> 32), (unsigned)pass,
               0x57617665u /* "Wave" */, u);
    // film position in [0,1)^2 (pixel + jitter), mitsuba_helper.py:104-117
    const float jx = (float)(u[0] >> 8) * (1.0f / 16777216.0f), jy = (float)(u[1] >> 8) * (1.0f / 16777216.0f);
    const float fx = ((float)col + jx) / (float)sc.width, fy = ((float)row + jy) / (float)sc.height;
    const float sx = (2.0f * fx - 1.0f) * sc.tan_half_fov;
    const float sy = (1.0f - 2.0f * fy) * sc.tan_half_fov * ((float)sc.height / (float)sc.width);
    V3 d = sc.fwd + sx * sc.right + sy * sc.up;
    d = (1.0f / sqrtf(dot(d, d))) * d;
    // closest hit among the analytic balls and the ground plane
    float t_best = 3.0e38f;
    int hit_k = -1;
    for (int k = 0; k < sc.n_sph; ++k) {
        const V3 oc = sc.o - v3(sc.sph[k][0], sc.sph[k][1], sc.sph[k][2]);
        const float b = dot(oc, d);
        const V3 perp = oc - b * d;  // discriminant as R^2 - (distance of the centre from the ray)^2: no b^2 - c cancellation
        const float disc = sc.sph[k][3] * sc.sph[k][3] - dot(perp, perp);
        const float t = -b - sqrtf(fmaxf(disc, 0.0f));
        if (disc > 0.0f && t > 0.0f && t < t_best) { t_best = t; hit_k = k; }
    }
    bool plane = false;
    if (sc.has_plane && d.y < 0.0f) {
        const float t = (sc.plane_y - sc.o.y) / d.y;
        if (t > 0.0f && t < t_best) { t_best = t; plane = true; hit_k = -1; }
    }
    V3 nn = v3(0.f, 0.f, 0.f), w_in = v3(0.f, 0.f, 1.f);
    long long material = sc.n_sph + 1;  // miss
    if (hit_k >= 0) {
        const V3 oc = sc.o - v3(sc.sph[hit_k][0], sc.sph[hit_k][1], sc.sph[hit_k][2]);
        nn = (1.0f / sc.sph[hit_k][3]) * (oc + t_best * d);
        nn = (1.0f / sqrtf(dot(nn, nn))) * nn;
        V3 fs, ft;
        onb(nn, fs, ft);
        w_in = v3(-dot(d, fs), -dot(d, ft), -dot(d, nn));
        material = hit_k;
    } else if (plane) {  // the floor is not neural: its reflectance travels in the wi slot, its id is n_sph
        const V3 h = sc.o + t_best * d;
        const int cx = (int)floorf(h.x * sc.checker_scale), cz = (int)floorf(h.z * sc.checker_scale);
        const float refl = ((cx + cz) & 1) ? sc.checker_c1 : sc.checker_c0;
        nn = v3(0.f, 1.f, 0.f);
        w_in = v3(refl, refl, refl);
        material = sc.n_sph;
    }
    // cosine-weighted light-sample direction in the local frame
    const V3 w_l = cosine_sample(u[2], u[3]);
    st3(wi + 3 * p, w_in);
    st3(wl + 3 * p, w_l);
    st3(nrm + 3 * p, nn);
    st3(dir + 3 * p, d);
    if (mat) mat[p] = material;
}

__global__ __launch_bounds__(256) void shade_kernel(Scene sc, const float* __restrict__ env, int row_begin,
                                                    int row_end, int spp, const float* __restrict__ wo,
                                                    const float* __restrict__ pdf_o, const float* __restrict__ wl,
                                                    const float* __restrict__ pdf_l, const float* __restrict__ nrm,
                                                    const float* __restrict__ dir, const float* __restrict__ f_o,
                                                    const float* __restrict__ f_l, const float* __restrict__ wi,
                                                    const long long* __restrict__ mat, float* __restrict__ film) {
    const long long npix = (long long)(row_end - row_begin) * sc.width;
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const float inv_pi = 0.31830988618379067154f;
    add_pixel_mean(film, pix, spp, [&](long long p, float L[3]) {
        const V3 n = ld3(nrm + 3 * p);
        if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) {  // miss: the camera sees the environment
            env_lookup(env, sc.env_w, sc.env_h, ld3(dir + 3 * p), L);
        } else if (mat && mat[p] == sc.n_sph) {  // diffuse floor, cosine-sampled: f cos / pdf = reflectance
            V3 fs, ft;
            onb(n, fs, ft);
            const V3 l = ld3(wl + 3 * p);
            floor_term(sc, env, l.x * fs + l.y * ft + l.z * n, wi[3 * p], L);
        } else {
            V3 fs, ft;
            onb(n, fs, ft);
            L[0] = L[1] = L[2] = 0.0f;
            // BSDF-sampled direction: weight f cos / pdf.  With the ground truth (f_o = plugin eval(), which
            // already carries the albedo tint) that is f_o / pdf; without it the proxy f cos = albedo * pdf
            // (the nets model pdf ∝ lum(f cos)) gives weight = albedo.
            // per-path opt-out: a NaN in the f arrays selects the proxy for that path (array scenes mix materials
            // with and without a ground-truth file)
            const bool gt_o = has_ground_truth(f_o, p), gt_l = has_ground_truth(f_l, p);
            const V3 o = ld3(wo + 3 * p);
            const float pb = usable_pdf(pdf_o[p]);
            if (pb > 0.0f) {
                const float w = mis_power(pb, fmaxf(o.z, 0.0f) * inv_pi);
                float e[3];
                env_lookup(env, sc.env_w, sc.env_h, o.x * fs + o.y * ft + o.z * n, e);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * e[c] * (gt_o ? f_o[3 * p + c] / pb : sc.albedo[c]);
            }
            // light-sampled direction (cosine hemisphere, pdf cos/pi): f cos / pdf_light
            const V3 l = ld3(wl + 3 * p);
            const float pl = l.z * inv_pi;
            const float pbl = usable_pdf(pdf_l[p]);
            if (pl > 0.0f && (pbl > 0.0f || gt_l)) {
                const float w = mis_power(pl, pbl) / pl;
                float e[3];
                env_lookup(env, sc.env_w, sc.env_h, l.x * fs + l.y * ft + l.z * n, e);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * e[c] * (gt_l ? f_l[3 * p + c] : sc.albedo[c] * pbl);
            }
        }
    });
}

}  // namespace

extern "C" {

int bsdfd_wf_primary(const bsdfd_wf_scene* scene, int32_t row_begin, int32_t row_end, int32_t spp, uint64_t seed,
                     uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material, void* stream) {
    Scene sc;
    if (int rc = to_scene(scene, row_begin, row_end, spp, sc)) return rc;
    const long long n = (long long)(row_end - row_begin) * sc.width * spp;
    if (n == 0) return BSDFD_OK;
    if (!wi || !wl || !nrm || !dir) return bsdfd_fail_(BSDFD_EINVAL, "null output pointer");
    if ((n + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "tile too large for one launch");
    return launch_lanes(n, primary_kernel, stream, sc, row_begin, row_end, spp, (unsigned long long)seed,
                        (unsigned long long)pass, wi, wl, nrm, dir, reinterpret_cast<long long*>(material));
}

int bsdfd_wf_shade(const bsdfd_wf_scene* scene, const float* env, int32_t row_begin, int32_t row_end, int32_t spp,
                   const float* wo, const float* pdf_o, const float* wl, const float* pdf_l, const float* nrm,
                   const float* dir, const float* f_o, const float* f_l, const float* wi, const int64_t* material,
                   float* film, void* stream) {
    Scene sc;
    if (int rc = to_scene(scene, row_begin, row_end, spp, sc)) return rc;
    if (sc.env_w <= 0 || sc.env_h <= 0) return bsdfd_fail_(BSDFD_EINVAL, "environment map size must be positive");
    const long long npix = (long long)(row_end - row_begin) * sc.width;
    if (npix == 0) return BSDFD_OK;
    if (!env || !wo || !pdf_o || !wl || !pdf_l || !nrm || !dir || !film)
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    if (material && !wi) return bsdfd_fail_(BSDFD_EINVAL, "the material ids need the wi array (floor reflectance)");
    if (sc.has_plane && !material) return bsdfd_fail_(BSDFD_EINVAL, "a scene with a floor needs the material ids");
    return launch_lanes(npix, shade_kernel, stream, sc, env, row_begin, row_end, spp, wo, pdf_o, wl, pdf_l, nrm, dir, f_o, f_l,
                        wi, reinterpret_cast<const long long*>(material), film);
}

}  // extern "C"
