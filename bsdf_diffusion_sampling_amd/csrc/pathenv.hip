// pathenv.hip — importance sampling of the environment map in the array-scene path tracer (pathtrace.hip, pathlights.hip).
//
// Four of the reference's nine array scenes (matpreview/disney_bsdf_array{0,1}_envmap.xml, disney_bsdf_array2_spherical_envmap.xml,
// scene_measured.xml) are lit by a Mitsuba `envmap` emitter, which draws directions in proportion to the map's luminance
// (sample_direction / pdf_direction).  Here the light strategy of a vertex that picked the environment becomes a draw from the
// piecewise-constant distribution of env_dev.h instead of the cosine-weighted direction primary / bounce left in wl:
//
//   env_sample / env_pdf : the distribution row by row (parity tests, tools)
//   sample_env : per live vertex that picked the environment (lsel == -1, or every live vertex without lights), a direction from a
//                Philox draw of its own (counter word 3 = "Envm" + depth), with p_l = pdf_env / n_e.  On a ball: wl = the local
//                direction — what the sampler's pdf() and the evaluator are then asked about —, lpdf = p_l, emit = E V / p_l, 0
//                below the horizon or (occlusion) behind a surface.  On the floor: wl stays (the cosine direction is the floor's
//                BSDF sample and the way on), emit = the whole term mis(p_l, cos/pi) (refl/pi) cos E V / p_l.
//   bounce_env : bounce_lit_kernel with that light term; the escaping BSDF samples (the floor's cosine direction included) are
//                weighted against pdf_env / n_e.  Where the path goes is bounce_kernel's, unchanged.
//
// One path per lane; the scene travels by value; a lane whose path has ended returns after reading its id.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsdfd.h"
#include "common.h"
#include "env_dev.h"
#include "wavefront_dev.h"

namespace {

using namespace wf_dev;
using env_dev::EnvDist;

__global__ __launch_bounds__(256) void env_sample_kernel(EnvDist e, long long n, const float* __restrict__ u,
                                                         float* __restrict__ dir, float* __restrict__ pdf) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    V3 d;
    int j, i;
    pdf[q] = env_dev::env_sample(e, u[2 * q], u[2 * q + 1], d, j, i);
    st3(dir + 3 * q, d);
}

__global__ __launch_bounds__(256) void env_pdf_kernel(EnvDist e, long long n, const float* __restrict__ dir,
                                                      float* __restrict__ pdf) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf[q] = env_dev::env_pdf(e, ld3(dir + 3 * q));
}

__global__ __launch_bounds__(256) void sample_env_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, int bounce,
                                                         int occlusion, unsigned long long seed, unsigned long long pass,
                                                         unsigned long long path_offset, long long n,
                                                         const float* __restrict__ org, const float* __restrict__ nrm,
                                                         const float* __restrict__ wi, const long long* __restrict__ mat,
                                                         const int* __restrict__ lsel, float* __restrict__ wl,
                                                         float* __restrict__ lpdf, float* __restrict__ emit) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long m = mat[p];
    if (m < 0 || m > sc.n_sph) return;   // the path has ended
    if (lsel && lsel[p] != -1) return;   // a point light was picked: sample_emitter's wl and emit stand
    const unsigned long long gp = path_offset + (unsigned long long)p;
    unsigned u[4];
    philox4x32((unsigned)seed, (unsigned)(seed >> 32), (unsigned)gp, (unsigned)(gp >> 32), (unsigned)pass,
               0x456E766Du + (unsigned)bounce, u);
    V3 d;
    int j, i;
    const float p_l = env_dev::env_sample(e, (float)(u[0] >> 8) * (1.0f / 16777216.0f), (float)(u[1] >> 8) * (1.0f / 16777216.0f),
                                          d, j, i) / (float)n_e;
    const V3 nn = ld3(nrm + 3 * p), x = ld3(org + 3 * p);
    const float cosl = dot(d, nn);
    bool lit = cosl > 0.0f && p_l > 0.0f;
    if (lit && occlusion) lit = trace(sc, x, d, (int)m).id < 0;
    float s = 0.0f;
    float E[3] = {0.f, 0.f, 0.f};
    if (lit) {
        env_lookup(env, sc.env_w, sc.env_h, d, E);
        s = 1.0f / p_l;
    }
    if (m == sc.n_sph) {
        // diffuse floor: f cos = (reflectance / pi) cos, weighted against the cosine strategy bounce_env runs along wl
        const float inv_pi = 0.31830988618379067154f;
        s *= mis_power(p_l, cosl * inv_pi) * wi[3 * p] * inv_pi * cosl;
    } else {
        V3 fs, ft;
        onb(nn, fs, ft);
        st3(wl + 3 * p, v3(dot(d, fs), dot(d, ft), cosl));
    }
    lpdf[p] = p_l;
    st3(emit + 3 * p, v3(s * E[0], s * E[1], s * E[2]));
}

__global__ __launch_bounds__(256) void bounce_env_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, int bounce,
                                                         int last, int occlusion, unsigned long long seed,
                                                         unsigned long long pass, unsigned long long path_offset, long long n,
                                                         float* __restrict__ org, float* __restrict__ nrm, float* __restrict__ wi,
                                                         float* __restrict__ wl, long long* __restrict__ mat,
                                                         float* __restrict__ beta, float* __restrict__ rad,
                                                         const float* __restrict__ wo, const float* __restrict__ pdf_o,
                                                         const float* __restrict__ pdf_l, const float* __restrict__ f_o,
                                                         const float* __restrict__ f_l, const int* __restrict__ lsel,
                                                         const float* __restrict__ lpdf, const float* __restrict__ emit) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long m = mat[p];
    if (m < 0 || m > sc.n_sph) return;   // the path has ended
    const float inv_pi = 0.31830988618379067154f;
    const float sel_p = 1.0f / (float)n_e;   // probability with which the one emitter sample went to the environment
    const V3 nn = ld3(nrm + 3 * p), x = ld3(org + 3 * p);
    V3 fs, ft;
    onb(nn, fs, ft);
    const V3 l = ld3(wl + 3 * p);
    const V3 lw = l.x * fs + l.y * ft + l.z * nn;
    const bool point = lsel && lsel[p] >= 0;
    const V3 em = ld3(emit + 3 * p);
    float L[3] = {0.f, 0.f, 0.f};   // the vertex' estimate, before the throughput
    float thr[3] = {1.f, 1.f, 1.f};  // throughput factor of the continuing direction
    V3 d = lw;                       // ... that direction
    Hit h;
    h.t = 3.0e38f; h.id = -1; h.c = v3(0.f, 0.f, 0.f); h.r = 1.0f;
    bool go = false;                 // the path continues at `h`
    if (m == sc.n_sph) {
        // diffuse floor: the cosine direction in wl is its BSDF sample, weighted against the environment's own density where it
        // escapes, and the way on; the emitter sample arrives ready-made in emit
        const float refl = wi[3 * p];
        if (occlusion) h = trace(sc, x, lw, (int)m);
        if (h.id < 0) {
            floor_term(sc, env, lw, refl, L);
            const float w = mis_power(l.z * inv_pi, env_dev::env_pdf(e, lw) * sel_p);
#pragma unroll
            for (int c = 0; c < 3; ++c) L[c] *= w;
        } else {
            go = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = refl;
        }
        L[0] += em.x; L[1] += em.y; L[2] += em.z;
    } else {
        const bool gt_o = has_ground_truth(f_o, p), gt_l = has_ground_truth(f_l, p);
        const V3 o = ld3(wo + 3 * p);
        const float pb = usable_pdf(pdf_o[p]);
        if (pb > 0.0f && (!occlusion || o.z > 0.0f)) {   // (a direction below the surface is blocked by the ball itself)
            d = o.x * fs + o.y * ft + o.z * nn;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = gt_o ? f_o[3 * p + c] / pb : sc.albedo[c];
            if (occlusion) h = trace(sc, x, d, (int)m);
            if (h.id >= 0) {
                go = true;   // geometry does not emit, and a BSDF sample cannot hit a point
            } else {
                const float w = mis_power(pb, env_dev::env_pdf(e, d) * sel_p);
                float ev[3];
                env_lookup(env, sc.env_w, sc.env_h, d, ev);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * ev[c] * thr[c];
            }
        }
        const float pbl = usable_pdf(pdf_l[p]);
        if (pbl > 0.0f || gt_l) {
            // f cos towards the emitter sample times what arrives (visibility and the density are in emit); a point is a delta
            // and has no MIS weight, the environment's draw is weighted against the sampler's density for its direction
            const float w = point ? 1.0f : mis_power(lpdf[p], pbl);
            const float ev[3] = {em.x, em.y, em.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) L[c] += w * ev[c] * (gt_l ? f_l[3 * p + c] : sc.albedo[c] * pbl);
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

// scene + environment + distribution (of the environment's size) + emitter count of a launch over N paths
int env_scene(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int n_e, bool has_lsel, long long n,
              Scene& sc, EnvDist& e) {
    if (int rc = path_scene(scene, env, n, sc)) return rc;
    if (int rc = env_dev::to_env_dist(dist, e)) return rc;
    if (e.w != sc.env_w || e.h != sc.env_h) return bsdfd_fail_(BSDFD_EINVAL, "the distribution is not of the environment map's size");
    if (n_e < 1 || n_e > BSDFD_WF_MAX_LIGHTS + 1) return bsdfd_fail_(BSDFD_EINVAL, "n_e must be 1..9: the environment and up to 8 point lights");
    if (!has_lsel && n_e != 1) return bsdfd_fail_(BSDFD_EINVAL, "without lsel the environment is the only emitter: n_e must be 1");
    return BSDFD_OK;
}

}  // namespace

extern "C" {

int bsdfd_env_sample(const bsdfd_env_dist* dist, int64_t N, const float* u, float* dir, float* pdf, void* stream) {
    EnvDist e;
    if (int rc = env_dev::to_env_dist(dist, e)) return rc;
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "negative row count");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "too many rows for one launch");
    if (N == 0) return BSDFD_OK;
    if (!u || !dir || !pdf) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, env_sample_kernel, stream, e, (long long)N, u, dir, pdf);
}

int bsdfd_env_pdf(const bsdfd_env_dist* dist, int64_t N, const float* dir, float* pdf, void* stream) {
    EnvDist e;
    if (int rc = env_dev::to_env_dist(dist, e)) return rc;
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "negative row count");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "too many rows for one launch");
    if (N == 0) return BSDFD_OK;
    if (!dir || !pdf) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, env_pdf_kernel, stream, e, (long long)N, dir, pdf);
}

int bsdfd_wf_sample_env(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int32_t n_e, int32_t bounce,
                        int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                        const float* nrm, const float* wi, const int64_t* material, const int32_t* lsel, float* wl, float* lpdf,
                        float* emit, void* stream) {
    Scene sc;
    EnvDist e;
    if (int rc = env_scene(scene, env, dist, n_e, lsel != nullptr, N, sc, e)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !material || !wl || !lpdf || !emit) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, sample_env_kernel, stream, sc, env, e, (int)n_e, (int)bounce, occlusion ? 1 : 0,
                        (unsigned long long)seed, (unsigned long long)pass, (unsigned long long)path_offset, (long long)N, org, nrm,
                        wi, reinterpret_cast<const long long*>(material), reinterpret_cast<const int*>(lsel), wl, lpdf, emit);
}

int bsdfd_wf_bounce_env(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, void* stream) {
    Scene sc;
    EnvDist e;
    int n_e = 1;
    if (lights) {
        if (lights->n_lights < 1 || lights->n_lights > BSDFD_WF_MAX_LIGHTS) return bsdfd_fail_(BSDFD_EINVAL, "1..8 point lights");
        if (!lights->has_env) return bsdfd_fail_(BSDFD_EINVAL, "the environment must be one of the emitters (has_env)");
        n_e = lights->n_lights + 1;
    }
    if ((lights == nullptr) != (lsel == nullptr) && N != 0)
        return bsdfd_fail_(BSDFD_EINVAL, "lights and lsel are both NULL or both given");
    if (int rc = env_scene(scene, env, dist, n_e, lights != nullptr, N, sc, e)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if ((f_o == nullptr) != (f_l == nullptr)) return bsdfd_fail_(BSDFD_EINVAL, "f_o and f_l are both NULL or both given");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !wl || !material || !beta || !rad || !wo || !pdf_o || !pdf_l || !emit || !lpdf)
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, bounce_env_kernel, stream, sc, env, e, n_e, (int)bounce, last ? 1 : 0, occlusion ? 1 : 0,
                        (unsigned long long)seed, (unsigned long long)pass, (unsigned long long)path_offset, (long long)N, org, nrm,
                        wi, wl, reinterpret_cast<long long*>(material), beta, rad, wo, pdf_o, pdf_l, f_o, f_l,
                        reinterpret_cast<const int*>(lsel), lpdf, emit);
}

}  // extern "C"
