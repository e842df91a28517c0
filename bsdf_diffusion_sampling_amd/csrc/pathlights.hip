// pathlights.hip — point emitters for the array-scene path tracer (pathtrace.hip).
//
// Five of the reference's nine array scenes are lit by a Mitsuba `point` emitter (matpreview/disney_bsdf_array*_pointlight*.xml,
// *_spherical_pointlight.xml) instead of, or next to, the environment map.  A vertex takes ONE emitter sample, the emitter chosen
// uniformly among the n_e = n_lights + has_env emitters (Mitsuba's sample_emitter_direction), so every emitter's term carries
// the factor n_e:
//
//   sample_emitter : per live vertex, pick = (u0 * n_e) >> 32 from a Philox draw of its own (counter word 3 = "Lite" + depth).
//                    The environment: lsel = -1, wl stays the cosine sample primary / bounce wrote, emit = 0.  Point k on a ball:
//                    wl = the local direction to the light — what the sampler's pdf() and the evaluator are then asked about —
//                    and emit = n_e I_k / d^2, 0 below the horizon or (occlusion) behind another surface.  Point k on the floor:
//                    wl stays (the path continues along it), emit = the whole term n_e (refl / pi) cos I_k / d^2.
//   bounce_lit     : bounce_kernel with the light strategy chosen by lsel.  A point light is a delta: no MIS weight, and the BSDF
//                    strategy can never hit it.  The environment's two MIS densities carry the selection probability 1 / n_e.
//
// The lights travel by value in the kernel arguments like the scene; the picked light is selected by a wave-uniform loop
// with a per-lane select, because indexing the argument array per lane would move it to scratch.  One path per lane; a
// lane whose path has ended returns after reading its id.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bsdfd.h"
#include "common.h"
#include "wavefront_dev.h"

namespace {

using namespace wf_dev;

struct Lights {
    int n;         // point emitters
    int n_e;       // emitters: n, plus one if the environment emits
    float pos[BSDFD_WF_MAX_LIGHTS][3];
    float inten[BSDFD_WF_MAX_LIGHTS][3];
};

__global__ __launch_bounds__(256) void sample_emitter_kernel(Scene sc, Lights lt, int bounce, int occlusion,
                                                             unsigned long long seed, unsigned long long pass,
                                                             unsigned long long path_offset, long long n,
                                                             const float* __restrict__ org, const float* __restrict__ nrm,
                                                             const float* __restrict__ wi, const long long* __restrict__ mat,
                                                             float* __restrict__ wl, int* __restrict__ lsel,
                                                             float* __restrict__ emit) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long m = mat[p];
    if (m < 0 || m > sc.n_sph) return;   // the path has ended
    const unsigned long long gp = path_offset + (unsigned long long)p;
    unsigned u[4];
    philox4x32((unsigned)seed, (unsigned)(seed >> 32), (unsigned)gp, (unsigned)(gp >> 32), (unsigned)pass,
               0x4C697465u + (unsigned)bounce, u);
    const int pick = (int)(((unsigned long long)u[0] * (unsigned long long)lt.n_e) >> 32);
    if (pick == lt.n) {   // the environment: bounce_lit looks it up along the cosine sample that is already in wl
        lsel[p] = -1;
        st3(emit + 3 * p, v3(0.f, 0.f, 0.f));
        return;
    }
    V3 P = v3(0.f, 0.f, 0.f), I = v3(0.f, 0.f, 0.f);
    for (int k = 0; k < lt.n; ++k)   // wave-uniform loop, per-lane select: no per-lane index into lt
        if (pick == k) { P = v3(lt.pos[k][0], lt.pos[k][1], lt.pos[k][2]); I = v3(lt.inten[k][0], lt.inten[k][1], lt.inten[k][2]); }
    const V3 nn = ld3(nrm + 3 * p), x = ld3(org + 3 * p);
    const V3 v = P - x;
    const float d2 = dot(v, v);
    const float dist = sqrtf(d2);
    const V3 dir = (1.0f / dist) * v;
    const float cosl = dot(dir, nn);
    bool lit = cosl > 0.0f;
    if (lit && occlusion) {
        const Hit h = trace(sc, x, dir, (int)m);
        lit = !(h.id >= 0 && h.t < dist);
    }
    float s = lit ? (float)lt.n_e / d2 : 0.0f;
    if (m == sc.n_sph) {
        s *= wi[3 * p] * 0.31830988618379067154f * cosl;   // diffuse floor: f cos = (reflectance / pi) cos
    } else {
        V3 fs, ft;
        onb(nn, fs, ft);
        st3(wl + 3 * p, v3(dot(dir, fs), dot(dir, ft), cosl));
    }
    lsel[p] = pick;
    st3(emit + 3 * p, s * I);
}

__global__ __launch_bounds__(256) void bounce_lit_kernel(Scene sc, const float* __restrict__ env, int n_e, int has_env, int bounce,
                                                         int last, int occlusion, unsigned long long seed,
                                                         unsigned long long pass, unsigned long long path_offset, long long n,
                                                         float* __restrict__ org, float* __restrict__ nrm, float* __restrict__ wi,
                                                         float* __restrict__ wl, long long* __restrict__ mat,
                                                         float* __restrict__ beta, float* __restrict__ rad,
                                                         const float* __restrict__ wo, const float* __restrict__ pdf_o,
                                                         const float* __restrict__ pdf_l, const float* __restrict__ f_o,
                                                         const float* __restrict__ f_l, const int* __restrict__ lsel,
                                                         const float* __restrict__ emit) {
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
    const bool point = lsel[p] >= 0;
    const V3 em = point ? ld3(emit + 3 * p) : v3(0.f, 0.f, 0.f);
    float L[3] = {0.f, 0.f, 0.f};   // the vertex' estimate, before the throughput
    float thr[3] = {1.f, 1.f, 1.f};  // throughput factor of the continuing direction
    V3 d = lw;                       // ... that direction
    Hit h;
    h.t = 3.0e38f; h.id = -1; h.c = v3(0.f, 0.f, 0.f); h.r = 1.0f;
    bool go = false;                 // the path continues at `h`
    if (m == sc.n_sph) {
        // diffuse floor: the cosine direction in wl is its BSDF sample (full weight towards the environment) and the way on;
        // a picked point light arrives ready-made in emit
        const float refl = wi[3 * p];
        if (occlusion) h = trace(sc, x, lw, (int)m);
        if (h.id < 0) {
            if (has_env) floor_term(sc, env, lw, refl, L);
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
            } else if (has_env) {
                const float w = mis_power(pb, fmaxf(o.z, 0.0f) * inv_pi * sel_p);
                float e[3];
                env_lookup(env, sc.env_w, sc.env_h, d, e);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * e[c] * thr[c];
            }
        }
        const float pbl = usable_pdf(pdf_l[p]);
        if (pbl > 0.0f || gt_l) {
            if (point) {
                // delta light: f cos towards it times what arrives (visibility, 1 / d^2 and n_e are in emit); no MIS weight
                const float e[3] = {em.x, em.y, em.z};
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += e[c] * (gt_l ? f_l[3 * p + c] : sc.albedo[c] * pbl);
            } else {
                // the environment along the cosine sample, chosen with probability 1 / n_e
                const float pl = l.z * inv_pi * sel_p;
                if (pl > 0.0f && !(occlusion && trace(sc, x, lw, (int)m).id >= 0)) {
                    const float w = mis_power(pl, pbl) / pl;
                    float e[3];
                    env_lookup(env, sc.env_w, sc.env_h, lw, e);
#pragma unroll
                    for (int c = 0; c < 3; ++c) L[c] += w * e[c] * (gt_l ? f_l[3 * p + c] : sc.albedo[c] * pbl);
                }
            }
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

// the kernel-argument form of a bsdfd_wf_lights
int to_lights(const bsdfd_wf_lights* l, Lights& lt) {
    if (!l) return bsdfd_fail_(BSDFD_EINVAL, "null lights");
    if (l->n_lights < 1 || l->n_lights > BSDFD_WF_MAX_LIGHTS) return bsdfd_fail_(BSDFD_EINVAL, "1..8 point lights");
    lt.n = l->n_lights;
    lt.n_e = l->n_lights + (l->has_env ? 1 : 0);
    for (int k = 0; k < BSDFD_WF_MAX_LIGHTS; ++k)
        for (int c = 0; c < 3; ++c) {
            lt.pos[k][c] = k < lt.n ? l->position[k][c] : 0.0f;
            lt.inten[k][c] = k < lt.n ? l->intensity[k][c] : 0.0f;
        }
    return BSDFD_OK;
}

}  // namespace

extern "C" {

int bsdfd_wf_sample_emitter(const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                            uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                            const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit, void* stream) {
    Scene sc;
    Lights lt;
    if (int rc = to_scene(scene, 0, 0, 1, sc)) return rc;
    if (int rc = to_lights(lights, lt)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "negative path count");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "wavefront too large for one launch");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !material || !wl || !lsel || !emit) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, sample_emitter_kernel, stream, sc, lt, (int)bounce, occlusion ? 1 : 0, (unsigned long long)seed,
                        (unsigned long long)pass, (unsigned long long)path_offset, (long long)N, org, nrm, wi,
                        reinterpret_cast<const long long*>(material), wl, reinterpret_cast<int*>(lsel), emit);
}

int bsdfd_wf_bounce_lit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, void* stream) {
    Scene sc;
    Lights lt;
    if (int rc = path_scene(scene, env, N, sc)) return rc;
    if (int rc = to_lights(lights, lt)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if ((f_o == nullptr) != (f_l == nullptr)) return bsdfd_fail_(BSDFD_EINVAL, "f_o and f_l are both NULL or both given");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !wl || !material || !beta || !rad || !wo || !pdf_o || !pdf_l || !lsel || !emit)
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    return launch_lanes(N, bounce_lit_kernel, stream, sc, env, lt.n_e, lt.n_e - lt.n, (int)bounce, last ? 1 : 0, occlusion ? 1 : 0,
                        (unsigned long long)seed, (unsigned long long)pass, (unsigned long long)path_offset, (long long)N, org, nrm,
                        wi, wl, reinterpret_cast<long long*>(material), beta, rad, wo, pdf_o, pdf_l, f_o, f_l,
                        reinterpret_cast<const int*>(lsel), emit);
}

}  // extern "C"
