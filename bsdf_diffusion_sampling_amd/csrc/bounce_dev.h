// bounce_dev.h — the one bounce of the array-scene path tracer, and what its launcher (bounce_launch.h) and the two emitter
// samplers (pathlights.hip, pathenv.hip) share.  bounce_launch.h instantiates bounce_vertex<Mode, RR, LIST, TRANSMIT, G> behind one
// __global__ template, bounce_kernel, with those template arguments:
//
//   COSINE : only the environment emits; the light strategy is the cosine-weighted direction primary / bounce left in wl
//   LIT    : one emitter sample per vertex, uniform among n_e = point lights [+ the environment] (sample_emitter: lsel, emit)
//   ENV    : LIT, or no point lights at all, with the environment's sample drawn from its own distribution (sample_env: lpdf, emit)
//
// Where the path goes — the floor's cosine direction, the ball's BSDF sample, the trace, continue_path — is written once and
// does not depend on the mode, so the three kernels' continuation states are equal bit for bit by construction.  The modes
// differ, under `if constexpr`, in where the emitter sample comes from, in how the floor's environment term is gated or
// weighted, in the light-strategy density the escaping BSDF sample is weighted against, and in the light strategy's own term.
// Each instantiation is straight-line code of its own.  RR = true is the same body with Russian roulette in front of
// continue_path.
//
// What the scene is made of is a parameter too: a geometry policy (Spheres below, the scene of bounce.hip's and pathlights.hip's
// entry points; mesh_dev::PathGeom, the scene of mesh.hip's) answers for the closest hit, for a shadow ray and for the next
// vertex.  The estimate, the MIS weights, the roulette and the Philox counters do not depend on it.
//
// The arrays travel in small structs passed by value (kernel arguments: scalar loads); no struct is indexed per lane.
#pragma once
#include <hip/hip_runtime.h>

#include "env_dev.h"
#include "wavefront_dev.h"

namespace bounce_dev {

using namespace wf_dev;
using env_dev::EnvDist;

enum Mode { COSINE, LIT, ENV };

struct PathState {    // the path at its vertex, lane-ordered; the bounce moves it on
    float *org, *nrm, *wi, *wl;
    long long* mat;
    float *beta, *rad;
};
struct SamplerAnswer {   // of the sampler (and, f: of the ground-truth evaluator) for the vertices that carry a material
    const float *wo, *pdf_o, *pdf_l, *f_o, *f_l;
};
struct EmitterSample {   // of sample_emitter (lsel, emit) and sample_env (lpdf, emit)
    const int* lsel;
    const float *lpdf, *emit;
};
struct Step {
    int bounce, last, occlusion;
    unsigned long long seed, pass, path_offset;
    long long n;
};

// A live-lane list: the kernels' list forms run over rows[0 .. n) instead of over every lane of the wavefront.  The entries are
// distinct lanes in [0, N); a lane that is not listed keeps every byte of every array.
struct Rows {
    const long long* rows;
    long long n;
};

// this thread's lane and its material id; false beyond the wavefront and for a path that has ended.  LIST: the lane is the
// thread's entry of `rows`, false beyond the list.  (The full-width instantiations never read `rows`: it folds away.)
template <bool LIST = false>
__device__ __forceinline__ bool live_lane(const Scene& sc, long long n, const long long* __restrict__ mat, long long& p, long long& m,
                                          const Rows& rows = Rows{}) {
    p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (LIST) {
        if (p >= rows.n) return false;
        p = rows.rows[p];
        if ((unsigned long long)p >= (unsigned long long)n) return false;   // (a contract violation: skipped, not followed)
    } else {
        if (p >= n) return false;
    }
    m = mat[p];
    return m >= 0 && m <= sc.n_sph;
}

// a Philox draw of lane p's own: primary's key and counter, counter word 3 = a four-letter tag + the depth of the vertex
__device__ __forceinline__ void tagged_draw(unsigned long long seed, unsigned long long pass, unsigned long long path_offset,
                                            long long p, unsigned tag, int bounce, unsigned u[4]) {
    const unsigned long long gp = path_offset + (unsigned long long)p;
    philox4x32((unsigned)seed, (unsigned)(seed >> 32), (unsigned)gp, (unsigned)(gp >> 32), (unsigned)pass, tag + (unsigned)bounce, u);
}

// The geometry policy: the three things the path kernels ask of the scene — the closest hit of a ray that leaves the vertex of
// lane p (own surface excepted), whether a shadow ray is blocked (at all: the environment; nearer than `dist`: a point light),
// and the next vertex written at a hit.  `Spheres` is the analytic scene that travels in `Scene`: trace and continue_path, as
// they are.  mesh_dev::PathGeom (mesh_dev.h) is the instanced triangle meshes.  ONE_WALK: a hit costs a run-time loop of its
// own, so bounce_vertex forms the continuation ray of every lane first and asks once for the whole wave.
struct Spheres {
    using Hit = wf_dev::Hit;
    static constexpr bool ONE_WALK = false;
    __device__ __forceinline__ static Hit nothing() {
        Hit h;
        h.t = 3.0e38f; h.id = -1; h.c = v3(0.f, 0.f, 0.f); h.r = 1.0f;
        return h;
    }
    __device__ __forceinline__ static bool is_hit(const Hit& h) { return h.id >= 0; }
    __device__ __forceinline__ Hit closest(const Scene& sc, V3 x, V3 d, long long m, long long) const { return trace(sc, x, d, (int)m); }
    __device__ __forceinline__ bool occluded(const Scene& sc, V3 x, V3 d, long long m, long long) const {
        return trace(sc, x, d, (int)m).id >= 0;
    }
    __device__ __forceinline__ bool occluded(const Scene& sc, V3 x, V3 d, long long m, long long, float dist) const {
        const Hit h = trace(sc, x, d, (int)m);
        return h.id >= 0 && h.t < dist;
    }
    template <class... A>
    __device__ __forceinline__ void advance(const Scene& sc, const Hit& h, A... a) const { continue_path(sc, h, a...); }
};

// An emitter sample along the world direction `dir` from the vertex (x, nn) of lane p, surface m: its cosine, and whether it
// arrives — above the horizon and (occlusion) nothing nearer than `dist` in the way.
template <class G = Spheres>
__device__ __forceinline__ bool emitter_arrives(const Scene& sc, V3 x, V3 nn, V3 dir, long long m, int occlusion, float dist,
                                                bool valid, float& cosl, long long p = 0, const G& g = G{}) {
    cosl = dot(dir, nn);
    bool lit = valid && cosl > 0.0f;
    if (lit && occlusion) lit = !g.occluded(sc, x, dir, m, p, dist);
    return lit;
}

// A ball vertex is asked about its emitter sample in its own frame: wl = the local direction.  (The floor keeps the cosine
// sample in wl: it is its BSDF sample and the way on.)
__device__ __forceinline__ void store_local_direction(float* __restrict__ wl, V3 nn, V3 dir, float cosl) {
    V3 fs, ft;
    onb(nn, fs, ft);
    st3(wl, v3(dot(dir, fs), dot(dir, ft), cosl));
}

// One bounce of lane p's path: rad += beta * (the vertex' estimate), then the path moves to what its BSDF sample hits or ends.
// `e`, `n_e` and `has_env` are read by the modes that have them (ENV; LIT and ENV; LIT).
//
// RR: Russian roulette, Mitsuba's `path` integrator's rule.  From the vertex with bounce + 1 >= rr_depth on (its
// `depth >= rr_depth`, depth = the surface vertices processed so far) a path that would continue survives with probability
// q = min(max over the channels of the throughput after this vertex, 0.95) — eta is 1 here — and its throughput is divided by q.
// The variate is a Philox draw of the lane's own (counter word 3 = "Roul" + depth), made only where the decision is.  A path
// that is killed ends exactly as one that escaped; `rad` is formed and stored before, and where a survivor goes does not depend on
// the roulette: only the `thr` that continue_path multiplies into beta does.
//
// LIST: the lanes are those of `rows` (the `_rows` entry points, on either geometry); nothing else differs.  With
// G::ONE_WALK the threads beyond the list and the listed paths that have ended leave in front of the walks, as ended lanes do.
//
// G: the geometry policy.  With G::ONE_WALK the rays are formed in front of the two branches — the floor's cosine direction, the
// ball's BSDF sample, and the shadow ray along wl of a ball that looks the environment up there (COSINE; LIT where the
// environment was picked) — and the wave asks for its closest hits in one call and for its shadow rays in another: asked from inside the branches, floor lanes and ball lanes of one wave would walk one after the other.
// The branches then read the answers; with Spheres they ask where they always did, and this block folds away.
//
// TRANSMIT: a usable BSDF sample below the surface (o.z < 0, under occlusion) at a vertex with ground truth for wo is followed
// into the ball instead of being dropped, if its throughput factor f_o / pb is positive in some channel: the ray enters, or stays
// in, the ball it is on, and its hit is that ball's far side, t = -2 (x - c) . d — the far root of trace's quadratic for an origin
// on the sphere, in the form that stays well conditioned down to grazing chords.  Nothing else is intersected inside a ball (the
// host refuses scenes whose balls touch each other or the floor).  continue_path then writes the vertex as any other: it keeps
// the OUTWARD normal, so a vertex reached from inside has wi.z < 0, and the rest of this body serves it unchanged — its light
// strategy draws above the outward normal (the directions one transmission can reach), the shadow ray skips its own ball, and a
// sample with o.z > 0 leaves the surface outward whichever side wi is on.  Without ground truth (the proxy) and with f_o == 0 in
// every channel (an opaque material) such a sample ends the path as before.
template <int M, bool RR = false, bool LIST = false, bool TRANSMIT = false, class G = Spheres>
__device__ __forceinline__ void bounce_vertex(const Scene& sc, const float* __restrict__ env, const EnvDist& e, int n_e, int has_env,
                                              const Step& st, const PathState& ps, const SamplerAnswer& sa,
                                              const EmitterSample& es, int rr_depth = 0, const Rows& rows = Rows{}, const G& g = G{}) {
    static_assert(!(G::ONE_WALK && (TRANSMIT || M == ENV)), "not on meshes yet");
    long long p, m;
    if (!live_lane<LIST>(sc, st.n, ps.mat, p, m, rows)) return;
    const int occlusion = st.occlusion;
    const float inv_pi = 0.31830988618379067154f;
    // probability with which the one emitter sample went to the environment
    const float sel_p = M == COSINE ? 1.0f : 1.0f / (float)n_e;
    const bool env_emits = M != LIT || has_env;
    const V3 nn = ld3(ps.nrm + 3 * p), x = ld3(ps.org + 3 * p);
    V3 fs, ft;
    onb(nn, fs, ft);
    const V3 l = ld3(ps.wl + 3 * p);
    const V3 lw = l.x * fs + l.y * ft + l.z * nn;
    // the emitter sample: what arrives from a picked point light (LIT, ENV) or the environment's own draw (ENV), ready-made in emit
    bool point = false;
    V3 em = v3(0.f, 0.f, 0.f);
    if constexpr (M != COSINE) {
        point = (M == LIT || es.lsel) && es.lsel[p] >= 0;
        if (M == ENV || point) em = ld3(es.emit + 3 * p);
    }
    float L[3] = {0.f, 0.f, 0.f};   // the vertex' estimate, before the throughput
    float thr[3] = {1.f, 1.f, 1.f};  // throughput factor of the continuing direction
    V3 d = lw;                       // ... that direction
    typename G::Hit h = G::nothing();
    bool go = false;                 // the path continues at `h`
    bool shadowed = false;           // ONE_WALK: something lies along the ball's cosine light sample
    if constexpr (G::ONE_WALK) {
        bool ask = occlusion, ask_shadow = false;
        if (m != sc.n_sph) {
            const V3 o = ld3(sa.wo + 3 * p);
            d = o.x * fs + o.y * ft + o.z * nn;
            ask = ask && usable_pdf(sa.pdf_o[p]) > 0.0f && o.z > 0.0f;
            // (LIT: the vertices that picked the environment take the cosine strategy too)
            ask_shadow = occlusion && !point && (usable_pdf(sa.pdf_l[p]) > 0.0f || has_ground_truth(sa.f_l, p)) && l.z * inv_pi * sel_p > 0.0f;
        }
        if (ask) h = g.closest(sc, x, d, m, p);
        if (ask_shadow) shadowed = g.occluded(sc, x, lw, m, p);
    }
    if (m == sc.n_sph) {
        // diffuse floor, cosine-sampled: f cos / pdf = reflectance (in the wi slot); the direction in wl is its BSDF sample — at
        // full weight towards the environment, or (ENV) weighted against the environment's own density — and the way on
        const float refl = ps.wi[3 * p];
        if constexpr (!G::ONE_WALK) {
            if (occlusion) h = g.closest(sc, x, lw, m, p);
        }
        if (!G::is_hit(h)) {
            if (env_emits) floor_term(sc, env, lw, refl, L);
            if constexpr (M == ENV) {
                const float w = mis_power(l.z * inv_pi, env_dev::env_pdf(e, lw) * sel_p);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] *= w;
            }
        } else {
            go = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = refl;
        }
        if constexpr (M != COSINE) { L[0] += em.x; L[1] += em.y; L[2] += em.z; }
    } else {
        // the two strategies of shade_kernel
        const bool gt_o = has_ground_truth(sa.f_o, p), gt_l = has_ground_truth(sa.f_l, p);
        const V3 o = ld3(sa.wo + 3 * p);
        const float pb = usable_pdf(sa.pdf_o[p]);
        if (pb > 0.0f && (!occlusion || o.z > 0.0f)) {   // (a direction below the surface is blocked by the ball itself)
            if constexpr (!G::ONE_WALK) d = o.x * fs + o.y * ft + o.z * nn;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] = gt_o ? sa.f_o[3 * p + c] / pb : sc.albedo[c];
            if constexpr (!G::ONE_WALK) {
                if (occlusion) h = g.closest(sc, x, d, m, p);
            }
            if (G::is_hit(h)) {
                go = true;   // geometry does not emit, and a BSDF sample cannot hit a point
            } else if (env_emits) {
                // the BSDF sample escapes: the environment, weighted against the light strategy's density for this direction
                const float p_light = (M == ENV ? env_dev::env_pdf(e, d) : fmaxf(o.z, 0.0f) * inv_pi) * sel_p;
                const float w = mis_power(pb, p_light);
                float ev[3];
                env_lookup(env, sc.env_w, sc.env_h, d, ev);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    // COSINE keeps shade_kernel's expression: the compiler fuses and packs these multiply-adds by the code around
                    // them, and with thr[c] this instantiation rounds differently from the recording
                    if constexpr (M == COSINE) L[c] += w * ev[c] * (gt_o ? sa.f_o[3 * p + c] / pb : sc.albedo[c]);
                    else L[c] += w * ev[c] * thr[c];
                }
            }
        } else if constexpr (TRANSMIT) {
            if (pb > 0.0f && o.z < 0.0f && gt_o) {   // (under occlusion: the sample the branch above drops)
#pragma unroll
                for (int c = 0; c < 3; ++c) thr[c] = sa.f_o[3 * p + c] / pb;
                if (fmaxf(fmaxf(thr[0], thr[1]), thr[2]) > 0.0f) {
                    d = o.x * fs + o.y * ft + o.z * nn;
                    // its own ball, picked as trace picks the winner: a wave-uniform loop and a per-lane select (indexing sc.sph
                    // with m would turn the kernel-argument array into scratch)
                    for (int k = 0; k < sc.n_sph; ++k) {
                        const V3 c = v3(sc.sph[k][0], sc.sph[k][1], sc.sph[k][2]);
                        const float r = sc.sph[k][3];
                        if (k == (int)m) { h.c = c; h.r = r; }
                    }
                    h.id = (int)m;
                    h.t = -2.0f * dot(x - h.c, d);
                    go = true;
                }
            }
        }
        // the light strategy: f cos towards the emitter sample times what arrives
        const float pbl = usable_pdf(sa.pdf_l[p]);
        if (pbl > 0.0f || gt_l) {
            if (M == ENV || point) {
                // visibility and the density are in emit; a point is a delta and has no MIS weight, the environment's draw is
                // weighted against the sampler's density for its direction
                const float w = M == LIT || point ? 1.0f : mis_power(es.lpdf[p], pbl);
                const float ev[3] = {em.x, em.y, em.z};
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += w * ev[c] * (gt_l ? sa.f_l[3 * p + c] : sc.albedo[c] * pbl);
            } else {
                // the environment along the cosine sample (pdf cos/pi, chosen with probability sel_p), unless something is in the way
                const float pl = l.z * inv_pi * sel_p;
                bool open;   // the sample is drawn and nothing is in its way
                if constexpr (G::ONE_WALK) open = pl > 0.0f && !shadowed;
                else open = pl > 0.0f && !(occlusion && g.occluded(sc, x, lw, m, p));
                if (open) {
                    const float w = mis_power(pl, pbl) / pl;
                    float ev[3];
                    env_lookup(env, sc.env_w, sc.env_h, lw, ev);
#pragma unroll
                    for (int c = 0; c < 3; ++c) L[c] += w * ev[c] * (gt_l ? sa.f_l[3 * p + c] : sc.albedo[c] * pbl);
                }
            }
        }
    }
    const V3 b = ld3(ps.beta + 3 * p);
    const V3 r0 = ld3(ps.rad + 3 * p);
    st3(ps.rad + 3 * p, v3(r0.x + b.x * L[0], r0.y + b.y * L[1], r0.z + b.z * L[2]));
    if (!go || st.last) {
        ps.mat[p] = sc.n_sph + 1;
        return;
    }
    if constexpr (RR) {
        if (st.bounce + 1 >= rr_depth) {   // (wave-uniform)
            const float q = fminf(fmaxf(fmaxf(b.x * thr[0], b.y * thr[1]), b.z * thr[2]), 0.95f);
            unsigned u[4];
            tagged_draw(st.seed, st.pass, st.path_offset, p, 0x526F756Cu /* "Roul" */, st.bounce, u);
            if (!(q > 0.0f && (float)(u[0] >> 8) * (1.0f / 16777216.0f) < q)) {   // (a NaN q ends the path too)
                ps.mat[p] = sc.n_sph + 1;
                return;
            }
            const float inv_q = 1.0f / q;
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] *= inv_q;
        }
    }
    g.advance(sc, h, x, d, b, thr, st.seed, st.pass, st.path_offset, st.bounce, p, ps.org, ps.nrm, ps.wi, ps.wl, ps.mat, ps.beta);
}

// ---- the point emitters' sample (pathlights.hip; on meshes: mesh.hip) ----
struct Lights {
    int n;         // point emitters
    int n_e;       // emitters: n, plus one if the environment emits
    float pos[BSDFD_WF_MAX_LIGHTS][3];
    float inten[BSDFD_WF_MAX_LIGHTS][3];
};

// The emitter sample of lane p's vertex (pathlights.hip's header has the rule).  LIST: the lanes of `rows`; G: the geometry the
// shadow ray is cast in.
template <bool LIST = false, class G = Spheres>
__device__ __forceinline__ void sample_emitter_vertex(const Scene& sc, const Lights& lt, const Step& st, const float* __restrict__ org,
                                                      const float* __restrict__ nrm, const float* __restrict__ wi,
                                                      const long long* __restrict__ mat, float* __restrict__ wl,
                                                      int* __restrict__ lsel, float* __restrict__ emit, const Rows& rows = Rows{},
                                                      const G& g = G{}) {
    long long p, m;
    if (!live_lane<LIST>(sc, st.n, mat, p, m, rows)) return;
    unsigned u[4];
    tagged_draw(st.seed, st.pass, st.path_offset, p, 0x4C697465u /* "Lite" */, st.bounce, u);
    const int pick = (int)(((unsigned long long)u[0] * (unsigned long long)lt.n_e) >> 32);
    if (pick == lt.n) {   // the environment: the bounce looks it up along the cosine sample that is already in wl
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
    float cosl;
    const bool lit = emitter_arrives(sc, x, nn, dir, m, st.occlusion, dist, true, cosl, p, g);
    float s = lit ? (float)lt.n_e / d2 : 0.0f;
    if (m == sc.n_sph) s *= wi[3 * p] * 0.31830988618379067154f * cosl;   // diffuse floor: f cos = (reflectance / pi) cos
    else store_local_direction(wl + 3 * p, nn, dir, cosl);
    lsel[p] = pick;
    st3(emit + 3 * p, s * I);
}

// ---- host side ----
inline Step make_step(int32_t bounce, int32_t last, int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N) {
    return Step{(int)bounce, last ? 1 : 0, occlusion ? 1 : 0, (unsigned long long)seed, (unsigned long long)pass,
                (unsigned long long)path_offset, (long long)N};
}

// the list of a list form over arrays of N rows: at most N entries, a pointer where there are any
inline int to_rows(const int64_t* rows, int64_t n_rows, int64_t N, Rows& out) {
    if (n_rows < 0 || n_rows > N) return bsdfd_fail_(BSDFD_EINVAL, "n_rows must be in [0, N]");
    if (n_rows > 0 && !rows) return bsdfd_fail_(BSDFD_EINVAL, "null rows pointer");
    out = Rows{reinterpret_cast<const long long*>(rows), (long long)n_rows};
    return BSDFD_OK;
}

// the emitter counts of a bsdfd_wf_lights: n point lights, n_e emitters with the environment
inline int light_counts(const bsdfd_wf_lights* l, int& n, int& n_e) {
    if (!l) return bsdfd_fail_(BSDFD_EINVAL, "null lights");
    if (l->n_lights < 1 || l->n_lights > BSDFD_WF_MAX_LIGHTS) return bsdfd_fail_(BSDFD_EINVAL, "1..8 point lights");
    n = l->n_lights;
    n_e = l->n_lights + (l->has_env ? 1 : 0);
    return BSDFD_OK;
}

// the kernel-argument form of a bsdfd_wf_lights
inline int to_lights(const bsdfd_wf_lights* l, Lights& lt) {
    if (int rc = light_counts(l, lt.n, lt.n_e)) return rc;
    for (int k = 0; k < BSDFD_WF_MAX_LIGHTS; ++k)
        for (int c = 0; c < 3; ++c) {
            lt.pos[k][c] = k < lt.n ? l->position[k][c] : 0.0f;
            lt.inten[k][c] = k < lt.n ? l->intensity[k][c] : 0.0f;
        }
    return BSDFD_OK;
}

// scene + environment + distribution (of the environment's size) + emitter count of a launch over N paths
inline int env_scene(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int n_e, bool has_lsel, long long n,
                     Scene& sc, EnvDist& e) {
    if (int rc = path_scene(scene, env, n, sc)) return rc;
    if (int rc = env_dev::to_env_dist(dist, e)) return rc;
    if (e.w != sc.env_w || e.h != sc.env_h) return bsdfd_fail_(BSDFD_EINVAL, "the distribution is not of the environment map's size");
    if (n_e < 1 || n_e > BSDFD_WF_MAX_LIGHTS + 1) return bsdfd_fail_(BSDFD_EINVAL, "n_e must be 1..9: the environment and up to 8 point lights");
    if (!has_lsel && n_e != 1) return bsdfd_fail_(BSDFD_EINVAL, "without lsel the environment is the only emitter: n_e must be 1");
    return BSDFD_OK;
}

}  // namespace bounce_dev
