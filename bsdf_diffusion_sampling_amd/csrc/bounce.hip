// bounce.hip — the bounce of the array-scene path tracer on the analytic spheres: its entry points.  The kernel template and the
// launcher are bounce_launch.h's, which mesh.hip instantiates once more on the triangle meshes; the body is bounce_dev.h's.
//
// The bounce itself is bounce_dev.h's bounce_vertex<Mode, RR, LIST, TRANSMIT, G>: rad += beta * (MIS estimate of what emits, seen
// from the vertex); the path moves to the vertex its BSDF sample hits (org, nrm, wi, material, beta, a fresh light sample wl) or
// ends (material = n_balls + 1, the "miss" id).  Every entry point here launches one instantiation of bounce_launch.h's
// bounce_kernel with G = Spheres:
//
//   COSINE (bsdfd_wf_bounce)     : only the environment emits, both strategies cosine-weighted against each other
//   LIT    (bsdfd_wf_bounce_lit) : the light strategy chosen by sample_emitter's lsel (pathlights.hip).  A point light is a delta: no
//                                  MIS weight, and the BSDF strategy can never hit it.  The environment's terms are gated by has_env,
//                                  and its two MIS densities carry the selection probability 1 / n_e.
//   ENV    (bsdfd_wf_bounce_env) : the light term is sample_env's (pathenv.hip): mis(lpdf, pdf_l) emit f cos, no lookup along wl; the
//                                  escaping BSDF samples (the floor's cosine direction included) are weighted against pdf_env / n_e.
//   RR     (bsdfd_wf_bounce_rr)  : the same three with Russian roulette from rr_depth on.  Six of the reference's nine array scenes
//       are rendered by Mitsuba's `path` integrator at max_depth = -1 and
//       its default rr_depth = 5, which is what makes "unbounded depth" a finite computation; the rule is restated (parity-unpinned
//       against Mitsuba, like the evaluator) inside the one body, because it needs the throughput the kernel has just formed.
//       While bounce + 1 < rr_depth, and at `last`, they write what the plain kernels write, bit for bit, and draw nothing.  From
//       then on a path that would continue draws u = (word 0 >> 8) 2^-24 of philox(key = seed, counter = (path lo, hi, pass,
//       "Roul" + bounce)) and continues iff q is positive and u < q, with beta = beta * (thr / q); otherwise it ends as a path that
//       escaped: material = n_balls + 1, nothing else written.  rad is stored before the decision and never depends on it; nor do
//       org, nrm, wi, wl, material of a survivor.
//   LIST   (bsdfd_wf_bounce_rows) : the same six over the lanes of a live-lane list (bounce_dev.h's Rows); they write what their
//       full-width siblings write, on the listed lanes only.
//   TRANSMIT (bsdfd_wf_bounce_transmit) : a BSDF sample below the surface is followed through the ball (bounce_dev.h), full width
//       and over a list, with roulette only — "no roulette" is rr_depth = INT_MAX.
//
// Where the path goes does not depend on the mode, so the modes' continuation states are equal bit for bit by construction.
// One path per lane; the scene travels by value; a lane whose path has ended returns after reading its id.  Streaming kernels:
// ~125 B read and ~90 B written per live path, a few hundred flops.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bounce_launch.h"
#include "bsdfd.h"
#include "common.h"

using namespace bounce_dev;

extern "C" {

int bsdfd_wf_bounce(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                    uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                    float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                    const float* pdf_l, const float* f_o, const float* f_l, void* stream) {
    return launch_bounce(SpheresHost{}, COSINE, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl,
                         material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int bsdfd_wf_bounce_lit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, void* stream) {
    return launch_bounce(SpheresHost{}, LIT, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl,
                         material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, nullptr, nullptr, stream);
}

int bsdfd_wf_bounce_env(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, void* stream) {
    return launch_bounce(SpheresHost{}, ENV, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl,
                         material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist, stream);
}

int bsdfd_wf_bounce_rr(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                       uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                       float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                       const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                       const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                       void* stream) {
    if (rr_depth < 1) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 1");
    return launch_bounce(SpheresHost{}, dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass,
                         path_offset, N, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist,
                         stream);
}

int bsdfd_wf_bounce_rows(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                         uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                         float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                         const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                         const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                         const int64_t* rows, int64_t n_rows, void* stream) {
    if (rr_depth < 0) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 0 (0: no Russian roulette)");
    Rows list;
    if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_bounce(SpheresHost{}, dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass,
                         path_offset, N, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist,
                         stream, &list);
}

int bsdfd_wf_bounce_transmit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                             uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                             float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                             const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                             const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                             const int64_t* rows, int64_t n_rows, void* stream) {
    if (rr_depth < 0) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 0 (0: no Russian roulette)");
    const bool full = !rows && n_rows == 0;   // no list at all: every lane
    Rows list{};
    if (!full)
        if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_bounce(SpheresHost{}, dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass,
                         path_offset, N, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist,
                         stream,
                         full ? nullptr : &list, true);
}

}  // extern "C"
