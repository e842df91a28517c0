// bounce.hip — the bounce of the array-scene path tracer: its six kernels, their list forms, the six transmitting forms
// (bounce_dev.h: TRANSMIT — a BSDF sample below the surface is followed through the ball), their one launcher and its entry points.
//
// The bounce itself is bounce_dev.h's bounce_vertex<Mode, RR>: rad += beta * (MIS estimate of what emits, seen from the vertex);
// the path moves to the vertex its BSDF sample hits (org, nrm, wi, material, beta, a fresh light sample wl) or ends
// (material = n_balls + 1, the "miss" id).  Each kernel here is one instantiation of it:
//
//   bounce_kernel     (COSINE) : only the environment emits, both strategies cosine-weighted against each other
//   bounce_lit_kernel (LIT)    : the light strategy chosen by sample_emitter's lsel (pathlights.hip).  A point light is a delta: no
//                                MIS weight, and the BSDF strategy can never hit it.  The environment's terms are gated by has_env,
//                                and its two MIS densities carry the selection probability 1 / n_e.
//   bounce_env_kernel (ENV)    : the light term is sample_env's (pathenv.hip): mis(lpdf, pdf_l) emit f cos, no lookup along wl; the
//                                escaping BSDF samples (the floor's cosine direction included) are weighted against pdf_env / n_e.
//   bounce_rr_kernel / bounce_lit_rr_kernel / bounce_env_rr_kernel : the same three with Russian roulette, rr_depth as one more
//       kernel argument.  Six of the reference's nine array scenes are rendered by Mitsuba's `path` integrator at max_depth = -1 and
//       its default rr_depth = 5, which is what makes "unbounded depth" a finite computation; the rule is restated (parity-unpinned
//       against Mitsuba, like the evaluator) inside the one body, because it needs the throughput the kernel has just formed.
//       While bounce + 1 < rr_depth, and at `last`, they write what the plain kernels write, bit for bit, and draw nothing.  From
//       then on a path that would continue draws u = (word 0 >> 8) 2^-24 of philox(key = seed, counter = (path lo, hi, pass,
//       "Roul" + bounce)) and continues iff q is positive and u < q, with beta = beta * (thr / q); otherwise it ends as a path that
//       escaped: material = n_balls + 1, nothing else written.  rad is stored before the decision and never depends on it; nor do
//       org, nrm, wi, wl, material of a survivor.
//
// Where the path goes does not depend on the mode, so the kernels' continuation states are equal bit for bit by construction.
// One path per lane; the scene travels by value; a lane whose path has ended returns after reading its id.  Streaming kernels:
// ~125 B read and ~90 B written per live path, a few hundred flops.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "bounce_dev.h"
#include "bsdfd.h"
#include "common.h"

namespace {

using namespace bounce_dev;

__global__ __launch_bounds__(256) void bounce_kernel(Scene sc, const float* __restrict__ env, Step st, PathState ps, SamplerAnswer sa) {
    bounce_vertex<COSINE>(sc, env, EnvDist{}, 1, 1, st, ps, sa, EmitterSample{});
}

__global__ __launch_bounds__(256) void bounce_lit_kernel(Scene sc, const float* __restrict__ env, int n_e, int has_env, Step st,
                                                         PathState ps, SamplerAnswer sa, EmitterSample es) {
    bounce_vertex<LIT>(sc, env, EnvDist{}, n_e, has_env, st, ps, sa, es);
}

__global__ __launch_bounds__(256) void bounce_env_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, Step st,
                                                         PathState ps, SamplerAnswer sa, EmitterSample es) {
    bounce_vertex<ENV>(sc, env, e, n_e, 1, st, ps, sa, es);
}

__global__ __launch_bounds__(256) void bounce_rr_kernel(Scene sc, const float* __restrict__ env, Step st, PathState ps, SamplerAnswer sa,
                                                        int rr_depth) {
    bounce_vertex<COSINE, true>(sc, env, EnvDist{}, 1, 1, st, ps, sa, EmitterSample{}, rr_depth);
}

__global__ __launch_bounds__(256) void bounce_lit_rr_kernel(Scene sc, const float* __restrict__ env, int n_e, int has_env, Step st,
                                                            PathState ps, SamplerAnswer sa, EmitterSample es, int rr_depth) {
    bounce_vertex<LIT, true>(sc, env, EnvDist{}, n_e, has_env, st, ps, sa, es, rr_depth);
}

__global__ __launch_bounds__(256) void bounce_env_rr_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, Step st,
                                                            PathState ps, SamplerAnswer sa, EmitterSample es, int rr_depth) {
    bounce_vertex<ENV, true>(sc, env, e, n_e, 1, st, ps, sa, es, rr_depth);
}

// The list forms: the same six bodies over the lanes of a live-lane list (bounce_dev.h's Rows), one template with every mode's
// arguments; a mode reads its own.  They write what their full-width siblings write, on the listed lanes only.
template <int M, bool RR>
__global__ __launch_bounds__(256) void bounce_rows_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, int has_env, Step st,
                                                          PathState ps, SamplerAnswer sa, EmitterSample es, int rr_depth, Rows rows) {
    bounce_vertex<M, RR, true>(sc, env, e, M == COSINE ? 1 : n_e, M == LIT ? has_env : 1, st, ps, sa, es, rr_depth, rows);
}

template <int M, class... A>
int launch_bounce_rows(int rr_depth, const Rows& rows, void* stream, A... args) {
    return rr_depth ? launch_lanes(rows.n, bounce_rows_kernel<M, true>, stream, args..., rr_depth, rows)
                    : launch_lanes(rows.n, bounce_rows_kernel<M, false>, stream, args..., rr_depth, rows);
}

// The transmitting forms (bounce_dev.h: TRANSMIT): the same template once more, full width (LIST = false never reads `rows`) and over
// a list, with roulette only — "no roulette" is rr_depth = INT_MAX, which costs one wave-uniform comparison per lane.
template <int M, bool LIST>
__global__ __launch_bounds__(256) void bounce_transmit_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, int has_env,
                                                              Step st, PathState ps, SamplerAnswer sa, EmitterSample es, int rr_depth,
                                                              Rows rows) {
    bounce_vertex<M, true, LIST, true>(sc, env, e, M == COSINE ? 1 : n_e, M == LIT ? has_env : 1, st, ps, sa, es, rr_depth, rows);
}

template <int M, class... A>
int launch_bounce_transmit(int rr_depth, const Rows* list, long long N, void* stream, A... args) {
    const int rr = rr_depth ? rr_depth : INT_MAX;
    return list ? launch_lanes(list->n, bounce_transmit_kernel<M, true>, stream, args..., rr, *list)
                : launch_lanes(N, bounce_transmit_kernel<M, false>, stream, args..., rr, Rows{});
}

// One bounce in `mode`, with Russian roulette from rr_depth on (0: none), over all N lanes or (`list`) over the lanes of a list.
// The mode's own scene and emitter arguments are checked first, then what the modes share; a mode ignores the emitter arguments
// it does not have.
//   COSINE : none
//   LIT    : lights, lsel, emit
//   ENV    : dist, emit, lpdf; `lights` and `lsel` both NULL (n_e = 1) or both given (has_env set, n_e = n_lights + 1)
// `transmit`: the transmitting kernels, which need the ground truth (f_o).
int launch_bounce(Mode mode, int rr_depth, const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last,
                  int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                  float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o, const float* pdf_l,
                  const float* f_o, const float* f_l, const bsdfd_wf_lights* lights, const int32_t* lsel, const float* emit,
                  const float* lpdf, const bsdfd_env_dist* dist, void* stream, const Rows* list = nullptr, bool transmit = false) {
    Scene sc;
    EnvDist e{};
    int n = 0, n_e = 1;
    bool emitter_arrays = true;   // the mode's own arrays are all given
    if (mode == ENV) {
        if (lights) {
            if (lights->n_lights < 1 || lights->n_lights > BSDFD_WF_MAX_LIGHTS) return bsdfd_fail_(BSDFD_EINVAL, "1..8 point lights");
            if (!lights->has_env) return bsdfd_fail_(BSDFD_EINVAL, "the environment must be one of the emitters (has_env)");
            n_e = lights->n_lights + 1;
        }
        if ((lights == nullptr) != (lsel == nullptr) && N != 0)
            return bsdfd_fail_(BSDFD_EINVAL, "lights and lsel are both NULL or both given");
        if (int rc = env_scene(scene, env, dist, n_e, lights != nullptr, N, sc, e)) return rc;
        emitter_arrays = emit && lpdf;
    } else {
        if (int rc = path_scene(scene, env, N, sc)) return rc;
        if (mode == LIT) {
            if (int rc = light_counts(lights, n, n_e)) return rc;
            emitter_arrays = lsel && emit;
        }
    }
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if ((f_o == nullptr) != (f_l == nullptr)) return bsdfd_fail_(BSDFD_EINVAL, "f_o and f_l are both NULL or both given");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !wl || !material || !beta || !rad || !wo || !pdf_o || !pdf_l || !emitter_arrays)
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    const Step st = make_step(bounce, last, occlusion, seed, pass, path_offset, N);
    const PathState ps{org, nrm, wi, wl, reinterpret_cast<long long*>(material), beta, rad};
    const SamplerAnswer sa{wo, pdf_o, pdf_l, f_o, f_l};
    const EmitterSample es{reinterpret_cast<const int*>(lsel), mode == ENV ? lpdf : nullptr, emit};
    if (transmit) {
        if (!f_o) return bsdfd_fail_(BSDFD_EINVAL, "transmission needs the ground truth: null f_o");
        if (list && list->n == 0) return BSDFD_OK;
        switch (mode) {
            case COSINE: return launch_bounce_transmit<COSINE>(rr_depth, list, N, stream, sc, env, e, n_e, n_e - n, st, ps, sa, es);
            case LIT: return launch_bounce_transmit<LIT>(rr_depth, list, N, stream, sc, env, e, n_e, n_e - n, st, ps, sa, es);
            default: return launch_bounce_transmit<ENV>(rr_depth, list, N, stream, sc, env, e, n_e, 1, st, ps, sa, es);
        }
    }
    if (list) {
        if (list->n == 0) return BSDFD_OK;
        switch (mode) {
            case COSINE: return launch_bounce_rows<COSINE>(rr_depth, *list, stream, sc, env, e, n_e, n_e - n, st, ps, sa, es);
            case LIT: return launch_bounce_rows<LIT>(rr_depth, *list, stream, sc, env, e, n_e, n_e - n, st, ps, sa, es);
            default: return launch_bounce_rows<ENV>(rr_depth, *list, stream, sc, env, e, n_e, 1, st, ps, sa, es);
        }
    }
    switch (mode) {
        case COSINE:
            return rr_depth ? launch_lanes(N, bounce_rr_kernel, stream, sc, env, st, ps, sa, rr_depth)
                            : launch_lanes(N, bounce_kernel, stream, sc, env, st, ps, sa);
        case LIT:
            return rr_depth ? launch_lanes(N, bounce_lit_rr_kernel, stream, sc, env, n_e, n_e - n, st, ps, sa, es, rr_depth)
                            : launch_lanes(N, bounce_lit_kernel, stream, sc, env, n_e, n_e - n, st, ps, sa, es);
        default:
            return rr_depth ? launch_lanes(N, bounce_env_rr_kernel, stream, sc, env, e, n_e, st, ps, sa, es, rr_depth)
                            : launch_lanes(N, bounce_env_kernel, stream, sc, env, e, n_e, st, ps, sa, es);
    }
}

}  // namespace

extern "C" {

int bsdfd_wf_bounce(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                    uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                    float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                    const float* pdf_l, const float* f_o, const float* f_l, void* stream) {
    return launch_bounce(COSINE, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl, material, beta, rad,
                         wo, pdf_o, pdf_l, f_o, f_l, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int bsdfd_wf_bounce_lit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, void* stream) {
    return launch_bounce(LIT, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl, material, beta, rad,
                         wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, nullptr, nullptr, stream);
}

int bsdfd_wf_bounce_env(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, void* stream) {
    return launch_bounce(ENV, 0, scene, env, bounce, last, occlusion, seed, pass, path_offset, N, org, nrm, wi, wl, material, beta, rad,
                         wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist, stream);
}

int bsdfd_wf_bounce_rr(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                       uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                       float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                       const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                       const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                       void* stream) {
    if (rr_depth < 1) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 1");
    return launch_bounce(dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass, path_offset, N,
                         org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist, stream);
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
    return launch_bounce(dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass, path_offset, N,
                         org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist, stream, &list);
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
    return launch_bounce(dist ? ENV : lights ? LIT : COSINE, (int)rr_depth, scene, env, bounce, last, occlusion, seed, pass, path_offset, N,
                         org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist, stream,
                         full ? nullptr : &list, true);
}

}  // extern "C"
