// pathrr.hip — Russian roulette for the array-scene path tracer (pathtrace.hip, pathlights.hip, pathenv.hip).
//
// Six of the reference's nine array scenes are rendered by Mitsuba's `path` integrator at max_depth = -1 and its default
// rr_depth = 5: from the fifth vertex on a path survives with probability q = min(max(throughput), 0.95) and its throughput is
// divided by q, which is what makes "unbounded depth" a finite computation.  That rule, restated (parity-unpinned against
// Mitsuba, like the evaluator), sits inside the one bounce body: bounce_dev.h's bounce_vertex<Mode, RR = true>, instantiated here
// once per mode.  It needs the throughput the kernel has just formed, so a sweep of its own would cost one more streaming launch
// per depth.
//
//   bounce_rr_kernel / bounce_lit_rr_kernel / bounce_env_rr_kernel : bounce_kernel / bounce_lit_kernel / bounce_env_kernel with
//       rr_depth as one more kernel argument.  While bounce + 1 < rr_depth, and at `last`, they write what those write, bit for
//       bit, and draw nothing.  From then on a path that would continue draws u = (word 0 >> 8) 2^-24 of
//       philox(key = seed, counter = (path lo, hi, pass, "Roul" + bounce)) and continues iff q is positive and u < q, with
//       beta = beta * (thr / q); otherwise it ends as a path that escaped: material = n_balls + 1, nothing else written.
//       rad is stored before the decision and never depends on it; nor do org, nrm, wi, wl, material of a survivor.
//
// One path per lane; the scene travels by value; a lane whose path has ended returns after reading its id.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bounce_dev.h"
#include "bsdfd.h"
#include "common.h"

namespace {

using namespace bounce_dev;

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

}  // namespace

extern "C" {

int bsdfd_wf_bounce_rr(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                       uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                       float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                       const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                       const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                       void* stream) {
    if (rr_depth < 1) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 1");
    Scene sc;
    const PathState ps{org, nrm, wi, wl, reinterpret_cast<long long*>(material), beta, rad};
    const SamplerAnswer sa{wo, pdf_o, pdf_l, f_o, f_l};
    const int rr = (int)rr_depth;
    if (dist) {   // ENV: the rules of bsdfd_wf_bounce_env
        EnvDist e;
        int n_e;
        if (int rc = env_bounce_scene(scene, env, dist, lights, lsel, N, sc, e, n_e)) return rc;
        const EmitterSample es{reinterpret_cast<const int*>(lsel), lpdf, emit};
        return checked_bounce(bounce, last, occlusion, seed, pass, path_offset, N, ps, sa, emit && lpdf, [&](const Step& st) {
            return launch_lanes(N, bounce_env_rr_kernel, stream, sc, env, e, n_e, st, ps, sa, es, rr);
        });
    }
    if (int rc = path_scene(scene, env, N, sc)) return rc;
    if (lights) {   // LIT: the rules of bsdfd_wf_bounce_lit
        int n, n_e;
        if (int rc = light_counts(lights, n, n_e)) return rc;
        const EmitterSample es{reinterpret_cast<const int*>(lsel), nullptr, emit};
        return checked_bounce(bounce, last, occlusion, seed, pass, path_offset, N, ps, sa, lsel && emit, [&](const Step& st) {
            return launch_lanes(N, bounce_lit_rr_kernel, stream, sc, env, n_e, n_e - n, st, ps, sa, es, rr);
        });
    }
    // COSINE: the rules of bsdfd_wf_bounce
    return checked_bounce(bounce, last, occlusion, seed, pass, path_offset, N, ps, sa, true,
                          [&](const Step& st) { return launch_lanes(N, bounce_rr_kernel, stream, sc, env, st, ps, sa, rr); });
}

}  // extern "C"
