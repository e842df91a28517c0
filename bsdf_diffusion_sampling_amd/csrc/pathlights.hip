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
//
// The kernel's body is bounce_dev.h's sample_emitter_vertex; the kernel template and the launcher are bounce_launch.h's, which
// mesh.hip instantiates once more on the mesh scene.  These are the entry points on the analytic spheres.
// The bounce that reads lsel and emit is bounce.hip's LIT kernel.  bsdfd_wf_sample_emitter_rows is the same kernel over the lanes of
// a live-lane list (bounce_dev.h's Rows), for the deep bounces of a wavefront that has mostly ended.
// The lights travel by value in the kernel arguments like the scene; the picked light is selected by a wave-uniform loop
// with a per-lane select, because indexing the argument array per lane would move it to scratch.  One path per lane; a
// lane whose path has ended returns after reading its id.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bounce_launch.h"
#include "bsdfd.h"
#include "common.h"

using namespace bounce_dev;

extern "C" {

int bsdfd_wf_sample_emitter(const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                            uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                            const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit, void* stream) {
    return launch_sample_emitter(SpheresHost{}, scene, lights, bounce, occlusion, seed, pass, path_offset, N, org, nrm, wi, material, wl,
                                 lsel, emit, stream, nullptr);
}

int bsdfd_wf_sample_emitter_rows(const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                                 uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                                 const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit,
                                 const int64_t* rows, int64_t n_rows, void* stream) {
    Rows list;
    if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_sample_emitter(SpheresHost{}, scene, lights, bounce, occlusion, seed, pass, path_offset, N, org, nrm, wi, material, wl,
                                 lsel, emit, stream, &list);
}

}  // extern "C"
