// bounce_launch.h — the two stages of the path tracer that ask the geometry something, the bounce and the point emitters' sample,
// from the kernel to the launch: ONE __global__ template and ONE launcher each, for every mode, with and without roulette, full
// width and over a live-lane list, transmitting or not, on the spheres (bounce.hip, pathlights.hip) and on the meshes (mesh.hip).
//
// The kernels forward to bounce_dev.h's bounce_vertex / sample_emitter_vertex with their own template arguments, so an entry point
// reaches the instantiation its arguments name.  One argument list: an instantiation reads what it has — `e` in ENV, `n_e` in LIT
// and ENV, `has_env` in LIT, `es` outside COSINE, `rr_depth` with RR, `rows` with LIST, `g` where the policy has members (Spheres
// is empty) — and the rest are kernel arguments nobody loads.
//
// What a launcher asks of the scene behind the geometry policy is the policy's host side, a small struct (SpheresHost below,
// mesh.hip's MeshHost):
//   Geom               the device-side policy (bounce_dev.h)
//   EMPTY_LIST_FIRST   an empty list is a no-op whatever the pointers, as N == 0 is: it takes N's place in the checks that go by
//                      the lane count.  (On the spheres an empty list returns where its launch would have been, behind the
//                      null-pointer test.)
//   admit(lpdf, dist)  the first check of all: the scene handle, and the emitter arguments the geometry has no kernel for
//   arrays()           the policy's own per-lane arrays are given (part of the null-pointer test)
//   geometry(sc, g)    the last checks, which may ask the device, and the kernel argument
#pragma once
#include <climits>
#include <cstdint>
#include <type_traits>

#include "bounce_dev.h"

namespace bounce_dev {

template <int M, bool RR, bool LIST, bool TRANSMIT, class G>
__global__ __launch_bounds__(256) void bounce_kernel(Scene sc, G g, const float* __restrict__ env, EnvDist e, int n_e, int has_env, Step st,
                                                     PathState ps, SamplerAnswer sa, EmitterSample es, int rr_depth, Rows rows) {
    bounce_vertex<M, RR, LIST, TRANSMIT, G>(sc, env, e, M == COSINE ? 1 : n_e, M == LIT ? has_env : 1, st, ps, sa, es, rr_depth, rows, g);
}

template <bool LIST, class G>
__global__ __launch_bounds__(256) void sample_emitter_kernel(Scene sc, G g, Lights lt, Step st, const float* __restrict__ org,
                                                             const float* __restrict__ nrm, const float* __restrict__ wi,
                                                             const long long* __restrict__ mat, float* __restrict__ wl,
                                                             int* __restrict__ lsel, float* __restrict__ emit, Rows rows) {
    sample_emitter_vertex<LIST, G>(sc, lt, st, org, nrm, wi, mat, wl, lsel, emit, rows, g);
}

struct SpheresHost {   // the analytic scene travels in `Scene`: nothing to admit, no array, no handle
    using Geom = Spheres;
    static constexpr bool EMPTY_LIST_FIRST = false;
    int admit(const float*, const bsdfd_env_dist*) const { return BSDFD_OK; }
    bool arrays() const { return true; }
    int geometry(const Scene&, Spheres&) const { return BSDFD_OK; }
};

// The emitter sample over all N lanes, or (`list`, which to_rows has checked against N) over the lanes of a list.  The checks, in
// the order a caller sees them fail:
//   1. host.admit                                     4. N == 0 (EMPTY_LIST_FIRST: or an empty list): BSDFD_OK
//   2. the scene, then the lights                     5. null pointers, host.arrays() among them
//   3. bounce < 0, N < 0, N too large for a launch    6. host.geometry; then an empty list: BSDFD_OK
template <class H>
int launch_sample_emitter(const H& host, const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                          uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                          const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit, void* stream, const Rows* list) {
    using G = typename H::Geom;
    if (int rc = host.admit(nullptr, nullptr)) return rc;
    Scene sc;
    Lights lt;
    if (int rc = to_scene(scene, 0, 0, 1, sc)) return rc;
    if (int rc = to_lights(lights, lt)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "negative path count");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "wavefront too large for one launch");
    if (N == 0 || (H::EMPTY_LIST_FIRST && list && list->n == 0)) return BSDFD_OK;
    if (!org || !nrm || !wi || !material || !wl || !lsel || !emit || !host.arrays()) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    G g{};
    if (int rc = host.geometry(sc, g)) return rc;
    if (list && list->n == 0) return BSDFD_OK;
    const Step st = make_step(bounce, 0, occlusion, seed, pass, path_offset, N);
    const long long* mat = reinterpret_cast<const long long*>(material);
    int* sel = reinterpret_cast<int*>(lsel);
    return list ? launch_lanes(list->n, sample_emitter_kernel<true, G>, stream, sc, g, lt, st, org, nrm, wi, mat, wl, sel, emit, *list)
                : launch_lanes(N, sample_emitter_kernel<false, G>, stream, sc, g, lt, st, org, nrm, wi, mat, wl, sel, emit, Rows{});
}

// One bounce in `mode`, with Russian roulette from rr_depth on (0: none), over all N lanes or (`list`, which to_rows has checked
// against N) over the lanes of a list.  `transmit`: the transmitting kernels, which need the ground truth (f_o) and have roulette
// only — their "no roulette" is rr_depth = INT_MAX, one wave-uniform comparison per lane.  A mode ignores the emitter arguments
// it does not have:
//   COSINE : none
//   LIT    : lights, lsel, emit
//   ENV    : dist, emit, lpdf; `lights` and `lsel` both NULL (n_e = 1) or both given (has_env set, n_e = n_lights + 1)
// The checks, in the order a caller sees them fail (an entry point's own — rr_depth, to_rows — come before all of them on the
// spheres, and between the null scene and 1. on the meshes):
//   1. host.admit, then rr_depth < 0
//   2. the mode's scene and emitters, by the lane count (N; EMPTY_LIST_FIRST: 0 for an empty list)
//        ENV  : the light count, has_env, lights / lsel pairing (N != 0), then env_scene
//        else : path_scene, then (LIT) light_counts
//   3. bounce < 0, then f_o / f_l pairing
//   4. a lane count of 0: BSDFD_OK
//   5. null pointers: the state, the sampler's answers, the mode's emitter arrays, host.arrays()
//   6. host.geometry
//   7. transmit without f_o; then an empty list: BSDFD_OK
template <class H>
int launch_bounce(const H& host, Mode mode, int rr_depth, const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last,
                  int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                  float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o, const float* pdf_l,
                  const float* f_o, const float* f_l, const bsdfd_wf_lights* lights, const int32_t* lsel, const float* emit,
                  const float* lpdf, const bsdfd_env_dist* dist, void* stream, const Rows* list = nullptr, bool transmit = false) {
    using G = typename H::Geom;
    if (int rc = host.admit(lpdf, dist)) return rc;
    if (rr_depth < 0) return bsdfd_fail_(BSDFD_EINVAL, "rr_depth must be >= 0 (0: no Russian roulette)");
    const int64_t count = H::EMPTY_LIST_FIRST && list && list->n == 0 ? 0 : N;
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
        if (int rc = env_scene(scene, env, dist, n_e, lights != nullptr, count, sc, e)) return rc;
        emitter_arrays = emit && lpdf;
    } else {
        if (int rc = path_scene(scene, env, count, sc)) return rc;
        if (mode == LIT) {
            if (int rc = light_counts(lights, n, n_e)) return rc;
            emitter_arrays = lsel && emit;
        }
    }
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if ((f_o == nullptr) != (f_l == nullptr)) return bsdfd_fail_(BSDFD_EINVAL, "f_o and f_l are both NULL or both given");
    if (count == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !wl || !material || !beta || !rad || !wo || !pdf_o || !pdf_l || !emitter_arrays || !host.arrays())
        return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    G g{};
    if (int rc = host.geometry(sc, g)) return rc;
    if (transmit && !f_o) return bsdfd_fail_(BSDFD_EINVAL, "transmission needs the ground truth: null f_o");
    if (list && list->n == 0) return BSDFD_OK;
    const Step st = make_step(bounce, last, occlusion, seed, pass, path_offset, N);
    const PathState ps{org, nrm, wi, wl, reinterpret_cast<long long*>(material), beta, rad};
    const SamplerAnswer sa{wo, pdf_o, pdf_l, f_o, f_l};
    const EmitterSample es{reinterpret_cast<const int*>(lsel), mode == ENV ? lpdf : nullptr, emit};
    // (mode, rr, list, transmit) -> the instantiation.  has_env = n_e - n is LIT's; the kernel folds it away elsewhere.
    const int rr = transmit && !rr_depth ? INT_MAX : rr_depth;
    auto launch = [&](auto kernel) {
        return launch_lanes(list ? list->n : (long long)N, kernel, stream, sc, g, env, e, n_e, n_e - n, st, ps, sa, es, rr,
                            list ? *list : Rows{});
    };
    auto in_mode = [&](auto m) {
        constexpr int M = decltype(m)::value;
        if constexpr (!G::ONE_WALK) {   // (bounce_vertex's static_assert: no transmission where a hit is a walk, yet)
            if (transmit) return list ? launch(bounce_kernel<M, true, true, true, G>) : launch(bounce_kernel<M, true, false, true, G>);
        }
        if (list) return rr ? launch(bounce_kernel<M, true, true, false, G>) : launch(bounce_kernel<M, false, true, false, G>);
        return rr ? launch(bounce_kernel<M, true, false, false, G>) : launch(bounce_kernel<M, false, false, false, G>);
    };
    switch (mode) {
        case COSINE: return in_mode(std::integral_constant<int, COSINE>{});
        case LIT: return in_mode(std::integral_constant<int, LIT>{});
        default:
            if constexpr (!G::ONE_WALK) return in_mode(std::integral_constant<int, ENV>{});   // (the same static_assert: nor ENV)
            else return bsdfd_fail_(BSDFD_EINVAL, "no ENV mode with this geometry");
    }
}

}  // namespace bounce_dev
