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
//
// The bounce that reads lpdf and emit is bounce.hip's ENV kernel.  bsdfd_wf_sample_env_rows is the same kernel over the lanes of a
// live-lane list (bounce_dev.h's Rows).
// One path per lane; the scene travels by value; a lane whose path has ended returns after reading its id.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bounce_dev.h"
#include "bsdfd.h"
#include "common.h"

namespace {

using namespace bounce_dev;

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

// LIST: the lanes of `rows` (the list form) instead of every lane of the wavefront
template <bool LIST>
__global__ __launch_bounds__(256) void sample_env_kernel(Scene sc, const float* __restrict__ env, EnvDist e, int n_e, Step st,
                                                         const float* __restrict__ org, const float* __restrict__ nrm,
                                                         const float* __restrict__ wi, const long long* __restrict__ mat,
                                                         const int* __restrict__ lsel, float* __restrict__ wl,
                                                         float* __restrict__ lpdf, float* __restrict__ emit, Rows rows) {
    long long p, m;
    if (!live_lane<LIST>(sc, st.n, mat, p, m, rows)) return;
    if (lsel && lsel[p] != -1) return;   // a point light was picked: sample_emitter's wl and emit stand
    unsigned u[4];
    tagged_draw(st.seed, st.pass, st.path_offset, p, 0x456E766Du /* "Envm" */, st.bounce, u);
    V3 d;
    int j, i;
    const float p_l = env_dev::env_sample(e, (float)(u[0] >> 8) * (1.0f / 16777216.0f), (float)(u[1] >> 8) * (1.0f / 16777216.0f),
                                          d, j, i) / (float)n_e;
    const V3 nn = ld3(nrm + 3 * p), x = ld3(org + 3 * p);
    float cosl;
    const bool lit = emitter_arrives(sc, x, nn, d, m, st.occlusion, 3.0e38f, p_l > 0.0f, cosl);   // (3e38: any hit is in the way)
    float s = 0.0f;
    float E[3] = {0.f, 0.f, 0.f};
    if (lit) {
        env_lookup(env, sc.env_w, sc.env_h, d, E);
        s = 1.0f / p_l;
    }
    if (m == sc.n_sph) {
        // diffuse floor: f cos = (reflectance / pi) cos, weighted against the cosine strategy the bounce runs along wl
        const float inv_pi = 0.31830988618379067154f;
        s *= mis_power(p_l, cosl * inv_pi) * wi[3 * p] * inv_pi * cosl;
    } else {
        store_local_direction(wl + 3 * p, nn, d, cosl);
    }
    lpdf[p] = p_l;
    st3(emit + 3 * p, v3(s * E[0], s * E[1], s * E[2]));
}

// the checks of both sample_env entry points and the launch: over all N lanes, or (`list`) over the lanes of a list
int launch_sample_env(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int32_t n_e, int32_t bounce,
                      int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                      const float* nrm, const float* wi, const int64_t* material, const int32_t* lsel, float* wl, float* lpdf,
                      float* emit, void* stream, const Rows* list) {
    Scene sc;
    EnvDist e;
    if (int rc = env_scene(scene, env, dist, n_e, lsel != nullptr, N, sc, e)) return rc;
    if (bounce < 0) return bsdfd_fail_(BSDFD_EINVAL, "bounce must be >= 0");
    if (N == 0) return BSDFD_OK;
    if (!org || !nrm || !wi || !material || !wl || !lpdf || !emit) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    const Step st = make_step(bounce, 0, occlusion, seed, pass, path_offset, N);
    if (list && list->n == 0) return BSDFD_OK;
    const long long* mat = reinterpret_cast<const long long*>(material);
    const int* sel = reinterpret_cast<const int*>(lsel);
    return list ? launch_lanes(list->n, sample_env_kernel<true>, stream, sc, env, e, (int)n_e, st, org, nrm, wi, mat, sel, wl, lpdf, emit,
                               *list)
                : launch_lanes(N, sample_env_kernel<false>, stream, sc, env, e, (int)n_e, st, org, nrm, wi, mat, sel, wl, lpdf, emit,
                               Rows{});
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
    return launch_sample_env(scene, env, dist, n_e, bounce, occlusion, seed, pass, path_offset, N, org, nrm, wi, material, lsel, wl, lpdf,
                             emit, stream, nullptr);
}

int bsdfd_wf_sample_env_rows(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int32_t n_e, int32_t bounce,
                             int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                             const float* nrm, const float* wi, const int64_t* material, const int32_t* lsel, float* wl, float* lpdf,
                             float* emit, const int64_t* rows, int64_t n_rows, void* stream) {
    Rows list;
    if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_sample_env(scene, env, dist, n_e, bounce, occlusion, seed, pass, path_offset, N, org, nrm, wi, material, lsel, wl, lpdf,
                             emit, stream, &list);
}

}  // extern "C"
