// mesh.hip — ray casting on instanced triangle meshes: the geometry of the reference's array scenes (matpreview.serialized: a
// plane, an interior and a shell, instanced 25 times) in place of the analytic spheres of wavefront.hip.
//
//   host    : bsdfd_mesh_bvh_build — a median-split binary BVH in depth-first order with skip links (a "threaded" BVH; no HIP
//             call, so C callers and the CPU suite can build and inspect one); bsdfd_mesh_scene_create — meshes uploaded once
//             with their BVH, instances with the fp64 inverse of their to_world and a padded world box
//   kernels : intersect (closest hit), occluded (any hit), primary (bsdfd_wf_primary's rays, closest hit, the five arrays
//             shade_kernel reads; its path form also stores the hit, and path_begin makes the first vertex of a path from it) — one ray per lane, the walk of
//             mesh_dev.h; no stack, no scratch
//             bounce, sample_emitter — the path tracer's one bounce and its point emitters' sample: bounce_launch.h's kernel
//             templates and launchers with mesh_dev::PathGeom as their geometry and MeshHost below as its host side.  COSINE
//             and LIT, with and without roulette, full width and over a live-lane list.  No ENV mode and no transmission on
//             meshes yet.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bounce_dev.h"
#include "bounce_launch.h"
#include "bsdfd.h"
#include "common.h"
#include "mesh_dev.h"
#include "wavefront_dev.h"

struct bsdfd_mesh_scene_ctx {
    int device = 0;
    int n_inst = 0;
    int max_material = -1;
    mesh_dev::Inst* d_inst = nullptr;
    std::vector<void*> allocs;
};

namespace {

using namespace bounce_dev;   // (and wf_dev, which it opens)
using mesh_dev::Inst;
using mesh_dev::MeshHit;

static_assert(sizeof(bsdfd_mesh_node) == 32, "a node is 32 bytes");

// ---- the builder ----
struct Builder {
    const float* pos;
    const uint32_t* idx;
    std::vector<float> cen;   // triangle centroids
    int32_t* order;
    bsdfd_mesh_node* nodes;
    int64_t cap, n = 0;
    bool overflow = false;

    void build(int64_t lo, int64_t hi) {
        if (n >= cap) { overflow = true; return; }
        bsdfd_mesh_node& me = nodes[n++];
        float clo[3], chi[3];
        for (int a = 0; a < 3; ++a) { me.lo[a] = clo[a] = INFINITY; me.hi[a] = chi[a] = -INFINITY; }
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t f = order[s];
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) {
                    const float v = pos[3 * (int64_t)idx[3 * f + k] + a];
                    me.lo[a] = std::min(me.lo[a], v); me.hi[a] = std::max(me.hi[a], v);
                }
            for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], cen[3 * f + a]); chi[a] = std::max(chi[a], cen[3 * f + a]); }
        }
        const int64_t count = hi - lo;
        if (count <= 4) {
            me.tris = (int32_t)(lo * 8 + count);
            me.skip = (int32_t)n;
            return;
        }
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
        const int64_t mid = lo + count / 2;   // the median: both halves are non-empty even where every centroid coincides
        std::nth_element(order + lo, order + mid, order + hi, [&](int32_t x, int32_t y) {
            const float cx = cen[3 * (int64_t)x + axis], cy = cen[3 * (int64_t)y + axis];
            return cx < cy || (cx == cy && x < y);
        });
        me.tris = 0;
        build(lo, mid);
        build(mid, hi);
        me.skip = (int32_t)n;   // (`me` stays valid: nodes_out is the caller's array, never reallocated)
    }
};

int check_mesh(const float* positions, int64_t nv, const uint32_t* indices, int64_t nt) {
    if (!positions || !indices) return bsdfd_fail_(BSDFD_EINVAL, "null mesh array");
    if (nv < 1 || nv > 0xffffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "a mesh needs 1 .. 2^32 - 1 vertices");
    if (nt < 1 || nt > (1LL << 27)) return bsdfd_fail_(BSDFD_EINVAL, "a mesh needs 1 .. 2^27 triangles");
    for (int64_t i = 0; i < 3 * nv; ++i)
        if (!std::isfinite(positions[i])) return bsdfd_fail_(BSDFD_EINVAL, "non-finite vertex " + std::to_string(i / 3));
    for (int64_t i = 0; i < 3 * nt; ++i)
        if ((int64_t)indices[i] >= nv)
            return bsdfd_fail_(BSDFD_EINVAL, "triangle " + std::to_string(i / 3) + " has a vertex index out of range");
    return BSDFD_OK;
}

int build_bvh(const float* positions, const uint32_t* indices, int64_t nt, bsdfd_mesh_node* nodes_out, int64_t node_cap,
              int32_t* order_out, int64_t* n_nodes) {
    Builder b;
    b.pos = positions; b.idx = indices; b.order = order_out; b.nodes = nodes_out; b.cap = node_cap;
    b.cen.resize(3 * (size_t)nt);
    for (int64_t f = 0; f < nt; ++f) {
        order_out[f] = (int32_t)f;
        for (int a = 0; a < 3; ++a)
            b.cen[3 * f + a] = (positions[3 * (int64_t)indices[3 * f] + a] + positions[3 * (int64_t)indices[3 * f + 1] + a] +
                                positions[3 * (int64_t)indices[3 * f + 2] + a]) * (1.0f / 3.0f);
    }
    b.build(0, nt);
    if (b.overflow) return bsdfd_fail_(BSDFD_EINVAL, "node_cap too small: 2 * nt - 1 nodes always suffice");
    *n_nodes = b.n;
    return BSDFD_OK;
}

// ---- kernels ----
__global__ __launch_bounds__(256) void intersect_kernel(const Inst* __restrict__ insts, int n_inst, long long n,
                                                        const float* __restrict__ org, const float* __restrict__ dir,
                                                        const float* __restrict__ tmax, const int* __restrict__ skip,
                                                        float* __restrict__ t, int* __restrict__ prim, float* __restrict__ bary) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const MeshHit h = mesh_dev::walk<false>(insts, n_inst, ld3(org + 3 * p), ld3(dir + 3 * p), tmax ? tmax[p] : mesh_dev::NOTHING,
                                            skip ? skip[2 * p] : -1, skip ? skip[2 * p + 1] : -1);
    t[p] = h.t;
    prim[2 * p] = h.inst; prim[2 * p + 1] = h.tri;
    bary[2 * p] = h.b1; bary[2 * p + 1] = h.b2;
    MESH_COUNT(bary[2 * p] = (float)h.nodes; bary[2 * p + 1] = (float)h.tris;)   // (the counting build reports them here)
}

__global__ __launch_bounds__(256) void occluded_kernel(const Inst* __restrict__ insts, int n_inst, long long n,
                                                       const float* __restrict__ org, const float* __restrict__ dir,
                                                       const float* __restrict__ tmax, const int* __restrict__ skip,
                                                       unsigned char* __restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const MeshHit h = mesh_dev::walk<true>(insts, n_inst, ld3(org + 3 * p), ld3(dir + 3 * p), tmax ? tmax[p] : mesh_dev::NOTHING,
                                           skip ? skip[2 * p] : -1, skip ? skip[2 * p + 1] : -1);
    out[p] = h.inst >= 0 ? 1 : 0;
}

// primary_kernel of wavefront.hip on the mesh scene: its path index, Philox words, film position, ray and light sample, statement
// for statement (dir and wl are its bits), then the closest hit among the instances.  With `prim` (the path form; wave-uniform)
// the hit itself is stored as well — prim = (instance, triangle) and t in the first slot of the lane's `hit_t` row (the path's org
// array, which mesh_path_begin_kernel reads and overwrites).  Stores only: the compiler fuses the ray and vertex arithmetic by the
// code around it, so the path form adds none here — dir and wl stay bsdfd_wf_primary's bits and wi, nrm the plain form's.
__global__ __launch_bounds__(256) void mesh_primary_kernel(Scene sc, const Inst* __restrict__ insts, int n_inst, int row_begin,
                                                           int row_end, int spp, unsigned long long seed, unsigned long long pass,
                                                           float* __restrict__ wi, float* __restrict__ wl, float* __restrict__ nrm,
                                                           float* __restrict__ dir, long long* __restrict__ mat,
                                                           float* __restrict__ hit_t, int* __restrict__ prim) {
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
    const float jx = (float)(u[0] >> 8) * (1.0f / 16777216.0f), jy = (float)(u[1] >> 8) * (1.0f / 16777216.0f);
    const float fx = ((float)col + jx) / (float)sc.width, fy = ((float)row + jy) / (float)sc.height;
    const float sx = (2.0f * fx - 1.0f) * sc.tan_half_fov;
    const float sy = (1.0f - 2.0f * fy) * sc.tan_half_fov * ((float)sc.height / (float)sc.width);
    V3 d = sc.fwd + sx * sc.right + sy * sc.up;
    d = (1.0f / sqrtf(dot(d, d))) * d;
    const MeshHit h = mesh_dev::walk<false>(insts, n_inst, sc.o, d, mesh_dev::NOTHING, -1, -1);
    V3 nn = v3(0.f, 0.f, 0.f), w_in = v3(0.f, 0.f, 1.f);
    long long material = sc.n_sph + 1;  // miss
    if (h.inst >= 0) mesh_dev::surface_vertex(insts, h, d, sc.n_sph, nn, w_in, material);
    const V3 w_l = cosine_sample(u[2], u[3]);
    st3(wi + 3 * p, w_in);
    st3(wl + 3 * p, w_l);
    st3(nrm + 3 * p, nn);
    st3(dir + 3 * p, d);
    if (mat) mat[p] = material;
    if (prim) {
        hit_t[3 * p] = h.t;
        prim[2 * p] = h.inst; prim[2 * p + 1] = h.tri;
    }
}

// path_begin_kernel of pathtrace.hip behind the kernel above: what it derives from dir, nrm and the id on the spheres comes from
// the stored hit here — org = cam + t dir for a hit; org = 0 and rad = the environment along dir for a miss; beta = 1, rad = 0 on a hit.
__global__ __launch_bounds__(256) void mesh_path_begin_kernel(Scene sc, const float* __restrict__ env, long long n,
                                                              const float* __restrict__ dir, const int* __restrict__ prim,
                                                              float* __restrict__ org, float* __restrict__ beta,
                                                              float* __restrict__ rad) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const V3 d = ld3(dir + 3 * p);
    V3 o = v3(0.f, 0.f, 0.f);
    float L[3] = {0.f, 0.f, 0.f};
    if (prim[2 * p] >= 0) o = sc.o + org[3 * p] * d;
    else env_lookup(env, sc.env_w, sc.env_h, d, L);   // the camera sees the environment
    st3(org + 3 * p, o);
    st3(beta + 3 * p, v3(1.f, 1.f, 1.f));
    st3(rad + 3 * p, v3(L[0], L[1], L[2]));
}

// ---- host side of the scene ----
template <class T>
int upload(bsdfd_mesh_scene_ctx* ctx, const T* host, size_t count, const T** dev) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, count * sizeof(T)));
    ctx->allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T*>(d);
    return BSDFD_OK;
}

struct DevMesh {
    const float4 *nodes, *tri;
    const int* order;
    const float *pos, *nrm, *uv;
    const unsigned* idx;
    int n_nodes;
    float lo[3], hi[3];
};

int upload_mesh(bsdfd_mesh_scene_ctx* ctx, const bsdfd_mesh_desc& m, DevMesh& dm) {
    if (int rc = check_mesh(m.positions, m.n_vertices, m.indices, m.n_triangles)) return rc;
    const int64_t nt = m.n_triangles, nv = m.n_vertices;
    std::vector<bsdfd_mesh_node> nodes(2 * (size_t)nt);
    std::vector<int32_t> order((size_t)nt);
    int64_t n_nodes = 0;
    if (int rc = build_bvh(m.positions, m.indices, nt, nodes.data(), (int64_t)nodes.size(), order.data(), &n_nodes)) return rc;
    std::vector<float4> tri(3 * (size_t)nt);
    for (int64_t s = 0; s < nt; ++s)
        for (int k = 0; k < 3; ++k) {
            const float* v = m.positions + 3 * (int64_t)m.indices[3 * (int64_t)order[s] + k];
            tri[3 * s + k] = make_float4(v[0], v[1], v[2], 0.0f);
        }
    dm.n_nodes = (int)n_nodes;
    for (int a = 0; a < 3; ++a) { dm.lo[a] = nodes[0].lo[a]; dm.hi[a] = nodes[0].hi[a]; }
    if (int rc = upload(ctx, reinterpret_cast<const float4*>(nodes.data()), 2 * (size_t)n_nodes, &dm.nodes)) return rc;
    if (int rc = upload(ctx, tri.data(), tri.size(), &dm.tri)) return rc;
    if (int rc = upload(ctx, order.data(), order.size(), &dm.order)) return rc;
    if (int rc = upload(ctx, m.positions, 3 * (size_t)nv, &dm.pos)) return rc;
    if (int rc = upload(ctx, reinterpret_cast<const unsigned*>(m.indices), 3 * (size_t)nt, &dm.idx)) return rc;
    dm.nrm = dm.uv = nullptr;
    if (m.normals)
        if (int rc = upload(ctx, m.normals, 3 * (size_t)nv, &dm.nrm)) return rc;
    if (m.uvs)
        if (int rc = upload(ctx, m.uvs, 2 * (size_t)nv, &dm.uv)) return rc;
    return BSDFD_OK;
}

// world -> object in fp64, and the world box of the mesh box's corners, padded: the kernels move the ray into object space in
// fp32, so a hit may lie a rounding error outside the exact box
int make_instance(const bsdfd_mesh_instance& s, const DevMesh& dm, Inst& in) {
    const float* m = s.to_world;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(m[k])) return bsdfd_fail_(BSDFD_EINVAL, "non-finite to_world");
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    double scale = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) scale = std::max(scale, std::fabs((double)m[4 * r + q]));
    if (!(std::fabs(det) > 1e-12 * scale * scale * scale) || !std::isfinite(det))
        return bsdfd_fail_(BSDFD_EINVAL, "singular to_world");
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                           (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                           (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) in.inv[4 * r + q] = (float)inv[3 * r + q];
        in.inv[4 * r + 3] = (float)-(inv[3 * r] * m[3] + inv[3 * r + 1] * m[7] + inv[3 * r + 2] * m[11]);
    }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int corner = 0; corner < 8; ++corner) {
        const double x = corner & 1 ? dm.hi[0] : dm.lo[0], y = corner & 2 ? dm.hi[1] : dm.lo[1], z = corner & 4 ? dm.hi[2] : dm.lo[2];
        for (int r = 0; r < 3; ++r) {
            const double w = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3];
            lo[r] = std::min(lo[r], w); hi[r] = std::max(hi[r], w);
        }
    }
    double ext = 0.0, mag = 0.0;
    for (int r = 0; r < 3; ++r) {
        ext = std::max(ext, hi[r] - lo[r]);
        mag = std::max(mag, std::max(std::fabs(lo[r]), std::fabs(hi[r])));
    }
    const double pad = 1e-4 * ext + 1e-6 * mag;
    for (int r = 0; r < 3; ++r) { in.lo[r] = (float)(lo[r] - pad); in.hi[r] = (float)(hi[r] + pad); }
    in.nodes = dm.nodes; in.tri = dm.tri; in.order = dm.order; in.pos = dm.pos; in.idx = dm.idx; in.nrm = dm.nrm; in.uv = dm.uv;
    in.n_nodes = dm.n_nodes;
    in.surface = s.surface; in.material = s.material;
    in.c0 = s.color0; in.c1 = s.color1; in.uscale = s.uscale; in.vscale = s.vscale;
    return BSDFD_OK;
}

// the checks the launchers share, N known to be >= 0
int check_scene(bsdfd_mesh_scene scene) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != scene->device) return bsdfd_fail_(BSDFD_EINVAL, "the mesh scene lives on another device");
    return BSDFD_OK;
}

int check_materials(bsdfd_mesh_scene scene, const Scene& sc) {
    if (scene->max_material >= sc.n_sph)
        return bsdfd_fail_(BSDFD_EINVAL, "an instance's material index is not below n_materials = 1 + n_extra_spheres");
    return BSDFD_OK;
}

// both forms of the primary rays: `path` carries env, org, prim, beta and rad, and launches mesh_path_begin_kernel behind the walk
int launch_primary(bool path, bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, int32_t row_begin, int32_t row_end, int32_t spp,
                   uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material, const float* env,
                   float* org, int32_t* prim, float* beta, float* rad, void* stream) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    Scene sc;
    if (int rc = to_scene(wf_scene, row_begin, row_end, spp, sc)) return rc;
    if (path && (sc.env_w <= 0 || sc.env_h <= 0)) return bsdfd_fail_(BSDFD_EINVAL, "environment map size must be positive");
    if (int rc = check_materials(scene, sc)) return rc;
    const long long n = (long long)(row_end - row_begin) * sc.width * spp;
    if (n == 0) return BSDFD_OK;
    if (!wi || !wl || !nrm || !dir || (path && (!org || !prim || !beta || !rad))) return bsdfd_fail_(BSDFD_EINVAL, "null output pointer");
    if (path && !env) return bsdfd_fail_(BSDFD_EINVAL, "null environment map");
    if ((n + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "tile too large for one launch");
    if (int rc = check_scene(scene)) return rc;
    if (int rc = launch_lanes(n, mesh_primary_kernel, stream, sc, (const Inst*)scene->d_inst, scene->n_inst, row_begin, row_end, spp,
                              (unsigned long long)seed, (unsigned long long)pass, wi, wl, nrm, dir,
                              reinterpret_cast<long long*>(material), org, reinterpret_cast<int*>(prim)))
        return rc;
    if (!path) return BSDFD_OK;
    return launch_lanes(n, mesh_path_begin_kernel, stream, sc, env, n, (const float*)dir, (const int*)reinterpret_cast<int*>(prim), org,
                        beta, rad);
}

// The mesh scene as the host side of the path launchers' geometry (bounce_launch.h; SpheresHost is its sibling).  prim is the
// policy's own array; the emitter sample reads it and never writes it.  A list's grid covers the list, so a wave's walks are
// shared by 64 listed lanes instead of by whatever is left alive among 64 neighbours: fewer waves walk while more than ~5 % of the
// lanes live, but a short list packs 64 unrelated rays into a wave that lasts as long as the longest of them in every instance,
// where the full-width launch runs them one to a wave (measured: profiles/mesh_path_compact.json).
struct MeshHost {
    using Geom = mesh_dev::PathGeom;
    static constexpr bool EMPTY_LIST_FIRST = true;
    bsdfd_mesh_scene scene;
    int32_t* prim;
    int admit(const float* lpdf, const bsdfd_env_dist* dist) const {
        if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
        if (lpdf || dist)
            return bsdfd_fail_(BSDFD_EINVAL, "importance sampling of the environment is not on meshes yet: lpdf and dist must be NULL");
        return BSDFD_OK;
    }
    bool arrays() const { return prim != nullptr; }
    int geometry(const Scene& sc, Geom& g) const {
        if (int rc = check_materials(scene, sc)) return rc;
        if (int rc = check_scene(scene)) return rc;
        g = Geom{scene->d_inst, scene->n_inst, reinterpret_cast<int*>(prim)};
        return BSDFD_OK;
    }
};

}  // namespace

extern "C" {

int bsdfd_mesh_bvh_build(const float* positions, int64_t nv, const uint32_t* indices, int64_t nt, bsdfd_mesh_node* nodes_out,
                         int64_t node_cap, int32_t* order_out, int64_t* n_nodes) {
    if (!nodes_out || !order_out || !n_nodes) return bsdfd_fail_(BSDFD_EINVAL, "null output pointer");
    if (int rc = check_mesh(positions, nv, indices, nt)) return rc;
    if (node_cap < 1) return bsdfd_fail_(BSDFD_EINVAL, "node_cap too small: 2 * nt - 1 nodes always suffice");
    return build_bvh(positions, indices, nt, nodes_out, node_cap, order_out, n_nodes);
}

int bsdfd_mesh_scene_create(const bsdfd_mesh_desc* meshes, int32_t n_meshes, const bsdfd_mesh_instance* instances,
                            int32_t n_instances, bsdfd_mesh_scene* scene) {
    if (!meshes || !instances || !scene) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    *scene = nullptr;
    if (n_meshes < 1) return bsdfd_fail_(BSDFD_EINVAL, "a mesh scene needs at least one mesh");
    if (n_instances < 1 || n_instances > BSDFD_MESH_MAX_INSTANCES)
        return bsdfd_fail_(BSDFD_EINVAL, "a mesh scene has 1 .. 64 instances");
    for (int k = 0; k < n_instances; ++k) {   // everything that needs no device first
        const bsdfd_mesh_instance& s = instances[k];
        if (s.mesh < 0 || s.mesh >= n_meshes) return bsdfd_fail_(BSDFD_EINVAL, "instance " + std::to_string(k) + ": mesh index out of range");
        if (s.surface != BSDFD_MESH_MATERIAL && s.surface != BSDFD_MESH_DIFFUSE && s.surface != BSDFD_MESH_CHECKER)
            return bsdfd_fail_(BSDFD_EINVAL, "instance " + std::to_string(k) + ": unknown surface kind");
        if (s.surface == BSDFD_MESH_MATERIAL && s.material < 0)
            return bsdfd_fail_(BSDFD_EINVAL, "instance " + std::to_string(k) + ": negative material index");
        if (s.surface == BSDFD_MESH_CHECKER && !meshes[s.mesh].uvs)
            return bsdfd_fail_(BSDFD_EINVAL, "instance " + std::to_string(k) + ": a checkerboard needs a mesh with uv");
    }
    bsdfd_mesh_scene_ctx* ctx = new bsdfd_mesh_scene_ctx;
    auto fail = [&](int rc) { bsdfd_mesh_scene_destroy(ctx); return rc; };
    if (hipGetDevice(&ctx->device) != hipSuccess) return fail(bsdfd_fail_(BSDFD_EHIP, "hipGetDevice failed"));
    std::vector<DevMesh> dms((size_t)n_meshes);
    for (int k = 0; k < n_meshes; ++k)
        if (int rc = upload_mesh(ctx, meshes[k], dms[k])) return fail(rc);
    std::vector<Inst> insts((size_t)n_instances);
    for (int k = 0; k < n_instances; ++k) {
        if (int rc = make_instance(instances[k], dms[instances[k].mesh], insts[k])) return fail(rc);
        if (instances[k].surface == BSDFD_MESH_MATERIAL) ctx->max_material = std::max(ctx->max_material, instances[k].material);
    }
    const Inst* d = nullptr;
    if (int rc = upload(ctx, insts.data(), insts.size(), &d)) return fail(rc);
    ctx->d_inst = const_cast<Inst*>(d);
    ctx->n_inst = n_instances;
    *scene = ctx;
    return BSDFD_OK;
}

void bsdfd_mesh_scene_destroy(bsdfd_mesh_scene scene) {
    if (!scene) return;
    for (void* p : scene->allocs) (void)hipFree(p);
    delete scene;
}

int bsdfd_mesh_intersect(bsdfd_mesh_scene scene, int64_t N, const float* org, const float* dir, const float* tmax,
                         const int32_t* skip, float* t, int32_t* prim, float* bary, void* stream) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (N == 0) return BSDFD_OK;
    if (!org || !dir || !t || !prim || !bary) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "wavefront too large for one launch");
    if (int rc = check_scene(scene)) return rc;
    return launch_lanes(N, intersect_kernel, stream, scene->d_inst, scene->n_inst, (long long)N, org, dir, tmax, skip, t, prim, bary);
}

int bsdfd_mesh_occluded(bsdfd_mesh_scene scene, int64_t N, const float* org, const float* dir, const float* tmax,
                        const int32_t* skip, uint8_t* out, void* stream) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    if (N < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (N == 0) return BSDFD_OK;
    if (!org || !dir || !out) return bsdfd_fail_(BSDFD_EINVAL, "null pointer");
    if ((N + 255) / 256 > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "wavefront too large for one launch");
    if (int rc = check_scene(scene)) return rc;
    return launch_lanes(N, occluded_kernel, stream, scene->d_inst, scene->n_inst, (long long)N, org, dir, tmax, skip, out);
}

int bsdfd_mesh_primary(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, int32_t row_begin, int32_t row_end, int32_t spp,
                       uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material,
                       void* stream) {
    return launch_primary(false, scene, wf_scene, row_begin, row_end, spp, seed, pass, wi, wl, nrm, dir, material, nullptr, nullptr,
                          nullptr, nullptr, nullptr, stream);
}

int bsdfd_mesh_path_primary(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, int32_t row_begin, int32_t row_end, int32_t spp,
                            uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material,
                            const float* env, float* org, int32_t* prim, float* beta, float* rad, void* stream) {
    return launch_primary(true, scene, wf_scene, row_begin, row_end, spp, seed, pass, wi, wl, nrm, dir, material, env, org, prim, beta,
                          rad, stream);
}

int bsdfd_mesh_sample_emitter(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const bsdfd_wf_lights* lights, int32_t bounce,
                              int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                              const float* nrm, const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit,
                              const int32_t* prim, void* stream) {
    return launch_sample_emitter(MeshHost{scene, const_cast<int32_t*>(prim)}, wf_scene, lights, bounce, occlusion, seed, pass, path_offset,
                                 N, org, nrm, wi, material, wl, lsel, emit, stream, nullptr);
}

int bsdfd_mesh_bounce(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const float* env, int32_t bounce, int32_t last,
                      int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm,
                      float* wi, float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                      const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights, const int32_t* lsel,
                      const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth, int32_t* prim,
                      void* stream) {
    return launch_bounce(MeshHost{scene, prim}, lights ? LIT : COSINE, (int)rr_depth, wf_scene, env, bounce, last, occlusion, seed, pass,
                         path_offset, N, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist,
                         stream);
}

int bsdfd_mesh_sample_emitter_rows(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const bsdfd_wf_lights* lights,
                                   int32_t bounce, int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N,
                                   const float* org, const float* nrm, const float* wi, const int64_t* material, float* wl,
                                   int32_t* lsel, float* emit, const int32_t* prim, const int64_t* rows, int64_t n_rows,
                                   void* stream) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    Rows list;
    if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_sample_emitter(MeshHost{scene, const_cast<int32_t*>(prim)}, wf_scene, lights, bounce, occlusion, seed, pass, path_offset,
                                 N, org, nrm, wi, material, wl, lsel, emit, stream, &list);
}

int bsdfd_mesh_bounce_rows(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const float* env, int32_t bounce, int32_t last,
                           int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm,
                           float* wi, float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                           const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                           const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                           int32_t* prim, const int64_t* rows, int64_t n_rows, void* stream) {
    if (!scene) return bsdfd_fail_(BSDFD_EINVAL, "null mesh scene");
    Rows list;
    if (int rc = to_rows(rows, n_rows, N, list)) return rc;
    return launch_bounce(MeshHost{scene, prim}, lights ? LIT : COSINE, (int)rr_depth, wf_scene, env, bounce, last, occlusion, seed, pass,
                         path_offset, N, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l, lights, lsel, emit, lpdf, dist,
                         stream, &list);
}

}  // extern "C"
