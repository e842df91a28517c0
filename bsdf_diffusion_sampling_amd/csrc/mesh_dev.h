// mesh_dev.h — the ray caster over instanced triangle meshes (mesh.hip): the instance record, the conservative slab test, the
// watertight ray/triangle test and the stackless walk of a threaded BVH.  One ray per lane.  `walk<false>` is the closest hit,
// `walk<true>` leaves at the first accepted hit; both skip the primitive a ray starts on.  `surface_vertex` is the vertex at a hit,
// and `PathGeom` hands both to the path kernels (bounce_dev.h's bounce_vertex and sample_emitter_vertex, instantiated in mesh.hip)
// in the place of wf_dev::trace and continue_path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsdfd.h"
#include "wavefront_dev.h"

namespace mesh_dev {

using wf_dev::V3;
using wf_dev::v3;
using wf_dev::dot;

constexpr float NOTHING = 3.0e38f;   // wf_dev::Hit's "nothing"

// tools/mesh_bench.py compiles this unit once more with -DBSDFD_MESH_COUNT, into a library of its own: the walk then counts the
// nodes it loads and the triangles it tests.  Never the product.
#ifdef BSDFD_MESH_COUNT
#define MESH_COUNT(x) x
#else
#define MESH_COUNT(x)
#endif

// One instance as the kernels read it (device memory; the index is wave-uniform in the walk, so the record arrives through
// scalar loads).  `inv` is world -> object, row-major 3x4; its transpose also carries normals object -> world.
struct Inst {
    float inv[12];
    float lo[3], hi[3];                  // world-space box, padded on the host
    const float4* nodes;                 // bsdfd_mesh_node[n_nodes], two float4 each
    const float4* tri;                   // three float4 (xyz + pad) per triangle, in leaf order
    const int* order;                    // leaf slot -> the file's triangle index
    const float* pos;                    // [nv,3]
    const unsigned* idx;                 // [nt,3], file order
    const float* nrm;                    // [nv,3] or null
    const float* uv;                     // [nv,2] or null
    int n_nodes, surface, material;
    float c0, c1, uscale, vscale;        // diffuse: c0 (constant) or the checkerboard's two colours and scales
};

struct MeshHit {
    float t;        // world parameter; NOTHING = no hit
    int inst, tri;  // instance, the file's triangle index; -1 = no hit
    float b1, b2;   // weights of the triangle's second and third vertex
    MESH_COUNT(int nodes; int tris;)
};

// Ray against a box, conservatively: true unless the ray certainly misses it within [0, limit].  The triangle test below decides
// in fp32 on vertices sheared into ray space, whose coordinates carry a few ulp of their distance from the ray's origin: a ray
// that passes that close OUTSIDE a triangle's box may still be accepted by the triangle (and must be, where the neighbour across
// the shared edge has turned it down), so every face is moved outwards by 16 ulp of the box's farthest distance from the origin
// (Woop et al. pad their box test for the same reason).  The far side is padded by a few ulp of t as well, a NaN slab — a zero
// direction component with the origin exactly in a box plane, 0 * inf — is the whole line, and the final comparison is written
// so that an unordered result does not cull.
__device__ __forceinline__ void slab_axis(float a, float b, float pad, float inv_d, float& tn, float& tf) {
    const float t0 = (a - pad) * inv_d, t1 = (b + pad) * inv_d;
    const bool open = t0 != t0 || t1 != t1;
    tn = fmaxf(tn, open ? -INFINITY : fminf(t0, t1));
    tf = fminf(tf, open ? INFINITY : fmaxf(t0, t1));
}
__device__ __forceinline__ bool slab(V3 o, V3 inv_d, V3 lo, V3 hi, float limit) {
    const V3 a = lo - o, b = hi - o;
    const float far = fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(b.x)), fmaxf(fabsf(a.y), fabsf(b.y))), fmaxf(fabsf(a.z), fabsf(b.z)));
    const float pad = far * (16.0f / 16777216.0f);
    float tn = 0.0f, tf = limit;
    slab_axis(a.x, b.x, pad, inv_d.x, tn, tf);
    slab_axis(a.y, b.y, pad, inv_d.y, tn, tf);
    slab_axis(a.z, b.z, pad, inv_d.z, tn, tf);
    return !(tn > tf * 1.000001f);
}

// The ray-space of Woop, Benthin and Wald 2013: z is the dominant axis of the direction, x and y follow it cyclically and are
// swapped where the direction points down z, so that the winding is kept; the shear maps the direction onto +z.
struct RaySpace {
    int kz;
    bool swap;
    float sx, sy, sz;
};
__device__ __forceinline__ V3 permute(const RaySpace& rs, V3 v) {   // selects, never an index: an indexed V3 goes to scratch
    const V3 p = rs.kz == 0 ? v3(v.y, v.z, v.x) : rs.kz == 1 ? v3(v.z, v.x, v.y) : v;
    return rs.swap ? v3(p.y, p.x, p.z) : p;
}
__device__ __forceinline__ RaySpace ray_space(V3 d) {
    RaySpace rs;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    rs.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    rs.swap = false;
    const float dz = permute(rs, d).z;
    rs.swap = dz < 0.0f;
    const V3 p = permute(rs, d);
    rs.sz = 1.0f / p.z;
    rs.sx = p.x * rs.sz;
    rs.sy = p.y * rs.sz;
    return rs;
}

// Watertight ray/triangle test.  a, b, c are the vertices minus the ray origin.  The three edge functions are formed WITHOUT
// contraction: with a fused multiply-add Cx*By - Cy*Bx seen from the two triangles of a shared edge is no longer an exactly
// opposite pair, and rays slip between them.  (The pragma, not __fmul_rn / __fsub_rn: this toolchain's headers define those as
// plain x * y and x - y, which contract like any other.)  Accepts 0 < t <= limit with zeros of the edge functions inclusive.
__device__ __forceinline__ bool ray_triangle(const RaySpace& rs, V3 a, V3 b, V3 c, float limit, float& t, float& b1, float& b2) {
#pragma clang fp contract(off)
    const V3 A = permute(rs, a), B = permute(rs, b), C = permute(rs, c);
    const float Ax = fmaf(-rs.sx, A.z, A.x), Ay = fmaf(-rs.sy, A.z, A.y);
    const float Bx = fmaf(-rs.sx, B.z, B.x), By = fmaf(-rs.sy, B.z, B.y);
    const float Cx = fmaf(-rs.sx, C.z, C.x), Cy = fmaf(-rs.sy, C.z, C.y);
    const float cxby = Cx * By, cybx = Cy * Bx, axcy = Ax * Cy, aycx = Ay * Cx, bxay = Bx * Ay, byax = By * Ax;
    const float U = cxby - cybx;
    const float V = axcy - aycx;
    const float W = bxay - byax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = U + V + W;
    if (det == 0.0f) return false;                     // the ray lies in the triangle's plane (or the triangle is degenerate)
    const float T = U * (rs.sz * A.z) + V * (rs.sz * B.z) + W * (rs.sz * C.z);
    const float inv = 1.0f / det;
    t = T * inv;
    if (!(t > 0.0f && t <= limit)) return false;
    b1 = V * inv;
    b2 = W * inv;
    return true;
}

__device__ __forceinline__ V3 to_object_point(const float* m, V3 p) {
    return v3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
              m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
__device__ __forceinline__ V3 to_object_vector(const float* m, V3 d) {
    return v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z, m[8] * d.x + m[9] * d.y + m[10] * d.z);
}
__device__ __forceinline__ V3 normal_to_world(const float* m, V3 n) {   // the inverse transpose of to_world
    return v3(m[0] * n.x + m[4] * n.y + m[8] * n.z, m[1] * n.x + m[5] * n.y + m[9] * n.z, m[2] * n.x + m[6] * n.y + m[10] * n.z);
}

// The walk.  Top level: a wave-uniform loop over the instances, a slab test of the world ray against the instance's box, the
// ray moved into object space — the direction is NOT renormalised, so t stays the world parameter and compares across instances —
// and the stackless walk of that mesh's nodes: nodes lie in depth-first order, an inner node's left child is the next node and
// `skip` is the first node behind a subtree, so "descend" is i + 1 and "leave" is skip.  Boxes are culled against t <= best, never
// <, and a hit wins on a smaller t, on equal t on the smaller (instance, file triangle): the answer does not depend on node order.
template <bool ANY>
__device__ __forceinline__ MeshHit walk(const Inst* __restrict__ insts, int n_inst, V3 o, V3 d, float tmax, int skip_inst,
                                        int skip_tri) {
    MeshHit best;
    best.t = NOTHING; best.inst = -1; best.tri = -1; best.b1 = 0.0f; best.b2 = 0.0f;
    MESH_COUNT(best.nodes = 0; best.tris = 0;)
    const V3 inv_dw = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    for (int i = 0; i < n_inst; ++i) {
        const Inst& in = insts[i];
        if (ANY && best.inst >= 0) continue;
        const float top = ANY ? tmax : fminf(tmax, best.t);
        if (!slab(o, inv_dw, v3(in.lo[0], in.lo[1], in.lo[2]), v3(in.hi[0], in.hi[1], in.hi[2]), top)) continue;
        const V3 oo = to_object_point(in.inv, o), od = to_object_vector(in.inv, d);
        const V3 inv_d = v3(1.0f / od.x, 1.0f / od.y, 1.0f / od.z);
        const RaySpace rs = ray_space(od);
        const float4* __restrict__ nodes = in.nodes;
        const float4* __restrict__ tris = in.tri;
        const int n_nodes = in.n_nodes;
        int node = 0;
        while (node < n_nodes) {
            const float4 n0 = nodes[2 * node], n1 = nodes[2 * node + 1];
            const float limit = ANY ? tmax : fminf(tmax, best.t);
            MESH_COUNT(++best.nodes;)
            int next = __float_as_int(n1.z);                       // skip
            if (slab(oo, inv_d, v3(n0.x, n0.y, n0.z), v3(n0.w, n1.x, n1.y), limit)) {
                next = node + 1;                                   // an inner node's left child; a leaf's skip
                const int leaf = __float_as_int(n1.w);             // 0: inner node; else first * 8 + count
                const int first = leaf >> 3, count = leaf & 7;
                for (int k = 0; k < count; ++k) {
                    const float4 a = tris[3 * (first + k)], b = tris[3 * (first + k) + 1], c = tris[3 * (first + k) + 2];
                    float t, b1, b2;
                    MESH_COUNT(++best.tris;)
                    const float lim = ANY ? tmax : fminf(tmax, best.t);
                    if (!ray_triangle(rs, v3(a.x, a.y, a.z) - oo, v3(b.x, b.y, b.z) - oo, v3(c.x, c.y, c.z) - oo, lim, t, b1, b2))
                        continue;
                    const int file = in.order[first + k];
                    if (i == skip_inst && file == skip_tri) continue;
                    if (t < best.t || (t == best.t && i == best.inst && file < best.tri)) {
                        best.t = t; best.inst = i; best.tri = file; best.b1 = b1; best.b2 = b2;
                    }
                }
                if (ANY && best.inst >= 0) next = n_nodes;
            }
            node = next;
        }
    }
    return best;
}

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// The vertex at the hit `h` (h.inst >= 0) of a ray of direction d, as the primary kernel and the path kernels write it: the normal
// — the interpolated shading normal, faced like the geometric one, where the mesh has normals and the ray arrives above it; else
// the geometric normal, faced towards the ray — then wi in the onb(nrm) frame and the material's lane for a material instance, the
// reflectance in all three wi slots and the id n_materials for a diffuse or checker instance.
__device__ __forceinline__ void surface_vertex(const Inst* __restrict__ insts, const MeshHit& h, V3 d, int n_materials, V3& nn,
                                               V3& w_in, long long& material) {
    const Inst& in = insts[h.inst];
    const unsigned i0 = in.idx[3 * h.tri], i1 = in.idx[3 * h.tri + 1], i2 = in.idx[3 * h.tri + 2];
    const float b0 = 1.0f - h.b1 - h.b2;
    const V3 p0 = wf_dev::ld3(in.pos + 3ll * i0), p1 = wf_dev::ld3(in.pos + 3ll * i1), p2 = wf_dev::ld3(in.pos + 3ll * i2);
    // geometric normal, through the inverse transpose (a mirroring transform turns the winding: faced by the ray, not by it)
    V3 ng = normal_to_world(in.inv, cross(p1 - p0, p2 - p0));
    ng = (1.0f / sqrtf(dot(ng, ng))) * ng;
    if (dot(ng, d) > 0.0f) ng = -1.0f * ng;
    nn = ng;
    if (in.nrm) {
        const V3 mix = b0 * wf_dev::ld3(in.nrm + 3ll * i0) + h.b1 * wf_dev::ld3(in.nrm + 3ll * i1) + h.b2 * wf_dev::ld3(in.nrm + 3ll * i2);
        V3 ns = normal_to_world(in.inv, mix);
        const float l2 = dot(ns, ns);
        if (l2 > 0.0f && l2 < INFINITY) {
            ns = (1.0f / sqrtf(l2)) * ns;
            if (dot(ns, ng) < 0.0f) ns = -1.0f * ns;
            if (-dot(d, ns) > 0.0f) nn = ns;   // else the geometric normal: every material lane has wi.z > 0
        }
    }
    if (in.surface == BSDFD_MESH_MATERIAL) {
        V3 fs, ft;
        wf_dev::onb(nn, fs, ft);
        w_in = v3(-dot(d, fs), -dot(d, ft), -dot(d, nn));
        material = in.material;
    } else {   // not neural: the reflectance travels in the wi slot, the id is n_materials
        float refl = in.c0;
        if (in.surface == BSDFD_MESH_CHECKER) {
            const float uu = b0 * in.uv[2ll * i0] + h.b1 * in.uv[2ll * i1] + h.b2 * in.uv[2ll * i2];
            const float vv = b0 * in.uv[2ll * i0 + 1] + h.b1 * in.uv[2ll * i1 + 1] + h.b2 * in.uv[2ll * i2 + 1];
            const int cu = (int)floorf(2.0f * in.uscale * uu), cv = (int)floorf(2.0f * in.vscale * vv);
            refl = ((cu + cv) & 1) ? in.c1 : in.c0;
        }
        w_in = v3(refl, refl, refl);
        material = n_materials;
    }
}

// The mesh scene as the geometry policy of the path kernels (bounce_dev.h: Spheres is its sibling).  prim [N,2] is one more array
// of the path state: the (instance, triangle) lane p's vertex lies on, which its rays skip — no epsilon, the rule of
// bsdfd_mesh_intersect — and which `advance` moves on with the vertex.  The walks are whole-wave calls (ONE_WALK): their instance
// loop is wave-uniform and the records arrive through scalar loads, as anywhere else.
struct PathGeom {
    using Hit = MeshHit;
    static constexpr bool ONE_WALK = true;
    const Inst* insts;
    int n_inst;
    int* prim;
    __device__ __forceinline__ static Hit nothing() {
        Hit h;
        h.t = NOTHING; h.inst = -1; h.tri = -1; h.b1 = 0.0f; h.b2 = 0.0f;
        MESH_COUNT(h.nodes = 0; h.tris = 0;)
        return h;
    }
    __device__ __forceinline__ static bool is_hit(const Hit& h) { return h.inst >= 0; }
    __device__ __forceinline__ Hit closest(const wf_dev::Scene&, V3 x, V3 d, long long, long long p) const {
        return walk<false>(insts, n_inst, x, d, NOTHING, prim[2 * p], prim[2 * p + 1]);
    }
    __device__ __forceinline__ bool occluded(const wf_dev::Scene&, V3 x, V3 d, long long, long long p, float dist = NOTHING) const {
        return walk<true>(insts, n_inst, x, d, dist, prim[2 * p], prim[2 * p + 1]).inst >= 0;
    }
    __device__ __forceinline__ void advance(const wf_dev::Scene& sc, const Hit& h, V3 x, V3 d, V3 b, const float thr[3],
                                            unsigned long long seed, unsigned long long pass, unsigned long long path_offset,
                                            int bounce, long long p, float* __restrict__ org, float* __restrict__ nrm,
                                            float* __restrict__ wi, float* __restrict__ wl, long long* __restrict__ mat,
                                            float* __restrict__ beta) const {
        V3 nn, w_in;
        long long material;
        surface_vertex(insts, h, d, sc.n_sph, nn, w_in, material);
        prim[2 * p] = h.inst; prim[2 * p + 1] = h.tri;
        wf_dev::store_vertex(x + h.t * d, nn, w_in, material, b, thr, seed, pass, path_offset, bounce, p, org, nrm, wi, wl, mat, beta);
    }
};

}  // namespace mesh_dev
