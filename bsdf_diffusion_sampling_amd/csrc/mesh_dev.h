// mesh_dev.h — the ray caster over instanced triangle meshes (mesh.hip): the instance record, the conservative slab test, the
// watertight ray/triangle test and the stackless walk of a threaded BVH.  One ray per lane.  `walk<false>` is the closest hit,
// `walk<true>` leaves at the first accepted hit; both skip the primitive a ray starts on.  A path kernel that intersects
// meshes includes this header and calls `walk` where it calls wf_dev::trace today.
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

}  // namespace mesh_dev
