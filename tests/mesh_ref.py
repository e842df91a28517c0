"""numpy reference of the mesh ray caster (csrc/mesh.hip), in fp64.

* ``brute_force``: every ray against every triangle of every instance (Möller-Trumbore in world space), the library's tie rule —
  smaller t, on equal t the smaller (instance, file triangle) — and the MARGINAL flag of a ray: it passes within barycentric
  distance ``EDGE_EPS`` of an edge of some triangle whose plane it crosses at 0 < t <= t_best (1 + EDGE_EPS), the crossing point
  inside or outside that triangle.  An fp32 walk may legitimately report the neighbour there; everywhere else it may not.
* ``bvh_walk``: the same answers from a numpy walk of the BVH the library built (``mesh.build_bvh``), one walker per
  (ray, instance) in object space, all walkers of a mesh advanced together.
* ``fp32_restatement_error``: the kernel's own formulas (object-space ray, Woop's shear, edge functions without contraction)
  restated in numpy fp32 on the reference's hit triangle: the worst error of t (relative) and of the barycentrics (absolute)
  against fp64.  The GPU tests hold the kernel to 4 x these figures.
* ``primary_arrays``: nrm, wi, material of ``bsdfd_mesh_primary`` from a hit record.
"""
import numpy as np

EDGE_EPS = 1e-5
NOTHING = 3.0e38
MARGINAL_CAP = 0.01


def instance_matrix(inst):
    """to_world as the library receives it: rounded to fp32, then exact."""
    return inst.matrix().astype(np.float32).astype(np.float64)


def world_triangles(meshes, instances):
    """-> (V [T,3,3] world vertices, inst [T], tri [T]) ordered by (instance, file triangle)."""
    V, I, T = [], [], []
    for k, inst in enumerate(instances):
        m = meshes[inst.mesh]
        M = instance_matrix(inst)
        p = m.positions.astype(np.float64) @ M[:, :3].T + M[:, 3]
        V.append(p[m.indices.astype(np.int64)])
        I.append(np.full(m.n_triangles, k, dtype=np.int64))
        T.append(np.arange(m.n_triangles, dtype=np.int64))
    return np.concatenate(V), np.concatenate(I), np.concatenate(T)


def _moller_trumbore(v0, e1, e2, o, d):
    """Broadcasting fp64 test -> (t, u, v, ok) with ok = the ray crosses the triangle's plane (det != 0)."""
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    ok = det != 0.0
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = o - v0
    u = (tv * p).sum(-1) * inv
    q = np.cross(tv, e1)
    v = (d * q).sum(-1) * inv
    t = (e2 * q).sum(-1) * inv
    return t, u, v, ok


def _near_edge(u, v):
    w = 1.0 - u - v
    e = EDGE_EPS
    band = lambda a, b, c: (np.abs(a) < e) & (b > -e) & (b < 1 + e) & (c > -e) & (c < 1 + e)
    return band(u, v, w) | band(v, u, w) | band(w, u, v)


def _result(n):
    return dict(t=np.full(n, NOTHING), prim=np.full((n, 2), -1, dtype=np.int64), bary=np.zeros((n, 2)),
                marginal=np.zeros(n, dtype=bool), edge_t=np.full(n, np.inf))


def brute_force(meshes, instances, org, dir, tmax=None, skip=None, chunk=96):
    V, I, T = world_triangles(meshes, instances)
    v0, e1, e2 = V[None, :, 0], (V[:, 1] - V[:, 0])[None], (V[:, 2] - V[:, 0])[None]
    org, dir = np.asarray(org, dtype=np.float64), np.asarray(dir, dtype=np.float64)
    n = org.shape[0]
    tmax = np.full(n, np.inf) if tmax is None else np.asarray(tmax, dtype=np.float64)
    out = _result(n)
    for lo in range(0, n, chunk):
        sl = slice(lo, min(lo + chunk, n))
        t, u, v, ok = _moller_trumbore(v0, e1, e2, org[sl, None], dir[sl, None])
        ok &= (t > 0.0) & (t <= tmax[sl, None])
        if skip is not None:
            ok &= ~((I[None] == skip[sl, 0:1]) & (T[None] == skip[sl, 1:2]))
        inside = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0)
        tt = np.where(inside, t, np.inf)
        best = tt.argmin(1)                       # the first minimum: the smaller (instance, triangle) on equal t
        rows = np.arange(tt.shape[0])
        tb = tt[rows, best]
        hit = np.isfinite(tb)
        out["t"][sl] = np.where(hit, tb, NOTHING)
        out["prim"][sl] = np.where(hit[:, None], np.stack([I[best], T[best]], 1), -1)
        out["bary"][sl] = np.where(hit[:, None], np.stack([u[rows, best], v[rows, best]], 1), 0.0)
        edge = ok & _near_edge(u, v)
        out["edge_t"][sl] = np.where(edge, t, np.inf).min(1)      # the nearest near-edge plane crossing
        out["marginal"][sl] = (edge & (t <= (tb * (1 + EDGE_EPS))[:, None])).any(1)
    return out


def _slab(o, inv_d, lo, hi, limit):
    with np.errstate(invalid="ignore", over="ignore"):
        t0, t1 = (lo - o) * inv_d, (hi - o) * inv_d
    bad = np.isnan(t0) | np.isnan(t1)
    near = np.where(bad, -np.inf, np.minimum(t0, t1)).max(1)
    far = np.where(bad, np.inf, np.maximum(t0, t1)).min(1)
    return ~(np.maximum(near, 0.0) > np.minimum(far, limit))


def bvh_walk(meshes, instances, bvhs, org, dir, tmax=None, skip=None):
    """``brute_force``'s answers through the library's BVH: bvhs[k] = mesh.build_bvh(meshes[k])."""
    org, dir = np.asarray(org, dtype=np.float64), np.asarray(dir, dtype=np.float64)
    n = org.shape[0]
    tmax = np.full(n, np.inf) if tmax is None else np.asarray(tmax, dtype=np.float64)
    out = _result(n)
    marg_t = np.full(n, np.inf)                    # the nearest near-edge plane crossing of each ray
    for k, inst in enumerate(instances):
        m = meshes[inst.mesh]
        nodes, order = bvhs[inst.mesh]
        M = instance_matrix(inst)
        A = np.linalg.inv(M[:, :3])
        o, d = (org - M[:, 3]) @ A.T, dir @ A.T
        with np.errstate(divide="ignore"):
            inv_d = 1.0 / d
        P = m.positions.astype(np.float64)
        tri = m.indices.astype(np.int64)
        pad = 1e-4 * float((nodes["hi"][0] - nodes["lo"][0]).max())
        nlo, nhi = nodes["lo"].astype(np.float64) - pad, nodes["hi"].astype(np.float64) + pad
        skips, leaf = nodes["skip"].astype(np.int64), nodes["tris"].astype(np.int64)
        bt, btri, bb = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.zeros((n, 2))
        node = np.zeros(n, dtype=np.int64)
        act = np.arange(n)
        while act.size:
            i = node[act]
            limit = np.minimum(tmax[act], bt[act]) * (1 + 2 * EDGE_EPS)
            hitbox = _slab(o[act], inv_d[act], nlo[i], nhi[i], limit)
            node[act] = np.where(hitbox, i + 1, skips[i])
            at_leaf = hitbox & (leaf[i] != 0)
            for j in range(int((leaf[i[at_leaf]] & 7).max()) if at_leaf.any() else 0):
                sel = at_leaf & ((leaf[i] & 7) > j)
                r = act[sel]
                f = order[(leaf[i[sel]] >> 3) + j].astype(np.int64)
                v0 = P[tri[f, 0]]
                t, u, v, ok = _moller_trumbore(v0, P[tri[f, 1]] - v0, P[tri[f, 2]] - v0, o[r], d[r])
                ok &= (t > 0.0) & (t <= tmax[r])
                if skip is not None:
                    ok &= ~((skip[r, 0] == k) & (skip[r, 1] == f))
                edge = ok & _near_edge(u, v)
                np.minimum.at(marg_t, r[edge], t[edge])
                inside = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0)
                win = inside & ((t < bt[r]) | ((t == bt[r]) & (f < btri[r])))
                # (a ray is in one leaf at a time and a leaf lists a triangle once: no two candidates of a ray in one step)
                bt[r[win]], btri[r[win]] = t[win], f[win]
                bb[r[win]] = np.stack([u[win], v[win]], 1)
            act = act[node[act] < nodes.shape[0]]
        better = bt < out["t"]                       # strict: the smaller instance keeps an equal t
        out["t"][better] = bt[better]
        out["prim"][better] = np.stack([np.full(int(better.sum()), k), btri[better]], 1)
        out["bary"][better] = bb[better]
    out["edge_t"] = marg_t
    out["marginal"] = np.isfinite(marg_t) & (marg_t <= np.where(out["t"] < NOTHING, out["t"], np.inf) * (1 + EDGE_EPS))
    return out


def assert_marginal_cap(ref):
    """The condition on the inputs the comparisons rest on: at most 1 % marginal rays."""
    share = ref["marginal"].mean() if ref["marginal"].size else 0.0
    assert share <= MARGINAL_CAP or ref["marginal"].sum() <= 1 and ref["marginal"].size < 100, f"{share:.3%} marginal rays"


# ---- the kernel's formulas in fp32 ----
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def woop_fp32(meshes, instances, org, dir, prim):
    """t, b1, b2 of the rays against their triangles prim [n,2] (all hits), every operation rounded to fp32 in the kernel's order
    (numpy fuses nothing): world -> object with the fp32 inverse, the permutation and shear, the edge functions, T / det."""
    org, dir = _f32(org), _f32(dir)
    n = org.shape[0]
    t, b1, b2 = (np.zeros(n, dtype=np.float32) for _ in range(3))
    for k, inst in enumerate(instances):
        r = np.nonzero(prim[:, 0] == k)[0]
        if not r.size:
            continue
        m = meshes[inst.mesh]
        M = instance_matrix(inst)
        A64 = np.linalg.inv(M[:, :3])
        A, tr = _f32(A64), _f32(-(A64 @ M[:, 3]))
        mul = lambda X: (A[:, 0] * X[:, 0:1] + A[:, 1] * X[:, 1:2]) + A[:, 2] * X[:, 2:3]
        o, d = mul(org[r]) + tr, mul(dir[r])
        kz = np.abs(d).argmax(1)                      # (first maximum: x over y over z on ties, as the kernel)
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        rows = np.arange(r.size)
        flip = d[rows, kz] < 0
        kx, ky = np.where(flip, ky, kx), np.where(flip, kx, ky)
        sz = np.float32(1.0) / d[rows, kz]
        sx, sy = d[rows, kx] * sz, d[rows, ky] * sz
        tri = m.indices[prim[r, 1]].astype(np.int64)
        P = []
        for c in range(3):
            q = m.positions[tri[:, c]] - o
            qz = q[rows, kz]
            P.append((q[rows, kx] - sx * qz, q[rows, ky] - sy * qz, sz * qz))
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = P
        U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        det = U + V + W
        inv = np.float32(1.0) / det
        t[r] = ((U * az + V * bz) + W * cz) * inv
        b1[r], b2[r] = V * inv, W * inv
    return t, b1, b2


def fp32_restatement_error(meshes, instances, org, dir, ref):
    """(worst relative error of t, worst absolute error of a barycentric) of ``woop_fp32`` against ``ref`` on its unmarginal hits."""
    sel = (ref["t"] < NOTHING) & ~ref["marginal"]
    if not sel.any():
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        t, b1, b2 = woop_fp32(meshes, instances, np.asarray(org)[sel], np.asarray(dir)[sel], ref["prim"][sel])
    et = np.abs(t.astype(np.float64) - ref["t"][sel]) / ref["t"][sel]
    eb = np.maximum(np.abs(b1 - ref["bary"][sel, 0]), np.abs(b2 - ref["bary"][sel, 1]))
    return float(et.max()), float(eb.max())


# ---- bsdfd_mesh_primary from a hit record ----
def onb(nv):
    """wf_dev::onb (Duff et al. 2017) on rows of unit normals."""
    sign = np.copysign(1.0, nv[:, 2])
    a = -1.0 / (sign + nv[:, 2])
    b = nv[:, 0] * nv[:, 1] * a
    s = np.stack([1.0 + sign * nv[:, 0] ** 2 * a, sign * b, -sign * nv[:, 0]], 1)
    t = np.stack([b, sign + nv[:, 1] ** 2 * a, -nv[:, 1]], 1)
    return s, t


def primary_arrays(meshes, instances, n_materials, dir, ref, bary_tol=0.0):
    """-> dict(nrm, wi, material, fragile, mix_len): what ``bsdfd_mesh_primary`` writes for the rays ``dir`` with the hit record
    ``ref``.  ``fragile`` marks the lanes within the kernel's error bar of one of the rule's own discontinuities, where fp32 may
    fall on the other side.  With barycentrics good to ``bary_tol`` the interpolated normal is good to 3 bary_tol (+ 1e-5 of
    rounding) and an interpolated uv to bary_tol times the triangle's uv span, so fragile is: the shading normal that close to
    grazing the ray or the geometric normal, a frame normal with |z| that small (the basis flips with the sign of z), a checker
    coordinate that close to a cell boundary."""
    near = 3.0 * bary_tol + 1e-5
    d = np.asarray(dir, dtype=np.float64)
    n = d.shape[0]
    nrm, wi = np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1))
    mat = np.full(n, n_materials + 1, dtype=np.int64)
    fragile = np.zeros(n, dtype=bool)
    mix_len = np.ones(n)
    for k, inst in enumerate(instances):
        r = np.nonzero(ref["prim"][:, 0] == k)[0]
        if not r.size:
            continue
        m = meshes[inst.mesh]
        M = instance_matrix(inst)
        NT = np.linalg.inv(M[:, :3]).T                # normals: the inverse transpose
        tri = m.indices[ref["prim"][r, 1]].astype(np.int64)
        b1, b2 = ref["bary"][r, 0], ref["bary"][r, 1]
        b0 = 1.0 - b1 - b2
        P = m.positions.astype(np.float64)
        ng = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]) @ NT.T
        ng /= np.linalg.norm(ng, axis=1, keepdims=True)
        ng[(ng * d[r]).sum(1) > 0] *= -1
        nn = ng.copy()
        if m.normals is not None:
            N = m.normals.astype(np.float64)
            mix = b0[:, None] * N[tri[:, 0]] + b1[:, None] * N[tri[:, 1]] + b2[:, None] * N[tri[:, 2]]
            ns = mix @ NT.T
            ln = np.linalg.norm(ns, axis=1)
            ok = (ln > 0) & np.isfinite(ln)
            ns = ns / np.where(ok, ln, 1.0)[:, None]
            facing = (ns * ng).sum(1)
            ns[facing < 0] *= -1
            cos = -(ns * d[r]).sum(1)
            use = ok & (cos > 0)
            nn[use] = ns[use]
            fragile[r] |= ok & ((np.abs(cos) < near) | (np.abs(facing) < near))
            mix_len[r] = np.where(ok, np.linalg.norm(mix, axis=1), 1.0)
        nrm[r] = nn
        if inst.material is not None:
            s, t = onb(nn)
            wi[r] = -np.stack([(d[r] * s).sum(1), (d[r] * t).sum(1), (d[r] * nn).sum(1)], 1)
            mat[r] = inst.material
            fragile[r] |= np.abs(nn[:, 2]) < near
        else:
            refl = np.full(r.size, inst.diffuse if inst.diffuse is not None else 0.0)
            if inst.checker is not None:
                c0, c1, us, vs = inst.checker
                UV = m.uvs.astype(np.float64)
                uv = b0[:, None] * UV[tri[:, 0]] + b1[:, None] * UV[tri[:, 1]] + b2[:, None] * UV[tri[:, 2]]
                cu, cv = 2 * us * uv[:, 0], 2 * vs * uv[:, 1]
                refl = np.where((np.floor(cu) + np.floor(cv)).astype(np.int64) & 1, c1, c0)
                span = np.abs(UV[tri[:, 1]] - UV[tri[:, 0]]) + np.abs(UV[tri[:, 2]] - UV[tri[:, 0]])
                fragile[r] |= ((np.abs(cu - np.round(cu)) < 2 * us * bary_tol * span[:, 0] + 1e-6)
                               | (np.abs(cv - np.round(cv)) < 2 * vs * bary_tol * span[:, 1] + 1e-6))
            wi[r] = refl[:, None]
            mat[r] = n_materials
    return dict(nrm=nrm, wi=wi, material=mat, fragile=fragile, mix_len=mix_len)


# ---- test geometry ----
def grid_mesh(nx, ny, TriMesh, z=0.0):
    """A flat nx x ny grid of quads over [0,1]^2, two triangles each, with normals and uv."""
    xs, ys = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="ij")
    pos = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, z)], 1)
    idx = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
            idx += [(a, b, c), (a, c, d)]
    return TriMesh(pos, np.array(idx), normals=np.tile([0.0, 0.0, 1.0], (pos.shape[0], 1)), uvs=pos[:, :2].copy())


def octahedron(levels, TriMesh):
    """A closed mesh: the unit octahedron subdivided ``levels`` times (8 * 4^levels triangles), shared vertices merged, normals =
    positions -> (TriMesh, edges [E,2])."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    verts = [np.array(v, dtype=np.float64) for v in verts]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nxt = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = nxt
    pos = np.array(verts, dtype=np.float32)
    idx = np.array(faces)
    edges = np.unique(np.sort(np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]), axis=1), axis=0)
    return TriMesh(pos, idx, normals=pos / np.linalg.norm(pos, axis=1, keepdims=True)), edges


def transforms():
    """The three instance transforms of the tests: plain, non-uniformly scaled and rotated, mirrored (and non-uniform)."""
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    plain = np.hstack([np.eye(3), [[0.0], [0.0], [0.0]]])
    scaled = np.hstack([rot @ np.diag([1.5, 0.6, 0.9]), [[3.0], [0.5], [-0.4]]])
    mirrored = np.hstack([np.diag([-0.8, 1.3, 0.7]), [[-3.0], [0.2], [0.6]]])
    return plain, scaled, mirrored


def instance_boxes(meshes, instances):
    """The world box [lo, hi] of every instance."""
    out = []
    for inst in instances:
        M = instance_matrix(inst)
        p = meshes[inst.mesh].positions.astype(np.float64) @ M[:, :3].T + M[:, 3]
        out.append((p.min(0), p.max(0)))
    return out


def rays_at(boxes, n, seed):
    """A mix of rays, each around one of the world boxes (lo, hi): origins on a sphere around it aimed at points in and just
    around it (hits and near misses), origins INSIDE the box with random directions, and rays pointing away (hits behind the
    origin).  A tmax that cuts hits off is the caller's, from the reference's t."""
    g = np.random.default_rng(seed)
    pick = g.integers(0, len(boxes), n)
    lo, hi = np.array([b[0] for b in boxes], dtype=np.float64)[pick], np.array([b[1] for b in boxes], dtype=np.float64)[pick]
    c, rad = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo, axis=1, keepdims=True)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    org = c + (1.5 + g.uniform(0, 2, (n, 1))) * rad * u
    target = lo + g.uniform(-0.15, 1.15, (n, 3)) * (hi - lo)
    d = target - org
    kind = g.uniform(size=n)
    inside = kind < 0.2
    org[inside] = (lo + g.uniform(0.05, 0.95, (n, 3)) * (hi - lo))[inside]
    v = g.normal(size=(n, 3))
    d[inside] = v[inside]
    away = (kind >= 0.2) & (kind < 0.3)
    d[away] *= -1
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= g.uniform(0.5, 2.0, (n, 1))               # the direction need not be a unit vector: t is the parameter
    return org.astype(np.float32), d.astype(np.float32)
