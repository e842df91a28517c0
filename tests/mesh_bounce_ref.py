"""Reference for the path kernels on the mesh scene (bsdf_diffusion_sampling_amd/csrc/mesh.hip: ``bsdfd_mesh_bounce``,
``bsdfd_mesh_sample_emitter``): ONE numpy restatement of ``bounce_dev.h``'s ``bounce_vertex`` and ``sample_emitter_vertex`` with
``mesh_dev::PathGeom`` as their geometry, fp64 by default, fp32 on request.

Test infrastructure only.  What comes from where:
* the hits: tests/mesh_ref.py's ``brute_force`` (fp64 in either precision: the hit is the input of the arithmetic here, and which
  rays fp32 may decide differently is its ``marginal`` flag), with ``skip`` = the primitive the vertex lies on and, for the shadow
  ray to a point light, ``tmax`` = the distance to it;
* the next vertex: ``mesh_ref.primary_arrays`` for the continuation ray and its hit — the rule ``bsdfd_mesh_primary`` writes by —
  and ``org = x + t d``;
* the shading arithmetic: tests/bounce_ref.py's ``_bounce``, section by section (modes "cosine" and "lit" only: nothing else is on
  meshes yet); the frames, the emitter pick, the roulette and the next light sample are imported from bounce_ref, pathtrace_ref
  and pathtrace_lights_ref.

The geometry is a dict ``meshes`` [TriMesh], ``instances`` [mesh.Instance], ``n_materials``, ``albedo`` (the proxy's).  A diffuse
or checker instance takes the floor's part: id ``n_materials``, reflectance in the wi slots.
"""
from __future__ import annotations

import numpy as np

import bounce_ref as B
import mesh_ref as MR
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from oracle.wavefront_oracle import env_lookup, mis_power

F = np.float32
MODES = ("cosine", "lit")


def cast_rays(geom: dict, org, d, prim, ask, tmax=None, cast=None):
    """``mesh_ref.brute_force`` on the rows ``ask`` (the others: no hit, nothing marginal), each ray skipping ``prim`` of its row.
    ``cast``: another hit source with ``brute_force``'s signature and record, ``cast(meshes, instances, org, dir, tmax=, skip=)``
    (``mesh_ref.bvh_walk`` over the library's BVHs, where every ray against every triangle costs too much)."""
    n = len(org)
    out = MR._result(n)
    r = np.nonzero(ask)[0]
    if r.size:
        got = (cast or MR.brute_force)(
            geom["meshes"], geom["instances"], np.asarray(org, dtype=np.float64)[r], np.asarray(d, dtype=np.float64)[r],
            tmax=None if tmax is None else np.asarray(tmax, dtype=np.float64)[r], skip=np.asarray(prim)[r])
        for k in out:
            out[k][r] = got[k]
    return out


def bounce(*args, **kwargs):
    """``_bounce`` with numpy's floating-point warnings off: rows that are masked out divide by zero on the way."""
    with np.errstate(all="ignore"):
        return _bounce(*args, **kwargs)


def _bounce(geom: dict, env, mode: str, bounce: int, last: bool, occlusion: bool, seed: int, pass_idx: int, path_offset: int,
            org, nrm, wi, wl, material, prim, beta, rad, wo, pdf_o, pdf_l, f_o=None, f_l=None, n_e: int = 1, has_env: bool = True,
            lsel=None, emit=None, rr_depth=None, bary_tol: float = 0.0, dtype=np.float64, cast=None):
    """One call of bsdfd_mesh_bounce -> dict(org, nrm, wi, wl, material, prim, beta, rad, thr): the arrays after the call (rows the
    kernel does not write keep their input values), and what the comparisons need: ``hit`` (the brute-force record of the
    continuation rays: t, prim, bary, marginal), ``shadow`` (of the cosine strategy's shadow rays), ``t`` [N] and ``d`` [N,3] of the
    continuation, ``fragile`` and ``mix_len`` of ``primary_arrays`` (with ``bary_tol``), ``would`` (rows that continue before the
    roulette) and, with ``rr_depth``, ``u``, ``q``, ``survive``, ``killed`` as tests/bounce_ref.py returns them.  ``cast``: ``cast_rays``'s hit source."""
    assert mode in MODES and (f_o is None) == (f_l is None) and (rr_depth is None or rr_depth >= 1)
    n_b = geom["n_materials"]
    n = len(material)
    to = lambda a: np.asarray(a).astype(dtype)
    x64 = np.asarray(org, dtype=np.float64)
    org, nrm, wi, wl, beta, rad, wo = (to(a) for a in (org, nrm, wi, wl, beta, rad, wo))
    live = (material >= 0) & (material <= n_b)
    floor = live & (material == n_b)
    ball = live & ~floor
    fs, ft, nn = LR._frames(nrm, live, dtype)
    to_world = lambda v: v[:, 0:1] * fs + v[:, 1:2] * ft + v[:, 2:3] * nn
    env64 = np.asarray(env, dtype=np.float64)
    look = lambda dw: env_lookup(env64, dw.astype(F)).astype(dtype)
    inv_pi = dtype(0.31830988618379067154)
    albedo = np.asarray(geom["albedo"], dtype=F).astype(dtype)[None, :]
    sel_p = dtype(1) if mode == "cosine" else dtype(1) / dtype(n_e)
    env_emits = mode != "lit" or has_env
    point = np.zeros(n, dtype=bool) if mode == "cosine" or lsel is None else live & (lsel >= 0)
    sampled = point
    emit = np.zeros((n, 3), dtype=dtype) if mode == "cosine" else to(emit)

    lw, dw = to_world(wl), to_world(wo)
    pb = np.where(np.isfinite(pdf_o) & (pdf_o > 0), pdf_o, 0).astype(dtype)
    pbl = np.where(np.isfinite(pdf_l) & (pdf_l > 0), pdf_l, 0).astype(dtype)
    gt_o = np.zeros(n, dtype=bool) if f_o is None else ~np.isnan(f_o[:, 0])
    gt_l = np.zeros(n, dtype=bool) if f_l is None else ~np.isnan(f_l[:, 0])
    thr_o = np.where(gt_o[:, None], (np.zeros((n, 3)) if f_o is None else np.nan_to_num(f_o)).astype(dtype) / pb[:, None], albedo)
    f_l_v = albedo * pbl[:, None] if f_l is None else np.where(gt_l[:, None], np.nan_to_num(f_l).astype(dtype), albedo * pbl[:, None])
    follow = ball & (pb > 0) & ((wo[:, 2] > 0) if occlusion else np.ones(n, dtype=bool))
    ok_l = ball & ((pbl > 0) | gt_l)
    pl = wl[:, 2] * inv_pi * sel_p
    # ---- the rays: one closest-hit walk along the continuation ray of floor and ball lanes alike, one any-hit walk along the
    # cosine strategy's light sample; both skip the primitive the vertex lies on ----
    d = np.where(floor[:, None], lw, dw)
    hit = cast_rays(geom, x64, d, prim, (floor | follow) & bool(occlusion), cast=cast)
    shadow = cast_rays(geom, x64, lw, prim, ok_l & ~sampled & (pl > 0) & bool(occlusion), cast=cast)
    is_hit = hit["prim"][:, 0] >= 0
    hit_l = np.where(floor, is_hit, shadow["prim"][:, 0] >= 0)   # something along wl
    hit_o = is_hit & ~floor
    e_l = look(lw)
    # ---- floor vertices ----
    refl = wi[:, 0:1]
    L_floor = np.where(hit_l[:, None], dtype(0), refl * e_l) if env_emits else np.zeros((n, 3), dtype=dtype)
    L_floor = L_floor + np.where(sampled[:, None], emit, dtype(0))
    # ---- ball vertices: the two strategies of shade_kernel ----
    p_light = np.maximum(wo[:, 2], 0) * inv_pi * sel_p
    w_o = mis_power(pb, p_light).astype(dtype)
    L = np.where((follow & ~hit_o)[:, None], w_o[:, None] * look(dw) * thr_o, dtype(0)) if env_emits else np.zeros((n, 3), dtype=dtype)
    L = L + np.where((ok_l & sampled)[:, None], emit * f_l_v, dtype(0))
    ok_c = ok_l & ~sampled & (pl > 0) & ~hit_l
    w_l = np.where(ok_c, mis_power(pl, pbl).astype(dtype) / pl, dtype(0))
    L = L + np.where(ok_c[:, None], w_l[:, None] * e_l * f_l_v, dtype(0))
    L = np.where(floor[:, None], L_floor, L)
    rad_new = np.where(live[:, None], rad + beta * L, rad)
    # ---- where the path goes ----
    go = (follow & hit_o) | (floor & hit_l)
    thr = np.where(floor[:, None], refl, thr_o)
    cont = would = go & (not last)
    thr_on = thr
    extra = {}
    if rr_depth is not None:
        u, q, ok = B.roulette(beta, thr, seed, pass_idx, bounce, path_offset, n, dtype)
        if not last and bounce + 1 >= rr_depth:
            cont = would & ok
            thr_on = thr * (dtype(1) / q)[:, None]
        extra = dict(u=u, q=q, survive=cont, killed=would & ~cont)
    # ---- the continuation: bsdfd_mesh_primary's vertex for the ray of direction d and its hit ----
    nxt = MR.primary_arrays(geom["meshes"], geom["instances"], n_b, d.astype(np.float64), hit, bary_tol=bary_tol)
    tt = np.where(is_hit, hit["t"], 0.0).astype(dtype)
    return dict(
        org=np.where(cont[:, None], org + tt[:, None] * d, org),
        nrm=np.where(cont[:, None], nxt["nrm"].astype(dtype), nrm),
        wi=np.where(cont[:, None], nxt["wi"].astype(dtype), wi),
        wl=np.where(cont[:, None], R.next_wl(seed, pass_idx, bounce, path_offset, n).astype(dtype), wl),
        material=np.where(live, np.where(cont, nxt["material"], n_b + 1), material).astype(np.int64),
        prim=np.where(cont[:, None], hit["prim"], prim).astype(np.int64),
        beta=np.where(cont[:, None], beta * thr_on, beta),
        rad=rad_new, thr=thr, hit=hit, shadow=shadow, t=np.where(is_hit, hit["t"], np.nan), d=d.astype(np.float64),
        fragile=nxt["fragile"] & is_hit, mix_len=nxt["mix_len"], would=would, **extra)


def sample_emitter(geom: dict, lights: dict, has_env: bool, bounce: int, occlusion: bool, seed: int, pass_idx: int, path_offset: int,
                   org, nrm, wi, material, prim, wl, dtype=np.float64, cast=None):
    """One call of bsdfd_mesh_sample_emitter -> dict(wl, lsel, emit, lit, shadow, cos): tests/pathtrace_lights_ref.py's
    ``sample_emitter`` with the shadow ray cast in the mesh scene, bounded by the distance to the light (``shadow``: its brute-force
    record; ``cos``: the light's cosine at the vertex).  ``cast``: ``cast_rays``'s hit source."""
    with np.errstate(all="ignore"):
        n_b, n = geom["n_materials"], len(material)
        n_l = len(lights["position"])
        n_e = n_l + int(bool(has_env))
        x64 = np.asarray(org, dtype=np.float64)
        org, nrm, wi, wl = (np.asarray(a).astype(dtype) for a in (org, nrm, wi, wl))
        live = (material >= 0) & (material <= n_b)
        floor = live & (material == n_b)
        pick = LR.pick_emitter(seed, pass_idx, bounce, path_offset, n, n_e)
        point = live & (pick < n_l)
        k = np.where(point, pick, 0)
        P, I = lights["position"].astype(dtype)[k], lights["intensity"].astype(dtype)[k]
        fs, ft, nn = LR._frames(nrm, live, dtype)
        v = P - org
        d2 = R._dot(v, v)
        dist = np.sqrt(d2)
        d = (dtype(1) / dist)[:, None] * v
        cosl = R._dot(d, nn)
        lit = point & (cosl > 0)
        shadow = cast_rays(geom, x64, d, prim, lit & bool(occlusion), tmax=dist, cast=cast)
        lit &= ~(shadow["prim"][:, 0] >= 0)
        s = np.where(lit, dtype(n_e) / d2, dtype(0))
        s = np.where(floor, s * wi[:, 0] * dtype(LR.INV_PI) * cosl, s)
        local = np.stack([R._dot(d, fs), R._dot(d, ft), cosl], 1)
        return dict(wl=np.where((point & ~floor)[:, None], local, wl).astype(dtype),
                    lsel=np.where(live, np.where(point, pick, -1), -2).astype(np.int32),
                    emit=np.where(point[:, None], s[:, None] * I, dtype(0)).astype(dtype), lit=lit, shadow=shadow, cos=cosl)


# ---- the kernel scene and the synthetic wavefront of tests/test_gpu_mesh_path.py ---------------------------------------------
LID = [[12.0, 0.0, 0.0, -6.0], [0.0, 0.0, 1.0, -1.2], [0.0, -12.0, 0.0, 6.0]]   # the unit grid -> a 12 x 12 floor at y = -1.2, facing up


def kernel_scene(M):
    """The octahedron (128 triangles, normals = positions) under mesh_ref's three transforms — plain: material 0, scaled and
    rotated: material 1, mirrored: diffuse 0.3 — over a 4 x 4 grid as a checkered floor.  ``M``: the mesh module."""
    octa, _ = MR.octahedron(2, M.TriMesh)
    grid = MR.grid_mesh(4, 4, M.TriMesh)
    plain, scaled, mirrored = MR.transforms()
    inst = [M.Instance(0, plain, material=0), M.Instance(0, scaled, material=1), M.Instance(0, mirrored, diffuse=0.3),
            M.Instance(1, LID, checker=(0.4, 0.2, 4.0, 4.0))]
    return dict(meshes=[octa, grid], instances=inst, n_materials=2, albedo=[0.9, 0.6, 0.3])


def synthetic_vertices(geom: dict, n: int = 4096, seed: int = 7):
    """``n`` vertices ON the scene's surfaces as bsdfd_mesh_bounce takes them: mesh_ref.rays_at(boxes, 3 n, seed) through fp64 brute
    force, the first n unmarginal hits, ``org = float32(o + t d)`` with prim, nrm, wi and the id from ``primary_arrays``; then the
    sampler's answers the way pathtrace_ref.synthetic_vertices makes them — wo over the whole sphere (~20 % below the surface),
    pdf_o over six decades with zeros, infinities and NaNs, NaN rows in f (= proxy) — and ~15 % ended rows, whose id is above
    n_materials and whose state is garbage the kernel must neither read into anything nor overwrite."""
    g = np.random.default_rng(seed)
    o, d = MR.rays_at(MR.instance_boxes(geom["meshes"], geom["instances"]), 3 * n, seed=seed)
    ref = MR.brute_force(geom["meshes"], geom["instances"], o, d)
    s = np.nonzero((ref["t"] < MR.NOTHING) & ~ref["marginal"])[0][:n]
    assert s.size == n, f"only {s.size} unmarginal hits"
    ref = {k: v[s] for k, v in ref.items()}
    o, d = o[s].astype(np.float64), d[s].astype(np.float64)
    org = o + ref["t"][:, None] * d                   # (t is the parameter of the unnormalised ray)
    d /= np.linalg.norm(d, axis=1, keepdims=True)      # (primary_arrays forms wi for a unit direction)
    v = MR.primary_arrays(geom["meshes"], geom["instances"], geom["n_materials"], d, ref)
    n_b = geom["n_materials"]
    mat = v["material"].copy()
    nrm, wi = v["nrm"].copy(), v["wi"].copy()
    prim = ref["prim"].astype(np.int32)
    dead = g.random(n) < 0.15
    mat[dead] = np.where(g.random(n) < 0.5, n_b + 1, n_b + 7)[dead]
    wl, wo = R._cosine_dirs(g, n), R._sphere_dirs(g, n)
    wo[:, 2] = np.where(g.random(n) < 0.8, np.abs(wo[:, 2]), -np.abs(wo[:, 2]))
    wo[g.random(n) < 0.01, 2] = 0.0
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    pdf_o = np.exp(g.uniform(np.log(1e-3), np.log(1e3), n))
    special = g.random(n)
    pdf_o = np.where(special < 0.03, 0.0, np.where(special < 0.06, np.inf, np.where(special < 0.09, np.nan, pdf_o)))
    pdf_l = np.where(g.random(n) < 0.05, 0.0, np.exp(g.uniform(np.log(1e-3), np.log(1e2), n)))
    f_o = np.where(np.isfinite(pdf_o) & (pdf_o > 0), pdf_o, 1.0)[:, None] * g.uniform(0.1, 1.0, (n, 3))
    f_l = g.uniform(0.0, 2.0, (n, 3))
    no_gt = g.random(n) < 0.4
    f_o[no_gt], f_l[no_gt] = np.nan, np.nan
    beta, rad = g.uniform(0.2, 1.0, (n, 3)), g.uniform(0.0, 1.0, (n, 3))
    for a in (org, nrm, wi, wl, beta):      # an ended path's state is garbage
        a[dead] = np.nan
    prim[dead] = -9
    out = dict(org=org, nrm=nrm, wi=wi, wl=wl, beta=beta, rad=rad, wo=wo, pdf_o=pdf_o, pdf_l=pdf_l, f_o=f_o, f_l=f_l)
    out = {k: np.ascontiguousarray(a, dtype=F) for k, a in out.items()}
    out["material"], out["prim"] = mat.astype(np.int64), prim
    return out


STATE = ("org", "nrm", "wi", "wl", "material", "prim", "beta", "rad", "wo", "pdf_o", "pdf_l", "f_o", "f_l")
