"""Reference for the point-emitter kernels (bsdf_diffusion_sampling_amd/csrc/pathlights.hip): a numpy restatement of
``bsdfd_wf_sample_emitter``, fp64 by default, fp32 on request, on top of tests/pathtrace_ref.py (``trace``, the bases, the
synthetic scene and wavefront).  ``bsdfd_wf_bounce_lit`` is tests/bounce_ref.py's ``bounce`` in the mode "lit".

Test infrastructure only.  Lights are a dict ``position`` [n,3], ``intensity`` [n,3] (world, y up, stored in fp32 like the scene).
"""
from __future__ import annotations

import numpy as np

import pathtrace_ref as R
from oracle.wavefront_oracle import onb

F = np.float32
INV_PI = 0.31830988618379067154


def make_lights(position, intensity):
    inten = [np.full(3, i, dtype=F) if np.ndim(i) == 0 else np.asarray(i, dtype=F) for i in intensity]
    return dict(position=np.asarray(position, dtype=F).reshape(-1, 3), intensity=np.stack(inten).reshape(-1, 3))


def pick_emitter(seed: int, pass_idx: int, bounce: int, path_offset: int, n: int, n_e: int):
    """(u0 * n_e) >> 32 of the paths path_offset .. path_offset + n - 1 at depth ``bounce`` — integers throughout."""
    u = R.tagged_draw(0x4C697465, seed, pass_idx, bounce, path_offset, n)   # "Lite"
    return ((u[0].astype(np.uint64) * np.uint64(n_e)) >> np.uint64(32)).astype(np.int64)


def _frames(nrm, live, dtype):
    safe_n = np.where(live[:, None], nrm, np.array([0.0, 0.0, 1.0], dtype=dtype))
    fs, ft = onb(safe_n.astype(F))
    return fs.astype(dtype), ft.astype(dtype), safe_n


def sample_emitter(scene: dict, lights: dict, has_env: bool, bounce: int, occlusion: bool, seed: int, pass_idx: int,
                   path_offset: int, org, nrm, wi, material, wl, dtype=np.float64):
    """One call of bsdfd_wf_sample_emitter -> dict(wl, lsel, emit, lit): ``wl`` after the call (rows the kernel does not write
    keep their input), ``lsel`` [N] (-2 on ended rows, which the kernel leaves alone), ``emit`` [N,3] (0 there), ``lit`` [N] the
    visibility decision of the rows that picked a point."""
    with np.errstate(all="ignore"):
        n_b, n = len(scene["spheres"]), len(material)
        n_l = len(lights["position"])
        n_e = n_l + int(bool(has_env))
        org, nrm, wi, wl = (np.asarray(a).astype(dtype) for a in (org, nrm, wi, wl))
        live = (material >= 0) & (material <= n_b)
        floor = live & (material == n_b)
        pick = pick_emitter(seed, pass_idx, bounce, path_offset, n, n_e)
        point = live & (pick < n_l)
        k = np.where(point, pick, 0)
        P, I = lights["position"].astype(dtype)[k], lights["intensity"].astype(dtype)[k]
        fs, ft, nn = _frames(nrm, live, dtype)
        v = P - org
        d2 = R._dot(v, v)
        dist = np.sqrt(d2)
        d = (dtype(1) / dist)[:, None] * v
        cosl = R._dot(d, nn)
        lit = point & (cosl > 0)
        if occlusion:
            t, hid, _, _ = R.trace(scene, org, d, np.where(live, material, -2), dtype)
            lit &= ~((hid >= 0) & (t < dist))
        s = np.where(lit, dtype(n_e) / d2, dtype(0))
        s = np.where(floor, s * wi[:, 0] * dtype(INV_PI) * cosl, s)
        local = np.stack([R._dot(d, fs), R._dot(d, ft), cosl], 1)
        return dict(wl=np.where((point & ~floor)[:, None], local, wl).astype(dtype),
                    lsel=np.where(live, np.where(point, pick, -1), -2).astype(np.int32),
                    emit=np.where(point[:, None], s[:, None] * I, dtype(0)).astype(dtype), lit=lit)


# ---- the synthetic lights and wavefront of tests/test_gpu_pathtrace_lights.py ------------------------------------------------
def synthetic_lights():
    """Three lights above ``pathtrace_ref.SYNTH_SCENE`` (balls of radius 0.25 .. 0.33 around the origin): one overhead, one to the
    side, and one only 0.45 above the floor, which throws long shadows over the floor vertices."""
    return make_lights([(0.0, 2.5, 0.5), (-1.5, 1.2, 1.0), (1.4, 0.45, 0.9)], [4.0, (3.0, 2.0, 1.0), (0.5, 1.0, 2.0)])


def _near_light_threshold(scene, lights, org, nrm, own, tol=1e-4):
    """Rows whose segment to any of the lights passes within ``tol`` (relative, in the discriminant, as
    ``pathtrace_ref._near_threshold``) of a ball's silhouette, or that see a light within ``tol`` of their horizon."""
    bad = np.zeros(len(org), dtype=bool)
    for P in lights["position"].astype(np.float64):
        v = P[None, :] - org
        d = v / np.linalg.norm(v, axis=1, keepdims=True)
        bad |= np.abs(R._dot(d, nrm)) < tol
        for k, (c, r) in enumerate(scene["spheres"]):
            oc = org - np.asarray(c, dtype=np.float64)[None, :]
            perp = oc - R._dot(oc, d)[:, None] * d
            bad |= (own != k) & (np.abs(r * r - R._dot(perp, perp)) < tol * r * r)
    return bad


def synthetic_lit_vertices(n: int = 4096, seed: int = 7, scene: dict = R.SYNTH_SCENE, lights: dict = None):
    """``pathtrace_ref.synthetic_vertices`` with every vertex moved whose segment to one of ``lights`` grazes a silhouette (or
    its own horizon) to within 1e-4; a moved vertex draws new directions too, until those graze nothing either."""
    lights = synthetic_lights() if lights is None else lights
    v = R.synthetic_vertices(n, seed, scene)
    g = np.random.default_rng(seed + 1000)
    n_b, mat = len(scene["spheres"]), v["material"]
    ball, live = mat < n_b, mat <= n_b
    cs = np.asarray([c for c, _ in scene["spheres"]], dtype=np.float64)[np.minimum(mat, n_b - 1)]
    rs = np.asarray([r for _, r in scene["spheres"]], dtype=np.float64)[np.minimum(mat, n_b - 1)]
    org, nrm, wl, wo = (v[k].astype(np.float64) for k in ("org", "nrm", "wl", "wo"))
    redo = np.zeros(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        for _ in range(32):
            grazes = R._near_threshold(scene, org, nrm, mat, wl) | R._near_threshold(scene, org, nrm, mat, wo)
            redo = live & (_near_light_threshold(scene, lights, org, nrm, mat) | (redo & grazes))
            if not redo.any():
                break
            nn = np.where(ball[:, None], R._sphere_dirs(g, n), np.array([0.0, 1.0, 0.0]))
            nn = np.where(ball[:, None] & (cs[:, 1:2] + rs[:, None] * nn[:, 1:2] < 0.02), nn * [1, -1, 1], nn)
            oo = np.where(ball[:, None], cs + rs[:, None] * nn, np.stack([g.uniform(-1.5, 1.5, n), np.zeros(n), g.uniform(-1.5, 1.5, n)], 1))
            f32 = lambda a: a.astype(F).astype(np.float64)
            nrm, org = np.where(redo[:, None], f32(nn), nrm), np.where(redo[:, None], f32(oo), org)
            wl = np.where(redo[:, None], f32(R._cosine_dirs(g, n)), wl)
            wo = np.where(redo[:, None], f32(np.abs(R._sphere_dirs(g, n))), wo)
        else:
            raise RuntimeError("could not move the synthetic vertices off the silhouettes")
    v.update(org=org.astype(F), nrm=nrm.astype(F), wl=wl.astype(F), wo=wo.astype(F))
    return v
