"""A recorder and a reference for WHOLE passes of ``PathArrayRenderer`` (bsdf_diffusion_sampling_amd/pathtrace.py).

Test infrastructure only.  The kernel tests hold every path kernel to its numpy restatement on one synthetic wavefront; what
strings the kernels together — ``render_pass`` — is held here:

``Recorder``        wraps the stage methods of ONE renderer instance (``primary``, ``path_begin``, ``sample_emitter``,
                    ``sample_env``, ``table.bucket``, ``table.sample_pdf``, ``measured_table.eval_t``, ``bounce``, ``resolve``) and
                    keeps, per call, the stage's name, its scalar arguments and CPU copies of the buffer dict before and after.
                    It calls no product code of its own.
``reference_pass``  the pass as the module docstring of pathtrace.py describes it, as a plain loop over the references of the
                    stages (oracle/wavefront_oracle.py ``primary``, tests/pathtrace_ref.py, tests/pathtrace_lights_ref.py,
                    tests/envmap_ref.py, tests/bounce_ref.py), fp64 by default, fp32 on request.  The sampler and the evaluator are inputs
                    (``answers``), exactly as in the kernel tests.
``reference_mesh_pass``  the same for ``mesh.MeshPathArrayRenderer``, from its class docstring: the camera rays of the oracle, the
                    hits of tests/mesh_ref.py, the vertices of ``mesh_ref.primary_arrays``, the stages of tests/mesh_bounce_ref.py,
                    with ``prim`` in the state.  The ``Recorder`` serves that renderer as it is: it wraps whatever the instance's
                    class defines, and snapshots every tensor of the buffer dict, ``prim`` among them.
"""
from __future__ import annotations

import math

import numpy as np

import bounce_ref as B
import envmap_ref as ER
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from oracle import wavefront_oracle as WO

F = np.float32
M64 = R.M64
STATE = ("org", "nrm", "wi", "wl", "material", "beta", "rad")
ANSWER = ("wo", "pdf_o", "pdf_l", "f_o", "f_l")


def sampler_key(seed: int, pass_idx: int, bounce: int) -> int:
    """The key ``table.sample_pdf`` draws bounce ``bounce`` of a pass with, from the class docstring of ``PathArrayRenderer``:
    bounce 0 uses ``ArrayRenderer.render_pass``'s key, bounce k > 0 that key ^ (k * 0xD1B54A32D192ED03)."""
    skey = (seed * 0x9E3779B97F4A7C15 + pass_idx + 1) & M64
    return skey if bounce == 0 else skey ^ ((bounce * 0xD1B54A32D192ED03) & M64)


def scene_dict(camera, centers, radii, checker=(0.4, 0.2, 2.0), albedo=(1.0, 1.0, 1.0), floor=True) -> dict:
    """The oracle's scene dict (camera, balls, floor) of what ``ArrayRenderer(table, centers, radii, camera, checker=, albedo=)``
    renders — from the arguments alone, no device."""
    rt, up, fw = camera.basis()
    d = dict(origin=[float(v) for v in camera.origin], right=rt, up=up, forward=fw,
             tan_half_fov=math.tan(math.radians(camera.fov_deg) * 0.5), width=int(camera.width), height=int(camera.height),
             albedo=[float(v) for v in albedo], spheres=[([float(v) for v in c], float(r)) for c, r in zip(centers, radii)])
    if floor:
        d["plane"] = dict(y=0.0, c0=float(checker[0]), c1=float(checker[1]), scale=float(checker[2]))
    return d


def scene_of(r) -> dict:
    """The oracle's scene dict of a renderer, read from its ``bsdfd_wf_scene`` (the fp32 numbers the kernels see)."""
    sc = r.scene
    spheres = [(list(sc.sphere_center), sc.sphere_radius)]
    spheres += [(list(sc.extra_spheres[k])[:3], sc.extra_spheres[k][3]) for k in range(sc.n_extra_spheres)]
    d = dict(origin=list(sc.cam_origin), right=list(sc.cam_right), up=list(sc.cam_up), forward=list(sc.cam_forward),
             tan_half_fov=sc.tan_half_fov, width=sc.width, height=sc.height, albedo=list(sc.albedo), spheres=spheres)
    if sc.has_plane:
        d["plane"] = dict(y=sc.plane_y, c0=sc.checker_color0, c1=sc.checker_color1, scale=sc.checker_scale)
    return d


# ---- the recorder --------------------------------------------------------------------------------------------------------------
class Recorder:
    """``with Recorder(r) as rec: r.render_pass(...)`` -> ``rec.stages``: one dict per stage call, in call order:
    ``name``, ``args`` (the scalars), ``before`` / ``after`` ({array name: numpy copy} of the buffer dict; ``before`` is None for
    ``primary``, which is where the dict comes from), for ``bucket`` also ``counts`` and ``perm``, for ``resolve`` also
    ``film_before`` / ``film_after``.  The ids are called ``mat`` as in the renderer's dict.  A stage on the dict that was called
    with keywords beyond its documented scalars (``lights=``, ``rows=``, ``env_dist=``, ``rr_depth=``) hands them on and keeps
    them as ``extra``; ``render_pass`` passes ``rows=`` with ``compact=True`` and nothing otherwise: its stages then have no
    such entry."""

    def __init__(self, r):
        self.r, self.stages, self.b, self._wrapped = r, [], None, []

    def _snap(self, **replace):
        import torch
        out = {}
        for k, v in dict(self.b, **replace).items():
            if isinstance(v, torch.Tensor):
                out[k] = v.detach().cpu().numpy().copy()
        return out

    def _wrap(self, owner, name, make):
        inner = getattr(owner, name)
        setattr(owner, name, make(inner))
        self._wrapped.append((owner, name))

    def _effective_occlusion(self, value):
        return self.r.occlusion if value is None else bool(value)

    def __enter__(self):
        r, rec = self.r, self

        def primary(inner):
            def f(row_begin, row_end, spp, seed, pass_idx, out=None):
                b = inner(row_begin, row_end, spp, seed, pass_idx, out)
                rec.b = b
                rec.stages.append(dict(name="primary", args=dict(row_begin=row_begin, row_end=row_end, spp=spp, seed=seed,
                                                                 pass_idx=pass_idx), before=None, after=rec._snap()))
                return b
            return f

        def on_dict(name, keys):
            def make(inner):
                def f(b, *a, **kw):
                    assert b is rec.b, f"{name} was handed another buffer dict than primary returned"
                    args = dict(zip(keys, a))
                    args.update({k: v for k, v in kw.items() if k in keys})
                    if "occlusion" in keys:
                        args["occlusion"] = rec._effective_occlusion(args.get("occlusion"))
                    before = rec._snap()
                    out = inner(b, *a, **kw)
                    stage = dict(name=name, args=args, before=before, after=rec._snap())
                    extra = {k: v for k, v in kw.items() if k not in keys}
                    if extra:          # keywords beyond the documented scalars (lights=, rows=, env_dist=, rr_depth=): handed on, and kept
                        stage["extra"] = extra
                    rec.stages.append(stage)
                    return out
                return f
            return make

        def bucket(inner):
            def f(material_id, extra_bins=0):
                before = rec._snap()
                plan = inner(material_id, extra_bins)
                rec.stages.append(dict(name="bucket", args=dict(extra_bins=extra_bins, ids_are_state=material_id is rec.b["mat"]),
                                       before=before, after=rec._snap(), counts=list(plan[1]), perm=plan[0].cpu().numpy().copy()))
                return plan
            return f

        def sample_pdf(inner):
            def f(plan, wi, wl, **kw):
                before = rec._snap()
                outs = inner(plan, wi, wl, **kw)
                args = {k: kw.get(k) for k in ("seed", "offset", "direct")}
                args.update(wi_is_state=wi is rec.b["wi"], wl_is_state=wl is rec.b["wl"], counts=list(plan[1]))
                rec.stages.append(dict(name="sample_pdf", args=args, before=before,
                                       after=rec._snap(wo=outs[0], pdf_o=outs[1], pdf_l=outs[2])))
                return outs
            return f

        def eval_t(inner):
            def f(material_id, wi, wo, wl=None, tint=None, out_o=None, out_l=None):
                before = rec._snap()
                out = inner(material_id, wi, wo, wl, tint=tint, out_o=out_o, out_l=out_l)
                b = rec.b
                args = dict(tint=None if tint is None else [float(v) for v in tint.tolist()],
                            reads_state=material_id is b["mat"] and wi is b["wi"] and wo is b["wo"] and wl is b["wl"],
                            writes_state=out_o is b.get("f_o") and out_l is b.get("f_l"))
                rec.stages.append(dict(name="eval_t", args=args, before=before, after=rec._snap()))
                return out
            return f

        def resolve(inner):
            def f(row_begin, row_end, spp, b, film):
                assert b is rec.b, "resolve was handed another buffer dict than primary returned"
                before, film_before = rec._snap(), film.detach().cpu().numpy().copy()
                out = inner(row_begin, row_end, spp, b, film)
                rec.stages.append(dict(name="resolve", args=dict(row_begin=row_begin, row_end=row_end, spp=spp), before=before,
                                       after=rec._snap(), film_before=film_before, film_after=film.detach().cpu().numpy().copy()))
                return out
            return f

        self._wrap(r, "primary", primary)
        self._wrap(r, "path_begin", on_dict("path_begin", ()))
        self._wrap(r, "sample_emitter", on_dict("sample_emitter", ("bounce", "seed", "pass_idx", "path_offset", "occlusion")))
        self._wrap(r, "sample_env", on_dict("sample_env", ("bounce", "seed", "pass_idx", "path_offset", "occlusion")))
        self._wrap(r, "bounce", on_dict("bounce", ("bounce", "last", "seed", "pass_idx", "path_offset", "occlusion")))
        self._wrap(r, "resolve", resolve)
        self._wrap(r.table, "bucket", bucket)
        self._wrap(r.table, "sample_pdf", sample_pdf)
        if getattr(r, "measured_table", None) is not None:
            self._wrap(r.measured_table, "eval_t", eval_t)
        return self

    def __exit__(self, *exc):
        for owner, name in self._wrapped:
            delattr(owner, name)        # the instance attribute goes, the class's method is back
        self._wrapped = []
        return False

    def named(self, name):
        return [s for s in self.stages if s["name"] == name]


# ---- the reference pass --------------------------------------------------------------------------------------------------------
def mock_answers(seed: int):
    """A stand-in for the sampler, for the runs that compare the reference with itself: per bounce ``wo`` cosine-distributed with
    10 % of the draws below the surface, ``pdf_o`` = |wo.z| / pi times a log-uniform factor in [0.1, 10], ``pdf_l`` = wl.z / pi of
    the vertex's own light direction.  The draws depend on (seed, bounce) alone: two precisions get the same ones."""
    def answer(k, st):
        n = len(st["material"])
        g = np.random.default_rng([seed, k])
        wo = R._cosine_dirs(g, n)
        wo[g.random(n) < 0.1, 2] *= -1.0
        pdf_o = np.abs(wo[:, 2]) / np.pi * np.exp(g.uniform(np.log(0.1), np.log(10.0), n))
        pdf_l = np.nan_to_num(st["wl"].astype(F)[:, 2].astype(np.float64)) / np.pi
        return dict(wo=wo.astype(F), pdf_o=pdf_o.astype(F), pdf_l=pdf_l.astype(F))
    return answer


def bounce_mode(mode: str, lights) -> str:
    """The mode of ``bounce_ref.bounce`` a renderer in ``mode`` ("cosine" / "importance") with or without ``lights`` calls."""
    return "env" if mode == "importance" else "cosine" if lights is None else "lit"


def reference_pass(scene: dict, env, mode: str, lights, tables, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int,
                   max_depth, occlusion: bool, answers, dtype=np.float64, rr_depth=None, depth_cap: int = 1024, scale=True):
    """One pass of ``PathArrayRenderer`` over rows [row_begin, row_end), written from the module docstring of pathtrace.py:

        primary -> path_begin
        per bounce k:  [sample_emitter(k)] [sample_env(k)] -> the sampler's and the evaluator's answers -> bounce(k, last)
        resolve

    ``mode``: "cosine" or "importance" (then ``tables`` = ``envmap_ref.build_tables(env)``); ``lights``: None or the dict of
    ``pathtrace_lights_ref.make_lights``; ``env`` None (with lights only): black, and no emitter.  ``answers``: a sequence of
    dicts ``wo, pdf_o, pdf_l[, f_o, f_l]`` per bounce (rows in path order), or ``f(k, state)`` that returns one; a sequence that
    runs out ends the loop (the device's pass was shorter: its rows then differ in their histories).  ``rr_depth``: Russian
    roulette in every bounce (``scale`` as in ``bounce_ref.bounce``), and only then may ``max_depth`` be None, the unbounded loop:
    it runs until no lane is live, ``depth_cap`` bounces at the most (the bounce at the cap is ``last``).
    -> dict(stages: [(name, bounce, state dict)] after every stage, history: [``decision_code`` after primary and after every
    bounce], rad [N,3], film [rows, width, 3]: the tile the pass adds, depth: bounces run, depth_cap_hit)."""
    assert mode in ("cosine", "importance")
    assert max_depth is not None or rr_depth is not None
    has_env = env is not None
    assert has_env or lights is not None
    env = np.zeros((2, 4, 3), F) if env is None else np.asarray(env, dtype=F)
    n_b, width = len(scene["spheres"]), scene["width"]
    n_l = 0 if lights is None else len(lights["position"])
    n_e = n_l + int(has_env)
    offset = row_begin * width * spp
    wi, wl, nrm, dir_, mat = WO.primary(scene, row_begin, row_end, spp, seed, pass_idx, with_material=True)
    n = len(mat)
    st = dict(wi=wi, wl=wl, nrm=nrm, material=mat)
    stages = [("primary", None, dict(st, dir=dir_))]
    org, beta, rad = R.path_begin(scene, env, dir_, nrm, mat, dtype=dtype)
    st = {k: (v if k == "material" else np.asarray(v).astype(dtype)) for k, v in dict(st, org=org, beta=beta, rad=rad).items()}
    stages.append(("path_begin", None, dict(st)))
    history = [decision_code(scene, mat, wi)]
    depth = depth_cap if max_depth is None else max_depth
    ran = 0
    for k in range(depth):
        live = (st["material"] >= 0) & (st["material"] <= n_b)
        if not live.any() or (not callable(answers) and k >= len(answers)):
            break
        vertex = [st[name] for name in ("org", "nrm", "wi", "material")]
        if lights is not None:
            s = LR.sample_emitter(scene, lights, has_env, k, occlusion, seed, pass_idx, offset, *vertex, st["wl"], dtype=dtype)
            st.update(wl=s["wl"].astype(dtype), lsel=s["lsel"], emit=s["emit"].astype(dtype), lit_point=s["lit"])
            stages.append(("sample_emitter", k, dict(st)))
        if mode == "importance":
            s = ER.sample_env(scene, env, tables, n_e, k, occlusion, seed, pass_idx, offset, *vertex, st.get("lsel"), st["wl"],
                              dtype=dtype)
            picked = s["picked"]
            st.update(wl=s["wl"].astype(dtype), lpdf=np.where(picked, s["lpdf"], 0).astype(dtype), lit_env=s["lit"],
                      emit=np.where(picked[:, None], s["emit"], st.get("emit", np.zeros((n, 3)))).astype(dtype))
            stages.append(("sample_env", k, dict(st)))
        a = answers(k, st) if callable(answers) else answers[k]
        out = B.bounce(scene, env, bounce_mode(mode, lights), k, k == depth - 1, occlusion, seed, pass_idx, offset,
                       *[st[name] for name in STATE], a["wo"], a["pdf_o"], a["pdf_l"], a.get("f_o"), a.get("f_l"), n_e=n_e,
                       has_env=has_env, lsel=st.get("lsel"), emit=st.get("emit"), lpdf=st.get("lpdf"), tables=tables,
                       rr_depth=rr_depth, scale=scale, dtype=dtype)
        st.update({name: (out[name] if name == "material" else out[name].astype(dtype)) for name in STATE})
        rr = {} if rr_depth is None else {name: out[name] for name in ("cos_in", "killed", "survive", "q")}
        stages.append(("bounce", k, dict(st, **rr)))
        history.append(decision_code(scene, st["material"], st["wi"]))
        ran = k + 1
    film = R.resolve(st["rad"], spp).reshape(row_end - row_begin, width, 3)
    return dict(stages=stages, history=history, rad=st["rad"], film=film, depth=ran, depth_cap_hit=max_depth is None and ran == depth)


def decision_code(scene: dict, material, wi):
    """What a vertex decided, as one integer per row: 2 * material id, plus 1 on a floor vertex of the checker's second colour.

    The id alone is not the whole decision.  A path that leaves a ball almost parallel to the floor lands 1e2 .. 1e3 away (real
    passes have such rows; the synthetic wavefront of the kernel tests redraws every ray that flies further than 50), where an
    fp32 position is uncertain by more than a checker cell: the colour the floor vertex reads — the 0.4 or the 0.2 in its ``wi``
    slot — is then a coin flip of the rounding, exactly like a hit at a silhouette.  It is counted with the ids, under the same
    cap."""
    material = np.asarray(material)
    plane = scene.get("plane")
    if plane is None:
        return material * 2
    w0 = np.nan_to_num(np.asarray(wi)[:, 0].astype(np.float64))
    odd = (material == len(scene["spheres"])) & (np.abs(w0 - F(plane["c1"])) < np.abs(w0 - F(plane["c0"])))
    return material * 2 + odd


def ids_of(code):
    return np.asarray(code) >> 1


def histories_differ(a, b):
    """Paths [N] whose decision histories (lists of ``decision_code`` arrays; a pass that stopped early repeats its last entry)
    differ."""
    m = max(len(a), len(b))
    pad = lambda h: list(h) + [h[-1]] * (m - len(h))
    return np.any([x != y for x, y in zip(pad(a), pad(b))], axis=0)


# ---- the kernels' stated capacity: WF_MAX_SPHERES = 32 balls, BSDFD_WF_MAX_LIGHTS = 8 lights ---------------------------------------
def capacity_scene() -> dict:
    """32 balls on a 4 x 8 grid — ball (j, i) at (-2.45 + 0.7 i, r, -1.05 + 0.7 j) with r = 0.2 + 0.13 ((3 i + 5 j) % 7) / 6, resting on
    the floor — over the plane, albedo and origin of ``pathtrace_ref.SYNTH_SCENE``.  Ids then run to 33 ("miss" = n_balls + 1)."""
    spheres = []
    for j in range(4):
        for i in range(8):
            r = 0.2 + 0.13 * ((3 * i + 5 * j) % 7) / 6
            spheres.append(((-2.45 + 0.7 * i, r, -1.05 + 0.7 * j), r))
    return dict(R.SYNTH_SCENE, spheres=spheres)


def capacity_lights() -> dict:
    """Eight lights over ``capacity_scene``: overhead, to the sides, low between the balls; one dim, one of intensity 0."""
    return LR.make_lights([(0.0, 2.5, 0.5), (-1.5, 1.2, 1.0), (1.4, 0.45, 0.9), (2.6, 0.9, -1.3), (-2.7, 0.6, 0.2), (0.3, 0.75, 0.33),
                           (-0.9, 3.0, -2.0), (1.0, 1.6, 1.9)],
                          [4.0, (3.0, 2.0, 1.0), (0.5, 1.0, 2.0), 1.0, 2.0, (0.2, 0.3, 0.1), 6.0, 0.0])


# ---- the pass on meshes: mesh.MeshPathArrayRenderer ---------------------------------------------------------------------------------
MESH_STATE = ("org", "nrm", "wi", "wl", "material", "prim", "beta", "rad")


def camera_scene(camera) -> dict:
    """The oracle's scene dict of a camera alone (one placeholder ball, which no mesh pass intersects): what
    ``wavefront_oracle.primary`` needs for ``dir`` and ``wl``."""
    return scene_dict(camera, [(0.0, 0.0, 0.0)], [1.0], floor=False)


def mesh_decision_code(geom: dict, material, prim, wi):
    """What a vertex on a mesh decided, as one integer per row: the material id, for a diffuse or checker vertex which of its
    instance's two reflectances sits in the ``wi`` slot (bit 40: the second colour of a checker; a plain diffuse instance has one),
    and both components of ``prim`` (bits 24 .. 39: instance + 1, bits 0 .. 23: triangle + 1) — on meshes the primitive is part of
    the decision, because the next ray skips it.  An ended row (id above ``n_materials``) keeps the ``prim`` it had; that is no
    decision of the stage that ended it (the byte comparisons hold it), and the code carries 0 there."""
    material, prim = np.asarray(material).astype(np.int64), np.asarray(prim).astype(np.int64)
    n_b = geom["n_materials"]
    live = (material >= 0) & (material <= n_b)
    c0 = np.array([i.checker[0] if i.checker is not None else i.diffuse if i.diffuse is not None else 0.0 for i in geom["instances"]])
    c1 = np.array([i.checker[1] if i.checker is not None else i.diffuse if i.diffuse is not None else 0.0 for i in geom["instances"]])
    k = np.clip(prim[:, 0], 0, len(c0) - 1)
    w0 = np.nan_to_num(np.asarray(wi)[:, 0].astype(np.float64))
    odd = live & (material == n_b) & (np.abs(w0 - F(c1[k])) < np.abs(w0 - F(c0[k])))
    assert prim.max(initial=0) < (1 << 24) - 1 and len(c0) < (1 << 16) - 1
    where = np.where(live, ((prim[:, 0] + 1) << 24) | (prim[:, 1] + 1), 0)
    return ((material * 2 + odd) << 40) | where


def mesh_ids_of(code):
    return np.asarray(code) >> 41


def _no_rays(meshes, instances, org, dir, tmax=None, skip=None):
    """A hit source that hits nothing (for a run of the bounce of which only the roulette's ``q`` is read)."""
    import mesh_ref as MR
    return MR._result(len(org))


def too_close_to_call(want: dict, q_other):
    """Rows [N] of a bounce with roulette (``want``: ``mesh_bounce_ref.bounce``'s dict) whose decision another precision may make
    differently — the rule of test_mesh_bounce_matches_reference: the path would continue and its variate is no farther from ``q``
    than the largest distance, over the rows that would continue, between ``q`` and the other precision's ``q_other``.
    -> (rows, that distance)."""
    would = want["would"]
    with np.errstate(invalid="ignore"):
        eq = np.abs(np.asarray(q_other, dtype=np.float64) - want["q"].astype(np.float64))[would].max(initial=0.0)
        near = ~(np.abs(want["u"].astype(np.float64) - want["q"].astype(np.float64)) > eq)
    return would & near, float(eq)


def reference_mesh_pass(geom: dict, camera_scene: dict, env, lights, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int,
                        max_depth, occlusion: bool, answers, dtype=np.float64, rr_depth=None, depth_cap: int = 1024, cast=None):
    """One pass of ``mesh.MeshPathArrayRenderer`` over rows [row_begin, row_end), written from its class docstring and the module
    docstring of pathtrace.py:

        primary: the camera rays, their closest hits, the first vertex (org, prim, beta = 1, rad = env for a miss); path_begin: nothing
        per bounce k:  [sample_emitter(k)] -> the sampler's and the evaluator's answers -> bounce(k, last)
        resolve

    ``geom``: mesh_bounce_ref's geometry dict; ``camera_scene``: the oracle's scene dict of the camera (``camera_scene(cam)`` or
    ``scene_of(renderer)``), of which ``wavefront_oracle.primary`` gives ``dir`` and ``wl`` — ``bsdfd_wf_primary``'s bits, which
    ``bsdfd_mesh_primary`` is tested to reproduce.  The first vertex is the hit from the camera's origin and
    ``mesh_ref.primary_arrays``; ``org = o + t d``, ``prim`` the hit or (-1, -1).  ``env`` None (with ``lights`` only): black, and no
    emitter.  ``answers``, ``rr_depth``, ``max_depth`` None and ``depth_cap``: as in ``reference_pass``.  ``cast``: the hit source
    in place of ``mesh_ref.brute_force`` (mesh_bounce_ref.cast_rays), for the camera rays too.
    -> what ``reference_pass`` returns (stages, history: ``mesh_decision_code`` after primary and after every bounce, rad, film,
    depth, depth_cap_hit) and, per path [N], the union over all rays the path cast — camera, continuation and shadow rays — of
    ``marginal``, of ``fragile`` (next vertices the path went on to), and with roulette of ``close``: decisions too close to call
    (``too_close_to_call`` against the other one of fp32 / fp64)."""
    import mesh_bounce_ref as MB
    import mesh_ref as MR
    assert max_depth is not None or rr_depth is not None
    has_env = env is not None
    assert has_env or lights is not None
    env = np.zeros((2, 4, 3), F) if env is None else np.asarray(env, dtype=F)
    meshes, instances, n_b = geom["meshes"], geom["instances"], geom["n_materials"]
    width = camera_scene["width"]
    n_l = 0 if lights is None else len(lights["position"])
    n_e = n_l + int(has_env)
    mode = "cosine" if lights is None else "lit"
    offset = row_begin * width * spp
    _, wl, _, dir_ = WO.primary(camera_scene, row_begin, row_end, spp, seed, pass_idx)
    n = len(dir_)
    o = np.tile(np.asarray(camera_scene["origin"], dtype=F).astype(np.float64), (n, 1))
    d64 = dir_.astype(np.float64)
    hit = (cast or MR.brute_force)(meshes, instances, o, d64)
    is_hit = hit["prim"][:, 0] >= 0
    v = MR.primary_arrays(meshes, instances, n_b, d64, hit)
    org = np.where(is_hit[:, None], o + np.where(is_hit, hit["t"], 0.0)[:, None] * d64, 0.0)
    rad = np.where(is_hit[:, None], 0.0, WO.env_lookup(env.astype(np.float64), dir_).astype(np.float64))
    st = dict(org=org, nrm=v["nrm"], wi=v["wi"], wl=wl, beta=np.ones((n, 3)), rad=rad)
    st = {k: a.astype(dtype) for k, a in st.items()}
    st.update(material=v["material"].astype(np.int64), prim=hit["prim"].astype(np.int64))
    marginal, fragile, close = hit["marginal"].copy(), v["fragile"] & is_hit, np.zeros(n, dtype=bool)
    code = lambda s: mesh_decision_code(geom, s["material"], s["prim"], s["wi"])
    stages = [("primary", None, dict(st, dir=dir_, hit=hit)), ("path_begin", None, dict(st))]
    history = [code(st)]
    depth = depth_cap if max_depth is None else max_depth
    other = np.float32 if np.dtype(dtype) == np.float64 else np.float64
    ran = 0
    for k in range(depth):
        live = (st["material"] >= 0) & (st["material"] <= n_b)
        if not live.any() or (not callable(answers) and k >= len(answers)):
            break
        if lights is not None:
            s = MB.sample_emitter(geom, lights, has_env, k, occlusion, seed, pass_idx, offset,
                                  *[st[name] for name in ("org", "nrm", "wi", "material", "prim", "wl")], dtype=dtype, cast=cast)
            st.update(wl=s["wl"].astype(dtype), lsel=s["lsel"], emit=s["emit"].astype(dtype), lit_point=s["lit"])
            marginal |= s["shadow"]["marginal"]
            stages.append(("sample_emitter", k, dict(st)))
        a = answers(k, st) if callable(answers) else answers[k]
        args = (geom, env, mode, k, k == depth - 1, occlusion, seed, pass_idx, offset, *[st[name] for name in MESH_STATE],
                a["wo"], a["pdf_o"], a["pdf_l"], a.get("f_o"), a.get("f_l"))
        kw = dict(n_e=n_e, has_env=has_env, lsel=st.get("lsel"), emit=st.get("emit"), rr_depth=rr_depth)
        out = MB.bounce(*args, dtype=dtype, cast=cast, **kw)
        marginal |= out["hit"]["marginal"] | out["shadow"]["marginal"]
        rr = {}
        if rr_depth is not None:
            rr = {name: out[name] for name in ("u", "q", "survive", "killed", "would")}
            if k != depth - 1 and k + 1 >= rr_depth:
                # (q is formed of beta and the vertex' throughput alone: the other precision's needs no ray)
                near, _ = too_close_to_call(out, MB.bounce(*args, dtype=other, cast=_no_rays, **kw)["q"])
                close |= near
        st.update({name: (out[name] if name in ("material", "prim") else out[name].astype(dtype)) for name in MESH_STATE})
        fragile |= out["fragile"] & (st["material"] <= n_b)
        stages.append(("bounce", k, dict(st, **rr)))
        history.append(code(st))
        ran = k + 1
    film = R.resolve(st["rad"], spp).reshape(row_end - row_begin, width, 3)
    return dict(stages=stages, history=history, rad=st["rad"], film=film, depth=ran, depth_cap_hit=max_depth is None and ran == depth,
                marginal=marginal, fragile=fragile, close=close)
