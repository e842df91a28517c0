"""Path tracer for the array scene: occlusion, further bounces (csrc/pathtrace.hip, C ABI ``bsdfd_wf_path_begin`` /
``bsdfd_wf_resolve``), point emitters (csrc/pathlights.hip, ``bsdfd_wf_sample_emitter``), importance sampling of the
environment map (csrc/pathenv.hip, ``bsdfd_wf_sample_env``; the distribution: ``envmap.EnvDistribution``), and the bounce
for each of them, with Russian roulette for unbounded depth (csrc/bounce.hip, ``bsdfd_wf_bounce`` / ``_lit`` / ``_env`` /
``_rr``).

The reference renders its 12-ball array scenes with Mitsuba's ``path`` integrator at unbounded depth
(matpreview/disney_bsdf_array*_envmap.xml, scene_measured.xml: ``max_depth = -1``): balls shadow the floor and each
other, light reflected by one measured material lands on the next, and every further vertex calls the plugin's
``sample()`` / ``pdf()`` again.  ``ArrayRenderer`` stops after one bounce and traces no secondary ray; this class adds
the loop that feeds a shrinking wavefront through the same pieces bounce after bounce:

    primary -> path_begin (org, beta = 1, rad = env for a miss)
    per bounce k:  table.bucket(mat)            ended paths carry the "miss" id and sort behind the materials
                   table.sample_pdf(plan, ...)  flow evaluations for the lanes that carry a material only
                   ground_truth_table.eval_t(...)   when there is ground truth: a MeasuredTable or an AnalyticTable
                   bounce(k, last = k == max_depth - 1)      [rr_depth: bounce_rr, which also ends paths by roulette]
    resolve -> film tile += mean_spp of rad

The geometry is at most 32 analytic spheres and one plane, intersected by brute force like the primary rays.  Without
``lights`` only the environment emits.  With ``lights`` (up to 8 ``PointLight``, the emitter of the reference's
matpreview/disney_bsdf_array*_pointlight*.xml scenes) every vertex takes one emitter sample, the emitter chosen uniformly
as Mitsuba's ``sample_emitter_direction`` does, and a depth becomes

    sample_emitter(k) -> bucket -> sample_pdf -> eval_t -> bounce_lit(k)

where ``sample_emitter`` puts the direction to a picked point light into ``wl`` — so the sampler's ``pdf()`` and the
evaluator answer for that direction — and what arrives from it (visibility, 1 / d^2, the selection's factor) into ``emit``.
A point light is a delta: its term has no MIS weight.

The light strategy towards the environment is a cosine-weighted hemisphere draw by default.  ``env_sampling="importance"``
draws it in proportion to the map's luminance instead, as the ``envmap`` emitter of the reference's
matpreview/disney_bsdf_array*_envmap.xml and scene_measured.xml does (``sample_direction`` / ``pdf_direction``), and a depth becomes

    [sample_emitter(k)] -> sample_env(k) -> bucket -> sample_pdf -> eval_t -> bounce_env(k)

``sample_env`` overwrites ``wl`` on the ball vertices that picked the environment with a direction drawn from
``envmap.EnvDistribution`` — a piecewise-constant density over the map's own texel grid, built from the 3x3 maximum of the
luminance times the row's solid angle; Mitsuba's is a bilinear ``Hierarchical2D`` over luminance x sin(theta), and this one is
parity-unpinned against it like the evaluator — and leaves its density in ``lpdf`` and radiance x visibility / density in
``emit``; ``bounce_env`` weights both strategies against that density.  The floor keeps its cosine direction as BSDF sample and
way on, so where a path goes does not depend on ``env_sampling``.

A path ends when it escapes, when its BSDF sample is invalid, at ``max_depth``, or — with ``rr_depth=R`` — by Russian
roulette: the reference's six ``max_depth = -1`` scenes set no ``rr_depth``, so Mitsuba's default of 5 applies, and from the fifth
vertex on (``bounce + 1 >= R``) a path that would continue survives with probability ``q = min(max(throughput), 0.95)`` and its
throughput is divided by ``q``.  The decision is made inside the bounce kernel (``bsdfd_wf_bounce_rr`` stands in for whichever of
the three bounce calls the emitters select; one Philox draw of the lane's own per decision, counter word 3 = "Roul" + depth), a
killed path carries the "miss" id like one that escaped, and ``rad`` and the way a survivor goes do not depend on it.  With
roulette ``max_depth=None`` is the reference's unbounded depth: the loop runs until the bucketing finds no live lane, or to
``PathArrayRenderer.DEPTH_CAP`` bounces — a truncation, should it ever be hit (``stats["depth_cap_hit"]``).  This is Mitsuba's
rule restated; like the evaluator it is parity-unpinned against Mitsuba (neither its random stream nor its images are matched).
``integrator_from_matpreview_xml`` reads both settings from a reference scene file.

``compact=True`` runs the bounces behind the first on a live-lane list instead of over all N lanes.  The bucketing sorts ended
paths behind everything else, so the front of its permutation is the list ``L`` of the lanes that were alive; the next depth becomes

    [sample_emitter(k, rows=L)] -> [sample_env(k, rows=L)] -> table.bucket_rows(mat, L)   -> L': "miss" ids dropped
        -> sample_pdf(plan, direct=True, out=(wo, pdf_o, pdf_l)) -> eval_t(..., rows=material prefix of L') -> bounce(k, rows=L')

and ``L'`` is the following depth's ``L`` (``bsdfd_wf_sample_emitter_rows``, ``bsdfd_wf_sample_env_rows``, ``bsdfd_bucket_rows``,
``bsdfd_measured_eval_table_rows`` / ``bsdfd_analytic_eval_table_rows``, ``bsdfd_wf_bounce_rows``).  The state stays in lane order and
a lane's Philox counters are keyed by the lane, never by the thread that serves it, so the film and the path state are those of
``compact=False`` bit for bit; the sampler's answers go into the arrays of bounce 0 with no fill, since ``bounce`` reads them on the
material lanes of its list only.  The host still reads the bucket counts back once per depth.  What it saves:
profiles/pathtrace_compact.json (tools/pathtrace_bench.py --compact).

The ground truth is ``ArrayRenderer``'s: {ball: ``MeasuredBSDF``}, or {ball: ``analytic.Principled`` / ``RoughDielectric``}
(``analytic.ground_truth_for(names)`` for the ``mybsdf idx = N`` balls of matpreview/disney_bsdf_array2_spherical_*.xml), evaluated
on the lane-ordered wavefront by ``measured.MeasuredTable`` or ``analytic.AnalyticTable``; with analytic ground truth on every ball
``ball_albedo`` gives each ball the colour its scene file gives it (``wavefront.albedos_from_matpreview_xml``).  Without occlusion
(``max_depth=1``) the estimator keeps looking the environment up along a BSDF sample below the surface, which the analytic
``f |cos|`` of the transmission lobe weights.  What the table costs a pass: profiles/analytic_table.json
(tools/analytic_table_bench.py).

Under occlusion ``bounce`` drops a BSDF sample with ``wo.z <= 0`` ("blocked by the ball itself"): a glass ball is its reflection lobe
on a black body.  ``transmission=True`` follows such a sample into the ball where the vertex has analytic ground truth and
``f_o / pdf_o`` is positive in some channel (``bsdfd_wf_bounce_transmit`` stands in for every bounce call): the ray enters, or stays
in, the ball it is on, and the next vertex is that ball's far side, ``t = -2 (x - c) . d`` along the ray.  Nothing else is
intersected inside a ball, so the balls must be pairwise disjoint and above the floor plane (checked in fp64 by the constructor).
A vertex keeps the OUTWARD normal, so one reached from inside has ``wi.z < 0``; its light strategy draws above the outward normal —
the directions one transmission can reach —, its shadow ray skips its own ball, and a sample with ``wo.z > 0`` leaves the surface
outward whichever side ``wi`` is on.  The reference's plugin answers for ``cos_theta_i > 0`` only (rendering/bsdf_myresult.py:63), so
the vertices inside are sampled by the analytic models themselves, which sample both sides of the surface: a depth k >= 1 becomes

    bucket -> sample_pdf -> sample_inside(k) -> eval_t -> bounce_transmit(k)            [compact: sample_inside over the material prefix]

where ``sample_inside`` (``AnalyticTable.sample_inside``, ``bsdfd_wf_sample_inside`` / ``_rows``) overwrites ``wo``, ``pdf_o`` and
``pdf_l`` on the lanes with ``wi.z < 0`` with the model's own sample, its density, and its density for ``wl``, at variates of the
lane's own (one Philox draw, counter word 3 = "Insd" + depth); the flow still runs on those lanes and its answers are overwritten.
The camera is outside, so bounce 0 has no such lane.  Limits: the roulette keeps ``eta = 1`` (Mitsuba rescales the throughput by
``eta^2`` before the survival test; here the ``1 / eta^2`` a path carries while inside lowers its survival probability — unbiased,
somewhat more variance); no absorption inside a ball; the balls are solid (the reference's shapes are a shell around a diffuse
interior, on a mesh); inside vertices tint with the ball's albedo like any other vertex; ``WavefrontRenderer`` / ``ArrayRenderer`` are
untouched; like the models, parity-unpinned against Mitsuba.  What it costs: profiles/pathtrace_transmission.json
(tools/pathtrace_bench.py --transmission).

There are no area or spot emitters.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Optional, Sequence

import torch

from . import _lib
from .wavefront import ArrayRenderer

_M64 = 0xFFFFFFFFFFFFFFFF

# a Mitsuba `point` emitter: world position (y up) and radiant intensity, a scalar or an RGB triple
PointLight = namedtuple("PointLight", "position intensity")


def _p(t: Optional[torch.Tensor]):
    """The device pointer of a tensor as a C argument (None stays NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


# What the geometry adds to the two stages that ask it something, ``sample_emitter`` and ``bounce`` (``PathArrayRenderer._geometry``):
# ``prefix`` of the entry points' names; ``one_form``: the family is one full-argument entry point per stage (the bounce: every emitter
# argument and ``rr_depth``) and its ``_rows`` form, for which an empty list is nothing to call — not the spheres' per-mode forms;
# the arguments in ``front`` of the shared list and ``behind`` it; the arrays the bounce has ``written`` besides the path state.
_Geometry = namedtuple("_Geometry", "prefix one_form front behind written")


def wf_lights(lights: Sequence[PointLight], has_env: bool) -> _lib.WfLights:
    """The ``bsdfd_wf_lights`` of 1..8 point lights; ``ValueError`` for anything the kernels should not see."""
    lights = list(lights)
    if not 1 <= len(lights) <= _lib.WF_MAX_LIGHTS:
        raise ValueError(f"1..{_lib.WF_MAX_LIGHTS} point lights, got {len(lights)}")
    out = _lib.WfLights()
    out.n_lights, out.has_env = len(lights), int(bool(has_env))
    for k, (position, intensity) in enumerate(lights):
        pos = [float(v) for v in position]
        rgb = [float(v) for v in intensity] if hasattr(intensity, "__len__") else [float(intensity)] * 3
        if len(pos) != 3 or not all(math.isfinite(v) for v in pos):
            raise ValueError(f"light {k}: the position must be three finite numbers")
        if len(rgb) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in rgb):
            raise ValueError(f"light {k}: the intensity must be finite and non-negative (a scalar or an RGB triple)")
        out.position[k] = (C.c_float * 3)(*pos)
        out.intensity[k] = (C.c_float * 3)(*rgb)
    return out


def lights_from_matpreview_xml(path: str):
    """The ``<emitter type="point">`` elements of a reference scene file (rendering/matpreview/disney_bsdf_array*_pointlight*.xml)
    as ``PointLight``s: the z-up position (x, y, z) becomes (x, z, -y), the mapping ``scene_from_matpreview_xml`` applies to the
    balls; the intensity is a scalar or an RGB triple.  [] for a file without point emitters."""
    import xml.etree.ElementTree as ET
    numbers = lambda text: [float(v) for v in text.replace(",", " ").split()]
    out = []
    for em in ET.parse(path).getroot().iter("emitter"):
        if em.get("type") != "point":
            continue
        pos, inten = (0.0, 0.0, 0.0), 1.0   # Mitsuba's defaults
        for child in em:
            if child.get("name") == "position":
                pos = numbers(child.get("value")) if child.get("value") is not None else \
                    [float(child.get(a, 0.0)) for a in ("x", "y", "z")]
            elif child.get("name") == "intensity":
                v = numbers(child.get("value"))
                inten = v[0] if len(v) == 1 else tuple(v)
        if len(pos) != 3:
            raise ValueError(f"{path}: a point emitter's position needs three numbers")
        out.append(PointLight((pos[0], pos[2], -pos[1]), inten))
    return out


def integrator_from_matpreview_xml(path: str):
    """``(max_depth, rr_depth)`` of the ``<integrator>`` of a reference scene file, as ``PathArrayRenderer`` takes them.  Mitsuba
    counts segments (``maxDepth = 2``: direct illumination) and this renderer counts vertices, so ``maxDepth = 2`` is
    ``max_depth = 1``, and ``-1`` (Mitsuba's default too) is ``None``: unbounded.  ``rrDepth`` is read if present and is otherwise
    Mitsuba's default, 5.  Both spellings of either name are read (``maxDepth`` / ``max_depth``, ``rrDepth`` / ``rr_depth``), and a
    ``$name`` value is looked up among the file's ``<default>`` elements (scene_measured.xml)."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    defaults = {d.get("name"): d.get("value") for d in root.iter("default")}
    found = {}
    for integ in root.iter("integrator"):
        for child in integ.iter("integer"):
            name = {"maxDepth": "max_depth", "rrDepth": "rr_depth"}.get(child.get("name"), child.get("name"))
            if name in ("max_depth", "rr_depth") and name not in found:
                value = child.get("value", "")
                if value.startswith("$"):
                    if value[1:] not in defaults:
                        raise ValueError(f"{path}: {child.get('name')} = {value} has no <default>")
                    value = defaults[value[1:]]
                found[name] = int(value)
    depth, rr = found.get("max_depth", -1), found.get("rr_depth", 5)
    if depth == 0 or depth == 1 or depth < -1:
        raise ValueError(f"{path}: maxDepth = {depth} leaves no surface vertex to shade")
    if rr < 1:
        raise ValueError(f"{path}: rrDepth must be >= 1, got {rr}")
    return (None if depth == -1 else depth - 1), rr


def _array_arguments(args, kwargs):
    """(floor, ground_truth, fused_ground_truth) of ``ArrayRenderer``'s arguments behind ``env``, given by position or by name."""
    names = ("floor", "checker", "albedo", "ground_truth", "device", "fused_ground_truth")
    given = dict(zip(names, args), **kwargs)
    return given.get("floor", True), given.get("ground_truth"), given.get("fused_ground_truth", True)


def _check_transmission(centers, radii, deep, occlusion, floor, ground_truth, fused_ground_truth, plane_y: float = 0.0):
    """What ``transmission=True`` needs, before any device work: analytic ground truth behind an ``AnalyticTable`` (the inside
    vertices' sampler), further bounces with occlusion (the rule it changes), and — the ray inside a ball tests nothing else —
    balls that are pairwise disjoint and above the floor plane, checked in fp64."""
    from .analytic import FullSphereGroundTruth
    ground_truth = dict(ground_truth or {})
    if not ground_truth:
        raise ValueError("transmission needs ground truth: without f nothing transmits (ground_truth=analytic.ground_truth_for(...))")
    if not all(isinstance(g, FullSphereGroundTruth) for g in ground_truth.values()) or not fused_ground_truth:
        raise ValueError("transmission needs analytic ground truth behind an AnalyticTable (Principled / RoughDielectric objects, "
                         "fused_ground_truth=True): its models sample the vertices inside a ball")
    if not deep:
        raise ValueError("transmission needs max_depth > 1: with one vertex no path gets inside a ball")
    if not occlusion:
        raise ValueError("transmission needs occlusion: it follows the samples occlusion would drop")
    c = [[float(v) for v in ck] for ck in centers]
    r = [float(v) for v in radii]
    for i in range(len(c)):
        if floor and not c[i][1] - r[i] >= plane_y:
            raise ValueError(f"transmission: ball {i} reaches below the floor plane (the ray inside a ball intersects nothing else)")
        for j in range(i):
            if not math.dist(c[i], c[j]) > r[i] + r[j]:
                raise ValueError(f"transmission: balls {j} and {i} touch or intersect (the ray inside a ball intersects nothing else)")


class PathArrayRenderer(ArrayRenderer):
    """``ArrayRenderer`` with ``max_depth`` vertices per path and, with ``occlusion``, shadow rays.

    ``max_depth=1, occlusion=False`` (the defaults) is ``ArrayRenderer``'s estimator through the path kernels.
    ``occlusion=None`` means ``max_depth > 1``: a deeper path must know what its BSDF sample hit, so ``max_depth > 1`` with
    ``occlusion=False`` is refused (it would count the environment through the balls at every depth).
    Bounce 0 draws with ``ArrayRenderer.render_pass``'s sampler key; bounce k > 0 with ``key ^ (k * 0xD1B54A32D192ED03)``.
    ``stats["lanes_per_bounce"]``: the material lanes served at each bounce of the last pass — the compaction is the
    bucketing itself, no mask machinery.

    ``lights``: up to 8 ``PointLight``.  None or [] is the renderer without the argument, bit for bit.  With lights and
    ``env=None`` the environment is black and is no emitter (camera misses are 0); with an explicit ``env`` both emit.

    ``env_sampling``: ``"cosine"`` (the default: the renderer without the argument, bit for bit) or ``"importance"``, which
    samples the environment in proportion to its luminance (``envmap.EnvDistribution``, built once here).  ``"importance"``
    needs an emitting environment: with lights and ``env=None`` it is refused.

    ``rr_depth``: None (the default: the renderer without the argument, bit for bit; ``bsdfd_wf_bounce_rr`` is never called) or an
    integer >= 1: Russian roulette from the vertex ``bounce + 1 >= rr_depth`` on (Mitsuba's default is 5).  ``max_depth=None``
    is unbounded depth; it needs ``rr_depth`` and implies occlusion.  A pass then ends when no live lane is left, or after
    ``DEPTH_CAP`` bounces (the bounce at the cap gets ``last=True``: a truncation, reported in ``stats["depth_cap_hit"]``).
    ``stats["depth"]``: the bounces the last pass ran.

    ``compact``: False (the default: the renderer without the argument, call for call) or True: from bounce 1 on every per-depth
    kernel runs over the live-lane list the previous bounce's bucketing produced, not over all N lanes.  Same film, same path
    state, bit for bit.  ``stats["list_per_bounce"]``: the lanes the bucketing of each bounce read (N at bounce 0; with
    ``compact=False`` N at every bounce).

    ``transmission``: False (the default: the renderer without the argument, call for call and bit for bit) or True: a BSDF sample
    below the surface is followed through the ball (the module docstring).  It needs analytic ground truth behind an
    ``AnalyticTable``, ``max_depth > 1`` (with occlusion), and balls that touch neither each other nor the floor: ``ValueError``
    otherwise.  ``compact=True`` keeps its property with it."""

    DEPTH_CAP = 1024   # bounces of a pass at max_depth=None; with roulette (q <= 0.95) a path outlives it with probability < 1e-22

    def __init__(self, table, centers, radii, camera=None, env: Optional[torch.Tensor] = None, *args, max_depth: Optional[int] = 1,
                 occlusion: Optional[bool] = None, lights: Optional[Sequence[PointLight]] = None, env_sampling: str = "cosine",
                 rr_depth: Optional[int] = None, compact: bool = False, transmission: bool = False, **kwargs):
        if rr_depth is not None:
            rr_depth = int(rr_depth)
            if rr_depth < 1:
                raise ValueError("rr_depth must be >= 1 (or None: no Russian roulette)")
        if max_depth is None:
            if rr_depth is None:
                raise ValueError("max_depth=None (unbounded depth) needs rr_depth: only Russian roulette makes it finite")
        else:
            max_depth = int(max_depth)
            if max_depth < 1:
                raise ValueError("max_depth must be >= 1")
        deep = max_depth is None or max_depth > 1
        occlusion = deep if occlusion is None else bool(occlusion)
        if deep and not occlusion:
            raise ValueError("max_depth > 1 needs occlusion: without it every vertex would see the environment through the balls")
        if env_sampling not in ("cosine", "importance"):
            raise ValueError(f'env_sampling must be "cosine" or "importance", got {env_sampling!r}')
        if transmission:
            _check_transmission(centers, radii, deep, occlusion, *_array_arguments(args, kwargs))
        self.lights = None
        if lights is not None and len(lights):
            if env_sampling == "importance" and env is None:
                raise ValueError('env_sampling="importance" needs an emitting environment: with lights, pass env')
            self.lights = wf_lights(lights, has_env=env is not None)
            if env is None:
                env = torch.zeros((2, 4, 3), dtype=torch.float32)   # black: path_begin and the lookups stay valid
        super().__init__(table, centers, radii, camera, env, *args, **kwargs)
        if self.use_ground_truth and self.measured_table is None:
            raise ValueError("PathArrayRenderer evaluates the ground truth on the lane-ordered wavefront (fused_ground_truth=True)")
        self.max_depth, self.occlusion, self.rr_depth = max_depth, occlusion, rr_depth
        self.env_sampling = env_sampling
        self.env_dist = None
        if env_sampling == "importance":
            from .envmap import EnvDistribution
            self.env_dist = EnvDistribution(self.env)
        self.compact = bool(compact)
        self.transmission = bool(transmission)
        self.stats = {"lanes_per_bounce": [], "list_per_bounce": [], "depth": 0, "depth_cap_hit": False}

    def _buffers(self, n: int):
        b = super()._buffers(n)
        if "org" not in b:
            for name in ("org", "beta", "rad"):
                b[name] = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            if self.lights is not None:
                b["lsel"] = torch.empty((n,), dtype=torch.int32, device=self.device)
            if self.lights is not None or self.env_dist is not None:
                b["emit"] = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            if self.env_dist is not None:
                b["lpdf"] = torch.empty((n,), dtype=torch.float32, device=self.device)
        return b

    # -- the path kernels ----------------------------------------------------------------------------
    def _list(self, rows, b):
        """(pointer, length) of a live-lane list for the ``_rows`` entry points; ``ValueError`` for what they should not see."""
        if not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()
                and rows.device == b["mat"].device and rows.shape[0] <= b["mat"].shape[0]):
            raise ValueError("rows must be a contiguous int64 tensor [n_rows <= N] on the renderer's device")
        return _p(rows), rows.shape[0]

    def path_begin(self, b):
        """org, beta, rad of the first vertices from what ``primary`` wrote into ``b``."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_wf_path_begin(C.byref(self.scene), _p(self.env), b["mat"].shape[0], _p(b["dir"]),
                                                      _p(b["nrm"]), _p(b["mat"]), _p(b["org"]), _p(b["beta"]), _p(b["rad"]),
                                                      self._stream()))

    def _geometry(self, b, env_dist=None) -> _Geometry:
        """The geometry's part of ``sample_emitter`` and ``bounce`` over ``b``; here: the analytic spheres, which travel in the scene."""
        return _Geometry("bsdfd_wf_", False, [], [], [])

    def sample_emitter(self, b, bounce: int, seed: int, pass_idx: int, path_offset: int, occlusion: Optional[bool] = None,
                       lights: Optional[_lib.WfLights] = None, rows: Optional[torch.Tensor] = None):
        """The emitter sample of the vertices in ``b``: ``lsel``, ``emit``, and ``wl`` towards a picked point light.  ``rows``
        (int64 [n_rows], distinct lanes): of the listed vertices only (``bsdfd_wf_sample_emitter_rows``)."""
        geo = self._geometry(b)
        listed = () if rows is None else self._list(rows, b)
        if geo.one_form and listed and listed[1] == 0:
            return
        occlusion = self.occlusion if occlusion is None else occlusion
        with torch.cuda.device(self.device):
            fn = getattr(_lib.lib(), geo.prefix + ("sample_emitter_rows" if listed else "sample_emitter"))
            _lib.check(fn(*geo.front, C.byref(self.scene), C.byref(self.lights if lights is None else lights), bounce,
                          int(bool(occlusion)), seed, pass_idx, path_offset, b["mat"].shape[0], _p(b["org"]), _p(b["nrm"]), _p(b["wi"]),
                          _p(b["mat"]), _p(b["wl"]), _p(b["lsel"]), _p(b["emit"]), *geo.behind, *listed, self._stream()))
        torch.autograd.graph.increment_version([b["wl"], b["lsel"], b["emit"]])

    def sample_env(self, b, bounce: int, seed: int, pass_idx: int, path_offset: int, occlusion: Optional[bool] = None,
                   lights: Optional[_lib.WfLights] = None, env_dist=None, rows: Optional[torch.Tensor] = None):
        """The environment's emitter sample of the vertices in ``b`` that picked it (``lsel == -1``; all live ones without
        lights): ``lpdf``, ``emit``, and ``wl`` on the balls, drawn from the ``EnvDistribution``.  ``rows`` (int64 [n_rows],
        distinct lanes): of the listed vertices only (``bsdfd_wf_sample_env_rows``)."""
        occlusion = self.occlusion if occlusion is None else occlusion
        lights = self.lights if lights is None else lights
        env_dist = self.env_dist if env_dist is None else env_dist
        with torch.cuda.device(self.device):
            args = [C.byref(self.scene), _p(self.env), C.byref(env_dist.struct(self.device)), 1 if lights is None else lights.n_lights + 1,
                    bounce, int(bool(occlusion)), seed, pass_idx, path_offset, b["mat"].shape[0], _p(b["org"]), _p(b["nrm"]), _p(b["wi"]),
                    _p(b["mat"]), None if lights is None else _p(b["lsel"]), _p(b["wl"]), _p(b["lpdf"]), _p(b["emit"])]
            if rows is None:
                _lib.check(_lib.lib().bsdfd_wf_sample_env(*args, self._stream()))
            else:
                _lib.check(_lib.lib().bsdfd_wf_sample_env_rows(*args, *self._list(rows, b), self._stream()))
        torch.autograd.graph.increment_version([b["wl"], b["lpdf"], b["emit"]])

    def bounce(self, b, bounce: int, last: bool, seed: int, pass_idx: int, path_offset: int, occlusion: Optional[bool] = None,
               lights: Optional[_lib.WfLights] = None, env_dist=None, rr_depth: Optional[int] = None,
               rows: Optional[torch.Tensor] = None):
        """Shade the vertices in ``b`` (``wo``, ``pdf_o``, ``pdf_l`` [, ``f_o``, ``f_l``] from the sampler; with lights also
        ``lsel`` and ``emit`` from ``sample_emitter``; with an ``EnvDistribution`` also ``lpdf`` and ``emit`` from ``sample_env``)
        and move the paths on.  ``rr_depth`` (default: the instance's): with an integer the same emitters go through
        ``bsdfd_wf_bounce_rr``, which plays Russian roulette on the paths that would continue once ``bounce + 1 >= rr_depth``.
        ``rows`` (int64 [n_rows], distinct lanes): the listed vertices only, through ``bsdfd_wf_bounce_rows`` in every mode.
        With ``self.transmission`` every mode, with or without ``rows``, goes through ``bsdfd_wf_bounce_transmit``, which follows a
        BSDF sample below the surface into the ball (it needs ``f_o``).  Other geometry (``_geometry``: a subclass's) has one entry
        point for all of these and its ``_rows`` form."""
        occlusion = self.occlusion if occlusion is None else occlusion
        lights = self.lights if lights is None else lights
        env_dist = self.env_dist if env_dist is None else env_dist
        rr_depth = self.rr_depth if rr_depth is None else rr_depth
        geo = self._geometry(b, env_dist)
        listed = () if rows is None else self._list(rows, b)
        if listed and listed[1] == 0 and (geo.one_form or self.transmission):
            return   # an empty list serves no lane (bsdfd_wf_bounce_transmit reads rows = NULL, n_rows = 0 as "every lane")
        with torch.cuda.device(self.device):
            args = [
                C.byref(self.scene), _p(self.env), bounce, int(bool(last)), int(bool(occlusion)), seed, pass_idx, path_offset,
                b["mat"].shape[0], _p(b["org"]), _p(b["nrm"]), _p(b["wi"]), _p(b["wl"]), _p(b["mat"]), _p(b["beta"]), _p(b["rad"]),
                _p(b["wo"]), _p(b["pdf_o"]), _p(b["pdf_l"]), _p(b.get("f_o")), _p(b.get("f_l"))]
            # the emitter tail (lights, lsel, emit, lpdf, dist), None where the mode has none: bounce takes none of it, bounce_lit
            # the first three, bounce_env all five; bounce_rr, bounce_rows, bounce_transmit and a one-form family all five + rr_depth
            lit, env = lights is not None, env_dist is not None
            tail = [C.byref(lights) if lit else None, _p(b["lsel"]) if lit else None, _p(b["emit"]) if lit or env else None,
                    _p(b["lpdf"]) if env else None, C.byref(env_dist.struct(self.device)) if env else None]
            full = args + tail + [int(rr_depth or 0)]
            if self.transmission:
                name, args, listed = "bounce_transmit", full, listed or (None, 0)
            elif listed:
                name, args = "bounce_rows", full
            elif geo.one_form:
                name, args = "bounce", full
            elif rr_depth is not None:
                name, args = "bounce_rr", full
            elif env:
                name, args = "bounce_env", args + tail
            elif lit:
                name, args = "bounce_lit", args + tail[:3]
            else:
                name = "bounce"
            _lib.check(getattr(_lib.lib(), geo.prefix + name)(*geo.front, *args, *geo.behind, *listed, self._stream()))
        # written through raw pointers: tell torch (the plugin cores key their per-query context cache on wi._version)
        torch.autograd.graph.increment_version([b["wi"], b["wl"], b["nrm"], b["org"], b["mat"], b["beta"], b["rad"]] + geo.written)

    def sample_inside(self, b, bounce: int, seed: int, pass_idx: int, path_offset: int, rows: Optional[torch.Tensor] = None):
        """The sampler's answer for the vertices inside a ball (``wi.z < 0``): ``wo``, ``pdf_o``, ``pdf_l`` of those lanes from the
        analytic model's own sampler (``AnalyticTable.sample_inside``), every other lane untouched."""
        self.measured_table.sample_inside(b["mat"], b["wi"], b["wl"], bounce, seed, pass_idx, path_offset,
                                          out=(b["wo"], b["pdf_o"], b["pdf_l"]), rows=rows)

    def resolve(self, row_begin: int, row_end: int, spp: int, b, film: torch.Tensor):
        """film [row_end-row_begin, width, 3] += the pass' estimate."""
        if film.shape != (row_end - row_begin, self.camera.width, 3) or film.dtype != torch.float32 \
                or not film.is_contiguous() or film.device != self.device:
            raise ValueError("film must be a contiguous fp32 [rows, width, 3] tensor on the renderer's device")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_wf_resolve(C.byref(self.scene), row_begin, row_end, spp, _p(b["rad"]), _p(film),
                                                   self._stream()))

    # -- one pass over a tile ------------------------------------------------------------------------
    def render_pass(self, film: torch.Tensor, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int,
                    x0: Optional[torch.Tensor] = None):
        n = (row_end - row_begin) * self.camera.width * spp
        if n == 0:
            return
        from .materials import WavefrontPipeline
        b = self.primary(row_begin, row_end, spp, seed, pass_idx)
        self.path_begin(b)
        offset = row_begin * self.camera.width * spp
        skey = (seed * 0x9E3779B97F4A7C15 + pass_idx + 1) & _M64
        n_balls = len(self.table)
        lanes, lists = [], []
        depth = self.DEPTH_CAP if self.max_depth is None else self.max_depth   # (unbounded: the loop ends where no lane is live)
        rows = None   # compact, from bounce 1 on: the lanes alive entering the bounce before, the front of its bucketing's permutation
        for k in range(depth):
            on = {} if rows is None else {"rows": rows}
            if self.lights is not None:
                self.sample_emitter(b, k, seed, pass_idx, offset, **on)
            if self.env_dist is not None:
                self.sample_env(b, k, seed, pass_idx, offset, **on)
            if rows is None:
                plan = self.table.bucket(b["mat"], extra_bins=2)  # floor vertices and ended paths behind the materials
            else:
                plan = self.table.bucket_rows(b["mat"], rows, extra_bins=1)   # ... and here ended paths are left out
            counts = plan[1]                                      # (already on the host)
            n_mat = sum(counts[:n_balls])
            n_live = n_mat + counts[n_balls]
            if n_live == 0:
                break
            lanes.append(n_mat)
            lists.append(n if rows is None else rows.shape[0])
            if n_mat:
                key = skey if k == 0 else skey ^ ((k * 0xD1B54A32D192ED03) & _M64)
                if rows is None:
                    b["wo"], b["pdf_o"], b["pdf_l"] = self.table.sample_pdf(plan, b["wi"], b["wl"], seed=key, offset=offset,
                                                                            direct=n <= WavefrontPipeline.DIRECT_MAX_LANES)
                    if self.transmission and k >= 1:   # (the camera is outside: bounce 0 has no vertex inside a ball)
                        self.sample_inside(b, k, seed, pass_idx, offset)
                    if self.use_ground_truth:
                        self.measured_table.eval_t(b["mat"], b["wi"], b["wo"], b["wl"], tint=self.plugin.albedo, out_o=b["f_o"],
                                                   out_l=b["f_l"])
                else:   # into the arrays of bounce 0, no fill: bounce reads them on the material lanes of this list only
                    self.table.sample_pdf(plan, b["wi"], b["wl"], seed=key, offset=offset, direct=True,
                                          out=(b["wo"], b["pdf_o"], b["pdf_l"]))
                    if self.transmission:
                        self.sample_inside(b, k, seed, pass_idx, offset, rows=plan[0][:n_mat])
                    if self.use_ground_truth:
                        self.measured_table.eval_t(b["mat"], b["wi"], b["wo"], b["wl"], tint=self.plugin.albedo, out_o=b["f_o"],
                                                   out_l=b["f_l"], rows=plan[0][:n_mat])
            # (no material lane: only floor vertices are left, which read neither the sampler's nor the evaluator's arrays)
            if rows is None:
                self.bounce(b, k, k == depth - 1, seed, pass_idx, offset)
            else:
                self.bounce(b, k, k == depth - 1, seed, pass_idx, offset, rows=plan[0])
            if self.compact:
                rows = plan[0][:n_live]
        self.stats["lanes_per_bounce"] = lanes
        self.stats["list_per_bounce"] = lists
        self.stats["depth"] = len(lanes)
        self.stats["depth_cap_hit"] = self.max_depth is None and len(lanes) == depth
        self.resolve(row_begin, row_end, spp, b, film)
