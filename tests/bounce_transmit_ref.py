"""Reference for the transmitting bounce of the array-scene path tracer (``bsdfd_wf_bounce_transmit``: ``bounce_dev.h``'s
``bounce_vertex<Mode, RR, LIST, TRANSMIT = true>``) and for what goes with it: the variates of ``bsdfd_wf_sample_inside``, the
synthetic wavefront both are checked on, and whole passes with transmission.

Test infrastructure only.  ``bounce`` is tests/bounce_ref.py's with ONE rule changed in its ball branch, fp64 by default, fp32 on
request: under occlusion a usable BSDF sample (``pdf_o > 0``) below the surface (``wo.z < 0``) at a vertex with ground truth
(``f_o`` not NaN) whose throughput factor ``thr = f_o / pdf_o`` is positive in some channel is not dropped.  The ray enters, or
stays in, the ball it is on and its next vertex is that ball's far side, ``t = -2 (x - c) . d`` along the ray (``chord``): the
far root of ``trace``'s quadratic for an origin on the sphere.  Everything else — the radiance the vertex adds (a sample that goes
inside adds no escape term, exactly as a dropped one), the roulette on ``beta * thr``, how the new vertex is written — is the
plain bounce's, so the reference IS the plain reference with the rows the rule triggers on continued instead of ended.
"""
from __future__ import annotations

import numpy as np

import bounce_ref as B
import pass_replay as PR
import pathtrace_lights_ref as LR
import pathtrace_ref as R

F = np.float32
TAG_INSIDE = 0x496E7364     # "Insd"


def inside_variates(seed: int, pass_idx: int, bounce: int, path_offset: int, n: int):
    """[n,3] fp32, exact: u_k = (word k >> 8) * 2^-24 of philox(key = seed, counter = (path lo, hi, pass, "Insd" + bounce)) — the
    variates ``bsdfd_wf_sample_inside`` hands the model's sampler on lane ``p`` (path = path_offset + p)."""
    w = R.tagged_draw(TAG_INSIDE, seed, pass_idx, bounce, path_offset, n)
    return np.stack([R.unit(w[0]), R.unit(w[1]), R.unit(w[2])], 1)


def chord(c, r, x, d, dtype=np.float64):
    """The far side of the ball (c [N,3], r [N]) along the ray from ``x`` ON the sphere in the inward direction ``d``, as
    ``continue_path`` writes a vertex: -> (t, position, outward normal, wi) with ``t = -2 (x - c) . d``, the normal
    normalised, the position projected onto the sphere, ``wi`` = -d in the frame of the OUTWARD normal (so wi.z < 0)."""
    c, x, d, r = (np.asarray(a).astype(dtype) for a in (c, x, d, r))
    oc = x - c
    t = dtype(-2) * R._dot(oc, d)
    nv = (oc + t[:, None] * d) / r[:, None]
    nv = nv / np.sqrt(R._dot(nv, nv))[:, None]
    gs, gt = R._onb(nv)
    wi = np.stack([-R._dot(d, gs), -R._dot(d, gt), -R._dot(d, nv)], 1)
    return t, c + r[:, None] * nv, nv, wi


def far_root(c, r, x, d):
    """The far root of the quadratic |x + t d - c|^2 = r^2 in fp64, by the stable form (no cancellation for an origin on the
    sphere): with b = (x - c) . d and q = -(b + sign(b) sqrt(b^2 - cc)) the roots are q and cc / q, cc = |x - c|^2 - r^2."""
    oc = np.asarray(x, np.float64) - np.asarray(c, np.float64)
    b = R._dot(oc, np.asarray(d, np.float64))
    cc = R._dot(oc, oc) - np.asarray(r, np.float64) ** 2
    q = -(b + np.copysign(np.sqrt(np.maximum(b * b - cc, 0.0)), b))
    with np.errstate(all="ignore"):
        return np.maximum(q, np.where(q != 0, cc / q, q))


def bounce(*args, **kwargs):
    with np.errstate(all="ignore"):
        return _bounce(*args, **kwargs)


def _bounce(scene: dict, env, mode: str, bounce: int, last: bool, occlusion: bool, seed: int, pass_idx: int, path_offset: int,
            org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o=None, f_l=None, rr_depth=None, scale=True,
            dtype=np.float64, **emitters):
    """One call of bsdfd_wf_bounce_transmit, with ``bounce_ref.bounce``'s arguments and result, plus ``enter`` [N]: the rows the
    rule triggers on (whether or not ``last`` or the roulette then ends them)."""
    out = B._bounce(scene, env, mode, bounce, last, occlusion, seed, pass_idx, path_offset, org, nrm, wi, wl, material, beta, rad, wo,
                    pdf_o, pdf_l, f_o, f_l, rr_depth=rr_depth, scale=scale, dtype=dtype, **emitters)
    n_b, n = len(scene["spheres"]), len(material)
    material = np.asarray(material)
    live = (material >= 0) & (material <= n_b)
    ball = live & (material < n_b)
    cast = lambda a: np.asarray(a).astype(dtype)
    org_d, nrm_d, wo_d, beta_d = cast(org), cast(nrm), cast(wo), cast(beta)
    pb = np.where(np.isfinite(pdf_o) & (pdf_o > 0), pdf_o, 0).astype(dtype)
    gt_o = np.zeros(n, dtype=bool) if f_o is None else ~np.isnan(f_o[:, 0])
    thr = (np.zeros((n, 3)) if f_o is None else np.nan_to_num(f_o)).astype(dtype) / pb[:, None]
    enter = ball & bool(occlusion) & (pb > 0) & (wo_d[:, 2] < 0) & gt_o & (np.fmax(np.fmax(thr[:, 0], thr[:, 1]), thr[:, 2]) > 0)
    would = enter & (not last)
    cont, thr_on = would, thr
    if rr_depth is not None:
        u, q, ok = B.roulette(beta_d, thr, seed, pass_idx, bounce, path_offset, n, dtype)
        if not last and bounce + 1 >= rr_depth:
            cont = would & ok
            if scale:
                thr_on = thr * (dtype(1) / q)[:, None]
    fs, ft, nn = LR._frames(nrm_d, live, dtype)
    d = wo_d[:, 0:1] * fs + wo_d[:, 1:2] * ft + wo_d[:, 2:3] * nn
    k = np.clip(material, 0, n_b - 1)
    cs = np.asarray([np.asarray(c, dtype=F) for c, _ in scene["spheres"]], dtype=F).astype(dtype)[k]
    rs = np.asarray([F(r) for _, r in scene["spheres"]], dtype=F).astype(dtype)[k]
    t, xv, nv, w_in = chord(cs, rs, org_d, d, dtype)
    m3 = cont[:, None]
    out.update(org=np.where(m3, xv, out["org"]), nrm=np.where(m3, nv, out["nrm"]), wi=np.where(m3, w_in, out["wi"]),
               wl=np.where(m3, R.next_wl(seed, pass_idx, bounce, path_offset, n).astype(dtype), out["wl"]),
               material=np.where(cont, material, out["material"]).astype(np.int64),
               beta=np.where(m3, beta_d * thr_on, out["beta"]), cos_in=np.where(cont, -R._dot(d, nv), out["cos_in"]),
               thr=np.where(enter[:, None], thr, out["thr"]), enter=enter)
    if rr_depth is not None:
        out.update(would=out["would"] | would, survive=out["survive"] | cont, killed=out["killed"] | (would & ~cont))
    return out


# ---- the synthetic wavefront -------------------------------------------------------------------------------------------------------
def synthetic_vertices(n: int = 4096, seed: int = 7):
    """``pathtrace_ref.synthetic_vertices`` (3 balls, the floor, ended rows) made to exercise the rule: on the ball rows ``wo`` points
    below the surface on 60 % (with ground truth, without it — the NaN rows —, and, on a tenth, with ``f_o == 0``: an opaque
    material), and half of the ball rows are vertices INSIDE their ball (``wi.z < 0``), with ``wo`` on either side.  A ray with
    wo.z < 0 is never traced, so flipping it moves no row towards a threshold of ``trace``.
    -> (dict of fp32 / int64 arrays, dict of the row classes)."""
    v = R.synthetic_vertices(n, seed)
    g = np.random.default_rng([seed, 0x496E])
    n_b = len(R.SYNTH_SCENE["spheres"])
    ball = v["material"] < n_b
    below = ball & (g.random(n) < 0.6)
    v["wo"][:, 2] = np.where(below, -np.abs(v["wo"][:, 2]), np.where(ball, np.abs(v["wo"][:, 2]), v["wo"][:, 2]))
    opaque = below & ~np.isnan(v["f_o"][:, 0]) & (g.random(n) < 0.1)
    v["f_o"][opaque] = 0.0
    inside = ball & (g.random(n) < 0.5)
    v["wi"][:, 2] = np.where(inside, -np.abs(v["wi"][:, 2]), v["wi"][:, 2])
    gt = ~np.isnan(v["f_o"][:, 0])
    usable = np.isfinite(v["pdf_o"]) & (v["pdf_o"] > 0)
    down = ball & (v["wo"][:, 2] < 0)
    classes = dict(with_gt=down & gt & ~opaque & usable, without_gt=down & ~gt, opaque=opaque, inside=inside,
                   inside_outward=inside & (v["wo"][:, 2] > 0), inside_inward=inside & down)
    return v, classes


# ---- whole passes ------------------------------------------------------------------------------------------------------------------
class Recorder(PR.Recorder):
    """``pass_replay.Recorder`` with the renderer's ``sample_inside`` stage recorded too (name "sample_inside"; args: bounce, seed,
    pass_idx, path_offset)."""

    def __enter__(self):
        super().__enter__()
        rec = self

        def make(inner):
            def f(b, bounce, seed, pass_idx, path_offset, rows=None):
                assert b is rec.b and rows is None
                before = rec._snap()
                out = inner(b, bounce, seed, pass_idx, path_offset, rows=rows)
                rec.stages.append(dict(name="sample_inside", args=dict(bounce=bounce, seed=seed, pass_idx=pass_idx,
                                                                       path_offset=path_offset), before=before, after=rec._snap()))
                return out
            return f
        self._wrap(self.r, "sample_inside", make)
        return self


def reference_pass(*args, **kwargs):
    """``pass_replay.reference_pass`` with the transmitting bounce in place of the plain one (the sampler's and the evaluator's
    answers are inputs there, the inside sampler's among them)."""
    plain = PR.B
    try:
        PR.B = _Transmitting
        return PR.reference_pass(*args, **kwargs)
    finally:
        PR.B = plain


class _Transmitting:
    bounce = staticmethod(bounce)
