"""Reference for the bounce of the array-scene path tracer (bsdf_diffusion_sampling_amd/csrc/bounce.hip: ``bsdfd_wf_bounce``,
``_lit``, ``_env``, ``_rr``): ONE numpy restatement of ``bounce_dev.h``'s ``bounce_vertex<Mode, RR>``, section by section, fp64 by
default, fp32 on request, on top of tests/pathtrace_ref.py (``trace``, the bases, the tagged draw), tests/pathtrace_lights_ref.py
(frames) and tests/envmap_ref.py (the environment's density).

Test infrastructure only.  The modes, as in the header: "cosine" — only the environment emits; "lit" — one emitter sample per
vertex among ``n_e`` = point lights [+ the environment] (``lsel``, ``emit`` of ``sample_emitter``); "env" — the environment's
sample drawn from its own distribution (``lpdf``, ``emit`` of ``sample_env``; ``lsel`` None: no point lights).  The roulette
(Mitsuba's ``path`` integrator, restated): once ``bounce + 1 >= rr_depth`` a path that would continue survives with probability
``q = min(max_c(beta_c thr_c), 0.95)`` — the throughput after the vertex — and its throughput is divided by ``q``; the variate is
``(word 0 >> 8) 2^-24`` of the lane's Philox draw with counter word 3 = "Roul" + bounce.
"""
from __future__ import annotations

import numpy as np

import envmap_ref as ER
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from oracle.wavefront_oracle import env_lookup, mis_power

F = np.float32
TAG = 0x526F756C            # "Roul"
Q_MAX = F(0.95)             # the kernel's constant is the fp32 number
MODES = ("cosine", "lit", "env")


def variates(seed: int, pass_idx: int, bounce: int, path_offset: int, n: int):
    """[n] fp32, exact: (word 0 >> 8) * 2^-24 of philox(key = seed, counter = (path lo, hi, pass, "Roul" + bounce))."""
    return R.unit(R.tagged_draw(TAG, seed, pass_idx, bounce, path_offset, n)[0])


def roulette(beta_in, thr, seed: int, pass_idx: int, bounce: int, path_offset: int, n: int, dtype=np.float64):
    """-> (u [n] fp32, q [n] ``dtype``, survive [n] bool) of rows ``beta_in`` [n,3] x ``thr`` [n,3]: the decision of every row, whether
    or not its path would continue (the caller masks).  A NaN product is skipped by the maximum, as fmaxf skips it; a q that is
    not a positive number kills."""
    with np.errstate(all="ignore"):
        t = np.asarray(beta_in).astype(dtype) * np.asarray(thr).astype(dtype)
        q = np.fmin(np.fmax(np.fmax(t[:, 0], t[:, 1]), t[:, 2]), dtype(Q_MAX)).astype(dtype)
        u = variates(seed, pass_idx, bounce, path_offset, n)
        survive = (q > 0) & (u.astype(dtype) < q)
    return u, q, survive


def bounce(*args, **kwargs):
    """``_bounce`` with numpy's floating-point warnings off: rows that are masked out divide by zero on the way."""
    with np.errstate(all="ignore"):
        return _bounce(*args, **kwargs)


def _bounce(scene: dict, env, mode: str, bounce: int, last: bool, occlusion: bool, seed: int, pass_idx: int, path_offset: int,
            org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o=None, f_l=None, n_e: int = 1, has_env: bool = True,
            lsel=None, emit=None, lpdf=None, tables=None, rr_depth=None, scale=True, dtype=np.float64):
    """One call of bsdfd_wf_bounce (``mode`` "cosine"), _lit ("lit"), _env ("env") or, with ``rr_depth``, of bsdfd_wf_bounce_rr in
    that mode -> dict(org, nrm, wi, wl, material, beta, rad, cos_in, thr): the arrays after the call (rows the kernel does not write
    keep their input values); ``cos_in`` [N] = -d . n at the new vertex (nan where none), for the grazing-hit bound; ``thr`` [N,3]
    the throughput factor of the continuing direction, before the roulette.  With ``rr_depth`` also ``would`` (rows that continue
    without roulette), ``u``, ``q``, ``survive`` (``would`` and the roulette lets it), ``killed``: a killed row gets the miss id and
    keeps its input values.  ``scale=False`` leaves out the division by q — the biased estimator the unbiasedness test must be
    able to tell apart."""
    assert mode in MODES and (f_o is None) == (f_l is None) and (rr_depth is None or rr_depth >= 1)
    n_b = len(scene["spheres"])
    n = len(material)
    cast = lambda a: np.asarray(a).astype(dtype)
    org, nrm, wi, wl, beta, rad, wo = (cast(a) for a in (org, nrm, wi, wl, beta, rad, wo))
    live = (material >= 0) & (material <= n_b)
    floor = live & (material == n_b)
    ball = live & ~floor
    fs, ft, nn = LR._frames(nrm, live, dtype)
    to_world = lambda v: v[:, 0:1] * fs + v[:, 1:2] * ft + v[:, 2:3] * nn
    own = np.where(live, material, -2)
    env64 = np.asarray(env, dtype=np.float64)
    look = lambda dw: env_lookup(env64, dw.astype(F)).astype(dtype)
    inv_pi = dtype(0.31830988618379067154)
    albedo = np.asarray(scene["albedo"], dtype=F).astype(dtype)[None, :]
    # probability with which the one emitter sample went to the environment, and whether the environment emits at all
    sel_p = dtype(1) if mode == "cosine" else dtype(1) / dtype(n_e)
    env_emits = mode != "lit" or has_env
    # the emitter sample, ready-made in emit: of a picked point light (lit, env) or the environment's own draw (env)
    point = np.zeros(n, dtype=bool) if mode == "cosine" or lsel is None else live & (lsel >= 0)
    sampled = np.ones(n, dtype=bool) if mode == "env" else point
    if mode == "env":   # (rows nobody wrote are rows nobody reads)
        emit, lpdf = np.nan_to_num(np.asarray(emit)).astype(dtype), np.nan_to_num(np.asarray(lpdf)).astype(dtype)
    else:
        emit = np.zeros((n, 3), dtype=dtype) if mode == "cosine" else cast(emit)

    nothing = (np.full(n, dtype(R.T_NONE)), np.full(n, -1), np.zeros((n, 3), dtype=dtype), np.ones(n, dtype=dtype))
    lw, dw = to_world(wl), to_world(wo)
    t_f, id_f, c_f, r_f = R.trace(scene, org, lw, own, dtype) if occlusion else nothing
    t_o, id_o, c_o, r_o = R.trace(scene, org, dw, own, dtype) if occlusion else nothing
    hit_l, hit_o = id_f >= 0, id_o >= 0
    e_l = look(lw)
    pb = np.where(np.isfinite(pdf_o) & (pdf_o > 0), pdf_o, 0).astype(dtype)
    pbl = np.where(np.isfinite(pdf_l) & (pdf_l > 0), pdf_l, 0).astype(dtype)
    gt_o = np.zeros(n, dtype=bool) if f_o is None else ~np.isnan(f_o[:, 0])
    gt_l = np.zeros(n, dtype=bool) if f_l is None else ~np.isnan(f_l[:, 0])
    thr_o = np.where(gt_o[:, None], (np.zeros((n, 3)) if f_o is None else np.nan_to_num(f_o)).astype(dtype) / pb[:, None], albedo)
    f_l_v = albedo * pbl[:, None] if f_l is None else np.where(gt_l[:, None], np.nan_to_num(f_l).astype(dtype), albedo * pbl[:, None])
    follow = ball & (pb > 0) & ((wo[:, 2] > 0) if occlusion else np.ones(n, dtype=bool))
    # ---- floor vertices: the cosine direction in wl is the BSDF sample — at full weight towards the environment, or (env) weighted
    # against the environment's own density — plus the emitter sample's whole term ----
    refl = wi[:, 0:1]
    w_f = mis_power(wl[:, 2] * inv_pi, ER.pdf(tables, lw, dtype) * sel_p).astype(dtype) if mode == "env" else np.ones(n, dtype=dtype)
    L_floor = np.where(hit_l[:, None], dtype(0), w_f[:, None] * refl * e_l) if env_emits else np.zeros((n, 3), dtype=dtype)
    L_floor = L_floor + np.where(sampled[:, None], emit, dtype(0))
    # ---- ball vertices: the two strategies of shade_kernel ----
    # a BSDF sample that escapes, weighted against the light strategy's density for its direction
    p_light = (ER.pdf(tables, dw, dtype) if mode == "env" else np.maximum(wo[:, 2], 0) * inv_pi) * sel_p
    w_o = mis_power(pb, p_light).astype(dtype)
    L = np.where((follow & ~hit_o)[:, None], w_o[:, None] * look(dw) * thr_o, dtype(0)) if env_emits else np.zeros((n, 3), dtype=dtype)
    # the light strategy.  The emitter sample: a point is a delta and has no MIS weight, the environment's draw is weighted against
    # the sampler's density for its direction ...
    ok_l = ball & ((pbl > 0) | gt_l)
    w_e = np.where(point, dtype(1), mis_power(lpdf, pbl).astype(dtype)) if mode == "env" else np.ones(n, dtype=dtype)
    L = L + np.where((ok_l & sampled)[:, None], w_e[:, None] * emit * f_l_v, dtype(0))
    # ... or the environment along the cosine sample (pdf cos/pi, chosen with probability sel_p), unless something is in the way
    pl = wl[:, 2] * inv_pi * sel_p
    ok_c = ok_l & ~sampled & (pl > 0) & ~hit_l
    w_l = np.where(ok_c, mis_power(pl, pbl).astype(dtype) / pl, dtype(0))
    L = L + np.where(ok_c[:, None], w_l[:, None] * e_l * f_l_v, dtype(0))
    L = np.where(floor[:, None], L_floor, L)
    rad_new = np.where(live[:, None], rad + beta * L, rad)
    # ---- where the path goes: the same in every mode ----
    go = (follow & hit_o) | (floor & hit_l)
    d = np.where(floor[:, None], lw, dw)
    t = np.where(floor, t_f, t_o)
    hid = np.where(floor, id_f, id_o)
    c, r = np.where(floor[:, None], c_f, c_o), np.where(floor, r_f, r_o)
    thr = np.where(floor[:, None], refl, thr_o)
    cont = would = go & (not last)
    # ---- Russian roulette on that thr: a path that is killed ends exactly as one that escaped ----
    thr_on = thr
    if rr_depth is not None:
        u, q, ok = roulette(beta, thr, seed, pass_idx, bounce, path_offset, n, dtype)
        if not last and bounce + 1 >= rr_depth:
            cont = would & ok
            if scale:
                thr_on = thr * (dtype(1) / q)[:, None]
    # ---- the continuation ----
    mat_new = np.where(live, np.where(cont, hid, n_b + 1), material).astype(np.int64)
    on_ball = cont & (hid < n_b)
    tt = np.where(cont, t, dtype(0))
    nv = ((org - c) + tt[:, None] * d) / r[:, None]
    nv = nv / np.sqrt(R._dot(nv, nv))[:, None]
    nv = np.where(on_ball[:, None], nv, np.array([0.0, 1.0, 0.0], dtype=dtype))
    gs, gt = R._onb(nv)   # (the oracle's onb rounds its input to fp32: the new basis is formed in `dtype`)
    w_ball = np.stack([-R._dot(d, gs), -R._dot(d, gt), -R._dot(d, nv)], 1)
    x_ball = c + r[:, None] * nv
    x_floor = org + tt[:, None] * d
    plane = scene.get("plane") or dict(scale=1.0, c0=0.0, c1=0.0)
    cx = np.floor(x_floor[:, 0] * dtype(F(plane["scale"]))).astype(np.int64)
    cz = np.floor(x_floor[:, 2] * dtype(F(plane["scale"]))).astype(np.int64)
    refl_new = np.where(((cx + cz) & 1) == 1, dtype(F(plane["c1"])), dtype(F(plane["c0"])))
    out = dict(
        org=np.where(cont[:, None], np.where(on_ball[:, None], x_ball, x_floor), org),
        nrm=np.where(cont[:, None], nv, nrm),
        wi=np.where(cont[:, None], np.where(on_ball[:, None], w_ball, refl_new[:, None]), wi),
        wl=np.where(cont[:, None], R.next_wl(seed, pass_idx, bounce, path_offset, n).astype(dtype), wl),
        material=mat_new,
        beta=np.where(cont[:, None], beta * thr_on, beta),
        rad=rad_new,
        cos_in=np.where(cont, -R._dot(d, nv), np.nan),
        thr=thr,
    )
    if rr_depth is not None:
        out.update(would=would, u=u, q=q, survive=cont, killed=would & ~cont)
    return out
