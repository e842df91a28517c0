"""Reference for Russian roulette in the array-scene path tracer (bsdf_diffusion_sampling_amd/csrc/pathrr.hip,
``bsdfd_wf_bounce_rr``): a numpy restatement of the rule inside ``bounce_vertex<Mode, RR>``, fp64 by default, fp32 on request, as a
wrapper around the references of the three bounce kernels (tests/pathtrace_ref.py, tests/pathtrace_lights_ref.py,
tests/envmap_ref.py), and ``reference_pass_rr``: ``pass_replay.reference_pass`` with that wrapper and the unbounded loop.

Test infrastructure only.  The rule (Mitsuba's ``path`` integrator, restated): once ``bounce + 1 >= rr_depth`` a path that would
continue survives with probability ``q = min(max_c(beta_c thr_c), 0.95)`` — the throughput after the vertex — and its throughput
is divided by ``q``; the variate is ``(word 0 >> 8) 2^-24`` of the lane's Philox draw with counter word 3 = "Roul" + bounce.
"""
from __future__ import annotations

import numpy as np

import envmap_ref as ER
import pass_replay as PR
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from oracle import wavefront_oracle as WO
from oracle.wavefront_oracle import philox4x32

F = np.float32
TAG = 0x526F756C            # "Roul"
Q_MAX = F(0.95)             # the kernel's constant is the fp32 number
OFFSET = (1 << 32) - 100    # the counter's low word wraps inside a wavefront that starts here
KEPT = ("org", "nrm", "wi", "wl", "beta")


def variates(seed: int, pass_idx: int, bounce: int, path_offset: int, n: int):
    """[n] fp32, exact: (word 0 >> 8) * 2^-24 of philox(key = seed, counter = (path lo, hi, pass, "Roul" + bounce))."""
    gp = (np.uint64(path_offset & PR.M64) + np.arange(n, dtype=np.uint64))
    u = philox4x32(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, gp & np.uint64(0xFFFFFFFF), gp >> np.uint64(32),
                   pass_idx & 0xFFFFFFFF, (TAG + bounce) & 0xFFFFFFFF)
    return (u[0] >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


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


def throughput_factor(scene: dict, wi, material, pdf_o, f_o=None, dtype=np.float64):
    """``thr`` [n,3] of the bounce body, restated from ``pathtrace_ref._bounce``: the reflectance in the wi slot on the floor,
    f_o / pdf_o on a ball with ground truth, the albedo on a proxy ball."""
    n = len(material)
    n_b = len(scene["spheres"])
    wi = np.asarray(wi).astype(dtype)
    albedo = np.asarray(scene["albedo"], dtype=F).astype(dtype)[None, :]
    with np.errstate(all="ignore"):
        pb = np.where(np.isfinite(pdf_o) & (pdf_o > 0), pdf_o, 0).astype(dtype)
        gt_o = np.zeros(n, dtype=bool) if f_o is None else ~np.isnan(f_o[:, 0])
        thr_o = np.where(gt_o[:, None], (np.zeros((n, 3)) if f_o is None else np.nan_to_num(f_o)).astype(dtype) / pb[:, None], albedo)
    return np.where((material == n_b)[:, None], wi[:, 0:1], thr_o).astype(dtype)


def with_roulette(scene: dict, out: dict, rr_depth: int, bounce: int, last: bool, seed: int, pass_idx: int, path_offset: int,
                  org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o=None, f_l=None, dtype=np.float64, scale=True):
    """The output dict of ``pathtrace_ref.bounce`` / ``pathtrace_lights_ref.bounce_lit`` / ``envmap_ref.bounce_env`` (called with
    the same inputs and the same ``last``) -> the output of the RR kernel: killed rows get the miss id and keep the input values
    of every other array, survivors get ``beta = beta_in (thr / q)``; ``rad`` is untouched.  Added keys: ``would`` (rows that
    continue without roulette), ``u``, ``q``, ``survive`` (``would`` and the roulette lets it), ``killed``.  ``scale=False`` leaves
    out the division — the biased estimator the unbiasedness test must be able to tell apart."""
    assert rr_depth >= 1
    n_b, n = len(scene["spheres"]), len(material)
    would = (material >= 0) & (material <= n_b) & (out["material"] >= 0) & (out["material"] <= n_b)
    out = dict(out)
    thr = throughput_factor(scene, wi, material, pdf_o, f_o, dtype)
    u, q, ok = roulette(beta, thr, seed, pass_idx, bounce, path_offset, n, dtype)
    active = (not last) and bounce + 1 >= rr_depth
    survive = would & ok if active else would
    killed = would & ~survive
    inputs = dict(org=org, nrm=nrm, wi=wi, wl=wl, beta=beta)
    for name in KEPT:
        out[name] = np.where(killed[:, None], np.asarray(inputs[name]).astype(dtype), out[name])
    out["material"] = np.where(killed, n_b + 1, out["material"]).astype(np.int64)
    out["cos_in"] = np.where(killed, np.nan, out["cos_in"])
    if active and scale:
        with np.errstate(all="ignore"):
            scaled = np.asarray(beta).astype(dtype) * (thr * (dtype(1) / q)[:, None])
        out["beta"] = np.where(survive[:, None], scaled, out["beta"])
    out.update(would=would, u=u, q=q, survive=survive, killed=killed)
    return out


def bounce_rr(scene: dict, env, rr_depth: int, bounce: int, last: bool, occlusion: bool, seed: int, pass_idx: int, path_offset: int,
              org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o=None, f_l=None, n_e: int = 1, has_env: bool = True,
              lsel=None, emit=None, lpdf=None, tables=None, dtype=np.float64, scale=True):
    """One call of bsdfd_wf_bounce_rr, with its mode selection: ``tables`` given -> ENV (``envmap_ref.bounce_env``), else ``lsel``
    given -> LIT (``pathtrace_lights_ref.bounce_lit``), else COSINE (``pathtrace_ref.bounce``)."""
    args = (bounce, last, occlusion, seed, pass_idx, path_offset, org, nrm, wi, wl, material, beta, rad, wo, pdf_o, pdf_l, f_o, f_l)
    if tables is not None:
        out = ER.bounce_env(scene, env, tables, n_e, *args, lsel=lsel, emit=emit, lpdf=lpdf, dtype=dtype)
    elif lsel is not None:
        out = LR.bounce_lit(scene, env, n_e, has_env, *args, lsel=lsel, emit=emit, dtype=dtype)
    else:
        out = R.bounce(scene, env, *args, dtype=dtype)
    return with_roulette(scene, out, rr_depth, *args[:2], *args[3:], dtype=dtype, scale=scale)


def rr_wavefront(v: dict, seed: int, zero_rows: int = 32, scene: dict = R.SYNTH_SCENE):
    """The synthetic wavefront ``v`` (``pathtrace_ref.synthetic_vertices`` or one of its two descendants) made fit for roulette:
    ``beta`` per row and channel log-uniform in [1e-3, 2], and ``f_o`` = 0 on ``zero_rows`` of the ball rows that have ground truth
    (q = 0: the path must end).  Ended rows keep their NaN state."""
    g = np.random.default_rng(seed)
    n = len(v["material"])
    n_b = len(scene["spheres"])
    beta = np.exp(g.uniform(np.log(1e-3), np.log(2.0), (n, 3)))
    beta[v["material"] > n_b] = np.nan
    out = dict(v, beta=beta.astype(F))
    if "f_o" in v:
        f_o = v["f_o"].copy()
        rows = np.flatnonzero((v["material"] < n_b) & ~np.isnan(f_o[:, 0]) & np.isfinite(v["pdf_o"]) & (v["pdf_o"] > 0) & (v["wo"][:, 2] > 0))
        f_o[g.choice(rows, zero_rows, replace=False)] = 0.0
        out["f_o"] = f_o
    return out


def reference_pass_rr(scene: dict, env, mode: str, lights, tables, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int,
                      max_depth, rr_depth: int, occlusion: bool, answers, dtype=np.float64, depth_cap: int = 1024, scale=True):
    """``pass_replay.reference_pass`` with Russian roulette in every bounce and, for ``max_depth=None``, the unbounded loop: it runs
    until no lane is live, ``depth_cap`` bounces at the most (the bounce at the cap is ``last``).  A sequence of ``answers`` that
    runs out ends the loop too (the device's pass was shorter: its rows then differ in their histories).
    -> the dict of ``reference_pass`` + depth (bounces run) + depth_cap_hit."""
    assert mode in ("cosine", "importance")
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
    history = [PR.decision_code(scene, mat, wi)]
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
        out = bounce_rr(scene, env, rr_depth, k, k == depth - 1, occlusion, seed, pass_idx, offset, *[st[name] for name in PR.STATE],
                        a["wo"], a["pdf_o"], a["pdf_l"], a.get("f_o"), a.get("f_l"), n_e=n_e, has_env=has_env,
                        lsel=st.get("lsel") if lights is not None else None, emit=st.get("emit"), lpdf=st.get("lpdf"),
                        tables=tables if mode == "importance" else None, dtype=dtype, scale=scale)
        st.update({name: (out[name] if name == "material" else out[name].astype(dtype)) for name in PR.STATE})
        stages.append(("bounce", k, dict(st, cos_in=out["cos_in"], killed=out["killed"], survive=out["survive"], q=out["q"])))
        history.append(PR.decision_code(scene, st["material"], st["wi"]))
        ran = k + 1
    film = R.resolve(st["rad"], spp).reshape(row_end - row_begin, width, 3)
    return dict(stages=stages, history=history, rad=st["rad"], film=film, depth=ran, depth_cap_hit=max_depth is None and ran == depth)
