"""GPU: the principled ground truth (csrc/principled.hip, ``analytic.Principled``) and the full-sphere plugin's use of it.

Accuracy is held to a yardstick computed here: tests/principled_ref.py run in fp32 on the same rows, both errors taken against
its fp64 run; the kernels may be 4x worse at the 99th percentile and at the maximum (the project's tail margin, DESIGN.md
section 5).  An error is relative to max(|fp64 value|, 1e-6 of the column's largest): smaller values are compared absolutely.

Where a product cannot be exact the check is the exact statement next to it: the weight is held, bit for bit, to ``eval_t / pdf``
formed in IEEE fp32 on the host.  The lobe a sample took is read off its direction: the nearest of the four candidate directions
of the fp64 reference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import principled_ref as R  # noqa: E402

N = 4096
TINT = (0.9, 0.2, 0.4)
# a material the reference's list does not reach: coloured, isotropic, part subsurface, another interface
CUSTOM = dict(base_color=(0.8, 0.3, 0.1), roughness=0.4, anisotropic=0.0, metallic=0.2, spec_trans=0.5, eta=1.33, spec_tint=0.7,
              sheen=0.5, sheen_tint=0.6, flatness=0.3, clearcoat=0.5, clearcoat_gloss=0.2)
MATERIALS = (2, 5, 10, 13, "custom")
SEED = {2: 2, 5: 5, 10: 10, 13: 13, "custom": 99}


def _params(key):
    return dict(CUSTOM) if key == "custom" else R.reference_params(key)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _hand_rows(eta):
    """(wi, wo, exactly_zero): the hand-placed pairs; ``exactly_zero`` marks those whose eval and pdf are 0 by rule."""
    w = R.wi_of
    graze = w(1.55, 0.3)[0]
    inside = w(np.pi - 1.2, 0.7)[0]                               # from inside, beyond the critical angle of every material here
    tilted = w(0.4, 2.0)[0]
    rows = [
        ((0, 0, 1), (0, 0, 1), False), ((0, 0, 1), w(0.3, 1.0)[0], False), ((0, 0, 1), (0, 0, -1), False),   # the normal
        ((0, 0, 1), w(np.pi - 0.2, 1.0)[0], False), ((0, 0, -1), w(0.2, 1.0)[0], False),
        (tilted, (1, 0, 0), True), (tilted, (0.6, -0.8, 0), True),                                            # co == 0
        ((1, 0, 0), tilted, True), ((0, 1, 0), -tilted, True), ((1, 0, 0), (0, 1, 0), True),                  # ci == 0
        (inside, w(1.0, 0.7 + np.pi)[0], False), (inside, w(0.3, 0.7)[0], False), (inside, inside * [-1, -1, 1], False),
        (tilted, -tilted / eta, True), (graze, -graze / eta, True),                                           # degenerate half vector
        (-tilted, tilted * eta, True),
        (graze, graze * [-1, -1, 1], False), (graze, w(np.pi - 0.72, 0.3 + np.pi)[0], False), (graze, -graze, False),
    ]
    wi, wo, z = zip(*rows)
    return np.array(wi, np.float32), np.array(wo, np.float32), np.array(z)


@pytest.fixture(scope="module")
def gpu():
    from bsdf_diffusion_sampling_amd.analytic import Principled, reference_bsdf
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return {k: Principled(**CUSTOM) if k == "custom" else reference_bsdf(k) for k in MATERIALS}


def make_rows(key):
    """The fp32 inputs of one material and its two numpy models: (wi, wo, u, exactly_zero, r64, r32)."""
    g = np.random.default_rng(SEED[key])
    r64, r32 = R.Principled(dtype=np.float64, **_params(key)), R.Principled(dtype=np.float32, **_params(key))
    # sample(): both sides of the surface, grazing rows included, and the hand-placed incident directions
    hw_i, hw_o, hz = _hand_rows(float(r64.eta))
    wi = R.sphere_dirs(g, N)
    wi[: N // 8] = _unit(wi[: N // 8] * [1, 1, 0.05])        # an eighth of them within ~3 degrees of the horizon
    wi = np.concatenate([wi.astype(np.float32), hw_i])
    u = g.random((len(wi), 3)).astype(np.float32)
    # eval() / pdf(): half of the directions around where the model puts its mass (its own samples, blurred), half anywhere
    wo = R.sphere_dirs(g, len(wi))
    k = N // 2
    own = r64.sample(wi[:k], g.random((k, 3)))[0]
    hit = np.abs(own).sum(1) > 0                              # (a failed sample has no direction: that row stays uniform)
    wo[:k][hit] = _unit(own + g.normal(size=(k, 3)) * 0.5 * float(np.sqrt(r64.ax * r64.ay)))[hit]
    wo = wo.astype(np.float32)
    wo[N:] = hw_o
    return wi, wo, u, np.concatenate([np.zeros(N, bool), hz]), r64, r32


@pytest.fixture(scope="module")
def case(gpu):
    """Per material, computed once and shared (read-only): the fp32 inputs, the fp64 reference, the fp32 yardstick and the kernels'
    results on the same rows."""
    cache = {}

    def get(key):
        if key in cache:
            return cache[key]
        wi, wo, u, zero, r64, r32 = make_rows(key)
        wi_d, wo_d, u_d = _cuda(wi), _cuda(wo), _cuda(u)
        b = gpu[key]
        c = dict(wi=wi, wo=wo, u=u, r64=r64, r32=r32, wi_d=wi_d, wo_d=wo_d, u_d=u_d, zero=zero,
                 eval_d=b.eval_t(wi_d, wo_d, tint=TINT), pdf_d=b.pdf_t(wi_d, wo_d), sample_d=b.sample_t(wi_d, u_d, tint=TINT),
                 sample_ref=r64.sample(wi, u, TINT, details=True), sample_yard=r32.sample(wi, u, TINT, details=True))
        cache[key] = c
        return c
    return get


def _err(got, ref):
    """Per-row error against fp64: relative to max(|ref|, 1e-6 of the column's largest)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max(0))


def _held_to_yardstick(label, got, yard):
    fig = {q: dict(gpu_p99=np.percentile(got[q], 99), yard_p99=np.percentile(yard[q], 99), gpu_max=got[q].max(), yard_max=yard[q].max())
           for q in got}
    msg = label + ": " + "; ".join(f"{q} p99 gpu {f['gpu_p99']:.3e} yardstick {f['yard_p99']:.3e}, max gpu {f['gpu_max']:.3e} "
                                   f"yardstick {f['yard_max']:.3e}" for q, f in fig.items())
    print(msg)
    for q, f in fig.items():
        assert f["gpu_p99"] <= 4 * f["yard_p99"], msg
        assert f["gpu_max"] <= 4 * f["yard_max"], msg


def lobe_classes(wi, wo, f_ref):
    """Share of the random rows on which each class of pair is scored with f > 0."""
    ci, co, pos = wi[:N, 2], wo[:N, 2], f_ref[:N, 0] > 0
    return {"front reflection": ((ci > 0) & (co > 0) & pos).mean(), "back reflection": ((ci < 0) & (co < 0) & pos).mean(),
            "transmission in": ((ci > 0) & (co < 0) & pos).mean(), "transmission out": ((ci < 0) & (co > 0) & pos).mean()}


def close_to_a_threshold(u, details):
    """Rows whose u2 is within 1e-5 of a cumulative threshold of the lobe choice (the last one is the reflection /
    transmission split)."""
    u2 = u[:, 2].astype(np.float64)
    return np.any([np.abs(u2 - t) < 1e-5 for t in details["thresholds"]], axis=0)


@pytest.mark.parametrize("key", MATERIALS)
def test_eval_and_pdf_match_fp64_within_the_fp32_yardstick(case, key):
    c = case(key)
    f, p = _np(c["eval_d"]), _np(c["pdf_d"])
    assert np.isfinite(f).all() and np.isfinite(p).all() and (f >= 0).all() and (p >= 0).all()
    f_ref, p_ref = c["r64"].eval(c["wi"], c["wo"], TINT), c["r64"].pdf(c["wi"], c["wo"])
    f_yard, p_yard = c["r32"].eval(c["wi"], c["wo"], TINT), c["r32"].pdf(c["wi"], c["wo"])
    # every lobe class is scored on a real share of the rows (a metal has nothing below the surface)
    share = lobe_classes(c["wi"], c["wo"], f_ref)
    print(f"{key}: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    assert share["front reflection"] > 0.2
    if key == 2:
        assert share["back reflection"] == share["transmission in"] == share["transmission out"] == 0
        inside = c["wi"][:, 2] < 0
        assert (f[inside] == 0).all() and (p[inside] == 0).all()
    else:
        assert share["back reflection"] > 0.05 and share["transmission in"] > 0.05 and share["transmission out"] > 0.02
    if key == "custom":       # the channels differ, and not by the tint alone
        ratio = f[:N, 1] / TINT[1] / np.maximum(f[:N, 0] / TINT[0], 1e-30)
        assert np.ptp(ratio[f[:N, 0] > 1e-3]) > 0.1
    # the degenerate rows: exactly zero, in the kernels and in both runs of the reference
    z = c["zero"]
    assert z.sum() == 8 and (f[z] == 0).all() and (p[z] == 0).all() and (f_ref[z] == 0).all() and (p_ref[z] == 0).all()
    assert (f_yard[z] == 0).all() and (p_yard[z] == 0).all()
    _held_to_yardstick(f"{key}", {"eval": _err(f, f_ref).max(1), "pdf": _err(p, p_ref)},
                       {"eval": _err(f_yard, f_ref).max(1), "pdf": _err(p_yard, p_ref)})


@pytest.mark.parametrize("key", MATERIALS)
def test_sample_matches_fp64_within_the_fp32_yardstick(case, key):
    c = case(key)
    wo, pdf, w = (_np(t) for t in c["sample_d"])
    wo_r, pdf_r, w_r, d_r = c["sample_ref"]
    wo_y, pdf_y, w_y, d_y = c["sample_yard"]
    assert all(np.isfinite(a).all() for a in (wo, pdf, w)) and (pdf >= 0).all() and (w >= 0).all()
    flat = c["wi"][:, 2] == 0
    assert flat.sum() == 3 and (wo[flat] == 0).all() and (pdf[flat] == 0).all() and (w[flat] == 0).all()
    ok = pdf > 0
    assert (wo[~ok] == 0).all() and (w[~ok] == 0).all()
    assert np.abs(np.linalg.norm(wo[ok].astype(np.float64), axis=1) - 1).max() <= 1e-5
    # rows within 1e-5 of a threshold of the lobe choice: excluded and counted (expected count 0.25)
    close = close_to_a_threshold(c["u"], d_r)
    assert close.sum() <= 4, close.sum()
    rows = ~close
    # the same samples succeed, and each took the reference's lobe: its direction is nearest that candidate
    assert np.array_equal(ok[rows], d_r["ok"][rows]), int((ok != d_r["ok"])[rows].sum())
    lobe = np.linalg.norm(wo[None].astype(np.float64) - d_r["candidates"], axis=2).argmin(0)
    both = rows & ok
    assert np.array_equal(lobe[both], d_r["lobe"][both]), int((lobe != d_r["lobe"])[both].sum())
    taken = np.bincount(d_r["lobe"][both], minlength=4) / both.sum()
    print(f"{key}: {ok.mean():.3f} of the samples succeed; lobes diffuse / clearcoat / transmission / reflection = "
          + " / ".join(f"{t:.3f}" for t in taken))
    if key == 2:
        assert taken[0] == 0 and taken[2] == 0 and taken[1] > 0.02 and not ok[c["wi"][:, 2] < 0].any()
    else:
        assert (taken > 0.02).all()
        # total internal reflection: from inside, a normal hit beyond the critical angle reflects whatever u2 says
        tir = rows & (d_r["F"] == 1.0) & (c["wi"][:, 2] < 0)
        assert tir.sum() >= 50 and (lobe[tir & ok] == R.LOBE_REFLECTION).all() and (c["u"][tir, 2] < 0.1).any()
    yrows = both & (d_y["lobe"] == d_r["lobe"]) & (d_y["ok"] == d_r["ok"])        # (the fp32 yardstick flips on rows of its own)
    got = {"wo": np.abs(wo.astype(np.float64) - wo_r).max(1)[both], "pdf": _err(pdf, pdf_r)[both], "weight": _err(w, w_r).max(1)[both]}
    yard = {"wo": np.abs(wo_y.astype(np.float64) - wo_r).max(1)[yrows], "pdf": _err(pdf_y, pdf_r)[yrows],
            "weight": _err(w_y, w_r).max(1)[yrows]}
    _held_to_yardstick(f"{key} sample", got, yard)


@pytest.mark.parametrize("key", MATERIALS)
def test_the_kernels_agree_bit_for_bit(case, gpu, key):
    c = case(key)
    b = gpu[key]
    wo_d, pdf_d, w_d = c["sample_d"]
    pdf, w = _np(pdf_d), _np(w_d)
    # pdf_t of the sampled pair IS the sampler's pdf (a failed sample has wo = 0, where the density is 0)
    assert torch.equal(b.pdf_t(c["wi_d"], wo_d), pdf_d)
    # the weight is eval_t of the sampled pair over that pdf — IEEE fp32 division, formed here on the host — where the sample
    # succeeded, and exactly 0 elsewhere
    f = _np(b.eval_t(c["wi_d"], wo_d, tint=TINT))
    keep = pdf > 0
    assert 0.2 < keep.mean() < 1 and (w[~keep] == 0).all() and (f[~keep] == 0).all()
    with np.errstate(all="ignore"):
        expect = (f / pdf[:, None]).astype(np.float32)
    assert np.array_equal(w[keep].view(np.uint32), expect[keep].view(np.uint32))
    back = w.astype(np.float64) * pdf.astype(np.float64)[:, None]
    assert (np.abs(back - f)[keep] <= 2.0 ** -23 * f[keep]).all()
    assert (f[keep, 0] > 0).mean() > 0.99


@pytest.mark.parametrize("n", [0, 1, 67])
def test_results_do_not_depend_on_the_grid(case, gpu, n):
    c, b = case(13), gpu[13]
    wi, wo, u = (c[k][:n].contiguous() for k in ("wi_d", "wo_d", "u_d"))
    got = b.sample_t(wi, u, tint=TINT)
    assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].shape == (n, 3)
    for a, full in zip(got, c["sample_d"]):
        assert torch.equal(a, full[:n])
    assert torch.equal(b.eval_t(wi, wo, tint=TINT), c["eval_d"][:n]) and torch.equal(b.pdf_t(wi, wo), c["pdf_d"][:n])


def test_masks_checks_and_call_shapes(case, gpu):
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.plugin_base import FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, BSDFSample3f, SurfaceInteraction
    c, b = case(13), gpu[13]
    n = len(c["wi"])
    wi_d, wo_d, u_d = c["wi_d"], c["wo_d"], c["u_d"]
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.6).cuda()
    out = (torch.full((n, 3), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda"), torch.full((n, 3), 7.0, device="cuda"))
    ret = b.sample_t(wi_d, u_d, tint=TINT, active=mask, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))
    for r, full in zip(ret, c["sample_d"]):
        assert torch.equal(r[mask], full[mask]) and bool((r[~mask] == 0).all())
    p = b.pdf_t(wi_d, wo_d, active=mask.to(torch.uint8))
    assert torch.equal(p[mask], c["pdf_d"][mask]) and bool((p[~mask] == 0).all())
    buf = torch.full((n, 3), 7.0, device="cuda")
    assert b.eval_t(wi_d, wo_d, out=buf, tint=TINT).data_ptr() == buf.data_ptr() and torch.equal(buf, c["eval_d"])
    pdf_sa = c["pdf_d"] * 0.1 + 1e-3
    wgt, pk = b.sample_weight(wi_d, wo_d, pdf_sa, tint=TINT)
    wgt_m, pk_m = b.sample_weight(wi_d, wo_d, pdf_sa, tint=TINT, active=mask)
    assert torch.equal(wgt_m[mask], wgt[mask]) and torch.equal(pk_m[mask], pk[mask])
    assert bool((wgt_m[~mask] == 0).all()) and bool((pk_m[~mask] == 0).all())
    # sample_weight against the reference's lines in fp64: the same rows are kept, the same values to fp32 rounding
    w_r, p_r = c["r64"].sample_weight(c["wi"], c["wo"], _np(pdf_sa), TINT, 3.5)
    v_r = c["r64"].eval(c["wi"], c["wo"], TINT) / _np(pdf_sa).astype(np.float64)[:, None]
    clear = np.abs(v_r[:, 0] - 3.5) > 1e-2
    assert np.array_equal((_np(pk) > 0)[clear], (p_r > 0)[clear]) and (_np(pk)[_np(pk) > 0] == _np(pdf_sa)[_np(pk) > 0]).all()
    assert (p_r == 0).mean() > 0.01 and (p_r > 0).mean() > 0.01
    kept = _np(pk) > 0
    with np.errstate(all="ignore"):
        expect = (_np(c["eval_d"]) / _np(pdf_sa)[:, None]).astype(np.float32)       # IEEE fp32 division of the kernels' own eval
    assert np.array_equal(_np(wgt)[kept].view(np.uint32), expect[kept].view(np.uint32)) and (_np(wgt)[~kept] == 0).all()
    # argument checks
    with pytest.raises(ValueError, match="u must be"):
        b.sample_t(wi_d, wo_d[:, :2].contiguous())
    with pytest.raises(ValueError, match="active"):
        b.sample_t(wi_d, u_d, active=mask[:5])
    with pytest.raises(ValueError, match="rows"):
        b.eval_t(wi_d, wo_d[:5].contiguous())
    import ctypes as C
    bad = _lib.Principled((C.c_float * 3)(1, 1, 1), 0.5, 0.0, 2.0, 0.0, 1.5)
    assert _lib.lib().bsdfd_principled_pdf(C.byref(bad), wi_d.data_ptr(), wo_d.data_ptr(), None, n, p.data_ptr(), None) == 1
    # Mitsuba's call shapes
    si = SurfaceInteraction(wi_d)
    bs, weight = b.sample(None, si, u_d[:, 2].contiguous(), u_d[:, :2].contiguous())
    wo_s, pdf_s, w_s = b.sample_t(wi_d, u_d)
    assert isinstance(bs, BSDFSample3f) and torch.equal(bs.wo, wo_s) and torch.equal(bs.pdf, pdf_s) and torch.equal(weight, w_s)
    d_r = c["sample_ref"][3]
    rows = ~close_to_a_threshold(c["u"], d_r) & d_r["ok"]
    assert np.array_equal(_np(bs.sampled_component)[rows], d_r["lobe"][rows]) and len(np.unique(d_r["lobe"][rows])) == 4
    across = _np(bs.sampled_component)[rows] == R.LOBE_TRANSMISSION
    front = c["wi"][rows, 2] > 0
    eta = float(np.float32(b.eta))
    assert np.allclose(_np(bs.eta)[rows], np.where(across, np.where(front, eta, 1 / eta), 1.0), rtol=1e-6)
    assert np.array_equal(_np(bs.sampled_type)[rows], np.where(across, FLAG_DIFFUSE_TRANSMISSION, FLAG_DIFFUSE_REFLECTION))
    e, q = b.eval_pdf(None, si, wo_d)
    assert torch.equal(e, b.eval_t(wi_d, wo_d)) and torch.equal(q, c["pdf_d"])
    assert torch.equal(e, b.eval(None, si, wo_d)) and torch.equal(q, b.pdf(None, si, wo_d))


# ---- the full-sphere plugin ---------------------------------------------------------------------------------------------------
class _EvalOnly:
    """A ground truth that exposes nothing but ``eval``: the plugin then runs its torch lines."""

    def __init__(self, b):
        self.b = b

    def eval(self, ctx, si, wo):
        return self.b.eval_t(si.wi, wo)


def plugin_inputs(n=4096):
    """(wi [n,3] fp32, x0 fp32): incident directions above the surface and base samples of the shipped net bsdf_13 — half as its
    sampler would draw them, half overdispersed: those land where the net's density is far below the model's, which is where the
    firefly rule bites."""
    from bsdf_diffusion_sampling_amd import weights as W
    from oracle import bsdf_oracle as O
    g = np.random.default_rng(5)
    th, ph = g.uniform(0.05, 1.5, n), g.uniform(-np.pi, np.pi, n)
    wi = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1).astype(np.float32)
    orc = O.Oracle(W.load(W.shipped_path("bsdf_13", "spherical")))
    cond = O.cart_to_spher(wi.astype(np.float64))
    mu, kappa = orc.base_von_mises_params(cond)
    x0 = orc.base_sample(cond, g.standard_normal(n), phi=g.vonmises(mu, kappa))
    # (six standard deviations wide: on the CPU oracle against the fp64 model the rule then cuts 2.1 % of the rows and spares 66 %;
    # the fp32 flow on the device: 1.5 % and 66 %)
    x0[n // 2:] = orc.base_sample(cond, 6.0 * g.standard_normal(n), phi=g.uniform(-np.pi, np.pi, n))[n // 2:]
    return wi, x0.astype(np.float32)


def test_plugin_sample_weight_is_the_torch_lines_bit_for_bit(gpu):
    from bsdf_diffusion_sampling_amd.analytic import Principled
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    from bsdf_diffusion_sampling_amd.plugin_base import SurfaceInteraction
    wi, x0 = plugin_inputs()
    x0_d, si = _cuda(x0), SurfaceInteraction(_cuda(wi))
    fused = MyBSDF({"idx": 13, "albedo": list(TINT), "analytic": "all"})
    assert isinstance(fused.bsdf, Principled) and fused.bsdf.roughness == 0.7 and fused._fused_gt() is fused.bsdf
    torch_lines = MyBSDF({"idx": 13, "albedo": list(TINT), "bsdf": _EvalOnly(fused.bsdf)})
    assert torch_lines._fused_gt() is None
    bs_a, w_a = fused.sample(None, si, x0=x0_d)
    bs_b, w_b = torch_lines.sample(None, si, x0=x0_d)
    assert torch.equal(bs_a.wo, bs_b.wo)
    kept = float((bs_b.pdf > 0).float().mean())
    pdf_sa = fused.sample_t(si.wi, x0=x0_d)[1]   # the density before the rule
    value_x = fused.bsdf.eval_t(si.wi, bs_a.wo, tint=TINT)[:, 0] / pdf_sa
    below = float(((value_x < 3.5) & (pdf_sa > 0) & (value_x > 0)).float().mean())
    above = float(((value_x >= 3.5) & (pdf_sa > 0)).float().mean())
    print(f"value.x below the threshold on {below:.3f} of the rows, at or above it on {above:.3f}; pdf kept on {kept:.3f}")
    assert below >= 0.01 and above >= 0.01
    assert torch.equal(bs_a.pdf.view(torch.int32), bs_b.pdf.view(torch.int32))
    assert torch.equal(w_a.view(torch.int32), w_b.view(torch.int32))
    assert bool((bs_a.pdf[value_x >= 3.5] == 0).all()) and bool((w_a[bs_a.pdf == 0] == 0).all())
    # eval(): one launch, the tint inside
    assert torch.equal(fused.eval(None, si, bs_a.wo), fused.bsdf.eval_t(si.wi, bs_a.wo, tint=TINT))
    assert torch.allclose(fused.eval(None, si, bs_a.wo), torch_lines.eval(None, si, bs_a.wo), rtol=1e-6, atol=0)


def test_plugin_defaults_stay_and_all_is_opt_in():
    from bsdf_diffusion_sampling_amd.analytic import Principled, RoughDielectric
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    from bsdf_diffusion_sampling_amd.plugin_base import SurfaceInteraction
    from bsdf_diffusion_sampling_amd.wavefront import WavefrontRenderer
    wi = _cuda(R.wi_of(0.5, 0.2, 64).astype(np.float32))
    p13 = MyBSDF({"idx": 13})
    assert p13.bsdf is None and p13.sample(None, SurfaceInteraction(wi), seed=1)[1] is None
    assert MyBSDF({"idx": 13, "analytic": True}).bsdf is None and MyBSDF({"idx": 13, "analytic": False}).bsdf is None
    on = MyBSDF({"idx": 13, "analytic": "all"})
    assert isinstance(on.bsdf, Principled)
    bs, w = on.sample(None, SurfaceInteraction(wi), seed=1)
    assert w is not None and w.shape == (64, 3) and bool(torch.isfinite(w).all())
    assert on.eval(None, SurfaceInteraction(wi), bs.wo).shape == (64, 3)
    assert isinstance(MyBSDF({"idx": 24, "analytic": "all"}).bsdf, RoughDielectric)
    assert isinstance(MyBSDF({"idx": 0, "analytic": "all"}).bsdf, Principled)
    with pytest.raises(ValueError, match="'all'"):
        MyBSDF({"idx": 13, "analytic": "some"})
    # the wavefront renderer shades such a plugin with the proxy, as it does without the evaluator
    assert WavefrontRenderer(on).use_ground_truth is False


@pytest.fixture(scope="module")
def sphere20k():
    return _cuda(R.sphere_dirs(np.random.default_rng(2), 20000).astype(np.float32))


IDENTIFY = (1, 6, 13, 17)


@pytest.mark.parametrize("idx", IDENTIFY)
def test_the_nets_identify_their_material(sphere20k, idx):
    """L1 distance between the normalised density of the shipped net (the full-sphere plugin's pdf, T = 8) and the normalised
    model on 20 000 uniform directions, for the four rough entries: smallest at the net's own.  On the CPU oracle against the fp64
    model the own distance is 0.14-0.64 and the nearest other 0.57 or more, never closer than the own."""
    from bsdf_diffusion_sampling_amd.analytic import reference_bsdf
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    plug = MyBSDF({"idx": idx})
    models = {i: reference_bsdf(i) for i in IDENTIFY}
    assert plug.T == 8 and plug.bsdf is None
    for theta in (0.3, 1.0):
        wi = _cuda(R.wi_of(theta, 0.0, 20000).astype(np.float32))
        p = plug.pdf_t(wi, sphere20k).double()
        p = p / p.sum()
        dist = {}
        for i, b in models.items():
            q = b.eval_t(wi, sphere20k)[:, 0].double()
            dist[i] = float((p - q / q.sum()).abs().sum())
        print(f"bsdf_{idx} theta_i {theta}: L1 to idx " + " / ".join(f"{i}: {dist[i]:.2f}" for i in IDENTIFY))
        assert min(dist, key=dist.get) == idx, dist
