"""CPU: the principled model as tests/principled_ref.py states it in fp64 — the reference the kernels of csrc/principled.hip are
held to on the GPU (tests/test_gpu_principled.py) — checked against what the model itself promises: reciprocity, a sampler whose
density is its pdf and whose weight is eval / pdf, and the statements that are exact.  And the host side that needs no GPU:
``analytic.Principled``, ``analytic.reference_bsdf``, the descriptor's checks, and the compiler's account of the four kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import principled_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsdfd_principled_eval", "bsdfd_principled_sample_weight", "bsdfd_principled_sample", "bsdfd_principled_pdf")
KERNELS = ("principled_eval_kernel", "principled_weight_kernel", "principled_sample_kernel", "principled_pdf_kernel")


@pytest.mark.parametrize("idx", (1, 5, 13, 21))
def test_reciprocity(idx):
    """f(wi, wo) = f(wo, wi) with both directions above the surface and with both below; across it, radiance transport scales
    by the squared index: f(wo, wi) = eta^2 f(wi, wo) for wi outside, and the two are zero on the same rows.  1e-9 relative, on
    100 000 random pairs."""
    g = np.random.default_rng(3 + idx)
    m = R.reference(idx)
    wi, wo = R.sphere_dirs(g, 100_000), R.sphere_dirs(g, 100_000)
    a = m.eval(wi, wo)[:, 0] / np.abs(wo[:, 2])
    b = m.eval(wo, wi)[:, 0] / np.abs(wi[:, 2])
    above = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    below = (wi[:, 2] < 0) & (wo[:, 2] < 0)
    across = (wi[:, 2] > 0) & (wo[:, 2] < 0)
    assert above.sum() > 20_000 and below.sum() > 20_000 and across.sum() > 20_000
    assert (a[above] > 0).all() and (a[below] > 0).sum() > 30 and (a[across] > 0).sum() > 30     # (narrow lobes at idx 5)
    assert np.array_equal(a[across] == 0, b[across] == 0)
    worst = {}
    for name, rows, left in (("above", above, a), ("below", below, a), ("across", across, float(m.eta) ** 2 * a)):
        err = np.abs(left - b)[rows] / np.maximum(np.maximum(np.abs(left), np.abs(b))[rows], 1e-300)
        worst[name] = err.max()
    print(f"idx {idx}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-9, worst


@pytest.fixture(scope="module")
def sphere():
    """2^20 directions uniform on the sphere, shared (read-only) by the integrals below."""
    return R.sphere_dirs(np.random.default_rng(11), 1 << 20)


def _sphere_integral(values):
    """Uniform-sphere estimate of an integral over directions and its standard error."""
    x = 4 * np.pi * values
    return x.mean(), x.std() / np.sqrt(len(x))


THETAS = (0.3, 1.0, 1.4, np.pi - 0.4, np.pi - 1.2)


@pytest.mark.parametrize("idx", (1, 13, 17, 21))
@pytest.mark.parametrize("theta", THETAS)
def test_sampler_has_the_density_pdf_states(sphere, theta, idx):
    """E[g(wo)] over 65 536 samples against the uniform-sphere estimate of the integral of g * pdf for three bounded g, E[weight]
    against the integral of eval, and the share of successful samples against the integral of pdf; a failed sample counts as 0.
    Every bound is 4 hypot(se_a, se_b).  (Not on the roughness-0.1 entries: a uniform sphere of this size puts a few dozen points
    in their lobe.)"""
    m = R.reference(idx)
    n = 65536
    g = np.random.default_rng(int(1000 * theta) + idx)
    wi = R.wi_of(theta, -2.0, n)
    wo, pdf, w, d = m.sample(wi, g.random((n, 3)), details=True)
    ok = d["ok"]
    assert np.isfinite(wo).all() and np.isfinite(pdf).all() and np.isfinite(w).all()
    assert np.array_equal(ok, pdf > 0) and (wo[~ok] == 0).all() and (w[~ok] == 0).all()
    assert np.abs(np.linalg.norm(wo[ok], axis=1) - 1).max() < 1e-12
    wi_s = R.wi_of(theta, -2.0, len(sphere))
    p = m.pdf(wi_s, sphere)
    fc = m.eval(wi_s, sphere)[:, 0]
    z = {}
    for name, fn in (("upper", lambda v: (v[:, 2] > 0).astype(np.float64)), ("x^2", lambda v: v[:, 0] ** 2), ("z^2", lambda v: v[:, 2] ** 2),
                     ("share", lambda v: np.ones(len(v)))):
        a = fn(wo) * ok
        mean_a, se_a = a.mean(), a.std() / np.sqrt(n)
        mean_b, se_b = _sphere_integral(fn(sphere) * p)
        z[name] = (mean_a - mean_b) / np.hypot(se_a, se_b)
        assert abs(mean_a - mean_b) <= 4 * np.hypot(se_a, se_b), (name, mean_a, se_a, mean_b, se_b)
    mean_a, se_a = w[:, 0].mean(), w[:, 0].std() / np.sqrt(n)
    mean_b, se_b = _sphere_integral(fc)
    z["weight"] = (mean_a - mean_b) / np.hypot(se_a, se_b)
    print(f"idx {idx} theta {theta:.2f}: success share {ok.mean():.3f}, largest weight {w.max():.2f}, z " +
          ", ".join(f"{k} {v:+.2f}" for k, v in z.items()))
    assert abs(mean_a - mean_b) <= 4 * np.hypot(se_a, se_b), ("weight", mean_a, se_a, mean_b, se_b)
    assert 0.3 < ok.mean() <= 1


def test_exact_statements():
    g = np.random.default_rng(5)
    n = 20000
    wi = R.sphere_dirs(g, n)
    u = g.random((n, 3))
    tint = (0.9, 0.2, 0.4)
    for idx in (1, 5, 13):
        m = R.reference(idx)
        wo, pdf, w, d = m.sample(wi, u, tint=tint, details=True)
        ok = d["ok"]
        # the weight is eval / pdf of the returned pair, pdf() of that pair is the sampler's pdf: bit for bit
        assert 0.3 < ok.mean() < 1 and (w[~ok] == 0).all() and (pdf[~ok] == 0).all() and (wo[~ok] == 0).all()
        assert np.array_equal(w[ok], m.eval(wi, wo, tint)[ok] / pdf[ok, None])
        assert np.array_equal(pdf, m.pdf(wi, wo))
        # the lobe thresholds: p_d and p_d + p_c over a sum that is a constant of the material, 0 from inside
        cum_d, cum_c, cum_t = d["thresholds"]
        front = wi[:, 2] > 0
        total = 1 + 0.25 * float(m.clearcoat) + float(m.brdf)
        assert np.ptp(cum_d[front]) == 0 and np.ptp(cum_c[front]) == 0 and (cum_d[~front] == 0).all() and (cum_c[~front] == 0).all()
        assert cum_d[front][0] == pytest.approx(float(m.brdf) / total, rel=1e-12)
        assert cum_c[front][0] == pytest.approx((float(m.brdf) + 0.25 * float(m.clearcoat)) / total, rel=1e-12)
        assert (cum_t >= cum_c).all() and (cum_t <= 1 + 1e-12).all()
        lobe = d["lobe"]
        assert np.array_equal(lobe == 0, u[:, 2] < cum_d) and np.array_equal(lobe <= 1, u[:, 2] < cum_c)
        assert all((lobe[front] == k).mean() > 0.01 for k in range(4)) and set(np.unique(lobe[~front])) == {2, 3}
        # the Schlick term is only ever taken at c >= 0, where Mitsuba's two-sided statement is r0 + (1 - r0) sw(c)
        c = g.random(1000)
        assert np.allclose(m.schlick_general(0.04, c), 0.04 + 0.96 * m.sw(c), rtol=1e-12, atol=0)


def test_a_metal_has_no_diffuse_sheen_or_transmission_and_nothing_inside():
    """idx 2 (metallic 1): above the surface the specular and clearcoat lobes alone; eval, pdf and samples all zero from inside."""
    g = np.random.default_rng(6)
    n = 20000
    m = R.reference(2)
    assert m.brdf == 0 and m.bsdf == 0
    wi, wo = R.sphere_dirs(g, n), R.sphere_dirs(g, n)
    f, p = m.eval(wi, wo), m.pdf(wi, wo)
    inside = wi[:, 2] < 0
    across = wi[:, 2] * wo[:, 2] < 0
    assert (f[inside | across] == 0).all() and (p[inside | across] == 0).all() and (f[~inside & ~across] > 0).mean() > 0.5
    # what is left above is the specular and clearcoat lobes: the parameters of the others change nothing
    bare = R.Principled(**dict(R.reference_params(2), sheen=0.0, sheen_tint=0.0, flatness=0.0, spec_trans=0.0))
    assert np.array_equal(bare.eval(wi, wo), f) and np.array_equal(bare.pdf(wi, wo), p)
    wo_s, pdf_s, w_s, d = m.sample(wi, g.random((n, 3)), details=True)
    assert (wo_s[inside] == 0).all() and (pdf_s[inside] == 0).all() and (w_s[inside] == 0).all()
    assert set(np.unique(d["lobe"][~inside])) == {1, 3} and (pdf_s[~inside] > 0).mean() > 0.5


def test_total_internal_reflection_reflects_whatever_u2_says():
    m = R.reference(13)
    g = np.random.default_rng(7)
    n = 4096
    wi_in = R.wi_of(np.pi - 1.2, 0.7, n)        # from inside, beyond the critical angle
    u = g.random((n, 3))
    u[:, 2] = np.where(np.arange(n) % 2 == 0, 0.0, 1 - 2.0 ** -53)
    wo, pdf, w, d = m.sample(wi_in, u, details=True)
    tir = d["F"] == 1.0
    assert tir.mean() > 0.3 and (d["lobe"][tir] == R.LOBE_REFLECTION).all() and (d["lobe"][~tir & (u[:, 2] == 0)] == R.LOBE_TRANSMISSION).all()
    assert (wo[tir & d["ok"], 2] < 0).all() and d["ok"][tir].mean() > 0.5


# ---- the host side -------------------------------------------------------------------------------------------------------
def test_reference_bsdf_and_the_constructor():
    from bsdf_diffusion_sampling_amd import analytic
    for idx in (0, 3, 7, 22):
        b = analytic.reference_bsdf(idx)
        metallic, specular, roughness, anisotropic = R.REFERENCE_ROWS[idx]
        assert isinstance(b, analytic.Principled) and (b.metallic, b.roughness, b.anisotropic) == (metallic, roughness, anisotropic)
        assert b.eta == pytest.approx(R.eta_of_specular(specular), rel=1e-15) and b.base_color == (1.0, 1.0, 1.0)
        assert (b.spec_tint, b.sheen, b.clearcoat, b.clearcoat_gloss, b.spec_trans, b.flatness) == (.5, .5, .5, .5, .9, 1.0)
        assert b.sheen_tint == (0.3 if idx == 7 else 0.5)
        assert analytic.REFERENCE_PRINCIPLED[idx] == R.REFERENCE_ROWS[idx]
        r = R.reference(idx)
        for k in R.PARAMS:
            assert np.float32(getattr(b._desc, k)) == np.float32(getattr(r, k)), k
        assert tuple(np.float32(c) for c in b._desc.base_color) == (1.0, 1.0, 1.0)
    assert sorted(analytic.REFERENCE_PRINCIPLED) == list(range(23)) and analytic.REFERENCE_PRINCIPLED[3] == (.2, .3, .3, .7)
    b23 = analytic.reference_bsdf(23)
    assert isinstance(b23, analytic.RoughDielectric) and b23.alpha == 0.2
    for idx in (-1, 26, 100):
        with pytest.raises(IndexError):
            analytic.reference_bsdf(idx)
    for idx in (0, 3, 22):       # the existing call keeps its meaning, and says where to go
        with pytest.raises(NotImplementedError, match="reference_bsdf"):
            analytic.reference_material(idx)
    # derived values: specular 1 is the reference plugin's 1.788; roughness^2 / aspect and roughness^2 * aspect
    b0, b5 = analytic.reference_bsdf(0), analytic.reference_bsdf(5)
    assert b0.eta == pytest.approx(2 / (1 - np.sqrt(0.08)) - 1, rel=1e-15) and abs(b0.eta - 1.788) < 1e-3 and b5.eta == b0.eta
    assert (b0.ax, b0.ay) == pytest.approx((0.04 / np.sqrt(0.55), 0.04 * np.sqrt(0.55)), rel=1e-12)
    assert (b5.ax, b5.ay) == pytest.approx((0.01 / np.sqrt(0.37), 0.01 * np.sqrt(0.37)), rel=1e-12)
    assert (b5.ax, b5.ay) == pytest.approx((float(R.reference(5).ax), float(R.reference(5).ay)), rel=1e-6)
    assert analytic.Principled(roughness=0.01).ax == 1e-3
    with pytest.raises(ValueError, match="specular"):
        analytic.Principled(specular=0.5, eta=1.5)
    with pytest.raises(ValueError, match="spec_trans"):
        analytic.Principled(eta=1.0, spec_trans=0.5)
    assert analytic.Principled(eta=1.0).eta == 1.0
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        analytic.Principled(metallic=1.5)
    with pytest.raises(ValueError, match="eta"):
        analytic.Principled(eta=0.9)


def test_library_declares_and_exports_the_entry_points():
    import ctypes as C
    from bsdf_diffusion_sampling_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    assert "bsdfd_principled;" in hdr and _lib.ABI_VERSION == 8 and L.bsdfd_abi_version() == 8
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    src, dev = os.path.join(csrc, "principled.hip"), os.path.join(csrc, "principled_dev.h")
    assert src in _lib.SRC_PATHS and src not in _lib.FLOW_TUS and src not in _lib.KERNEL_SOURCES and os.path.exists(src)
    assert dev in _lib.DEP_PATHS and dev not in _lib.SRC_PATHS and os.path.exists(dev)
    assert C.sizeof(_lib.Principled) == 64
    assert [n for n, _ in _lib.Principled._fields_] == ["base_color", *R.PARAMS, "reserved"]

    def desc(**kw):
        p = dict(R.reference_params(13), **kw)
        return _lib.Principled((C.c_float * 3)(*p["base_color"]), *[p[k] for k in R.PARAMS])

    # the launchers check the descriptor before anything touches a device: no GPU is needed to be refused
    for bad, word in ((desc(metallic=1.5), b"[0, 1]"), (desc(roughness=float("nan")), b"finite"), (desc(eta=0.8), b"eta"),
                      (desc(eta=1.0), b"spec_trans"), (desc(base_color=(1.0, -0.1, 1.0)), b"[0, 1]")):
        for name in NAMES:
            args = {"bsdfd_principled_eval": (None, None, 0, None, None, None),
                    "bsdfd_principled_sample_weight": (None, None, None, None, 0, None, 3.5, None, None, None),
                    "bsdfd_principled_sample": (None, None, None, 0, None, None, None, None, None),
                    "bsdfd_principled_pdf": (None, None, None, 0, None, None)}[name]
            assert getattr(L, name)(C.byref(bad), *args) == 1     # BSDFD_EINVAL
            assert word in L.bsdfd_last_error(), (word, L.bsdfd_last_error())
    assert L.bsdfd_principled_eval(None, None, None, 0, None, None, None) == 1
    assert L.bsdfd_principled_eval(C.byref(desc()), None, None, 0, None, None, None) == 0       # N = 0: a no-op
    assert L.bsdfd_principled_pdf(C.byref(desc(eta=1.0, spec_trans=0.0)), None, None, None, 0, None, None) == 0
    assert L.bsdfd_principled_eval(C.byref(desc()), None, None, -1, None, None, None) == 1


def test_the_kernels_need_no_scratch():
    """Cross-compile csrc/principled.hip for gfx950 and read the compiler's resource report: 0 bytes of scratch on all four."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import tempfile
    from bsdf_diffusion_sampling_amd import _lib
    with tempfile.TemporaryDirectory(prefix="principled_cc_") as td:
        cmd = ["hipcc", *_lib.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-I", _lib.INCLUDE_DIR, "-c",
               os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc", "principled.hip"), "-o", os.path.join(td, "principled.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for block in text.split("Function Name: ")[1:]:
        name = next((k for k in KERNELS if re.search(r"\d+" + k + "E", block.split()[0])), None)
        if name:
            grab = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
            seen[name] = (grab(r" VGPRs"), grab(r"ScratchSize \[bytes/lane\]"), grab(r"Occupancy \[waves/SIMD\]"))
    print(", ".join(f"{k}: {v[0]} VGPRs, {v[1]} B scratch, {v[2]} waves/SIMD" for k, v in seen.items()))
    assert sorted(seen) == sorted(KERNELS)
    assert all(v[1] == 0 for v in seen.values()), seen
