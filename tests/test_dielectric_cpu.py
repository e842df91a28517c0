"""CPU: the rough-dielectric model as tests/dielectric_ref.py states it in fp64 — the reference the kernels of csrc/dielectric.hip
are held to on the GPU (tests/test_gpu_dielectric.py) — checked against what the model itself promises: reciprocity, energy
conservation, and a sampler whose density is its pdf.  And the host side that needs no GPU: ``analytic.reference_material``."""
import os

import numpy as np
import pytest

import dielectric_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = (0.2, 0.3, 0.5)
ETA0 = R.ETA_BK7_AIR


def test_reciprocity():
    """f(wi, wo) = f(wo, wi) on reflection pairs (either side); across the surface, radiance transport scales by the squared
    index: f(wo, wi) = eta0^2 f(wi, wo) for wi outside.  1e-9 relative, on 100 000 random pairs per alpha."""
    g = np.random.default_rng(3)
    for alpha in ALPHAS:
        m = R.RoughDielectric(alpha)
        wi, wo = R.sphere_dirs(g, 100_000), R.sphere_dirs(g, 100_000)
        a = m.f_cos(wi, wo) / np.abs(wo[:, 2])
        b = m.f_cos(wo, wi) / np.abs(wi[:, 2])
        refl = wi[:, 2] * wo[:, 2] > 0
        trans = (wi[:, 2] > 0) & (wo[:, 2] < 0)
        assert refl.sum() > 40_000 and trans.sum() > 20_000
        assert (a[refl] > 0).sum() > 10_000 and (a[trans] > 0).sum() > 1_000   # (the lobes are narrow)
        for rows, left, right in ((refl, a, b), (trans, ETA0 ** 2 * a, b)):
            err = np.abs(left - right)[rows] / np.maximum(np.maximum(np.abs(left), np.abs(right))[rows], 1e-300)
            assert err.max() <= 1e-9, (alpha, err.max())


@pytest.fixture(scope="module")
def sphere():
    """2^20 directions uniform on the sphere, shared (read-only) by the integrals below."""
    return R.sphere_dirs(np.random.default_rng(11), 1 << 20)


def _sphere_integral(values):
    """Uniform-sphere estimate of an integral over directions and its standard error."""
    x = 4 * np.pi * values
    return x.mean(), x.std() / np.sqrt(len(x))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_energy(sphere, alpha):
    """For wi outside, the reflected energy plus the transmitted one (radiance mode divides the transmitted radiance by eta0^2)
    does not exceed what arrives: R + eta0^2 T <= 1 within 4 standard errors."""
    m = R.RoughDielectric(alpha)
    for theta in (0.0, 0.3, 1.0, 1.3, 1.5):
        wi = R.wi_of(theta, 0.4, len(sphere))
        fc = m.f_cos(wi, sphere)
        total, se = _sphere_integral(np.where(sphere[:, 2] > 0, fc, ETA0 ** 2 * fc))
        assert 0.3 < total <= 1 + 4 * se, (alpha, theta, total, se)


@pytest.mark.parametrize("alpha", (0.2, 0.5))
@pytest.mark.parametrize("theta", (0.0, 0.3, 1.0, 1.4))
def test_sampler_has_the_density_pdf_states(sphere, theta, alpha):
    """E[g(wo)] over 65 536 samples against the uniform-sphere estimate of the integral of g * pdf, for three bounded g; the
    bound is 4 sqrt(se_a^2 + se_b^2).  A sample whose direction ends up on the wrong side of the surface for its lobe (a
    reflection below it, a refraction above it) is a failed one — its weight is 0 — and counts as g = 0: pdf(wi, wo) is the
    density of the others (at such a wo it describes the OTHER lobe's geometry)."""
    m = R.RoughDielectric(alpha)
    n = 65536
    g = np.random.default_rng(int(1000 * theta) + int(10 * alpha))
    wi = R.wi_of(theta, -2.0, n)
    wo, pdf, w, refl, F = m.sample(wi, g.random((n, 3)), details=True)
    valid = np.where(refl, wi[:, 2] * wo[:, 2] > 0, wi[:, 2] * wo[:, 2] < 0)
    assert np.isfinite(wo).all() and np.isfinite(pdf).all() and np.isfinite(w).all() and (pdf > 0).mean() > 0.95
    assert valid.mean() > 0.8 and (w[~valid] == 0).all() and (w[valid & (pdf > 0)] > 0).mean() > 0.99
    assert np.abs(np.linalg.norm(wo, axis=1) - 1).max() < 1e-12
    p = m.pdf(R.wi_of(theta, -2.0, len(sphere)), sphere)
    for name, fn in (("upper", lambda d: (d[:, 2] > 0).astype(np.float64)), ("x^2", lambda d: d[:, 0] ** 2), ("z^2", lambda d: d[:, 2] ** 2)):
        a = fn(wo) * valid
        mean_a, se_a = a.mean(), a.std() / np.sqrt(n)
        mean_b, se_b = _sphere_integral(fn(sphere) * p)
        print(f"theta {theta} alpha {alpha} {name}: sampled {mean_a:.5f} +- {se_a:.5f}, integral {mean_b:.5f} +- {se_b:.5f}")
        assert abs(mean_a - mean_b) <= 4 * np.hypot(se_a, se_b), (name, mean_a, se_a, mean_b, se_b)


def test_sample_weight_is_eval_over_pdf_and_total_internal_reflection():
    """The weight is f |cos| / pdf of the returned pair and vanishes exactly where the lobe's side test fails; total internal reflection."""
    m = R.RoughDielectric(0.3)
    g = np.random.default_rng(5)
    wi = R.sphere_dirs(g, 20000)
    wo, pdf, w, refl, F = m.sample(wi, g.random((20000, 3)), tint=(0.9, 0.2, 0.4), details=True)
    side = np.where(refl, wi[:, 2] * wo[:, 2] > 0, wi[:, 2] * wo[:, 2] < 0)
    keep = side & (pdf > 0)
    assert 0.5 < keep.mean() < 1 and (w[~keep] == 0).all()
    assert np.array_equal(w[keep], m.eval(wi, wo, (0.9, 0.2, 0.4))[keep] / pdf[keep, None])
    assert np.array_equal(pdf, m.pdf(wi, wo))
    # from inside, beyond the critical angle (sin = 1 / eta0 = 0.665): wherever the sampled normal is hit beyond it too, Fresnel
    # is exactly 1 and the sample reflects, whatever u2 says.  (A transmission PAIR never sees this: its generalised half vector
    # always has |wi . m| >= the critical cosine.)
    n = 4096
    wi_in = R.wi_of(np.pi - 1.2, 0.7, n)
    u = g.random((n, 3))
    u[:, 2] = 1 - 2.0 ** -53
    wo, pdf, w, refl, F = m.sample(wi_in, u, details=True)
    tir = F == 1.0
    assert tir.mean() > 0.5 and refl[tir].all() and not refl[~tir].any()
    assert (wo[tir & (pdf > 0), 2] < 0).mean() > 0.9


def test_reference_material():
    """idx 23 / 24 / 25: the reference's three rough dielectrics; 0..22: principled, not built; anything else: no such entry."""
    from bsdf_diffusion_sampling_amd import analytic
    for idx, alpha in R.REFERENCE_ALPHA.items():
        b = analytic.reference_material(idx)
        assert isinstance(b, analytic.RoughDielectric) and b.alpha == alpha and b.distribution == "beckmann"
        assert b.int_ior == analytic.IOR["bk7"] == 1.5046 and b.ext_ior == analytic.IOR["air"] == 1.000277
        assert float(np.float32(b.eta)) == ETA0 and b._desc.distribution == 0
        assert np.float32(b._desc.alpha) == np.float32(alpha) and np.float32(b._desc.eta) == np.float32(ETA0)
    assert set(analytic.IOR) == {"bk7", "air", "vacuum"} and analytic.IOR == R.IOR
    for idx in (0, 3, 22):
        with pytest.raises(NotImplementedError, match="principled"):
            analytic.reference_material(idx)
    for idx in (-1, 26, 100):
        with pytest.raises(IndexError):
            analytic.reference_material(idx)
    with pytest.raises(ValueError, match="beckmann"):
        analytic.RoughDielectric(0.2, distribution="ggx")
    with pytest.raises(ValueError, match="index of refraction"):
        analytic.RoughDielectric(0.2, int_ior="diamond-ish")


def test_library_declares_and_exports_the_entry_points():
    import ctypes as C
    from bsdf_diffusion_sampling_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    L = _lib.lib()
    for name in ("bsdfd_dielectric_eval", "bsdfd_dielectric_sample_weight", "bsdfd_dielectric_sample", "bsdfd_dielectric_pdf"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    src, dev = os.path.join(csrc, "dielectric.hip"), os.path.join(csrc, "dielectric_dev.h")
    assert src in _lib.SRC_PATHS and src not in _lib.FLOW_TUS and src not in _lib.KERNEL_SOURCES and os.path.exists(src)
    assert dev in _lib.DEP_PATHS and dev not in _lib.SRC_PATHS and os.path.exists(dev)
    assert C.sizeof(_lib.Dielectric) == 16 and [n for n, _ in _lib.Dielectric._fields_] == ["alpha", "eta", "distribution", "reserved"]
    # the launchers check the descriptor before anything touches a device: no GPU is needed to be refused
    bad = _lib.Dielectric(0.3, 1.5, 1, 0)
    assert L.bsdfd_dielectric_eval(C.byref(bad), None, None, 0, None, None, None) == 1   # BSDFD_EINVAL
    assert b"Beckmann" in L.bsdfd_last_error()
    assert L.bsdfd_dielectric_eval(C.byref(_lib.Dielectric(0.3, 1.5, 0, 0)), None, None, 0, None, None, None) == 0   # N = 0: a no-op
