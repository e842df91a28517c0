"""CPU side of the environment map's importance sampler (bsdf_diffusion_sampling_amd/envmap.py, csrc/pathenv.hip): the table
builder against the reference's (tests/envmap_ref.py), the properties the distribution is built for — exact CDF ends, a density
that is positive wherever the bilinear lookup is, an unbiased estimator — the reference against its own fp32 run, and the host's
refusals.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounce_ref as B
import envmap_ref as ER
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from oracle.wavefront_oracle import env_lookup
from test_pathtrace_cpu import STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bsdfd_env_sample", "bsdfd_env_pdf", "bsdfd_wf_sample_env", "bsdfd_wf_bounce_env")
VERTEX = ("org", "nrm", "wi", "material")


def _sky(h, w, seed):
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    return make_sky(h, w, seed=seed).numpy()


def _half_black(h=64, w=128, seed=5):
    env = _sky(h, w, seed).copy()
    env[h // 2:] = 0.0
    return env


MAPS = {"sky16x32": lambda: _sky(16, 32, 3), "sky64x128": lambda: _sky(64, 128, 5), "half_black": _half_black,
        "2x4": lambda: _sky(2, 4, 1), "13x29": lambda: _sky(13, 29, 2)}


@pytest.fixture(scope="module")
def maps():
    out = {}
    for name, make in MAPS.items():
        env = make()
        out[name] = (env, ER.build_tables(env))
    return out


def test_library_exports_the_environment_kernels_without_a_new_abi():
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert all(name + "()" in note for name in SYMBOLS)
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr
    assert C.sizeof(_lib.WfScene) == 616 and C.sizeof(_lib.WfLights) == 200
    assert len(L.bsdfd_wf_sample_env.argtypes) == 19 and len(L.bsdfd_wf_bounce_env.argtypes) == len(L.bsdfd_wf_bounce_lit.argtypes) + 2
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    assert os.path.join(csrc, "pathenv.hip") in _lib.SRC_PATHS and os.path.join(csrc, "env_dev.h") in _lib.DEP_PATHS


def test_distribution_struct_mirrors_the_header(tmp_path):
    """_lib.EnvDist has the size and the field offsets gcc gives bsdfd_env_dist."""
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from bsdf_diffusion_sampling_amd import _lib
    names = [n for n, _ in _lib.EnvDist._fields_]
    assert names == ["marginal", "conditional", "pdf_uv", "width", "height"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bsdfd.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(bsdfd_env_dist));']
    src += [f'  printf("{f} %zu\\n", offsetof(bsdfd_env_dist, {f}));' for f in names] + ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.EnvDist) == 32
    for f in names:
        assert int(got[f]) == getattr(_lib.EnvDist, f).offset, f


@pytest.mark.parametrize("name", list(MAPS))
def test_table_builder_equals_the_reference(maps, name):
    from bsdf_diffusion_sampling_amd.envmap import EnvDistribution, build_tables
    env, want = maps[name]
    got = build_tables(env)
    h, w = env.shape[:2]
    assert got["marginal"].shape == (h + 1,) and got["conditional"].shape == (h, w + 1) and got["pdf_uv"].shape == (h, w)
    for k in ("marginal", "conditional", "pdf_uv"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), k
    import torch
    d = EnvDistribution(torch.from_numpy(env))
    assert (d.height, d.width) == (h, w) and all(np.array_equal(d.tables[k], want[k]) for k in want)


@pytest.mark.parametrize("name", list(MAPS))
def test_cdfs_are_exact_at_their_ends_and_the_density_averages_to_one(maps, name):
    env, t = maps[name]
    assert t["marginal"][0] == 0.0 and t["marginal"][-1] == 1.0
    assert (t["conditional"][:, 0] == 0.0).all() and (t["conditional"][:, -1] == 1.0).all()
    assert (np.diff(t["marginal"]) >= 0).all() and (np.diff(t["conditional"], axis=1) >= 0).all()
    assert abs(t["pdf_uv"].astype(np.float64).mean() - 1.0) < 1e-6
    # the CDFs are the density's: the probability of a cell, from the tables' widths, is pdf_uv / (W H)
    h, w = t["pdf_uv"].shape
    prob = np.diff(t["marginal"].astype(np.float64))[:, None] * np.diff(t["conditional"].astype(np.float64), axis=1)
    assert np.abs(prob - t["pdf_uv"] / (w * h)).max() < 4e-7


@pytest.mark.parametrize("name", ["sky16x32", "sky64x128", "half_black"])
def test_density_is_positive_wherever_the_lookup_is(maps, name):
    """Structurally — a cell whose 3x3 neighbourhood (wrapped in x, clamped in y) holds a positive texel has positive density, and
    a cell is never chosen otherwise — and by 200 000 directions: positive looked-up radiance means positive density, and
    radiance / density stays bounded."""
    env, t = maps[name]
    h, w = env.shape[:2]
    lum = env.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    rows = [np.clip(np.arange(h) + dj, 0, h - 1) for dj in (-1, 0, 1)]
    near = np.max([np.roll(lum[r], s, axis=1) for r in rows for s in (-1, 0, 1)], axis=0) > 0
    assert np.array_equal(t["pdf_uv"] > 0, near)
    chosen = np.diff(t["marginal"])[:, None] * np.diff(t["conditional"], axis=1) > 0
    assert not (chosen & ~near).any()
    d = R._sphere_dirs(np.random.default_rng(11), 200_000)
    e = env_lookup(env.astype(np.float64), d.astype(np.float32)).astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    p = ER.pdf(t, d.astype(np.float32))
    assert (e > 0).sum() > 50_000 and (p[e > 0] > 0).all()
    ratio = (e[e > 0] / p[e > 0]).max() / (e.mean() * 4 * np.pi)
    print(f"{name}: max radiance / density = {ratio:.1f} x the map's integral")
    assert ratio < 100
    if name == "half_black":
        assert (t["pdf_uv"][h // 2 + 1:] == 0).all() and (t["pdf_uv"][h // 2] > 0).all()
        assert (np.diff(t["marginal"])[h // 2 + 1:] == 0).all()       # zero-width cells, never chosen


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(MAPS))
def test_sample_and_pdf_round_trip(maps, name, dtype):
    """The density sample() returns is pdf() of its direction, and pdf() finds the cell sample() drew from — except where the
    direction lies on a cell boundary to within what the precision resolves."""
    env, t = maps[name]
    g = np.random.default_rng(5)
    u = (g.integers(0, 1 << 24, (100_000, 2)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    s = ER.sample(t, u, dtype)
    assert (s["pdf"] > 0).all() and np.isfinite(s["pdf"]).all()
    assert np.abs(np.linalg.norm(s["dir"].astype(np.float64), axis=1) - 1).max() < (1e-12 if dtype == np.float64 else 1e-6)
    j, i, _, edge = ER.cell_of(t["pdf_uv"].shape, s["dir"], dtype)
    inside = edge > (1e-9 if dtype == np.float64 else 1e-6 * max(t["pdf_uv"].shape) + 1e-5)
    assert inside.mean() > 0.98
    assert np.array_equal(j[inside], s["j"][inside]) and np.array_equal(i[inside], s["i"][inside])
    back = ER.pdf(t, s["dir"], dtype)
    assert np.abs(back[inside] / s["pdf"][inside] - 1).max() < (1e-12 if dtype == np.float64 else 1e-5)
    if dtype == np.float32:     # the two precisions draw from the same cell on every row
        s64 = ER.sample(t, u, np.float64)
        assert np.array_equal(s64["j"], s["j"]) and np.array_equal(s64["i"], s["i"])
        assert (np.abs(s["dir"] - s64["dir"]).max(1) <= ER.direction_bound(t["pdf_uv"].shape, s64)).all()


@pytest.mark.parametrize("name", ["sky16x32", "sky64x128", "half_black"])
def test_monte_carlo_mean_matches_a_quadrature_of_the_map(maps, name):
    """mean(radiance / pdf) over 200 000 draws against the integral of the bilinear lookup over the sphere by the midpoint rule on
    8 x 8 sub-cells per texel (exact for the bilinear factor, whose kinks lie on sub-cell edges; the sin(theta) factor costs a
    relative (pi / 8H)^2 / 24 < 3e-5): within 5 standard errors of the mean."""
    env, t = maps[name]
    h, w = env.shape[:2]
    k = 8
    v, u = (np.arange(h * k) + 0.5) / (h * k), (np.arange(w * k) + 0.5) / (w * k)
    theta, phi = np.pi * v[:, None] * np.ones((1, w * k)), 2 * np.pi * u[None, :] * np.ones((h * k, 1))
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1).reshape(-1, 3)
    e = env_lookup(env.astype(np.float64), d.astype(np.float32)).astype(np.float64).mean(1)
    want = (e * np.sin(theta).ravel()).sum() * 2 * np.pi * np.pi / (h * k * w * k)
    g = np.random.default_rng(8)
    uu = (g.integers(0, 1 << 24, (200_000, 2)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    s = ER.sample(t, uu)
    x = env_lookup(env.astype(np.float64), s["dir"].astype(np.float32)).astype(np.float64).mean(1) / s["pdf"]
    mean, sem = x.mean(), x.std(ddof=1) / np.sqrt(len(x))
    print(f"{name}: Monte Carlo {mean:.5f} +- {sem:.5f}, quadrature {want:.5f} ({(mean - want) / sem:+.2f} sigma)")
    assert abs(mean - want) < 5 * sem


def test_mis_pair_and_cosine_estimator_agree_in_the_mean():
    """A horizontal diffuse plane under make_sky(64, 128, 5), 400 000 draws, no occluders: the per-sample difference between the
    MIS pair and the cosine estimator has mean 0 within 5 of its standard errors; and the pair's variance is several times
    smaller, which is the point of the feature."""
    env = _sky(64, 128, 5)
    cosine, pair = ER.plane_estimators(env, ER.build_tables(env), 400_000, seed=1)
    diff = pair - cosine
    sem = diff.std(ddof=1) / np.sqrt(len(diff))
    print(f"cosine {cosine.mean():.5f} (variance {cosine.var():.3f}), pair {pair.mean():.5f} (variance {pair.var():.3f}): "
          f"ratio {cosine.var() / pair.var():.1f}, difference {diff.mean() / sem:+.2f} sigma")
    assert abs(diff.mean()) < 5 * sem
    assert cosine.var() / pair.var() > 2


@pytest.mark.parametrize("with_lights", [False, True])
def test_reference_decides_the_same_in_fp32_and_fp64(with_lights):
    """On the synthetic wavefront of the GPU test: the same cell on every row in both precisions, and at most 0.1 % of the rows
    differ in a visibility decision of sample_env — the cap the kernel is held to."""
    env = R.synthetic_env()
    t = ER.build_tables(env)
    v, lights = ER.synthetic_env_vertices(env.shape[:2]), LR.synthetic_lights()
    n, n_b = len(v["material"]), len(R.SYNTH_SCENE["spheres"])
    seed, pass_idx, offset, bounce = 0x1234567890ABCDEF, 3, (1 << 32) - 2000, 1
    lsel, n_e = None, 1
    if with_lights:
        lsel = LR.sample_emitter(R.SYNTH_SCENE, lights, True, bounce, True, seed, pass_idx, offset,
                                 *[v[k] for k in VERTEX], v["wl"])["lsel"]
        n_e = 4
    runs = [ER.sample_env(R.SYNTH_SCENE, env, t, n_e, bounce, True, seed, pass_idx, offset, *[v[k] for k in VERTEX], lsel, v["wl"],
                          dtype=dt) for dt in (np.float64, np.float32)]
    s64, s32 = runs
    assert np.array_equal(s64["cell"][0], s32["cell"][0]) and np.array_equal(s64["cell"][1], s32["cell"][1])
    assert np.array_equal(s64["picked"], s32["picked"])
    differ = s64["lit"] != s32["lit"]
    print(f"lights = {with_lights}: {int(differ.sum())} of {n} rows decide visibility differently in fp32")
    assert differ.sum() <= n // 1000
    # the wavefront exercises what it is meant to
    live, picked = v["material"] <= n_b, s64["picked"]
    ball, floor = picked & (v["material"] < n_b), picked & (v["material"] == n_b)
    open_ = ER.sample_env(R.SYNTH_SCENE, env, t, n_e, bounce, False, seed, pass_idx, offset, *[v[k] for k in VERTEX], lsel, v["wl"])
    print(f"  picked {int(picked.sum())}, below the horizon {int((ball & (s64['wl'][:, 2] <= 0)).sum())}, "
          f"shadowed {int((open_['lit'] & ~s64['lit']).sum())}")
    assert picked.sum() >= (400 if with_lights else 3000) and (picked == live).all() == (not with_lights)
    assert (ball & (s64["wl"][:, 2] <= 0)).sum() >= 100 and (open_["lit"] & ~s64["lit"]).sum() >= 50
    assert (floor & s64["lit"]).sum() >= 50 and np.isnan(s64["emit"][~picked]).all()
    # and the "env" bounce moves the paths as the "cosine" bounce does, whatever the light sample was
    st = dict(v, wl=s64["wl"].astype(np.float32))
    b = B.bounce(R.SYNTH_SCENE, env, "env", bounce, False, True, seed, pass_idx, offset, *[st[k] for k in STATE], n_e=n_e, lsel=lsel,
                 emit=s64["emit"].astype(np.float32), lpdf=s64["lpdf"].astype(np.float32), tables=t)
    plain = B.bounce(R.SYNTH_SCENE, env, "cosine", bounce, False, True, seed, pass_idx, offset, *[st[k] for k in STATE])
    assert all(np.array_equal(b[k], plain[k], equal_nan=True) for k in ("org", "nrm", "wi", "wl", "material", "beta"))
    assert np.isfinite(b["rad"][live]).all()


def test_value_errors_before_a_device_is_touched():
    from bsdf_diffusion_sampling_amd.envmap import EnvDistribution, build_tables
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer, PointLight
    with pytest.raises(ValueError, match="black"):
        EnvDistribution(np.zeros((4, 8, 3), np.float32))
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        build_tables(np.ones((4, 8), np.float32))
    bad = np.ones((4, 8, 3), np.float32)
    bad[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        build_tables(bad)
    with pytest.raises(ValueError, match="finite and non-negative"):
        build_tables(-np.ones((4, 8, 3), np.float32))
    for word in ("uniform", "", None, "Importance"):
        with pytest.raises(ValueError, match="env_sampling"):
            PathArrayRenderer(None, [], [], env_sampling=word)
    with pytest.raises(ValueError, match="emitting environment"):
        PathArrayRenderer(None, [], [], lights=[PointLight((0.0, 4.0, 5.0), 200.0)], env_sampling="importance")
    with pytest.raises(ValueError, match="max_depth must be >= 1"):   # (the earlier checks still come first)
        PathArrayRenderer(None, [], [], max_depth=0, env_sampling="bogus")
