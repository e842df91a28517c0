"""CPU side of the point emitters of the array-scene path tracer (csrc/pathlights.hip, bsdf_diffusion_sampling_amd/pathtrace.py):
the C ABI stays version 8 with two more symbols and one more struct, and the numpy restatement the GPU tests hold the kernels
to (tests/pathtrace_lights_ref.py) is itself held to closed forms, to its own bookkeeping and to its own fp32 run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounce_ref as B
import pathtrace_lights_ref as LR
import pathtrace_ref as R
from test_pathtrace_cpu import STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bsdfd_wf_sample_emitter", "bsdfd_wf_bounce_lit")
VERTEX = ("org", "nrm", "wi", "material", "wl")          # what bsdfd_wf_sample_emitter reads


def _shade_bound(got, want):
    """The project's shading bound: relative error with a 1e-3 floor -> (p99.9, max), held to 2e-4 and 5e-3."""
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    return np.percentile(err, 99.9), err.max()


def test_library_exports_the_light_kernels_without_a_new_abi():
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert all(name + "()" in note for name in SYMBOLS)
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr
    assert C.sizeof(_lib.WfScene) == 616
    assert C.sizeof(_lib.WfLights) == 4 * (2 + 8 * 3 + 8 * 3) == 200 and _lib.WF_MAX_LIGHTS == 8
    assert "#define BSDFD_WF_MAX_LIGHTS 8\n" in hdr
    assert len(L.bsdfd_wf_sample_emitter.argtypes) == 16 and len(L.bsdfd_wf_bounce_lit.argtypes) == len(L.bsdfd_wf_bounce.argtypes) + 3
    src = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc", "pathlights.hip")
    assert src in _lib.SRC_PATHS and src in _lib.DEP_PATHS and os.path.exists(src)


def test_lights_struct_mirrors_the_header(tmp_path):
    """_lib.WfLights has the size and the field offsets gcc gives bsdfd_wf_lights."""
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from bsdf_diffusion_sampling_amd import _lib
    names = [n for n, _ in _lib.WfLights._fields_]
    assert names == ["n_lights", "has_env", "position", "intensity"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bsdfd.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(bsdfd_wf_lights));']
    src += [f'  printf("{f} %zu\\n", offsetof(bsdfd_wf_lights, {f}));' for f in names] + ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.WfLights) == 200
    for f in names:
        assert int(got[f]) == getattr(_lib.WfLights, f).offset, f


# ---- closed forms: one light at height H over the centre of a ball of radius r resting on the floor, n_e = 1, last = 1 ----------
H_LIGHT, R_BALL, I_LIGHT = 2.0, 0.33, 7.0
ONE_BALL = dict(spheres=[((0.0, R_BALL, 0.0), R_BALL)], plane=dict(y=0.0, c0=1.0, c1=1.0, scale=2.0), albedo=[1.0, 1.0, 1.0],
                origin=(0.0, 1.0, 3.0))
SHADOW_RADIUS = H_LIGHT * np.tan(np.arcsin(R_BALL / (H_LIGHT - R_BALL)))


def _lit_floor(d, occlusion, dtype):
    """Unit-reflectance floor vertices at the horizontal distances ``d`` from the light's foot, at random azimuths, through
    sample_emitter and the "lit" bounce (a bright environment that is no emitter: has_env = 0) -> rad[:, c], want."""
    n = len(d)
    g = np.random.default_rng(3)
    az = g.uniform(0, 2 * np.pi, n)
    one, zero = np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32)
    st = dict(org=np.stack([d * np.cos(az), np.zeros(n), d * np.sin(az)], 1).astype(np.float32),
              nrm=np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n, 1)), wi=one, wl=R._cosine_dirs(g, n).astype(np.float32),
              material=np.full(n, 1, dtype=np.int64), beta=one.copy(), rad=zero, wo=zero.copy(), pdf_o=np.zeros(n, np.float32),
              pdf_l=np.zeros(n, np.float32))
    lights = LR.make_lights([(0.0, H_LIGHT, 0.0)], [I_LIGHT])
    s = LR.sample_emitter(ONE_BALL, lights, False, 0, occlusion, 5, 0, 0, *[st[k] for k in VERTEX], dtype=dtype)
    assert (s["lsel"] == 0).all() and np.array_equal(s["wl"], st["wl"].astype(dtype))     # floor rows keep their direction
    out = B.bounce(ONE_BALL, np.full((4, 8, 3), 9.0, np.float32), "lit", 0, True, occlusion, 5, 0, 0,
                   *[s["wl"] if k == "wl" else st[k] for k in STATE[:10]], n_e=1, has_env=False, lsel=s["lsel"], emit=s["emit"],
                   dtype=dtype)
    assert (out["material"] == 2).all()
    d64 = np.linalg.norm(st["org"].astype(np.float64)[:, [0, 2]], axis=1)       # (the fp32 positions the reference saw)
    return out["rad"].astype(np.float64), I_LIGHT * H_LIGHT / (np.pi * (d64 ** 2 + H_LIGHT ** 2) ** 1.5), d64


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_matches_the_inverse_square_cosine_law(dtype):
    """rad = I H / (pi (d^2 + H^2)^(3/2)) on every row: the selection is trivial, so there is no sampling noise."""
    rad, want, _ = _lit_floor(np.random.default_rng(1).uniform(0.0, 4.0, 20000), False, dtype)
    p999, worst = _shade_bound(rad, want[:, None])
    print(f"{np.dtype(dtype).name}: p99.9 {p999:.2e} max {worst:.2e}")
    assert p999 < 2e-4 and worst < 5e-3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_casts_the_shadow_disc_of_a_ball(dtype):
    """The ball's shadow is a disc of radius H tan(alpha), sin(alpha) = r / (H - r): exactly 0 inside 0.98 of it with occlusion,
    the open value without; the open value outside 1.02 of it either way.  The vertices start at 0.01 of the radius (4e-3) from the
    point where the ball touches the floor: at distance d from it the ball is d^2 / 2r above the floor, and the ray tracer, which
    has no epsilon and asks for t > 0, resolves that gap in fp32 only while it exceeds an ulp of r, i.e. beyond d ~ 1.5e-4."""
    g = np.random.default_rng(2)
    d = np.concatenate([g.uniform(0.01, 0.98, 10000), g.uniform(1.02, 3.0, 10000)]) * SHADOW_RADIUS
    occl, want, d64 = _lit_floor(d, True, dtype)
    open_, _, _ = _lit_floor(d, False, dtype)
    inside = d64 < SHADOW_RADIUS
    assert inside.sum() == 10000 and (occl[inside] == 0).all()
    assert np.array_equal(occl[~inside], open_[~inside])
    p999, worst = _shade_bound(open_, want[:, None])
    assert p999 < 2e-4 and worst < 5e-3


def test_reference_one_sample_estimator_sums_the_lights():
    """Three lights, has_env = 0, 400 000 paths through one floor vertex: the mean of emit is the sum of the three terms each
    light gives when it is the only emitter, within 5 standard errors of the sample."""
    n = 400_000
    lights = LR.synthetic_lights()
    vert = dict(org=np.tile(np.array([0.3, 0.0, 0.7], np.float32), (n, 1)), nrm=np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n, 1)),
                wi=np.full((n, 3), 0.4, np.float32), material=np.full(n, 3, dtype=np.int64), wl=np.zeros((n, 3), np.float32))
    s = LR.sample_emitter(R.SYNTH_SCENE, lights, False, 1, True, 11, 2, 12345, *[vert[k] for k in VERTEX])
    counts = np.bincount(s["lsel"], minlength=3)
    assert (np.abs(counts - n / 3) < 5 * np.sqrt(n * (1 / 3) * (2 / 3))).all()
    want = np.zeros(3)
    for k in range(3):
        one = LR.make_lights(lights["position"][k:k + 1], lights["intensity"][k:k + 1])
        e = LR.sample_emitter(R.SYNTH_SCENE, one, False, 1, True, 11, 2, 0, *[vert[key][:1] for key in VERTEX])["emit"][0]
        assert (e > 0).all()                                     # (the vertex sees all three)
        want += e
    mean, sem = s["emit"].mean(0), s["emit"].std(0, ddof=1) / np.sqrt(n)
    print(f"mean emit {mean}, sum of the three terms {want}, {(mean - want) / sem} sigma")
    assert (np.abs(mean - want) < 5 * sem).all()


def test_reference_environment_with_a_dark_light_is_the_unlit_estimator():
    """has_env = 1 and one light of intensity 0 (n_e = 2), 400 000 synthetic ball vertices with a sampler whose densities are
    consistent (cosine-weighted wo, pdf = cos / pi): the mean per-row difference between the lit estimate and
    the "cosine" bounce's is zero within 5 of its own standard errors — the 1 / n_e in both MIS densities and the factor
    n_e of picking the environment half of the time cancel."""
    v = R.synthetic_vertices(400_000, seed=3)
    n_b = len(R.SYNTH_SCENE["spheres"])
    v = {k: a[v["material"] < n_b] for k, a in v.items()}
    n = len(v["material"])
    assert n > 150_000
    g = np.random.default_rng(4)
    v["wo"], v["wl"] = R._cosine_dirs(g, n).astype(np.float32), R._cosine_dirs(g, n).astype(np.float32)
    v["pdf_o"], v["pdf_l"] = v["wo"][:, 2] / np.float32(np.pi), v["wl"][:, 2] / np.float32(np.pi)
    v["beta"], v["rad"] = np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32)
    env = R.synthetic_env()
    dark = LR.make_lights([(0.0, 2.5, 0.5)], [0.0])
    args = lambda st: [st[k] for k in STATE[:10]]
    unlit = B.bounce(R.SYNTH_SCENE, env, "cosine", 0, True, True, 21, 0, 0, *args(v))["rad"]
    s = LR.sample_emitter(R.SYNTH_SCENE, dark, True, 0, True, 21, 0, 0, *[v[k] for k in VERTEX])
    assert (s["emit"] == 0).all() and 0.49 < (s["lsel"] == 0).mean() < 0.51
    lit = B.bounce(R.SYNTH_SCENE, env, "lit", 0, True, True, 21, 0, 0, *args(dict(v, wl=s["wl"])), n_e=2, has_env=True, lsel=s["lsel"],
                   emit=s["emit"])["rad"]
    diff = lit - unlit
    mean, sem = diff.mean(0), diff.std(0, ddof=1) / np.sqrt(n)
    print(f"unlit mean {unlit.mean(0)}, lit - unlit {mean}, {mean / sem} sigma")
    assert (np.abs(diff) > 1e-3).mean() > 0.3                     # (the two estimators do differ row by row)
    assert (np.abs(mean) < 5 * sem).all()


@pytest.mark.parametrize("has_env", [False, True])
def test_reference_decides_the_same_in_fp32_and_fp64(has_env):
    """On the synthetic wavefront of the GPU test with its three lights: the same emitter on every row in both precisions, and at
    most 0.1 % of the rows differ in a visibility or continuation decision — the cap the kernels are held to."""
    v, lights, env = LR.synthetic_lit_vertices(), LR.synthetic_lights(), R.synthetic_env()
    n, n_b = len(v["material"]), len(R.SYNTH_SCENE["spheres"])
    runs = []
    for dt in (np.float64, np.float32):
        s = LR.sample_emitter(R.SYNTH_SCENE, lights, has_env, 1, True, 0x1234567890, 3, 1000, *[v[k] for k in VERTEX], dtype=dt)
        st = dict(v, wl=s["wl"].astype(np.float32))
        b = B.bounce(R.SYNTH_SCENE, env, "lit", 1, False, True, 0x1234567890, 3, 1000, *[st[k] for k in STATE], n_e=3 + has_env,
                     has_env=has_env, lsel=s["lsel"], emit=s["emit"].astype(np.float32), dtype=dt)
        runs.append((s, b))
    (s64, b64), (s32, b32) = runs
    assert np.array_equal(s64["lsel"], s32["lsel"])
    differ = (s64["lit"] != s32["lit"]) | (b64["material"] != b32["material"])
    print(f"has_env = {has_env}: {int(differ.sum())} of {n} rows decide differently in fp32")
    assert differ.sum() <= n // 1000
    # the wavefront exercises what it is meant to
    live, point = v["material"] <= n_b, s64["lsel"] >= 0
    assert all((s64["lsel"] == k).sum() >= 200 for k in range(3))
    assert (point & ~s64["lit"]).sum() >= 100
    below = point & (v["material"] < n_b) & (s64["wl"][:, 2] <= 0)
    shadowed_floor = point & (v["material"] == n_b) & ~s64["lit"]
    assert below.sum() >= 100 and shadowed_floor.sum() >= 30
    assert ((s64["lsel"] == -1).sum() > 200) == has_env and (s64["lsel"][~live] == -2).all()


# ---- host ------------------------------------------------------------------------------------------------------------
XML = """<scene version="0.5.0">
  <integrator type="path"><integer name="maxDepth" value="2"/></integrator>
  <shape type="serialized"><bsdf type="mybsdf"><string name="filename" value="aniso_miro_7_rgb"/></bsdf>
    <transform name="toWorld"><translate x="-4" y="1" z="0"/></transform></shape>
  <emitter type="envmap"><string name="filename" value="envmap.exr"/></emitter>
  <emitter type="point"><point name="position" value="0, 4.0, 5.0"/><rgb name="intensity" value="200.0"/></emitter>
  <emitter type="point"><point name="position" x="1" y="-2" z="3.5"/><rgb name="intensity" value="1, 0.5, 0.25"/></emitter>
</scene>
"""


def test_lights_from_matpreview_xml(tmp_path):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight, lights_from_matpreview_xml
    from bsdf_diffusion_sampling_amd.wavefront import parse_matpreview_xml
    f = tmp_path / "scene.xml"
    f.write_text(XML)
    lights = lights_from_matpreview_xml(str(f))
    assert lights == [PointLight((0.0, 5.0, -4.0), 200.0), PointLight((1.0, 3.5, 2.0), (1.0, 0.5, 0.25))]
    assert len(parse_matpreview_xml(str(f))) == 1                  # (the ball parser still reads the same file)
    g = tmp_path / "envmap_only.xml"
    g.write_text(XML.replace('type="point"', 'type="spot"'))
    assert lights_from_matpreview_xml(str(g)) == []


def test_renderer_refuses_bad_lights_before_it_touches_a_device():
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer, PointLight, wf_lights
    ok = PointLight((0.0, 4.0, 5.0), 200.0)
    with pytest.raises(ValueError, match="point lights"):
        PathArrayRenderer(None, [], [], lights=[ok] * 9)
    for bad in (PointLight((0.0, float("nan"), 1.0), 1.0), PointLight((float("inf"), 0.0, 1.0), 1.0), PointLight((0.0, 1.0), 1.0)):
        with pytest.raises(ValueError, match="position"):
            PathArrayRenderer(None, [], [], lights=[ok, bad])
    for bad in (-1.0, float("nan"), float("inf"), (1.0, -0.5, 1.0), (1.0, 2.0)):
        with pytest.raises(ValueError, match="intensity"):
            PathArrayRenderer(None, [], [], lights=[PointLight((0.0, 4.0, 5.0), bad)])
    with pytest.raises(ValueError, match="max_depth must be >= 1"):   # (the earlier checks still come first)
        PathArrayRenderer(None, [], [], max_depth=0, lights=[ok])
    s = wf_lights([ok, PointLight((1, 2, 3), (1.0, 0.5, 0.25))], has_env=True)
    assert isinstance(s, _lib.WfLights) and (s.n_lights, s.has_env) == (2, 1)
    assert list(s.position[1]) == [1.0, 2.0, 3.0] and list(s.intensity[0]) == [200.0] * 3 and list(s.intensity[1]) == [1.0, 0.5, 0.25]
