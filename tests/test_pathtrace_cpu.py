"""CPU side of the array-scene path tracer (csrc/pathtrace.hip, bsdf_diffusion_sampling_amd/pathtrace.py): the C ABI stays
version 8 with three more symbols, and the numpy restatement the GPU tests hold the kernels to (tests/pathtrace_ref.py) is itself
held to a closed form and to its own fp32 run."""
import ctypes as C
import os

import numpy as np
import pytest

import bounce_ref as B
import pathtrace_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bsdfd_wf_path_begin", "bsdfd_wf_bounce", "bsdfd_wf_resolve")
STATE = ("org", "nrm", "wi", "wl", "material", "beta", "rad", "wo", "pdf_o", "pdf_l", "f_o", "f_l")


def test_library_exports_the_path_kernels_without_a_new_abi():
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert all(name + "()" in note for name in SYMBOLS)
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr
    # bsdfd_wf_scene as it was: 12 + 1 floats, 2 ints, 3 + 1 + 3 floats, 3 ints, 31 x 4 floats, 1 int, 4 floats
    assert C.sizeof(_lib.WfScene) == 4 * (13 + 2 + 7 + 3 + 124 + 1 + 4) == 616
    src = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc", "pathtrace.hip")
    assert src in _lib.SRC_PATHS and src in _lib.DEP_PATHS and os.path.exists(src)
    body = os.path.join(os.path.dirname(src), "bounce_dev.h")   # the bounce body csrc/bounce.hip instantiates
    assert body in _lib.DEP_PATHS and body not in _lib.SRC_PATHS and os.path.exists(body)


def test_renderer_argument_checks():
    """The constructor refuses its arguments before it touches a device."""
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    with pytest.raises(ValueError, match="max_depth must be >= 1"):
        PathArrayRenderer(None, [], [], max_depth=0)
    with pytest.raises(ValueError, match="needs occlusion"):
        PathArrayRenderer(None, [], [], max_depth=2, occlusion=False)


def _floor_vertices(d, n, r=0.33, seed=0):
    """n floor vertices at horizontal distance d from the contact point of one ball of radius r resting on the plane, each with a
    cosine-weighted direction; unit reflectance, unit throughput."""
    scene = dict(spheres=[((0.0, r, 0.0), r)], plane=dict(y=0.0, c0=1.0, c1=1.0, scale=2.0), albedo=[1.0, 1.0, 1.0],
                 origin=(0.0, 1.0, 3.0))
    wl = R._cosine_dirs(np.random.default_rng(seed), n).astype(np.float32)
    one, zero = np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32)
    state = dict(org=np.tile(np.array([d, 0.0, 0.0], np.float32), (n, 1)), nrm=np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n, 1)),
                 wi=one, wl=wl, material=np.full(n, 1, dtype=np.int64), beta=one.copy(), rad=zero, wo=zero.copy(),
                 pdf_o=np.zeros(n, np.float32), pdf_l=np.zeros(n, np.float32))
    return scene, state


def form_factor_complement(d, r=0.33):
    """1 - (cosine-weighted form factor of a sphere of radius r tangent to the plane, seen from the plane at distance d from the
    contact point) = 1 - r^3 / (d^2 + r^2)^(3/2): what a unit-reflectance floor under a unit environment reflects there."""
    return 1.0 - r ** 3 / (d * d + r * r) ** 1.5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [0.2, 0.33, 0.7, 1.5])
def test_reference_matches_the_tangent_sphere_form_factor(d, dtype):
    n = 400_000
    scene, st = _floor_vertices(d, n, seed=int(d * 100))
    out = B.bounce(scene, np.ones((4, 8, 3), np.float32), "cosine", 0, True, True, 1, 0, 0, *[st[k] for k in STATE[:10]], dtype=dtype)
    assert (out["material"] == 2).all()                          # last = 1: every path has ended
    vals = out["rad"].astype(np.float64)
    assert ((vals == 0) | (np.abs(vals - 1) < 1e-6)).all()        # shadowed, or the unit environment (bilinear weights sum to 1 +- ulp)
    want = form_factor_complement(d)
    sigma = np.sqrt(want * (1 - want) / n)
    got = vals[:, 0].mean()
    print(f"d = {d}: mean {got:.6f}, closed form {want:.6f}, {(got - want) / sigma:+.2f} sigma")
    assert abs(got - want) < 5 * sigma


@pytest.mark.parametrize("occlusion", [False, True])
def test_reference_decides_the_same_in_fp32_and_fp64(occlusion):
    """On the synthetic wavefront of the GPU test the hit decisions (ended or not, the next id) of the fp32 and the fp64 run
    differ on at most 0.1 % of the rows: the cap the kernel is held to is one the arithmetic alone respects."""
    v = R.synthetic_vertices()
    env = R.synthetic_env()
    a, b = (B.bounce(R.SYNTH_SCENE, env, "cosine", 0, False, occlusion, 0x1234567890, 3, 1000, *[v[k] for k in STATE], dtype=dt)
            for dt in (np.float64, np.float32))
    differ = int((a["material"] != b["material"]).sum())
    print(f"occlusion = {occlusion}: {differ} of {len(v['material'])} rows decide differently in fp32")
    assert differ <= len(v["material"]) // 1000
    if occlusion:   # the wavefront exercises what it is meant to: every kind of next vertex, grazing hits included
        n_b = len(R.SYNTH_SCENE["spheres"])
        live = v["material"] <= n_b
        assert all((a["material"][live] == m).sum() > 30 for m in range(n_b + 2))
        assert (a["cos_in"] < 0.1).sum() > 10
    else:
        assert (a["material"] > len(R.SYNTH_SCENE["spheres"])).all()


def test_reference_decides_the_same_in_fp32_and_fp64_at_the_kernels_capacity():
    """The same at the stated capacity of the kernels — 32 balls (ids to 33) and 8 lights (pass_replay.capacity_scene /
    capacity_lights): the generators reach all 34 ids and all 8 lights, and the fp32 and fp64 references disagree on at most 0.1 %
    of the rows of ``bounce`` (with and without occlusion) and of the ``lit`` decisions of ``sample_emitter`` (has_env 0 and 1)."""
    import pass_replay as PR
    import pathtrace_lights_ref as LR
    scene, lights, env = PR.capacity_scene(), PR.capacity_lights(), R.synthetic_env()
    n_b = len(scene["spheres"])
    assert n_b == 32 and len(lights["position"]) == 8
    v = R.synthetic_vertices(scene=scene)
    n = len(v["material"])
    assert set(np.unique(v["material"]).tolist()) == set(range(n_b + 2))
    for occlusion in (False, True):
        a, b = (B.bounce(scene, env, "cosine", 0, False, occlusion, 0x1234567890, 3, 1000, *[v[k] for k in STATE], dtype=dt)
                for dt in (np.float64, np.float32))
        differ = int((a["material"] != b["material"]).sum())
        print(f"32 balls, occlusion = {occlusion}: {differ} of {n} rows decide differently in fp32")
        assert differ <= n // 1000
        if occlusion:
            live = v["material"] <= n_b
            assert len(np.unique(a["material"][live])) >= n_b and (a["material"][live] == n_b).sum() > 30
    v = LR.synthetic_lit_vertices(scene=scene, lights=lights)
    vertex = [v[k] for k in ("org", "nrm", "wi", "material", "wl")]
    for has_env in (False, True):
        s64, s32 = (LR.sample_emitter(scene, lights, has_env, 1, True, 0x1234567890, 3, 1000, *vertex, dtype=dt)
                    for dt in (np.float64, np.float32))
        assert np.array_equal(s64["lsel"], s32["lsel"])
        differ = int((s64["lit"] != s32["lit"]).sum())
        picks = [int((s64["lsel"] == k).sum()) for k in range(8)]
        print(f"8 lights, has_env = {has_env}: {differ} of {n} lit decisions differ in fp32; picks per light {picks}")
        assert differ <= n // 1000 and min(picks) >= 200 and s64["lsel"].max() == 7


def test_reference_leaves_ended_paths_alone_and_replays_philox():
    v = R.synthetic_vertices()
    out = B.bounce(R.SYNTH_SCENE, R.synthetic_env(), "cosine", 2, False, True, 9, 1, 77, *[v[k] for k in STATE])
    dead = v["material"] > len(R.SYNTH_SCENE["spheres"])
    assert dead.sum() > 100
    for k in ("org", "nrm", "wi", "wl", "beta", "rad"):
        assert np.array_equal(out[k][dead], v[k][dead].astype(np.float64), equal_nan=True), k
    assert (out["material"][dead] == v["material"][dead]).all()
    cont = ~dead & (out["material"] <= len(R.SYNTH_SCENE["spheres"]))
    wl = R.next_wl(9, 1, 2, 77, len(dead))
    assert cont.sum() > 100 and np.array_equal(out["wl"][cont], wl[cont].astype(np.float64))
    assert np.abs(np.linalg.norm(wl, axis=1) - 1).max() < 1e-6 and (wl[:, 2] >= 0).all()
    # depth 0's draw is primary's own (counter word 3 = "Wave"): the next one must not repeat it
    assert not np.array_equal(R.next_wl(9, 1, -1, 77, 16), R.next_wl(9, 1, 0, 77, 16))
