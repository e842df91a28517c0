"""GPU tests of the point emitters of the array-scene path tracer: ``bsdfd_wf_sample_emitter`` and ``bsdfd_wf_bounce_lit``
(csrc/pathlights.hip) row by row against tests/pathtrace_lights_ref.py, and ``PathArrayRenderer(..., lights=...)`` at the level
of images — no lights is the renderer as it was, intensity scales the film exactly, a ball casts its shadow, depth only adds."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_ref as B  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from test_gpu_pathtrace import ROOT, _array, _scene_renderer, _shade_bound, _to_device  # noqa: E402
from test_pathtrace_cpu import STATE  # noqa: E402

VERTEX = ("org", "nrm", "wi", "material", "wl")
SEED, PASS, OFFSET, BOUNCE = 0x1234567890ABCDEF, 3, (1 << 32) - 2000, 1   # (the path index crosses 2^32 inside the wavefront)
LSEL_SENTINEL, EMIT_SENTINEL = 0x5A5A5A5A, -123.25


def _device_lights(lights, has_env):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight, wf_lights
    return wf_lights([PointLight(tuple(p), tuple(i)) for p, i in zip(lights["position"].tolist(), lights["intensity"].tolist())],
                     has_env)


def synthetic_inputs():
    v, lights, env = LR.synthetic_lit_vertices(), LR.synthetic_lights(), R.synthetic_env()
    sampled = {(occ, he): LR.sample_emitter(R.SYNTH_SCENE, lights, bool(he), BOUNCE, bool(occ), SEED, PASS, OFFSET,
                                            *[v[k] for k in VERTEX]) for occ in (0, 1) for he in (0, 1)}
    return v, lights, env, sampled


@pytest.fixture(scope="module")
def synth():
    return synthetic_inputs()


def _with_emitter_arrays(r, b, n):
    b["lsel"] = torch.full((n,), LSEL_SENTINEL, dtype=torch.int32, device=r.device)
    b["emit"] = torch.full((n, 3), EMIT_SENTINEL, dtype=torch.float32, device=r.device)
    return b


@pytest.mark.parametrize("has_env", [0, 1])
@pytest.mark.parametrize("occlusion", [0, 1])
def test_sample_emitter_kernel_matches_reference(synth, occlusion, has_env):
    """4096 synthetic vertices over 3 balls and the floor, three lights (one of them low), through ONE bsdfd_wf_sample_emitter
    call, row by row against the fp64 reference."""
    v, lights, env, sampled = synth
    want, open_ = sampled[(occlusion, has_env)], sampled[(0, has_env)]
    scene = R.SYNTH_SCENE
    n_b, n = len(scene["spheres"]), len(v["material"])
    r = _scene_renderer(scene, env)
    b = _with_emitter_arrays(r, _to_device(r, v), n)
    r.sample_emitter(b, BOUNCE, SEED, PASS, OFFSET, occlusion=bool(occlusion), lights=_device_lights(lights, has_env))
    torch.cuda.synchronize()
    wl, lsel, emit = (b[k].cpu().numpy() for k in ("wl", "lsel", "emit"))
    live, floor = v["material"] <= n_b, v["material"] == n_b
    point = live & (want["lsel"] >= 0)
    assert np.array_equal(lsel[live], want["lsel"][live])
    # ended paths: not a byte moves
    assert np.array_equal(wl[~live], v["wl"][~live], equal_nan=True)
    assert (lsel[~live] == LSEL_SENTINEL).all() and (emit[~live] == EMIT_SENTINEL).all()
    for k in ("org", "nrm", "wi"):
        assert np.array_equal(b[k].cpu().numpy(), v[k], equal_nan=True), k
    # floor rows and rows that picked the environment keep their cosine sample bit for bit
    keep = live & (floor | ~point)
    assert np.array_equal(wl[keep], v["wl"][keep]) and (emit[live & ~point] == 0).all()
    # the case is not vacuous
    assert all((want["lsel"] == k).sum() >= 200 for k in range(3)) and ((want["lsel"] == -1).sum() >= 200) == bool(has_env)
    if occlusion:
        assert (open_["lit"] & ~want["lit"]).sum() >= 100           # rows in the shadow of another surface
    assert (point & ~floor & (want["wl"][:, 2] <= 0)).sum() >= 100   # ball rows that see their light below the horizon
    lit = (emit > 0).any(1)                                           # (every intensity and reflectance is positive)
    differ = point & (lit != want["lit"])
    print(f"occlusion={occlusion} has_env={has_env}: {int(differ.sum())} of {n} rows decide visibility differently")
    assert differ.sum() <= n // 1000
    same = point & ~differ
    turned = same & ~floor
    e_wl = np.abs(wl[turned] - want["wl"][turned]).max()
    p999, worst = _shade_bound(emit[same], want["emit"][same])
    print(f"  wl: max error {e_wl:.2e}; emit: p99.9 {p999:.2e} max {worst:.2e}")
    assert e_wl < 2e-5
    assert np.isfinite(emit[live]).all() and p999 < 2e-4 and worst < 5e-3


def _lit_inputs(synth, has_env, with_f):
    """The vertices, lsel and emit of one bsdfd_wf_bounce_lit call: the reference's emitter samples at occlusion = 1, rounded to
    fp32."""
    v, lights, env, sampled = synth
    s = sampled[(1, has_env)]
    v = dict(v, wl=s["wl"].astype(np.float32))
    if not with_f:
        v = {k: a for k, a in v.items() if k not in ("f_o", "f_l")}
    return v, s["lsel"], s["emit"].astype(np.float32)


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("has_env", [0, 1])
def test_bounce_lit_kernel_matches_reference(synth, has_env, last, with_f):
    """The same vertices with the reference's emitter samples (rounded to fp32) through ONE bsdfd_wf_bounce_lit call, occlusion on:
    the assertions of test_bounce_kernel_matches_reference on the continuation state and on rad."""
    v, lights, env, sampled = synth
    v, lsel, emit = _lit_inputs(synth, has_env, with_f)
    scene = R.SYNTH_SCENE
    n_b, n = len(scene["spheres"]), len(v["material"])
    want = B.bounce(scene, env, "lit", BOUNCE, bool(last), True, SEED, PASS, OFFSET, *[v.get(k) for k in STATE], n_e=3 + has_env,
                    has_env=bool(has_env), lsel=lsel, emit=emit)
    r = _scene_renderer(scene, env)
    b, unlit = _to_device(r, v), _to_device(r, v)
    b["lsel"], b["emit"] = torch.from_numpy(lsel).to(r.device), torch.from_numpy(emit).to(r.device)
    r.bounce(b, BOUNCE, bool(last), SEED, PASS, OFFSET, occlusion=True, lights=_device_lights(lights, has_env))
    r.bounce(unlit, BOUNCE, bool(last), SEED, PASS, OFFSET, occlusion=True)
    torch.cuda.synchronize()
    keys = ("org", "nrm", "wi", "wl", "material", "beta", "rad")
    got = {k: b["mat" if k == "material" else k].cpu().numpy() for k in keys}
    identical = all(torch.equal(b[k].view(torch.int32), unlit[k].view(torch.int32)) for k in ("org", "nrm", "wi", "wl", "beta")) \
        and torch.equal(b["mat"], unlit["mat"])
    print(f"has_env={has_env} last={last} f={with_f}: continuation state bit-identical to bsdfd_wf_bounce's: {identical}")
    live = (v["material"] >= 0) & (v["material"] <= n_b)
    for k in got:   # ended paths: not a byte of their state moves
        assert np.array_equal(got[k][~live], v[k][~live], equal_nan=True), k
    assert np.array_equal(b["lsel"].cpu().numpy(), lsel) and np.array_equal(b["emit"].cpu().numpy(), emit)
    differ = got["material"] != want["material"]
    print(f"  {int(differ.sum())} of {n} rows decide differently")
    assert differ.sum() <= n // 1000
    assert ((got["material"] == n_b + 1) == (want["material"] == n_b + 1))[~differ].all()
    same = live & ~differ
    cont = same & (want["material"] <= n_b)
    if last:
        assert not cont.any() and (got["material"][live] == n_b + 1).all()
    else:
        assert cont.sum() > 500
        graze = cont & (want["cos_in"] < 0.1)
        ok = cont & ~graze
        for k in ("org", "nrm", "wi", "beta"):
            e_ok, e_all = np.abs(got[k][ok] - want[k][ok]).max(), np.abs(got[k][cont] - want[k][cont]).max()
            print(f"  {k}: max error {e_ok:.2e} ({e_all:.2e} with the {int(graze.sum())} grazing hits)")
            assert e_ok < 2e-5 and e_all < 2e-3, k
        e_wl = np.abs(got["wl"][cont] - R.next_wl(SEED, PASS, BOUNCE, OFFSET, n)[cont]).max()
        assert e_wl < 2e-6
    ended = same & ~cont   # rows that end keep the rest of their state
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert np.array_equal(got[k][ended], v[k][ended], equal_nan=True), k
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same])
    print(f"  rad: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3
    lit_rows = same & (lsel >= 0) & (emit > 0).any(1)
    assert lit_rows.sum() > 500 and (np.abs(want["rad"][lit_rows] - v["rad"][lit_rows]) > 0).any(1).mean() > 0.5   # (not vacuous)


def recorded_arrays(synth):
    """What tests/golden/bounce_kernels_before_merge.npz holds of this file's kernels (tests/golden/make_bounce_merge_golden.py):
    wl, lsel, emit of ONE bsdfd_wf_sample_emitter call (occlusion = 1, has_env = 1) on the inputs of
    test_sample_emitter_kernel_matches_reference, and rad of ONE bsdfd_wf_bounce_lit call (occlusion = 1, last = 0) on those of
    test_bounce_lit_kernel_matches_reference, as {key: array}."""
    v, lights, env, sampled = synth
    r = _scene_renderer(R.SYNTH_SCENE, env)
    out = {}
    b = _with_emitter_arrays(r, _to_device(r, v), len(v["material"]))
    r.sample_emitter(b, BOUNCE, SEED, PASS, OFFSET, occlusion=True, lights=_device_lights(lights, 1))
    out.update({f"sample_emitter_{k}": b[k].cpu().numpy() for k in ("wl", "lsel", "emit")})
    for has_env in (0, 1):
        for with_f in (True, False):
            v_in, lsel, emit = _lit_inputs(synth, has_env, with_f)
            b = _to_device(r, v_in)
            b["lsel"], b["emit"] = torch.from_numpy(lsel).to(r.device), torch.from_numpy(emit).to(r.device)
            r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True, lights=_device_lights(lights, has_env))
            out[f"bounce_lit_env{has_env}_f{int(with_f)}_rad"] = b["rad"].cpu().numpy()
    return out


def test_lit_kernels_are_bit_identical_to_the_recording(synth):
    """Every array bsdfd_wf_sample_emitter and bsdfd_wf_bounce_lit wrote before the three bounce kernels became one templated body
    (tests/golden/bounce_kernels_before_merge.npz), bit for bit.  The continuation state is pinned by
    test_bounce_kernel_is_bit_identical_to_the_recording through the "equal to bsdfd_wf_bounce's" assertions."""
    before = np.load(os.path.join(ROOT, "tests", "golden", "bounce_kernels_before_merge.npz"))
    got = recorded_arrays(synth)
    assert len(got) == 7
    for k, a in got.items():
        assert np.array_equal(a, before[k], equal_nan=True), k
    # ... and where a path goes is bsdfd_wf_bounce's on the same inputs, bit for bit
    v, lights, env, sampled = synth
    r = _scene_renderer(R.SYNTH_SCENE, env)
    for has_env in (0, 1):
        v_in, lsel, emit = _lit_inputs(synth, has_env, True)
        b, unlit = _to_device(r, v_in), _to_device(r, v_in)
        b["lsel"], b["emit"] = torch.from_numpy(lsel).to(r.device), torch.from_numpy(emit).to(r.device)
        r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True, lights=_device_lights(lights, has_env))
        r.bounce(unlit, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True)
        for k in ("org", "nrm", "wi", "wl", "beta"):
            assert torch.equal(b[k].view(torch.int32), unlit[k].view(torch.int32)), k
        assert torch.equal(b["mat"], unlit["mat"])


def test_errors(synth):
    from bsdf_diffusion_sampling_amd import _lib
    v, lights, env, sampled = synth
    n = len(v["material"])
    r = _scene_renderer(R.SYNTH_SCENE, env)
    b = _with_emitter_arrays(r, _to_device(r, v), n)
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    ok = _device_lights(lights, 1)
    vertex = [p(b["mat" if k == "material" else k]) for k in VERTEX]
    state = [p(b["mat" if k == "material" else k]) for k in STATE]
    emitter = lambda S, n, vert, lsel, emit: L.bsdfd_wf_sample_emitter(C.byref(r.scene), C.byref(S), 0, 1, 0, 0, 0, n, *vert, lsel, emit, None)
    lit = lambda S, n, st, lsel, emit: L.bsdfd_wf_bounce_lit(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *st, C.byref(S), lsel, emit, None)
    for count in (0, 9):
        bad = _device_lights(lights, 1)
        bad.n_lights = count
        for call, arrays in ((emitter, vertex), (lit, state)):
            assert call(bad, n, arrays, p(b["lsel"]), p(b["emit"])) == 1           # BSDFD_EINVAL
            assert b"point lights" in L.bsdfd_last_error()
    for call, arrays in ((emitter, vertex), (lit, state)):
        for lsel, emit in ((None, p(b["emit"])), (p(b["lsel"]), None)):
            assert call(ok, n, arrays, lsel, emit) == 1
            assert b"null pointer" in L.bsdfd_last_error()
        assert call(ok, 0, [None] * len(arrays), None, None) == 0               # N = 0: a no-op
    assert L.bsdfd_wf_sample_emitter(C.byref(r.scene), None, 0, 1, 0, 0, 0, n, *vertex, p(b["lsel"]), p(b["emit"]), None) == 1
    torch.cuda.synchronize()
    assert (b["lsel"] == LSEL_SENTINEL).all() and (b["emit"] == EMIT_SENTINEL).all()   # nothing ran


# ---- images: the 5-ball scene seen from 1.2 above the floor (balls, floor and sky in the frame), one light above the array ----
W, H, SPP = 96, 64, 2
LIGHT_POS, LIGHT_I = (-1.5, 4.0, -1.5), 200.0


def _lit(intensity=LIGHT_I, env=None, **kw):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    return _array(dict(lights=[PointLight(LIGHT_POS, intensity)], **kw), w=W, h=H, env=env, low_camera=True)


@pytest.mark.parametrize("depth", [1, 3])
def test_no_lights_is_the_renderer_without_the_argument(depth):
    films = [_array(dict(max_depth=depth, **kw), w=W, h=H, low_camera=True).render(1, spp=SPP, seed=4)
             for kw in ({}, dict(lights=None), dict(lights=[]))]
    assert torch.equal(films[0], films[1]) and torch.equal(films[0], films[2]) and float(films[0].mean()) > 0


def test_determinism_and_exact_scaling_with_the_intensity():
    """Two renders of one seed are equal, another seed differs; and twice the intensity is twice the film, bit for bit: every
    operation between the intensity and the film is a product with it or a sum of terms that carry it, and 2 is exact."""
    r = _lit(max_depth=3)
    a = r.render(1, spp=SPP, seed=5)
    assert torch.isfinite(a).all() and float(a.mean()) > 0
    assert torch.equal(a, r.render(1, spp=SPP, seed=5)) and torch.equal(a, _lit(max_depth=3).render(1, spp=SPP, seed=5))
    assert not torch.equal(a, r.render(1, spp=SPP, seed=6))
    assert torch.equal(2 * a, _lit(2 * LIGHT_I, max_depth=3).render(1, spp=SPP, seed=5))
    assert len(r.stats["lanes_per_bounce"]) >= 2 and r.stats["lanes_per_bounce"][0] > 0


def test_shadows_misses_and_the_inverse_square_law_at_depth_one():
    """max_depth = 1, black environment.  A floor pixel whose samples all lie inside the shadow of a ball shrunk to 0.98 of its
    radius (the line from the sample to the light passes the centre within 0.98 r) is exactly 0 with occlusion and positive
    without; a pixel whose samples all miss is exactly 0; and an unshadowed floor path carries refl I cos / (pi d^2), computed
    from the device's own position of the vertex."""
    occl, open_ = _lit(max_depth=1, occlusion=True), _lit(max_depth=1, occlusion=False)
    f_occl = torch.zeros((H, W, 3), device=occl.device)
    f_open = torch.zeros_like(f_occl)
    occl.render_pass(f_occl, 0, H, SPP, 3, 0)
    open_.render_pass(f_open, 0, H, SPP, 3, 0)
    torch.cuda.synchronize()
    n_b = len(open_.table)
    b = open_._buffers(H * W * SPP)
    org, rad = b["org"].cpu().numpy().astype(np.float64), b["rad"].cpu().numpy().astype(np.float64)
    first = open_.primary(0, H, SPP, 3, 0)                        # the ids and reflectances the pass started from
    mat, refl = first["mat"].cpu().numpy(), first["wi"].cpu().numpy()[:, 0].astype(np.float64)
    floor, miss = mat == n_b, mat == n_b + 1
    P = np.asarray(LIGHT_POS)
    to_light = P[None, :] - org
    d = np.linalg.norm(to_light, axis=1)
    want = refl * LIGHT_I * (to_light[:, 1] / d) / (np.pi * d * d)
    p999, worst = _shade_bound(rad[floor], np.repeat(want[floor, None], 3, 1))
    print(f"floor paths {int(floor.sum())}: rad against refl I cos / (pi d^2): p99.9 {p999:.2e} max {worst:.2e}")
    assert floor.sum() > 3000 and p999 < 2e-4 and worst < 5e-3
    shadowed = np.zeros(len(mat), dtype=bool)
    sc = open_.scene
    balls = [(list(sc.sphere_center), sc.sphere_radius)] + [(list(sc.extra_spheres[k])[:3], sc.extra_spheres[k][3]) for k in range(n_b - 1)]
    for c, r in balls:
        oc = org - np.asarray(c)[None, :]
        u = to_light / d[:, None]
        perp = oc - (oc * u).sum(1)[:, None] * u
        shadowed |= (perp * perp).sum(1) < (0.98 * r) ** 2
    px = lambda m: torch.from_numpy(m.reshape(H, W, SPP).all(-1)).to(occl.device)
    in_shadow, sky = px(floor & shadowed), px(miss)
    print(f"pixels in shadow {int(in_shadow.sum())}, pixels that miss {int(sky.sum())}")
    assert int(in_shadow.sum()) >= 50 and int(sky.sum()) >= 500
    assert (f_occl[in_shadow] == 0).all() and (f_open[in_shadow] > 0).all()
    assert (f_occl[sky] == 0).all() and (f_open[sky] == 0).all()
    assert (f_occl <= f_open).all()


def test_depth_only_adds():
    """Same seed, same draws, every addition non-negative: depth 3 is element-wise at least depth 1, and more somewhere."""
    a = _lit(max_depth=1, occlusion=True).render(1, spp=SPP, seed=3)
    c = _lit(max_depth=3).render(1, spp=SPP, seed=3)
    assert torch.isfinite(c).all() and (c >= a).all() and (c > a).any()


def test_environment_with_a_dark_light_is_the_unlit_renderer_in_the_mean():
    """An explicit environment and a light of intensity 0 (n_e = 2): the film is finite and its mean over the ball pixels is the
    unlit renderer's.  The spread s of that mean over 8 seeds of the unlit renderer is the yardstick: the difference between one
    lit render and the unlit mean of 8 has the standard error s sqrt(1 + 1/8); 5 of those are allowed."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=5)
    unlit = _array(dict(max_depth=2), w=W, h=H, env=env, low_camera=True)
    n_b = len(unlit.table)
    ids = torch.stack([unlit.primary(0, H, SPP, s, 0)["mat"].reshape(H, W, SPP) for s in range(9)], -1).reshape(H, W, -1)
    ball = (ids < n_b).all(-1)
    assert int(ball.sum()) > 300
    means = np.array([float(unlit.render(1, spp=SPP, seed=s)[ball].mean()) for s in range(8)])
    film = _lit(0.0, env=env, max_depth=2).render(1, spp=SPP, seed=8)
    assert torch.isfinite(film).all()
    got, s = float(film[ball].mean()), means.std(ddof=1)
    print(f"ball pixels {int(ball.sum())}: lit {got:.5f}, unlit {means.mean():.5f} +- {s:.5f} per seed")
    assert abs(got - means.mean()) < 5 * s * np.sqrt(1 + 1 / 8)
