"""GPU: the path tracer on meshes — ``bsdfd_mesh_bounce``, ``bsdfd_mesh_sample_emitter`` and ``bsdfd_mesh_path_primary``
(csrc/mesh.hip, csrc/bounce_dev.h with mesh_dev::PathGeom) row by row against the fp64 reference of tests/mesh_bounce_ref.py, and
``mesh.MeshPathArrayRenderer`` at the level of images.

What is held to what (kernels):
* the conditions first: at most 1 % of any ray set marginal (mesh_ref.assert_marginal_cap), at most 3 % of the continuations
  fragile (within 4 x the fp32 restatement's barycentric error of one of the vertex rule's own discontinuities);
* on rows that are neither: ``material`` and ``prim`` equal the reference's — with roulette on the rows whose variate is farther
  from q than the fp32 run of the reference moves q;
* continuing rows: ``org`` to 4 et of t (et, eb: mesh_ref.fp32_restatement_error on the same rays), ``nrm`` / ``wi`` to
  tests/test_gpu_mesh.py's ``tol_n`` / ``4 tol_n``, diffuse reflectances exact, ``wl`` 2e-6, ``beta`` 2e-5;
* ``rad`` (and the emitter sample's ``emit``) to the sphere tests' ``_shade_bound``: p99.9 < 2e-4, max < 5e-3;
* ended rows keep every byte, ``prim`` included; nothing behind lane N is written;
* across commits: the full-width entry points reproduce tests/golden/mesh_path_before_unify.npz bit for bit, and their ``_rows``
  forms write those bits on the listed lanes and nothing else (section 3b).
Every figure is printed before it is asserted."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import mesh_bounce_ref as MB  # noqa: E402
import mesh_ref as MR  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from bsdf_diffusion_sampling_amd import _lib, mesh as M  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402
from oracle.wavefront_oracle import env_lookup  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MESH_FILE = os.path.join(GOLDEN, "matpreview.serialized")
SCENE_FILE = os.path.join(GOLDEN, "disney_bsdf_array2_spherical_envmap.xml")
SEED, PASS, OFFSET, BOUNCE = 0x1234567890ABCDEF, 3, (1 << 32) - 2000, 2   # (the path index crosses 2^32 inside the wavefront)
GUARD = 11
KEYS = ("org", "nrm", "wi", "wl", "material", "prim", "beta", "rad")
LSEL_SENTINEL, EMIT_SENTINEL = 0x5A5A5A5A, -123.25


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _p(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def _shade_bound(got, want):
    """tests/test_gpu_pathtrace.py's bound: relative error with a 1e-3 floor -> (p99.9, max), held to 2e-4 and 5e-3."""
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    return np.percentile(err, 99.9), err.max()


def wf_scene(cam, n_materials, albedo=(1.0, 1.0, 1.0), env_shape=(8, 16)):
    """The bsdfd_wf_scene a renderer builds for n_materials placeholder balls and this camera."""
    r, u, f = cam.basis()
    sc = _lib.WfScene()
    for name, val in (("cam_origin", cam.origin), ("cam_right", r), ("cam_up", u), ("cam_forward", f),
                      ("sphere_center", (0.0, 0.0, 0.0)), ("albedo", albedo)):
        setattr(sc, name, (C.c_float * 3)(*[float(x) for x in val]))
    sc.tan_half_fov = math.tan(math.radians(cam.fov_deg) * 0.5)
    sc.width, sc.height, sc.sphere_radius = cam.width, cam.height, 1.0
    sc.env_height, sc.env_width = env_shape
    sc.n_extra_spheres = n_materials - 1
    for k in range(1, n_materials):
        sc.extra_spheres[k - 1] = (C.c_float * 4)(0.0, 0.0, 0.0, 1.0)
    return sc


# ---- the kernel scene: made once, with every reference the tests share ----
def make_kernel_case(n=4096):
    geom = MB.kernel_scene(M)
    v = MB.synthetic_vertices(geom, n=n, seed=7)
    env = R.synthetic_env()
    lights = LR.make_lights([(1.0, 4.0, 2.0), (-2.5, 3.0, -1.0)], [40.0, (30.0, 20.0, 10.0)])
    cam = WF.Camera(origin=(0.0, 1.0, 8.0), width=8, height=8)
    return dict(geom=geom, v=v, env=env, lights=lights, scene=M.MeshScene(geom["meshes"], geom["instances"]),
                sc=wf_scene(cam, geom["n_materials"], geom["albedo"], env.shape[:2]), emitter={})


@pytest.fixture(scope="module")
def kernel_case():
    return make_kernel_case()


def _emitter(kc, occlusion, has_env):
    """The reference's emitter sample of the synthetic vertices (cached)."""
    key = (int(occlusion), int(has_env))
    if key not in kc["emitter"]:
        v = kc["v"]
        kc["emitter"][key] = MB.sample_emitter(kc["geom"], kc["lights"], bool(has_env), BOUNCE, bool(occlusion), SEED, PASS, OFFSET,
                                               *[v[k] for k in ("org", "nrm", "wi", "material", "prim", "wl")])
    return kc["emitter"][key]


def _device_lights(lights, has_env):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight, wf_lights
    return wf_lights([PointLight(tuple(p), tuple(i)) for p, i in zip(lights["position"].tolist(), lights["intensity"].tolist())],
                     has_env)


def _guarded(a, n_rows):
    """The rows of a host array on the device, GUARD rows of -7 behind them."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    pad = torch.full((GUARD,) + tuple(t.shape[1:]), -7, dtype=t.dtype, device=t.device)
    return torch.cat([t[:n_rows], pad]).contiguous()


def run_bounce(kc, v, n, mode, last, occlusion, rr_depth, lsel=None, emit=None, has_env=1, rows=None, bounce=BOUNCE):
    """One bsdfd_mesh_bounce call over the first n rows of ``v`` -> the eight state arrays (n + GUARD rows) as numpy.  ``rows`` (a
    host int64 array): bsdfd_mesh_bounce_rows over that list instead."""
    b = {k: _guarded(v[k], n) for k in MB.STATE if v.get(k) is not None}
    env = torch.from_numpy(kc["env"]).to(dev())
    lit = mode == "lit"
    if lit:
        lights = _device_lights(kc["lights"], has_env)
        b["lsel"], b["emit"] = _guarded(lsel, n), _guarded(emit, n)
    fn, listed = _lib.lib().bsdfd_mesh_bounce, ()
    if rows is not None:
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev())
        fn, listed = _lib.lib().bsdfd_mesh_bounce_rows, (_p(rows), rows.shape[0])
    with torch.cuda.device(dev()):
        _lib.check(fn(
            kc["scene"].handle(), C.byref(kc["sc"]), _p(env), bounce, int(last), int(occlusion), SEED, PASS, OFFSET, n,
            _p(b["org"]), _p(b["nrm"]), _p(b["wi"]), _p(b["wl"]), _p(b["material"]), _p(b["beta"]), _p(b["rad"]), _p(b["wo"]),
            _p(b["pdf_o"]), _p(b["pdf_l"]), _p(b.get("f_o")), _p(b.get("f_l")), C.byref(lights) if lit else None,
            _p(b["lsel"]) if lit else None, _p(b["emit"]) if lit else None, None, None, int(rr_depth or 0), _p(b["prim"]),
            *listed, None))
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy() for k in KEYS}


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _lit_inputs(kc):
    """The vertices, lsel and emit of a LIT bounce: the reference's emitter samples at occlusion = 1, rounded to fp32."""
    s = _emitter(kc, 1, 1)
    return dict(kc["v"], wl=s["wl"].astype(np.float32)), s["lsel"], s["emit"].astype(np.float32)


# ---- 1. the bounce against the fp64 reference ----
@pytest.mark.parametrize("rr_depth", [None, 1])
@pytest.mark.parametrize("occlusion", [0, 1])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("mode", ["cosine", "lit"])
def test_mesh_bounce_matches_reference(kernel_case, mode, last, occlusion, rr_depth):
    kc = kernel_case
    geom, n_b = kc["geom"], kc["geom"]["n_materials"]
    v, lsel, emit = (kc["v"], None, None) if mode == "cosine" else _lit_inputs(kc)
    n = len(v["material"])
    kw = dict(n_e=3, has_env=True, lsel=lsel, emit=emit) if mode == "lit" else {}
    args = [v[k] for k in MB.STATE]
    want = MB.bounce(geom, kc["env"], mode, BOUNCE, bool(last), bool(occlusion), SEED, PASS, OFFSET, *args, rr_depth=rr_depth, **kw)
    got = run_bounce(kc, v, n, mode, last, occlusion, rr_depth, lsel, emit)
    live = (v["material"] >= 0) & (v["material"] <= n_b)
    hit, shadow = want["hit"], want["shadow"]
    # the conditions on this test's own rays
    MR.assert_marginal_cap(hit)
    MR.assert_marginal_cap(shadow)
    et, eb = MR.fp32_restatement_error(geom["meshes"], geom["instances"], v["org"], want["d"], hit)
    nxt = MR.primary_arrays(geom["meshes"], geom["instances"], n_b, want["d"], hit, bary_tol=4 * eb)
    fragile = nxt["fragile"] & (hit["prim"][:, 0] >= 0)
    print(f"{mode} last={last} occlusion={occlusion} rr={rr_depth}: continuation rays hit {np.mean(hit['prim'][live, 0] >= 0):.3f}, "
          f"marginal {int(hit['marginal'].sum())} + {int(shadow['marginal'].sum())} (shadow), fragile {int(fragile.sum())}; "
          f"fp32 restatement: t rel {et:.3e}, bary abs {eb:.3e}")
    assert fragile.mean() <= 0.03
    # nothing behind lane N, and ended rows keep every byte, prim included
    for k in KEYS:
        assert (got[k][n:] == -7).all(), k
        assert _bytes_equal(got[k][:n][~live], v[k][~live]), k
    got = {k: a[:n] for k, a in got.items()}
    ok = live & ~hit["marginal"] & ~shadow["marginal"] & ~fragile
    # the roulette decides alike wherever the variate is farther from q than fp32 moves q
    decided = np.ones(n, dtype=bool)
    if rr_depth is not None and not last:
        q32 = MB.bounce(geom, kc["env"], mode, BOUNCE, bool(last), bool(occlusion), SEED, PASS, OFFSET, *args, rr_depth=rr_depth,
                        dtype=np.float32, **kw)["q"]
        with np.errstate(invalid="ignore"):
            eq = np.abs(q32.astype(np.float64) - want["q"])[want["would"]]
            decided = ~want["would"] | (np.abs(want["u"].astype(np.float64) - want["q"]) > eq.max(initial=0.0))
        print(f"  roulette: {int(want['would'].sum())} decisions, {int(want['killed'].sum())} kills, fp32 error of q {eq.max(initial=0.0):.3e}, "
              f"{int((~decided).sum())} rows too close to call")
        if occlusion:
            assert want["killed"].sum() > 50 and (want["would"] & ~want["killed"]).sum() > 50
    sure = ok & decided
    differ = sure & ((got["material"] != want["material"]) | (got["prim"] != want["prim"]).any(1))
    print(f"  {int(differ.sum())} of {int(sure.sum())} rows that are neither marginal nor fragile decide differently")
    assert not differ.any(), np.nonzero(differ)[0][:8]
    cont = sure & (want["material"] <= n_b)
    if last or not occlusion:
        assert (got["material"][live] == n_b + 1).all() and not cont.any()
    else:
        ids = np.bincount(want["material"][cont], minlength=n_b + 1)
        would = int((ok & want["would"]).sum())                          # (before the roulette, which ends more than half of them)
        print(f"  {would} rows reach a next vertex, {int(cont.sum())} continue: ids {ids.tolist()}")
        assert would > 500 and cont.sum() > (100 if rr_depth else 500) and (ids > 0).all()
        t = want["t"][cont]
        e_org = np.abs(got["org"][cont] - want["org"][cont]).max(1) / t
        tol_n = 2 * 3 * (4 * eb) / nxt["mix_len"].min() + 16 * 2.0 ** -24
        e_nrm = np.abs(got["nrm"][cont] - want["nrm"][cont]).max()
        lanes = cont & (want["material"] < n_b)
        diffuse = cont & (want["material"] == n_b)
        e_wi = np.abs(got["wi"][lanes] - want["wi"][lanes]).max()
        e_wl = np.abs(got["wl"][cont] - R.next_wl(SEED, PASS, BOUNCE, OFFSET, n)[cont]).max()
        e_beta = np.abs(got["beta"][cont] - want["beta"][cont]).max()
        print(f"  org / t: max {e_org.max():.3e} (bound {4 * et:.3e}); nrm {e_nrm:.3e} (bound {tol_n:.3e}); wi {e_wi:.3e} "
              f"(bound {4 * tol_n:.3e}); wl {e_wl:.3e}; beta {e_beta:.3e}")
        assert e_org.max() <= 4 * et
        assert e_nrm <= tol_n and e_wi <= 4 * tol_n
        assert np.array_equal(got["wi"][diffuse], want["wi"][diffuse].astype(np.float32))   # reflectances: exact
        assert e_wl < 2e-6 and e_beta < 2e-5
    # rows that end keep the rest of their state, prim included
    ended = sure & ~cont
    for k in ("org", "nrm", "wi", "wl", "beta", "prim"):
        assert _bytes_equal(got[k][ended], v[k][ended]), k
    same = live & ~hit["marginal"] & ~shadow["marginal"] & (got["material"] == want["material"]) & (got["prim"] == want["prim"]).all(1)
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same])
    print(f"  rad on the {int(same.sum())} rows that decide alike: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3


# ---- 2. tails ----
@pytest.mark.parametrize("mode", ["cosine", "lit"])
def test_mesh_bounce_tails(kernel_case, mode):
    kc = kernel_case
    v, lsel, emit = (kc["v"], None, None) if mode == "cosine" else _lit_inputs(kc)
    full = run_bounce(kc, v, len(v["material"]), mode, 0, 1, 1, lsel, emit)
    for n in (1, 63, 64, 65, 257):
        got = run_bounce(kc, v, n, mode, 0, 1, 1, lsel, emit)
        for k in KEYS:
            assert (got[k][n:] == -7).all(), (n, k)
            assert _bytes_equal(got[k][:n], full[k][:n]), (n, k)


# ---- 3. the emitter sample ----
@pytest.mark.parametrize("has_env", [0, 1])
@pytest.mark.parametrize("occlusion", [0, 1])
def test_mesh_sample_emitter_matches_reference(kernel_case, occlusion, has_env):
    kc = kernel_case
    v, n_b = kc["v"], kc["geom"]["n_materials"]
    n = len(v["material"])
    want, open_ = _emitter(kc, occlusion, has_env), _emitter(kc, 0, has_env)
    MR.assert_marginal_cap(want["shadow"])
    b = {k: _guarded(v[k], n) for k in ("org", "nrm", "wi", "material", "prim", "wl")}
    b["lsel"] = torch.full((n + GUARD,), LSEL_SENTINEL, dtype=torch.int32, device=dev())
    b["emit"] = torch.full((n + GUARD, 3), EMIT_SENTINEL, dtype=torch.float32, device=dev())
    lights = _device_lights(kc["lights"], has_env)
    with torch.cuda.device(dev()):
        _lib.check(_lib.lib().bsdfd_mesh_sample_emitter(
            kc["scene"].handle(), C.byref(kc["sc"]), C.byref(lights), BOUNCE, occlusion, SEED, PASS, OFFSET, n, _p(b["org"]),
            _p(b["nrm"]), _p(b["wi"]), _p(b["material"]), _p(b["wl"]), _p(b["lsel"]), _p(b["emit"]), _p(b["prim"]), None))
    torch.cuda.synchronize()
    h = {k: a.cpu().numpy() for k, a in b.items()}
    assert (h["wl"][n:] == -7).all() and (h["lsel"][n:] == LSEL_SENTINEL).all() and (h["emit"][n:] == EMIT_SENTINEL).all()
    for k in ("org", "nrm", "wi", "material", "prim"):                  # read only
        assert _bytes_equal(h[k][:n], v[k]), k
    wl, lsel, emit = h["wl"][:n], h["lsel"][:n], h["emit"][:n]
    live, floor = v["material"] <= n_b, v["material"] == n_b
    point = live & (want["lsel"] >= 0)
    assert np.array_equal(lsel[live], want["lsel"][live])               # exact
    assert _bytes_equal(wl[~live], v["wl"][~live]) and (lsel[~live] == LSEL_SENTINEL).all() and (emit[~live] == EMIT_SENTINEL).all()
    keep = live & (floor | ~point)
    assert _bytes_equal(wl[keep], v["wl"][keep]) and (emit[live & ~point] == 0).all()
    assert all((want["lsel"] == k).sum() >= 200 for k in range(2)) and ((want["lsel"] == -1).sum() >= 200) == bool(has_env)
    blocked = open_["lit"] & ~want["lit"]
    print(f"occlusion={occlusion} has_env={has_env}: {int(point.sum())} rows picked a light, {int(open_['lit'].sum())} see it above "
          f"their horizon, {int(blocked.sum())} of those are occluded, {int(want['shadow']['marginal'].sum())} shadow rays marginal")
    if occlusion:
        assert blocked.sum() >= 100 and (want["lit"] & point).sum() >= 100
    with np.errstate(invalid="ignore"):
        ok = point & ~want["shadow"]["marginal"] & (np.abs(want["cos"]) > 1e-5)   # (a light within rounding of the horizon may go either way)
    lit = (emit > 0).any(1)                                            # (every intensity and reflectance is positive)
    assert np.array_equal(lit[ok], want["lit"][ok])
    turned = ok & ~floor
    e_wl = np.abs(wl[turned] - want["wl"][turned]).max()
    p999, worst = _shade_bound(emit[ok], want["emit"][ok])
    print(f"  wl: max error {e_wl:.2e}; emit: p99.9 {p999:.2e} max {worst:.2e}")
    assert e_wl < 2e-5
    assert np.isfinite(emit[live]).all() and p999 < 2e-4 and worst < 5e-3


# ---- 3b. the kernels' bits across commits ----
# tests/golden/mesh_path_before_unify.npz (tests/golden/make_mesh_path_golden.py, run on the commit before the sphere and mesh
# kernels got one __global__ template and one launcher per stage): 1024 synthetic vertices on the kernel scene, ONE call each.
#   emitter_{wl,lsel,emit}       : bsdfd_mesh_sample_emitter (occlusion = 1, has_env = 1) over lsel / emit filled with the sentinels
#   {cosine,lit}_rr{0,2}_{KEYS}  : bsdfd_mesh_bounce (occlusion = 1, last = 0, bounce = 1) with rr_depth 0 and 2 — at bounce 1 the
#                                  roulette of rr_depth = 2 decides; LIT reads the recorded emitter sample (wl, lsel, emit)
RECORDING = os.path.join(GOLDEN, "mesh_path_before_unify.npz")
RECORDED_N, RECORDED_BOUNCE = 1024, 1
RECORDED_CASES = [(mode, rr) for mode in ("cosine", "lit") for rr in (0, 2)]


def run_sample_emitter(kc, v, n, occlusion, has_env, rows=None, bounce=BOUNCE):
    """One bsdfd_mesh_sample_emitter call over the first n rows of ``v``, lsel and emit filled with the sentinels -> wl, lsel, emit
    (n + GUARD rows) as numpy.  ``rows`` (a host int64 array): bsdfd_mesh_sample_emitter_rows over that list instead."""
    b = {k: _guarded(v[k], n) for k in ("org", "nrm", "wi", "material", "prim", "wl")}
    b["lsel"] = torch.full((n + GUARD,), LSEL_SENTINEL, dtype=torch.int32, device=dev())
    b["emit"] = torch.full((n + GUARD, 3), EMIT_SENTINEL, dtype=torch.float32, device=dev())
    lights = _device_lights(kc["lights"], has_env)
    fn, listed = _lib.lib().bsdfd_mesh_sample_emitter, ()
    if rows is not None:
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev())
        fn, listed = _lib.lib().bsdfd_mesh_sample_emitter_rows, (_p(rows), rows.shape[0])
    with torch.cuda.device(dev()):
        _lib.check(fn(kc["scene"].handle(), C.byref(kc["sc"]), C.byref(lights), bounce, occlusion, SEED, PASS, OFFSET, n, _p(b["org"]),
                      _p(b["nrm"]), _p(b["wi"]), _p(b["material"]), _p(b["wl"]), _p(b["lsel"]), _p(b["emit"]), _p(b["prim"]), *listed,
                      None))
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy() for k in ("wl", "lsel", "emit")}


def recorded_emitter(kc, rows=None):
    """The emitter sample of the recording's vertices, keyed as the recording keys it (n + GUARD rows)."""
    v = kc["v"]
    return {"emitter_" + k: a for k, a in run_sample_emitter(kc, v, len(v["material"]), 1, 1, rows, RECORDED_BOUNCE).items()}


def recorded_bounces(kc, emitter, rows=None):
    """The four bounces of the recording, keyed as the recording keys them (n + GUARD rows); ``emitter``: the emitter sample LIT
    reads, n rows under the recording's keys."""
    v, out = kc["v"], {}
    n = len(v["material"])
    lit = dict(v, wl=emitter["emitter_wl"][:n])
    for mode, rr in RECORDED_CASES:
        args = (lit, n, mode, 0, 1, rr, emitter["emitter_lsel"][:n], emitter["emitter_emit"][:n]) if mode == "lit" else \
            (v, n, mode, 0, 1, rr)
        got = run_bounce(kc, *args, rows=rows, bounce=RECORDED_BOUNCE)
        out.update({f"{mode}_rr{rr}_{k}": got[k] for k in KEYS})
    return out


def recorded_arrays(kc):
    """What tests/golden/make_mesh_path_golden.py saves: every key above, n rows each."""
    n = len(kc["v"]["material"])
    em = recorded_emitter(kc)
    return {k: a[:n] for k, a in dict(em, **recorded_bounces(kc, em)).items()}


@pytest.fixture(scope="module")
def recorded_case():
    return make_kernel_case(RECORDED_N), dict(np.load(RECORDING))


def test_mesh_kernels_are_bit_identical_to_the_recording(recorded_case):
    kc, rec = recorded_case
    n = RECORDED_N
    got = dict(recorded_emitter(kc), **recorded_bounces(kc, rec))
    assert sorted(got) == sorted(rec) and len(rec) == 3 + 8 * len(RECORDED_CASES)
    for k in sorted(rec):
        assert _bytes_equal(got[k][:n], rec[k]), k
    # the recording exercises what it pins: both roulette outcomes, continuing and ending paths, every emitter
    live = kc["v"]["material"] <= kc["geom"]["n_materials"]
    for mode in ("cosine", "lit"):
        on0, on2 = (rec[f"{mode}_rr{rr}_material"] <= kc["geom"]["n_materials"] for rr in (0, 2))
        print(f"{mode}: {int(live.sum())} live vertices, {int(on0.sum())} continue without roulette, {int(on2.sum())} survive rr_depth = 2")
        assert 0 < on2.sum() < on0.sum() < live.sum() and not (on2 & ~on0).any()
    assert all((rec["emitter_lsel"][live] == k).sum() > 50 for k in (-1, 0, 1))


def test_mesh_list_forms_write_the_recording_on_their_lanes(recorded_case):
    """The _rows entry points over every second live lane: the recording's bits on the listed lanes, every other byte as it was."""
    kc, rec = recorded_case
    v, n = kc["v"], RECORDED_N
    rows = np.nonzero(v["material"] <= kc["geom"]["n_materials"])[0][::2]
    assert rows.size > 256                                                 # (more than one block)
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    got = dict(recorded_emitter(kc, rows), **recorded_bounces(kc, rec, rows))
    before = {"emitter_wl": v["wl"], "emitter_lsel": np.full(n, LSEL_SENTINEL, dtype=np.int32),
              "emitter_emit": np.full((n, 3), EMIT_SENTINEL, dtype=np.float32)}
    for mode, rr in RECORDED_CASES:
        before.update({f"{mode}_rr{rr}_{k}": rec["emitter_wl"] if (mode, k) == ("lit", "wl") else v[k] for k in KEYS})
    for k in sorted(rec):
        assert (got[k][n:] == -7).all() or k in ("emitter_lsel", "emitter_emit"), k
        assert _bytes_equal(got[k][:n][listed], rec[k][listed]), k
        assert _bytes_equal(got[k][:n][~listed], before[k][~listed]), k
    assert (got["emitter_lsel"][n:] == LSEL_SENTINEL).all() and (got["emitter_emit"][n:] == EMIT_SENTINEL).all()


# ---- 4. the primary rays of a path ----
@pytest.fixture(scope="module")
def shapes():
    return M.load_serialized(MESH_FILE)


@pytest.fixture(scope="module")
def primary_case(shapes):
    """tests/test_gpu_mesh.py's: the checkered plane, two interiors carrying materials 0 and 1 (one mirrored and non-uniform) and a
    diffuse one, seen from a camera that also sees past them; 64 x 48 x 4."""
    plain, scaled, mirrored = MR.transforms()
    lift = lambda t, dy: np.hstack([t[:, :3], t[:, 3:] + [[0.0], [dy], [0.0]]])
    y_up = M.TO_Y_UP[:3, :3]
    inst = [M.Instance(1, np.hstack([y_up @ (4.0 * np.eye(3)), [[0.0], [-1.0], [0.0]]]), checker=(0.4, 0.2, 8.0, 16.0)),
            M.Instance(0, np.hstack([y_up, [[0.0], [0.0], [0.0]]]), material=0),
            M.Instance(0, lift(np.hstack([y_up @ mirrored[:, :3], mirrored[:, 3:]]), 0.5), material=1),
            M.Instance(0, lift(np.hstack([y_up @ scaled[:, :3], scaled[:, 3:]]), 0.3), diffuse=0.18)]
    meshes = [shapes[1], shapes[0]]
    cam = WF.Camera(origin=(1.0, 2.5, 9.0), target=(0.0, 0.8, 0.0), fov_deg=50.0, width=64, height=48)
    return dict(meshes=meshes, inst=inst, scene=M.MeshScene(meshes, inst), cam=cam, n_mat=2)


def _path_buffers(n):
    mk = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev())
    return dict(wi=mk(n, 3), wl=mk(n, 3), nrm=mk(n, 3), dir=mk(n, 3), mat=torch.full((n,), -7, dtype=torch.int64, device=dev()),
                org=mk(n, 3), prim=torch.full((n, 2), -7, dtype=torch.int32, device=dev()), beta=mk(n, 3), rad=mk(n, 3))


def _path_primary(scene, sc, env, rows, spp, seed, pas, b):
    with torch.cuda.device(dev()):
        return _lib.lib().bsdfd_mesh_path_primary(scene.handle(), C.byref(sc), rows[0], rows[1], spp, seed, pas, _p(b["wi"]), _p(b["wl"]),
                                                  _p(b["nrm"]), _p(b["dir"]), _p(b["mat"]), _p(env), _p(b["org"]), _p(b["prim"]),
                                                  _p(b["beta"]), _p(b["rad"]), None)


@pytest.mark.parametrize("rows", [(0, 48), (5, 17)])
def test_mesh_path_primary(primary_case, rows):
    pc = primary_case
    spp, seed, pas = 4, 77, 3
    env_h = R.synthetic_env()
    env = torch.from_numpy(env_h).to(dev())
    sc = wf_scene(pc["cam"], pc["n_mat"], env_shape=env_h.shape[:2])
    n = (rows[1] - rows[0]) * 64 * spp
    b, w = _path_buffers(n + GUARD), _path_buffers(n)
    _lib.check(_path_primary(pc["scene"], sc, env, rows, spp, seed, pas, b))
    pc["scene"].primary(sc, rows[0], rows[1], spp, seed, pas, w)
    torch.cuda.synchronize()
    for k in b:
        assert (b[k][n:] == -7).all(), k                                 # nothing behind the tile is written
    for k in ("wi", "wl", "nrm", "dir", "mat"):                          # bsdfd_mesh_primary's bits
        assert torch.equal(b[k][:n], w[k]), k
    g = {k: a[:n].cpu().numpy() for k, a in b.items()}
    cam = torch.from_numpy(np.tile(np.asarray(pc["cam"].origin, dtype=np.float32), (n, 1))).to(dev())
    t, prim, _ = pc["scene"].intersect(cam, b["dir"][:n].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(g["prim"], prim.cpu().numpy())                 # MeshScene.intersect's
    hit = g["prim"][:, 0] >= 0
    assert np.array_equal(hit, g["mat"] <= pc["n_mat"]) and hit.sum() > 500 and (~hit).sum() > 500
    org = cam.cpu().numpy()
    ref = MR.bvh_walk(pc["meshes"], pc["inst"], [pc["scene"].bvh(0), pc["scene"].bvh(1)], org, g["dir"])
    MR.assert_marginal_cap(ref)
    et, _ = MR.fp32_restatement_error(pc["meshes"], pc["inst"], org, g["dir"], ref)
    ok = hit & ~ref["marginal"] & (ref["t"] < MR.NOTHING)
    x = org[ok].astype(np.float64) + ref["t"][ok, None] * g["dir"][ok].astype(np.float64)
    e_org = np.abs(g["org"][ok] - x).max(1) / ref["t"][ok]
    print(f"path primary rows {rows}: {n} paths, {int(hit.sum())} hits; org / t: max {e_org.max():.3e} (bound {4 * et:.3e})")
    assert e_org.max() <= 4 * et
    assert (g["beta"] == 1).all() and (g["rad"][hit] == 0).all()
    assert (g["prim"][~hit] == -1).all() and (g["org"][~hit] == 0).all()
    look = env_lookup(env_h.astype(np.float64), g["dir"][~hit])
    p999, worst = _shade_bound(g["rad"][~hit], look)
    print(f"  rad of the {int((~hit).sum())} misses against the lookup: p99.9 {p999:.2e} max {worst:.2e}")
    assert p999 < 2e-4 and worst < 5e-3
    if rows != (0, 48):                                                  # a tile is the rows of the whole film
        full = _path_buffers(48 * 64 * spp)
        _lib.check(_path_primary(pc["scene"], sc, env, (0, 48), spp, seed, pas, full))
        torch.cuda.synchronize()
        lo = rows[0] * 64 * spp
        for k in b:
            assert torch.equal(full[k][lo:lo + n], b[k][:n]), k
    # an empty tile is a no-op; an instance whose material is not below n_materials is refused
    assert _path_primary(pc["scene"], sc, env, (7, 7), spp, seed, pas, {k: None for k in b}) == 0
    assert _path_primary(pc["scene"], wf_scene(pc["cam"], 1, env_shape=env_h.shape[:2]), env, rows, spp, seed, pas, b) == 1
    assert "n_materials" in _lib.lib().bsdfd_last_error().decode()


# ---- 5. the renderer ----
@pytest.fixture(scope="module")
def two_shells():
    """tests/test_gpu_mesh.py's: two shells of the fixture scene and its checkered plane, at 64 x 48."""
    names, _, full, albedo = M.mesh_scene_from_matpreview_xml(SCENE_FILE, MESH_FILE, 64, 48)
    shells = [i for i in full.instances if i.material is not None][:2]
    plane = next(i for i in full.instances if i.checker is not None)
    inst = [M.Instance(s.mesh, s.to_world, material=k) for k, s in enumerate(shells)] + [plane]
    cam = WF.Camera(origin=(1.0, 1.05, -1.5), target=(-3.5, 0.75, -1.5), fov_deg=40.0, width=64, height=48)
    return dict(scene=M.MeshScene(full.meshes, inst), cam=cam, env=WF.make_sky(64, 128, seed=5), albedo=albedo[:2], meshes=full.meshes,
                inst=inst)


def _disk_table():
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    return MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS[:2]])


def _renderer(ts, table=None, scene=None, **kw):
    dev()
    kw.setdefault("env", ts["env"])
    return M.MeshPathArrayRenderer(table or _disk_table(), scene or ts["scene"], camera=ts["cam"], **kw)


def _film(r, **kw):
    f = r.render(1, 4, seed=3, **kw)
    torch.cuda.synchronize()
    return f.cpu().numpy()


def _pixel_classes(r):
    """(all paths miss, all paths see the diffuse id, some path sees a material) per pixel, from the primary rays of seed 3."""
    mat = r.primary(0, 48, 4, 3, 0)["mat"].view(48, 64, 4).cpu().numpy()
    n_b = len(r.table)
    return (mat == n_b + 1).all(2), (mat == n_b).all(2), (mat < n_b).any(2)


def test_depth_one_is_the_mesh_array_renderer(two_shells):
    ts = two_shells
    tab = _disk_table()
    one = M.MeshArrayRenderer(tab, ts["scene"], camera=ts["cam"], env=ts["env"])
    path = _renderer(ts, tab, max_depth=1, occlusion=False)
    a, b = one.primary(0, 48, 4, 3, 0), path.primary(0, 48, 4, 3, 0)
    torch.cuda.synchronize()
    assert torch.equal(a["mat"], b["mat"])                               # the ids after primary
    for k in ("wi", "wl", "nrm", "dir"):
        assert torch.equal(a[k], b[k]), k
    f1, fp = _film(one), _film(path)
    p999, worst = _shade_bound(fp, f1)
    print(f"depth 1 without occlusion against MeshArrayRenderer: p99.9 {p999:.2e} max {worst:.2e}, bit-identical: {_bytes_equal(fp, f1)}")
    assert np.isfinite(fp).all() and p999 < 2e-4 and worst < 5e-3


def test_occlusion_removes_light_and_depth_adds_it(two_shells):
    ts = two_shells
    tab = _disk_table()
    open_, occ, deep = (_renderer(ts, tab, max_depth=d, occlusion=o) for d, o in ((1, False), (1, True), (3, True)))
    _, diffuse, _ = _pixel_classes(open_)
    f_open, f_occ, f_deep = _film(open_), _film(occ), _film(deep)
    assert diffuse.sum() > 500
    a, b, c = f_open[diffuse], f_occ[diffuse], f_deep[diffuse]
    print(f"{int(diffuse.sum())} pixels see only the diffuse id: occlusion darkens {int((b < a).any(1).sum())}, depth 3 brightens "
          f"{int((c > b).any(1).sum())}; lanes per bounce at depth 3: {deep.stats['lanes_per_bounce']}")
    assert (b <= a).all() and (b < a).any()                              # occlusion only removes light
    assert (c >= b).all() and (c > b).any()                              # depth only adds to it
    assert np.isfinite(f_deep).all() and (f_deep >= 0).all()


def test_furnace(two_shells):
    """Unit environment, albedo 1, a white plane, proxy shading, occlusion on at every depth: a pixel that sees nothing is 1, and
    a path's estimate only grows with the depth it is followed to (the same path, one more non-negative term per vertex)."""
    ts = two_shells
    tab = _disk_table()
    plane = ts["inst"][2]
    white = M.MeshScene(ts["meshes"], ts["inst"][:2] + [M.Instance(plane.mesh, plane.to_world, checker=(1.0, 1.0, plane.checker[2], plane.checker[3]))])
    env = torch.ones((4, 8, 3), dtype=torch.float32)
    means = []
    for depth in (1, 2, 4):
        r = _renderer(ts, tab, scene=white, env=env, max_depth=depth, occlusion=True, albedo=(1.0, 1.0, 1.0))
        miss, _, material = _pixel_classes(r)
        f = _film(r)
        assert miss.sum() > 50 and np.abs(f[miss] - 1).max() < 1e-5
        assert np.isfinite(f).all() and (f >= 0).all()
        means.append(float(f[material].mean()))
    print(f"furnace: mean over the {int(material.sum())} material pixels at depths 1, 2, 4: {means}")
    assert means[0] <= means[1] <= means[2] and means[0] < means[2]


def test_point_light(two_shells):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    ts = two_shells
    tab = _disk_table()
    centre = np.mean([i.matrix()[:, 3] for i in ts["inst"][:2]], axis=0)
    light = [PointLight(tuple(float(c) for c in centre + [0.0, 3.0, 0.0]), 40.0)]
    films = {}
    for occlusion in (False, True):
        r = _renderer(ts, tab, env=None, lights=light, max_depth=1, occlusion=occlusion)
        miss, diffuse, _ = _pixel_classes(r)
        f = films[occlusion] = _film(r)
        assert np.isfinite(f).all() and (f >= 0).all() and f.max() > 0
        assert miss.sum() > 50 and (f[miss] == 0).all()
    a, b = films[False][diffuse], films[True][diffuse]
    print(f"point light: {int(diffuse.sum())} floor pixels, {int((b < a).any(1).sum())} of them darker under occlusion")
    assert (b <= a).all() and (b < a).any()                              # the shells cast shadows


def test_unbounded_depth_ends(two_shells):
    ts = two_shells
    r = _renderer(ts, max_depth=None, rr_depth=5)
    live, n_b, inner = [], len(r.table), r.bounce

    def counting(b, *args, **kwargs):
        live.append(int((b["mat"] <= n_b).sum()))
        return inner(b, *args, **kwargs)
    r.bounce = counting
    f = _film(r)
    lanes = r.stats["lanes_per_bounce"]
    print(f"unbounded depth with rr_depth = 5: depth {r.stats['depth']}, material lanes {lanes}, live paths {live}")
    assert np.isfinite(f).all() and (f >= 0).all() and f.max() > 0
    assert r.stats["depth"] < r.DEPTH_CAP and not r.stats["depth_cap_hit"] and r.stats["depth"] >= 2
    assert lanes[1] < lanes[0]
    assert all(b <= a for a, b in zip(live, live[1:])) and live[-1] < live[0]   # the live paths never grow


def test_determinism_and_tiles(two_shells):
    ts = two_shells
    tab = _disk_table()
    r = _renderer(ts, tab, max_depth=3)
    a, b = _film(r), _film(r)
    c = _film(_renderer(ts, tab, max_depth=3))
    tile = _film(r, rows=(5, 17))
    assert _bytes_equal(a, b) and _bytes_equal(a, c)
    assert _bytes_equal(tile, a[5:17])                                   # a tile is the rows of the whole film
    assert not _bytes_equal(a, r.render(1, 4, seed=4).cpu().numpy())


@pytest.mark.parametrize("table", ["disk", "analytic"])
def test_both_tables_render(two_shells, table):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    ts = two_shells
    kw = {}
    if table == "disk":
        tab = _disk_table()
    else:
        from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
        stems = ["bsdf_13", "bsdf_24"]
        tab = MaterialTable([s + "_spherical" for s in stems])
        kw = dict(ground_truth=ground_truth_for(stems), ball_albedo=ts["albedo"])
    r = _renderer(ts, tab, max_depth=3, **kw)
    f = _film(r)
    print(f"[{table}] depth 3: mean {f.mean():.4f}, lanes per bounce {r.stats['lanes_per_bounce']}")
    assert f.shape == (48, 64, 3) and np.isfinite(f).all() and (f >= 0).all() and f.max() > 0
    assert len(r.stats["lanes_per_bounce"]) == 3 and all(n > 0 for n in r.stats["lanes_per_bounce"])


# ---- 6. the tool ----
def test_render_array_tool_traces_paths_on_meshes(tmp_path):
    dev()
    out = str(tmp_path / "mesh_path")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "render_array.py"), "--scene", SCENE_FILE, "--mesh-file", MESH_FILE, "--max-depth", "2",
           "--width", "64", "--height", "48", "--passes", "1", "--out", out]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout.strip().splitlines()[-1])
    img = np.load(out + ".npy")
    assert img.shape == (48, 64, 3) and np.isfinite(img).all() and img.max() > 0 and os.path.getsize(out + ".png") > 0
    assert '"max_depth": 2' in done.stdout and '"occlusion": true' in done.stdout
