"""GPU tests of the path kernels at their stated capacity: ``WF_MAX_SPHERES`` = 32 balls — ``trace()`` walks the whole kernel-argument
array ``sc.sph[32][4]``, ids run to 33 ("miss" = n_balls + 1) — and ``BSDFD_WF_MAX_LIGHTS`` = 8 lights (``lsel`` to 7, n_e = 9 with
the environment).  The largest scene of the other tests has 5 balls and 3 lights.  One call of each kernel on the synthetic
wavefront of its 3-ball test, generated over ``pass_replay.capacity_scene`` / ``capacity_lights``, against the same reference with
the same assertions; primary and path_begin of a film of that scene against the oracle; and the sizes past the capacity are
refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_ref as B  # noqa: E402
import envmap_ref as ER  # noqa: E402
import pass_replay as PR  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from oracle import wavefront_oracle as WO  # noqa: E402
from test_gpu_pathtrace import _gpu, _shade_bound, _to_device  # noqa: E402
from test_gpu_pathtrace_lights import _device_lights  # noqa: E402
from test_pathtrace_cpu import STATE  # noqa: E402

SEED, PASS, OFFSET, BOUNCE = 0x1234567890ABCDEF, 3, (1 << 32) - 2000, 1   # (the path index crosses 2^32 inside the wavefront)
SCENE, LIGHTS = PR.capacity_scene(), PR.capacity_lights()
N_B = len(SCENE["spheres"])
VERTEX = ("org", "nrm", "wi", "material")
LSEL_SENTINEL, EMIT_SENTINEL, LPDF_SENTINEL = 0x5A5A5A5A, -123.25, -77.5


def _stems(n):
    """Any ``n`` shipped weight sets: the table's nets are not run here."""
    from bsdf_diffusion_sampling_amd import weights as W
    return (W.list_shipped("disk") + W.list_shipped("spherical"))[:n]


@pytest.fixture(scope="module")
def table():
    _gpu()
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    return MaterialTable(_stems(N_B))


def _renderer(table, env, w=96, h=64):
    """The 32-ball scene seen from (0, 2.5, 5) with a 70 degree lens: every ball, the floor and the sky are in the frame."""
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    from bsdf_diffusion_sampling_amd.wavefront import Camera
    pl = SCENE["plane"]
    return PathArrayRenderer(table, [c for c, _ in SCENE["spheres"]], [r for _, r in SCENE["spheres"]],
                             camera=Camera(origin=(0.0, 2.5, 5.0), target=(0.0, 0.3, 0.0), fov_deg=70.0, width=w, height=h),
                             env=torch.from_numpy(env), checker=(pl["c0"], pl["c1"], pl["scale"]), albedo=SCENE["albedo"])


def _check_continuation(v, got, want, last=False):
    """The assertions of test_bounce_kernel_matches_reference (occlusion on) on the state after one bounce call."""
    n = len(v["material"])
    live = (v["material"] >= 0) & (v["material"] <= N_B)
    for k in got:   # ended paths: not a byte of their state moves
        assert np.array_equal(got[k][~live], v[k][~live], equal_nan=True), k
    differ = got["material"] != want["material"]
    assert differ.sum() <= n // 1000
    assert ((got["material"] == N_B + 1) == (want["material"] == N_B + 1))[~differ].all()
    same = live & ~differ
    cont = same & (want["material"] <= N_B)
    out = f"{int(differ.sum())} of {n} rows decide differently"
    if last:
        assert not cont.any() and (got["material"][live] == N_B + 1).all()
    else:
        assert cont.sum() > 500
        assert len(np.unique(want["material"][cont])) == N_B + 1        # paths go on to every ball (ids 0..31) and to the floor
        graze = cont & (want["cos_in"] < 0.1)
        ok = cont & ~graze
        for k in ("org", "nrm", "wi", "beta"):
            e_ok, e_all = np.abs(got[k][ok] - want[k][ok]).max(), np.abs(got[k][cont] - want[k][cont]).max()
            out += f"; {k} {e_ok:.1e} ({e_all:.1e} grazing)"
            assert e_ok < 2e-5 and e_all < 2e-3, k
        assert np.abs(got["wl"][cont] - R.next_wl(SEED, PASS, BOUNCE, OFFSET, n)[cont]).max() < 2e-6
    ended = same & ~cont   # rows that end keep the rest of their state
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert np.array_equal(got[k][ended], v[k][ended], equal_nan=True), k
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same])
    print(out + f"; rad p99.9 {p999:.1e} max {worst:.1e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3


def _state_of(b):
    return {k: b["mat" if k == "material" else k].cpu().numpy() for k in ("org", "nrm", "wi", "wl", "material", "beta", "rad")}


def test_bounce_with_32_balls(table):
    """bsdfd_wf_bounce, occlusion 1, last 0, on 4096 synthetic vertices that carry all 34 ids."""
    v, env = R.synthetic_vertices(scene=SCENE), R.synthetic_env()
    assert set(np.unique(v["material"]).tolist()) == set(range(N_B + 2))
    want = B.bounce(SCENE, env, "cosine", BOUNCE, False, True, SEED, PASS, OFFSET, *[v[k] for k in STATE])
    r = _renderer(table, env)
    b = _to_device(r, v)
    r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True)
    torch.cuda.synchronize()
    _check_continuation(v, _state_of(b), want)


@pytest.fixture(scope="module")
def lit():
    v, env = LR.synthetic_lit_vertices(scene=SCENE, lights=LIGHTS), R.synthetic_env()
    sampled = LR.sample_emitter(SCENE, LIGHTS, True, BOUNCE, True, SEED, PASS, OFFSET, *[v[k] for k in VERTEX], v["wl"])
    return v, env, sampled


def test_sample_emitter_and_bounce_lit_with_8_lights(table, lit):
    """bsdfd_wf_sample_emitter (has_env 1: n_e = 9) and bsdfd_wf_bounce_lit over 32 balls and 8 lights, one of them of intensity 0:
    the assertions of test_sample_emitter_kernel_matches_reference and test_bounce_lit_kernel_matches_reference."""
    v, env, want = lit
    n = len(v["material"])
    r = _renderer(table, env)
    lights = _device_lights(LIGHTS, 1)
    b = _to_device(r, v)
    b["lsel"] = torch.full((n,), LSEL_SENTINEL, dtype=torch.int32, device=r.device)
    b["emit"] = torch.full((n, 3), EMIT_SENTINEL, dtype=torch.float32, device=r.device)
    r.sample_emitter(b, BOUNCE, SEED, PASS, OFFSET, occlusion=True, lights=lights)
    torch.cuda.synchronize()
    wl, lsel, emit = (b[k].cpu().numpy() for k in ("wl", "lsel", "emit"))
    live, floor = v["material"] <= N_B, v["material"] == N_B
    point = live & (want["lsel"] >= 0)
    assert np.array_equal(lsel[live], want["lsel"][live])
    assert np.array_equal(wl[~live], v["wl"][~live], equal_nan=True)
    assert (lsel[~live] == LSEL_SENTINEL).all() and (emit[~live] == EMIT_SENTINEL).all()
    for k in ("org", "nrm", "wi"):
        assert np.array_equal(b[k].cpu().numpy(), v[k], equal_nan=True), k
    keep = live & (floor | ~point)
    assert np.array_equal(wl[keep], v["wl"][keep]) and (emit[live & ~point] == 0).all()
    picks = [int((want["lsel"] == k).sum()) for k in range(8)]
    assert min(picks) >= 200 and (want["lsel"] == -1).sum() >= 200 and lsel[live].max() == 7
    dark = point & (want["lsel"] == 7)                                # the light of intensity 0: nothing arrives, lit or not
    assert (emit[dark] == 0).all()
    bright = point & ~dark
    differ = bright & ((emit > 0).any(1) != want["lit"])
    assert differ.sum() <= n // 1000
    same = point & ~differ
    turned = same & ~floor
    e_wl = np.abs(wl[turned] - want["wl"][turned]).max()
    p999, worst = _shade_bound(emit[same], want["emit"][same])
    print(f"8 lights, picks {picks}: {int(differ.sum())} of {n} rows decide visibility differently; wl {e_wl:.1e}; emit p99.9 {p999:.1e} "
          f"max {worst:.1e}")
    assert (bright & ~want["lit"]).sum() >= 100 and (turned & (want["wl"][:, 2] <= 0)).sum() >= 100
    assert e_wl < 2e-5 and np.isfinite(emit[live]).all() and p999 < 2e-4 and worst < 5e-3
    # the bounce, on the reference's emitter samples rounded to fp32
    u = dict(v, wl=want["wl"].astype(np.float32))
    lsel_in, emit_in = want["lsel"], want["emit"].astype(np.float32)
    ref = B.bounce(SCENE, env, "lit", BOUNCE, False, True, SEED, PASS, OFFSET, *[u[k] for k in STATE], n_e=9, has_env=True, lsel=lsel_in,
                   emit=emit_in)
    b = _to_device(r, u)
    b["lsel"], b["emit"] = torch.from_numpy(lsel_in).to(r.device), torch.from_numpy(emit_in).to(r.device)
    r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True, lights=lights)
    torch.cuda.synchronize()
    assert np.array_equal(b["lsel"].cpu().numpy(), lsel_in) and np.array_equal(b["emit"].cpu().numpy(), emit_in)
    _check_continuation(u, _state_of(b), ref)
    lit_rows = (lsel_in >= 0) & (emit_in > 0).any(1) & live
    assert lit_rows.sum() > 500 and (np.abs(ref["rad"][lit_rows] - u["rad"][lit_rows]) > 0).any(1).mean() > 0.5


def test_sample_env_and_bounce_env_with_8_lights(table):
    """bsdfd_wf_sample_env and bsdfd_wf_bounce_env behind 8 lights (n_e = 9) over 32 balls: the assertions of
    test_sample_env_kernel_matches_reference and test_bounce_env_kernel_matches_reference."""
    from bsdf_diffusion_sampling_amd.envmap import EnvDistribution
    env = R.synthetic_env()
    t = ER.build_tables(env)
    v = ER.synthetic_env_vertices(env.shape[:2], scene=SCENE, lights=LIGHTS)
    n = len(v["material"])
    point = LR.sample_emitter(SCENE, LIGHTS, True, BOUNCE, True, SEED, PASS, OFFSET, *[v[k] for k in VERTEX], v["wl"])
    wl_in, lsel = point["wl"].astype(np.float32), point["lsel"]
    emit_in = np.full((n, 3), EMIT_SENTINEL, np.float32)
    emit_in[lsel >= 0] = point["emit"].astype(np.float32)[lsel >= 0]
    want = ER.sample_env(SCENE, env, t, 9, BOUNCE, True, SEED, PASS, OFFSET, *[v[k] for k in VERTEX], lsel, wl_in)
    r = _renderer(table, env)
    lights, dist = _device_lights(LIGHTS, 1), EnvDistribution(env)
    b = _to_device(r, dict(v, wl=wl_in, emit=emit_in, lpdf=np.full(n, LPDF_SENTINEL, np.float32), lsel=lsel))
    r.sample_env(b, BOUNCE, SEED, PASS, OFFSET, occlusion=True, lights=lights, env_dist=dist)
    torch.cuda.synchronize()
    wl, emit, lpdf = (b[k].cpu().numpy() for k in ("wl", "emit", "lpdf"))
    live, floor, picked = v["material"] <= N_B, v["material"] == N_B, want["picked"]
    assert np.array_equal(wl[~picked], wl_in[~picked], equal_nan=True)
    assert np.array_equal(emit[~picked], emit_in[~picked]) and (lpdf[~picked] == LPDF_SENTINEL).all()
    assert np.array_equal(b["lsel"].cpu().numpy(), lsel) and np.array_equal(b["mat"].cpu().numpy(), v["material"])
    for k in ("org", "nrm", "wi"):
        assert np.array_equal(b[k].cpu().numpy(), v[k], equal_nan=True), k
    assert np.array_equal(wl[floor], wl_in[floor])
    assert picked.sum() >= 200 and (picked & ~floor & (want["wl"][:, 2] <= 0)).sum() >= 30
    lit = (emit > 0).any(1)
    differ = picked & (lit != want["lit"])
    assert differ.sum() <= n // 1000 and (emit[picked & ~lit] == 0).all()
    same = picked & ~differ
    e_wl = np.abs(wl[same & ~floor] - want["wl"][same & ~floor]).max()
    e_pdf = np.abs(lpdf[picked] / want["lpdf"][picked] - 1).max()
    p999, worst = _shade_bound(emit[same], want["emit"][same])
    print(f"n_e = 9, {int(picked.sum())} rows picked the environment: {int(differ.sum())} decide visibility differently; wl {e_wl:.1e}; "
          f"lpdf {e_pdf:.1e}; emit p99.9 {p999:.1e} max {worst:.1e}")
    assert e_wl < 2e-5 and e_pdf < 1e-5 and (lpdf[picked] > 0).all()
    assert np.isfinite(emit[picked]).all() and p999 < 2e-4 and worst < 5e-3
    # the bounce, on the reference's emitter samples rounded to fp32
    u = dict(v, wl=np.where(picked[:, None], want["wl"], wl_in).astype(np.float32))
    emit_b = np.where(picked[:, None], want["emit"], np.where(emit_in == EMIT_SENTINEL, 0.0, emit_in)).astype(np.float32)
    lpdf_b = np.where(picked, want["lpdf"], 0.0).astype(np.float32)
    ref = B.bounce(SCENE, env, "env", BOUNCE, False, True, SEED, PASS, OFFSET, *[u[k] for k in STATE], n_e=9, lsel=lsel, emit=emit_b,
                   lpdf=lpdf_b, tables=t)
    b = _to_device(r, dict(u, emit=emit_b, lpdf=lpdf_b, lsel=lsel))
    r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=True, lights=lights, env_dist=dist)
    torch.cuda.synchronize()
    assert np.array_equal(b["emit"].cpu().numpy(), emit_b) and np.array_equal(b["lpdf"].cpu().numpy(), lpdf_b)
    _check_continuation(u, _state_of(b), ref)
    lit_rows = same & (emit_b > 0).any(1)
    assert lit_rows.sum() > 50 and (np.abs(ref["rad"][lit_rows] - u["rad"][lit_rows]) > 0).any(1).mean() > 0.5   # (one emitter in nine)


def test_primary_and_path_begin_of_a_32_ball_film(table):
    """primary (with ids to 33) and path_begin of a 96x64 film of the 32-ball scene against the oracle, as
    test_array_scene_matches_oracle and test_path_begin_and_resolve_match_reference hold them on 5 balls."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=5).numpy()
    r = _renderer(table, env)
    sc = PR.scene_of(r)
    assert len(sc["spheres"]) == N_B and r.scene.n_extra_spheres == 31
    spp = 2
    b = r.primary(0, 64, spp, seed=4, pass_idx=1)
    r.path_begin(b)
    torch.cuda.synchronize()
    h = {k: t.cpu().numpy() for k, t in b.items() if isinstance(t, torch.Tensor)}
    wi_o, wl_o, n_o, d_o, mat_o = WO.primary(sc, 0, 64, spp, seed=4, pass_idx=1, with_material=True)
    differ = h["mat"] != mat_o
    print(f"32 balls: {int(differ.sum())} of {len(mat_o)} primary rays decide differently; ids {np.unique(h['mat']).tolist()}")
    assert differ.sum() <= 4                                  # silhouettes / floor-ball contact: last-ulp decisions
    same = ~differ
    assert np.abs(h["dir"] - d_o).max() < 1e-6 and np.abs(h["wl"] - wl_o).max() < 2e-6
    floor = same & (mat_o == N_B)
    near = floor & (np.abs(h["org"]).max(1) < 16)             # (further out the checker cell is fp32's to decide)
    assert (h["wi"][near] == wi_o[near]).all() and (h["nrm"][floor] == [0, 1, 0]).all()
    ball = same & (mat_o < N_B) & (-(d_o * n_o).sum(1) > 0.1)
    assert np.abs(h["wi"][ball] - wi_o[ball]).max() < 5e-5
    assert set(np.unique(h["mat"]).tolist()) == set(range(N_B + 2))    # every ball, the floor and the sky
    org, beta, rad = R.path_begin(sc, env, h["dir"], h["nrm"], h["mat"])
    hit = h["mat"] <= N_B
    assert (h["beta"] == 1).all() and np.isfinite(h["org"]).all()
    err, size = np.abs(h["org"][hit] - org[hit]).max(1), np.abs(org[hit]).max(1)
    assert (err < 2e-5 + 4e-7 * size).all()
    assert (h["rad"][hit] == 0).all()
    p999, worst = _shade_bound(h["rad"], rad)
    assert p999 < 2e-4 and worst < 5e-3


def test_sizes_past_the_capacity_are_refused(table, lit):
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer, PointLight, wf_lights
    with pytest.raises(ValueError, match="1..32 balls"):
        PathArrayRenderer(MaterialTable(_stems(33)), [(0.0, 0.3, float(k)) for k in range(33)], [0.3] * 33)
    with pytest.raises(ValueError, match="1..8 point lights"):
        wf_lights([PointLight((0.0, 1.0, 0.0), 1.0)] * 9, has_env=True)
    v, env, sampled = lit
    n = len(v["material"])
    r = _renderer(table, env)
    b = _to_device(r, v)
    b["lsel"] = torch.full((n,), LSEL_SENTINEL, dtype=torch.int32, device=r.device)
    b["emit"] = torch.full((n, 3), EMIT_SENTINEL, dtype=torch.float32, device=r.device)
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    state = [p(b["mat" if k == "material" else k]) for k in STATE]
    vertex = [p(b["mat" if k == "material" else k]) for k in VERTEX + ("wl",)]
    before = {k: t.clone() for k, t in b.items()}
    sc = _lib.WfScene()
    C.memmove(C.byref(sc), C.byref(r.scene), C.sizeof(sc))
    sc.n_extra_spheres = 32
    assert L.bsdfd_wf_bounce(C.byref(sc), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, None) == 1
    assert b"at most 31 extra spheres" in L.bsdfd_last_error()
    nine = _device_lights(LIGHTS, 1)
    nine.n_lights = 9
    assert L.bsdfd_wf_sample_emitter(C.byref(r.scene), C.byref(nine), 0, 1, 0, 0, 0, n, *vertex, p(b["lsel"]), p(b["emit"]), None) == 1
    assert b"1..8 point lights" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_lit(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, C.byref(nine), p(b["lsel"]), p(b["emit"]),
                                 None) == 1
    assert b"1..8 point lights" in L.bsdfd_last_error()
    torch.cuda.synchronize()
    for k, t in b.items():                                    # nothing ran
        assert t.cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), k
