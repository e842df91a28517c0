"""GPU tests of the environment map's importance sampler: ``bsdfd_env_sample`` / ``bsdfd_env_pdf`` and ``bsdfd_wf_sample_env`` /
``bsdfd_wf_bounce_env`` (csrc/pathenv.hip) row by row against tests/envmap_ref.py, and
``PathArrayRenderer(..., env_sampling="importance")`` at the level of images — cosine is the renderer as it was, the film scales
exactly with the map, the mean is the cosine renderer's, and the variance is several times smaller."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_ref as B  # noqa: E402
import envmap_ref as ER  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from test_gpu_pathtrace import ROOT, _array, _gpu, _scene_renderer, _shade_bound, _to_device  # noqa: E402
from test_gpu_pathtrace_lights import _device_lights  # noqa: E402
from test_pathtrace_cpu import STATE  # noqa: E402

VERTEX = ("org", "nrm", "wi", "material")
SEED, PASS, OFFSET, BOUNCE = 0x1234567890ABCDEF, 3, (1 << 32) - 2000, 1   # (the path index crosses 2^32 inside the wavefront)
LPDF_SENTINEL, EMIT_SENTINEL = -77.5, -123.25


def _sky(h, w, seed):
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    return make_sky(h, w, seed=seed).numpy()


def _half_black():
    env = _sky(64, 128, 5).copy()
    env[32:] = 0.0
    return env


# 2x4: the smallest map the renderer makes; 13x29: no power of two (the searches' trip counts over-run); the black lower half:
# cells of zero width; 4096 rows: twelve probes of the marginal, rows a 7.7e-4 rad high next to the poles
MAPS = {"2x4": lambda: _sky(2, 4, 1), "13x29": lambda: _sky(13, 29, 2), "half_black": _half_black, "4096x8": lambda: _sky(4096, 8, 4)}


def _dist(env):
    _gpu()
    from bsdf_diffusion_sampling_amd.envmap import EnvDistribution
    return EnvDistribution(env)


def _variates(t, n=4096, seed=9):
    """24-bit variates, with the ends of the range and entries of the CDFs themselves (a variate ON an entry belongs to the cell
    that begins there) among them."""
    g = np.random.default_rng(seed)
    u = (g.integers(0, 1 << 24, (n, 2)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    u[0], u[1], u[2], u[3] = (0.0, 0.0), (1 - 2.0 ** -24, 1 - 2.0 ** -24), (0.0, 1 - 2.0 ** -24), (1 - 2.0 ** -24, 0.0)
    m = t["marginal"][t["marginal"] < 1]
    u[4:64, 0] = m[g.integers(0, len(m), 60)]
    rows = ER.sample(t, u[:128])["j"]
    c = t["conditional"][rows, g.integers(0, t["conditional"].shape[1] - 1, 128)]
    u[64:128, 1] = np.where(c[64:128] < 1, c[64:128], 0.5)
    return u


@pytest.mark.parametrize("name", list(MAPS))
def test_env_sample_rows_match_reference(name):
    """bsdfd_env_sample on 4096 variates.  The device returns no cell index; that it drew from the reference's cell on EVERY row is
    held by two facts together: its density times 2 pi^2 max(sin theta, 1e-6) is that cell's table entry, and its direction lies
    within the fp32 bound (envmap_ref.direction_bound) of the fp64 direction in that cell.  Where the direction is clear of the
    cell's boundary, looking it up again finds the same cell and density."""
    env = MAPS[name]()
    t = ER.build_tables(env)
    shape = t["pdf_uv"].shape
    u = _variates(t)
    want = ER.sample(t, u)
    dist = _dist(env)
    d, p = dist.sample_t(torch.from_numpy(u).cuda())
    back = dist.pdf_t(d)
    torch.cuda.synchronize()
    d, p, back = d.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64), back.cpu().numpy().astype(np.float64)
    assert np.isfinite(d).all() and np.isfinite(p).all() and (p > 0).all()                   # no sampled row has pdf 0
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    sin_dev = np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2)
    cell_pdf = t["pdf_uv"][want["j"], want["i"]].astype(np.float64)
    assert (cell_pdf > 0).all()
    ref_at_dev = cell_pdf / (ER.TWO_PI_SQ * np.maximum(sin_dev, 1e-6))                         # the reference's pdf at the device's direction
    e_pdf = np.abs(p / ref_at_dev - 1).max()
    err, bound = np.abs(d - want["dir"]).max(1), ER.direction_bound(shape, want)
    print(f"{name}: pdf against the reference's at the device's direction {e_pdf:.2e}; direction error / bound max {(err / bound).max():.3f} "
          f"(bound {bound.min():.1e} .. {bound.max():.1e})")
    assert e_pdf < 1e-5
    assert (err <= bound).all()
    j, i, _, edge = ER.cell_of(shape, d)
    inside = edge > 1e-6 * max(shape) + 1e-5
    assert inside.mean() > 0.93         # (124 of the variates sit ON a CDF entry: offset 0, the cell's edge)
    assert np.array_equal(j[inside], want["j"][inside]) and np.array_equal(i[inside], want["i"][inside])
    assert np.abs(back[inside] / p[inside] - 1).max() < 1e-5 and np.abs(ER.pdf(t, d)[inside] / p[inside] - 1).max() < 1e-5
    if name == "half_black":
        assert (want["j"] <= 32).all() and (d[:, 1] > np.cos(np.pi * 33 / 64) - 1e-6).all()   # a zero-width cell is never chosen


@pytest.mark.parametrize("name", list(MAPS))
def test_env_pdf_rows_match_reference(name):
    """bsdfd_env_pdf on 4096 directions over the sphere, the poles and the seam of the azimuth among them."""
    env = MAPS[name]()
    t = ER.build_tables(env)
    shape = t["pdf_uv"].shape
    d = R._sphere_dirs(np.random.default_rng(3), 4096).astype(np.float32)
    d[:6] = [(0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (-1e-8, 0, -1), (1, 0, 0)]
    got = _dist(env).pdf_t(torch.from_numpy(d).cuda()).cpu().numpy().astype(np.float64)
    want = ER.pdf(t, d)
    inside = ER.cell_of(shape, d)[3] > 1e-6 * max(shape) + 1e-5
    inside[:6] = False
    assert np.isfinite(got).all() and (got >= 0).all() and inside.mean() > 0.97
    assert (np.abs(got[inside] - want[inside]) <= 1e-5 * want[inside]).all()
    assert ((got > 0) == (want > 0))[inside].all()
    if name == "half_black":
        assert (got[inside & (d[:, 1] < -0.1)] == 0).all() and (got[inside & (d[:, 1] > 0.1)] > 0).all()
    # at a pole the clamp of sin(theta) keeps the density finite: one of the first row's entries over 2 pi^2 1e-6
    assert np.isclose(got[0], t["pdf_uv"][0].astype(np.float64) / (ER.TWO_PI_SQ * 1e-6), rtol=1e-5).any()


# ---- the path kernels on the synthetic wavefront -----------------------------------------------------------------------------
def synthetic_inputs():
    env = R.synthetic_env()
    t = ER.build_tables(env)
    v, lights = ER.synthetic_env_vertices(env.shape[:2]), LR.synthetic_lights()
    point = LR.sample_emitter(R.SYNTH_SCENE, lights, True, BOUNCE, True, SEED, PASS, OFFSET, *[v[k] for k in VERTEX], v["wl"])
    sampled = {}
    for with_lights in (0, 1):
        wl = point["wl"].astype(np.float32) if with_lights else v["wl"]
        for occ in (0, 1):
            sampled[(with_lights, occ)] = ER.sample_env(R.SYNTH_SCENE, env, t, 4 if with_lights else 1, BOUNCE, bool(occ), SEED, PASS,
                                                        OFFSET, *[v[k] for k in VERTEX], point["lsel"] if with_lights else None, wl)
    return v, lights, env, t, point, sampled


@pytest.fixture(scope="module")
def synth():
    return synthetic_inputs()


def _emitter_inputs(v, point, with_lights):
    """wl, lsel, emit, lpdf as bsdfd_wf_sample_env finds them: after bsdfd_wf_sample_emitter with lights (its emit on the rows that
    picked a point), sentinels where nothing may be written."""
    n = len(v["material"])
    emit = np.full((n, 3), EMIT_SENTINEL, np.float32)
    if not with_lights:
        return v["wl"], None, emit, np.full(n, LPDF_SENTINEL, np.float32)
    is_point = point["lsel"] >= 0
    emit[is_point] = point["emit"].astype(np.float32)[is_point]
    return point["wl"].astype(np.float32), point["lsel"], emit, np.full(n, LPDF_SENTINEL, np.float32)


@pytest.mark.parametrize("occlusion", [0, 1])
@pytest.mark.parametrize("with_lights", [0, 1])
def test_sample_env_kernel_matches_reference(synth, with_lights, occlusion):
    """4096 synthetic vertices over 3 balls and the floor through ONE bsdfd_wf_sample_env call, row by row against the fp64
    reference: without lights (lsel NULL, n_e = 1) and behind sample_emitter with three lights (n_e = 4)."""
    v, lights, env, t, point, sampled = synth
    want, open_ = sampled[(with_lights, occlusion)], sampled[(with_lights, 0)]
    scene = R.SYNTH_SCENE
    n_b, n = len(scene["spheres"]), len(v["material"])
    wl_in, lsel, emit_in, lpdf_in = _emitter_inputs(v, point, with_lights)
    r = _scene_renderer(scene, env)
    b = _to_device(r, dict(v, wl=wl_in))
    b["emit"], b["lpdf"] = torch.from_numpy(emit_in).to(r.device), torch.from_numpy(lpdf_in).to(r.device)
    if with_lights:
        b["lsel"] = torch.from_numpy(lsel).to(r.device)
    r.sample_env(b, BOUNCE, SEED, PASS, OFFSET, occlusion=bool(occlusion), lights=_device_lights(lights, 1) if with_lights else None,
                 env_dist=_dist(env))
    torch.cuda.synchronize()
    wl, emit, lpdf = (b[k].cpu().numpy() for k in ("wl", "emit", "lpdf"))
    live, floor = v["material"] <= n_b, v["material"] == n_b
    picked = want["picked"]
    # ended paths and vertices that picked a point light: not a byte moves
    assert np.array_equal(wl[~picked], wl_in[~picked], equal_nan=True)
    assert np.array_equal(emit[~picked], emit_in[~picked]) and (lpdf[~picked] == LPDF_SENTINEL).all()
    if with_lights:
        assert np.array_equal(b["lsel"].cpu().numpy(), lsel)
    for k in ("org", "nrm", "wi"):
        assert np.array_equal(b[k].cpu().numpy(), v[k], equal_nan=True), k
    assert np.array_equal(b["mat"].cpu().numpy(), v["material"])
    assert np.array_equal(wl[floor], wl_in[floor])            # the floor keeps its cosine direction bit for bit
    # the case is not vacuous
    ball = picked & ~floor
    assert picked.sum() >= (400 if with_lights else 3000) and (picked == live).all() == (not with_lights)
    assert (ball & (want["wl"][:, 2] <= 0)).sum() >= 100             # below the horizon
    if occlusion:
        assert (open_["lit"] & ~want["lit"]).sum() >= 50             # in the shadow of another surface
    lit = (emit > 0).any(1)                                           # (the synthetic environment is positive everywhere)
    differ = picked & (lit != want["lit"])
    print(f"lights={with_lights} occlusion={occlusion}: {int(differ.sum())} of {n} rows decide visibility differently")
    assert differ.sum() <= n // 1000
    assert (emit[picked & ~lit] == 0).all()
    same = picked & ~differ
    e_wl = np.abs(wl[same & ~floor] - want["wl"][same & ~floor]).max()
    e_pdf = np.abs(lpdf[picked] / want["lpdf"][picked] - 1).max()
    p999, worst = _shade_bound(emit[same], want["emit"][same])
    print(f"  wl: max error {e_wl:.2e}; lpdf: {e_pdf:.2e}; emit: p99.9 {p999:.2e} max {worst:.2e}")
    assert e_wl < 2e-5 and e_pdf < 1e-5 and (lpdf[picked] > 0).all()
    assert np.isfinite(emit[picked]).all() and p999 < 2e-4 and worst < 5e-3


def _bounce_inputs(synth, with_lights, occlusion, with_f):
    """The vertices, lsel, emit, lpdf and picked rows of one bsdfd_wf_bounce_env call: the reference's emitter samples, rounded to
    fp32."""
    v, lights, env, t, point, sampled = synth
    s = sampled[(with_lights, occlusion)]
    wl_in, lsel, emit_in, lpdf_in = _emitter_inputs(v, point, with_lights)
    picked = s["picked"]
    v = dict(v, wl=np.where(picked[:, None], s["wl"], wl_in).astype(np.float32))
    if not with_f:
        v = {k: a for k, a in v.items() if k not in ("f_o", "f_l")}
    emit = np.where(picked[:, None], s["emit"], np.where(emit_in == EMIT_SENTINEL, 0.0, emit_in)).astype(np.float32)
    lpdf = np.where(picked, s["lpdf"], 0.0).astype(np.float32)
    return v, lsel, emit, lpdf, picked


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("occlusion", [0, 1])
@pytest.mark.parametrize("with_lights", [0, 1])
def test_bounce_env_kernel_matches_reference(synth, with_lights, occlusion, last, with_f):
    """The same vertices with the reference's emitter samples (rounded to fp32) through ONE bsdfd_wf_bounce_env call: the
    assertions of test_bounce_lit_kernel_matches_reference on rad and on the continuation state, which is bsdfd_wf_bounce's on
    the same inputs bit for bit."""
    v, lights, env, t, point, sampled = synth
    v, lsel, emit, lpdf, picked = _bounce_inputs(synth, with_lights, occlusion, with_f)
    scene = R.SYNTH_SCENE
    n_b, n = len(scene["spheres"]), len(v["material"])
    n_e = 4 if with_lights else 1
    want = B.bounce(scene, env, "env", BOUNCE, bool(last), bool(occlusion), SEED, PASS, OFFSET, *[v.get(k) for k in STATE], n_e=n_e,
                    lsel=lsel, emit=emit, lpdf=lpdf, tables=t)
    r = _scene_renderer(scene, env)
    b, plain = _to_device(r, v), _to_device(r, v)
    b["emit"], b["lpdf"] = torch.from_numpy(emit).to(r.device), torch.from_numpy(lpdf).to(r.device)
    if with_lights:
        b["lsel"] = torch.from_numpy(lsel).to(r.device)
    r.bounce(b, BOUNCE, bool(last), SEED, PASS, OFFSET, occlusion=bool(occlusion), lights=_device_lights(lights, 1) if with_lights else None,
             env_dist=_dist(env))
    r.bounce(plain, BOUNCE, bool(last), SEED, PASS, OFFSET, occlusion=bool(occlusion))
    torch.cuda.synchronize()
    keys = ("org", "nrm", "wi", "wl", "material", "beta", "rad")
    got = {k: b["mat" if k == "material" else k].cpu().numpy() for k in keys}
    # where a path goes does not depend on how the light was sampled
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert torch.equal(b[k].view(torch.int32), plain[k].view(torch.int32)), k
    assert torch.equal(b["mat"], plain["mat"])
    live = (v["material"] >= 0) & (v["material"] <= n_b)
    for k in got:   # ended paths: not a byte of their state moves
        assert np.array_equal(got[k][~live], v[k][~live], equal_nan=True), k
    assert np.array_equal(b["emit"].cpu().numpy(), emit) and np.array_equal(b["lpdf"].cpu().numpy(), lpdf)
    differ = got["material"] != want["material"]
    print(f"lights={with_lights} occlusion={occlusion} last={last} f={with_f}: {int(differ.sum())} of {n} rows decide differently")
    assert differ.sum() <= n // 1000
    assert ((got["material"] == n_b + 1) == (want["material"] == n_b + 1))[~differ].all()
    same = live & ~differ
    cont = same & (want["material"] <= n_b)
    if last or not occlusion:
        assert not cont.any() and (got["material"][live] == n_b + 1).all()
    else:
        assert cont.sum() > 500
        graze = cont & (want["cos_in"] < 0.1)
        ok = cont & ~graze
        for k in ("org", "nrm", "wi", "beta"):
            e_ok, e_all = np.abs(got[k][ok] - want[k][ok]).max(), np.abs(got[k][cont] - want[k][cont]).max()
            assert e_ok < 2e-5 and e_all < 2e-3, k
        assert np.abs(got["wl"][cont] - R.next_wl(SEED, PASS, BOUNCE, OFFSET, n)[cont]).max() < 2e-6
    ended = same & ~cont   # rows that end keep the rest of their state
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert np.array_equal(got[k][ended], v[k][ended], equal_nan=True), k
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same])
    print(f"  rad: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3
    lit_rows = same & picked & (emit > 0).any(1)     # (not vacuous: the environment's draw arrives)
    assert lit_rows.sum() > (100 if with_lights else 500)
    assert (np.abs(want["rad"][lit_rows] - v["rad"][lit_rows]) > 0).any(1).mean() > 0.5


def recorded_arrays(synth):
    """What tests/golden/bounce_kernels_before_merge.npz holds of this file's kernels (tests/golden/make_bounce_merge_golden.py):
    wl, lsel, emit, lpdf after ONE bsdfd_wf_sample_env call (occlusion = 1; without and with lights) on the inputs of
    test_sample_env_kernel_matches_reference, and rad of ONE bsdfd_wf_bounce_env call (last = 0) on those of
    test_bounce_env_kernel_matches_reference, as {key: array}."""
    v, lights, env, t, point, sampled = synth
    r = _scene_renderer(R.SYNTH_SCENE, env)
    dist = _dist(env)
    device_lights = lambda with_lights: _device_lights(lights, 1) if with_lights else None
    out = {}
    for with_lights in (0, 1):
        wl_in, lsel, emit_in, lpdf_in = _emitter_inputs(v, point, with_lights)
        b = _to_device(r, dict(v, wl=wl_in, emit=emit_in, lpdf=lpdf_in, **({"lsel": lsel} if with_lights else {})))
        r.sample_env(b, BOUNCE, SEED, PASS, OFFSET, occlusion=True, lights=device_lights(with_lights), env_dist=dist)
        out.update({f"sample_env_lights{with_lights}_{k}": b[k].cpu().numpy() for k in ("wl", "lsel", "emit", "lpdf") if k in b})
    cases = [(wl, occ, True) for wl in (0, 1) for occ in (0, 1)] + [(0, 1, False), (1, 1, False)]
    for with_lights, occlusion, with_f in cases:
        v_in, lsel, emit, lpdf, picked = _bounce_inputs(synth, with_lights, occlusion, with_f)
        b = _to_device(r, dict(v_in, emit=emit, lpdf=lpdf, **({"lsel": lsel} if with_lights else {})))
        r.bounce(b, BOUNCE, False, SEED, PASS, OFFSET, occlusion=bool(occlusion), lights=device_lights(with_lights), env_dist=dist)
        out[f"bounce_env_lights{with_lights}_occlusion{occlusion}_f{int(with_f)}_rad"] = b["rad"].cpu().numpy()
    return out


def test_env_kernels_are_bit_identical_to_the_recording(synth):
    """Every array bsdfd_wf_sample_env and bsdfd_wf_bounce_env wrote before the three bounce kernels became one templated body
    (tests/golden/bounce_kernels_before_merge.npz), bit for bit.  The continuation state is pinned by
    test_bounce_kernel_is_bit_identical_to_the_recording through test_bounce_env_kernel_matches_reference's "equal to
    bsdfd_wf_bounce's" assertions."""
    before = np.load(os.path.join(ROOT, "tests", "golden", "bounce_kernels_before_merge.npz"))
    got = recorded_arrays(synth)
    assert len(got) == 3 + 4 + 6
    for k, a in got.items():
        assert np.array_equal(a, before[k], equal_nan=True), k


def test_errors(synth):
    from bsdf_diffusion_sampling_amd import _lib
    v, lights, env, t, point, sampled = synth
    n = len(v["material"])
    r = _scene_renderer(R.SYNTH_SCENE, env)
    b = _to_device(r, v)
    b["emit"] = torch.full((n, 3), EMIT_SENTINEL, dtype=torch.float32, device=r.device)
    b["lpdf"] = torch.full((n,), LPDF_SENTINEL, dtype=torch.float32, device=r.device)
    b["lsel"] = torch.full((n,), -1, dtype=torch.int32, device=r.device)
    L, p = _lib.lib(), (lambda x: C.c_void_p(x.data_ptr()))
    dist = _dist(env)
    good = dist.struct(r.device)
    u = torch.rand((n, 2), device=r.device)
    out3, out1 = torch.full((n, 3), 7.0, device=r.device), torch.full((n,), 7.0, device=r.device)
    vertex = [p(b["mat" if k == "material" else k]) for k in VERTEX]
    state = [p(b["mat" if k == "material" else k]) for k in STATE]
    lt = _device_lights(lights, 1)

    def calls(S, count):
        return (L.bsdfd_env_sample(C.byref(S), count, p(u), p(out3), p(out1), None),
                L.bsdfd_env_pdf(C.byref(S), count, p(out3), p(out1), None),
                L.bsdfd_wf_sample_env(C.byref(r.scene), p(r.env), C.byref(S), 1, 0, 1, 0, 0, 0, count, *vertex, None, p(b["wl"]),
                                      p(b["lpdf"]), p(b["emit"]), None),
                L.bsdfd_wf_bounce_env(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, count, *state, None, None, p(b["emit"]),
                                      p(b["lpdf"]), C.byref(S), None))

    def broken(**fields):
        S = _lib.EnvDist()
        C.memmove(C.byref(S), C.byref(good), C.sizeof(S))
        for k, val in fields.items():
            setattr(S, k, val)
        return S
    for field in ("marginal", "conditional", "pdf_uv"):                      # null table pointers
        assert calls(broken(**{field: None}), n) == (1, 1, 1, 1)
        assert b"null environment distribution table" in L.bsdfd_last_error()
    for field in ("width", "height"):                                        # non-positive sizes
        for bad in (0, -4):
            assert calls(broken(**{field: bad}), n) == (1, 1, 1, 1)
            assert b"size must be positive" in L.bsdfd_last_error()
    # a distribution of another size than the environment map is refused by the path kernels
    half = broken(width=good.width // 2)
    assert L.bsdfd_wf_sample_env(C.byref(r.scene), p(r.env), C.byref(half), 1, 0, 1, 0, 0, 0, n, *vertex, None, p(b["wl"]),
                                 p(b["lpdf"]), p(b["emit"]), None) == 1 and b"environment map's size" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_env(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, None, None, p(b["emit"]), p(b["lpdf"]),
                                 C.byref(half), None) == 1 and b"environment map's size" in L.bsdfd_last_error()
    # lsel NULL with n_e != 1
    assert L.bsdfd_wf_sample_env(C.byref(r.scene), p(r.env), C.byref(good), 2, 0, 1, 0, 0, 0, n, *vertex, None, p(b["wl"]),
                                 p(b["lpdf"]), p(b["emit"]), None) == 1
    assert b"n_e must be 1" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_env(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, C.byref(lt), None, p(b["emit"]),
                                 p(b["lpdf"]), C.byref(good), None) == 1
    assert b"both NULL or both given" in L.bsdfd_last_error()
    no_env = _device_lights(lights, 0)
    assert L.bsdfd_wf_bounce_env(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, C.byref(no_env), p(b["lsel"]), p(b["emit"]),
                                 p(b["lpdf"]), C.byref(good), None) == 1
    assert b"has_env" in L.bsdfd_last_error()
    for bad in (0, 10):
        assert L.bsdfd_wf_sample_env(C.byref(r.scene), p(r.env), C.byref(good), bad, 0, 1, 0, 0, 0, n, *vertex, p(b["lsel"]),
                                     p(b["wl"]), p(b["lpdf"]), p(b["emit"]), None) == 1
    # null arrays
    assert L.bsdfd_env_sample(C.byref(good), n, None, p(out3), p(out1), None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_env_pdf(C.byref(good), n, p(out3), None, None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_env(C.byref(r.scene), p(r.env), C.byref(good), 1, 0, 1, 0, 0, 0, n, *vertex, None, p(b["wl"]), None,
                                 p(b["emit"]), None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_env(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, None, None, p(b["emit"]), None,
                                 C.byref(good), None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_env_sample(None, n, p(u), p(out3), p(out1), None) == 1
    assert L.bsdfd_env_sample(C.byref(good), -1, p(u), p(out3), p(out1), None) == 1
    # N = 0: a no-op
    assert L.bsdfd_env_sample(C.byref(good), 0, None, None, None, None) == 0 and L.bsdfd_env_pdf(C.byref(good), 0, None, None, None) == 0
    assert L.bsdfd_wf_sample_env(C.byref(r.scene), None, C.byref(good), 1, 0, 1, 0, 0, 0, 0, *[None] * 4, None, None, None, None, None) == 0
    assert L.bsdfd_wf_bounce_env(C.byref(r.scene), None, 0, 0, 1, 0, 0, 0, 0, *[None] * len(state), None, None, None, None,
                                 C.byref(good), None) == 0
    torch.cuda.synchronize()
    assert (b["emit"] == EMIT_SENTINEL).all() and (b["lpdf"] == LPDF_SENTINEL).all()   # nothing ran
    assert (out3 == 7.0).all() and (out1 == 7.0).all()
    assert np.array_equal(b["wl"].cpu().numpy(), v["wl"], equal_nan=True)


# ---- images: the 5-ball scene of the lights test (balls, floor and sky in the frame) -------------------------------------------
W, H, SPP = 96, 64, 2
LIGHT_POS, LIGHT_I = (-1.5, 4.0, -1.5), 200.0


def _render(env=None, lights=False, **kw):
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    if lights:
        kw["lights"] = [PointLight(LIGHT_POS, LIGHT_I)]
    return _array(kw, w=W, h=H, env=env, low_camera=True)


def _sky_env():
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    return make_sky(64, 128, seed=5)


@pytest.mark.parametrize("lights", [False, True])
@pytest.mark.parametrize("depth", [1, 3])
def test_cosine_is_the_renderer_without_the_argument(depth, lights):
    a = _render(max_depth=depth, lights=lights).render(1, spp=SPP, seed=4)
    c = _render(max_depth=depth, lights=lights, env_sampling="cosine").render(1, spp=SPP, seed=4)
    assert torch.equal(a, c) and float(a.mean()) > 0


@pytest.mark.parametrize("lights", [False, True])
def test_determinism_and_exact_scaling_with_the_map(lights):
    """Two renders of one seed are equal, another seed differs; and twice the map is twice the film, bit for bit: scaling by a
    power of two commutes with the normalisation of the distribution, so the draws are the same, and every term carries the map
    (with lights: twice the intensity too)."""
    env = _sky_env()
    r = _render(env, lights, max_depth=3, env_sampling="importance")
    a = r.render(1, spp=SPP, seed=5)
    assert torch.isfinite(a).all() and float(a.mean()) > 0
    assert torch.equal(a, r.render(1, spp=SPP, seed=5))
    assert torch.equal(a, _render(env, lights, max_depth=3, env_sampling="importance").render(1, spp=SPP, seed=5))
    assert not torch.equal(a, r.render(1, spp=SPP, seed=6))
    assert not torch.equal(a, _render(env, lights, max_depth=3).render(1, spp=SPP, seed=5))       # (it is another estimator)
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    twice = dict(lights=[PointLight(LIGHT_POS, 2 * LIGHT_I)]) if lights else {}
    b = _array(dict(max_depth=3, env_sampling="importance", **twice), w=W, h=H, env=2 * env, low_camera=True).render(1, spp=SPP, seed=5)
    assert torch.equal(2 * a, b)
    assert len(r.stats["lanes_per_bounce"]) >= 2 and r.stats["lanes_per_bounce"][0] > 0


def _floor_paths(r, seed):
    """One pass at depth 1 -> rad / reflectance [n_floor] of its floor paths (channel 0)."""
    film = torch.zeros((H, W, 3), device=r.device)
    r.render_pass(film, 0, H, SPP, seed, 0)
    torch.cuda.synchronize()
    rad = r._buffers(H * W * SPP)["rad"].cpu().numpy().astype(np.float64)
    first = r.primary(0, H, SPP, seed, 0)                        # the ids and reflectances the pass started from
    mat, refl = first["mat"].cpu().numpy(), first["wi"].cpu().numpy()[:, 0].astype(np.float64)
    floor = mat == len(r.table)
    return rad[floor] / refl[floor, None]


def test_constant_environment_is_integrated_exactly_in_the_mean():
    """A constant environment of 1, depth 1, no occlusion: a floor path estimates its reflectance; the mean of rad / refl over the
    floor paths is 1 within 5 standard errors of that mean."""
    r = _render(torch.ones((8, 16, 3)), max_depth=1, occlusion=False, env_sampling="importance")
    x = _floor_paths(r, 3)[:, 0]
    sem = x.std(ddof=1) / np.sqrt(len(x))
    print(f"floor paths {len(x)}: mean rad / refl {x.mean():.5f} +- {sem:.5f}")
    assert len(x) > 3000 and sem > 0 and abs(x.mean() - 1.0) < 5 * sem


def test_importance_is_the_cosine_renderer_in_the_mean():
    """make_sky(64, 128, 5), depth 2: the mean over the ball pixels, and over the floor pixels, is the cosine renderer's.  The spread
    s of that mean over 8 seeds of the cosine renderer is the yardstick (as in test_environment_with_a_dark_light_...): the
    difference between one render and the cosine mean of 8 has the standard error s sqrt(1 + 1/8); 5 of those are allowed."""
    env = _sky_env()
    cosine = _render(env, max_depth=2)
    n_b = len(cosine.table)
    ids = torch.stack([cosine.primary(0, H, SPP, s, 0)["mat"].reshape(H, W, SPP) for s in range(9)], -1).reshape(H, W, -1)
    film = _render(env, max_depth=2, env_sampling="importance").render(1, spp=SPP, seed=8)
    assert torch.isfinite(film).all()
    cos_films = [cosine.render(1, spp=SPP, seed=s) for s in range(8)]
    for name, px in (("ball", (ids < n_b).all(-1)), ("floor", (ids == n_b).all(-1))):
        assert int(px.sum()) > 300
        means = np.array([float(f[px].mean()) for f in cos_films])
        got, s = float(film[px].mean()), means.std(ddof=1)
        print(f"{name} pixels {int(px.sum())}: importance {got:.5f}, cosine {means.mean():.5f} +- {s:.5f} per seed")
        assert abs(got - means.mean()) < 5 * s * np.sqrt(1 + 1 / 8)


def test_importance_sampling_cuts_the_variance_of_the_floor():
    """The point of the feature.  Depth 1, no occlusion, make_sky(64, 128, 5): the per-path variance of rad / refl over the floor
    paths, cosine over importance, against the same ratio of envmap_ref.plane_estimators on the same sky (about 17).  The device
    must reach half of the reference's: the factor 2 is for the sampling error of a variance estimated from a few thousand
    heavy-tailed paths."""
    env = _sky_env()
    e = env.numpy()
    c_ref, p_ref = ER.plane_estimators(e, ER.build_tables(e), 400_000, seed=1)
    ref = c_ref.var() / p_ref.var()
    cos = _floor_paths(_render(env, max_depth=1, occlusion=False), 3).mean(1)
    imp = _floor_paths(_render(env, max_depth=1, occlusion=False, env_sampling="importance"), 3).mean(1)
    ratio = cos.var() / imp.var()
    print(f"floor paths {len(cos)}: variance cosine {cos.var():.3f} / importance {imp.var():.3f} = {ratio:.1f}; "
          f"reference {c_ref.var():.3f} / {p_ref.var():.3f} = {ref:.1f}")
    assert len(cos) > 3000 and len(cos) == len(imp)
    assert ratio >= 0.5 * ref
