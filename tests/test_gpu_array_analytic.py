"""GPU: the array renderers shade `mybsdf idx = N` balls with their analytic ground truth (analytic.AnalyticTable on the
lane-ordered wavefront), each ball under an albedo of its own.

Four balls carrying the shipped full-sphere nets bsdf_13 / 24 / 1 / 20 — a principled BSDF, a rough dielectric, a second principled
one, and one ball left WITHOUT ground truth, which takes the proxy path — over the checkerboard, seen from the low camera of
tests/test_gpu_pathtrace.py (so that the frame also holds sky), 96x64, 2 spp, 2 passes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import pass_replay as PR  # noqa: E402

W, H, SPP, PASSES, SEED = 96, 64, 2, 2, 4
NAMES = ["bsdf_13_spherical", "bsdf_24_spherical", "bsdf_1_spherical", "bsdf_20_spherical"]
N_BALLS = len(NAMES)
ALBEDO = (0.9, 0.8, 0.7)
COLOUR = (0.9, 0.2, 0.4)
VERTEX = ("org", "nrm", "wi", "wl", "mat")


@pytest.fixture(scope="module")
def scene():
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    _, centers, radii = WF.array0_scene(W, H)
    order = [5, 6, 9, 10]
    cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=W, height=H)
    return dict(table=MaterialTable(NAMES), centers=[centers[i] for i in order], radii=[radii[i] for i in order], camera=cam,
                env=WF.make_sky(64, 128, seed=5), three=ground_truth_for(NAMES[:3]), four=ground_truth_for(NAMES))


def _make(scene, cls, ground_truth, **kw):
    return cls(scene["table"], scene["centers"], scene["radii"], camera=scene["camera"], env=scene["env"],
               ground_truth=ground_truth, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_fused_analytic_ground_truth_renders_the_film_of_the_per_material_loop(scene, monkeypatch):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable
    from bsdf_diffusion_sampling_amd.ground_truth import GroundTruth
    assert sorted(scene["three"]) == [0, 1, 2]
    fused = _make(scene, WF.ArrayRenderer, scene["three"], albedo=ALBEDO)
    loop = _make(scene, WF.ArrayRenderer, scene["three"], albedo=ALBEDO, fused_ground_truth=False)
    assert isinstance(fused.ground_truth_table, AnalyticTable) and fused.measured_table is fused.ground_truth_table
    assert len(fused.ground_truth_table) == N_BALLS and fused.ground_truth_table.entries[3] is None
    assert loop.ground_truth_table is None and loop.measured_table is None
    calls = []
    plain = GroundTruth.eval_t
    monkeypatch.setattr(GroundTruth, "eval_t", lambda self, *a, **k: (calls.append(self), plain(self, *a, **k))[1])
    a = fused.render(PASSES, SPP, seed=SEED)
    assert calls == []                                      # one table launch per pass, no per-material launch at all
    b = loop.render(PASSES, SPP, seed=SEED)
    torch.cuda.synchronize()
    assert len(calls) > 0 and len(calls) % 2 == 0           # the loop: two launches per material that has lanes
    assert a.shape == (H, W, 3) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    # the pass saw all of it: the three balls with ground truth, the ball without, the floor, the sky
    n = H * W * SPP
    buf = fused._buffers(n)
    mat, f_o = buf["mat"], buf["f_o"]
    for m in (0, 1, 2):
        assert int((mat == m).sum()) > 0 and not bool(torch.isnan(f_o[mat == m]).any())
    for m in (3, N_BALLS, N_BALLS + 1):
        assert int((mat == m).sum()) > 0 and bool(torch.isnan(f_o[mat == m]).all())
    assert torch.equal(buf["f_o"].view(torch.int32), loop._buffers(n)["f_o"].view(torch.int32))
    assert torch.equal(buf["f_l"].view(torch.int32), loop._buffers(n)["f_l"].view(torch.int32))
    # the nets sample the whole sphere: the transmission lobe is in the film's estimator (no occlusion here)
    below = (buf["wo"][:, 2] < 0) & (mat < 3)
    assert int(below.sum()) > 0 and bool((f_o[below] >= 0).all()) and bool((f_o[below] > 0).any())


def _record(r, pass_idx=0):
    film = torch.zeros((H, W, 3), dtype=torch.float32, device=r.device)
    with PR.Recorder(r) as rec:
        r.render_pass(film, 0, H, SPP, SEED, pass_idx)
    torch.cuda.synchronize()
    return rec, film


def test_path_tracer_evaluates_the_table_once_per_depth_and_goes_the_same_way(scene):
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    r = _make(scene, PathArrayRenderer, scene["three"], albedo=ALBEDO, max_depth=3)
    plain = _make(scene, PathArrayRenderer, None, albedo=ALBEDO, max_depth=3)
    rec, film = _record(r)
    rec0, film0 = _record(plain)
    lanes = r.stats["lanes_per_bounce"]
    evals, bounces = rec.named("eval_t"), rec.named("bounce")
    assert len(bounces) == 3 and len(lanes) == 3 and all(n > 0 for n in lanes)
    assert len(evals) == sum(1 for n in lanes if n > 0) and rec0.named("eval_t") == []      # once per depth with material lanes
    table = r.ground_truth_table
    for k, s in enumerate(evals):
        assert s["args"]["reads_state"] and s["args"]["writes_state"]
        assert s["args"]["tint"] == [float(v) for v in np.float32(ALBEDO)]
        d = {name: torch.from_numpy(s["before"][name]).to(r.device) for name in ("mat", "wi", "wo", "wl")}
        want_o, want_l = (x.cpu().numpy() for x in table.eval_t(d["mat"], d["wi"], d["wo"], d["wl"], tint=s["args"]["tint"]))
        mat = s["before"]["mat"]
        gt = (mat >= 0) & (mat < 3)
        assert gt.sum() > 0, k
        for got, want in ((s["after"]["f_o"], want_o), (s["after"]["f_l"], want_l)):
            assert np.array_equal(_bits(got[gt]), _bits(want[gt])) and np.isfinite(got[gt]).all(), k
            assert np.isnan(got[~gt]).all(), k             # the floor, misses, ended paths, the ball without ground truth
        for other in (3, N_BALLS, N_BALLS + 1) if k == 0 else (N_BALLS + 1,):
            assert (mat == other).sum() > 0, (k, other)
    # where a path goes does not depend on f: the vertices after every bounce are those of the renderer without ground truth
    for k, (s, s0) in enumerate(zip(bounces, rec0.named("bounce"))):
        for name in VERTEX:
            assert np.array_equal(_bits(s["after"][name]), _bits(s0["after"][name])), (k, name)
    assert not np.array_equal(bounces[-1]["after"]["rad"], rec0.named("bounce")[-1]["after"]["rad"])
    assert bool(torch.isfinite(film).all()) and bool(torch.isfinite(film0).all()) and not torch.equal(film, film0)


@pytest.mark.parametrize("path", [True, False])
def test_a_common_ball_albedo_is_the_scene_wide_albedo(scene, path):
    """Every ball has ground truth; ``ball_albedo`` = one colour c on every ball against ``albedo=c``: the effective tint is the
    same single fp32 product (1 * c and c * 1), so at one bounce the films are equal bit for bit."""
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    cls, kw = (PathArrayRenderer, dict(max_depth=1)) if path else (WF.ArrayRenderer, {})
    per_ball = _make(scene, cls, scene["four"], ball_albedo=[COLOUR] * N_BALLS, **kw)
    scene_wide = _make(scene, cls, scene["four"], albedo=COLOUR, **kw)
    white = _make(scene, cls, scene["four"], **kw)
    assert per_ball.ground_truth_table.albedo == [COLOUR] * N_BALLS and scene_wide.ground_truth_table.albedo == [(1.0, 1.0, 1.0)] * N_BALLS
    a, b, c = (r.render(1, SPP, seed=SEED) for r in (per_ball, scene_wide, white))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(a, c)
    # a colour per ball reaches the film: the same scene with the colours of two balls exchanged is another image
    colours = [(0.1, 0.9, 0.9), (0.9, 0.1, 0.9), (0.9, 0.8, 0.8), (0.1, 0.9, 0.4)]
    d = _make(scene, cls, scene["four"], ball_albedo=colours, **kw).render(1, SPP, seed=SEED)
    e = _make(scene, cls, scene["four"], ball_albedo=colours[::-1], **kw).render(1, SPP, seed=SEED)
    assert bool(torch.isfinite(d).all()) and not torch.equal(d, e)


def test_arguments_that_cannot_be_served_are_refused(scene, tmp_path):
    from bsdf_diffusion_sampling_amd import measured_synth as F
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    colours = [COLOUR] * N_BALLS
    measured = MeasuredBSDF(F.write_isotropic(str(tmp_path / "iso_synth_rgb.bsdf")))
    for cls in (WF.ArrayRenderer, PathArrayRenderer):
        with pytest.raises(ValueError, match="every ball"):          # ball 3 would take the proxy
            _make(scene, cls, scene["three"], ball_albedo=colours)
        with pytest.raises(ValueError, match="every ball"):          # no ground truth at all
            _make(scene, cls, None, ball_albedo=colours)
        with pytest.raises(ValueError, match="fused_ground_truth"):
            _make(scene, cls, scene["four"], ball_albedo=colours, fused_ground_truth=False)
        with pytest.raises(ValueError, match="one RGB triple per ball"):
            _make(scene, cls, scene["four"], ball_albedo=colours[:3])
        with pytest.raises(ValueError, match="not a mixture"):
            _make(scene, cls, {0: scene["four"][0], 1: measured})
        with pytest.raises(ValueError, match="every ball"):          # measured ground truth has no per-ball factor
            _make(scene, cls, {m: measured for m in range(N_BALLS)}, ball_albedo=colours)
    # the path tracer keeps refusing the per-material loop
    with pytest.raises(ValueError, match="lane-ordered"):
        _make(scene, PathArrayRenderer, scene["three"], fused_ground_truth=False)
