"""The reference pass of tests/pass_replay.py held to itself in two precisions: on whole passes over real scenes — where deep
bounces serve tens of lanes, the floor can be 1e3 away and ``wi`` comes out of the continuation — the fp32 and the fp64 run follow
the same paths on all but 0.1 % of them and agree on ``rad`` within the shade bound.  The caps tests/test_gpu_pass_replay.py holds
the device to are ones the arithmetic alone respects."""
import numpy as np
import pytest

import envmap_ref as ER
import pass_replay as PR
import pathtrace_lights_ref as LR

ORDER = [5, 6, 9, 10, 1]          # the balls of tests/test_gpu_pathtrace.py::_array
SEED = 4
# pathtrace_lights_ref.synthetic_lights() (around the origin) moved by (-1.7, 0, -1.5), the middle of the five balls: one overhead,
# one to the side, one 0.45 above the floor between the balls
LIGHT_POSITIONS = [(-1.7, 2.5, -1.0), (-3.2, 1.2, -0.5), (-0.3, 0.45, -0.6)]


def five_ball_lights():
    return LR.make_lights(LIGHT_POSITIONS, list(LR.synthetic_lights()["intensity"]))


def _shade_bound(got, want):
    """The project's shading bound: relative error with a 1e-3 floor -> (p99.9, max), held to 2e-4 and 5e-3."""
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    return np.percentile(err, 99.9), err.max()


def five_ball_scene(w, h, low_camera=True):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    cam, centers, radii = WF.array0_scene(w, h)
    if low_camera:
        cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=w, height=h)
    return PR.scene_dict(cam, [centers[i] for i in ORDER], [radii[i] for i in ORDER])


def _twelve_ball_scene(w, h):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    return PR.scene_dict(*WF.array0_scene(w, h))


def _sky():
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    return make_sky(64, 128, seed=5).numpy()


# name: (scene, rows, balls in the frame at bounce 0, sky in the frame).  The 12-ball scene keeps the reference scene's own camera,
# which looks down on the array: none of its primary rays reaches the sky, and rows 7..29 of 48 do not hold the twelfth ball
SCENES = {"5 balls, 120x90": (lambda: five_ball_scene(120, 90), None, 5, True),
          "12 balls, 64x48": (lambda: _twelve_ball_scene(64, 48), None, 12, False),
          "12 balls, 64x48, rows 7..29": (lambda: _twelve_ball_scene(64, 48), (7, 29), 11, False)}


def _two_precisions(scene, mode, lights, rows, depth=4, spp=2):
    env = _sky()
    tables = ER.build_tables(env) if mode == "importance" else None
    r0, r1 = rows or (0, scene["height"])
    return [PR.reference_pass(scene, env, mode, lights, tables, r0, r1, spp, SEED, 0, depth, True, PR.mock_answers(11), dtype=dt)
            for dt in (np.float64, np.float32)]


def _check(tag, scene, a, b, balls_in_frame, sky_in_frame):
    n_b, n = len(scene["spheres"]), len(a["rad"])
    differ = PR.histories_differ(a["history"], b["history"])
    p999, worst = _shade_bound(b["rad"][~differ].astype(np.float64), a["rad"][~differ])
    lanes = [int((PR.ids_of(m) < n_b).sum()) for m in a["history"][:-1]]
    print(f"{tag}: histories differ on {int(differ.sum())} of {n} paths; rad p99.9 {p999:.2e} max {worst:.2e}; "
          f"ball lanes per bounce {lanes}")
    assert differ.sum() <= n // 1000
    assert np.isfinite(b["rad"]).all() and p999 < 2e-4 and worst < 5e-3
    first = PR.ids_of(a["history"][0])
    seen = set(np.unique(first).tolist())
    assert sum(m in seen for m in range(n_b)) == balls_in_frame and n_b in seen      # the balls and the floor at bounce 0
    assert (n_b + 1 in seen) == sky_in_frame                                          # and "miss"
    assert len(lanes) == 4 and lanes[-1] >= 20
    return differ


@pytest.mark.parametrize("name", list(SCENES))
def test_reference_pass_follows_the_same_paths_in_fp32_and_fp64(name):
    make, rows, balls_in_frame, sky_in_frame = SCENES[name]
    scene = make()
    a, b = _two_precisions(scene, "cosine", None, rows)
    _check(f"cosine, {name}", scene, a, b, balls_in_frame, sky_in_frame)


@pytest.mark.parametrize("mode,lit", [("cosine", True), ("importance", False)])
def test_reference_pass_with_lights_and_with_importance_tables(mode, lit):
    """The same once with three lights and once with the importance tables of make_sky(64, 128, 5), on the 5-ball scene."""
    scene = five_ball_scene(120, 90)
    lights = five_ball_lights() if lit else None
    a, b = _two_precisions(scene, mode, lights, None)
    differ = _check(f"{mode}, lights={lit}", scene, a, b, 5, True)
    for (name, k, sa), (_, _, sb) in zip(a["stages"], b["stages"]):
        if name == "sample_emitter":
            assert np.array_equal(sa["lsel"], sb["lsel"])
            flips = int((sa["lit_point"] != sb["lit_point"])[~differ].sum())
            assert flips <= len(differ) // 1000, (k, flips)
        if name == "sample_env":
            flips = int((sa["lit_env"] != sb["lit_env"])[~differ].sum())
            assert flips <= len(differ) // 1000, (k, flips)
