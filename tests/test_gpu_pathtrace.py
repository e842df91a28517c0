"""GPU tests of the array-scene path tracer: the bounce kernel (csrc/pathtrace.hip) row by row against tests/pathtrace_ref.py and
against a closed form, and ``PathArrayRenderer`` (bsdf_diffusion_sampling_amd/pathtrace.py) at the level of images — depth 1 is
``ArrayRenderer``, occlusion only removes light, depth only adds it, a furnace stays a furnace, ended paths cost no flow lanes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_ref as B  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from test_pathtrace_cpu import STATE, _floor_vertices, form_factor_complement  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ["chm_orange_rgb_disk", "aniso_miro_7_rgb_spherical", "vch_silk_blue_rgb_disk", "aniso_copper_sheet_rgb_disk",
         "aurora_white_rgb_spherical"]


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")


def _scene_renderer(scene, env):
    """A PathArrayRenderer over the balls of a reference scene dict (its flow nets are not used: the kernels are called directly)."""
    _gpu()
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    from bsdf_diffusion_sampling_amd.wavefront import Camera
    pl = scene["plane"]
    n_b = len(scene["spheres"])
    return PathArrayRenderer(MaterialTable(STEMS[:n_b]), [c for c, _ in scene["spheres"]], [r for _, r in scene["spheres"]],
                             camera=Camera(origin=scene["origin"], width=64, height=64), env=torch.from_numpy(env),
                             checker=(pl["c0"], pl["c1"], pl["scale"]), albedo=scene["albedo"])


def _to_device(r, state):
    """The arrays of a reference state as the renderer's buffer dict (which calls the ids ``mat``)."""
    return {"mat" if k == "material" else k: torch.from_numpy(np.ascontiguousarray(v)).to(r.device) for k, v in state.items()}


def _scene_dict(r):
    """The reference's scene dict of a renderer."""
    sc = r.scene
    spheres = [(list(sc.sphere_center), sc.sphere_radius)]
    spheres += [(list(sc.extra_spheres[k])[:3], sc.extra_spheres[k][3]) for k in range(sc.n_extra_spheres)]
    return dict(origin=list(sc.cam_origin), albedo=list(sc.albedo), spheres=spheres,
                plane=dict(y=sc.plane_y, c0=sc.checker_color0, c1=sc.checker_color1, scale=sc.checker_scale))


def _array(cls_kwargs=None, w=120, h=90, gt=False, env=None, path=True, low_camera=False, **scene_kw):
    """The 5-ball scene of tests/test_gpu_wavefront.py (_array_renderer), as an ArrayRenderer or a PathArrayRenderer.
    ``low_camera``: seen from 1.2 above the floor instead of 4.9, so that the frame also holds sky (that scene's camera sees
    none: every primary ray lands on a ball or on the floor)."""
    _gpu()
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    cam, centers, radii = WF.array0_scene(w, h)
    if low_camera:
        cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=w, height=h)
    order = [5, 6, 9, 10, 1]
    gts = {}
    if gt:
        from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF
        gts = {0: MeasuredBSDF(os.path.join(ROOT, "tests", "golden", "chm_orange_rgb.bsdf"))}
    cls = PathArrayRenderer if path else WF.ArrayRenderer
    return cls(MaterialTable(STEMS), [centers[i] for i in order], [radii[i] for i in order], camera=cam, env=env,
               ground_truth=gts, **scene_kw, **(cls_kwargs or {}))


def _shade_bound(got, want):
    """The bound of test_array_scene_matches_oracle: relative error with a 1e-3 floor, p99.9 < 2e-4, max < 5e-3."""
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    return np.percentile(err, 99.9), err.max()


@pytest.fixture(scope="module")
def synth():
    return R.synthetic_vertices(), R.synthetic_env()


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("bounce", [0, 2])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("occlusion", [0, 1])
def test_bounce_kernel_matches_reference(synth, occlusion, last, bounce, with_f):
    """4096 synthetic vertices over 3 balls and the floor (ball, floor and ended rows; wo below the surface; pdf 0 / inf / NaN; NaN
    rows in f) through ONE bsdfd_wf_bounce call, row by row against the fp64 reference."""
    v, env = synth
    if not with_f:
        v = {k: a for k, a in v.items() if k not in ("f_o", "f_l")}
    scene = R.SYNTH_SCENE
    n_b, n = len(scene["spheres"]), len(v["material"])
    seed, pass_idx, offset = 0x1234567890ABCDEF, 3, (1 << 32) - 2000     # (the path index crosses 2^32 inside the wavefront)
    want = B.bounce(scene, env, "cosine", bounce, bool(last), bool(occlusion), seed, pass_idx, offset, *[v.get(k) for k in STATE])
    r = _scene_renderer(scene, env)
    b = _to_device(r, v)
    r.bounce(b, bounce, bool(last), seed, pass_idx, offset, occlusion=bool(occlusion))
    torch.cuda.synchronize()
    got = {k: b["mat" if k == "material" else k].cpu().numpy() for k in ("org", "nrm", "wi", "wl", "material", "beta", "rad")}
    live = (v["material"] >= 0) & (v["material"] <= n_b)
    # ended paths: not a byte of their state moves
    for k in got:
        assert np.array_equal(got[k][~live], v[k][~live], equal_nan=True), k
    differ = got["material"] != want["material"]
    print(f"occlusion={occlusion} last={last} bounce={bounce} f={with_f}: {int(differ.sum())} of {n} rows decide differently")
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
            print(f"  {k}: max error {e_ok:.2e} ({e_all:.2e} with the {int(graze.sum())} grazing hits)")
            assert e_ok < 2e-5 and e_all < 2e-3, k
        e_wl = np.abs(got["wl"][cont] - R.next_wl(seed, pass_idx, bounce, offset, n)[cont]).max()
        print(f"  wl: max error {e_wl:.2e}")
        assert e_wl < 2e-6
    # rows that end keep the rest of their state
    ended = same & ~cont
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert np.array_equal(got[k][ended], v[k][ended], equal_nan=True), k
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same])
    print(f"  rad: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3


@pytest.mark.parametrize("occlusion,last,bounce,keys", [(1, 0, 2, ("org", "nrm", "wi", "wl", "material", "beta", "rad")),
                                                        (0, 1, 0, ("material", "rad"))])
def test_bounce_kernel_is_bit_identical_to_the_recording(synth, occlusion, last, bounce, keys):
    """The synthetic vertices (f_o and f_l given, the arguments of test_bounce_kernel_matches_reference) through ONE
    bsdfd_wf_bounce call: every output array is, bit for bit, what the kernel wrote before it shared its light sample, floor
    term and pdf / ground-truth tests with primary_kernel and shade_kernel (tests/golden/bounce_kernel_before_sharing.npz)."""
    v, env = synth
    r = _scene_renderer(R.SYNTH_SCENE, env)
    b = _to_device(r, v)
    r.bounce(b, bounce, bool(last), 0x1234567890ABCDEF, 3, (1 << 32) - 2000, occlusion=bool(occlusion))
    torch.cuda.synchronize()
    before = np.load(os.path.join(ROOT, "tests", "golden", "bounce_kernel_before_sharing.npz"))
    for k in keys:
        got = b["mat" if k == "material" else k].cpu().numpy()
        assert np.array_equal(got, before[f"occlusion{occlusion}_last{last}_bounce{bounce}_{k}"], equal_nan=True), k


def test_path_begin_and_resolve_match_reference():
    """The two small kernels on a real primary wavefront of the 5-ball scene (an odd tile: rows 5..57 of 64, 3 spp)."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=5)
    r = _array(env=env, w=96, h=64, low_camera=True)
    rows, spp = (5, 57), 3
    b = r.primary(rows[0], rows[1], spp, seed=4, pass_idx=1)
    r.path_begin(b)
    film = torch.full((rows[1] - rows[0], r.camera.width, 3), 0.25, device=r.device)
    r.resolve(rows[0], rows[1], spp, b, film)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in b.items() if isinstance(v, torch.Tensor)}
    org, beta, rad = R.path_begin(_scene_dict(r), env.numpy(), h["dir"], h["nrm"], h["mat"])
    n_b = len(r.table)
    assert (h["beta"] == 1).all() and np.isfinite(h["org"]).all()
    hit = h["mat"] <= n_b
    assert all((h["mat"] == m).sum() >= 10 for m in range(n_b)) and all((h["mat"] == m).sum() > 1000 for m in (n_b, n_b + 1))
    # the primary-ray bound where positions are O(1); a floor point near the horizon is 1e3..1e5 away, where an fp32 position is
    # held to its own grid instead: quotient, product and sum round once each, <= 1.5 ulp <= 1.8e-7 |x|; 4e-7 |x| allowed
    err = np.abs(h["org"][hit] - org[hit]).max(1)
    size = np.abs(org[hit]).max(1)
    print(f"org: max error {err[size < 16].max():.2e} within 16 of the origin, max error / |x| {(err / np.maximum(size, 1)).max():.2e}, "
          f"farthest floor point {size.max():.3g}")
    assert (err < 2e-5 + 4e-7 * size).all()
    assert (h["rad"][hit] == 0).all()
    p999, worst = _shade_bound(h["rad"], rad)
    assert p999 < 2e-4 and worst < 5e-3
    want = 0.25 + R.resolve(h["rad"], spp)
    assert np.abs(film.cpu().numpy().reshape(-1, 3) - want).max() < 1e-5 * max(1.0, want.max())


@pytest.mark.parametrize("d", [0.2, 0.33, 0.7, 1.5])
def test_tangent_sphere_form_factor_on_the_device(d):
    """Floor vertices at distance d from the contact point of a ball resting on the plane, unit environment and reflectance,
    occlusion on, last = 1: the mean of rad is 1 - r^3 / (d^2 + r^2)^(3/2), within 5 sigma of the binomial standard error."""
    n = 65536
    scene, st = _floor_vertices(d, n, seed=int(d * 100) + 1)
    r = _scene_renderer(scene, np.ones((4, 8, 3), np.float32))
    b = _to_device(r, st)
    r.bounce(b, 0, True, 1, 0, 0, occlusion=True)
    torch.cuda.synchronize()
    vals = b["rad"].cpu().numpy().astype(np.float64)
    assert (b["mat"] == 2).all()
    assert ((vals == 0) | (np.abs(vals - 1) < 1e-6)).all()
    want = form_factor_complement(d)
    sigma = np.sqrt(want * (1 - want) / n)
    got = vals[:, 0].mean()
    print(f"d = {d}: mean {got:.6f}, closed form {want:.6f}, {(got - want) / sigma:+.2f} sigma")
    assert abs(got - want) < 5 * sigma


@pytest.mark.parametrize("gt", [False, True])
def test_depth_one_is_the_array_renderer(gt):
    """PathArrayRenderer(max_depth=1) against ArrayRenderer: same material ids after primary, the same film within the shade
    bound; and ArrayRenderer's own film is, bit for bit, the one recorded before the path tracer existed
    (tests/golden/array_renderer_before_pathtrace.npz: this scene, 120x90, spp 2, one pass, seed 4)."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=5)
    old, new = _array(path=False, gt=gt, env=env), _array(dict(max_depth=1), gt=gt, env=env)
    assert new.occlusion is False
    a, b = old.render(1, spp=2, seed=4), new.render(1, spp=2, seed=4)
    torch.cuda.synchronize()
    n = old.camera.height * old.camera.width * 2
    assert torch.equal(old._buffers(n)["mat"], new.primary(0, old.camera.height, 2, 4, 0)["mat"])
    p999, worst = _shade_bound(b.cpu().numpy().reshape(-1, 3), a.cpu().numpy().reshape(-1, 3).astype(np.float64))
    print(f"gt={gt}: depth 1 vs ArrayRenderer p99.9 {p999:.2e} max {worst:.2e}; bit-identical: {torch.equal(a, b)}")
    assert torch.isfinite(b).all() and p999 < 2e-4 and worst < 5e-3
    before = np.load(os.path.join(ROOT, "tests", "golden", "array_renderer_before_pathtrace.npz"))["gt" if gt else "proxy"]
    assert torch.equal(a.cpu(), torch.from_numpy(before))


def test_occlusion_removes_light_and_depth_adds_it():
    """Same seed, same draws: on floor pixels a shadow ray can only remove the environment term, and every deeper vertex only adds
    a non-negative one — element-wise, exactly (fp32 addition is monotone)."""
    w, h = 96, 64
    imgs = {}
    for name, kw in (("open1", dict(max_depth=1, occlusion=False)), ("occl1", dict(max_depth=1, occlusion=True)),
                     ("occl3", dict(max_depth=3))):
        r = _array(kw, w=w, h=h)
        imgs[name] = r.render(2, spp=2, seed=3)
    assert r.occlusion is True                                    # occlusion=None means max_depth > 1
    mat = r.primary(0, h, 2, 3, 0)["mat"].reshape(h, w, 2)
    floor = (mat == len(r.table)).all(-1)                         # both samples of the pixel see the floor (pass 0's ids;
    mat1 = r.primary(0, h, 2, 3, 1)["mat"].reshape(h, w, 2)       #  and pass 1's)
    floor &= (mat1 == len(r.table)).all(-1)
    assert int(floor.sum()) > 1000
    o1, c1, c3 = (imgs[k][floor] for k in ("open1", "occl1", "occl3"))
    assert (c1 <= o1).all() and (c1 < o1).any()
    assert (c3 >= c1).all() and (c3 > c1).any()
    print(f"floor pixels {int(floor.sum())}: shadowed {int((c1 < o1).any(-1).sum())}, brightened by depth {int((c3 > c1).any(-1).sum())}")


def test_furnace():
    """Unit environment, albedo 1, white floor, proxy shading: nothing can exceed what the one-bounce furnace allows, pixels that
    miss everything are 1, and depth only adds."""
    env = torch.ones((8, 16, 3))
    w, h = 96, 64
    means = []
    for depth in (1, 2, 4):
        r = _array(dict(max_depth=depth, occlusion=True), w=w, h=h, env=env, checker=(1.0, 1.0, 2.0), low_camera=True)
        img = r.render(4, spp=4, seed=1)
        assert torch.isfinite(img).all()
        ids = torch.stack([r.primary(0, h, 4, 1, k)["mat"].reshape(h, w, 4) for k in range(4)], -1).reshape(h, w, -1)
        miss = (ids == len(r.table) + 1).all(-1)
        ball = (ids < len(r.table)).all(-1)
        assert int(miss.sum()) > 50 and int(ball.sum()) > 100
        assert torch.allclose(img[miss], torch.ones_like(img[miss]), atol=1e-5, rtol=0)
        means.append(float(img[ball].mean()))
    print("furnace means over ball pixels at depth 1, 2, 4:", means)
    assert all(m <= 1.08 for m in means)
    assert means[0] <= means[1] <= means[2]


@pytest.mark.parametrize("floor", [True, False])
def test_compaction_lanes_per_bounce(floor):
    """stats['lanes_per_bounce'][k] = the rows that carry a material when bounce k begins: ended paths are not served, and fewer
    rows are served at bounce 1 than at bounce 0.  (Without a floor that is forced: a path reaches bounce 1 only from a ball,
    through a BSDF sample that hits another ball.  With it, floor paths that land on a ball gain a material; in this scene
    they are fewer than the ball paths that leave.)  The live paths as a whole never grow."""
    h, w, spp = 64, 96, 2
    r = _array(dict(max_depth=3), w=w, h=h, floor=floor)
    n_b = len(r.table)
    film = torch.zeros((h, w, 3), device=r.device)
    entering, live = [], []
    bounce = r.bounce

    def spy(b, *a, **k):
        entering.append(int((b["mat"] < n_b).sum()))
        live.append(int((b["mat"] <= n_b).sum()))
        return bounce(b, *a, **k)
    r.bounce = spy
    r.render_pass(film, 0, h, spp, seed=2, pass_idx=0)
    lanes = r.stats["lanes_per_bounce"]
    print(f"floor={floor}: material lanes per bounce {lanes}, live paths {live}, wavefront {h * w * spp}")
    assert lanes == entering and 2 <= len(lanes) <= 3 and lanes[0] > 0
    assert live[1] < live[0] and all(y <= x for x, y in zip(live, live[1:]))
    assert 0 < lanes[1] < lanes[0]


def test_determinism():
    r = _array(dict(max_depth=3), w=96, h=64)
    a = r.render(2, spp=2, seed=5)
    assert torch.equal(a, r.render(2, spp=2, seed=5))
    assert torch.equal(a, _array(dict(max_depth=3), w=96, h=64).render(2, spp=2, seed=5))
    assert not torch.equal(a, r.render(2, spp=2, seed=6))


def test_errors(synth):
    import ctypes as C
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    with pytest.raises(ValueError, match="max_depth must be >= 1"):
        _array(dict(max_depth=0))
    with pytest.raises(ValueError, match="needs occlusion"):
        _array(dict(max_depth=2, occlusion=False))
    v, env = synth
    r = _scene_renderer(R.SYNTH_SCENE, env)
    b = _to_device(r, v)
    with pytest.raises(RuntimeError, match="bounce must be >= 0"):
        r.bounce(b, -1, False, 0, 0, 0)
    one = {k: t for k, t in b.items() if k != "f_l"}
    with pytest.raises(RuntimeError, match="both NULL or both given"):
        r.bounce(one, 0, False, 0, 0, 0)
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    args = [p(b["mat" if k == "material" else k]) for k in STATE]
    n = len(v["material"])
    for missing in (0, 4, 7):                                     # org, material, wo
        bad = list(args)
        bad[missing] = None
        assert L.bsdfd_wf_bounce(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *bad, None) == 1
        assert b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce(C.byref(r.scene), None, 0, 0, 1, 0, 0, 0, n, *args, None) == 1
    assert L.bsdfd_wf_bounce(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, 0, *([None] * 12), None) == 0      # N = 0: a no-op
    assert L.bsdfd_wf_path_begin(C.byref(r.scene), p(r.env), n, None, p(b["nrm"]), p(b["mat"]), p(b["org"]), p(b["beta"]),
                                 p(b["rad"]), None) == 1
    assert L.bsdfd_wf_resolve(C.byref(r.scene), 0, 1, 1, None, p(b["rad"]), None) == 1
    assert L.bsdfd_wf_resolve(C.byref(r.scene), 0, 65, 1, p(b["rad"]), p(b["rad"]), None) == 1
    assert b"row range" in L.bsdfd_last_error()
    torch.cuda.synchronize()
    assert isinstance(r, PathArrayRenderer)
