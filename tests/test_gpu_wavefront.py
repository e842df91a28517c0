"""GPU parity of the wavefront harness (csrc/wavefront.hip) against oracle/wavefront_oracle.py, and
renderer-level properties (row-split invariance, white furnace)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import wavefront_oracle as WO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _renderer(material="aniso_miro_7_rgb", plugin="disk", w=96, h=64, env=None, albedo=(1.0, 1.0, 1.0), gt=False):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from bsdf_diffusion_sampling_amd import wavefront as WF
    if plugin == "disk":
        from bsdf_diffusion_sampling_amd.brdf_measured_disk import MyBSDF
    else:
        from bsdf_diffusion_sampling_amd.brdf_measured_spherical import MyBSDF
    props = {"filename": material, "albedo": list(albedo)}
    if gt:
        props["measured_dir"] = os.path.join(ROOT, "tests", "golden")
    plug = MyBSDF(props)
    return WF.WavefrontRenderer(plug, WF.Camera(width=w, height=h), env=env)


def _scene_dict(r):
    cam = r.camera
    rt, up, fw = cam.basis()
    return dict(origin=cam.origin, right=rt, up=up, forward=fw, tan_half_fov=math.tan(math.radians(cam.fov_deg) / 2),
                width=cam.width, height=cam.height, center=(0, 0, 0), radius=1.0,
                albedo=[float(a) for a in r.plugin.albedo.tolist()])


def test_primary_matches_oracle():
    r = _renderer()
    spp = 3
    for rows in ((0, r.camera.height), (17, 40)):
        b = r.primary(rows[0], rows[1], spp, seed=0x1234567890, pass_idx=7)
        torch.cuda.synchronize()
        wi_o, wl_o, n_o, d_o = WO.primary(_scene_dict(r), rows[0], rows[1], spp, seed=0x1234567890, pass_idx=7)
        got = {k: b[k].cpu().numpy() for k in ("wi", "wl", "nrm", "dir")}
        assert np.abs(got["dir"] - d_o).max() < 1e-6       # same Philox draws (jitter), same camera
        assert np.abs(got["wl"] - wl_o).max() < 2e-6
        hit_g, hit_o = (got["nrm"] != 0).any(1), (n_o != 0).any(1)
        assert (hit_g != hit_o).sum() <= 2                   # silhouette rays: the discriminant's last ulp
        both = hit_g & hit_o
        # the normal at a grazing hit is ill-conditioned (sqrt of a tiny discriminant): compare where it is not
        graze = -(d_o * n_o).sum(1) < 0.1
        ok = both & ~graze
        assert np.abs(got["nrm"][ok] - n_o[ok]).max() < 2e-5
        assert np.abs(got["wi"][ok] - wi_o[ok]).max() < 2e-5
        assert np.abs(got["nrm"][both] - n_o[both]).max() < 2e-3
        assert (got["wi"][~hit_g] == [0, 0, 1]).all()


@pytest.mark.parametrize("plugin", ["disk", "spherical"])
def test_shade_matches_oracle(plugin):
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=3)
    r = _renderer(plugin=plugin, env=env, albedo=(0.9, 0.6, 0.3))
    spp, rows = 2, (8, 56)
    film = torch.zeros((rows[1] - rows[0], r.camera.width, 3), device=r.device)
    r.render_pass(film, rows[0], rows[1], spp, seed=11, pass_idx=2)
    torch.cuda.synchronize()
    b = {k: v.cpu().numpy() for k, v in r._buffers((rows[1] - rows[0]) * r.camera.width * spp).items()}
    want = WO.shade(_scene_dict(r), env.numpy(), spp, b["wo"], b["pdf_o"], b["wl"], b["pdf_l"], b["nrm"], b["dir"])
    got = film.cpu().numpy().reshape(-1, 3)
    assert np.isfinite(got).all()
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    assert np.percentile(err, 99.9) < 2e-4 and err.max() < 5e-3, (np.percentile(err, 99.9), err.max())
    # the sampler call inside the pass is the plugin's own pair: pdf_l == plugin.pdf_t(wi, wl) up to fp32 noise (the fused
    # launch carries the Jacobian in forward mode, the single-op kernel forms it by meeting in the middle)
    from conftest import same_density
    pl = r.plugin.pdf_t(torch.from_numpy(b["wi"]).to(r.device), torch.from_numpy(b["wl"]).to(r.device))
    assert same_density(pl, b["pdf_l"])


def test_row_split_invariance_and_pass_streams():
    r = _renderer()
    full = r.render(passes=2, spp=2, seed=5)
    h = r.camera.height
    parts = [r.render(passes=2, spp=2, seed=5, rows=(a, b)) for a, b in ((0, 13), (13, 40), (40, h))]
    assert torch.equal(torch.cat(parts, 0), full)            # image independent of the tile split
    assert not torch.equal(r.render(passes=2, spp=2, seed=6), full)
    one = r.render(passes=1, spp=2, seed=5)
    assert not torch.equal(one, full)                        # the second pass uses a new RNG stream


@pytest.mark.parametrize("plugin,material", [("disk", "chm_orange_rgb"), ("spherical", "chm_orange_rgb")])
def test_white_furnace(plugin, material):
    """Constant unit environment, albedo 1: misses are exactly 1; hits estimate the mass the flow puts on
    valid directions (<= 1, close to 1), and the two MIS strategies partition it — a double-counting bug
    would give ~2, a dropped strategy ~0.5."""
    env = torch.ones((8, 16, 3))
    r = _renderer(material=material, plugin=plugin, env=env, w=64, h=64)
    img = r.render(passes=8, spp=4, seed=1).cpu().numpy()
    b = r.primary(0, 64, 1, seed=1, pass_idx=0)
    hit = (b["nrm"].cpu().numpy() != 0).any(1).reshape(64, 64)
    yy, xx = np.mgrid[0:64, 0:64]
    inner = ((xx - 31.5) ** 2 + (yy - 31.5) ** 2) < 10 ** 2  # well inside the silhouette (near-normal view)
    assert inner.sum() > 100 and hit[inner].all()
    corner = ~hit
    corner[1:-1, 1:-1] &= ~(hit[:-2, 1:-1] | hit[2:, 1:-1] | hit[1:-1, :-2] | hit[1:-1, 2:])
    assert np.allclose(img[corner & (np.minimum(xx, yy) < 4)], 1.0, atol=1e-5)
    m = img[inner].mean()
    assert 0.85 < m < 1.08, m


def test_error_paths():
    r = _renderer()
    with pytest.raises(RuntimeError, match="row range"):
        r.primary(0, r.camera.height + 1, 1, 0, 0)
    with pytest.raises(RuntimeError, match="spp"):
        r.primary(0, 4, 0, 0, 0, out=r._buffers(16))
    with pytest.raises(ValueError, match="film"):
        r.shade(0, 4, 1, r._buffers(4 * r.camera.width), torch.zeros((3, r.camera.width, 3), device=r.device))


def test_sharded_render_two_ranks_one_gpu(tmp_path):
    """Image-tile split over 2 processes (gloo, both on the one GPU of the test box): the gathered image
    equals the single-process image bit for bit."""
    script = tmp_path / "r.py"
    script.write_text(f"""
import sys, os, torch, torch.distributed as dist
sys.path.insert(0, {ROOT!r})
from bsdf_diffusion_sampling_amd import wavefront as WF
from bsdf_diffusion_sampling_amd.brdf_measured_disk import MyBSDF
dist.init_process_group("gloo")
torch.cuda.set_device(0)
r = WF.WavefrontRenderer(MyBSDF({{"filename": "aniso_miro_7_rgb"}}), WF.Camera(width=64, height=50))
tile = r.render_sharded(passes=2, spp=2, seed=9, gather=False)
from bsdf_diffusion_sampling_amd.sharding import gather_to_root
full = gather_to_root(tile.reshape(tile.shape[0], -1).cpu(), 50)
if dist.get_rank() == 0:
    ref = r.render(passes=2, spp=2, seed=9).cpu()
    assert torch.equal(full.reshape(50, 64, 3), ref)
    print("SHARDED_OK", flush=True)
dist.destroy_process_group()
""")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29617", str(script)],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "SHARDED_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("plugin", ["disk", "spherical"])
def test_ground_truth_shading_matches_oracle_and_proxy(plugin):
    """With measuredbsdfs/<material>.bsdf present the harness weighs samples with the real f (the
    reference's loop: eval() per sample); kernel vs oracle on the same buffers, and the proxy render
    of the same material agrees in the mean (the net is trained to pdf ∝ lum(f cos))."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=3)
    r = _renderer(material="chm_orange_rgb", plugin=plugin, env=env, albedo=(1.0, 1.0, 1.0), gt=True)
    assert r.use_ground_truth
    spp, rows = 2, (8, 56)
    film = torch.zeros((rows[1] - rows[0], r.camera.width, 3), device=r.device)
    r.render_pass(film, rows[0], rows[1], spp, seed=11, pass_idx=2)
    torch.cuda.synchronize()
    b = {k: v.cpu().numpy() for k, v in r._buffers((rows[1] - rows[0]) * r.camera.width * spp).items()}
    want = WO.shade(_scene_dict(r), env.numpy(), spp, b["wo"], b["pdf_o"], b["wl"], b["pdf_l"], b["nrm"], b["dir"],
                    f_o=b["f_o"], f_l=b["f_l"])
    got = film.cpu().numpy().reshape(-1, 3)
    assert np.isfinite(got).all()
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    assert np.percentile(err, 99.9) < 2e-4 and err.max() < 5e-3, (np.percentile(err, 99.9), err.max())
    # f_o is the plugin's eval() on the sampled directions
    f = r.plugin.eval(None, torch.from_numpy(b["wi"]).to(r.device), torch.from_numpy(b["wo"]).to(r.device))
    assert torch.allclose(f.cpu(), torch.from_numpy(b["f_o"]), rtol=1e-6, atol=1e-7)
    # ground-truth and proxy renders: same lighting, same lobe -> same luminance on the ball
    rp = _renderer(material="chm_orange_rgb", plugin=plugin, env=env, albedo=(1.0, 1.0, 1.0), gt=False)
    assert not rp.use_ground_truth
    a = r.render(passes=16, spp=4, seed=2).cpu().numpy()
    p = rp.render(passes=16, spp=4, seed=2).cpu().numpy()
    hit = (r.primary(0, r.camera.height, 1, 2, 0)["nrm"].cpu().numpy() != 0).any(1).reshape(r.camera.height, -1)
    lum = lambda im: 0.2126 * im[..., 0] + 0.7152 * im[..., 1] + 0.0722 * im[..., 2]
    la, lp = lum(a)[hit], lum(p)[hit]
    assert np.corrcoef(la, lp)[0, 1] > 0.8
    # the proxy is colour-blind (weight = albedo): scale by the material's luminance albedo ~ 0.3-0.45
    ratio = la.mean() / lp.mean()
    assert 0.2 < ratio < 0.7, ratio
    assert a[hit][:, 0].mean() > 1.5 * a[hit][:, 2].mean()   # the real f renders the film orange


def _array_renderer(w=120, h=90, n_balls=5, gt=False, env=None):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    cam, centers, radii = WF.array0_scene(w, h)
    stems = ["chm_orange_rgb_disk", "aniso_miro_7_rgb_spherical", "vch_silk_blue_rgb_disk", "aniso_copper_sheet_rgb_disk",
             "aurora_white_rgb_spherical"][:n_balls]
    order = [5, 6, 9, 10, 1][:n_balls]                   # balls in the middle of the frame
    tab = MaterialTable(stems)
    gts = {}
    if gt:
        from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF
        gts = {0: MeasuredBSDF(os.path.join(ROOT, "tests", "golden", "chm_orange_rgb.bsdf"))}
    return WF.ArrayRenderer(tab, [centers[i] for i in order], [radii[i] for i in order], camera=cam, env=env,
                            ground_truth=gts)


def _array_scene_dict(r):
    d = _scene_dict(r)
    sc = r.scene
    d["spheres"] = [(list(sc.sphere_center), sc.sphere_radius)]
    d["spheres"] += [(list(sc.extra_spheres[k])[:3], sc.extra_spheres[k][3]) for k in range(sc.n_extra_spheres)]
    d["plane"] = dict(y=sc.plane_y, c0=sc.checker_color0, c1=sc.checker_color1, scale=sc.checker_scale)
    return d


@pytest.mark.parametrize("gt", [False, True])
def test_array_scene_matches_oracle(gt):
    """Several balls with one material each over a checkerboard floor: primary (with material ids) and shade
    vs the oracle; the sampler outputs inside the pass are MaterialTable.sample_pdf's."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    env = make_sky(64, 128, seed=5)
    r = _array_renderer(gt=gt, env=env)
    sc = _array_scene_dict(r)
    spp = 2
    h, w = r.camera.height, r.camera.width
    film = torch.zeros((h, w, 3), device=r.device)
    r.render_pass(film, 0, h, spp, seed=4, pass_idx=1)
    torch.cuda.synchronize()
    b = {k: v.cpu().numpy() for k, v in r._buffers(h * w * spp).items()}
    wi_o, wl_o, n_o, d_o, mat_o = WO.primary(sc, 0, h, spp, seed=4, pass_idx=1, with_material=True)
    assert (b["mat"] != mat_o).sum() <= 4                 # silhouettes / floor-ball contact: last-ulp decisions
    same = b["mat"] == mat_o
    assert np.abs(b["dir"] - d_o).max() < 1e-6 and np.abs(b["wl"] - wl_o).max() < 2e-6
    n_b = len(r.table)
    floor = same & (mat_o == n_b)
    assert (b["wi"][floor] == wi_o[floor]).all() and (b["nrm"][floor] == [0, 1, 0]).all()
    ball = same & (mat_o < n_b) & (-(d_o * n_o).sum(1) > 0.1)
    assert np.abs(b["wi"][ball] - wi_o[ball]).max() < 5e-5
    assert len(np.unique(b["mat"][b["mat"] < n_b])) == n_b  # every ball is visible
    # paths that carry no material got no sample
    nomat = b["mat"] >= n_b
    assert (b["pdf_o"][nomat] == 0).all() and (b["wo"][nomat] == 0).all()
    want = WO.shade(sc, env.numpy(), spp, b["wo"], b["pdf_o"], b["wl"], b["pdf_l"], b["nrm"], b["dir"],
                    f_o=b.get("f_o"), f_l=b.get("f_l"), wi=b["wi"], material=b["mat"])
    got = film.cpu().numpy().reshape(-1, 3)
    err = np.abs(got - want) / (np.abs(want) + 1e-3)
    assert np.isfinite(got).all() and np.percentile(err, 99.9) < 2e-4 and err.max() < 5e-3
    if gt:  # ball 0 (chm_orange) is shaded with its measured f, the others with the proxy
        rows = b["mat"] == 0
        assert rows.sum() > 50
        assert np.isfinite(b["f_o"][rows]).all() and np.isfinite(b["f_l"][rows]).all()
        assert np.abs(b["f_o"][rows] - b["pdf_o"][rows][:, None]).max() > 1e-3        # the measured f, not the proxy
        assert np.isnan(b["f_o"][b["mat"] != 0]).all() and np.isnan(b["f_l"][b["mat"] != 0]).all()


def test_array_scene_renders_and_shards():
    r = _array_renderer(w=96, h=64)
    a = r.render(passes=4, spp=2, seed=1)
    assert torch.isfinite(a).all() and float(a.mean()) > 0.05
    # the same image whatever the row split (bit for bit, in fact: test_array_scene_tiles_are_the_rows_of_the_whole_film_bit_for_bit)
    parts = torch.cat([r.render(passes=4, spp=2, seed=1, rows=(0, 30)), r.render(passes=4, spp=2, seed=1, rows=(30, 64))], 0)
    assert abs(float(parts.mean()) - float(a.mean())) < 0.05 * float(a.mean())
    # floor pixels (no BSDF sampling noise source but the light sample) are independent of the split
    b = r.primary(0, 64, 1, 1, 0)
    floor = (b["mat"] == len(r.table)).reshape(64, 96)
    close = torch.isclose(parts, a, rtol=1e-5, atol=1e-6).all(-1)
    assert float(close[floor].float().mean()) > 0.97     # all but pixels on a ball's silhouette


@pytest.mark.parametrize("gt", [False, True])
def test_array_scene_tiles_are_the_rows_of_the_whole_film_bit_for_bit(gt):
    """Every draw of a pass is keyed by the global path index — primary's Philox counter, and the sampler's through rng = "lane"
    with the tile's first path as offset — so rows (0, 1), (1, 30), (30, 64), concatenated, ARE the whole render."""
    from bsdf_diffusion_sampling_amd.wavefront import make_sky
    r = _array_renderer(w=96, h=64, gt=gt, env=make_sky(64, 128, seed=5))
    whole = r.render(passes=2, spp=2, seed=1)
    parts = torch.cat([r.render(passes=2, spp=2, seed=1, rows=rows) for rows in ((0, 1), (1, 30), (30, 64))], 0)
    assert torch.isfinite(whole).all() and float(whole.mean()) > 0.05
    assert torch.equal(parts, whole)
