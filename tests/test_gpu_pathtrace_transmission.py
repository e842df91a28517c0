"""GPU tests of transmitted paths through the balls of the array scene: ``bsdfd_wf_sample_inside`` / ``_rows``
(csrc/analytic_table.hip) and ``bsdfd_wf_bounce_transmit`` (csrc/bounce.hip) row by row on one synthetic 4096-row wavefront
(tests/bounce_transmit_ref.py), and ``PathArrayRenderer(..., transmission=True)`` as whole recorded passes, in the mean against an
independent estimator (a glass ball in a furnace), on an opaque scene, and switched off."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_ref as B  # noqa: E402
import bounce_transmit_ref as T  # noqa: E402
import dielectric_ref as DR  # noqa: E402
import envmap_ref as ER  # noqa: E402
import pass_replay as PR  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from oracle import wavefront_oracle as WO  # noqa: E402
from test_gpu_envmap import _dist  # noqa: E402
from test_gpu_pathtrace import _gpu, _scene_renderer, _shade_bound, _to_device  # noqa: E402
from test_gpu_pathtrace_lights import _device_lights  # noqa: E402
from test_pathtrace_cpu import STATE  # noqa: E402

SEED, PASS, OFFSET = 0x1234567890ABCDEF, 3, (1 << 32) - 2000      # (the path index crosses 2^32 inside the wavefront)
SCENE = R.SYNTH_SCENE
N_B = len(SCENE["spheres"])
OUT = ("org", "nrm", "wi", "wl", "mat", "beta", "rad")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.tobytes()


# ---- 1. sample_inside row by row ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inside_case():
    """The synthetic wavefront on the device, the table [bsdf 23 (a rough dielectric), a Principled with spec_trans = 1, None], and
    what the full-width call left in outputs pre-filled with 7.25 (shared: nobody writes them)."""
    _gpu()
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, Principled, reference_bsdf
    v, cls = T.synthetic_vertices()
    table = AnalyticTable([reference_bsdf(23), Principled(roughness=0.4, spec_trans=1.0, eta=1.5), None])
    n = len(v["material"])
    d = {k: _dev(v[k]) for k in ("material", "wi", "wl")}
    out = (torch.full((n, 3), 7.25, device="cuda"), torch.full((n,), 7.25, device="cuda"), torch.full((n,), 7.25, device="cuda"))
    bounce = 2
    table.sample_inside(d["material"], d["wi"], d["wl"], bounce, SEED, PASS, OFFSET, out=out)
    torch.cuda.synchronize()
    return dict(v=v, cls=cls, table=table, d=d, n=n, bounce=bounce, full=tuple(t.cpu().numpy() for t in out))


def test_sample_inside_is_the_tables_own_sampler_on_the_inside_rows_and_nothing_elsewhere():
    c = _inside_case()
    v, table, d, n = c["v"], c["table"], c["d"], c["n"]
    wo, pdf_o, pdf_l = c["full"]
    inside = (v["material"] >= 0) & (v["material"] < 3) & (v["wi"][:, 2] < 0)
    assert np.array_equal(inside, c["cls"]["inside"]) and all(((v["material"] == m) & inside).sum() >= 200 for m in range(3))
    # every other row — floor, ended (NaN state), outside — keeps every byte
    for a in (wo, pdf_o, pdf_l):
        assert (a[~inside] == np.float32(7.25)).all()
    u = T.inside_variates(SEED, PASS, c["bounce"], OFFSET, n)
    want_wo, want_pdf, want_w = table.sample_t(d["material"], d["wi"], _dev(u))
    want_l = table.pdf_t(d["material"], d["wi"], d["wl"])
    torch.cuda.synchronize()
    want_wo, want_pdf, want_l, want_w = want_wo.cpu().numpy(), want_pdf.cpu().numpy(), want_l.cpu().numpy(), want_w.cpu().numpy()
    gt = inside & (v["material"] < 2)
    # a sample the model weights with 0 (the dielectric's wo on the wrong side for its lobe) is handed on as unusable: the bounce
    # forms f(wi, wo) / pdf_o of the pair itself, which is not 0 there (the furnace test below is what saw it)
    failed = gt & (want_pdf > 0) & ~(want_w.max(1) > 0)
    print(f"{int(failed.sum())} samples with a density and no weight get pdf_o = 0")
    assert failed.sum() >= 5
    want_pdf = np.where(want_w.max(1) > 0, want_pdf, np.float32(0))
    for name, got, want in (("wo", wo, want_wo), ("pdf_o", pdf_o, want_pdf), ("pdf_l", pdf_l, want_l)):
        assert _bits(got[gt]) == _bits(want[gt]), name
    none = inside & (v["material"] == 2)                                              # a record without ground truth: zeros
    assert (wo[none] == 0).all() and (pdf_o[none] == 0).all() and (pdf_l[none] == 0).all()
    # (not vacuous) the samplers answer on both sides of the surface, with usable densities
    ok = gt & (pdf_o > 0)
    print(f"{int(inside.sum())} inside rows, {int(ok.sum())} with a usable sample: {int((wo[ok, 2] > 0).sum())} leave the ball, "
          f"{int((wo[ok, 2] < 0).sum())} stay inside; pdf_l > 0 on {int((pdf_l[gt] > 0).sum())}")
    assert ok.sum() >= 0.5 * gt.sum() and (wo[ok, 2] > 0).sum() >= 100 and (wo[ok, 2] < 0).sum() >= 100 and (pdf_l[gt] > 0).sum() >= 100
    assert np.isfinite(wo[gt]).all() and np.isfinite(pdf_o[gt]).all() and np.isfinite(pdf_l[gt]).all()


def test_sample_inside_rows_serves_the_listed_rows_only():
    c = _inside_case()
    table, d, n = c["table"], c["d"], c["n"]
    rows = np.random.default_rng(5).permutation(n)[:1000].astype(np.int64)
    out = (torch.full((n, 3), -3.5, device="cuda"), torch.full((n,), -3.5, device="cuda"), torch.full((n,), -3.5, device="cuda"))
    table.sample_inside(d["material"], d["wi"], d["wl"], c["bounce"], SEED, PASS, OFFSET, out=out, rows=_dev(rows))
    torch.cuda.synchronize()
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    written = listed & c["cls"]["inside"]
    assert written.sum() >= 150
    for got, full in zip(out, c["full"]):
        got = got.cpu().numpy()
        assert _bits(got[written]) == _bits(full[written])
        assert (got[~written] == np.float32(-3.5)).all()
    before = tuple(t.clone() for t in out)
    table.sample_inside(d["material"], d["wi"], d["wl"], c["bounce"], SEED, PASS, OFFSET, out=out,
                        rows=torch.empty(0, dtype=torch.int64, device="cuda"))           # an empty list: a no-op
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, before))


def test_sample_inside_errors():
    from bsdf_diffusion_sampling_amd import _lib
    c = _inside_case()
    table, d, n = c["table"], c["d"], c["n"]
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    out = (torch.zeros((n, 3), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"))
    arrays = [p(d["material"]), p(d["wi"]), p(d["wl"]), p(out[0]), p(out[1]), p(out[2])]
    assert L.bsdfd_wf_sample_inside(None, 0, 0, 0, 0, n, *arrays, None) == 1 and b"null analytic table" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_inside(table._t, -1, 0, 0, 0, n, *arrays, None) == 1 and b"bounce must be >= 0" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_inside(table._t, 0, 0, 0, 0, -1, *arrays, None) == 1 and b"N must be >= 0" in L.bsdfd_last_error()
    for missing in range(6):
        bad = list(arrays)
        bad[missing] = None
        assert L.bsdfd_wf_sample_inside(table._t, 0, 0, 0, 0, n, *bad, None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_inside_rows(table._t, 0, 0, 0, 0, n, *arrays, None, 5, None) == 1 and b"null pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_inside_rows(table._t, 0, 0, 0, 0, n, *arrays, p(d["material"]), n + 1, None) == 1
    assert b"n_rows must be in [0, N]" in L.bsdfd_last_error()
    assert L.bsdfd_wf_sample_inside(table._t, 0, 0, 0, 0, 0, *([None] * 6), None) == 0                  # N = 0: a no-op
    assert L.bsdfd_wf_sample_inside_rows(table._t, 0, 0, 0, 0, n, *arrays, None, 0, None) == 0          # n_rows = 0 too
    with pytest.raises(ValueError, match="rows must be a contiguous int64"):
        table.sample_inside(d["material"], d["wi"], d["wl"], 0, 0, 0, 0, out=out, rows=torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="triple"):
        table.sample_inside(d["material"], d["wi"], d["wl"], 0, 0, 0, 0, out=None)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0 for t in out)                                                   # nothing ran


# ---- 2. bounce_transmit row by row --------------------------------------------------------------------------------------------------
MODES = ("cosine", "lit", "env")


@functools.lru_cache(maxsize=None)
def _inputs(mode):
    """The synthetic wavefront of ``mode``: the state and the sampler's answers [+ lsel, emit | lpdf, emit from the references of
    the emitter stages], fp32 / int, shared by the tests (nobody writes them)."""
    v = dict(T.synthetic_vertices()[0])
    env = R.synthetic_env()
    vertex = [v[k] for k in ("org", "nrm", "wi", "material")]
    if mode == "lit":
        s = LR.sample_emitter(SCENE, LR.synthetic_lights(), True, 1, True, SEED, PASS, OFFSET, *vertex, v["wl"])
        v.update(wl=s["wl"].astype(np.float32), lsel=s["lsel"], emit=s["emit"].astype(np.float32))
    if mode == "env":
        s = ER.sample_env(SCENE, env, ER.build_tables(env), 1, 1, True, SEED, PASS, OFFSET, *vertex, None, v["wl"])
        picked = s["picked"]
        v.update(wl=np.where(picked[:, None], s["wl"], v["wl"]).astype(np.float32), lpdf=np.where(picked, s["lpdf"], 0.0).astype(np.float32),
                 emit=np.where(picked[:, None], s["emit"], 0.0).astype(np.float32))
    return v


@functools.lru_cache(maxsize=None)
def _env_dist():
    return _dist(R.synthetic_env())


@functools.lru_cache(maxsize=None)
def _tables():
    return ER.build_tables(R.synthetic_env())


@pytest.fixture(scope="module")
def renderer():
    return _scene_renderer(SCENE, R.synthetic_env())


def _call(r, v, mode, bounce, last, rr_depth, transmission):
    b = _to_device(r, v)
    r.transmission = transmission           # (the renderer is only a handle on the scene here: the kernels are called directly)
    try:
        r.bounce(b, bounce, bool(last), SEED, PASS, OFFSET, occlusion=True, lights=_device_lights(LR.synthetic_lights(), 1) if mode == "lit" else None,
                 env_dist=_env_dist() if mode == "env" else None, rr_depth=rr_depth)
    finally:
        r.transmission = False
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy() for k in OUT}


def _near_cell(v):
    """tests/test_gpu_pass_replay.py::_near_cell: live rows whose environment-density lookup lies within 1e-3 cells of a cell
    boundary, where the fp32 kernel may read the neighbouring cell's density."""
    mat = v["material"]
    live = (mat >= 0) & (mat <= N_B)
    fs, ft, nn = LR._frames(v["nrm"].astype(np.float64), live, np.float64)
    local = np.where((mat == N_B)[:, None], v["wl"], v["wo"]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        edge = ER.cell_of(_tables()["pdf_uv"].shape, local[:, 0:1] * fs + local[:, 1:2] * ft + local[:, 2:3] * nn)[3]
    return live & ~(edge >= 1e-3)


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_bounce_transmit_matches_reference(renderer, mode, active, last):
    """4096 synthetic vertices (wo below the surface with ground truth, without it, with f_o == 0; inside vertices with wo on either
    side) through ONE bsdfd_wf_bounce_transmit call, row by row against the fp64 reference with the decision cap, the error bounds
    and the shade bound of test_bounce_kernel_matches_reference; the rows that enter or stay inside on their own terms; the rows the
    rule does not trigger on against bsdfd_wf_bounce_rr."""
    bounce = 2
    rr_depth = 1 if active else None
    v = _inputs(mode)
    n = len(v["material"])
    kw = dict(n_e=4 if mode == "lit" else 1, lsel=v.get("lsel"), emit=v.get("emit"), lpdf=v.get("lpdf"),
              tables=_tables() if mode == "env" else None)
    want = T.bounce(SCENE, R.synthetic_env(), mode, bounce, bool(last), True, SEED, PASS, OFFSET, *[v[k] for k in STATE], rr_depth=rr_depth, **kw)
    got = _call(renderer, v, mode, bounce, last, rr_depth, True)
    rr = _call(renderer, v, mode, bounce, last, rr_depth if active else bounce + 2, False)     # bsdfd_wf_bounce_rr, inactive or active
    live = (v["material"] >= 0) & (v["material"] <= N_B)
    vv = dict(v, mat=v["material"])
    for k in OUT:                                                                     # ended paths: not a byte of their state moves
        assert _bits(got[k][~live]) == _bits(vv[k][~live]), k
    differ = got["mat"] != want["material"]
    enter = want["enter"]
    print(f"{mode} active={active} last={last}: {int(differ.sum())} of {n} rows decide differently; {int(enter.sum())} trigger the rule")
    assert differ.sum() <= n // 1000
    same = live & ~differ
    cont = same & (want["material"] <= N_B)
    inside = cont & enter
    if last:
        assert not cont.any() and (got["mat"][live] == N_B + 1).all()
    else:
        assert cont.sum() > 500 and inside.sum() >= 300
        graze = cont & (want["cos_in"] < 0.1)
        ok = cont & ~graze
        for k in ("org", "nrm", "wi", "beta"):
            e_ok, e_all = np.abs(got[k][ok] - want[k][ok]).max(), np.abs(got[k][cont] - want[k][cont]).max()
            print(f"  {k}: max error {e_ok:.2e} ({e_all:.2e} with the {int(graze.sum())} grazing hits)")
            assert e_ok < 2e-5 and e_all < 2e-3, k
        assert np.abs(got["wl"][cont] - R.next_wl(SEED, PASS, bounce, OFFSET, n)[cont]).max() < 2e-6
        # the rows that enter or stay inside: on the sphere of their own ball, wi.z < 0, the id unchanged, beta = beta_in f_o / pdf_o
        cs = np.asarray([c for c, _ in SCENE["spheres"]], np.float32).astype(np.float64)[v["material"][inside]]
        rs = np.asarray([r for _, r in SCENE["spheres"]], np.float32).astype(np.float64)[v["material"][inside]]
        off = np.abs(np.linalg.norm(got["org"][inside].astype(np.float64) - cs, axis=1) - rs) / rs
        scale = 1.0 / want["q"][inside, None] if active else 1.0
        beta = v["beta"][inside].astype(np.float64) * v["f_o"][inside].astype(np.float64) / v["pdf_o"][inside, None].astype(np.float64) * scale
        e_beta = np.abs(got["beta"][inside] - beta).max()
        print(f"  {int(inside.sum())} rows enter or stay inside: | |org - c| - r | / r max {off.max():.1e}, beta error {e_beta:.1e}; of them "
              f"{int((v['wi'][inside, 2] < 0).sum())} were inside already")
        assert off.max() < 2e-5 and (got["wi"][inside, 2] < 0).all() and np.array_equal(got["mat"][inside], v["material"][inside])
        assert e_beta < 2e-5 and (v["wi"][inside, 2] < 0).sum() >= 100 and (v["wi"][inside, 2] > 0).sum() >= 100
        assert (cont & ~enter & (v["wi"][:, 2] < 0) & (v["material"] < N_B)).sum() >= 30     # inside vertices that leave and hit something
    # wo below the surface without ground truth, or with f_o == 0: the path ends as before
    cls = T.synthetic_vertices()[1]
    assert (got["mat"][cls["without_gt"] | cls["opaque"]] == N_B + 1).all()
    ended = same & ~cont                                                              # rows that end keep the rest of their state
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert _bits(got[k][ended]) == _bits(vv[k][ended]), k
    rows = same & ~_near_cell(v) if mode == "env" else same
    assert rows.sum() >= 0.98 * same.sum()
    p999, worst = _shade_bound(got["rad"][rows], want["rad"][rows])
    print(f"  rad: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3
    # where the rule is not triggered the call agrees with bsdfd_wf_bounce_rr on the same inputs, within the same bounds
    rest = live & ~enter
    d_rr = rest & (got["mat"] != rr["mat"])
    assert d_rr.sum() <= n // 1000
    both = rest & ~d_rr
    moved = both & (got["mat"] <= N_B)
    for k in ("org", "nrm", "wi", "wl", "beta"):
        assert np.abs(got[k][moved] - rr[k][moved]).max(initial=0.0) < 2e-5, k
        assert _bits(got[k][both & ~moved]) == _bits(rr[k][both & ~moved]), k
    p999, worst = _shade_bound(got["rad"][live & ~d_rr], rr["rad"][live & ~d_rr].astype(np.float64))   # rad: the entering rows too
    assert p999 < 2e-4 and worst < 5e-3
    assert (rr["mat"][enter] == N_B + 1).all()                                        # ... and there the plain bounce drops the sample


def test_bounce_transmit_list_form_and_errors(renderer):
    """The list form on a shuffled 1000-row list: the full-width call's bits on the listed rows, nothing elsewhere; an empty list
    is a no-op; f_o is required."""
    from bsdf_diffusion_sampling_amd import _lib
    r = renderer
    v = _inputs("cosine")
    n = len(v["material"])
    full = _call(r, v, "cosine", 2, 0, 1, True)
    rows = np.random.default_rng(6).permutation(n)[:1000].astype(np.int64)
    b = _to_device(r, v)
    r.transmission = True
    r.bounce(b, 2, False, SEED, PASS, OFFSET, occlusion=True, rr_depth=1, rows=_dev(rows))
    torch.cuda.synchronize()
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    vv = dict(v, mat=v["material"])
    for k in OUT:
        got = b[k].cpu().numpy()
        assert _bits(got[listed]) == _bits(full[k][listed]), k
        assert _bits(got[~listed]) == _bits(vv[k][~listed]), k
    before = {k: t.clone() for k, t in b.items()}
    try:
        r.bounce(b, 2, False, SEED, PASS, OFFSET, occlusion=True, rr_depth=1, rows=torch.empty(0, dtype=torch.int64, device=r.device))
        no_f = {k: t for k, t in b.items() if k not in ("f_o", "f_l")}
        with pytest.raises(RuntimeError, match="transmission needs the ground truth"):
            r.bounce(no_f, 2, False, SEED, PASS, OFFSET, occlusion=True)
    finally:
        r.transmission = False
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    state = [p(b["mat" if k == "material" else k]) for k in STATE]
    assert L.bsdfd_wf_bounce_transmit(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, None, None, None, None, None, -1, None, 0,
                                      None) == 1 and b"rr_depth must be >= 0" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_transmit(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, n, *state, None, None, None, None, None, 0, None, 5,
                                      None) == 1 and b"null rows pointer" in L.bsdfd_last_error()
    assert L.bsdfd_wf_bounce_transmit(C.byref(r.scene), p(r.env), 0, 0, 1, 0, 0, 0, 0, *([None] * 12), None, None, None, None, None, 0,
                                      None, 0, None) == 0                              # N = 0: a no-op
    torch.cuda.synchronize()
    for k, t in b.items():
        assert torch.equal(t.view(torch.uint8), before[k].view(torch.uint8)), k


# ---- 3. whole passes ----------------------------------------------------------------------------------------------------------------
W, H, SPP, PASS_SEED, FILL = 64, 64, 2, 4, 0.25
NAMES = ["bsdf_24_spherical", "bsdf_13_spherical", "bsdf_1_spherical", "bsdf_20_spherical"]      # glass, two principled, one without


@functools.lru_cache(maxsize=None)
def _glass_scene():
    _gpu()
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    _, centers, radii = WF.array0_scene(W, H)
    order = [5, 6, 9, 10]
    cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=W, height=H)
    return dict(table=MaterialTable(NAMES), centers=[centers[i] for i in order], radii=[radii[i] for i in order], camera=cam,
                env=WF.make_sky(64, 128, seed=5), ground_truth=ground_truth_for(NAMES[:3]))


def _glass_renderer(**kw):
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    s = _glass_scene()
    return PathArrayRenderer(s["table"], s["centers"], s["radii"], camera=s["camera"], env=s["env"], ground_truth=s["ground_truth"], **kw)


PASSES = {"depth6": dict(max_depth=6), "unbounded": dict(max_depth=None, rr_depth=5)}


@functools.lru_cache(maxsize=None)
def _recorded(case):
    r = _glass_renderer(transmission=True, **PASSES[case])
    film = torch.full((H, W, 3), FILL, dtype=torch.float32, device=r.device)
    with T.Recorder(r) as rec:
        r.render_pass(film, 0, H, SPP, PASS_SEED, 0)
    torch.cuda.synchronize()
    k = 0
    for s in rec.stages:
        s["k"] = k
        k += s["name"] == "bounce"
    state = {name: r._buffers(H * W * SPP)[name].cpu().numpy() for name in OUT}
    return dict(r=r, stages=rec.stages, stats={k: (list(v) if isinstance(v, list) else v) for k, v in r.stats.items()},
                scene=PR.scene_of(r), env=_glass_scene()["env"].numpy(), n_b=len(r.table), n=H * W * SPP, film=film.cpu().numpy(),
                state=state)


@pytest.mark.parametrize("case", list(PASSES))
def test_recorded_pass_with_transmission_matches_the_replay(case):
    """One recorded pass of the 4-ball scene (a glass ball, two principled ones with spec_trans 0.9, one without ground truth),
    64x64, 2 spp: the stages come in the documented order — sample_inside behind sample_pdf at every bounce k >= 1 —, the inside
    sampler's rows are the table's own sampler bit for bit at the documented variates, the evaluator answers for the overwritten wo,
    every bounce is held to the transmitting reference on the device's own input with the bounds of
    tests/test_gpu_pass_replay.py::_check_bounce, and the whole pass to the free-running fp64 replay with the recorded answers."""
    rec = _recorded(case)
    r, n_b, n, scene = rec["r"], rec["n_b"], rec["n"], rec["scene"]
    max_depth, rr_depth = PASSES[case]["max_depth"], PASSES[case].get("rr_depth")
    named = lambda name: [s for s in rec["stages"] if s["name"] == name]
    bounces, buckets = named("bounce"), named("bucket")
    depth = len(bounces)
    cap = r.DEPTH_CAP if max_depth is None else max_depth
    lanes = rec["stats"]["lanes_per_bounce"]
    want = ["primary", "path_begin"]
    for k in range(depth):
        want += ["bucket"] + (["sample_pdf"] + ["sample_inside"] * (k >= 1) + ["eval_t"]) * (lanes[k] > 0) + ["bounce"]
    if depth < cap:
        want += ["bucket"]
    got = [s["name"] for s in rec["stages"]]
    print(f"{case}: {depth} bounces, material lanes {lanes}")
    assert got == want + ["resolve"]
    assert rec["stats"]["depth"] == depth and rec["stats"]["depth_cap_hit"] is False and 4 <= depth <= cap
    for s in bounces:
        assert s["args"] == dict(bounce=s["k"], last=s["k"] == cap - 1, seed=PASS_SEED, pass_idx=0, path_offset=0, occlusion=True)
    for s, t in zip(rec["stages"], rec["stages"][1:]):                                # nothing writes the state between two stages
        for key, a in s["after"].items():
            assert _bits(a) == _bits(t["before"][key]), (s["name"], t["name"], key)
    # the inside sampler
    table = r.measured_table
    served = 0
    for s in named("sample_inside"):
        v, out = s["before"], s["after"]
        assert s["args"] == dict(bounce=s["k"], seed=PASS_SEED, pass_idx=0, path_offset=0) and s["k"] >= 1
        inside = (v["mat"] >= 0) & (v["mat"] < n_b) & (v["wi"][:, 2] < 0)
        for key in out:
            rows = ~inside if key in ("wo", "pdf_o", "pdf_l") else slice(None)
            assert _bits(out[key][rows]) == _bits(v[key][rows]), key
        if not inside.any():
            continue
        u = T.inside_variates(PASS_SEED, 0, s["k"], 0, n)
        wo, pdf, weight = table.sample_t(_dev(v["mat"]), _dev(v["wi"]), _dev(u))
        pdf = torch.where(weight.max(1).values > 0, pdf, torch.zeros_like(pdf))      # (a failed sample is handed on as unusable)
        pl = table.pdf_t(_dev(v["mat"]), _dev(v["wi"]), _dev(v["wl"]))
        gt = inside & (v["mat"] < 3)
        assert not (inside & ~gt).any()                                               # (no path gets into the ball without ground truth)
        for key, t in (("wo", wo), ("pdf_o", pdf), ("pdf_l", pl)):
            assert _bits(out[key][gt]) == _bits(t.cpu().numpy()[gt]), (s["k"], key)
        served += int(gt.sum())
        ev = [e for e in named("eval_t") if e["k"] == s["k"]][0]                      # f_o is formed from the overwritten wo
        f_o, f_l = table.eval_t(_dev(out["mat"]), _dev(out["wi"]), _dev(out["wo"]), _dev(out["wl"]))
        assert _bits(ev["after"]["f_o"][gt]) == _bits(f_o.cpu().numpy()[gt]) and _bits(ev["after"]["f_l"][gt]) == _bits(f_l.cpu().numpy()[gt])
    print(f"  {served} inside vertices served by the models' own samplers")
    assert served >= 100
    # every bounce against the transmitting reference on the device's own input
    names = ("org", "nrm", "wi", "wl", "mat", "beta", "rad", "wo", "pdf_o", "pdf_l", "f_o", "f_l")
    entered = stayed = 0
    for s in bounces:
        v, out = s["before"], s["after"]
        ref = T.bounce(scene, rec["env"], "cosine", s["k"], s["args"]["last"], True, PASS_SEED, 0, 0, *[v[k] for k in names], rr_depth=rr_depth)
        live = (v["mat"] >= 0) & (v["mat"] <= n_b)
        for k in OUT:
            assert _bits(out[k][~live]) == _bits(v[k][~live]), k
        differ = live & (PR.decision_code(scene, out["mat"], out["wi"]) != PR.decision_code(scene, ref["material"], ref["wi"]))
        assert differ.sum() <= live.sum() // 1000, (s["k"], int(differ.sum()), int(live.sum()))
        same = live & ~differ
        cont = same & (ref["material"] <= n_b)
        inside = cont & ref["enter"]
        entered += int((inside & (v["wi"][:, 2] > 0)).sum())
        stayed += int((inside & (v["wi"][:, 2] < 0)).sum())
        if cont.any():
            t = np.linalg.norm(ref["org"] - v["org"].astype(np.float64), axis=1)
            far = cont & (ref["material"] == n_b) & (t > 50.0)
            graze = cont & (ref["cos_in"] < 0.1)
            ok = cont & ~graze
            for k in ("org", "nrm", "wi", "beta"):
                err = np.abs(out[k] - ref[k]).max(1)
                rows = cont & ~far if k == "org" else cont
                assert err[ok & rows].max(initial=0.0) < 2e-5 and err[rows].max(initial=0.0) < 2e-3, (s["k"], k)
            if far.any():
                err = np.abs(out["org"] - ref["org"]).max(1)[far]
                assert (err <= 2e-5 + 2.0 ** -22 * t[far] / ref["cos_in"][far]).all()
            assert np.abs(out["wl"][cont] - R.next_wl(PASS_SEED, 0, s["k"], 0, n)[cont]).max() < 2e-6
            assert (out["wi"][inside, 2] < 0).all() and np.array_equal(out["mat"][inside], v["mat"][inside])
        ended = same & ~cont
        for k in ("org", "nrm", "wi", "wl", "beta"):
            assert _bits(out[k][ended]) == _bits(v[k][ended]), k
        if same.any():
            p999, worst = _shade_bound(out["rad"][same], ref["rad"][same])
            assert np.isfinite(out["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3, (s["k"], p999, worst)
    print(f"  {entered} paths enter a ball, {stayed} times a path stays inside")
    assert entered >= 100 and stayed >= 50
    # end to end
    answers = [{k: s["before"][k] for k in ("wo", "pdf_o", "pdf_l", "f_o", "f_l")} for s in bounces]
    ref = T.reference_pass(scene, rec["env"], "cosine", None, None, 0, H, SPP, PASS_SEED, 0, max_depth, True, answers, rr_depth=rr_depth)
    codes = lambda snap: PR.decision_code(scene, snap["mat"], snap["wi"])
    history = [codes(named("primary")[0]["after"])] + [codes(s["after"]) for s in bounces]
    differ = PR.histories_differ(history, ref["history"])
    assert differ.sum() <= n // 1000
    agree = ~differ
    final = named("resolve")[0]
    rad = final["before"]["rad"]
    p999, worst = _shade_bound(rad[agree], ref["rad"][agree])
    print(f"  histories differ on {int(differ.sum())} of {n} paths; rad p99.9 {p999:.1e} max {worst:.1e}")
    assert np.isfinite(rad).all() and p999 < 2e-4 and worst < 5e-3
    want_film = FILL + R.resolve(rad, SPP)
    assert (final["film_before"] == FILL).all()
    assert np.abs(final["film_after"].astype(np.float64).reshape(-1, 3) - want_film).max() < 1e-5 * max(1.0, want_film.max())


@pytest.mark.parametrize("case", list(PASSES))
def test_compact_keeps_its_property_with_transmission(case):
    """compact=True: the same film, the same final path state and the same statistics, bit for bit; and the glass scene serves
    strictly more material lanes at every bounce >= 2 than the renderer without transmission does."""
    rec = _recorded(case)
    comp = _glass_renderer(transmission=True, compact=True, **PASSES[case])
    film = torch.full((H, W, 3), FILL, dtype=torch.float32, device=comp.device)
    comp.render_pass(film, 0, H, SPP, PASS_SEED, 0)
    torch.cuda.synchronize()
    assert _bits(film.cpu().numpy()) == _bits(rec["film"])
    b = comp._buffers(rec["n"])
    for k in OUT:
        assert _bits(b[k].cpu().numpy()) == _bits(rec["state"][k]), k
    for k in ("lanes_per_bounce", "depth", "depth_cap_hit"):
        assert comp.stats[k] == rec["stats"][k], k
    lists = comp.stats["list_per_bounce"]
    assert lists[0] == rec["n"] and all(x < rec["n"] for x in lists[1:]) and rec["stats"]["list_per_bounce"] == [rec["n"]] * len(lists)
    off = _glass_renderer(transmission=False, **PASSES[case])
    off.render_pass(torch.zeros_like(film), 0, H, SPP, PASS_SEED, 0)
    a, o = rec["stats"]["lanes_per_bounce"], list(off.stats["lanes_per_bounce"])
    print(f"{case}: material lanes per bounce with transmission {a}, without {o}")
    assert a[:1] == o[:1] and min(len(a), len(o)) >= 4
    assert all(a[k] > o[k] for k in range(2, min(len(a), len(o), 6)))


# ---- 4. the mean is right: a glass ball in a furnace ----------------------------------------------------------------------------------
def _furnace(transmission, spp, passes, seed):
    """Per-path radiance (channel 0) of the paths whose primary ray hits the ball: one RoughDielectric(0.3) ball (its net:
    bsdf_24_spherical), no floor, a constant white environment, max_depth = 8, no roulette."""
    _gpu()
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.analytic import RoughDielectric
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    cam = WF.Camera(origin=(0.0, 0.5, 2.0), target=(0.0, 0.5, 0.0), fov_deg=30.0, width=64, height=64)
    r = PathArrayRenderer(MaterialTable(["bsdf_24_spherical"]), [(0.0, 0.5, 0.0)], [0.45], camera=cam, env=torch.ones((8, 16, 3)),
                          floor=False, ground_truth={0: RoughDielectric(0.3)}, max_depth=8, transmission=transmission)
    film = torch.zeros((64, 64, 3), device=r.device)
    n = 64 * 64 * spp
    vals = []
    for p in range(passes):
        r.render_pass(film, 0, 64, spp, seed, p)
        rad = r._buffers(n)["rad"][:, 0].clone()
        hit = r.primary(0, 64, spp, seed, p)["mat"] == 0
        vals.append(rad[hit].double().cpu().numpy())
    torch.cuda.synchronize()
    return np.concatenate(vals), PR.scene_dict(cam, [(0.0, 0.5, 0.0)], [0.45], floor=False), list(r.stats["lanes_per_bounce"])


def _numpy_furnace(scene, n_paths, seed, vertices=8):
    """The same truncated path integral by an independent fp64 estimator: BSDF sampling only, with ``dielectric_ref``'s own sampler
    at every vertex.  A sample that leaves the ball sees the white environment (weight x 1) and ends the path; one that goes inside
    continues at the far side of the ball, where — a chord meets the sphere at equal angles, and the model is isotropic — the
    incident direction is (sqrt(1 - z^2), 0, z) with z = wo.z < 0; at most ``vertices`` vertices."""
    model = DR.RoughDielectric(0.3)
    g = np.random.default_rng(seed)
    spp = 4
    wi0 = []
    p = 0
    while sum(len(a) for a in wi0) < n_paths:
        wi, _, _, _, mat = WO.primary(scene, 0, scene["height"], spp, seed, p, with_material=True)
        wi0.append(wi[mat == 0].astype(np.float64))
        p += 1
    wi = np.concatenate(wi0)[:n_paths]
    total = np.zeros(len(wi))
    rows, beta = np.arange(len(wi)), np.ones(len(wi))          # the paths still alive, and their throughput
    for _ in range(vertices):
        wo, pdf, w = model.sample(wi, g.random((len(wi), 3)))
        w = w[:, 0]
        out = (w > 0) & (wo[:, 2] > 0)
        total[rows[out]] += beta[out] * w[out]
        on = (w > 0) & (wo[:, 2] < 0)
        rows, beta, z = rows[on], beta[on] * w[on], wo[on, 2]
        wi = np.stack([np.sqrt(np.maximum(1 - z * z, 0.0)), np.zeros_like(z), z], 1)
    return total


def test_glass_furnace_mean_matches_an_independent_estimator():
    """Mean radiance over the ball's paths, GPU (MIS of the net's BSDF sample and a cosine light sample at the first vertex, the
    model's own sampler inside) against the numpy estimator: the two truncate at the same depth and share their expectation, so they
    differ by at most 4 sqrt(se_a^2 + se_b^2) — the rule of the roulette test.  Without transmission the same scene lies more than
    ten of those tolerances below (the test cannot pass on noise), and the transmitting mean does not exceed 1 by more than the
    tolerance (energy conservation)."""
    a, scene, lanes = _furnace(True, spp=8, passes=4, seed=31)
    off, _, lanes_off = _furnace(False, spp=8, passes=1, seed=31)
    b = _numpy_furnace(scene, 150_000, seed=32)
    se = lambda x: x.std(ddof=1) / np.sqrt(len(x))
    tol = 4.0 * np.sqrt(se(a) ** 2 + se(b) ** 2)
    print(f"glass furnace: GPU mean {a.mean():.5f} +- {se(a):.5f} over {len(a)} paths, numpy mean {b.mean():.5f} +- {se(b):.5f} over {len(b)}, "
          f"difference {a.mean() - b.mean():+.5f}, tolerance {tol:.5f}; without transmission {off.mean():.5f}: "
          f"{(a.mean() - off.mean()) / tol:.1f} tolerances below; material lanes per bounce {lanes} (without: {lanes_off})")
    assert len(a) >= 50_000 and np.isfinite(a).all()
    assert abs(a.mean() - b.mean()) <= tol
    assert a.mean() - off.mean() > 10 * tol
    assert a.mean() <= 1.0 + tol


# ---- 5. an opaque scene does not change ---------------------------------------------------------------------------------------------
def test_an_opaque_scene_does_not_change():
    """Analytic ground truth whose materials all have spec_trans = 0: no sample below the surface carries throughput, so nothing
    goes inside — the lanes per bounce are those of transmission=False and the film lies within the shade bound of it (the two run
    different instantiations of the bounce)."""
    from bsdf_diffusion_sampling_amd.analytic import Principled
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    s = _glass_scene()
    gt = {i: Principled(base_color=(0.8, 0.7, 0.6), roughness=0.3 + 0.1 * i, metallic=0.2 * i, spec_trans=0.0, clearcoat=0.5) for i in range(4)}
    films, lanes = [], []
    for transmission in (False, True):
        r = PathArrayRenderer(s["table"], s["centers"], s["radii"], camera=s["camera"], env=s["env"], ground_truth=gt, max_depth=5,
                              transmission=transmission)
        films.append(r.render(2, spp=SPP, seed=PASS_SEED).cpu().numpy().reshape(-1, 3))
        lanes.append(list(r.stats["lanes_per_bounce"]))
    p999, worst = _shade_bound(films[1], films[0].astype(np.float64))
    print(f"opaque scene: lanes {lanes[0]}; film p99.9 {p999:.1e} max {worst:.1e}; bit-identical: {np.array_equal(films[0], films[1])}")
    assert lanes[0] == lanes[1] and len(lanes[0]) == 5 and lanes[0][-1] > 0
    assert np.isfinite(films[1]).all() and p999 < 2e-4 and worst < 5e-3


# ---- 6. the default is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
def test_without_transmission_none_of_the_new_entry_points_is_called(monkeypatch, compact):
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    calls = {}

    def spy(name):
        inner = getattr(L, name)

        def f(*args):
            calls[name] = calls.get(name, 0) + 1
            return inner(*args)
        monkeypatch.setattr(L, name, f)
    for name in ("bsdfd_wf_bounce_transmit", "bsdfd_wf_sample_inside", "bsdfd_wf_sample_inside_rows"):
        spy(name)
    r = _glass_renderer(max_depth=4, compact=compact)
    assert r.transmission is False
    img = r.render(1, spp=SPP, seed=PASS_SEED)
    assert calls == {} and float(img.mean()) > 0
    on = _glass_renderer(max_depth=4, compact=compact, transmission=True)
    on.render(1, spp=SPP, seed=PASS_SEED)
    depth = on.stats["depth"]
    assert calls["bsdfd_wf_bounce_transmit"] == depth == 4                           # ... and with it every bounce is one
    assert calls.get("bsdfd_wf_sample_inside_rows" if compact else "bsdfd_wf_sample_inside", 0) == depth - 1
    assert ("bsdfd_wf_sample_inside" if compact else "bsdfd_wf_sample_inside_rows") not in calls
