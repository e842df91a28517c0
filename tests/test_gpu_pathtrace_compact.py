"""GPU tests of the live-lane list of the array-scene path tracer: the list forms of the per-depth kernels
(``bsdfd_wf_bounce_rows``, ``bsdfd_wf_sample_emitter_rows``, ``bsdfd_wf_sample_env_rows``, ``bsdfd_measured_eval_table_rows``,
``bsdfd_analytic_eval_table_rows``) against their full-width siblings, bit for bit on the listed rows and with every byte of the
unlisted rows in place, and ``PathArrayRenderer(..., compact=True)`` against ``compact=False`` as whole passes: the same film, the
same path state, the same statistics, and no full-width launch behind bounce 0.

The kernel tests run on the synthetic wavefronts of tests/test_gpu_pathtrace_rr.py (``_inputs``: 4096 rows, and 4096 + 37) with a
seeded shuffle of 1000 of the rows as the list: no multiple of the block, and unsorted."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import pathtrace_lights_ref as LR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
from test_gpu_pathtrace import ROOT, STEMS, _gpu, _scene_renderer, _to_device  # noqa: E402
from test_gpu_pathtrace_lights import _device_lights  # noqa: E402
from test_gpu_pathtrace_rr import FILL, H, OFFSET, PASS, PASS_SEED, SEED, SPP, W, _env_dist, _inputs, _sky  # noqa: E402
from test_pass_replay_cpu import ORDER, five_ball_lights  # noqa: E402
from test_pathtrace_compact_cpu import NEW  # noqa: E402

SCENE = R.SYNTH_SCENE
N_B = len(SCENE["spheres"])
LISTED = 1000
STATE7 = ("org", "nrm", "wi", "wl", "mat", "beta", "rad")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _list(n, count=LISTED, seed=17):
    """A seeded shuffle of ``count`` of the rows 0..n-1 -> (int64 device tensor, boolean mask of the listed rows)."""
    rows = np.random.default_rng(seed + n).permutation(n)[:count].astype(np.int64)
    assert count == 0 or (np.diff(rows) < 0).any()                                  # unsorted
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    return torch.from_numpy(rows).cuda(), listed


def _compare(full, part, before, listed):
    """Every array of the buffer dict: the full-width call's bits on the listed rows, the input's on every other row."""
    assert set(full) == set(part) == set(before)
    for k in before:
        a, b, v = (t[k].detach().cpu().numpy() for t in (full, part, before))
        assert a.dtype == b.dtype == v.dtype and a.shape == b.shape == v.shape, k
        assert b[listed].tobytes() == a[listed].tobytes(), k
        assert b[~listed].tobytes() == v[~listed].tobytes(), k


@pytest.fixture(scope="module")
def renderer():
    return _scene_renderer(SCENE, R.synthetic_env())


def _lights(mode):
    return _device_lights(LR.synthetic_lights(), 1) if ("lit" in mode or "lights" in mode) else None


def _three(r, v, call):
    """``call(b, rows)`` on fresh device copies of ``v``: full width (rows None), on the list, on an empty list -> compared."""
    n = len(v["material"])
    rows, listed = _list(n)
    before, full, part, none = (_to_device(r, v) for _ in range(4))
    call(full, None)
    call(part, rows)
    call(none, _list(n, 0)[0])
    torch.cuda.synchronize()
    _compare(full, part, before, listed)
    _compare(full, none, before, np.zeros(n, dtype=bool))                           # n_rows == 0 writes nothing
    changed = [k for k in before if _bits(full[k]) != _bits(before[k])]
    return changed


@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("rr_depth", [None, 1])
@pytest.mark.parametrize("mode", ["cosine", "lit", "env", "env+lights"])
def test_bounce_rows_is_the_full_width_bounce_on_the_listed_rows(renderer, mode, rr_depth, tail):
    """Three modes (and ENV with lights) x roulette off / active from the first vertex, bounce 2: all seven state arrays."""
    r = renderer
    v = _inputs(mode, True, tail)

    def call(b, rows):
        r.bounce(b, 2, False, SEED, PASS, OFFSET, occlusion=True, lights=_lights(mode), env_dist=_env_dist() if "env" in mode else None,
                 rr_depth=rr_depth, rows=rows)
    changed = _three(r, v, call)
    assert set(changed) == set(STATE7), changed                                      # (the full-width call does write all seven)


@pytest.mark.parametrize("tail", [0, 37])
def test_bounce_rows_last_and_without_ground_truth(renderer, tail):
    r = renderer
    v = _inputs("cosine", False, tail)
    changed = _three(r, v, lambda b, rows: r.bounce(b, 0, True, SEED, PASS, OFFSET, occlusion=True, rows=rows))
    assert "rad" in changed and "mat" in changed


@pytest.mark.parametrize("tail", [0, 37])
def test_sample_emitter_rows(renderer, tail):
    r = renderer
    v = dict(_inputs("cosine", True, tail))
    n = len(v["material"])
    v.update(lsel=np.full(n, -77, dtype=np.int32), emit=np.full((n, 3), 123.25, dtype=np.float32))     # the pre-filled pattern
    lights = _device_lights(LR.synthetic_lights(), 1)
    changed = _three(r, v, lambda b, rows: r.sample_emitter(b, 1, SEED, PASS, OFFSET, occlusion=True, lights=lights, rows=rows))
    assert set(changed) == {"wl", "lsel", "emit"}


@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("mode", ["env", "env+lights"])
def test_sample_env_rows(renderer, mode, tail):
    r = renderer
    src = _inputs("lit" if "lights" in mode else "cosine", True, tail)             # (lsel and wl as sample_emitter leaves them)
    v = {k: a for k, a in src.items() if k != "emit"}
    n = len(v["material"])
    v.update(lpdf=np.full(n, 55.5, dtype=np.float32), emit=np.full((n, 3), 123.25, dtype=np.float32))
    changed = _three(r, v, lambda b, rows: r.sample_env(b, 1, SEED, PASS, OFFSET, occlusion=True, lights=_lights(mode),
                                                        env_dist=_env_dist(), rows=rows))
    assert set(changed) == {"wl", "lpdf", "emit"}


@functools.lru_cache(maxsize=None)
def _tables():
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, reference_bsdf
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable
    _gpu()
    m = MeasuredBSDF(os.path.join(ROOT, "tests", "golden", "chm_orange_rgb.bsdf"))
    return {"measured": MeasuredTable([m, None, m]),
            "analytic": AnalyticTable([reference_bsdf(0), reference_bsdf(23), None], albedo=[(0.9, 0.5, 0.3), (1.0, 1.0, 1.0), (0.2, 0.2, 0.2)])}


@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("with_wl", [True, False])
@pytest.mark.parametrize("which", ["measured", "analytic"])
def test_eval_table_rows(renderer, which, with_wl, tail):
    table = _tables()[which]
    src = _inputs("cosine", True, tail)
    n = len(src["material"])
    v = {k: src[k] for k in ("material", "wi", "wo")}
    v["f_o"] = np.full((n, 3), 7.25, dtype=np.float32)                               # the pre-filled pattern
    if with_wl:
        v.update(wl=src["wl"], f_l=np.full((n, 3), -3.5, dtype=np.float32))

    def call(b, rows):
        table.eval_t(b["mat"], b["wi"], b["wo"], b.get("wl"), tint=(0.9, 0.8, 0.7), out_o=b["f_o"], out_l=b.get("f_l"), rows=rows)
    changed = _three(renderer, v, call)
    assert set(changed) == ({"f_o", "f_l"} if with_wl else {"f_o"})
    rows, listed = _list(n)
    with_gt = listed & np.isin(src["material"], [0, 2] if which == "measured" else [0, 1])
    assert with_gt.sum() > 100 and (listed & ~with_gt).sum() > 100                   # evaluated rows, and listed rows that get NaN


# ---- whole passes ---------------------------------------------------------------------------------------------------------------
N = W * H * SPP
EMITTERS = ("cosine", "lights", "importance+lights")
DEPTHS = ((6, None), (6, 2), (None, 2))
GROUND_TRUTH = ("none", "measured", "analytic")
COMBINATIONS = [(EMITTERS[i], DEPTHS[j], GROUND_TRUTH[(i + j) % 3]) for i in range(3) for j in range(3)]
FULL_WIDTH = ("bsdfd_bucket_by_material", "bsdfd_wf_bounce", "bsdfd_wf_bounce_lit", "bsdfd_wf_bounce_env", "bsdfd_wf_bounce_rr",
              "bsdfd_wf_sample_emitter", "bsdfd_wf_sample_env", "bsdfd_measured_eval_table", "bsdfd_analytic_eval_table")


def _pass_renderer(emitters, max_depth, rr_depth, ground_truth, compact):
    """The 5-ball scene from the low camera (tests/test_gpu_pathtrace.py::_array, low_camera) at 120x90."""
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer, PointLight
    _gpu()
    _, centers, radii = WF.array0_scene(W, H)
    cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=W, height=H)
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, compact=compact, env=_sky())
    if "lights" in emitters:
        lights = five_ball_lights()
        kw["lights"] = [PointLight(tuple(p), tuple(i)) for p, i in zip(lights["position"].tolist(), lights["intensity"].tolist())]
    if emitters == "lights":
        kw["env"] = None                                                             # a black environment that is no emitter
    if emitters == "importance+lights":
        kw["env_sampling"] = "importance"
    if ground_truth == "measured":
        from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF
        kw["ground_truth"] = {0: MeasuredBSDF(os.path.join(ROOT, "tests", "golden", "chm_orange_rgb.bsdf"))}
    elif ground_truth == "analytic":
        from bsdf_diffusion_sampling_amd.analytic import reference_bsdf
        kw["ground_truth"] = {m: reference_bsdf(idx) for m, idx in enumerate((0, 3, 23, 7, 11))}
        kw["ball_albedo"] = [(0.9, 0.5, 0.3), (0.3, 0.9, 0.5), (1.0, 1.0, 1.0), (0.6, 0.6, 0.9), (0.9, 0.8, 0.2)]
    return PathArrayRenderer(MaterialTable(STEMS), [centers[i] for i in ORDER], [radii[i] for i in ORDER], camera=cam, **kw)


def _spy(monkeypatch, names):
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    calls = {name: 0 for name in names}
    for name in names:
        def spy(*args, _inner=getattr(L, name), _name=name):
            calls[_name] += 1
            return _inner(*args)
        monkeypatch.setattr(L, name, spy)
    return calls


def _one_pass(r):
    film = torch.full((H, W, 3), FILL, dtype=torch.float32, device=r.device)
    r.render_pass(film, 0, H, SPP, PASS_SEED, 0)
    torch.cuda.synchronize()
    return film


@pytest.mark.parametrize("emitters,depth,ground_truth", COMBINATIONS)
def test_compact_pass_is_the_full_width_pass_bit_for_bit(monkeypatch, emitters, depth, ground_truth):
    max_depth, rr_depth = depth
    calls = _spy(monkeypatch, FULL_WIDTH + NEW)
    # -- compact=False, with the counts of its bucketings recorded
    plain = _pass_renderer(emitters, max_depth, rr_depth, ground_truth, False)
    counted, bucket = [], plain.table.bucket

    def bucket_recorded(material_id, extra_bins=0):
        plan = bucket(material_id, extra_bins)
        counted.append(list(plan[1]))
        return plan
    plain.table.bucket = bucket_recorded
    film_plain = _one_pass(plain)
    del plain.table.bucket
    n_b = len(plain.table)
    assert all(calls[name] == 0 for name in NEW), calls                              # compact=False calls none of the list forms
    full_width_calls = dict(calls)
    live = [sum(c[:n_b + 1]) for c in counted]
    stats = {k: (list(v) if isinstance(v, list) else v) for k, v in plain.stats.items()}
    print(f"{emitters} max_depth={max_depth} rr_depth={rr_depth} gt={ground_truth}: depth {stats['depth']}, material lanes "
          f"{stats['lanes_per_bounce']}, live lanes {live}")
    # the conditions on the inputs, without which the comparison below shows nothing
    assert stats["depth"] >= 4 and stats["list_per_bounce"] == [N] * stats["depth"]
    assert sum(b < a for a, b in zip(live, live[1:])) >= 2
    assert any(c[n_b] > 0 and sum(x > 0 for x in c[:n_b]) >= 2 for c in counted[1:stats["depth"]])
    if max_depth is None:
        assert 0 < live[stats["depth"] - 1] < 256 and stats["depth_cap_hit"] is False
    # -- compact=True
    for name in calls:
        calls[name] = 0
    comp = _pass_renderer(emitters, max_depth, rr_depth, ground_truth, True)
    assert comp.compact is True and plain.compact is False
    outs, sample_pdf, table_bucket = [], comp.table.sample_pdf, comp.table.bucket
    buckets = []

    def sample_pdf_recorded(plan, wi, wl, **kw):
        own = {k: comp._buffers(N)[k] for k in ("wo", "pdf_o", "pdf_l")}
        got = sample_pdf(plan, wi, wl, **kw)
        outs.append((kw.get("out"), got, own))
        return got

    def table_bucket_counted(*args, **kw):
        buckets.append(1)
        return table_bucket(*args, **kw)
    comp.table.sample_pdf, comp.table.bucket = sample_pdf_recorded, table_bucket_counted
    film_comp = _one_pass(comp)
    del comp.table.sample_pdf, comp.table.bucket
    # the equalities
    assert _bits(film_comp) == _bits(film_plain) and bool(torch.isfinite(film_comp).all()) and float(film_comp.mean()) > FILL
    bp, bc = plain._buffers(N), comp._buffers(N)
    for k in STATE7:
        assert _bits(bc[k]) == _bits(bp[k]), k
    assert (bc["mat"] > n_b).all()
    for k in ("lanes_per_bounce", "depth", "depth_cap_hit"):
        assert comp.stats[k] == stats[k], k
    lists = comp.stats["list_per_bounce"]
    assert lists[0] == N and len(lists) == stats["depth"]
    assert lists[1:] == live[:stats["depth"] - 1]
    # no full-width launch behind bounce 0
    depth_run = stats["depth"]
    assert len(buckets) == 1 and calls["bsdfd_bucket_by_material"] == 1
    for name in FULL_WIDTH:
        assert calls[name] <= 1 and calls[name] == (full_width_calls[name] > 0), (name, calls[name], full_width_calls[name])
    ended_by_bucketing = depth_run < (comp.DEPTH_CAP if max_depth is None else max_depth)
    assert calls["bsdfd_wf_bounce_rows"] == depth_run - 1
    assert calls["bsdfd_bucket_rows"] == depth_run - 1 + ended_by_bucketing
    if "lights" in emitters:
        assert calls["bsdfd_wf_sample_emitter_rows"] == calls["bsdfd_bucket_rows"]
    if emitters == "importance+lights":
        assert calls["bsdfd_wf_sample_env_rows"] == calls["bsdfd_bucket_rows"]
    served = sum(1 for m in stats["lanes_per_bounce"][1:] if m)
    if ground_truth != "none":
        assert calls[f"bsdfd_{ground_truth}_eval_table_rows"] == served > 0
    # sample_pdf behind bounce 0 writes into the renderer's own arrays: nothing N rows long is allocated
    assert len(outs) == 1 + served and outs[0][0] is None
    for out, got, own in outs[1:]:
        assert out is not None
        for t, g, k in zip(out, got, ("wo", "pdf_o", "pdf_l")):
            assert t.data_ptr() == g.data_ptr() == own[k].data_ptr() == comp._buffers(N)[k].data_ptr() and t.shape[0] == N, k


def test_errors(renderer):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    r = renderer
    v = _inputs("env+lights", True)
    n = len(v["material"])
    b = _to_device(r, v)
    before = {k: t.clone() for k, t in b.items()}
    good, _ = _list(n)
    lights = _device_lights(LR.synthetic_lights(), 1)
    bad_lists = (good.to(torch.int32), good.cpu(), torch.arange(n + 1, dtype=torch.int64, device=r.device), good.reshape(-1, 1),
                 torch.arange(2 * LISTED, dtype=torch.int64, device=r.device)[::2])
    for rows in bad_lists:
        with pytest.raises(ValueError, match="rows"):
            r.bounce(b, 0, False, SEED, PASS, OFFSET, occlusion=True, rows=rows)
        with pytest.raises(ValueError, match="rows"):
            r.sample_emitter(b, 0, SEED, PASS, OFFSET, occlusion=True, lights=lights, rows=rows)
        with pytest.raises(ValueError, match="rows"):
            r.sample_env(b, 0, SEED, PASS, OFFSET, occlusion=True, env_dist=_env_dist(), rows=rows)
        for table in _tables().values():
            with pytest.raises(ValueError, match="rows"):
                table.eval_t(b["mat"], b["wi"], b["wo"], b["wl"], out_o=b["f_o"], out_l=b["f_l"], rows=rows)
    # a plan that covers fewer rows than the batch: refused without out=, as before
    table = MaterialTable(STEMS[:N_B])
    plan = table.bucket_rows(b["mat"], good, extra_bins=1)
    assert 0 < plan[0].shape[0] < LISTED
    with pytest.raises(ValueError, match="covers"):
        table.sample_pdf(plan, b["wi"], b["wl"], seed=1, offset=0, direct=True)
    with pytest.raises(ValueError, match="direct"):
        table.sample_pdf(plan, b["wi"], b["wl"], seed=1, offset=0, out=(b["wo"], b["pdf_o"], b["pdf_l"]))
    with pytest.raises(ValueError, match="64"):
        table.bucket_rows(b["mat"], good, extra_bins=62)
    torch.cuda.synchronize()
    for k, t in b.items():                                                           # nothing ran
        assert _bits(t) == _bits(before[k]), k
    # ... and with out= it serves exactly the plan's material rows
    wo, pdf_o, pdf_l = (torch.full_like(b[k], 9.5) for k in ("wo", "pdf_o", "pdf_l"))
    got = table.sample_pdf(plan, b["wi"], b["wl"], seed=1, offset=0, direct=True, out=(wo, pdf_o, pdf_l))
    torch.cuda.synchronize()
    assert got[0] is wo and got[1] is pdf_o and got[2] is pdf_l
    served = np.zeros(n, dtype=bool)
    served[plan[0][: sum(plan[1][:N_B])].cpu().numpy()] = True
    assert served.sum() == sum(plan[1][:N_B]) > 100
    for t in (wo, pdf_o, pdf_l):
        a = t.cpu().numpy()
        assert (a[~served] == 9.5).all() and not (a[served] == 9.5).all(-1).any() if a.ndim == 2 else \
            (a[~served] == 9.5).all() and not (a[served] == 9.5).any()
