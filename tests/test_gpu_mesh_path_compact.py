"""GPU tests of the live-lane list of the path tracer on meshes: the list forms of the two mesh path kernels
(``bsdfd_mesh_bounce_rows``, ``bsdfd_mesh_sample_emitter_rows``) against their full-width siblings — bit for bit on the listed
rows, every byte of the unlisted rows and of the guard rows behind N in place, ``prim`` included — and
``mesh.CompactMeshPathArrayRenderer`` against ``mesh.MeshPathArrayRenderer`` as whole passes: the same film, the same path state,
the same statistics, no full-width launch behind bounce 0, and the same state after every stage of a recorded pass.

The kernel tests run on ``mesh_bounce_ref.kernel_scene`` with ``synthetic_vertices(geom, n)`` for n = 4096 and 4133 (odd, no
multiple of the wave or of the block) and the seeded shuffle ``default_rng(17 + n).permutation(n)[:1000]`` as the list: unsorted, a
multiple neither of 64 nor of 256, with more than 100 rows of either material, of the floor and of ended paths (132 / 128 / 611 /
129 at n = 4096, 134 / 115 / 610 / 141 at n = 4133).  The whole passes are cases a, c, e and f of
tests/test_gpu_mesh_pass_replay.py (64 x 48, 2 spp) and its two-shells scene at 32 x 24, unbounded."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import mesh_bounce_ref as MB  # noqa: E402
import pass_replay as PR  # noqa: E402
import pathtrace_lights_ref as LR  # noqa: E402
import test_gpu_mesh_pass_replay as TR  # noqa: E402
import test_gpu_mesh_path as TP  # noqa: E402
from bsdf_diffusion_sampling_amd import _lib, mesh as M  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402

LISTED = 1000
GUARD = TP.GUARD
STATE8 = TR.KEYS                                  # org, nrm, wi, wl, mat, prim, beta, rad: what a bounce may write
FULL_WIDTH = ("bsdfd_mesh_bounce", "bsdfd_mesh_sample_emitter", "bsdfd_bucket_by_material")
LIST_FORMS = ("bsdfd_mesh_bounce_rows", "bsdfd_mesh_sample_emitter_rows", "bsdfd_bucket_rows")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_renderer():
    """A plain renderer on the kernel scene (cosine; the lit calls are handed their lights)."""
    return TR._make_renderer(False, True, "disk", 4, None)


@functools.lru_cache(maxsize=None)
def _vertices(n):
    """The synthetic wavefront of n rows (made once per size; nobody changes it), ids under the renderer's name."""
    v = MB.synthetic_vertices(TR._world()["geom"], n)
    v["mat"] = v.pop("material")
    return v


def _lights(has_env=1):
    return TP._device_lights(LR.make_lights([(1.0, 4.0, 2.0), (-2.5, 3.0, -1.0)], [40.0, (30.0, 20.0, 10.0)]), has_env)


@functools.lru_cache(maxsize=None)
def _lit_vertices(n):
    """The vertices a LIT bounce meets: wl, lsel and emit as the full-width emitter sample leaves them."""
    v = dict(_vertices(n))
    v.update(lsel=np.full(n, -77, dtype=np.int32), emit=np.full((n, 3), 123.25, dtype=np.float32))
    big, b = _to_device(v)
    _kernel_renderer().sample_emitter(b, TP.BOUNCE, TP.SEED, TP.PASS, TP.OFFSET, occlusion=True, lights=_lights())
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in b.items()}


def _to_device(v):
    """(the arrays with GUARD rows of -7 behind them, the buffer dict of their first N rows)."""
    n = len(v["mat"])
    big = {k: TP._guarded(a, n) for k, a in v.items()}
    return big, {k: t[:n] for k, t in big.items()}


def _lists(v):
    """The seeded shuffle of LISTED rows, the same rows sorted by material (stable in lane order: the order render_pass produces),
    the empty list, and the mask of the listed rows over N + GUARD rows."""
    n = len(v["mat"])
    rows = np.random.default_rng(17 + n).permutation(n)[:LISTED].astype(np.int64)
    assert (np.diff(rows) < 0).any() and LISTED % 64 and LISTED % 256                # unsorted; no multiple of the wave or the block
    by_lane = np.sort(rows)
    by_material = by_lane[np.argsort(v["mat"][by_lane], kind="stable")]
    n_b = TR._world()["geom"]["n_materials"]
    ids = v["mat"][rows]
    classes = [int((ids == m).sum()) for m in range(n_b + 1)] + [int((ids > n_b).sum())]
    assert min(classes) >= 100, classes                                              # either material, the floor, ended paths
    listed = np.zeros(n + GUARD, dtype=bool)
    listed[rows] = True
    to_dev = lambda a: torch.from_numpy(a).to(TP.dev())
    return to_dev(rows), to_dev(by_material), to_dev(rows[:0].copy()), listed


def _three(v, call):
    """``call(b, rows)`` on fresh device copies of ``v``: full width (rows None), on the shuffled list, on the list sorted by
    material, on the empty list.  On listed rows every array has the full-width call's bits; every other row, the guard rows
    included, keeps the input's bytes.  -> the names of the arrays the full-width call changed."""
    rows, by_material, empty, listed = _lists(v)
    (before, _), (full, b_full), (part, b_part), (ordered, b_ordered), (none, b_none) = (_to_device(v) for _ in range(5))
    call(b_full, None)
    call(b_part, rows)
    call(b_ordered, by_material)
    call(b_none, empty)
    torch.cuda.synchronize()
    for k in before:
        f, p, o, e, v0 = (t[k].cpu().numpy() for t in (full, part, ordered, none, before))
        assert p[listed].tobytes() == f[listed].tobytes(), k
        assert p[~listed].tobytes() == v0[~listed].tobytes(), k
        assert o.tobytes() == p.tobytes(), k                                         # the order of the list does not matter
        assert e.tobytes() == v0.tobytes(), k                                        # n_rows == 0 writes nothing
        assert (f[len(v["mat"]):] == -7).all(), k
    return {k for k in before if _bits(full[k]) != _bits(before[k])}


BOUNCE_CASES = [(mode, rr, last, 1) for mode in MB.MODES for rr in (None, 1) for last in (0, 1)] + [("cosine", None, 0, 0)]


@pytest.mark.parametrize("n", [4096, 4133])
@pytest.mark.parametrize("mode,rr_depth,last,occlusion", BOUNCE_CASES)
def test_bounce_rows_is_the_full_width_bounce_on_the_listed_rows(mode, rr_depth, last, occlusion, n):
    r = _kernel_renderer()
    v = _lit_vertices(n) if mode == "lit" else _vertices(n)
    lights = _lights() if mode == "lit" else None

    def call(b, rows):
        r.bounce(b, TP.BOUNCE, bool(last), TP.SEED, TP.PASS, TP.OFFSET, occlusion=bool(occlusion), lights=lights, rr_depth=rr_depth,
                 rows=rows)
    changed = _three(v, call)
    # (not vacuous) the full-width call writes all eight state arrays where paths go on; rad and the id where they all end — at the
    # last bounce, and without occlusion, where nothing is intersected
    assert changed == (set(STATE8) if occlusion and not last else {"rad", "mat"}), changed


@pytest.mark.parametrize("n", [4096, 4133])
@pytest.mark.parametrize("has_env", [0, 1])
def test_sample_emitter_rows_is_the_full_width_sample_on_the_listed_rows(has_env, n):
    r = _kernel_renderer()
    v = dict(_vertices(n))
    v.update(lsel=np.full(n, -77, dtype=np.int32), emit=np.full((n, 3), 123.25, dtype=np.float32))    # the pre-filled pattern
    lights = _lights(has_env)
    changed = _three(v, lambda b, rows: r.sample_emitter(b, TP.BOUNCE, TP.SEED, TP.PASS, TP.OFFSET, occlusion=True, lights=lights,
                                                         rows=rows))
    assert changed == {"wl", "lsel", "emit"}, changed


def test_bad_lists_are_refused_and_nothing_runs():
    r = _kernel_renderer()
    v = dict(_lit_vertices(4096))
    n = len(v["mat"])
    big, b = _to_device(v)
    before = {k: t.clone() for k, t in big.items()}
    good = _lists(v)[0]
    lights = _lights()
    bad_lists = (good.to(torch.int32), good.cpu(), torch.arange(n + 1, dtype=torch.int64, device=good.device), good.reshape(-1, 1),
                 torch.arange(2 * LISTED, dtype=torch.int64, device=good.device)[::2])
    for rows in bad_lists:
        with pytest.raises(ValueError, match="rows"):
            r.bounce(b, 0, False, TP.SEED, TP.PASS, TP.OFFSET, occlusion=True, rows=rows)
        with pytest.raises(ValueError, match="rows"):
            r.sample_emitter(b, 0, TP.SEED, TP.PASS, TP.OFFSET, occlusion=True, lights=lights, rows=rows)
    with pytest.raises(ValueError, match="not on meshes yet"):                       # env_dist stays refused, with a list too
        r.bounce(b, 0, False, TP.SEED, TP.PASS, TP.OFFSET, occlusion=True, env_dist=object(), rows=good)
    torch.cuda.synchronize()
    for k, t in big.items():
        assert _bits(t) == _bits(before[k]), k


# ---- whole passes ---------------------------------------------------------------------------------------------------------------
def _make(cls, lit, with_env, kind, depth, rr, geom=None, scene=None, camera=None):
    """test_gpu_mesh_pass_replay._make_renderer for either class: the same scene, camera, sky, lights and tables."""
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    w = TR._world()
    geom = geom or w["geom"]
    kw = dict(max_depth=depth, rr_depth=rr, albedo=tuple(geom["albedo"]))
    if lit:
        lights = TR.mesh_lights()
        kw["lights"] = [PointLight(tuple(p), tuple(i)) for p, i in zip(lights["position"].tolist(), lights["intensity"].tolist())]
    if kind == "analytic":
        from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
        kw.update(ground_truth=ground_truth_for(TR.ANALYTIC), ball_albedo=w["ball_albedo"])
    return cls(TR._table(kind), scene or w["scene"], camera=camera or TR.mesh_camera(), env=TR._sky() if with_env else None, **kw)


@functools.lru_cache(maxsize=None)
def _shells():
    """test_gpu_mesh_pass_replay._recorded_shells' scene: two 57 152-triangle shells of the fixture scene over its plane."""
    w, h = TR.SHELLS_SIZE
    _, _, full, _ = M.mesh_scene_from_matpreview_xml(TP.SCENE_FILE, TP.MESH_FILE, w, h)
    shells = [i for i in full.instances if i.material is not None][:2]
    plane = next(i for i in full.instances if i.checker is not None)
    inst = [M.Instance(s.mesh, s.to_world, material=k) for k, s in enumerate(shells)] + [plane]
    return dict(scene=M.MeshScene(full.meshes, inst), geom=dict(meshes=full.meshes, instances=inst, n_materials=2, albedo=[0.9, 0.6, 0.3]),
                camera=WF.Camera(origin=(1.0, 1.05, -1.5), target=(-3.5, 0.75, -1.5), fov_deg=40.0, width=w, height=h))


def _pair(case):
    """(plain, compact, rows, pass index) of a case of the replay tests, or of the two-shells scene unbounded with rr_depth 2."""
    if case == "shells":
        kw = _shells()
        args, rows, pass_idx = (False, True, "disk", None, 2), (0, TR.SHELLS_SIZE[1]), 0
    else:
        lit, with_env, kind, depth, rr, tile, pass_idx, _ = TR.CASES[case]
        kw, args, rows = {}, (lit, with_env, kind, depth, rr), tile or (0, TR.H)
    return _make(M.MeshPathArrayRenderer, *args, **kw), _make(M.CompactMeshPathArrayRenderer, *args, **kw), rows, pass_idx


def _spy(monkeypatch, names):
    L = _lib.lib()
    calls = {name: 0 for name in names}
    for name in names:
        def spy(*args, _inner=getattr(L, name), _name=name):
            calls[_name] += 1
            return _inner(*args)
        monkeypatch.setattr(L, name, spy)
    return calls


def _one_pass(r, rows, pass_idx):
    film = torch.full((rows[1] - rows[0], r.camera.width, 3), TR.FILL, dtype=torch.float32, device=r.device)
    r.render_pass(film, rows[0], rows[1], TR.SPP, TR.SEED, pass_idx)
    torch.cuda.synchronize()
    return film


@pytest.mark.parametrize("case", ["a", "c", "e", "f", "shells"])
def test_compact_pass_is_the_plain_pass_bit_for_bit(monkeypatch, case):
    TP.dev()
    calls = _spy(monkeypatch, FULL_WIDTH + LIST_FORMS)
    plain, comp, rows, pass_idx = _pair(case)
    assert type(comp) is M.CompactMeshPathArrayRenderer and comp.compact is True and plain.compact is False
    n = (rows[1] - rows[0]) * plain.camera.width * TR.SPP
    n_b = len(plain.table)
    # -- the plain pass, with the counts of its bucketings recorded
    counted, bucket = [], plain.table.bucket

    def bucket_recorded(material_id, extra_bins=0):
        plan = bucket(material_id, extra_bins)
        counted.append(list(plan[1]))
        return plan
    plain.table.bucket = bucket_recorded
    film_plain = _one_pass(plain, rows, pass_idx)
    del plain.table.bucket
    assert all(calls[name] == 0 for name in LIST_FORMS), calls                       # the plain pass calls none of the list forms
    plain_calls = dict(calls)
    stats = {k: (list(v) if isinstance(v, list) else v) for k, v in plain.stats.items()}
    depth = stats["depth"]
    live = [sum(c[:n_b + 1]) for c in counted]
    print(f"case {case}: {n} paths, depth {depth}, material lanes {stats['lanes_per_bounce']}, live lanes {live}, "
          f"bucketings {[c[:n_b + 1] for c in counted]}")
    # the conditions on the inputs, without which the equalities below show nothing
    assert depth >= 3 and stats["list_per_bounce"] == [n] * depth
    assert sum(b < a for a, b in zip(live, live[1:])) >= 2
    assert any(c[n_b] > 0 and all(x > 0 for x in c[:n_b]) for c in counted[1:depth])  # a list with floor lanes and both materials
    assert any(x % 64 for x in live[:depth - 1])                                      # a list that is no multiple of the wave
    # -- the compact pass
    for name in calls:
        calls[name] = 0
    film_comp = _one_pass(comp, rows, pass_idx)
    assert _bits(film_comp) == _bits(film_plain) and bool(torch.isfinite(film_comp).all()) and float(film_comp.mean()) > TR.FILL
    bp, bc = plain._buffers(n), comp._buffers(n)
    for k in STATE8:
        assert bc[k].shape[0] == n and _bits(bc[k]) == _bits(bp[k]), k
    for k in ("lanes_per_bounce", "depth", "depth_cap_hit"):
        assert comp.stats[k] == stats[k], k
    lists = comp.stats["list_per_bounce"]
    print(f"  lists {lists}; calls {calls}")
    assert lists[0] == n and len(lists) == depth and lists[1:] == live[:depth - 1]
    # no full-width launch behind bounce 0
    for name in FULL_WIDTH:
        assert calls[name] <= 1 and calls[name] == (plain_calls[name] > 0), (name, calls[name], plain_calls[name])
    assert calls["bsdfd_mesh_bounce"] == 1 and calls["bsdfd_bucket_by_material"] == 1
    assert calls["bsdfd_mesh_bounce_rows"] == depth - 1
    ended_by_bucketing = depth < (comp.DEPTH_CAP if comp.max_depth is None else comp.max_depth)
    assert calls["bsdfd_bucket_rows"] == depth - 1 + ended_by_bucketing
    if comp.lights is not None:
        assert calls["bsdfd_mesh_sample_emitter"] == 1
        assert calls["bsdfd_mesh_sample_emitter_rows"] == calls["bsdfd_bucket_rows"] > 0
    else:
        assert calls["bsdfd_mesh_sample_emitter"] == calls["bsdfd_mesh_sample_emitter_rows"] == 0


def test_every_stage_of_a_compact_pass_leaves_the_plain_pass_state():
    """Case f (lit, rr_depth 1, a tile, depth 4), both passes recorded: an unlisted row that is written and overwritten later
    would leave the final state alone and show here."""
    plain, comp, rows, pass_idx = _pair("f")
    n_b = len(plain.table)
    recorded = []
    n = (rows[1] - rows[0]) * plain.camera.width * TR.SPP
    for r in (plain, comp):
        for t in r._buffers(n).values():    # lsel and emit are written on live lanes only: the same pattern under both passes
            t.fill_(-77)
        film = torch.full((rows[1] - rows[0], r.camera.width, 3), TR.FILL, dtype=torch.float32, device=r.device)
        with PR.Recorder(r) as rec:
            r.render_pass(film, rows[0], rows[1], TR.SPP, TR.SEED, pass_idx)
        torch.cuda.synchronize()
        recorded.append([s for s in rec.stages if s["name"] in ("sample_emitter", "bounce")])
    sp, sc = recorded
    assert [s["name"] for s in sp] == [s["name"] for s in sc] and sum(s["name"] == "bounce" for s in sp) >= 3
    assert [s["args"] for s in sp] == [s["args"] for s in sc]
    seen_lists = answered = 0
    for k, (a, b) in enumerate(zip(sp, sc)):
        assert "rows" not in a.get("extra", {})
        first = a["args"]["bounce"] == 0
        assert ("rows" in b.get("extra", {})) == (not first), (k, a["name"])
        seen_lists += not first
        for key in STATE8 + ("lsel", "emit"):
            assert b["before"][key].tobytes() == a["before"][key].tobytes(), (k, a["name"], key, "before")
            assert b["after"][key].tobytes() == a["after"][key].tobytes(), (k, a["name"], key)
        if a["name"] == "bounce":       # the sampler's answers: on this bounce's material lanes (elsewhere the list form leaves them unfilled)
            lanes = (a["before"]["mat"] >= 0) & (a["before"]["mat"] < n_b)
            answered += int(lanes.sum()) * (not first)
            for key in ("wo", "pdf_o", "pdf_l"):
                assert b["before"][key][lanes].tobytes() == a["before"][key][lanes].tobytes(), (k, key)
    print(f"{len(sp)} stages, {seen_lists} of them on a list; {answered} material lanes answered behind bounce 0")
    assert seen_lists >= 4 and answered >= 100


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def test_render_array_tool_compact_writes_the_same_image(tmp_path):
    TP.dev()
    images = []
    for flag in ([], ["--compact"]):
        out = str(tmp_path / ("mesh_path" + "_compact" * bool(flag)))
        cmd = [sys.executable, os.path.join(TP.ROOT, "tools", "render_array.py"), "--scene", TP.SCENE_FILE, "--mesh-file", TP.MESH_FILE,
               "--max-depth", "3", "--width", "32", "--height", "24", "--passes", "1", "--out", out] + flag
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-2000:]
        line = done.stdout.strip().splitlines()[-1]
        print(line)
        assert '"max_depth": 3' in line and ('"compact": true' in line) == bool(flag)
        images.append(np.load(out + ".npy"))
    assert images[0].shape == (24, 32, 3) and np.isfinite(images[0]).all() and images[0].max() > 0
    assert images[1].tobytes() == images[0].tobytes()
