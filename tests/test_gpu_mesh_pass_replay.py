"""GPU tests of ``mesh.MeshPathArrayRenderer.render_pass`` as a WHOLE: one recorded pass per case (tests/pass_replay.py
``Recorder``), held stage by stage to the fp64 references of the kernel tests (tests/mesh_ref.py, tests/mesh_bounce_ref.py) and, end
to end, to ``pass_replay.reference_mesh_pass``.

tests/test_gpu_mesh_path.py runs every mesh path kernel alone on one synthetic wavefront and holds the renderer by statements
about images.  Here the loop that strings the kernels together is on the bench: the order of the stages and the scalars they are
handed (bounce, last, seed, pass, path offset, occlusion, the sampler's key per bounce), ``path_begin`` being the no-op it is
documented to be, ``prim`` — the state array the mesh renderer adds — carried from stage to stage and written by the bounce alone,
each stage on the REAL wavefront a pass meets (tens of live lanes at depth, samples that enter a closed mesh, a mirrored instance
reached by a secondary ray, answer buffers nobody wrote), the sampler's rows bit for bit, the evaluator on the ``wl`` the emitter
stage left, roulette on the throughputs a pass forms, the end of an unbounded pass, the film, and tiles.

The scene (cases a .. g): ``mesh_bounce_ref.kernel_scene`` — three 128-triangle octahedra with normals = positions (plain:
material 0; scaled and rotated: material 1; mirrored: diffuse 0.3) over a checkered 4 x 4 grid floor at y = -1.2 — seen from
(1.0, 2.5, 9.0) at 64 x 48, 2 spp, seed 4, a film pre-filled with 0.25, the sky make_sky(64, 128, 5), three lights
(tests/test_mesh_pass_replay_cpu.py holds the reference to itself on exactly this scene).  Rows 0-9 see only sky, rows 30-47 only
the floor.  Exclusions are the kernel tests': rows whose ray is marginal (at most 1 % of a stage's live rows), whose next vertex
is fragile (at most 3 %), whose roulette decision is too close to call, and paths whose histories differ (at most 0.1 %); each is
counted, printed and held to its cap.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dielectric_ref as D  # noqa: E402
import mesh_bounce_ref as MB  # noqa: E402
import mesh_ref as MR  # noqa: E402
import pass_replay as PR  # noqa: E402
import pathtrace_ref as R  # noqa: E402
import principled_ref as PRI  # noqa: E402
from bsdf_diffusion_sampling_amd import mesh as M  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402
from oracle import wavefront_oracle as WO  # noqa: E402
from test_gpu_analytic_table import _err, _held_to_yardstick  # noqa: E402
from test_gpu_mesh_path import MESH_FILE, SCENE_FILE, _bytes_equal, _shade_bound, dev  # noqa: E402
from test_mesh_pass_replay_cpu import CAMERA, FLOOR_ROWS, SKY_ROWS, mesh_camera, mesh_lights, through_a_mesh  # noqa: E402

W, H, SPP, SEED, FILL = CAMERA["width"], CAMERA["height"], 2, 4, 0.25
TILE = (5, 41)
#            lights  env    table       depth  rr    rows  pass  occlusion
CASES = {"a": (False, True, "disk", 4, None, None, 0, None),
         "b": (False, True, "analytic", 3, None, TILE, 1, None),
         "c": (True, True, "analytic", 3, None, None, 1, None),
         "d": (True, False, "disk", 3, None, TILE, 0, None),
         "e": (False, True, "disk", None, 2, None, 0, None),
         "f": (True, True, "disk", 4, 1, TILE, 1, None),
         "g": (False, True, "disk", 1, None, None, 0, False)}
ANALYTIC = ["bsdf_13", "bsdf_24"]                 # a principled material and the rough dielectric of alpha 0.3
KEYS = ("org", "nrm", "wi", "wl", "mat", "prim", "beta", "rad")           # what a bounce may write
VERTEX = ("org", "nrm", "wi", "mat", "prim", "wl")
ANSWERS = ("wo", "pdf_o", "pdf_l")


def _sky():
    return WF.make_sky(64, 128, seed=5)


# ---- the scene, the tables and the renderers: made once ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world():
    dev()
    geom = MB.kernel_scene(M)
    return dict(geom=geom, scene=M.MeshScene(geom["meshes"], geom["instances"]), ball_albedo=WF.albedos_from_matpreview_xml(SCENE_FILE)[:2])


@functools.lru_cache(maxsize=None)
def _table(kind):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    if kind == "disk":
        return MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS[:2]])
    return MaterialTable([s + "_spherical" for s in ANALYTIC])


def _make_renderer(lit, with_env, kind, depth, rr, occlusion=None, geom=None, scene=None, camera=None):
    """A ``MeshPathArrayRenderer`` on the scene: the proxy's albedo is the geometry dict's, the lights are
    test_mesh_pass_replay_cpu.mesh_lights(), the analytic table has ground truth on both materials and the scene file's first two
    ball albedos (test_both_tables_render's setup)."""
    from bsdf_diffusion_sampling_amd.pathtrace import PointLight
    w = _world()
    geom = geom or w["geom"]
    kw = dict(max_depth=depth, rr_depth=rr, occlusion=occlusion, albedo=tuple(geom["albedo"]))
    if lit:
        lights = mesh_lights()
        kw["lights"] = [PointLight(tuple(p), tuple(i)) for p, i in zip(lights["position"].tolist(), lights["intensity"].tolist())]
    if kind == "analytic":
        from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
        kw.update(ground_truth=ground_truth_for(ANALYTIC), ball_albedo=w["ball_albedo"])
    return M.MeshPathArrayRenderer(_table(kind), scene or w["scene"], camera=camera or mesh_camera(), env=_sky() if with_env else None, **kw)


def _renderer(case):
    lit, with_env, kind, depth, rr, _, _, occlusion = CASES[case]
    return _make_renderer(lit, with_env, kind, depth, rr, occlusion)


def _record_pass(r, rows, pass_idx, fill=FILL):
    r0, r1 = rows
    film = torch.full((r1 - r0, r.camera.width, 3), fill, dtype=torch.float32, device=r.device)
    with PR.Recorder(r) as rec:
        r.render_pass(film, r0, r1, SPP, SEED, pass_idx)
    torch.cuda.synchronize()
    k = 0
    for s in rec.stages:          # the bounce a stage belongs to: the bounces that ran before it
        s["k"] = k
        k += s["name"] == "bounce"
    return rec.stages, dict(r.stats), film


def _context(r, case_tuple, stages, stats, rows, geom, cast=None):
    lit, with_env, kind, depth, rr, _, pass_idx, _ = case_tuple
    width = r.camera.width
    return dict(r=r, stages=stages, stats=stats, rows=rows, offset=rows[0] * width * SPP, cam_scene=PR.scene_of(r), geom=geom,
                env=_sky().numpy() if with_env else None, with_env=with_env, lights=mesh_lights() if lit else None, lit=lit,
                gt=kind == "analytic", depth=depth, rr=rr, pass_idx=pass_idx, occlusion=r.occlusion, n_b=len(r.table),
                n=(rows[1] - rows[0]) * width * SPP, cast=cast, width=width)


@functools.lru_cache(maxsize=None)
def _recorded(case):
    """ONE recorded render_pass of the case, shared by its tests (nobody changes it)."""
    r = _renderer(case)
    rows = CASES[case][5] or (0, H)
    stages, stats, _ = _record_pass(r, rows, CASES[case][6])
    return _context(r, CASES[case], stages, stats, rows, _world()["geom"])


def _named(rec, name):
    return [s for s in rec["stages"] if s["name"] == name]


def _codes(rec, snap):
    return PR.mesh_decision_code(rec["geom"], snap["mat"], snap["prim"], snap["wi"])


def _live(rec, snap):
    return (snap["mat"] >= 0) & (snap["mat"] <= rec["n_b"])


# ---- 1. the order of the stages and what they are handed ------------------------------------------------------------------------
def _check_order_and_arguments(rec, tag):
    r, n_b, offset, lit, gt, pass_idx = (rec[k] for k in ("r", "n_b", "offset", "lit", "gt", "pass_idx"))
    depth = r.DEPTH_CAP if rec["depth"] is None else rec["depth"]
    buckets = _named(rec, "bucket")
    want, lanes = ["primary", "path_begin"], []
    for k in range(depth):
        want += ["sample_emitter"] * lit + ["bucket"]
        if k >= len(buckets):
            break
        counts = buckets[k]["counts"]
        n_mat = sum(counts[:n_b])
        if n_mat + counts[n_b] == 0:                 # the loop stops at the first bucketing without a live lane
            break
        lanes.append(n_mat)
        want += (["sample_pdf"] + ["eval_t"] * gt) * (n_mat > 0) + ["bounce"]
    want.append("resolve")
    got = [s["name"] for s in rec["stages"]]
    print(f"{tag}: {' '.join(got)}; material lanes per bounce {rec['stats']['lanes_per_bounce']}")
    assert got == want
    assert not any("extra" in s for s in rec["stages"])        # render_pass hands the stages the documented scalars and nothing else
    # the ids the bucketing saw are the state's, and its counts are theirs
    for s in buckets:
        assert s["args"] == dict(extra_bins=2, ids_are_state=True)
        assert s["counts"] == np.bincount(s["before"]["mat"], minlength=n_b + 2).tolist()
    bounces = _named(rec, "bounce")
    stats = rec["stats"]
    assert stats["lanes_per_bounce"] == lanes == [int((s["before"]["mat"] < n_b).sum()) for s in bounces]
    assert stats["depth"] == len(bounces) and stats["list_per_bounce"] == [rec["n"]] * len(bounces)
    assert stats["depth_cap_hit"] is False
    # the scalars
    rows = rec["rows"]
    tile = dict(row_begin=rows[0], row_end=rows[1], spp=SPP)
    assert _named(rec, "primary")[0]["args"] == dict(tile, seed=SEED, pass_idx=pass_idx)
    assert _named(rec, "resolve")[0]["args"] == tile
    assert _named(rec, "path_begin")[0]["args"] == {}
    assert offset == rows[0] * rec["width"] * SPP
    for name in ("sample_emitter", "bounce"):
        for s in _named(rec, name):
            a = dict(bounce=s["k"], seed=SEED, pass_idx=pass_idx, path_offset=offset, occlusion=rec["occlusion"])
            if name == "bounce":
                a["last"] = s["k"] == depth - 1
            assert s["args"] == a, (name, s["k"], s["args"])
    n_keys = len(bounces) + 1
    keys = {(p, k): PR.sampler_key(SEED, p, k) for p in (0, 1) for k in range(n_keys)}
    assert len(set(keys.values())) == 2 * n_keys               # pairwise distinct across the bounces of passes 0 and 1
    for s in _named(rec, "sample_pdf"):
        a = s["args"]
        assert a["seed"] == keys[(pass_idx, s["k"])] and a["offset"] == offset, (s["k"], hex(a["seed"]))
        assert a["wi_is_state"] and a["wl_is_state"] and a["counts"] == buckets[s["k"]]["counts"]
    tint = [float(v) for v in r.plugin.albedo.tolist()]
    assert tint == [float(np.float32(v)) for v in rec["geom"]["albedo"]]
    for s in _named(rec, "eval_t"):
        assert s["args"] == dict(tint=tint, reads_state=True, writes_state=True)
    return bounces, lanes


@pytest.mark.parametrize("case", list(CASES))
def test_stages_come_in_the_documented_order_with_the_documented_arguments(case):
    lit, with_env, kind, depth, rr, _, pass_idx, occlusion = CASES[case]
    rec = _recorded(case)
    bounces, lanes = _check_order_and_arguments(rec, f"case {case}")
    assert rec["occlusion"] is (occlusion is None)             # implied by depth > 1 everywhere but in g, which switches it off
    assert rec["r"].rr_depth == rr
    if depth is not None:
        assert len(bounces) == depth
        if case in "abcd":
            assert lanes[-1] >= 20                              # (not vacuous: material lanes are served at the last bounce)
    else:   # the end of an unbounded pass: the loop stopped because nothing was alive, not at the cap
        assert 2 <= len(bounces) < rec["r"].DEPTH_CAP
        before_resolve = rec["stages"][-2]
        assert before_resolve["name"] in ("bucket", "bounce") and not _live(rec, before_resolve["after"]).any()
        live = [int(_live(rec, s["before"]).sum()) for s in bounces]
        print(f"  live lanes per bounce {live}")
        assert all(b <= a for a, b in zip(live, live[1:])) and not any(s["args"]["last"] for s in bounces)


# ---- 2. nothing writes the state between two stages ------------------------------------------------------------------------------
def _check_no_writes_between_stages(rec):
    stages = rec["stages"]
    assert "prim" in stages[0]["after"] and stages[0]["after"]["prim"].dtype == np.int32
    for s, t in zip(stages, stages[1:]):
        assert set(s["after"]) == set(t["before"]), (s["name"], t["name"])
        for key, a in s["after"].items():
            assert a.dtype == t["before"][key].dtype and a.tobytes() == t["before"][key].tobytes(), (s["name"], t["name"], key)
    for s in stages:                       # prim is the bounce's to write (and primary's, where the dict comes from); everybody else reads it
        if s["name"] not in ("primary", "bounce"):
            assert s["before"]["prim"].tobytes() == s["after"]["prim"].tobytes(), s["name"]
    begin = _named(rec, "path_begin")
    assert len(begin) == 1
    for key, a in begin[0]["before"].items():                  # path_begin: a no-op on meshes
        assert a.tobytes() == begin[0]["after"][key].tobytes(), key


@pytest.mark.parametrize("case", list(CASES))
def test_nothing_writes_the_state_between_two_stages(case):
    """What a stage left is, byte for byte, what the next one finds — every array of the buffer dict, ``prim`` and the ones
    nobody has written yet included — and ``path_begin`` changes nothing."""
    _check_no_writes_between_stages(_recorded(case))


# ---- 3. every stage against its reference, on the device's own input -----------------------------------------------------------
def _cap(flags, rows, cap, what):
    """At most ``cap`` of the stage's ``rows`` (or one row, as mesh_ref.assert_marginal_cap allows a small set) carry the flag."""
    count, size = int((flags & rows).sum()), int(rows.sum())
    assert count <= max(cap * size, 1), f"{what}: {count} of {size} rows"
    return count


def _tol_n(eb, nxt):
    """tests/test_gpu_mesh.py's bound of an interpolated unit normal, from the barycentrics' error bar."""
    return 2 * 3 * (4 * eb) / nxt["mix_len"].min() + 16 * 2.0 ** -24


def _check_primary(rec):
    """test_mesh_path_primary's assertions on the recorded first vertex, against the reference's: the camera rays are the
    oracle's, the hit the reference's closest one from the camera's origin, the vertex mesh_ref.primary_arrays'."""
    geom, n_b, rows, n = rec["geom"], rec["n_b"], rec["rows"], rec["n"]
    meshes, inst = geom["meshes"], geom["instances"]
    b = _named(rec, "primary")[0]["after"]
    _, wl_o, _, d_o = WO.primary(rec["cam_scene"], rows[0], rows[1], SPP, SEED, rec["pass_idx"])
    assert np.abs(b["dir"] - d_o).max() < 1e-6 and np.abs(b["wl"] - wl_o).max() < 2e-6
    cam = np.tile(np.asarray(rec["cam_scene"]["origin"], dtype=np.float32), (n, 1))
    ref = (rec["cast"] or MR.brute_force)(meshes, inst, cam, b["dir"])
    et, eb = MR.fp32_restatement_error(meshes, inst, cam, b["dir"], ref)
    nxt = MR.primary_arrays(meshes, inst, n_b, b["dir"], ref, bary_tol=4 * eb)
    hit_ref = ref["prim"][:, 0] >= 0
    everyone = np.ones(n, dtype=bool)
    n_marginal = _cap(ref["marginal"], everyone, MR.MARGINAL_CAP, "marginal camera rays")
    fragile = nxt["fragile"] & hit_ref
    n_fragile = _cap(fragile, everyone, 0.03, "fragile first vertices")
    ok = ~ref["marginal"] & ~fragile
    differ = ok & ((b["mat"] != nxt["material"]) | (b["prim"] != ref["prim"]).any(1))
    print(f"  primary: {n} paths, ids {np.bincount(b['mat'], minlength=n_b + 2).tolist()}, {n_marginal} marginal, {n_fragile} fragile, "
          f"{int(differ.sum())} of the others decide differently; fp32 restatement: t rel {et:.3e}, bary abs {eb:.3e}")
    assert not differ.any(), np.nonzero(differ)[0][:8]
    hit = b["prim"][:, 0] >= 0
    assert np.array_equal(hit, b["mat"] <= n_b)
    assert (b["beta"] == 1).all() and (b["rad"][hit] == 0).all() and (b["prim"][~hit] == -1).all() and (b["org"][~hit] == 0).all()
    on = ok & hit_ref
    if on.any():
        x = cam[on].astype(np.float64) + ref["t"][on, None] * b["dir"][on].astype(np.float64)
        e_org = (np.abs(b["org"][on] - x).max(1) / ref["t"][on]).max()
        tol_n = _tol_n(eb, nxt)
        e_nrm = np.abs(b["nrm"][on] - nxt["nrm"][on]).max()
        lanes, diffuse = on & (nxt["material"] < n_b), on & (nxt["material"] == n_b)
        e_wi = np.abs(b["wi"][lanes] - nxt["wi"][lanes]).max(initial=0.0)
        print(f"    org / t {e_org:.3e} (bound {4 * et:.3e}); nrm {e_nrm:.3e} (bound {tol_n:.3e}); wi {e_wi:.3e} (bound {4 * tol_n:.3e})")
        assert e_org <= 4 * et and e_nrm <= tol_n and e_wi <= 4 * tol_n
        assert np.array_equal(b["wi"][diffuse], nxt["wi"][diffuse].astype(np.float32))    # reflectances: exact
    if rec["with_env"] and (~hit).any():
        p999, worst = _shade_bound(b["rad"][~hit], WO.env_lookup(rec["env"].astype(np.float64), b["dir"][~hit]))
        print(f"    rad of the {int((~hit).sum())} misses against the lookup: p99.9 {p999:.2e} max {worst:.2e}")
        assert p999 < 2e-4 and worst < 5e-3
    if not rec["with_env"]:
        assert (b["rad"] == 0).all()


def _check_sample_emitter(rec, s):
    """test_mesh_sample_emitter_matches_reference's assertions and exclusions on one recorded call."""
    geom, n_b = rec["geom"], rec["n_b"]
    v, got = s["before"], s["after"]
    want = MB.sample_emitter(geom, rec["lights"], rec["with_env"], s["k"], rec["occlusion"], SEED, rec["pass_idx"], rec["offset"],
                             *[v[k] for k in VERTEX], cast=rec["cast"])
    live, floor = _live(rec, v), v["mat"] == n_b
    point = live & (want["lsel"] >= 0)
    assert np.array_equal(got["lsel"][live], want["lsel"][live])                       # exact
    for k in got:                                    # ended paths: not a byte moves; nor does anything but wl, lsel, emit (prim: read only)
        rows = ~live if k in ("wl", "lsel", "emit") else slice(None)
        assert got[k][rows].tobytes() == v[k][rows].tobytes(), k
    keep = live & (floor | ~point)     # floor rows and rows that picked the environment keep their cosine sample bit for bit
    assert _bytes_equal(got["wl"][keep], v["wl"][keep]) and (got["emit"][live & ~point] == 0).all()
    n_marginal = _cap(want["shadow"]["marginal"], point, MR.MARGINAL_CAP, "marginal shadow rays")
    with np.errstate(invalid="ignore"):
        horizon = point & ~(np.abs(want["cos"]) > 1e-5)                                # (a light within rounding of the horizon may go either way)
    assert horizon.sum() <= max(live.sum() // 1000, 1), int(horizon.sum())
    ok = point & ~want["shadow"]["marginal"] & ~horizon
    lit = (got["emit"] > 0).any(1)                                                     # (every intensity and reflectance is positive)
    flips = ok & (lit != want["lit"])
    turned = ok & ~floor
    e_wl = np.abs(got["wl"][turned] - want["wl"][turned]).max(initial=0.0)
    p999, worst = _shade_bound(got["emit"][ok], want["emit"][ok]) if ok.any() else (0.0, 0.0)
    print(f"  sample_emitter {s['k']}: {int(live.sum())} live rows, {int(point.sum())} picked a light, {n_marginal} shadow rays marginal, "
          f"{int(horizon.sum())} lights on the horizon, {int(flips.sum())} of the others decide visibility differently, "
          f"{int((turned & (want['wl'][:, 2] <= 0)).sum())} see their light below the horizon; wl {e_wl:.1e}; emit p99.9 {p999:.1e} max {worst:.1e}")
    assert not flips.any(), np.nonzero(flips)[0][:8]
    assert e_wl < 2e-5
    assert np.isfinite(got["emit"][live]).all() and p999 < 2e-4 and worst < 5e-3
    return want


def _reference_bounce(rec, s, dtype=np.float64, rr="own", cast="own"):
    v = s["before"]
    lit = rec["lit"]
    args = [v[k] for k in KEYS + ANSWERS] + [v.get("f_o") if rec["gt"] else None, v.get("f_l") if rec["gt"] else None]
    kw = dict(n_e=3 + int(rec["with_env"]), has_env=rec["with_env"], lsel=v["lsel"], emit=v["emit"]) if lit else {}
    env = rec["env"] if rec["with_env"] else np.zeros((2, 4, 3), np.float32)
    return MB.bounce(rec["geom"], env, "lit" if lit else "cosine", s["k"], s["args"]["last"], rec["occlusion"], SEED, rec["pass_idx"],
                     rec["offset"], *args, rr_depth=rec["rr"] if rr == "own" else rr, dtype=dtype,
                     cast=rec["cast"] if cast == "own" else cast, **kw)


def _check_bounce(rec, s, rr="own"):
    """test_mesh_bounce_matches_reference's assertions on one recorded bounce -> dict of what it counted."""
    geom, n_b, n = rec["geom"], rec["n_b"], rec["n"]
    meshes, inst = geom["meshes"], geom["instances"]
    rr_depth = rec["rr"] if rr == "own" else rr
    last, occlusion = s["args"]["last"], rec["occlusion"]
    v, got = s["before"], s["after"]
    want = _reference_bounce(rec, s, rr=rr)
    live = _live(rec, v)
    hit, shadow = want["hit"], want["shadow"]
    # the conditions on this bounce's own rays
    n_marginal = _cap(hit["marginal"] | shadow["marginal"], live, MR.MARGINAL_CAP, "marginal rays")
    et, eb = MR.fp32_restatement_error(meshes, inst, v["org"], want["d"], hit)
    nxt = MR.primary_arrays(meshes, inst, n_b, want["d"], hit, bary_tol=4 * eb)
    fragile = nxt["fragile"] & (hit["prim"][:, 0] >= 0)
    n_fragile = _cap(fragile, live, 0.03, "fragile next vertices")
    out = (f"  bounce {s['k']}{' (last)' if last else ''}: {int(live.sum())} live rows, {int((v['mat'] < n_b).sum())} material lanes, "
           f"{n_marginal} marginal, {n_fragile} fragile")
    # ended paths keep every byte, prim included; and the bounce writes nothing but the eight state arrays
    for k in KEYS:
        assert _bytes_equal(got[k][~live], v[k][~live]), k
    for k in got:
        if k not in KEYS:
            assert got[k].tobytes() == v[k].tobytes(), k
    ok = live & ~hit["marginal"] & ~shadow["marginal"] & ~fragile
    # the roulette decides alike wherever the variate is farther from q than fp32 moves q
    decided = np.ones(n, dtype=bool)
    if rr_depth is not None and not last and s["k"] + 1 >= rr_depth:
        q32 = _reference_bounce(rec, s, dtype=np.float32, rr=rr, cast=PR._no_rays)["q"]   # (q needs no ray)
        near, eq = PR.too_close_to_call(want, q32)
        decided = ~near
        out += (f"; roulette: {int(want['would'].sum())} decisions, {int(want['killed'].sum())} kills, fp32 error of q {eq:.3e}, "
                f"{int(near.sum())} too close to call")
        assert near.sum() <= max(live.sum() // 1000, 1)
    elif rr_depth is not None:
        assert not want["killed"].any()
    sure = ok & decided
    differ = sure & ((got["mat"] != want["material"]) | (got["prim"] != want["prim"]).any(1))
    out += f"; {int(differ.sum())} of {int(sure.sum())} sure rows decide differently"
    cont = sure & (want["material"] <= n_b)
    if last or not occlusion:
        print(out)
        assert not differ.any(), np.nonzero(differ)[0][:8]
        assert (got["mat"][live] == n_b + 1).all() and not cont.any()
    else:
        ids = np.bincount(want["material"][cont], minlength=n_b + 1)
        out += f", {int(cont.sum())} continue: ids {ids.tolist()}"
        if cont.any():
            t = want["t"][cont]
            # the kernel test's 4 et, plus what storing x + t d in fp32 costs whatever the error of t: the sum and the product
            # round once each, 2^-24 (|x| + t) each at the most.  Among the kernel test's 4096 rays there always is one whose
            # restated t is worse than that; a bounce at depth may serve ONE lane whose restated t happens to be exact.
            b_org = 4 * et + 2.0 ** -23 * (np.abs(v["org"][cont]).max(1) + t) / t
            r_org = (np.abs(got["org"][cont] - want["org"][cont]).max(1) / t / b_org).max()
            e_org = (np.abs(got["org"][cont] - want["org"][cont]).max(1) / t).max()
            tol_n = _tol_n(eb, nxt)
            e_nrm = np.abs(got["nrm"][cont] - want["nrm"][cont]).max()
            lanes, diffuse = cont & (want["material"] < n_b), cont & (want["material"] == n_b)
            e_wi = np.abs(got["wi"][lanes] - want["wi"][lanes]).max(initial=0.0)
            e_wl = np.abs(got["wl"][cont] - R.next_wl(SEED, rec["pass_idx"], s["k"], rec["offset"], n)[cont]).max()
            e_beta = np.abs(got["beta"][cont] - want["beta"][cont]).max()
            print(out + f"; org / t {e_org:.3e} (4 et = {4 * et:.3e}; largest error / bound {r_org:.2f}); nrm {e_nrm:.3e} (bound {tol_n:.3e}); wi {e_wi:.3e} "
                        f"(bound {4 * tol_n:.3e}); wl {e_wl:.3e}; beta {e_beta:.3e} (largest {np.abs(want['beta'][cont]).max():.3g})")
            assert not differ.any(), np.nonzero(differ)[0][:8]
            assert r_org <= 1.0
            assert e_nrm <= tol_n and e_wi <= 4 * tol_n
            assert np.array_equal(got["wi"][diffuse], want["wi"][diffuse].astype(np.float32))   # reflectances: exact
            assert e_wl < 2e-6 and e_beta < 2e-5
        else:
            print(out)
            assert not differ.any(), np.nonzero(differ)[0][:8]
    # rows that end keep the rest of their state, prim included
    ended = sure & ~cont
    for k in ("org", "nrm", "wi", "wl", "beta", "prim"):
        assert _bytes_equal(got[k][ended], v[k][ended]), k
    same = live & ~hit["marginal"] & ~shadow["marginal"] & (got["mat"] == want["material"]) & (got["prim"] == want["prim"]).all(1)
    p999, worst = _shade_bound(got["rad"][same], want["rad"][same]) if same.any() else (0.0, 0.0)
    print(f"    rad on the {int(same.sum())} rows that decide alike: p99.9 {p999:.2e} max {worst:.2e}")
    assert np.isfinite(got["rad"][live]).all() and p999 < 2e-4 and worst < 5e-3
    through = through_a_mesh(v["mat"], v["prim"], got["mat"], got["prim"], n_b) & sure
    mirrored = _live(rec, got) & (got["prim"][:, 0] == 2)
    return dict(want=want, through=int(through.sum()), mirrored=int(mirrored.sum()), kills=int(want["killed"].sum()) if "killed" in want else 0)


def _check_every_stage(rec, tag):
    print(f"{tag}:")
    _check_primary(rec)
    emitter = [_check_sample_emitter(rec, s) for s in _named(rec, "sample_emitter")]
    bounces = [_check_bounce(rec, s) for s in _named(rec, "bounce")]
    return emitter, bounces


@pytest.mark.parametrize("case", list(CASES))
def test_every_stage_matches_its_reference_on_the_device_input(case):
    lit, with_env, kind, depth, rr, _, pass_idx, _ = CASES[case]
    rec = _recorded(case)
    n_b = rec["n_b"]
    emitter, bounces = _check_every_stage(rec, f"case {case}")
    if lit:   # (not vacuous) every light is picked, lit and occluded rows occur at bounce 0
        s, want = _named(rec, "sample_emitter")[0], emitter[0]
        v = s["before"]
        open_ = MB.sample_emitter(rec["geom"], rec["lights"], with_env, 0, False, SEED, pass_idx, rec["offset"], *[v[k] for k in VERTEX])
        point = want["lsel"] >= 0
        picks = [int((want["lsel"] == j).sum()) for j in range(3)]
        n_lit, removed = int((point & want["lit"]).sum()), int((open_["lit"] & ~want["lit"]).sum())
        print(f"  bounce 0: rows per light {picks}, {n_lit} lit, occlusion removes {removed}")
        assert min(picks) >= 50 and n_lit >= 50 and removed >= 50
    stages = _named(rec, "bounce")
    first = stages[0]["before"]["mat"]
    rows = first.reshape(rec["rows"][1] - rec["rows"][0], -1)
    r0 = rec["rows"][0]
    assert set(np.unique(first).tolist()) == set(range(n_b + 2))              # (not vacuous) all four ids at bounce 0
    assert (rows[:SKY_ROWS[1] - r0] == n_b + 1).all() and (rows[FLOOR_ROWS[0] - r0:] == n_b).all()
    if len(stages) > 1:                                                      # floor -> material and material -> material at bounce 1
        second = stages[1]["before"]["mat"]
        assert ((first == n_b) & (second < n_b)).any() and ((first < n_b) & (second < n_b)).any()
    if rr is not None:
        assert sum(b["kills"] for b in bounces) >= 50
    print(f"  paths through a mesh per bounce {[b['through'] for b in bounces]}; live vertices on the mirrored instance after each "
          f"bounce {[b['mirrored'] for b in bounces]}")
    if depth != 1:
        assert sum(b["mirrored"] for b in bounces) >= 1                       # a mirrored instance reached by a secondary ray


def test_some_recorded_path_goes_through_a_mesh():
    """A BSDF sample above the shading normal but below the triangle's plane is followed into the closed mesh (README): in some
    bounce of the recorded passes a continuing row's next ``prim`` lies on the instance it started on, on another triangle."""
    count = {}
    for case in CASES:
        rec = _recorded(case)
        count[case] = [int(through_a_mesh(s["before"]["mat"], s["before"]["prim"], s["after"]["mat"], s["after"]["prim"], rec["n_b"]).sum())
                       for s in _named(rec, "bounce")]
    print(f"rows that go through a mesh, per case and bounce: {count}")
    assert sum(sum(c) for c in count.values()) >= 1


# ---- 4. the sampler's rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_sampler_rows_are_the_single_material_call_with_the_documented_key(case):
    rec = _recorded(case)
    r, n_b = rec["r"], rec["n_b"]
    table = r.table
    for s in _named(rec, "sample_pdf"):
        v, got = s["before"], s["after"]
        nomat = ~((v["mat"] >= 0) & (v["mat"] < n_b))
        assert nomat.any() and (got["wo"][nomat] == 0).all() and (got["pdf_o"][nomat] == 0).all() and (got["pdf_l"][nomat] == 0).all()
        key = PR.sampler_key(SEED, rec["pass_idx"], s["k"])
        for m in range(n_b):
            rows = np.flatnonzero(v["mat"] == m)
            if not len(rows):
                continue
            to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(r.device)
            wo, pdf_o, pdf_l = table.samplers[m].plugin_sample_pdf(to_dev(v["wi"][rows]), to_dev(v["wl"][rows]), None, T=table.T[m],
                                                                   variant=table.variant[m], seed=key, offset=rec["offset"],
                                                                   rng_index=to_dev(rows.astype(np.int64)))
            for name, t in (("wo", wo), ("pdf_o", pdf_o), ("pdf_l", pdf_l)):
                assert np.array_equal(t.cpu().numpy(), got[name][rows], equal_nan=True), (s["k"], m, name)
    served = sum(1 for s in _named(rec, "bounce") if (s["before"]["mat"] < n_b).any())
    assert len(_named(rec, "sample_pdf")) == served >= 1


# ---- 5. the evaluator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][2] == "analytic"])
def test_evaluator_answers_for_the_light_direction_the_emitter_stage_left(case):
    """f_o at (wi, wo) and f_l at (wi, wl) of the material rows, as the bounce finds them, against tests/principled_ref.py
    (bsdf_13) and tests/dielectric_ref.py (bsdf_24) in fp64 with tests/test_gpu_analytic_table.py's bound for ``eval_t`` — the
    same references in fp32 on the same rows are the yardstick, 4 x at p99 and at the maximum, each row's error relative within
    its own material — and NaN on every other row.  The tint of material m is float32(renderer's tint) * float32(ball albedo m),
    and ``wl`` is the one in the state when the evaluator ran: with lights that is the emitter stage's direction, not primary's."""
    rec = _recorded(case)
    r, n_b = rec["r"], rec["n_b"]
    models = [(PRI.reference(13, dtype=dt), D.RoughDielectric(0.3, dtype=dt)) for dt in (np.float64, np.float32)]
    tints = [tuple(float(c) for c in np.float32(r.plugin.albedo.numpy()) * np.float32(a)) for a in _world()["ball_albedo"]]
    got, yard = {"f_o": [], "f_l": []}, {"f_o": [], "f_l": []}
    evals = _named(rec, "eval_t")
    assert len(evals) == len(_named(rec, "sample_pdf")) >= 2
    moved = 0
    for s in evals:
        b = s["after"]
        bounce = next(t for t in _named(rec, "bounce") if t["k"] == s["k"])["before"]
        assert _bytes_equal(bounce["f_o"], b["f_o"]) and _bytes_equal(bounce["f_l"], b["f_l"])     # (what the bounce finds)
        nomat = ~((b["mat"] >= 0) & (b["mat"] < n_b))
        assert np.isnan(b["f_o"][nomat]).all() and np.isnan(b["f_l"][nomat]).all()
        for m in range(n_b):
            rows = b["mat"] == m
            if not rows.any():
                continue
            wi = b["wi"][rows]
            for name, d in (("f_o", b["wo"][rows]), ("f_l", b["wl"][rows])):
                g = b[name][rows]
                assert np.isfinite(g).all() and (g >= 0).all(), (s["k"], m, name)
                ref = models[0][m].eval(wi.astype(np.float64), d.astype(np.float64), tints[m])
                y = models[1][m].eval(wi, d, tints[m])
                got[name].append(_err(g, ref).max(1))
                yard[name].append(_err(y, ref).max(1))
        if s["k"] == 0:
            first = _named(rec, "primary")[0]["after"]["wl"]
            lanes = b["mat"] < n_b
            moved = int((np.abs(first[lanes] - b["wl"][lanes]).max(1) > 1e-3).sum())
    print(f"case {case}: {sum(len(a) for a in got['f_o'])} material rows over {len(evals)} bounces; the emitter stage moved wl on {moved} "
          f"material rows of bounce 0")
    _held_to_yardstick(f"case {case}", {q: np.concatenate(a) for q, a in got.items()}, {q: np.concatenate(a) for q, a in yard.items()})
    assert (moved >= 50) if rec["lit"] else (moved == 0)


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
def _check_end_to_end(rec, tag, fill=FILL):
    n, n_b, rows, gt = rec["n"], rec["n_b"], rec["rows"], rec["gt"]
    bounces = _named(rec, "bounce")
    names = ANSWERS + (("f_o", "f_l") if gt else ())
    answers = [{k: s["before"][k] for k in names} for s in bounces]
    ref = PR.reference_mesh_pass(rec["geom"], rec["cam_scene"], rec["env"], rec["lights"], rows[0], rows[1], SPP, SEED, rec["pass_idx"],
                                 rec["depth"], rec["occlusion"], answers, rr_depth=rec["rr"], cast=rec["cast"])
    history = [_codes(rec, _named(rec, "primary")[0]["after"])] + [_codes(rec, s["after"]) for s in bounces]
    differ = PR.histories_differ(history, ref["history"])
    n_marginal, n_fragile, n_close = (int(ref[k].sum()) for k in ("marginal", "fragile", "close"))
    final = _named(rec, "resolve")[0]
    rad = final["before"]["rad"]
    agree = ~differ & ~ref["marginal"]
    p999, worst = _shade_bound(rad[agree], ref["rad"][agree])
    film = final["film_after"].astype(np.float64)
    px = agree.reshape(-1, SPP).all(1)
    f999, fworst = _shade_bound((film - fill).reshape(-1, 3)[px], ref["film"].reshape(-1, 3)[px])
    print(f"{tag}: histories differ on {int(differ.sum())} of {n} paths ({int((differ & ~ref['marginal'] & ~ref['fragile'] & ~ref['close']).sum())} "
          f"of them neither marginal, fragile nor too close to call); {n_marginal} marginal, {n_fragile} fragile, {n_close} too close to call; "
          f"device depth {len(bounces)}, reference depth {ref['depth']}; {int(agree.sum())} paths compared: rad p99.9 {p999:.1e} max {worst:.1e}; "
          f"film on {int(px.sum())} pixels p99.9 {f999:.1e} max {fworst:.1e}")
    assert differ.sum() <= n // 1000
    assert n_marginal <= MR.MARGINAL_CAP * n and n_fragile <= 0.03 * n and n_close <= n // 1000
    assert np.isfinite(rad).all() and p999 < 2e-4 and worst < 5e-3
    assert f999 < 2e-4 and fworst < 5e-3
    assert (final["film_before"] == fill).all()
    want = fill + R.resolve(rad, SPP)
    assert np.abs(film.reshape(-1, 3) - want).max() < 1e-5 * max(1.0, want.max())
    assert ref["depth"] == len(bounces) and not ref["depth_cap_hit"]
    return ref, differ


@pytest.mark.parametrize("case", list(CASES))
def test_pass_matches_the_free_running_reference_pass(case):
    """``reference_mesh_pass`` in fp64 from the oracle's camera rays, with the recorded answers of the sampler and the evaluator:
    the same decision history — ids, checker colours and primitives — on all but 0.1 % of the paths; on the others that cast no
    marginal ray the final ``rad``, and on the pixels all of whose paths are such the film, inside the shade bound."""
    rec = _recorded(case)
    n_b = rec["n_b"]
    ref, differ = _check_end_to_end(rec, f"case {case}")
    first = PR.mesh_ids_of(ref["history"][0])
    assert set(np.unique(first).tolist()) == set(range(n_b + 2))
    if len(ref["history"]) > 2:
        second = PR.mesh_ids_of(ref["history"][1])
        assert ((first == n_b) & (second < n_b) & ~differ).any() and ((first < n_b) & (second < n_b) & ~differ).any()
    if rec["depth"] is None:            # for the unbounded pass the reference runs to the device's depth, and nothing is alive there
        assert not ((PR.mesh_ids_of(ref["history"][-1]) <= n_b) & ~differ).any()


# ---- 7. tiles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disk", "analytic"])
def test_tiles_are_the_rows_of_the_whole_film_bit_for_bit(kind):
    """Every draw of a pass is keyed by the global path index, so rows (0, 9), (9, 31), (31, 48) of a lit depth-3 render,
    concatenated, ARE the whole render.  The first tile sees only sky: its loop stops at the first bucketing.  The last sees only
    the floor at bounce 0: its first bounce serves no material lane, the sampler and the evaluator do not run, and the bounce must
    not read what they would have written — the tile rendered once more over answer buffers full of NaN is the same, bit for bit."""
    tiles = ((0, 9), (9, 31), (31, 48))
    assert tiles[0][1] <= SKY_ROWS[1] and tiles[2][0] >= FLOOR_ROWS[0]
    r = _make_renderer(True, True, kind, 3, None)
    whole = r.render(2, spp=SPP, seed=SEED)
    parts = [r.render(2, spp=SPP, seed=SEED, rows=rows) for rows in tiles]
    assert torch.isfinite(whole).all() and float(whole.mean()) > 0
    assert torch.equal(torch.cat(parts, 0), whole)
    gt = ["eval_t"] * (kind == "analytic")
    stages, stats, _ = _record_pass(r, tiles[0], 0)
    assert [s["name"] for s in stages] == ["primary", "path_begin", "sample_emitter", "bucket", "resolve"]
    assert stats["depth"] == 0 and stats["lanes_per_bounce"] == []
    n = (tiles[2][1] - tiles[2][0]) * W * SPP
    b = r._buffers(n)
    poisoned = [k for k in ANSWERS + ("f_o", "f_l") if k in b]
    assert len(poisoned) == (5 if kind == "analytic" else 3)
    for k in poisoned:
        b[k].fill_(float("nan"))
    stages, stats, _ = _record_pass(r, tiles[2], 0)
    names = [s["name"] for s in stages]
    assert names[:5] == ["primary", "path_begin", "sample_emitter", "bucket", "bounce"] and stats["lanes_per_bounce"][0] == 0
    assert names[5:9] == ["sample_emitter", "bucket", "sample_pdf"] + (gt or ["bounce"])[:1] and stats["lanes_per_bounce"][1] > 0
    first = next(s for s in stages if s["name"] == "bounce")["before"]
    assert all(np.isnan(first[k]).all() for k in poisoned)                      # (the first bounce did find them full of NaN)
    for k in poisoned:                                                            # once more, for render() itself
        r._buffers(n)[k].fill_(float("nan"))
    again = r.render(2, spp=SPP, seed=SEED, rows=tiles[2])
    assert torch.equal(again, parts[2])


# ---- 8. render() ---------------------------------------------------------------------------------------------------------------------
def test_render_is_the_mean_of_its_passes():
    """render(passes=2) = (pass 0 + pass 1) / 2 of two recorded passes of case a, bit for bit: the second pass is added to the film
    the first one left (resolve is ``film +=``), with pass indices 0 and 1 and nothing else changed."""
    r = _renderer("a")
    film = torch.zeros((H, W, 3), dtype=torch.float32, device=r.device)
    ends = []
    for pass_idx in (0, 1):
        with PR.Recorder(r) as rec:
            r.render_pass(film, 0, H, SPP, SEED, pass_idx)
        ends.append(rec.named("resolve")[0])
        assert rec.named("primary")[0]["args"]["pass_idx"] == pass_idx
        assert all(s["args"]["pass_idx"] == pass_idx for s in rec.named("bounce"))
    assert (ends[0]["film_before"] == 0).all() and np.array_equal(ends[0]["film_after"], ends[1]["film_before"])
    want = ends[1]["film_before"] + R.resolve(ends[1]["before"]["rad"], SPP).reshape(ends[1]["film_before"].shape)
    assert np.abs(ends[1]["film_after"] - want).max() < 1e-5 * max(1.0, want.max())
    assert not np.array_equal(ends[0]["before"]["rad"], ends[1]["before"]["rad"])
    both = r.render(2, spp=SPP, seed=SEED)
    assert torch.equal(both, film / 2) and float(both.mean()) > 0


# ---- the recorder on a mesh renderer ---------------------------------------------------------------------------------------------------
def test_recorder_wraps_the_mesh_stages_and_hands_their_keywords_on():
    """The Recorder wraps the methods ``MeshPathArrayRenderer`` overrides — its stages carry ``prim``, which only the mesh entry
    points write — records ``path_begin``, and hands ``lights=``, ``rows=``, ``env_dist=`` and ``rr_depth=`` on: a bounce called with
    ``rr_depth=1`` on a renderer that has none plays roulette, and is held to the reference with it.  Afterwards the class's
    methods are back."""
    r = _make_renderer(True, True, "disk", 4, None)
    rec = PR.Recorder(r)
    with rec:
        assert all(name in vars(r) for name in ("primary", "path_begin", "sample_emitter", "bounce", "resolve"))
        b = r.primary(0, H, SPP, SEED, 0)
        r.path_begin(b)
        r.sample_emitter(b, 0, SEED, 0, 0, occlusion=True, lights=None, rows=None)
        plan = r.table.bucket(b["mat"], extra_bins=2)
        b["wo"], b["pdf_o"], b["pdf_l"] = r.table.sample_pdf(plan, b["wi"], b["wl"], seed=PR.sampler_key(SEED, 0, 0), offset=0)
        r.bounce(b, 0, False, SEED, 0, 0, lights=None, env_dist=None, rr_depth=1, rows=None)
        torch.cuda.synchronize()
    assert not any(name in vars(r) for name in ("primary", "path_begin", "sample_emitter", "bounce", "resolve"))
    assert r.bounce.__func__ is M.MeshPathArrayRenderer.bounce and r.path_begin.__func__ is M.MeshPathArrayRenderer.path_begin
    names = [s["name"] for s in rec.stages]
    assert names == ["primary", "path_begin", "sample_emitter", "bucket", "sample_pdf", "bounce"]
    for s in rec.stages:
        s["k"] = 0
        assert "prim" in s["after"]
    emitter, bounce = rec.stages[2], rec.stages[5]
    assert emitter["args"]["occlusion"] is True and emitter["extra"] == dict(lights=None, rows=None)
    assert bounce["args"] == dict(bounce=0, last=False, seed=SEED, pass_idx=0, path_offset=0, occlusion=True)
    assert bounce["extra"] == dict(lights=None, env_dist=None, rr_depth=1, rows=None)
    begin = rec.stages[1]
    assert all(a.tobytes() == begin["after"][k].tobytes() for k, a in begin["before"].items())
    ctx = _context(r, (True, True, "disk", 4, None, None, 0, None), rec.stages, {}, (0, H), _world()["geom"])
    print("recorded by hand, bounce with rr_depth=1:")
    _check_sample_emitter(ctx, emitter)
    counted = _check_bounce(ctx, bounce, rr=1)
    assert counted["kills"] >= 50
    assert not _bytes_equal(bounce["before"]["prim"], bounce["after"]["prim"])


# ---- one case on the reference's own meshes ---------------------------------------------------------------------------------------------
SHELLS_SIZE = (32, 24)


@functools.lru_cache(maxsize=None)
def _recorded_shells():
    """tests/test_gpu_mesh_path.py's ``two_shells`` scene — two 57 152-triangle shells of the fixture scene and its 512-triangle
    plane — at SHELLS_SIZE, disk table, cosine, depth 2, pass 0; the hit source of every reference is ``mesh_ref.bvh_walk`` over
    the library's own BVHs (pinned to brute force on the CPU by test_bvh_walk_equals_brute_force_on_every_ray)."""
    dev()
    w, h = SHELLS_SIZE
    _, _, full, _ = M.mesh_scene_from_matpreview_xml(SCENE_FILE, MESH_FILE, w, h)
    shells = [i for i in full.instances if i.material is not None][:2]
    plane = next(i for i in full.instances if i.checker is not None)
    inst = [M.Instance(s.mesh, s.to_world, material=k) for k, s in enumerate(shells)] + [plane]
    scene = M.MeshScene(full.meshes, inst)
    geom = dict(meshes=full.meshes, instances=inst, n_materials=2, albedo=[0.9, 0.6, 0.3])
    bvhs = [scene.bvh(k) for k in range(len(full.meshes))]
    cast = lambda meshes, instances, org, d, tmax=None, skip=None: MR.bvh_walk(meshes, instances, bvhs, org, d, tmax=tmax, skip=skip)
    cam = WF.Camera(origin=(1.0, 1.05, -1.5), target=(-3.5, 0.75, -1.5), fov_deg=40.0, width=w, height=h)
    case = (False, True, "disk", 2, None, None, 0, None)
    r = _make_renderer(*case[:5], geom=geom, scene=scene, camera=cam)
    stages, stats, _ = _record_pass(r, (0, h), 0)
    return _context(r, case, stages, stats, (0, h), geom, cast=cast)


def test_two_shells_pass_matches_its_references():
    """The stage order, tests 2, 3 and 6 on the reference's own meshes at 32 x 24 x 2 spp = 1 536 paths, the largest of 32 x 24,
    24 x 16 and 16 x 12: one fp64 ``reference_mesh_pass`` through ``bvh_walk`` takes 0.72 / 0.87 / 1.08 s on the CPU at
    16 x 12 / 24 x 16 / 32 x 24 (the walk advances all rays of a mesh together, so its cost hardly depends on their number), and
    the whole test — the recorded pass, the walks of the stage checks and that pass — 1.2 s on the MI355X machine's CPU."""
    rec = _recorded_shells()
    _check_order_and_arguments(rec, "two shells")
    _check_no_writes_between_stages(rec)
    _check_every_stage(rec, "two shells")
    ref, differ = _check_end_to_end(rec, "two shells")
    first = PR.mesh_ids_of(ref["history"][0])
    assert set(np.unique(first).tolist()) == set(range(rec["n_b"] + 2))
