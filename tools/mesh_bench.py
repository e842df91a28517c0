"""Cost of the mesh ray caster (csrc/mesh.hip, bsdf_diffusion_sampling_amd/mesh.py) -> profiles/mesh.json.

Workload: the fixture scene (tests/golden/disney_bsdf_array2_spherical_envmap.xml on tests/golden/matpreview.serialized: 25
instances, 12 shells of 57 152 triangles) at 683x512, 4 spp.  Every timing is the median over interleaved rounds in one process
(each variant once per round, ``--reps`` launches per timing, ending in a device synchronise).  Recorded:

* ``primary``: bsdfd_mesh_primary in Mrays/s, next to bsdfd_wf_primary on the twelve-sphere scene of the same file;
* ``intersect`` / ``occluded`` on the primary rays, and on cosine-distributed secondary rays leaving the hit points (skip = the
  triangle they start on);
* nodes loaded and triangles tested per ray, mean and p99, from a COUNTING build of csrc/mesh.hip (-DBSDFD_MESH_COUNT, compiled
  by this tool into a library of its own, never the product);
* the host's BVH build time per mesh; a ``MeshArrayRenderer`` pass against an ``ArrayRenderer`` pass (same table, proxy shading);
* the fp32 error figures tests/test_gpu_mesh.py takes its bounds from (tests/mesh_ref.py: the kernel's formulas restated in numpy
  fp32 against fp64, on that file's own cases);
* VGPRs, scratch and occupancy per kernel, from the metadata of a compilation of csrc/mesh.hip.

``--path`` measures the path tracer on meshes instead (``mesh.MeshPathArrayRenderer``) -> profiles/mesh_path.json: a pass at
max_depth 1 (with and without occlusion), 2, 4 and unbounded with rr_depth = 5, next to the ``MeshArrayRenderer`` pass and to the
sphere ``PathArrayRenderer`` at the same depths (variants alternate in one process, medians over the rounds, a host clock that
ends in a synchronise); and, per bounce of the unbounded pass, the ``bounce`` launch between two device events with that bounce's
live-lane count, next to ``MeshScene.intersect`` plus ``occluded`` on the same rays — the continuation rays and the cosine
strategy's shadow rays the fused kernel walks — which is the yardstick for what the fusion costs or saves.

``--path --compact`` measures the live-lane list on meshes (``mesh.CompactMeshPathArrayRenderer``) -> profiles/mesh_path_compact.json,
by the protocol of ``--path``: a pass at max_depth 1, 2 and 4 and unbounded with rr_depth = 5 of the plain ``MeshPathArrayRenderer``
and of the compact one, the two alternating within every round of one process; the medians, the difference round by round with its
spread, whether the two films are equal byte for byte; and, per bounce of the unbounded pass, the ``bounce`` launch of either
renderer between two device events, with the lanes alive, the list's length and the lanes the list form is launched over.

Nothing here is a gate.  The record is there to decide whether an ordered traversal with a stack in LDS, or a wider node, is
worth a change of its own, and what a bounce of the path tracer on meshes will cost.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from bsdf_diffusion_sampling_amd import _lib, mesh as M
from bsdf_diffusion_sampling_amd import wavefront as WF
from bsdf_diffusion_sampling_amd.materials import MaterialTable

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=683); ap.add_argument("--height", type=int, default=512)
ap.add_argument("--spp", type=int, default=4); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "disney_bsdf_array2_spherical_envmap.xml"))
ap.add_argument("--mesh-file", default=os.path.join(ROOT, "tests", "golden", "matpreview.serialized"))
ap.add_argument("--no-counting", action="store_true", help="skip the counting build (needs hipcc)")
ap.add_argument("--no-errors", action="store_true", help="skip the fp32 error figures (a minute of numpy brute force)")
ap.add_argument("--path", action="store_true", help="measure the path tracer on meshes instead -> profiles/mesh_path.json")
ap.add_argument("--compact", action="store_true",
                help="with --path: the live-lane list (mesh.CompactMeshPathArrayRenderer) against the plain renderer -> "
                     "profiles/mesh_path_compact.json")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.compact and not a.path:
    ap.error("--compact needs --path")
a.out = a.out or os.path.join(ROOT, "profiles", "mesh_path_compact.json" if a.compact else "mesh_path.json" if a.path else "mesh.json")
if not torch.cuda.is_available():
    sys.exit("tools/mesh_bench.py measures on the GPU: no device visible")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
L = _lib.lib()
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

names, cam, scene, albedo = M.mesh_scene_from_matpreview_xml(a.scene, a.mesh_file, a.width, a.height)
table = MaterialTable([m + "_spherical" if m.startswith("bsdf_") else m + "_disk" for m in names])
_, cam_s, centers, radii = WF.scene_from_matpreview_xml(a.scene, a.width, a.height)
mesh_r = M.MeshArrayRenderer(table, scene, camera=cam)
sphere_r = WF.ArrayRenderer(table, centers, radii, camera=cam_s)
n = a.width * a.height * a.spp
rec = {"workload": f"{os.path.basename(a.scene)} {a.width}x{a.height}x{a.spp}", "rays": n, "rounds": a.rounds, "reps": a.reps,
       "device": torch.cuda.get_device_name(dev), "library": L.bsdfd_version().decode(), "bvh": scene.stats}



def median_ms(variants, rounds, reps, keep=False):
    """{name: ms} -> medians over interleaved rounds: each variant once per round, ``reps`` calls per timing, a synchronise at the end.
    ``keep``: every round's figure as well ("rounds_ms")."""
    times = {k: [] for k in variants}
    for fn in variants.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / reps)
    return {k: dict({"ms": 1e3 * float(np.median(v)), "ms_min": 1e3 * min(v), "ms_max": 1e3 * max(v)},
                    **({"rounds_ms": [1e3 * x for x in v]} if keep else {})) for k, v in times.items()}


def measure_paths():
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    cfgs = {"depth1": dict(max_depth=1, occlusion=False), "depth1_occlusion": dict(max_depth=1, occlusion=True),
            "depth2": dict(max_depth=2), "depth4": dict(max_depth=4), "unbounded_rr5": dict(max_depth=None, rr_depth=5)}
    mesh_p = {k: M.MeshPathArrayRenderer(table, scene, camera=cam, **kw) for k, kw in cfgs.items()}
    sphere_p = {k: PathArrayRenderer(table, centers, radii, camera=cam_s, **kw) for k, kw in cfgs.items()}
    films = {}

    def one_pass(r):
        film = films.setdefault(id(r), torch.zeros((a.height, a.width, 3), device=dev))
        return lambda: r.render_pass(film, 0, a.height, a.spp, 0, 0)
    variants = {"mesh_array_renderer_pass": one_pass(mesh_r), "array_renderer_pass_spheres": one_pass(sphere_r)}
    variants.update({"mesh_path_" + k: one_pass(r) for k, r in mesh_p.items()})
    variants.update({"sphere_path_" + k: one_pass(r) for k, r in sphere_p.items()})
    rec["pass_ms"] = median_ms(variants, a.rounds, a.reps)
    rec["lanes_per_bounce"] = {k: r.stats["lanes_per_bounce"] for k, r in mesh_p.items()}
    rec["lanes_per_bounce_spheres"] = {k: r.stats["lanes_per_bounce"] for k, r in sphere_p.items()}
    # ---- per bounce of the unbounded pass: the launch between two device events, the live lanes, and the rays it walks ----
    r = mesh_p["unbounded_rr5"]
    n_b, inner = len(table), r.bounce
    per, rays, capture = [], [], [True]

    def timed(b, k, *args, **kwargs):
        if capture[0]:   # first instrumented pass only: the rays of this bounce, as the kernel forms them
            mat, nv = b["mat"], b["nrm"]
            live, floor = mat <= n_b, mat == n_b
            sign = torch.copysign(torch.ones_like(nv[:, 2]), nv[:, 2])
            aa = -1.0 / (sign + nv[:, 2]); bb = nv[:, 0] * nv[:, 1] * aa
            fs = torch.stack([1.0 + sign * nv[:, 0] ** 2 * aa, sign * bb, -sign * nv[:, 0]], 1)
            ft = torch.stack([bb, sign + nv[:, 1] ** 2 * aa, -nv[:, 1]], 1)
            world = lambda v: v[:, 0:1] * fs + v[:, 1:2] * ft + v[:, 2:3] * nv
            ball = live & ~floor
            follow = ball & torch.isfinite(b["pdf_o"]) & (b["pdf_o"] > 0) & (b["wo"][:, 2] > 0)
            ask = floor | follow
            shadow = ball & torch.isfinite(b["pdf_l"]) & (b["pdf_l"] > 0) & (b["wl"][:, 2] > 0)
            dc = torch.where(floor[:, None], world(b["wl"]), world(b["wo"]))
            rays.append(dict(live=int(live.sum()), material_lanes=int(ball.sum()),
                             closest=(b["org"][ask].contiguous(), dc[ask].contiguous(), b["prim"][ask].contiguous()),
                             shadow=(b["org"][shadow].contiguous(), world(b["wl"])[shadow].contiguous(), b["prim"][shadow].contiguous())))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(b, k, *args, **kwargs)
        e1.record()
        per[-1].append((e0, e1))
    r.bounce = timed
    film = torch.zeros((a.height, a.width, 3), device=dev)
    for _ in range(a.rounds):
        per.append([])
        r.render_pass(film, 0, a.height, a.spp, 0, 0)
        torch.cuda.synchronize()
        per[-1] = [e0.elapsed_time(e1) for e0, e1 in per[-1]]
        capture[0] = False
    r.bounce = inner
    depth = len(per[0])
    assert all(len(p) == depth for p in per)   # (the same seed and pass: the same paths)
    bounces = []
    for k in range(depth):
        row = {"bounce": k, "live_lanes": rays[k]["live"], "material_lanes": rays[k]["material_lanes"],
               "closest_hit_rays": int(rays[k]["closest"][0].shape[0]), "shadow_rays": int(rays[k]["shadow"][0].shape[0]),
               "fused_bounce_ms": float(np.median([p[k] for p in per]))}
        if k < 6:   # the unfused pair on the same rays
            (o1, d1, s1), (o2, d2, s2) = rays[k]["closest"], rays[k]["shadow"]
            pair = {}
            if o1.shape[0]:
                pair["intersect"] = lambda: scene.intersect(o1, d1, None, s1)
            if o2.shape[0]:
                pair["occluded"] = lambda: scene.occluded(o2, d2, None, s2)
            got = median_ms(pair, a.rounds, a.reps)
            row["intersect_ms"] = got.get("intersect", {"ms": 0.0})["ms"]
            row["occluded_ms"] = got.get("occluded", {"ms": 0.0})["ms"]
        bounces.append(row)
    rec["bounces_unbounded_rr5"] = bounces
    rec["depth_unbounded_rr5"] = depth


def measure_compact():
    """The live-lane list on meshes: ``CompactMeshPathArrayRenderer`` against the plain ``MeshPathArrayRenderer`` (the yardstick) in
    one process, the two alternating within every round."""
    cfgs = {"depth1": dict(max_depth=1, occlusion=True), "depth2": dict(max_depth=2), "depth4": dict(max_depth=4),
            "unbounded_rr5": dict(max_depth=None, rr_depth=5)}
    plain = {k: M.MeshPathArrayRenderer(table, scene, camera=cam, **kw) for k, kw in cfgs.items()}
    comp = {k: M.CompactMeshPathArrayRenderer(table, scene, camera=cam, **kw) for k, kw in cfgs.items()}
    films = {}

    def one_pass(r):
        film = films.setdefault(id(r), torch.zeros((a.height, a.width, 3), device=dev))
        return lambda: r.render_pass(film, 0, a.height, a.spp, 0, 0)
    variants = {}
    for k in cfgs:
        variants["plain_" + k], variants["compact_" + k] = one_pass(plain[k]), one_pass(comp[k])
    got = median_ms(variants, a.rounds, a.reps, keep=True)
    rec["pass_ms"] = {k: {x: y for x, y in v.items() if x != "rounds_ms"} for k, v in got.items()}
    rec["plain_minus_compact_ms"] = {}
    for k in cfgs:   # the difference round by round (the two ran back to back in it), its median and its spread
        d = [p - c for p, c in zip(got["plain_" + k]["rounds_ms"], got["compact_" + k]["rounds_ms"])]
        rec["plain_minus_compact_ms"][k] = {"median": float(np.median(d)), "min": min(d), "max": max(d),
                                            "ratio_of_medians": got["plain_" + k]["ms"] / got["compact_" + k]["ms"]}
    # the same film: one pass of each into a fresh film, compared byte for byte
    rec["films_equal"] = {}
    for k in cfgs:
        fp, fc = (torch.zeros((a.height, a.width, 3), device=dev) for _ in range(2))
        plain[k].render_pass(fp, 0, a.height, a.spp, 0, 0)
        comp[k].render_pass(fc, 0, a.height, a.spp, 0, 0)
        torch.cuda.synchronize()
        rec["films_equal"][k] = bool(torch.equal(fp.view(torch.int32), fc.view(torch.int32)))
    rec["lanes_per_bounce"] = {k: r.stats["lanes_per_bounce"] for k, r in plain.items()}
    rec["list_per_bounce"] = {k: r.stats["list_per_bounce"] for k, r in comp.items()}
    # ---- per bounce of the unbounded pass: the bounce launch of either renderer between two device events ----
    rp, rc = plain["unbounded_rr5"], comp["unbounded_rr5"]
    n_b = len(table)
    live, launched, per = [], [], {"plain": [], "compact": []}

    def instrument(r, name, count):
        inner = r.bounce

        def timed(b, k, *args, **kwargs):
            if count:   # the untimed first pass: the lanes alive entering this bounce
                live.append(int((b["mat"] <= n_b).sum()))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inner(b, k, *args, **kwargs)
            e1.record()
            per[name][-1].append((e0, e1))
            if name == "compact" and len(per[name]) == 1:   # the lanes this launch is given: the list without its ended paths
                launched.append(n if kwargs.get("rows") is None else int(kwargs["rows"].shape[0]))
        r.bounce = timed
        return inner
    film = torch.zeros((a.height, a.width, 3), device=dev)
    inner_p = instrument(rp, "plain", True)
    per["plain"].append([])
    rp.render_pass(film, 0, a.height, a.spp, 0, 0)
    torch.cuda.synchronize()
    per["plain"].clear()
    rp.bounce = inner_p
    inner_p, inner_c = instrument(rp, "plain", False), instrument(rc, "compact", False)
    for _ in range(a.rounds):
        for name, r in (("plain", rp), ("compact", rc)):
            per[name].append([])
            r.render_pass(film, 0, a.height, a.spp, 0, 0)
            torch.cuda.synchronize()
            per[name][-1] = [e0.elapsed_time(e1) for e0, e1 in per[name][-1]]
    rp.bounce, rc.bounce = inner_p, inner_c
    depth = len(live)
    assert all(len(p) == depth for v in per.values() for p in v)   # (the same seed and pass: the same paths)
    lists = rc.stats["list_per_bounce"]
    rec["bounces_unbounded_rr5"] = [
        {"bounce": k, "live_lanes": live[k], "list_length": lists[k], "lanes_launched": launched[k],
         "full_width_bounce_ms": float(np.median([p[k] for p in per["plain"]])),
         "list_bounce_ms": float(np.median([p[k] for p in per["compact"]])),
         "list_bounce_ms_min": min(p[k] for p in per["compact"]), "list_bounce_ms_max": max(p[k] for p in per["compact"])}
        for k in range(depth)]
    rec["depth_unbounded_rr5"] = depth
    rec["bounce_launches_ms"] = {name: float(np.median([sum(p) for p in v])) for name, v in per.items()}


if a.path:
    measure_compact() if a.compact else measure_paths()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("pass_ms", "plain_minus_compact_ms", "films_equal", "bounce_launches_ms",
                                          "bounces_unbounded_rr5") if k in rec}))
    sys.exit(0)

# ---- BVH build time per mesh (host) ----
for k, m in enumerate(scene.meshes):
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); M.build_bvh(m); ts.append(time.perf_counter() - t0)
    rec["bvh"][k]["build_ms"] = 1e3 * float(np.median(ts))

# ---- the rays ----
b = mesh_r.primary(0, a.height, a.spp, 0, 0)
org = torch.tensor(cam.origin, dtype=torch.float32, device=dev).repeat(n, 1).contiguous()
d = b["dir"].clone()
t, prim, bary = scene.intersect(org, d)
hit = t < M.NOTHING
# secondary rays: from the hit points along the cosine sample wl in the frame of the shading normal (wf_dev::onb), hits only
nv, wl = b["nrm"][hit], b["wl"][hit]
sign = torch.copysign(torch.ones_like(nv[:, 2]), nv[:, 2])
aa = -1.0 / (sign + nv[:, 2]); bb = nv[:, 0] * nv[:, 1] * aa
fs = torch.stack([1.0 + sign * nv[:, 0] ** 2 * aa, sign * bb, -sign * nv[:, 0]], 1)
ft = torch.stack([bb, sign + nv[:, 1] ** 2 * aa, -nv[:, 1]], 1)
org2 = (org[hit] + t[hit, None] * d[hit]).contiguous()
d2 = (wl[:, 0:1] * fs + wl[:, 1:2] * ft + wl[:, 2:3] * nv).contiguous()
skip2 = prim[hit].contiguous()
n2 = org2.shape[0]
rec["hit_fraction"] = float(hit.float().mean())
rec["secondary_rays"] = n2
rec["secondary_occluded_fraction"] = float(scene.occluded(org2, d2, None, skip2).float().mean())

film_m = torch.zeros((a.height, a.width, 3), device=dev)
film_s = torch.zeros((a.height, a.width, 3), device=dev)
variants = {
    "mesh_primary": (n, lambda: mesh_r.primary(0, a.height, a.spp, 0, 0)),
    "wf_primary_spheres": (n, lambda: sphere_r.primary(0, a.height, a.spp, 0, 0)),
    "intersect_primary_rays": (n, lambda: scene.intersect(org, d)),
    "occluded_primary_rays": (n, lambda: scene.occluded(org, d)),
    "intersect_secondary_rays": (n2, lambda: scene.intersect(org2, d2, None, skip2)),
    "occluded_secondary_rays": (n2, lambda: scene.occluded(org2, d2, None, skip2)),
    "mesh_array_renderer_pass": (n, lambda: mesh_r.render_pass(film_m, 0, a.height, a.spp, 0, 0)),
    "array_renderer_pass_spheres": (n, lambda: sphere_r.render_pass(film_s, 0, a.height, a.spp, 0, 0)),
}
times = {k: [] for k in variants}
for k, (_, fn) in variants.items():   # warm-up
    fn()
torch.cuda.synchronize()
for _ in range(a.rounds):
    for k, (_, fn) in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / a.reps)
rec["timings"] = {k: {"ms": 1e3 * float(np.median(v)), "ms_min": 1e3 * min(v), "ms_max": 1e3 * max(v),
                      "Mrays_per_s": variants[k][0] / float(np.median(v)) / 1e6} for k, v in times.items()}

# ---- kernel metadata, and the counting build ----
src = os.path.join(os.path.dirname(_lib.SRC_PATH), "mesh.hip")
with tempfile.TemporaryDirectory(prefix="mesh_bench_") as td:
    try:
        subprocess.run(["hipcc", *_lib.HIPCC_FLAGS, "-save-temps=obj", "-I", _lib.INCLUDE_DIR, "-c", src, "-o", os.path.join(td, "mesh.o")],
                       check=True, cwd=td)
        asm = open(next(os.path.join(td, f) for f in os.listdir(td) if f.endswith(".s") and "gfx950" in f)).read()
        kernels = {}
        for blk in asm.split("- .agpr_count:")[1:]:
            get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            vg = get("vgpr_count")
            kernels[re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", name).split("E")[0]] = {
                "vgprs": vg, "sgprs": get("sgpr_count"), "scratch_bytes": get("private_segment_fixed_size"),
                "waves_per_simd": min(8, 512 // (8 * ((vg + 7) // 8)))}
        rec["kernels"] = kernels
        if not a.no_counting:
            stub = os.path.join(td, "stub.cpp")
            open(stub, "w").write('#include <string>\nint bsdfd_fail_(int code, const std::string&) { return code; }\n')
            so = os.path.join(td, "libmeshcount.so")
            subprocess.run(["hipcc", *_lib.HIPCC_FLAGS, "-DBSDFD_MESH_COUNT", "-I", _lib.INCLUDE_DIR, "-shared", src, stub, "-o", so],
                           check=True, cwd=td)
            LC = C.CDLL(so)
            LC.bsdfd_mesh_scene_create.argtypes = L.bsdfd_mesh_scene_create.argtypes
            LC.bsdfd_mesh_scene_destroy.argtypes = L.bsdfd_mesh_scene_destroy.argtypes
            LC.bsdfd_mesh_scene_destroy.restype = None
            LC.bsdfd_mesh_intersect.argtypes = L.bsdfd_mesh_intersect.argtypes
            descs, recs = scene._records()
            h = C.c_void_p()
            assert LC.bsdfd_mesh_scene_create(descs, len(scene.meshes), recs, len(scene.instances), C.byref(h)) == 0
            counts = {}
            for label, (o_, d_, s_) in {"primary_rays": (org, d, None), "secondary_rays": (org2, d2, skip2)}.items():
                m_ = o_.shape[0]
                tt = torch.empty(m_, device=dev); pp = torch.empty((m_, 2), dtype=torch.int32, device=dev)
                cc = torch.empty((m_, 2), device=dev)
                assert LC.bsdfd_mesh_intersect(h, m_, ptr(o_), ptr(d_), None, ptr(s_), ptr(tt), ptr(pp), ptr(cc), None) == 0
                torch.cuda.synchronize()
                c = cc.cpu().numpy()
                counts[label] = {"nodes_mean": float(c[:, 0].mean()), "nodes_p99": float(np.percentile(c[:, 0], 99)),
                                 "triangles_mean": float(c[:, 1].mean()), "triangles_p99": float(np.percentile(c[:, 1], 99))}
            LC.bsdfd_mesh_scene_destroy(h)
            rec["visited_per_ray_closest_hit"] = counts
    except (OSError, subprocess.CalledProcessError, StopIteration) as exc:
        rec["kernels_error"] = f"{type(exc).__name__}: {exc}"

# ---- the fp32 error figures of the tests ----
if not a.no_errors:
    import mesh_ref as R
    shapes = M.load_serialized(a.mesh_file)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    one = M.TriMesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    pos5 = [[0, 0, 0]] + [[np.cos(x), np.sin(x), 0.1 * k] for k, x in enumerate(np.linspace(0, 2.5, 6))]
    five = M.TriMesh(pos5, [[0, k + 1, k + 2] for k in range(5)])
    cases = {"one": ([one], [M.Instance(0, eye, diffuse=0.5)]), "five": ([five], [M.Instance(0, eye, diffuse=0.5)]),
             "plane": ([shapes[0]], [M.Instance(0, eye, diffuse=0.5)]),
             "interior3": ([shapes[1]], [M.Instance(0, t_, diffuse=0.18) for t_ in R.transforms()])}
    errs = {}
    for k, (name, (meshes, inst)) in enumerate(cases.items()):   # tests/test_gpu_mesh.py: case()
        boxes = [(lo - 0.05 * np.linalg.norm(hi - lo), hi + 0.05 * np.linalg.norm(hi - lo)) for lo, hi in R.instance_boxes(meshes, inst)]
        o_, d_ = R.rays_at(boxes, 4099, seed=20 + k)
        ref = R.brute_force(meshes, inst, o_, d_)
        et, eb = R.fp32_restatement_error(meshes, inst, o_, d_, ref)
        errs[name] = {"t_rel": et, "bary_abs": eb, "marginal": int(ref["marginal"].sum()), "hits": int((ref["t"] < R.NOTHING).sum())}
    o_, d_ = org[::a.spp * 37].cpu().numpy(), d[::a.spp * 37].cpu().numpy()
    ref = R.bvh_walk(scene.meshes, scene.instances, [scene.bvh(k) for k in range(len(scene.meshes))], o_, d_)
    et, eb = R.fp32_restatement_error(scene.meshes, scene.instances, o_, d_, ref)
    errs["fixture_scene_primary_rays"] = {"t_rel": et, "bary_abs": eb, "marginal": int(ref["marginal"].sum()), "rays": int(o_.shape[0])}
    rec["fp32_restatement_error"] = errs

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps({k: rec[k] for k in ("timings", "kernels", "visited_per_ray_closest_hit") if k in rec}))
