"""A/B of the ANALYTIC ground truth of a mixed-material wavefront: ONE launch on the lane-ordered arrays (analytic.AnalyticTable,
csrc/analytic_table.hip) against the per-material loop it replaces (gathered copies, two single-material eval_t launches per
material, NaN fills, indexed scatter: what ArrayRenderer does with fused_ground_truth=False).  Writes profiles/analytic_table.json.

  eval alone     ~1 Mi rows; 12 materials (the ids of matpreview/disney_bsdf_array2_spherical_envmap.xml: 21, 20, 20, 1, 19, 4, 25,
                 7, 24, 12, 13, 14) and all 26 of the reference's list; image-coherent ids (the primary rays of a scene with that
                 many balls — floor hits and misses among them, which have no ground truth) and ids drawn per lane
  sample / pdf   AnalyticTable.sample_t and pdf_t on the same rows (no loop to compare with: recorded as they are)
  render pass    that 12-ball scene, 683x512, 4 spp: ArrayRenderer.render_pass with the table, with the loop and without ground
                 truth; a depth-4 PathArrayRenderer pass with the table and without ground truth

The paths of a comparison run in the same process in interleaved rounds, each round timed with device events around several
repetitions; the record keeps every round (tools/measured_table_bench.py: the same routine).  The loop is timed as a lane-order
caller pays for it: the stable sort of the ids is NOT included, the gathers, the launches, the fills and the scatter are.  The two
paths' outputs are compared bit for bit before anything is timed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402
from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, reference_bsdf  # noqa: E402
from bsdf_diffusion_sampling_amd.materials import MaterialTable  # noqa: E402
from tools.measured_table_bench import summary, time_rounds, verdict  # noqa: E402

ARRAY2_IDX = (21, 20, 20, 1, 19, 4, 25, 7, 24, 12, 13, 14)
TINT = (0.9, 0.8, 0.7)


def sphere_dirs(g, n):
    v = g.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def net_of(idx):
    """A shipped full-sphere net for ball ``idx`` (bsdf_2 ships none: its neighbour's stands in — the nets only place the rays)."""
    return f"bsdf_{3 if idx == 2 else idx}_spherical"


def scene_of(n_balls, width, height):
    """(camera, centres, radii): the array0 scene for 12 balls, else rows of nine balls on the same floor under the same camera
    direction."""
    cam, centers, radii = WF.array0_scene(width, height)
    if n_balls == 12:
        return cam, centers, radii
    centers = [(-5.2 + 0.8 * (k % 9), 0.33, -0.9 - 0.9 * (k // 9)) for k in range(n_balls)]
    cx, cz = sum(c[0] for c in centers) / n_balls, sum(c[2] for c in centers) / n_balls
    cam = WF.Camera(origin=cam.origin, target=(cx, 0.33, cz), up=cam.up, fov_deg=cam.fov_deg * 1.5, width=width, height=height)
    return cam, centers, [0.33] * n_balls


def coherent_ids(idx, width, height, spp):
    """The material ids of the primary rays of a scene with one ball per entry of ``idx``."""
    cam, centers, radii = scene_of(len(idx), width, height)
    r = WF.ArrayRenderer(MaterialTable([net_of(i) for i in idx]), centers, radii, camera=cam)
    return r.primary(0, height, spp, 0, 0)["mat"].clone()


def bench_eval(idx, ids_kind, width, height, spp, rounds, reps):
    mats = [reference_bsdf(i) for i in idx]
    n_mat = len(mats)
    dev = torch.device("cuda")
    if ids_kind == "coherent":
        ids = coherent_ids(idx, width, height, spp)
    else:
        ids = torch.from_numpy(np.random.default_rng(n_mat).integers(0, n_mat, size=width * height * spp).astype(np.int64)).to(dev)
    n = ids.shape[0]
    g = np.random.default_rng(n_mat + 100)
    wi, wo, wl = (torch.from_numpy(sphere_dirs(g, n)).to(dev) for _ in range(3))
    u = torch.from_numpy(g.random((n, 3)).astype(np.float32)).to(dev)
    table = AnalyticTable(mats)
    rows = torch.sort(ids, stable=True).indices
    seg_end = torch.cumsum(torch.bincount(ids, minlength=n_mat)[:n_mat], 0).tolist()
    n_gt = seg_end[-1]
    f_o, f_l, g_o, g_l = (torch.empty_like(wi) for _ in range(4))
    s_out = (torch.empty_like(wi), torch.empty(n, dtype=torch.float32, device=dev), torch.empty_like(wi))
    p_out = torch.empty(n, dtype=torch.float32, device=dev)

    def fused():
        table.eval_t(ids, wi, wo, wl, tint=TINT, out_o=f_o, out_l=f_l)

    def loop():
        wi_s, wo_s, wl_s = wi[rows], wo[rows], wl[rows]
        fo_s = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        fl_s = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        lo = 0
        for m, hi in enumerate(seg_end):
            if hi > lo:
                mats[m].eval_t(wi_s[lo:hi], wo_s[lo:hi], out=fo_s[lo:hi], tint=TINT)
                mats[m].eval_t(wi_s[lo:hi], wl_s[lo:hi], out=fl_s[lo:hi], tint=TINT)
            lo = hi
        g_o.fill_(float("nan"))
        g_l.fill_(float("nan"))
        g_o[rows] = fo_s
        g_l[rows] = fl_s

    fused(), loop()
    torch.cuda.synchronize()
    same = torch.equal(f_o.view(torch.int32), g_o.view(torch.int32)) and torch.equal(f_l.view(torch.int32), g_l.view(torch.int32))
    if not same:
        raise SystemExit(f"eval {n_mat} materials, {ids_kind} ids: the fused and the loop results differ")
    s = summary(time_rounds({"fused": fused, "loop": loop}, rounds, reps))
    own = summary(time_rounds({"sample_t": lambda: table.sample_t(ids, wi, u, tint=TINT, out=s_out),
                               "pdf_t": lambda: table.pdf_t(ids, wi, wo, out=p_out)}, rounds, reps))
    return {"what": "eval alone", "rows": n, "rows_with_ground_truth": n_gt, "materials": n_mat, "ids": ids_kind,
            "launches": {"fused": 1, "loop": 2 * sum(1 for a, b in zip([0] + seg_end, seg_end) if b > a)}, "bit_identical": same,
            **s, **verdict(s), "table_sample_t": own["sample_t"], "table_pdf_t": own["pdf_t"]}


def bench_render(rounds, reps, width, height, spp):
    cam, centers, radii = scene_of(12, width, height)
    tab = MaterialTable([net_of(i) for i in ARRAY2_IDX])
    gts = {m: reference_bsdf(i) for m, i in enumerate(ARRAY2_IDX)}
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    out = []
    # ArrayRenderer: the table, the loop, no ground truth
    mk = lambda gt, fused=True: WF.ArrayRenderer(tab, centers, radii, camera=cam, albedo=TINT, ground_truth=gt, fused_ground_truth=fused)
    r = {"fused": mk(gts), "loop": mk(gts, False), "no_ground_truth": mk(None)}
    films = {k: v.render(2, spp, seed=9) for k, v in r.items()}
    torch.cuda.synchronize()
    same = torch.equal(films["fused"], films["loop"])
    if not same:
        raise SystemExit("render pass: the fused and the loop films differ")
    film = {k: torch.zeros((height, width, 3), device="cuda") for k in r}
    s = summary(time_rounds({k: (lambda k=k: r[k].render_pass(film[k], 0, height, spp, 0, 1)) for k in r}, rounds, reps))
    mat = r["fused"].primary(0, height, 1, 0, 0)["mat"]
    out.append({"what": "ArrayRenderer.render_pass, analytic ground truth on every ball", "film": [width, height], "spp": spp, "balls": 12,
                "lanes": width * height * spp, "ball_fraction": float((mat < 12).float().mean()), "bit_identical_film": same,
                **s, **verdict(s), "fused_over_no_ground_truth": s["fused"]["median_ms"] / s["no_ground_truth"]["median_ms"]})
    # PathArrayRenderer, four vertices: the table against no ground truth
    mk = lambda gt: PathArrayRenderer(tab, centers, radii, camera=cam, albedo=TINT, ground_truth=gt, max_depth=4)
    r = {"fused": mk(gts), "no_ground_truth": mk(None)}
    for v in r.values():
        v.render(2, spp, seed=9)
    torch.cuda.synchronize()
    film = {k: torch.zeros((height, width, 3), device="cuda") for k in r}
    s = summary(time_rounds({k: (lambda k=k: r[k].render_pass(film[k], 0, height, spp, 0, 1)) for k in r}, rounds, reps))
    out.append({"what": "PathArrayRenderer.render_pass, max_depth 4, analytic ground truth on every ball", "film": [width, height],
                "spp": spp, "balls": 12, "lanes": width * height * spp, "lanes_per_bounce": list(r["fused"].stats["lanes_per_bounce"]),
                **s, "fused_over_no_ground_truth": s["fused"]["median_ms"] / s["no_ground_truth"]["median_ms"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=683)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--eval-spp", type=int, default=3, help="paths per pixel of the eval-alone rows: 683 x 512 x 3 = 1 049 088 rows, ~1 Mi")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analytic_table.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("analytic_table_bench needs the GPU: nothing is measured without one")
    record = {"tool": "tools/analytic_table_bench.py", "device": torch.cuda.get_device_name(0),
              "library": _lib.lib().bsdfd_version().decode(), "rounds": a.rounds, "repetitions_per_round": a.reps,
              "timing": "device events around the repetitions of a round; the paths of a comparison interleaved inside every round",
              "materials": "analytic.reference_bsdf(idx): 12 = the ids of matpreview/disney_bsdf_array2_spherical_envmap.xml, 26 = the whole list",
              "results": []}

    def keep(res):
        brief = {k: v for k, v in res.items() if not isinstance(v, dict) or k == "launches"}
        brief.update({k + "_median_ms": v["median_ms"] for k, v in res.items() if isinstance(v, dict) and "median_ms" in v})
        print(json.dumps(brief), flush=True)
        record["results"].append(res)

    for idx in (ARRAY2_IDX, tuple(range(26))):
        for kind in ("coherent", "random"):
            keep(bench_eval(idx, kind, a.width, a.height, a.eval_spp, a.rounds, a.reps))
    for res in bench_render(a.rounds, a.reps, a.width, a.height, a.spp):
        keep(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
