"""A/B of the ground-truth eval() of a mixed-material wavefront: ONE launch on the lane-ordered arrays (measured.MeasuredTable,
csrc/measured_table.hip) against the per-material loop (gathered copies, two MeasuredBSDF.eval_t launches per material, NaN
fills, indexed scatter).  Writes profiles/measured_table.json.

  eval alone     1 Mi rows, 12 and 77 materials, image-coherent ids (runs of 4096 lanes) and ids drawn per lane
  render pass    ArrayRenderer, 683x512, 4 spp, the 12-ball array scene with ground truth on every ball,
                 fused_ground_truth=True against False

Both paths run in the same process in interleaved rounds (fused, loop, fused, loop, ...), each round timed with device events
around several repetitions; the record keeps every round, so the round-to-round spread is there to judge the difference by.
The loop is timed as a lane-order caller pays for it: the stable sort of the ids is NOT included (a renderer has it anyway for
sample() / pdf()), the gathers of wi / wo / wl into bucket order, the launches, the fills and the scatter are.  The two paths'
outputs are compared bit for bit before anything is timed.

Only one real RGL file is available to this repository (tests/golden/chm_orange_rgb.bsdf); the other materials are synthetic
files of the same layout (bsdf_diffusion_sampling_amd/measured_synth.py) with grids of the real files' order of magnitude."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd import measured_synth as F  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402
from bsdf_diffusion_sampling_amd.materials import MaterialTable  # noqa: E402
from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable  # noqa: E402


def make_materials(d, n):
    """n MeasuredBSDF: the real file first, then synthetic anisotropic / isotropic files with varying grids."""
    out = [MeasuredBSDF(os.path.join(ROOT, "tests", "golden", "chm_orange_rgb.bsdf"))]
    for k in range(1, n):
        p = os.path.join(d, f"synth_{k}_rgb.bsdf")
        if k % 2:
            F.write_anisotropic(p, seed=k, vndf_hw=(32 + 8 * (k % 3), 32), rgb_hw=(16, 16 + 4 * (k % 2)), ndf_hw=(2, 64))
        else:
            F.write_isotropic(p, seed=k, n_theta=8, vndf_hw=(64, 64 + 16 * (k % 3)), rgb_hw=(32, 32), ndf_hw=(2, 128), jacobian=k % 4 // 2)
        out.append(MeasuredBSDF(p))
    return out


def time_rounds(paths, rounds, reps):
    """{name: [ms per call, one entry per round]} with the paths interleaved inside every round."""
    ms = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    return ms


def summary(ms):
    out = {}
    for name, v in ms.items():
        out[name] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "rounds_ms": [float(x) for x in v]}
    return out


def verdict(s):
    """fused vs loop by the medians, against the larger of the two paths' own round-to-round spreads (max - min)."""
    spread = max(s["fused"]["max_ms"] - s["fused"]["min_ms"], s["loop"]["max_ms"] - s["loop"]["min_ms"])
    diff = s["fused"]["median_ms"] - s["loop"]["median_ms"]
    return {"loop_over_fused": s["loop"]["median_ms"] / s["fused"]["median_ms"], "spread_ms": spread,
            "fused_slower_beyond_spread": bool(diff > spread)}


def bench_eval(mats, ids_kind, n, rounds, reps, tint):
    g = np.random.default_rng(len(mats))
    dev = torch.device("cuda")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    wi, wo, wl = to(F.dirs(g, n)), to(F.dirs(g, n)), to(F.dirs(g, n))
    if ids_kind == "coherent":
        ids = torch.from_numpy((g.permutation(n // 4096 + 1)[np.arange(n) // 4096] % len(mats)).astype(np.int64)).to(dev)
    else:
        ids = torch.from_numpy(g.integers(0, len(mats), size=n).astype(np.int64)).to(dev)
    table = MeasuredTable(mats)
    rows = torch.sort(ids, stable=True).indices
    seg_end = torch.cumsum(torch.bincount(ids, minlength=len(mats)), 0).tolist()
    f_o, f_l = torch.empty_like(wi), torch.empty_like(wi)
    g_o, g_l = torch.empty_like(wi), torch.empty_like(wi)

    def fused():
        table.eval_t(ids, wi, wo, wl, tint=tint, out_o=f_o, out_l=f_l)

    def loop():
        wi_s, wo_s, wl_s = wi[rows], wo[rows], wl[rows]
        fo_s = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        fl_s = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
        lo = 0
        for m, hi in enumerate(seg_end):
            if hi > lo:
                mats[m].eval_t(wi_s[lo:hi], wo_s[lo:hi], out=fo_s[lo:hi], tint=tint)
                mats[m].eval_t(wi_s[lo:hi], wl_s[lo:hi], out=fl_s[lo:hi], tint=tint)
            lo = hi
        g_o.fill_(float("nan"))
        g_l.fill_(float("nan"))
        g_o[rows] = fo_s
        g_l[rows] = fl_s

    fused(), loop()
    torch.cuda.synchronize()
    same = torch.equal(f_o.view(torch.int32), g_o.view(torch.int32)) and torch.equal(f_l.view(torch.int32), g_l.view(torch.int32))
    if not same:
        raise SystemExit(f"eval {len(mats)} materials, {ids_kind} ids: the fused and the loop results differ")
    s = summary(time_rounds({"fused": fused, "loop": loop}, rounds, reps))
    return {"what": "eval alone", "rows": n, "materials": len(mats), "ids": ids_kind, "launches": {"fused": 1, "loop": 2 * len(mats)},
            "bit_identical": same, **s, **verdict(s)}


def bench_render(mats12, rounds, reps, width, height, spp):
    cam, centers, radii = WF.array0_scene(width, height)
    tab = MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS])
    gts = dict(enumerate(mats12))
    mk = lambda fused: WF.ArrayRenderer(tab, centers, radii, camera=cam, albedo=(0.9, 0.8, 0.7), ground_truth=gts,
                                        fused_ground_truth=fused)
    r = {"fused": mk(True), "loop": mk(False)}
    films = {k: v.render(2, spp, seed=9) for k, v in r.items()}
    torch.cuda.synchronize()
    same = torch.equal(films["fused"], films["loop"])
    if not same:
        raise SystemExit("render pass: the fused and the loop films differ")
    film = {k: torch.zeros((height, width, 3), device="cuda") for k in r}
    paths = {k: (lambda k=k: r[k].render_pass(film[k], 0, height, spp, 0, 1)) for k in r}
    s = summary(time_rounds(paths, rounds, reps))
    mat = r["fused"].primary(0, height, 1, 0, 0)["mat"]
    return {"what": "ArrayRenderer.render_pass, ground truth on every ball", "film": [width, height], "spp": spp, "balls": len(mats12),
            "lanes": width * height * spp, "ball_fraction": float((mat < len(mats12)).float().mean()), "bit_identical_film": same,
            **s, **verdict(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=683)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measured_table.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measured_table_bench needs the GPU: nothing is measured without one")
    tint = (0.9, 0.8, 0.7)
    with tempfile.TemporaryDirectory(prefix="measured_table_bench_") as d:
        mats = make_materials(d, 77)
        record = {"tool": "tools/measured_table_bench.py", "device": torch.cuda.get_device_name(0),
                  "library": _lib.lib().bsdfd_version().decode(), "rounds": a.rounds, "repetitions_per_round": a.reps,
                  "timing": "device events around the repetitions of a round; fused and loop interleaved inside every round",
                  "materials": "tests/golden/chm_orange_rgb.bsdf + synthetic files (bsdf_diffusion_sampling_amd/measured_synth.py)", "results": []}
        for n_mat in (12, 77):
            for kind in ("coherent", "random"):
                res = bench_eval(mats[:n_mat], kind, a.rows, a.rounds, a.reps, tint)
                print(json.dumps({k: v for k, v in res.items() if k not in ("fused", "loop")} |
                                 {"fused_median_ms": res["fused"]["median_ms"], "loop_median_ms": res["loop"]["median_ms"]}), flush=True)
                record["results"].append(res)
        res = bench_render(mats[:12], a.rounds, a.reps, a.width, a.height, a.spp)
        print(json.dumps({k: v for k, v in res.items() if k not in ("fused", "loop")} |
                         {"fused_median_ms": res["fused"]["median_ms"], "loop_median_ms": res["loop"]["median_ms"]}), flush=True)
        record["results"].append(res)
        record["fused_ground_truth_default"] = not res["fused_slower_beyond_spread"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
