"""The principled ground truth (analytic.Principled; csrc/principled.hip, csrc/principled_dev.h) in figures.  Writes
profiles/principled.json:

  kernels     registers, scratch and occupancy of the four kernels as the compiler reports them (needs hipcc)
  accuracy    idx 5, 10, 13 and 17, 32 768 rows on both sides of the surface: error of eval_t, pdf_t, sample_t and sample_weight
              against the fp64 run of tests/principled_ref.py, next to the yardstick the GPU tests use — the same numpy code in fp32
  timing      1 Mi rows on one `wi` set (both sides of the surface): the four kernels next to RoughDielectric's four on the same
              rows and to the full-sphere plugin's sample_t (the neural sampler of bsdf_13)
  identify    L1 distance between the normalised density of each of the 22 shipped nets bsdf_0..22 (plugin pdf, T = 8) and its
              own normalised model, on 20 000 uniform directions, theta_i = 0.3 and 1.0
  variance    idx 1, 13, 17 and theta_i = 0.3 / 1.0 / 1.3: mean and variance of f |cos| / pdf under the neural sampler and under the
              model's own sampler (the reference paper's comparison), with the share of neural samples the firefly rule would cut

Every timed path runs in the same process in interleaved rounds, each round timed with device events around several repetitions;
the record keeps the median, minimum and maximum over the rounds.  Nothing here is asserted."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import principled_ref as R  # noqa: E402
from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd import weights as W  # noqa: E402
from bsdf_diffusion_sampling_amd.analytic import REFERENCE_PRINCIPLED, RoughDielectric, reference_bsdf  # noqa: E402
from tools.measured_sample_bench import time_rounds, to_dev  # noqa: E402

TINT = (0.9, 0.2, 0.4)
ACCURACY_IDX = (5, 10, 13, 17)
VARIANCE_IDX = (1, 13, 17)
KERNELS = ("principled_eval_kernel", "principled_weight_kernel", "principled_sample_kernel", "principled_pdf_kernel")


def kernel_resources():
    if not shutil.which("hipcc"):
        return None
    out = {}
    with tempfile.TemporaryDirectory(prefix="principled_bench_cc_") as td:
        cmd = ["hipcc", *_lib.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-I", _lib.INCLUDE_DIR, "-c",
               os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc", "principled.hip"), "-o", os.path.join(td, "principled.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        for block in text.split("Function Name: ")[1:]:
            name = next((k for k in KERNELS if re.search(r"\d+" + k + "E", block.split()[0])), None)
            if name:
                grab = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
                out[name] = {"vgprs": grab(r" VGPRs"), "sgprs": grab(r"TotalSGPRs"), "scratch_bytes_per_lane": grab(r"ScratchSize \[bytes/lane\]"),
                             "lds_bytes_per_block": grab(r"LDS Size \[bytes/block\]"), "occupancy_waves_per_simd": grab(r"Occupancy \[waves/SIMD\]")}
    return out


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max(0))


def _fig(e):
    e = e.max(1) if e.ndim == 2 else e
    return {"p99": float(np.percentile(e, 99)), "max": float(e.max())}


def accuracy(n):
    out = []
    for idx in ACCURACY_IDX:
        g = np.random.default_rng(idx)
        r64, r32, b = R.reference(idx), R.reference(idx, np.float32), reference_bsdf(idx)
        wi = R.sphere_dirs(g, n).astype(np.float32)
        u = g.random((n, 3)).astype(np.float32)
        wo = R.sphere_dirs(g, n)
        own = r64.sample(wi[: n // 2], g.random((n // 2, 3)))[0]
        hit = np.abs(own).sum(1) > 0
        blur = own + g.normal(size=(n // 2, 3)) * 0.5 * float(np.sqrt(r64.ax * r64.ay))
        wo[: n // 2][hit] = (blur / np.linalg.norm(blur, axis=1, keepdims=True))[hit]
        wo = wo.astype(np.float32)
        wi_d, wo_d, u_d = to_dev(wi), to_dev(wo), to_dev(u)
        ref = {"eval": r64.eval(wi, wo, TINT), "pdf": r64.pdf(wi, wo)}
        yard = {"eval": r32.eval(wi, wo, TINT), "pdf": r32.pdf(wi, wo)}
        got = {"eval": b.eval_t(wi_d, wo_d, tint=TINT).cpu().numpy(), "pdf": b.pdf_t(wi_d, wo_d).cpu().numpy()}
        pdf_sa = (0.1 * ref["pdf"] + 1e-3).astype(np.float32)
        ref["sample_weight"], yard["sample_weight"] = r64.sample_weight(wi, wo, pdf_sa, TINT)[0], r32.sample_weight(wi, wo, pdf_sa, TINT)[0]
        got["sample_weight"] = b.sample_weight(wi_d, wo_d, to_dev(pdf_sa), tint=TINT)[0].cpu().numpy()
        # (rows whose value is within 1e-2 of the firefly threshold may fall on either side of it: not scored)
        clear = np.abs(ref["eval"][:, 0] / pdf_sa - 3.5) > 1e-2
        s_ref, s_yard = r64.sample(wi, u, TINT, details=True), r32.sample(wi, u, TINT, details=True)
        s_got = tuple(t.cpu().numpy() for t in b.sample_t(wi_d, u_d, tint=TINT))
        d_r, d_y = s_ref[3], s_yard[3]
        close = np.any([np.abs(u[:, 2].astype(np.float64) - t) < 1e-5 for t in d_r["thresholds"]], axis=0)
        rows_g = ~close & d_r["ok"] & (s_got[1] > 0)
        rows_y = ~close & d_r["ok"] & d_y["ok"] & (d_y["lobe"] == d_r["lobe"])
        rec = {"idx": idx, "rows": n, "rows_within_1e-5_of_a_lobe_threshold": int(close.sum()),
               "rows_whose_success_differs_from_fp64": {"gpu": int(((s_got[1] > 0) != d_r["ok"])[~close].sum()),
                                                        "fp32_yardstick": int((d_y["ok"] != d_r["ok"])[~close].sum())},
               "gpu": {q: _fig(_err(got[q], ref[q])[clear] if q == "sample_weight" else _err(got[q], ref[q])) for q in got},
               "fp32_yardstick": {q: _fig(_err(yard[q], ref[q])[clear] if q == "sample_weight" else _err(yard[q], ref[q])) for q in yard}}
        for name, res, rows in (("gpu", s_got, rows_g), ("fp32_yardstick", s_yard, rows_y)):
            rec[name]["sample wo"] = _fig(np.abs(np.asarray(res[0], np.float64) - s_ref[0])[rows])
            rec[name]["sample pdf"] = _fig(_err(res[1], s_ref[1])[rows])
            rec[name]["sample weight"] = _fig(_err(res[2], s_ref[2])[rows])
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def timing(n, rounds, reps):
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    g = np.random.default_rng(1)
    wi = to_dev(R.sphere_dirs(g, n))
    u3 = to_dev(g.random((n, 3)))
    b, dl = reference_bsdf(13), RoughDielectric(0.3)
    plug = MyBSDF({"idx": 13})
    out3 = (torch.empty_like(wi), torch.empty(n, device="cuda"), torch.empty_like(wi))
    buf1, buf3 = torch.empty(n, device="cuda"), torch.empty_like(wi)
    wo = b.sample_t(wi, u3)[0].clone()
    wo = torch.where((wo == 0).all(1, keepdim=True), dl.sample_t(wi, u3)[0], wo).contiguous()     # (a failed sample has no direction)
    pdf_sa = plug.sample_t(wi, seed=11)[1].clone()
    paths = {}
    for name, m in (("principled", b), ("dielectric", dl)):
        paths[f"{name} eval_t"] = lambda m=m: m.eval_t(wi, wo, out=buf3, tint=TINT)
        paths[f"{name} sample_t"] = lambda m=m: m.sample_t(wi, u3, tint=TINT, out=out3)
        paths[f"{name} pdf_t"] = lambda m=m: m.pdf_t(wi, wo, out=buf1)
        paths[f"{name} sample_weight"] = lambda m=m: m.sample_weight(wi, wo, pdf_sa, tint=TINT)
    paths["full-sphere plugin sample_t (bsdf_13, T = 8)"] = lambda: plug.sample_t(wi, seed=11)
    res = time_rounds(paths, rounds, reps)
    for k, v in res.items():
        print(f"{k:50s} {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max {v['max_ms']:.4f})", flush=True)
    ratio = {c: res[f"principled {c}"]["median_ms"] / res[f"dielectric {c}"]["median_ms"] for c in ("eval_t", "sample_t", "pdf_t", "sample_weight")}
    return {"rows": n, "rounds": rounds, "repetitions_per_round": reps, "wi": "uniform on the sphere", "paths": res,
            "principled_over_dielectric_median": ratio}


def identify(n=20000):
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    dirs = to_dev(R.sphere_dirs(np.random.default_rng(2), n))
    out = []
    for idx in sorted(REFERENCE_PRINCIPLED):
        if not os.path.exists(W.shipped_path(f"bsdf_{idx}", "spherical")):
            continue
        plug, b = MyBSDF({"idx": idx}), reference_bsdf(idx)
        for theta in (0.3, 1.0):
            wi = to_dev(R.wi_of(theta, 0.0, n))
            p = plug.pdf_t(wi, dirs).double()
            p = p / p.sum()
            q = b.eval_t(wi, dirs)[:, 0].double()
            q = q / q.sum()
            low = dirs[:, 2] < 0
            out.append({"set": f"bsdf_{idx}", "theta_i": theta, "l1_to_own_model": float((p - q).abs().sum()),
                        "lower_hemisphere_mass": {"net": float(p[low].sum()), "model": float(q[low].sum())}})
            print(json.dumps(out[-1]), flush=True)
    return out


def variance(n):
    from bsdf_diffusion_sampling_amd.bsdf_myresult import MyBSDF
    out = []
    gen = torch.Generator(device="cuda").manual_seed(7)
    for idx in VARIANCE_IDX:
        plug = MyBSDF({"idx": idx, "analytic": "all"})
        b = plug.bsdf
        for theta in (0.3, 1.0, 1.3):
            wi = to_dev(R.wi_of(theta, 0.0, n))
            wo, pdf_sa = plug.sample_t(wi, seed=1234 + idx)
            f = b.eval_t(wi, wo)[:, 0]
            w_net = torch.where(pdf_sa > 0, f / pdf_sa.clamp_min(1e-30), torch.zeros_like(f)).double()
            w_own = b.sample_t(wi, torch.rand(n, 3, generator=gen, device="cuda"))[2][:, 0].double()
            rec = {"set": f"bsdf_{idx}", "theta_i": theta, "samples": n,
                   "neural": {"mean": float(w_net.mean()), "variance": float(w_net.var()), "max": float(w_net.max()),
                              "share_at_or_above_3.5": float((w_net >= 3.5).double().mean())},
                   "analytic": {"mean": float(w_own.mean()), "variance": float(w_own.var()), "max": float(w_own.max()),
                                "failed_share": float((w_own == 0).double().mean())}}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--accuracy-rows", type=int, default=32768)
    ap.add_argument("--variance-samples", type=int, default=1 << 18)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "principled.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("principled_bench needs the GPU: nothing is measured without one")
    record = {"tool": "tools/principled_bench.py", "device": torch.cuda.get_device_name(0), "library": _lib.lib().bsdfd_version().decode(),
              "timing_method": "device events around the repetitions of a round; all paths interleaved inside every round; "
                               "median / min / max over the rounds",
              "accuracy_method": "error against the fp64 run of tests/principled_ref.py, relative to max(|fp64 value|, 1e-6 of the "
                                 "column's largest); wo: max_c |wo - ref|; the sample rows are those the fp64 run succeeds on, without those "
                                 "within 1e-5 of a lobe threshold (and, for the yardstick, the rows where its lobe or success differs); the "
                                 "yardstick is the same numpy code in fp32",
              "variance_method": "weight = f |cos| / pdf, channel x, no tint, no firefly rule; neural: the full-sphere plugin's sample_t "
                                 "(T = 8) weighted with eval_t; analytic: sample_t's own weight (0 for a failed sample)",
              "kernels": kernel_resources(), "accuracy": accuracy(a.accuracy_rows), "timing": timing(a.rows, a.rounds, a.reps),
              "identify": identify(), "variance": variance(a.variance_samples)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
