"""What honouring an `active` mask costs and buys (csrc/live.hip, FlowSampler.plugin_*(active=), WavefrontRenderer(skip_misses=)):

  (a) the compaction pass alone (live.live_rows: mask -> row list, dead rows of three result arrays zeroed, read-back of the
      count) next to torch.nonzero + three masked fills, at 1 Mi and 16 Mi lanes, live fraction 0.5;
  (b) sample() + pdf() of the disk_1Mi wavefront (bench.py's inputs) at T = 4 and T = 8 with a Bernoulli mask of live fraction
      1.0 / 0.75 / 0.5 / 0.25 against the unmasked pair of the same build; the overhead at fraction 1.0, the break-even
      fraction, and at 16 Mi lanes the row-index form (active=) against a gathered copy (compact inputs, plain launches,
      scatter of the results);
  (c) the 512^2 one-ball render with skip_misses on and off, and the hit fraction of that frame.

All legs of a comparison run alternately in one process, round after round, with device events around a few back-to-back
calls; the median round is reported (ms per call, host read-backs included: the events span them).  Board power and shader
clock are polled during every section.

    python tools/live_bench.py --out profiles/active_lanes.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from bsdf_diffusion_sampling_amd import _lib, live  # noqa: E402
from bsdf_diffusion_sampling_amd import weights as W  # noqa: E402
from bsdf_diffusion_sampling_amd.power import PowerSampler  # noqa: E402
from bsdf_diffusion_sampling_amd.sampler import FlowSampler  # noqa: E402

MATERIAL = "aniso_miro_7_rgb"


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(sides, rounds, calls):
    """{name: fn} -> {name: {median, min, max}} ms per call, legs interleaved round by round; + power / clock of the section."""
    for fn in sides.values():
        timed_ms(fn, calls)
    ms = {k: [] for k in sides}
    ps = PowerSampler(allow_rocm_smi=False)
    ps.start()
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed_ms(fn, calls))
    pw = ps.stop()
    out = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}
    return out, {"socket_power_w": pw["socket_power_w"], "sclk_mhz": pw["sclk_mhz"], "power_source": pw["source"]}


def bernoulli(n, frac, seed, dev):
    if frac >= 1.0:
        return torch.ones(n, dtype=torch.bool, device=dev)
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < frac).to(dev)


def compaction_alone(n, dev, rounds, calls):
    mask = bernoulli(n, 0.5, 7, dev)
    wo, pdf, pdf2 = torch.ones((n, 3), device=dev), torch.ones(n, device=dev), torch.ones(n, device=dev)
    dead = ~mask

    def native():
        return live.live_rows(mask, zero=(wo, pdf, pdf2))

    def with_torch():
        rows = torch.nonzero(mask).flatten()
        wo.masked_fill_(dead[:, None], 0.0)
        pdf.masked_fill_(dead, 0.0)
        pdf2.masked_fill_(dead, 0.0)
        return rows
    same = bool(torch.equal(native(), with_torch()))
    res, pw = alternate({"native": native, "torch_nonzero_plus_fills": with_torch}, rounds, calls)
    return {"n": n, "live_fraction": float(mask.float().mean()), "equal_to_torch": same, **res,
            "torch_over_native": res["torch_nonzero_plus_fills"]["ms_median"] / res["native"]["ms_median"], **pw}


def masked_pairs(n, T, fractions, dev, rounds, calls, gathered_at=None):
    s = FlowSampler(W.load(W.shipped_path(MATERIAL, "disk")))
    wi, wl = bench.make_wi("disk", n, 1234, dev), bench.make_wi("disk", n, 4321, dev)
    wo, p, p2 = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    masks = {f: bernoulli(n, f, 100 + int(f * 100), dev) for f in fractions}

    def pair(mask):
        def run():
            s.plugin_sample(wi, None, T=T, seed=5, out=(wo, p), active=mask)
            s.plugin_pdf(wi, wl, T=T, out=p2, active=mask)
        return run

    def gathered(mask):   # what a host without row_index would do: compact copies in, plain launches, results scattered back
        def run():
            rows = live.live_rows(mask, zero=(wo, p, p2))
            wi_c, wl_c = wi[rows], wl[rows]
            wo_c, p_c = s.plugin_sample(wi_c, None, T=T, seed=5, rng_index=rows)
            p2_c = s.plugin_pdf(wi_c, wl_c, T=T)
            wo[rows], p[rows], p2[rows] = wo_c, p_c, p2_c
        return run
    sides = {"unmasked": pair(None)}
    sides.update({f"active_{f:g}": pair(masks[f]) for f in fractions})
    if gathered_at is not None:
        sides[f"gathered_copy_{gathered_at:g}"] = gathered(masks[gathered_at])
        # the two forms compute the same numbers
        pair(masks[gathered_at])()
        ref = (wo.clone(), p.clone(), p2.clone())
        gathered(masks[gathered_at])()
        same = all(torch.equal(a, b) for a, b in zip(ref, (wo, p, p2)))
    res, pw = alternate(sides, rounds, calls)
    base = res["unmasked"]["ms_median"]
    row = {"n": n, "T": T, "material": MATERIAL, "domain": "disk", "tile": s.tile, "legs": res, **pw,
           "relative_to_unmasked": {k: v["ms_median"] / base for k, v in res.items()}}
    if 1.0 in fractions:
        row["overhead_at_fraction_1"] = res["active_1"]["ms_median"] / base - 1.0
    # break-even: the live fraction at which the masked pair costs what the unmasked one does (linear between the two measured
    # fractions that bracket it; None if every measured fraction is on one side)
    pts = sorted((f, res[f"active_{f:g}"]["ms_median"] / base) for f in fractions)
    row["break_even_fraction"] = None
    for (f0, r0), (f1, r1) in zip(pts, pts[1:]):
        if (r0 - 1.0) * (r1 - 1.0) <= 0 and r0 != r1:
            row["break_even_fraction"] = f0 + (1.0 - r0) * (f1 - f0) / (r1 - r0)
    if gathered_at is not None:
        row["gathered_copy_equals_row_index_form"] = bool(same)
        row["row_index_over_gathered_copy"] = res[f"active_{gathered_at:g}"]["ms_median"] / res[f"gathered_copy_{gathered_at:g}"]["ms_median"]
    s.close()
    return row


def render(kind, size, passes, spp, dev, rounds):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    if kind == "disk":
        from bsdf_diffusion_sampling_amd.brdf_measured_disk import MyBSDF
    else:
        from bsdf_diffusion_sampling_amd.brdf_measured_spherical import MyBSDF
    plug = MyBSDF({"filename": MATERIAL, "albedo": [0.9, 0.9, 0.9], "measured": False})
    cam = WF.Camera(width=size, height=size)
    rs = {skip: WF.WavefrontRenderer(plug, cam, skip_misses=skip) for skip in (False, True)}
    b = rs[True].primary(0, size, spp, 0, 0)
    hit = float((b["mat"] == 0).float().mean())
    same = bool(torch.equal(rs[False].render(2, spp, seed=3), rs[True].render(2, spp, seed=3)))
    res, pw = alternate({"skip_misses_off": lambda: rs[False].render(passes, spp, seed=0),
                         "skip_misses_on": lambda: rs[True].render(passes, spp, seed=0)}, rounds, 1)
    return {"workload": f"render_{size}x{size}_{passes}x{spp}spp_{kind}", "euler_steps": plug.T, "hit_fraction": hit,
            "same_film": same, **{k: {kk: vv / passes for kk, vv in v.items()} for k, v in res.items()}, "unit": "ms per pass",
            "on_over_off": res["skip_misses_on"]["ms_median"] / res["skip_misses_off"]["ms_median"], **pw}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back calls per timed window")
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the control flow, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("live_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    mi, big, size = ((1 << 12, 1 << 14, 64) if args.small else (1 << 20, 1 << 24, 512))
    fr = [1.0, 0.75, 0.5, 0.25]
    rec = {"what": "cost and gain of honouring an `active` mask: alternating legs in one process, median of rounds, ms per call "
                   "(device events around back-to-back calls; the masked legs include their read-back of the live count)",
           "device": torch.cuda.get_device_name(0), "library": _lib.lib().bsdfd_version().decode(), "torch": torch.__version__,
           "rounds": args.rounds, "calls_per_round": args.calls}
    rec["compaction_alone"] = [compaction_alone(n, dev, args.rounds, args.calls) for n in (mi, big)]
    print(json.dumps(rec["compaction_alone"]), flush=True)
    rec["sample_plus_pdf"] = [masked_pairs(mi, T, fr, dev, args.rounds, args.calls) for T in (4, 8)]
    print(json.dumps(rec["sample_plus_pdf"]), flush=True)
    rec["row_index_vs_gathered_copy_16Mi"] = masked_pairs(big, 4, [0.5], dev, args.rounds, 2, gathered_at=0.5)
    print(json.dumps(rec["row_index_vs_gathered_copy_16Mi"]), flush=True)
    rec["render"] = [render(k, size, 8, 4, dev, args.rounds) for k in ("disk", "spherical")]
    print(json.dumps(rec["render"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
