"""Native bucketing by material (sharding.bucket_by_material_native: csrc/bucket.hip up to 64 materials, csrc/bucket_wide.hip
above) against torch.argsort(stable=True) + torch.bincount on the same ids, in one process: per (N, n_materials) the two are
timed alternately, round after round, with device events around a few back-to-back calls each, and the median round is
reported.  Both sides allocate their outputs from torch's caching allocator, as sharding.bucket_by_material does.

    python tools/bucket_bench.py --out profiles/bucket_wide.json

sharding.NATIVE_MAX_MATERIALS is set from the record: the largest width at which native wins at every measured size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd.sharding import bucket_by_material_native  # noqa: E402


def torch_bucket(ids, m):
    return torch.argsort(ids, stable=True), torch.bincount(ids, minlength=m)


def timed_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 24, 1 << 20])
    ap.add_argument("--materials", type=int, nargs="+", default=[64, 79, 256, 4096, 65536])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bucket_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    rows = []
    for n in args.sizes:
        for m in args.materials:
            ids = torch.randint(0, m, (n,), generator=torch.Generator().manual_seed(n + m)).to(dev)
            perm, counts = bucket_by_material_native(ids, m)
            perm_t, counts_t = torch_bucket(ids, m)
            same = bool(torch.equal(perm, perm_t) and torch.equal(counts, counts_t))
            del perm, counts, perm_t, counts_t
            sides = {"native": lambda: bucket_by_material_native(ids, m), "torch": lambda: torch_bucket(ids, m)}
            for fn in sides.values():          # warm-up of both at this shape
                timed_ms(fn, args.calls)
            ms = {k: [] for k in sides}
            for _ in range(args.rounds):       # alternating
                for k, fn in sides.items():
                    ms[k].append(timed_ms(fn, args.calls))
            row = {"n": n, "n_materials": m, "kernel": "bucket.hip" if m <= 64 else "bucket_wide.hip", "equal_to_torch": same}
            for k, v in ms.items():
                row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(v), min(v), max(v)
            row["torch_over_native"] = row["torch_ms_median"] / row["native_ms_median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    widths = sorted(args.materials)
    wins = [m for m in widths if all(r["torch_over_native"] > 1 for r in rows if r["n_materials"] == m)]
    rec = {"what": "stable bucketing of int64 material ids, uniform random in [0, n_materials): native vs "
                   "torch.argsort(stable=True) + torch.bincount, alternating rounds in one process, median of rounds, ms per call",
           "device": torch.cuda.get_device_name(0), "library": _lib.lib().bsdfd_version().decode(), "torch": torch.__version__,
           "rounds": args.rounds, "calls_per_round": args.calls, "rows": rows,
           "native_faster_at_every_size": wins,
           "largest_width_where_native_wins_everywhere": max(wins) if wins else None}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "rows"}))


if __name__ == "__main__":
    main()
