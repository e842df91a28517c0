"""CPU-only tests of the host logic: weight format, C-ABI surface, reference-shaped
containers, sharding (incl. world_size-2 gloo), and the no-fallback rule."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from bsdf_diffusion_sampling_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_file_roundtrip(tmp_path):
    fw = W.load(W.shipped_path("chm_orange_rgb", "disk"))
    p = tmp_path / "x.bsdfw"
    W.save(str(p), fw)
    f2 = W.load(str(p))
    for k in ("w_in", "w_hidden", "w_out", "base_w1", "base_b1", "base_w2", "base_b2"):
        assert np.array_equal(getattr(fw, k), getattr(f2, k))
    assert (f2.domain, f2.width, f2.n_hidden, f2.name) == (0, 32, 3, "chm_orange_rgb")
    raw = p.read_bytes()
    (tmp_path / "bad.bsdfw").write_bytes(raw[:-4])
    with pytest.raises(ValueError):
        W.load(str(tmp_path / "bad.bsdfw"))
    (tmp_path / "bad2.bsdfw").write_bytes(b"NOTMAGIC" + raw[8:])
    with pytest.raises(ValueError):
        W.load(str(tmp_path / "bad2.bsdfw"))


def test_shipped_weight_inventory():
    """27 disk + 25 measured spherical + 25 bsdf_<i> spherical sets."""
    disk, sph = W.list_shipped("disk"), W.list_shipped("spherical")
    assert len(disk) == 27
    assert len([s for s in sph if s.startswith("bsdf_")]) == 25
    assert len([s for s in sph if not s.startswith("bsdf_")]) == 25
    fw = W.load(W.shipped_path("bsdf_3", "spherical"))
    assert (fw.width, fw.n_hidden, fw.in_dim) == (32, 4, 26)
    fc = W.load(W.shipped_path("aniso_miro_7_rgb", "spherical", "complex"))
    assert (fc.width, fc.n_hidden) == (64, 6)


def test_algorithmic_flops_match_survey():
    """SURVEY.md §8(d) / BASELINE.md §3."""
    d = W.load(W.shipped_path("aniso_miro_7_rgb", "disk"))
    s = W.load(W.shipped_path("aniso_miro_7_rgb", "spherical"))
    c = W.load(W.shipped_path("aniso_miro_7_rgb", "spherical", "complex"))
    assert d.flops_per_step() == 14272 and d.flops_per_query(4) == 57664 and d.flops_per_query(8) == 114752
    assert s.flops_per_step() == 20608 and s.flops_per_query(8) == 165440
    assert c.flops_per_step() == 127232 and c.flops_per_query(8) == 1018432


def test_c_abi_library_loads_and_exports_every_declared_symbol():
    from bsdf_diffusion_sampling_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    declared = set(re.findall(r"\b(bsdfd_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(L, name)
    assert b"gfx950" in L.bsdfd_version()
    # the code object really is gfx950
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o",
                          f"--input={_lib.LIB_PATH}"], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        assert "gfx950" in out.stdout


def test_header_is_plain_c(tmp_path):
    """The drop-in boundary is a C ABI: include/bsdfd.h compiles as strict C99 (what cgo / JNI / a ctypes generator would parse)
    and as C++11, warnings as errors, with nothing but the standard headers it includes itself."""
    import shutil
    if not shutil.which("gcc") or not shutil.which("g++"):
        pytest.skip("needs gcc and g++")
    inc = os.path.join(ROOT, "include")
    c = tmp_path / "hdr.c"
    c.write_text('#include "bsdfd.h"\nint main(void) { bsdfd_desc d; bsdfd_opts o; (void)d; (void)o; return BSDFD_OK; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-unused-but-set-variable", "-I", inc,
                        "-c", str(c), "-o", str(tmp_path / "hdr_c.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "hdr.cpp"
    cpp.write_text('#include "bsdfd.h"\nint main() { bsdfd_desc d{}; (void)d; return BSDFD_OK; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(cpp), "-o",
                        str(tmp_path / "hdr_cpp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_structs_mirror_the_header(tmp_path):
    """The ctypes mirrors of the boundary's structs (bsdf_diffusion_sampling_amd/_lib.py: Desc, Opts, WfScene) have the size and
    the field offsets gcc gives the C declarations of include/bsdfd.h, and the host's ABI_VERSION is the header's
    BSDFD_ABI_VERSION (structs grow at the end between versions: a stale mirror would pass garbage for the new fields)."""
    import ctypes as C
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from bsdf_diffusion_sampling_amd import _lib
    fields = {"bsdfd_desc": [n for n, _ in _lib.Desc._fields_], "bsdfd_opts": [n for n, _ in _lib.Opts._fields_],
              "bsdfd_wf_scene": [n for n, _ in _lib.WfScene._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bsdfd.h"', 'int main(void) {', '  printf("abi %d\\n", BSDFD_ABI_VERSION);']
    for st, names in fields.items():
        src.append(f'  printf("{st} size %zu\\n", sizeof({st}));')
        for f in names:
            src.append(f'  printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        parts = line.split()
        got[tuple(parts[:-1])] = int(parts[-1])
    assert got[("abi",)] == _lib.ABI_VERSION
    for st, cls in (("bsdfd_desc", _lib.Desc), ("bsdfd_opts", _lib.Opts), ("bsdfd_wf_scene", _lib.WfScene)):
        assert got[(st, "size")] == C.sizeof(cls), st
        for f in fields[st]:
            assert got[(st, f)] == getattr(cls, f).offset, (st, f)
    assert [n for n, _ in _lib.Opts._fields_] == ["ctx_out", "ctx_in", "rng_index", "row_index"]


def test_no_cpu_fallback():
    """The product path must fail loudly without the GPU / the HIP library."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    with pytest.raises(RuntimeError, match="no CPU path"):
        FlowSampler(W.load(W.shipped_path("chm_orange_rgb", "disk")))
    from bsdf_diffusion_sampling_amd.brdf_measured_disk import MyBSDF
    with pytest.raises(RuntimeError):
        MyBSDF({"filename": "chm_orange_rgb"})
    # and nothing in the package imports the oracle
    pkg = os.path.join(ROOT, "bsdf_diffusion_sampling_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_reference_shaped_containers():
    from bsdf_diffusion_sampling_amd import model as M
    fw = W.load(W.shipped_path("aniso_miro_7_rgb", "spherical"))
    db, ds = M.from_flow_weights(fw)
    assert sorted(ds.state_dict()) == ["linear1.weight", "linear2.weight", "linear3.weight", "linear4.weight",
                                       "output.weight"]
    assert sorted(db.state_dict()) == ["linear1.bias", "linear1.weight", "output.bias", "output.weight"]
    assert ds.linear1.weight.shape == (32, 26) and db.linear1.weight.shape == (16, 14)
    f2 = M.to_flow_weights(db, ds, W.DOMAIN_SPHERICAL)
    assert np.array_equal(f2.w_hidden, fw.w_hidden) and np.array_equal(f2.base_w2, fw.base_w2)
    # the reference's constructor calls (brdf_measured_disk.py:43,49)
    d = M.NN_cond_pos_simpler(input_dim=5, output_dim=2, N_NEURONS=32, POSITIONAL_ENCODING_BASIS_NUM=5)
    b = M.NN_cond_pretrain_disk_one(input_dim=2, N_NEURONS=16, POSITIONAL_ENCODING_BASIS_NUM=3)
    assert d.linear1.weight.shape == (32, 25) and d.linear3.weight.shape == (32, 32) and d.output.weight.shape == (2, 32)
    assert b.linear1.weight.shape == (16, 14)
    c = M.NN_cond_pos_spherical_complicate(input_dim=6, output_dim=2, N_NEURONS=64, POSITIONAL_ENCODING_BASIS_NUM=5)
    assert c.linear6.weight.shape == (64, 64)
    with pytest.raises(NotImplementedError):
        d(torch.zeros(1, 2), torch.zeros(1, 1), torch.zeros(1, 2))


def test_shard_ranges_partition():
    from bsdf_diffusion_sampling_amd.sharding import shard_range, shard_sizes
    for n in (0, 1, 7, 8, 9, 1 << 20, (1 << 27) + 3):
        for w in (1, 2, 3, 8):
            rs = [shard_range(n, r, w) for r in range(w)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(rs[i][1] == rs[i + 1][0] for i in range(w - 1))
            sz = shard_sizes(n, w)
            assert sum(sz) == n and max(sz) - min(sz) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


def test_bucket_by_material():
    from bsdf_diffusion_sampling_amd.sharding import bucket_by_material
    ids = torch.tensor([3, 0, 2, 3, 0, 0, 1])
    perm, counts = bucket_by_material(ids, 5)
    assert counts.tolist() == [3, 1, 1, 2, 0]
    assert ids[perm].tolist() == [0, 0, 0, 1, 2, 3, 3]
    assert perm.tolist() == [1, 4, 5, 6, 2, 0, 3]  # stable


_GLOO_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from bsdf_diffusion_sampling_amd.sharding import shard_range, gather_to_root, all_gather, pack_result
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
for n in (10, 11, 4096, 1):
    full = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)
    lo, hi = shard_range(n, rank, world)
    wo, pdf = full[lo:hi, :3].clone(), full[lo:hi, 3].clone()
    local = pack_result(wo, pdf)
    got = gather_to_root(local, n, root=0)
    if rank == 0:
        assert torch.equal(got, full), (n, got, full)
    else:
        assert got is None
    assert torch.equal(all_gather(local, n), full)
try:
    gather_to_root(torch.zeros(3, 4), 100)
    raise SystemExit("expected ValueError")
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
print("ok", rank)
"""


def test_gather_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533", str(script), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2


def test_torch_eager_port_matches_oracle():
    """The CPU-baseline port (oracle/torch_eager_port.py) computes what the oracle computes."""
    from conftest import load_case
    from oracle import bsdf_oracle as O
    from oracle import torch_eager_port as P
    for stem in ("chm_orange_rgb_disk", "aniso_miro_7_rgb_spherical"):
        g, fw = load_case(stem)
        T = int(g["meta_T"])
        base, net = P.BaseNet(fw), P.VelocityNet(fw)
        n = 256
        wi, x0 = torch.from_numpy(g["wi"][:n]), torch.from_numpy(g["x0"][:n])
        x, p = P.network_sampling(base, net, wi, T, x0=x0)
        # bit-identical to the reference's own outputs (the golden) on the same rows is not
        # guaranteed across batch sizes (BLAS blocking), so compare at fp32 round-off
        assert np.abs(x.numpy() - g[f"sample_x_T{T}"][:n]).max() < 2e-5
        xo, po = O.Oracle(fw).network_sampling(g["wi"][:n], g["x0"][:n], T)
        r = np.abs(p.numpy() - po) / np.maximum(np.abs(po), 1e-30)
        assert np.median(r) < 1e-5
        pp = P.network_pdf(base, net, torch.from_numpy(g["pdf_wo_a"][:n]), wi, T)
        ref = g[f"pdf_a_T{T}"][:n]
        ok = np.abs(ref) > 1e-6 * np.percentile(np.abs(ref), 99)
        assert np.median(np.abs(pp.numpy() - ref)[ok] / np.abs(ref[ok])) < 1e-5


def test_cpu_timing_record_present():
    import json
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "cpu_timing.json")))
    for c in rec["cases"]:
        assert c["x_max_abs_diff"] == 0.0 and c["pdf_max_rel_diff"] == 0.0  # port == reference, bit for bit
        assert 0.6 < c["port_sample_s"] / c["ref_sample_s"] < 1.4


def test_reference_modules_pack_to_the_shipped_weights():
    """INTEGRATION.md level 1: the reference's checkpoints (tests/golden/reference_checkpoints.npz: their state_dicts,
    unchanged, tests/golden/make_checkpoint_golden.py) load strictly into the containers that carry the reference's class
    names and state_dict keys, and packing them yields exactly the shipped .bsdfw weights."""
    from bsdf_diffusion_sampling_amd import model as M
    ck = np.load(os.path.join(ROOT, "tests", "golden", "reference_checkpoints.npz"))

    def sd(stem):
        return {k[len(stem) + 1:]: torch.from_numpy(ck[k]) for k in ck.files if k.startswith(stem + "/")}

    ds = M.NN_cond_pos_simpler(input_dim=5, output_dim=2, N_NEURONS=32, POSITIONAL_ENCODING_BASIS_NUM=5)
    ds.load_state_dict(sd("chm_orange_rgb_disk/brdf_rectify_networkchm_orange_rgb"))
    db = M.NN_cond_pretrain_disk_one(input_dim=2, N_NEURONS=16, POSITIONAL_ENCODING_BASIS_NUM=3)
    db.load_state_dict(sd("chm_orange_rgb_disk/brdf_pretrain_networkchm_orange_rgb"))
    fw = M.to_flow_weights(db, ds, W.DOMAIN_DISK)
    ship = W.load(W.shipped_path("chm_orange_rgb", "disk"))
    for k in ("w_in", "w_hidden", "w_out", "base_w1", "base_b1", "base_w2", "base_b2"):
        assert np.array_equal(getattr(fw, k), getattr(ship, k)), k
    dsp = M.NN_cond_pos(input_dim=6, output_dim=2, N_NEURONS=32, POSITIONAL_ENCODING_BASIS_NUM=5)
    dsp.load_state_dict(sd("bsdf_3_spherical/brdf_rectify_network3"))
    dbp = M.NN_cond_pretrain_spherical_one(input_dim=2, N_NEURONS=16)
    dbp.load_state_dict(sd("bsdf_3_spherical/brdf_pretrain_network3"))
    fws = M.to_flow_weights(dbp, dsp, W.DOMAIN_SPHERICAL)
    ships = W.load(W.shipped_path("bsdf_3", "spherical"))
    assert np.array_equal(fws.w_hidden, ships.w_hidden) and np.array_equal(fws.base_w1, ships.base_w1)


def test_mitsuba_adapter_fails_loudly_without_mitsuba():
    """The optional adapter is import-guarded: with no Mitsuba in the image it must raise, not degrade."""
    import importlib.util
    if importlib.util.find_spec("mitsuba") is not None:
        pytest.skip("mitsuba is installed")
    from bsdf_diffusion_sampling_amd import mitsuba_adapter
    with pytest.raises(RuntimeError, match="mitsuba / drjit are not installed"):
        mitsuba_adapter.make_bsdf_class("disk")


def test_weight_file_loader_rejects_malformed_files(tmp_path):
    """.bsdfw reader (weights.load): magic, header consistency, exact payload size."""
    from bsdf_diffusion_sampling_amd import weights as W
    good = open(W.shipped_path("chm_orange_rgb", "disk"), "rb").read()
    cases = {
        "short.bsdfw": (good[:40], "truncated header"),
        "magic.bsdfw": (b"XXXXXXXX" + good[8:], "bad magic"),
        "cut.bsdfw": (good[:-8], "truncated payload"),
        "tail.bsdfw": (good + b"\0\0\0\0", "trailing bytes"),
    }
    # state_dim field (7th int32 of the header, after magic + 64-byte name) inconsistent with the domain
    hdr = bytearray(good)
    off = 8 + 64 + 6 * 4
    hdr[off:off + 4] = (3).to_bytes(4, "little")
    cases["sd.bsdfw"] = (bytes(hdr), "state_dim")
    for name, (blob, msg) in cases.items():
        p = tmp_path / name
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=msg):
            W.load(str(p))
    fw = W.load(W.shipped_path("chm_orange_rgb", "disk"))
    out = tmp_path / "round.bsdfw"
    W.save(str(out), fw)
    assert out.read_bytes() == good


def test_shard_and_bucket_properties_hypothesis():
    """Property tests of the host-side partitioning: shards tile [0, n) in rank order with sizes differing by at
    most one; bucketing is a stable permutation whose runs have the counted lengths."""
    hyp = pytest.importorskip("hypothesis")
    st = pytest.importorskip("hypothesis.strategies")
    from bsdf_diffusion_sampling_amd.sharding import bucket_by_material, shard_range, shard_sizes

    @hyp.settings(max_examples=200, deadline=None)
    @hyp.given(st.integers(0, 10 ** 9), st.integers(1, 64))
    def shards(n, world):
        r = [shard_range(n, k, world) for k in range(world)]
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        sizes = [b - a for a, b in r]
        assert sizes == shard_sizes(n, world) and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    shards()

    @hyp.settings(max_examples=50, deadline=None)
    @hyp.given(st.lists(st.integers(0, 6), max_size=300))
    def buckets(ids):
        t = torch.tensor(ids, dtype=torch.int64)
        perm, counts = bucket_by_material(t, 7)
        assert sorted(perm.tolist()) == list(range(len(ids))) and counts.tolist() == [ids.count(m) for m in range(7)]
        s = t[perm].tolist()
        assert s == sorted(ids)
        for m in range(7):  # stability: rows of one material keep their order
            rows = [p for p in perm.tolist() if ids[p] == m]
            assert rows == sorted(rows)
    buckets()


def test_bench_self_launch_fails_loudly_without_gpus():
    """`python bench.py --gpus 2` outside a launcher starts its own ranks as child processes and returns their
    exit code: on this GPU-less container the ranks die at torch.cuda.set_device, and the parent must report
    failure (non-zero, no hang, no JSON line) instead of a fabricated number."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["BSDFD_BENCH_BACKEND"] = "gloo"
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a GPU-less host")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline", "--no-secondary"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_dump_outputs_caps_the_bytes_with_one_seeded_row_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 .npy files of the last pass's arrays; over the cap, the same seeded rows of every array
    (indices in rows.npy) and never more than the cap in all."""
    import bench

    class Wl:
        def __init__(self, n):
            g = torch.Generator().manual_seed(3)
            self.out = {"wo": torch.randn(n, 3, generator=g), "sample_pdf": torch.rand(n, generator=g), "pdf": torch.rand(n, generator=g)}

        def outputs(self):
            return self.out

    wl = Wl(1000)
    d = bench.dump_outputs(wl, str(tmp_path / "all"))
    assert d["rows"] == "all" and not (tmp_path / "all" / "rows.npy").exists()
    for k, t in wl.out.items():
        x = np.load(tmp_path / "all" / (k + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, t.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10000)
    for sub in ("s1", "s2"):
        bench.dump_outputs(wl, str(tmp_path / sub))
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "s2" / "rows.npy"))
    assert len(rows) == 10000 // (4 * 5 + 8) and np.all(np.diff(rows) > 0)
    total = rows.nbytes
    for k, t in wl.out.items():
        x = np.load(tmp_path / "s1" / (k + ".npy"))
        assert np.array_equal(x, t.numpy()[rows.astype(np.int64)])
        total += x.nbytes
    assert total <= 10000


def test_torch_operator_library_registers_every_operator():
    """libbsdfd_torch.so (csrc/torch_ops.cpp) loads without a GPU and registers torch.ops.bsdfd.* — one operator per
    C-ABI entry point of the hot path; compute calls need the GPU and fail loudly without one."""
    import torch
    from bsdf_diffusion_sampling_amd import torch_ext
    ns = torch_ext.load()
    for name in torch_ext.OPS:
        assert hasattr(ns, name), name
    schema = torch.ops.bsdfd.plugin_sample.default._schema
    assert [a.name for a in schema.arguments] == ["handle", "variant", "wi", "x0", "seed", "offset", "T"]
    with pytest.raises(RuntimeError):
        ns.plugin_pdf(0, 0, torch.zeros(4, 3), torch.zeros(4, 3), 4)      # CPU tensors / null handle: refused
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ns.create_from_file("/nonexistent.bsdfw", 0, 0)



def test_asynchronous_lds_reads_are_not_touched_before_their_wait():
    """csrc/bsdfd.hip fetches weight fragments with inline-asm ds_read_b128 whose destination registers only become valid
    at the following s_waitcnt (the compiler believes them valid at once).  tools/isa_mix.py --check-async verifies on the
    assembly of THIS toolchain's build that nothing reads, writes or spills them in between (a different hipcc
    could schedule a copy into that window)."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), "--check-async"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(", 0 violations") == 8 and "25 asynchronous" in r.stdout and "21 asynchronous" in r.stdout
    assert "census of the two translation units: 0 problem(s)" in r.stdout
    assert "MFMA results consumed before their wait states: 0 of 64 kernels" in r.stdout
    assert "lane swaps of a register written fewer than 2 wait states earlier: 0 of 64 kernels" in r.stdout
    assert r.stdout.count("occupancy ") == 9 and "LOST" not in r.stdout, r.stdout   # waves/SIMD of the tracked kernels


_ASM_OK = """
_ZN12_GLOBAL__N_111flow_kernelILi0ELi2ELi2ELb1ELi3ELb0EEEvNS_7KParamsE:
\ts_load_dword s0, s[4:5], 0x0
.LBB0_1:
\t;;#ASMSTART
\tds_read_b128 v[10:13], v2 offset:512
\t;;#ASMEND
\tv_mul_f32_e32 v3, v4, v5
\tv_mfma_f32_16x16x32_f16 v[20:23], v[30:33], v[34:37], 0
\t;;#ASMSTART
\ts_waitcnt lgkmcnt(0)
\t;;#ASMEND
\tv_mfma_f32_16x16x32_f16 v[20:23], v[10:13], v[34:37], v[20:23]
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
"""


def test_asmcheck_flags_a_touched_asynchronous_destination(tmp_path):
    """bsdf_diffusion_sampling_amd/_asmcheck.py on hand-made assembly: clean code passes; a copy out of a pending destination,
    a spill of one, spill traffic inside the Euler loop, and a branch with reads pending are each reported."""
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    key = "flow_kernelILi0ELi2ELi2ELb1ELi3ELb0E"
    n, bad = A.check_async_lines(_ASM_OK.splitlines(), key)
    assert n == 1 and bad == []
    for doctor, what in (("\tv_mov_b32_e32 v50, v11", "touches v11"),                                  # the compiler copies a pending register
                         ("\tscratch_store_dwordx4 off, v[10:13], off offset:16", "touches v1"),       # ... or spills one
                         ("\ts_cbranch_vccz .LBB0_1", "control flow")):
        txt = _ASM_OK.replace("\tv_mul_f32_e32 v3, v4, v5", doctor)
        n, bad = A.check_async_lines(txt.splitlines(), key)
        assert n == 1 and bad and what in bad[0], (doctor, bad)
    txt = _ASM_OK.replace("\ts_cbranch_scc1 .LBB0_1", "\tscratch_load_dword v60, off, off offset:4\n\ts_cbranch_scc1 .LBB0_1")
    n, bad = A.check_async_lines(txt.splitlines(), key)
    assert bad and "scratch instructions inside the Euler-step loop" in bad[0]
    f = tmp_path / "k.s"
    f.write_text(_ASM_OK)
    assert A.check_file(str(f)) == {"_ZN12_GLOBAL__N_111flow_kernelILi0ELi2ELi2ELb1ELi3ELb0EEEvNS_7KParamsE": (1, [])}


_ASM_HAZARD = """
_ZN12_GLOBAL__N_111flow_kernelILi1ELi2ELi2ELb1ELi4ELb0EEEvNS_7KParamsE:
\tv_mfma_f32_16x16x4_f32 v[10:13], v29, v0, v[30:33]
\ts_cbranch_vccnz .LBB0_2
\tglobal_store_dwordx4 v[24:25], v[14:17], off
\ts_nop 7
.LBB0_2:
\ts_waitcnt vmcnt(0)
\tv_mul_f32_e32 v0, 0x3fb8aa3b, v13
\ts_endpgm
"""


def test_asmcheck_flags_an_mfma_result_read_before_its_wait_states():
    """The pattern hipcc 7.2 emitted in round 4 (an MFMA right in front of a taken branch, its result read two instructions into
    the target block): flagged; with the padding in place or when the reader is another MFMA: clean."""
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    key = "flow_kernelILi1ELi2ELi2ELb1ELi4ELb0E"
    n, bad = A.check_mfma_hazards_lines(_ASM_HAZARD.splitlines(), key)
    assert n == 1 and len(bad) == 1 and "reads the destination" in bad[0] and "after 2 wait states (needs 10)" in bad[0]
    ok = _ASM_HAZARD.replace("\ts_waitcnt vmcnt(0)", "\ts_waitcnt vmcnt(0)\n\ts_nop 7")
    assert A.check_mfma_hazards_lines(ok.splitlines(), key) == (1, [])
    # an intervening MFMA counts ONE wait state (as in the compiler's own rule), not its passes: still flagged
    mm = _ASM_HAZARD.replace("\ts_waitcnt vmcnt(0)", "\ts_waitcnt vmcnt(0)\n\tv_mfma_f32_16x16x4_f32 v[40:43], v29, v0, v[40:43]")
    assert "after 3 wait states (needs 10)" in A.check_mfma_hazards_lines(mm.splitlines(), key)[1][0]
    # the 4-pass fp16 shape needs 8 states before a VALU read (LLVM gfx950: passes + 4), one short is flagged
    x16 = _ASM_HAZARD.replace("v_mfma_f32_16x16x4_f32 v[10:13], v29, v0, v[30:33]", "v_mfma_f32_16x16x32_f16 v[10:13], v[26:29], v[0:3], v[30:33]")
    short = x16.replace("\ts_waitcnt vmcnt(0)", "\ts_waitcnt vmcnt(0)\n\ts_nop 4")
    assert "after 7 wait states (needs 8)" in A.check_mfma_hazards_lines(short.splitlines(), key)[1][0]
    assert A.check_mfma_hazards_lines(x16.replace("\ts_waitcnt vmcnt(0)", "\ts_waitcnt vmcnt(0)\n\ts_nop 5").splitlines(), key)[1] == []
    ok3 = _ASM_HAZARD.replace("\tv_mul_f32_e32 v0, 0x3fb8aa3b, v13", "\tv_mfma_f32_16x16x4_f32 v[10:13], v29, v0, v[10:13]")
    assert A.check_mfma_hazards_lines(ok3.splitlines(), key)[1] == []
    waw = _ASM_HAZARD.replace("\tv_mul_f32_e32 v0, 0x3fb8aa3b, v13", "\tv_mov_b32_e32 v12, 0")
    assert "overwrites" in A.check_mfma_hazards_lines(waw.splitlines(), key)[1][0]
    ld = _ASM_HAZARD.replace("\tv_mul_f32_e32 v0, 0x3fb8aa3b, v13", "\tds_read_b128 v[10:13], v5")            # a load INTO the register: no hazard
    assert A.check_mfma_hazards_lines(ld.splitlines(), key)[1] == []


def test_asmcheck_flags_a_lane_swap_of_a_freshly_written_register():
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    key = "flow_kernelILi1ELi2ELi2ELb1ELi4ELb0E"
    head = "_ZN12_GLOBAL__N_111flow_kernelILi1ELi2ELi2ELb1ELi4ELb0EEEvNS_7KParamsE:\n"
    tail = "\ts_endpgm\n"
    bad = head + "\tv_mul_f32_e32 v16, v16, v17\n\tv_mov_b32_e32 v3, v4\n\tv_permlane16_swap_b32_e32 v16, v17\n" + tail
    n, msgs = A.check_swap_hazards_lines(bad.splitlines(), key)
    assert n == 1 and len(msgs) == 1 and "1 wait states earlier (needs 2)" in msgs[0]
    ok = bad.replace("\tv_mov_b32_e32 v3, v4\n", "\tv_mov_b32_e32 v3, v4\n\ts_nop 0\n")
    assert A.check_swap_hazards_lines(ok.splitlines(), key) == (1, [])
    # through a taken branch (one state) as well; a swap's own results feeding the next swap count too
    br = head + "\tv_mul_f32_e32 v16, v16, v17\n\ts_cbranch_vccnz .LBB0_2\n\ts_nop 7\n.LBB0_2:\n\tv_permlane32_swap_b32_e32 v16, v17\n" + tail
    assert len(A.check_swap_hazards_lines(br.splitlines(), key)[1]) == 1
    chain = head + "\tv_permlane32_swap_b32_e32 v16, v17\n\tv_permlane16_swap_b32_e32 v17, v18\n" + tail
    assert len(A.check_swap_hazards_lines(chain.splitlines(), key)[1]) == 1


def test_build_refuses_to_ship_when_mfma_results_are_consumed_too_early(tmp_path, monkeypatch):
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    from bsdf_diffusion_sampling_amd import _lib
    assert _lib._check_asm_mfma.__doc__
    monkeypatch.setattr(_lib, "_check_asm_mfma", lambda path: {"flow_kernel<doctored>": ["`v_mul_f32 v0, v13` reads the destination of "
                                                                                        "`v_mfma_f32_16x16x4_f32 v[10:13]` after 2 wait states (needs 10)"]})
    out = str(tmp_path / "libbsdfd_never.so")
    with pytest.raises(RuntimeError, match="refusing to ship"):
        _lib.build(force=True, lib_path=out)
    assert not os.path.exists(out)


def _product_asm():
    """Device assembly of the product build (kept by _lib.build() under build/asm/)."""
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    from bsdf_diffusion_sampling_amd import _lib
    paths = _lib.cached_asm_paths()   # None unless the cache carries the hash of the current kernel sources
    if paths is None:
        _lib.build(force=True, lib_path=_lib.DEFAULT_LIB_PATH)
        paths = _lib.cached_asm_paths()
    assert paths is not None, "build() did not leave the verified assembly of the current sources under build/asm/"
    return paths


def test_assembly_census_fails_closed(tmp_path):
    """`_check_asm('/tmp/empty.s')` used to be "no violations".  The census (`_asmcheck.verify_census`) is
    what `_lib.build()` now holds the assembly to before it trusts "0 violations": the product build passes it; an empty file,
    renamed kernel labels, asynchronous reads under another mnemonic, a kernel without recognisable MFMAs, missing metadata
    and scratch memory are each reported."""
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    paths = _product_asm()
    assert A.verify_census(paths, "async") == []
    exp = A.expected_flow_kernels("async")
    assert len(exp) == 64 and sum(1 for v in exp.values() if v["async"]) == 8      # 54 in csrc/bsdfd.hip + 10 in csrc/flow32.hip
    assert all((v["async"], v["waits"]) == (0, 0) for v in A.expected_flow_kernels("plain").values())
    assert sum(1 for v in exp.values() if v.get("sel")) == 3 + 7                    # the packed-fp16 sigmoids (inline-asm SDWA halves)
    empty = tmp_path / "empty.s"
    empty.write_text("")
    assert len(A.verify_census([str(empty)], "async")) == 64                        # (a) nothing found
    text = open(paths[0]).read()
    renamed = tmp_path / "renamed.s"
    renamed.write_text(text.replace("flow_kernel", "flowkernel"))
    got = A.verify_census([str(renamed), paths[1]], "async")
    assert len(got) == 54 and all("not found" in m for m in got)                   # (b) labels the parser does not know
    spelled = tmp_path / "spelled.s"
    spelled.write_text(text.replace("ds_read_b128", "ds_load_b128"))
    got = A.verify_census([str(spelled), paths[1]], "async")
    assert len(got) == 8 and all("0 asynchronous ds_read_b128" in m for m in got)  # (c) the reads it must verify are invisible
    assert A.verify_census([str(spelled)], "async", only="flow_kernelI") == got     # ... which sends build() to the fallback variant
    nomfma = tmp_path / "nomfma.s"
    nomfma.write_text(text.replace("v_mfma_", "v_wmma_"))
    assert sum("no MFMA instruction recognised" in m for m in A.verify_census([str(nomfma), paths[1]], "async")) == 54
    nometa = tmp_path / "nometa.s"
    nometa.write_text(text.replace(".vgpr_count:", ".vgprs:"))
    assert sum("metadata not found" in m for m in A.verify_census([str(nometa), paths[1]], "async")) == 54
    scratch = tmp_path / "scratch.s"
    scratch.write_text(text.replace(".private_segment_fixed_size: 0", ".private_segment_fixed_size: 68", 1))
    got = A.verify_census([str(scratch), paths[1]], "async")
    assert len(got) == 1 and "68 B of scratch" in got[0]
    nosel = tmp_path / "nosel.s"                                                    # (d) destination selects under another spelling
    nosel.write_text(open(paths[1]).read().replace("dst_sel:WORD_1", "dstsel:WORD_1"))
    got = A.verify_census([paths[0], str(nosel)], "async")
    assert len(got) == 3 and all("0 destination-select writes" in m for m in got)
    nosel.write_text(text.replace("dst_sel:WORD_1", "dstsel:WORD_1"))
    got = A.verify_census([str(nosel), paths[1]], "async")
    assert len(got) == 7 and all("0 destination-select writes" in m for m in got)
    extra = tmp_path / "extra.s"
    extra.write_text(text.replace("flow_kernelILi0ELi2ELi2ELb1ELi3ELb0EE", "flow_kernelILi0ELi2ELi2ELb1ELi5ELb0EE"))
    got = A.verify_census([str(extra), paths[1]], "async")
    assert any("unexpected flow kernel" in m for m in got) and any("not found" in m for m in got)


def test_asmcheck_mfma_operands_in_agprs_and_as_matrix_inputs():
    """an MFMA whose destination the parser does not understand is a finding, not a skip; AGPR destinations are
    tracked; a result consumed as SrcA / SrcB of a later MFMA needs the wait states (only an unchanged SrcC is interlocked)."""
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    key = "flow_kernelILi1ELi2ELi2ELb1ELi4ELb0E"
    head = "_ZN12_GLOBAL__N_111flow_kernelILi1ELi2ELi2ELb1ELi4ELb0EEEvNS_7KParamsE:\n"
    tail = "\ts_endpgm\n"
    weird = head + "\tv_mfma_f32_16x16x32_f16 acc[0:3], v[26:29], v[0:3], 0\n" + tail
    n, bad = A.check_mfma_hazards_lines(weird.splitlines(), key)
    assert n == 1 and len(bad) == 1 and "not understood" in bad[0]
    agpr = head + "\tv_mfma_f32_16x16x32_f16 a[0:3], v[26:29], v[0:3], 0\n\tv_accvgpr_read_b32 v5, a2\n" + tail
    n, bad = A.check_mfma_hazards_lines(agpr.splitlines(), key)
    assert n == 1 and len(bad) == 1 and "after 0 wait states (needs 8)" in bad[0]
    assert A.check_mfma_hazards_lines(agpr.replace("\tv_accvgpr", "\ts_nop 7\n\tv_accvgpr").splitlines(), key) == (1, [])
    src_b = head + "\tv_mfma_f32_16x16x32_f16 v[10:13], v[26:29], v[0:3], 0\n\tv_mfma_f32_16x16x32_f16 v[40:43], v[26:29], v[10:13], 0\n" + tail
    n, bad = A.check_mfma_hazards_lines(src_b.splitlines(), key)
    assert n == 2 and len(bad) == 1 and "as a matrix operand after 0 wait states (needs 8)" in bad[0]
    partial_c = src_b.replace("v[40:43], v[26:29], v[10:13], 0", "v[12:15], v[26:29], v[30:33], v[12:15]")
    assert "as a matrix operand" in A.check_mfma_hazards_lines(partial_c.splitlines(), key)[1][0]
    same_c = src_b.replace("v[40:43], v[26:29], v[10:13], 0", "v[10:13], v[26:29], v[30:33], v[10:13]")
    assert A.check_mfma_hazards_lines(same_c.splitlines(), key) == (2, [])
    # a register the next MFMA has rewritten belongs to THAT MFMA: the first one's walk does not claim it any more
    taken = head + ("\tv_mfma_f32_16x16x4_f32 v[56:59], v1, v2, 0\n\tv_mfma_f32_16x16x4_f32 v[54:57], v3, v4, v[56:59]\n"
                    "\tv_mfma_f32_16x16x4_f32 v[54:57], v5, v6, v[54:57]\n\ts_nop 7\n\ts_nop 1\n\tv_mov_b32_e32 v0, v55\n") + tail
    assert A.check_mfma_hazards_lines(taken.splitlines(), key) == (3, [])


def test_asmcheck_forwarding_hazards_of_transcendentals_and_destination_selects():
    """gfx940-class forwarding hazards (LLVM checkVALUHazards): a non-transcendental VALU reading a transcendental's result, and any
    VALU reading a register written through a destination select, must be one wait state behind it.  The packed-fp16 sigmoids of
    csrc/flow32.hip are inline asm the compiler's hazard recogniser cannot see into: the build checks every kernel."""
    from bsdf_diffusion_sampling_amd import _asmcheck as A
    head, tail = "_Z3toyflow_kernelX:\n", "\ts_endpgm\n"
    def chk(body):
        return A.check_forwarding_hazards_lines((head + body + tail).splitlines(), "flow_kernelX")
    n, bad = chk("\tv_exp_f32_e32 v1, v0\n\tv_add_f32_e32 v2, 1.0, v1\n")
    assert n == 0 and len(bad) == 1 and "a transcendental" in bad[0]
    assert chk("\tv_exp_f32_e32 v1, v0\n\ts_nop 0\n\tv_add_f32_e32 v2, 1.0, v1\n") == (0, [])
    assert chk("\tv_exp_f32_e32 v1, v0\n\tv_mov_b32_e32 v9, v8\n\tv_add_f32_e32 v2, 1.0, v1\n") == (0, [])
    assert chk("\tv_exp_f32_e32 v1, v0\n\tv_rcp_f32_e32 v2, v1\n") == (0, [])             # transcendental -> transcendental: exempt
    sdwa = "\tv_exp_f16_sdwa v7, v0 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
    n, bad = chk(sdwa + "\tv_rcp_f16_e32 v8, v7\n")                                       # ... but not behind a destination select
    assert n == 1 and len(bad) == 1 and "destination-select write" in bad[0]
    n, bad = chk(sdwa + "\tv_pk_mul_f16 v8, v7, v9\n")
    assert n == 1 and len(bad) == 1
    assert chk(sdwa + "\ts_nop 0\n\tv_pk_mul_f16 v8, v7, v9\n") == (1, [])
    n, bad = chk(sdwa + sdwa.replace("WORD_1", "WORD_0"))                                  # the preserved half is a read of the destination
    assert n == 2 and len(bad) == 1
    # on a taken branch too
    n, bad = chk("\tv_exp_f32_e32 v1, v0\n\ts_cbranch_scc1 .LBB0_2\n\tv_mov_b32_e32 v3, v4\n.LBB0_2:\n\tv_add_f32_e32 v2, 1.0, v1\n")
    assert len(bad) == 0      # the branch itself is the wait state
    n, bad = chk("\tv_exp_f32_e32 v1, v0\n\tv_readlane_b32 s0, v1, 3\n")
    assert len(bad) == 1
    # the shipped kernels: the packed-fp16 blocks are found, and nothing in any kernel (compiler-generated code included) is short
    total = 0
    for path in _product_asm():
        for k, (n, bad) in A.check_file_forwarding(path).items():
            assert bad == [], (k, bad[:2])
            total += n
    assert total == (160 + 32 + 48) + (24 + 16 + 32 + 32 + 16 + 96 + 32)     # csrc/flow32.hip + the 7 f16 samples-only kernels of csrc/bsdfd.hip


def test_build_refuses_an_unverifiable_compilation_unless_overridden(tmp_path, monkeypatch, capsys):
    """The census failing (here: a doctored verdict) aborts the build and writes every finding next to the library;
    BSDFD_ALLOW_UNVERIFIED_BUILD=1 ships it, marked in the build info and in bsdfd_version()."""
    import ctypes as C
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    from bsdf_diffusion_sampling_amd import _lib
    real = _lib._census
    monkeypatch.setattr(_lib, "_census", lambda paths, variant, only=None: real(paths, variant, only=only) if only else
                        ["flow kernel flow_kernelILi0ELi2ELi2ELb1ELi3ELb0EE not found in the assembly"])
    out = str(tmp_path / "libbsdfd_unverified.so")
    with pytest.raises(RuntimeError, match="refusing to ship"):
        _lib.build(force=True, lib_path=out)
    assert not os.path.exists(out) and "not found in the assembly" in open(out + ".asmcheck.txt").read()
    monkeypatch.setenv("BSDFD_ALLOW_UNVERIFIED_BUILD", "1")
    assert _lib.build(force=True, lib_path=out) == out
    assert _lib.build_info(out)["unverified"] is True and "SHIPPING IT ANYWAY" in capsys.readouterr().out
    import torch  # noqa: F401
    L = C.CDLL(out)
    L.bsdfd_version.restype = C.c_char_p
    assert b"UNVERIFIED BUILD" in L.bsdfd_version()
    assert _lib.build_info().get("unverified") is False and b"UNVERIFIED" not in _lib.lib().bsdfd_version()


def test_compiler_only_build(tmp_path, monkeypatch, capsys):
    """BSDFD_COMPILER_ONLY_BUILD=1 ("a ROCm bump will stop every build until someone updates the parser; there is
    no compiler-only fallback for act_pack8"): both flow translation units are compiled without the inline-asm LDS reads and without
    the SDWA sigmoids, nothing is parsed — the checkers are never called — and the library says what it is."""
    import ctypes as C
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    from bsdf_diffusion_sampling_amd import _lib

    def never(*a, **k):
        raise AssertionError("the compiler-only build must not call the assembly checkers")
    for seam in ("_check_asm", "_check_asm_mfma", "_census"):
        monkeypatch.setattr(_lib, seam, never)
    monkeypatch.setenv("BSDFD_COMPILER_ONLY_BUILD", "1")
    out = str(tmp_path / "libbsdfd_compiler_only.so")
    assert _lib.build(force=True, lib_path=out) == out
    info = _lib.build_info(out)
    assert info["compiler_only"] is True and info["variant"] == "plain" and info["unverified"] is False
    assert info["inline_asm_constructs_left"] == {"ds_read_b128 inside inline asm": 0, "_sdwa inside inline asm": 0}
    assert "BSDFD_COMPILER_ONLY_BUILD=1" in capsys.readouterr().out
    import torch  # noqa: F401  (the HIP runtime the library links against)
    L = C.CDLL(out)
    L.bsdfd_version.restype = C.c_char_p
    v = L.bsdfd_version()
    assert b"COMPILER-ONLY BUILD" in v and b"compiler-written fp16 sigmoids" in v and b"fallback" in v
    for name in _lib.EXPORTS:
        getattr(L, name)
    # the product library of this tree is untouched by it
    assert _lib.build_info().get("compiler_only") in (False, None) and b"COMPILER-ONLY" not in _lib.lib().bsdfd_version()


def test_build_falls_back_to_compiler_managed_lds_reads_when_the_asm_check_fails(tmp_path, monkeypatch, capsys):
    """_lib.build() verifies the assembly of ITS OWN compilation of csrc/bsdfd.hip and, when an instruction touches the
    destination of an asynchronous LDS read before its wait, rebuilds with -DBSDFD_NO_ASYNC_LDS instead of shipping a library
    that could multiply with stale weights.  The check is fed a doctored verdict for the first
    compilation; the library that comes out must be the fallback variant and say so."""
    import ctypes as C
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("needs hipcc")
    from bsdf_diffusion_sampling_amd import _lib
    real, calls = _lib._check_asm, []

    def doctored(path):
        calls.append(open(path).read().count("ds_read_b128"))
        if len(calls) == 1:
            assert real(path) == {}          # this toolchain's real build is clean ...
            return {"flow_kernel<doctored>": ["line 1: `v_mov_b32 v50, v11` touches v11, the destination of the asynchronous read at line 0"]}
        return real(path)                    # ... and so is the fallback build (no asynchronous reads to check)
    monkeypatch.setattr(_lib, "_check_asm", doctored)
    out = str(tmp_path / "libbsdfd_fallback_test.so")
    assert _lib.build(force=True, lib_path=out) == out
    info = _lib.build_info(out)
    assert len(calls) == 2 and info["variant"] == "plain" and "flow_kernel<doctored>" in info["violations"]
    assert "rebuilding the flow kernels with -DBSDFD_NO_ASYNC_LDS" in capsys.readouterr().out
    import torch  # noqa: F401  (the HIP runtime the library links against)
    L = C.CDLL(out)
    L.bsdfd_version.restype = C.c_char_p
    assert b"fallback" in L.bsdfd_version()
    # the product library of this tree, built by the same routine, is the asynchronous variant
    assert _lib.build_info().get("variant") == "async" and b"asynchronous LDS reads" in _lib.lib().bsdfd_version()


def test_host_code_is_a_translation_unit_outside_the_kernel_fingerprint():
    """The handle, run() and every entry point live in csrc/host.hip: built and tracked as a dependency like every translation
    unit, but not hashed by `kernel_source_sha256()` — an edit to an error message or an entry point cannot change an instruction
    of a kernel and must not invalidate the committed profiles.  The fingerprinted files hold no host entry point at all."""
    from bsdf_diffusion_sampling_amd import _lib
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    host, hdr = os.path.join(csrc, "host.hip"), os.path.join(csrc, "flow_kernels.h")
    assert host in _lib.SRC_PATHS and host in _lib.DEP_PATHS and host not in _lib.KERNEL_SOURCES and os.path.exists(host)
    assert hdr in _lib.DEP_PATHS and hdr not in _lib.SRC_PATHS and os.path.exists(hdr)
    assert len(_lib.KERNEL_SOURCES) == 3
    for f in _lib.KERNEL_SOURCES:
        assert 'extern "C"' not in open(f).read(), f


def test_committed_profiles_match_the_kernel_source():
    """bench.py looks `roofline.traffic` (PMC passes) and the instruction-issue model (ISA of the build) up in profiles/*.json
    and withholds them when csrc/bsdfd.hip has changed since they were taken ("a kernel change without a profile
    refresh would silently carry stale figures").  The committed tree must never be in that state."""
    import json
    from bsdf_diffusion_sampling_amd import _lib
    sha = _lib.kernel_source_sha256()
    for f in ("isa_mix_latest.json", "pmc_latest.json"):
        meta = json.load(open(os.path.join(ROOT, "profiles", f))).get("_meta", {})
        assert meta.get("kernel_source_sha256") == sha, f"profiles/{f} was taken with other flow-kernel sources: re-run tools/profile.sh / tools/isa_mix.py --profile"
    sys.path.insert(0, ROOT)
    import bench
    for wl in ("disk_1Mi_T8", "spherical_16Mi_T8"):
        entry, prov = bench.profile_lookup("pmc_latest.json", wl)
        assert prov["status"] == "current" and entry["hbm_bytes_per_launch"] > 0
        entry, prov = bench.isa_model(wl)
        assert prov["status"] == "current" and entry["n_mfma"] > 0
