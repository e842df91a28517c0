"""GPU: the part of the launchers' shared host contract that needs a device (csrc/rows.h: launch_checks, launch_rows;
csrc/material_table.h: launch) — the twin of tests/test_launch_contract_cpu.py.  For each of the five ground-truth families: the
empty call is OK whatever the pointers, the family's too-large N is refused before a launch, and one ragged call — 257 rows, a
full block and one row; for the tables, waves of one id and waves of mixed ids — returns the bits of the same rows of a 512-row
call (one thread per row: a row's result does not depend on the launch it is part of)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_launch_contract_cpu import FAMILIES, misuse  # noqa: E402

N, RAGGED = 512, 257
TINT = (0.9, 0.2, 0.4)
SENTINEL = 123.25
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chm_orange_rgb.bsdf")
# the first N each family refuses: a grid of 2^31 blocks of 256 (single material), a thread index of 2^32 (tables)
TOO_LARGE = {"measured": 0x7fffffff * 256 + 1, "dielectric": 0x7fffffff * 256 + 1, "principled": 0x7fffffff * 256 + 1,
             "measured table": 0xffffffff - 254, "analytic table": 0xffffffff - 254}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from bsdf_diffusion_sampling_amd import measured_synth as F
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, RoughDielectric, reference_bsdf
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    d = tmp_path_factory.mktemp("launch_contract")
    m0, m2 = MeasuredBSDF(GOLDEN_FILE), MeasuredBSDF(F.write_anisotropic(str(d / "aniso_synth_rgb.bsdf")))
    diel, prin = RoughDielectric(0.3), reference_bsdf(13)
    g = np.random.default_rng(31)
    to =lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()
    wi, wo, wl = (g.normal(size=(N, 3)) for _ in range(3))
    for v in (wi, wo, wl):
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        up = g.uniform(size=N) < 0.8                      # most lanes above the surface, where the measured model lives
        v[up, 2] = np.abs(v[up, 2])
    pdf = g.uniform(0.05, 5.0, size=N)
    pdf[g.uniform(size=N) < 0.05] = 1e-3                  # fireflies
    # waves 0, 1, 3 carry one id (wave 3: the slot without ground truth), wave 2 and everything from row 256 on an id per lane
    ids = np.concatenate([np.full(64, 0), np.full(64, 2), g.integers(-1, 4, size=64), np.full(64, 1), g.integers(-1, 4, size=N - 256)])
    return dict(objects={"measured": m0, "dielectric": diel, "principled": prin,
                         "measured table": MeasuredTable([m0, None, m2]), "analytic table": AnalyticTable([prin, None, diel])},
                wi=to(wi), wo=to(wo), wl=to(wl), u=to(g.random((N, 3))), pdf=to(pdf),
                active=torch.from_numpy(g.uniform(size=N) < 0.8).cuda(), ids=torch.from_numpy(ids.astype(np.int64)).cuda())


def outputs(world, family, n):
    """Every output of the family's four calls on the first ``n`` rows: {name: tensor}."""
    obj = world["objects"][family]
    wi, wo, wl, pdf, act = (world[k][:n] for k in ("wi", "wo", "wl", "pdf", "active"))
    u = world["u"][:n, :obj.U_COLS].contiguous()
    front = (world["ids"][:n],) if "table" in family else ()
    out = {}
    if front:
        out["eval"], out["eval wl"] = obj.eval_t(*front, wi, wo, wl, tint=TINT)
    else:
        out["eval"] = obj.eval_t(wi, wo, tint=TINT)
    out["weight"], out["weight pdf"] = obj.sample_weight(*front, wi, wo, pdf, tint=TINT, active=act)
    out["sample wo"], out["sample pdf"], out["sample weight"] = obj.sample_t(*front, wi, u, tint=TINT, active=act)
    out["pdf"] = obj.pdf_t(*front, wi, wo, active=act)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def full(world):
    """The 512-row calls, once."""
    return {family: outputs(world, family, N) for family in FAMILIES}


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_empty_call_is_ok_whatever_the_pointers(world, family):
    for name in FAMILIES[family][0]:
        rc, msg = misuse(name, world["objects"][family]._lead(), 0)
        assert rc == 0, (name, rc, msg)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_familys_too_large_n_is_refused_before_a_launch(world, family):
    from bsdf_diffusion_sampling_amd import _lib
    L, EINVAL = _lib.lib(), 1
    for name in FAMILIES[family][0]:
        fn = getattr(L, name)
        for n in (TOO_LARGE[family], 2 ** 40):
            bufs, args, seen_n = [], [world["objects"][family]._lead()], False
            for t in fn.argtypes[1:-1]:                   # small valid buffers behind every pointer, a huge N
                if t is C.c_int64:
                    args.append(0 if seen_n else n)
                    seen_n = True
                elif t is C.c_float:
                    args.append(3.5)
                elif t is C.c_void_p:
                    bufs.append(torch.full((64, 3), SENTINEL, device="cuda"))
                    args.append(C.c_void_p(bufs[-1].data_ptr()))
                else:
                    args.append(None)                     # tint
            rc = fn(*args, None)
            assert rc == EINVAL and L.bsdfd_last_error().decode() == "N too large for one launch", (name, n, rc, L.bsdfd_last_error())
            torch.cuda.synchronize()
            assert all(bool((b == SENTINEL).all()) for b in bufs), name      # a refused call writes nothing


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_ragged_call_returns_the_bits_of_the_same_rows_of_a_longer_one(world, full, family):
    got = outputs(world, family, RAGGED)
    assert sorted(got) == sorted(full[family])
    for k, want in full[family].items():
        assert got[k].shape[0] == RAGGED and torch.equal(bits(got[k]), bits(want[:RAGGED])), (family, k)
    # ... and the rows are worth comparing: ground truth that is neither zero nor NaN, and for a table the NaN of a row without
    ev = full[family]["eval"][:RAGGED]
    assert int((torch.isfinite(ev).all(1) & (ev > 0).any(1)).sum()) > RAGGED // 4
    assert bool(torch.isnan(ev[192:256]).all()) == ("table" in family)


@pytest.mark.parametrize("family", ["measured table", "analytic table"])
def test_a_ragged_row_list_returns_the_bits_of_its_rows_and_keeps_the_others(world, full, family):
    obj, n = world["objects"][family], RAGGED
    some = np.random.default_rng(5).permutation(n - 1)[:128]
    # 129 distinct rows in no order — two waves and one lane — with the one row beyond the first block among them
    listed = torch.from_numpy(np.concatenate([some[:64], [n - 1], some[64:]]).astype(np.int64)).cuda()
    out_o, out_l = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda")
    obj.eval_t(world["ids"][:n], world["wi"][:n], world["wo"][:n], world["wl"][:n], tint=TINT, out_o=out_o, out_l=out_l, rows=listed)
    torch.cuda.synchronize()
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[listed] = False
    for got, want in ((out_o, full[family]["eval"]), (out_l, full[family]["eval wl"])):
        assert torch.equal(bits(got[listed]), bits(want[:n][listed])) and bool((got[rest] == SENTINEL).all())


def test_an_object_of_another_device_is_refused(world):
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: there is no other device to call from")
    with torch.cuda.device(1):
        for family, owner in (("measured", "measured handle"), ("measured table", "measured table"), ("analytic table", "analytic table")):
            for name in FAMILIES[family][0]:
                rc, msg = misuse(name, world["objects"][family]._lead(), 64)
                assert rc == 1 and msg == owner + " belongs to another device", (name, rc, msg)
