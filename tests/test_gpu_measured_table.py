"""GPU: eval() of a mixed-material wavefront in one launch (csrc/measured_table.hip, measured.MeasuredTable) returns THE BITS of
the single-material evaluator (csrc/measured.hip) on each material's rows, and NaN on the rows without ground truth.

Reference = MeasuredBSDF.eval_t / sample_weight of every material on ALL rows, once per module (one thread per row: a row's
result does not depend on the launch it is part of); a case picks, per row, the reference of the row's id.  Bit patterns are
compared (int32 views), never floats: NaN rows defeat float equality, and a tolerance would hide a contraction difference.
(There was one: with hipcc's default, fused multiply-adds are formed wherever the optimiser finds a product next to a sum, which
depends on the code around an inlined copy of measured_f — 45 % of the rows came out 2-15 ulp apart, up to 1036 ulp near the
specular peak; csrc/measured_dev.h now has them formed per source expression.)  The table kernel is also held to the fp64 oracle
directly, with the bounds tests/test_gpu_measured.py holds the single-material kernel to."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bsdf_diffusion_sampling_amd import measured_synth as F  # noqa: E402
from oracle import measured_oracle as M  # noqa: E402

N_MAX = 20001                       # 78 full blocks and a 33-row tail: one partial wave in the last block
SIZES = [0, 1, 63, 64, 65, 257, N_MAX]
TINT = (0.9, 0.8, 0.7)
N_SLOTS = 4                         # real isotropic | synthetic anisotropic | None | synthetic n_phi = 1, jacobian = 0
BOUNDS = {0: (2e-4, 5e-3), 1: (1e-4, 2e-3), 3: (1e-4, 2e-3)}   # (p99, max) of |got - oracle| / (max_c |oracle| + 1e-3): test_gpu_measured.py
SENTINEL = 123.25
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chm_orange_rgb.bsdf")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    d = tmp_path_factory.mktemp("measured_table")
    entries = [MeasuredBSDF(GOLDEN_FILE), MeasuredBSDF(F.write_anisotropic(str(d / "aniso_synth_rgb.bsdf"))), None,
               MeasuredBSDF(F.write_isotropic(str(d / "iso_synth_rgb.bsdf")))]
    assert (entries[0].isotropic, entries[0].jacobian, entries[0].n_phi) == (True, True, 1)
    assert (entries[1].isotropic, entries[1].reduction, entries[1].jacobian) == (False, 4, True)
    assert (entries[3].isotropic, entries[3].jacobian, entries[3].n_phi, entries[3].n_theta) == (True, False, 1, 3)
    g = np.random.default_rng(20)
    n = N_MAX
    wi, wo, wl = F.dirs(g, n), F.dirs(g, n), F.dirs(g, n)
    k = n // 2                                            # half of the pairs near the specular direction
    wo[:k] = wi[:k] * [-1, -1, 1] + g.normal(size=(k, 3)) * 0.05
    wo[:k] /= np.linalg.norm(wo[:k], axis=1, keepdims=True)
    for v in (wi, wo, wl):                                # ~1 % of lower-hemisphere lanes in each
        v[g.uniform(size=n) < 0.01, 2] *= -1
    pdf = g.uniform(0.05, 5.0, size=n)
    pdf[g.uniform(size=n) < 0.05] = 1e-3                  # fireflies
    pdf[g.uniform(size=n) < 0.02] = 0.0
    active = g.uniform(size=n) < 0.8
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()
    w = dict(entries=entries, table=MeasuredTable(entries), wi=to(wi), wo=to(wo), wl=to(wl), pdf=to(pdf),
             active=torch.from_numpy(active).cuda())
    w["ref_o"] = [None if e is None else e.eval_t(w["wi"], w["wo"], tint=TINT) for e in entries]
    w["ref_l"] = [None if e is None else e.eval_t(w["wi"], w["wl"], tint=TINT) for e in entries]
    w["ref_w"] = {masked: [None if e is None else e.sample_weight(w["wi"], w["wo"], w["pdf"], tint=TINT,
                                                                  active=w["active"] if masked else None) for e in entries]
                  for masked in (False, True)}
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(r).all()) for r in w["ref_o"] + w["ref_l"] if r is not None)
    # the fp64 oracle on the same fp32 directions, untinted: [material][direction] -> [N_MAX, 3] (None = no ground truth)
    wi64 = w["wi"].cpu().numpy().astype(np.float64)
    paths = [e and e.path for e in entries]
    w["oracle"] = [None if p is None else [M.MeasuredBSDF(p).eval(wi64, w[k].cpu().numpy().astype(np.float64)) for k in ("wo", "wl")]
                   for p in paths]
    return w


def make_ids(layout, n):
    """int64 [n] on the CPU.  "runs": 64-aligned runs of one id — every wave uniform: the four slots (the None slot among them),
    the floor's id and an id whose low 32 bits name a material — except wave 0 and wave 3, where ONE lane differs; "lanes": an id
    per lane — every wave divergent; "stray": "lanes" with ids outside the table sprinkled in."""
    g = np.random.default_rng(n + 1)
    if layout == "runs":
        pattern = np.array([0, 1, 2, 3, 1, N_SLOTS, 3, 0, 2**40 + 1, 2, -1], dtype=np.int64)
        ids = pattern[(np.arange(n) // 64) % len(pattern)]
        for lone in (40, 64 * 3 + 17):
            if lone < n:
                ids[lone] = 1 if ids[lone] != 1 else 0
        return torch.from_numpy(ids)
    ids = g.integers(0, N_SLOTS, size=n).astype(np.int64)
    if layout == "stray":
        for start, step, val in ((5, 37, -1), (11, 41, N_SLOTS), (17, 43, N_SLOTS + 7), (23, 47, 2**40 + 1), (0, 53, -2**40)):
            ids[start::step] = val
    return torch.from_numpy(ids)


def expected(refs, ids, n):
    """(values [n, ...] picked per row from the per-material references, has ground truth [n] bool)."""
    want = torch.full_like(refs[0][:n], float("nan"))
    gt = torch.zeros(n, dtype=torch.bool, device=want.device)
    for m, r in enumerate(refs):
        if r is not None:
            rows = ids == m
            want[rows] = r[:n][rows]
            gt |= rows
    return want, gt


def same_bits(got, want, gt, what=""):
    """Bit-identical where there is ground truth, NaN in every channel elsewhere."""
    assert got.shape == want.shape and got.dtype == torch.float32
    if not torch.equal(got[gt].view(torch.int32), want[gt].view(torch.int32)):
        d = (got[gt].view(torch.int32).long() - want[gt].view(torch.int32).long()).abs().reshape(int(gt.sum()), -1)
        rows = gt.nonzero()[:, 0][(d > 0).any(1)][:8].tolist()
        pytest.fail(f"{what}: {int((d > 0).any(1).sum())} of {int(gt.sum())} ground-truth rows differ, e.g. rows {rows}; "
                    f"largest distance {int(d.max())} ulp")
    assert bool(torch.isnan(got[~gt]).all()), f"{what}: a row without ground truth was not written as NaN"


def within_oracle_bound(world, got, ids, direction, tint, only=None):
    """The bound of tests/test_gpu_measured.py, per material, on the rows the case gives that material (and `only` selects);
    zeros in the same rows."""
    n = got.shape[0]
    got = got.cpu().numpy().astype(np.float64)
    ids = ids.cpu().numpy()
    for m, (p99, worst) in BOUNDS.items():
        rows = ids == m
        if only is not None:
            rows &= only.cpu().numpy()
        if not rows.any():
            continue
        want = world["oracle"][m][direction][:n][rows] * np.asarray(tint, dtype=np.float64)
        g = got[rows]
        assert ((g == 0).all(1) == (want == 0).all(1)).all(), f"material {m}: zeros (lower hemispheres) in other rows than the oracle's"
        err = np.abs(g - want) / (np.abs(want).max(1, keepdims=True) + 1e-3)
        if rows.sum() >= 100:
            assert np.percentile(err, 99) < p99, (m, np.percentile(err, 99))
        assert err.max() < worst, (m, err.max())


@pytest.mark.parametrize("layout", ["runs", "lanes", "stray"])
@pytest.mark.parametrize("n", SIZES)
def test_eval_table_returns_the_bits_of_the_single_material_evaluator(world, n, layout):
    ids = make_ids(layout, n).cuda()
    wi, wo, wl = (world[k][:n] for k in ("wi", "wo", "wl"))
    want_o, gt = expected(world["ref_o"], ids, n)
    want_l, _ = expected(world["ref_l"], ids, n)
    if n >= 257:   # the case is not vacuous: rows with and rows without ground truth
        assert int(gt.sum()) > 0 and int((~gt).sum()) > 0
    # both directions in one launch, into sentinel-filled outputs (an unwritten row would show)
    out_o, out_l = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda")
    r = world["table"].eval_t(ids, wi, wo, wl, tint=TINT, out_o=out_o, out_l=out_l)
    assert r[0] is out_o and r[1] is out_l
    same_bits(out_o, want_o, gt, "f_o")
    same_bits(out_l, want_l, gt, "f_l")
    within_oracle_bound(world, out_o, ids, 0, TINT)
    within_oracle_bound(world, out_l, ids, 1, TINT)
    # wo alone, outputs allocated by the call
    f = world["table"].eval_t(ids, wi, wo, tint=TINT)
    assert isinstance(f, torch.Tensor)
    same_bits(f, want_o, gt, "f_o alone")
    # wl given, out_l not
    f_o, f_l = world["table"].eval_t(ids, wi, wo, wl, tint=TINT)
    same_bits(f_o, want_o, gt, "f_o")
    same_bits(f_l, want_l, gt, "f_l")


def test_uniform_and_divergent_waves_give_a_row_the_same_bits(world):
    """A row's value depends on its own id, not on what its wave-mates carry: the same rows in uniform waves ("runs") and, after
    a permutation of the rows, in divergent ones."""
    n = N_MAX
    ids = make_ids("runs", n).cuda()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    wi, wo = world["wi"], world["wo"]
    a = world["table"].eval_t(ids, wi, wo, tint=TINT)
    b = world["table"].eval_t(ids[perm].contiguous(), wi[perm].contiguous(), wo[perm].contiguous(), tint=TINT)
    assert torch.equal(a[perm].view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", ["runs", "stray"])
def test_eval_table_without_tint_on_a_side_stream_and_twice_into_the_same_outputs(world, layout):
    n = N_MAX
    ids = make_ids(layout, n).cuda()
    ref_o = [None if e is None else e.eval_t(world["wi"], world["wo"]) for e in world["entries"]]   # tint = None -> 1
    ref_l = [None if e is None else e.eval_t(world["wi"], world["wl"]) for e in world["entries"]]
    want_o, gt = expected(ref_o, ids, n)
    want_l, _ = expected(ref_l, ids, n)
    out_o, out_l = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        world["table"].eval_t(ids, world["wi"], world["wo"], world["wl"], out_o=out_o, out_l=out_l)
    side.synchronize()
    same_bits(out_o, want_o, gt, "side stream f_o")
    same_bits(out_l, want_l, gt, "side stream f_l")
    # a second call with other ids into the SAME outputs: nothing of the first call's contents survives
    ids2 = torch.roll(ids, 97)
    want_o2, gt2 = expected(ref_o, ids2, n)
    want_l2, _ = expected(ref_l, ids2, n)
    world["table"].eval_t(ids2, world["wi"], world["wo"], world["wl"], out_o=out_o, out_l=out_l)
    same_bits(out_o, want_o2, gt2, "second call f_o")
    same_bits(out_l, want_l2, gt2, "second call f_l")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["runs", "lanes", "stray"])
@pytest.mark.parametrize("n", [0, 65, N_MAX])
def test_sample_weight_table(world, n, layout, masked):
    ids = make_ids(layout, n).cuda()
    refs = world["ref_w"][masked]
    want_w, gt = expected([None if r is None else r[0] for r in refs], ids, n)
    want_p, _ = expected([None if r is None else r[1] for r in refs], ids, n)
    pdf = world["pdf"][:n]
    weight, p = world["table"].sample_weight(ids, world["wi"][:n], world["wo"][:n], pdf, tint=TINT,
                                             active=world["active"][:n] if masked else None)
    same_bits(weight, want_w, gt, "weight")
    assert torch.equal(p[gt].view(torch.int32), want_p[gt].view(torch.int32))
    assert torch.equal(p[~gt].view(torch.int32), pdf[~gt].view(torch.int32))      # no ground truth: pdf_sa passes through
    if n == N_MAX:   # the reference exercises the firefly rule and the masks
        fire = gt & (p == 0) & (pdf > 0)
        assert int(fire.sum()) > 0 and int((gt & (p > 0)).sum()) > 0
    with pytest.raises(ValueError, match="active must be"):                      # a CPU mask is refused, not copied across
        world["table"].sample_weight(ids, world["wi"][:n], world["wo"][:n], pdf, active=torch.ones(n, dtype=torch.bool))


def test_launch_calls_reject_bad_arguments(world):
    from bsdf_diffusion_sampling_amd import _lib
    L, t = _lib.lib(), world["table"]._table()
    ids = make_ids("lanes", 64).cuda()
    p = lambda x: C.c_void_p(x.data_ptr())
    wi, wo, wl, pdf = (world[k][:64] for k in ("wi", "wo", "wl", "pdf"))
    out, out2, out1 = torch.full((64, 3), SENTINEL, device="cuda"), torch.full((64, 3), SENTINEL, device="cuda"), torch.empty(64, device="cuda")

    def einval(rc, expect):
        assert rc == 1 and expect in L.bsdfd_last_error().decode(), (rc, L.bsdfd_last_error().decode())
    einval(L.bsdfd_measured_eval_table(t, p(ids), p(wi), p(wo), None, -1, None, p(out), None, None), "N must be >= 0")
    einval(L.bsdfd_measured_eval_table(t, None, p(wi), p(wo), None, 64, None, p(out), None, None), "null pointer")
    einval(L.bsdfd_measured_eval_table(t, p(ids), p(wi), p(wo), None, 64, None, None, None, None), "null pointer")
    einval(L.bsdfd_measured_eval_table(t, p(ids), p(wi), p(wo), p(wl), 64, None, p(out), None, None), "both NULL or both given")
    einval(L.bsdfd_measured_eval_table(t, p(ids), p(wi), p(wo), None, 64, None, p(out), p(out2), None), "both NULL or both given")
    einval(L.bsdfd_measured_sample_weight_table(t, p(ids), p(wi), p(wo), p(pdf), None, -5, None, 30.0, p(out), p(out1), None),
           "N must be >= 0")
    einval(L.bsdfd_measured_sample_weight_table(t, p(ids), p(wi), p(wo), None, None, 64, None, 30.0, p(out), p(out1), None),
           "null pointer")
    # N == 0 launches nothing, whatever the pointers
    assert L.bsdfd_measured_eval_table(t, None, None, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all())   # a rejected call writes nothing
    # an all-None table is refused by the library when the first launch creates it
    from bsdf_diffusion_sampling_amd.measured import MeasuredTable
    with pytest.raises(RuntimeError, match="at least one"):
        MeasuredTable([None, None]).eval_t(ids, wi, wo)
