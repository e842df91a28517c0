"""GPU: the analytic ground truth of a mixed-material wavefront in one launch (csrc/analytic_table.hip, analytic.AnalyticTable)
returns THE BITS of the single-material kernels (csrc/principled.hip, csrc/dielectric.hip) on each material's rows, and NaN on
the rows without ground truth.

Reference = the single-material call of every entry on ALL rows, once per module (one thread per row: a row's result does not
depend on the launch it is part of, which tests/test_gpu_principled.py holds); a case picks, per row, the reference of the row's
id.  The shapes are the smallest at which the dispatch can go wrong: 0, 1, 67 rows, three waves plus five rows, and the rows of
tests/test_gpu_principled.py (4096 random + 19 hand-placed); ids constant per wave, different in every lane, and drawn per lane
with ids outside the table among them.  The six entries put both kinds, a metal and a slot without ground truth into one wave."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dielectric_ref as D  # noqa: E402
import principled_ref as R  # noqa: E402

N = 4096
TINT = (0.9, 0.2, 0.4)
# a material the reference's list does not reach: coloured, isotropic, part subsurface, another interface
CUSTOM = dict(base_color=(0.8, 0.3, 0.1), roughness=0.4, anisotropic=0.0, metallic=0.2, spec_trans=0.5, eta=1.33, spec_tint=0.7,
              sheen=0.5, sheen_tint=0.6, flatness=0.3, clearcoat=0.5, clearcoat_gloss=0.2)
SLOTS = (13, None, 24, "custom", 2, 23)                   # reference_bsdf(idx), no ground truth, Principled(**CUSTOM)
M = len(SLOTS)
ALBEDO = ((0.1, 0.9, 0.9), (0.4, 0.8, 0.4), (0.9, 0.2, 0.4), (1.0, 1.0, 1.0), (0.0, 0.5, 0.25), (0.3, 0.7, 1.0))
SIZES = [0, 1, 67, 197, N + 19]
LAYOUTS = ["uniform", "divergent", "random"]
SENTINEL = 123.25
SEED = 13


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _hand_rows(eta):
    """(wi, wo, exactly_zero): the hand-placed pairs of tests/test_gpu_principled.py."""
    w = R.wi_of
    graze = w(1.55, 0.3)[0]
    inside = w(np.pi - 1.2, 0.7)[0]                               # from inside, beyond the critical angle of every material here
    tilted = w(0.4, 2.0)[0]
    rows = [
        ((0, 0, 1), (0, 0, 1), False), ((0, 0, 1), w(0.3, 1.0)[0], False), ((0, 0, 1), (0, 0, -1), False),   # the normal
        ((0, 0, 1), w(np.pi - 0.2, 1.0)[0], False), ((0, 0, -1), w(0.2, 1.0)[0], False),
        (tilted, (1, 0, 0), True), (tilted, (0.6, -0.8, 0), True),                                            # co == 0
        ((1, 0, 0), tilted, True), ((0, 1, 0), -tilted, True), ((1, 0, 0), (0, 1, 0), True),                  # ci == 0
        (inside, w(1.0, 0.7 + np.pi)[0], False), (inside, w(0.3, 0.7)[0], False), (inside, inside * [-1, -1, 1], False),
        (tilted, -tilted / eta, True), (graze, -graze / eta, True),                                           # degenerate half vector
        (-tilted, tilted * eta, True),
        (graze, graze * [-1, -1, 1], False), (graze, w(np.pi - 0.72, 0.3 + np.pi)[0], False), (graze, -graze, False),
    ]
    wi, wo, z = zip(*rows)
    return np.array(wi, np.float32), np.array(wo, np.float32), np.array(z)


def make_rows():
    """The fp32 inputs of tests/test_gpu_principled.py::make_rows for material 13 — (wi, wo, u) — and a second direction wl."""
    g = np.random.default_rng(SEED)
    r64 = R.Principled(dtype=np.float64, **R.reference_params(13))
    # sample(): both sides of the surface, grazing rows included, and the hand-placed incident directions
    hw_i, hw_o, _ = _hand_rows(float(r64.eta))
    wi = R.sphere_dirs(g, N)
    wi[: N // 8] = _unit(wi[: N // 8] * [1, 1, 0.05])        # an eighth of them within ~3 degrees of the horizon
    wi = np.concatenate([wi.astype(np.float32), hw_i])
    u = g.random((len(wi), 3)).astype(np.float32)
    # eval() / pdf(): half of the directions around where the model puts its mass (its own samples, blurred), half anywhere
    wo = R.sphere_dirs(g, len(wi))
    k = N // 2
    own = r64.sample(wi[:k], g.random((k, 3)))[0]
    hit = np.abs(own).sum(1) > 0                              # (a failed sample has no direction: that row stays uniform)
    wo[:k][hit] = _unit(own + g.normal(size=(k, 3)) * 0.5 * float(np.sqrt(r64.ax * r64.ay)))[hit]
    wo = wo.astype(np.float32)
    wo[N:] = hw_o
    wl = R.sphere_dirs(g, len(wi)).astype(np.float32)
    return wi, wo, u, wl


def make_ids(layout, n):
    """int64 [n] on the CPU.  "uniform": constant over each 64-row block — every wave carries one id, the slot without ground truth
    in its turn; "divergent": id = row % M — every wave holds all six; "random": drawn per row from -1 .. M — ids outside the table
    occur."""
    rows = np.arange(n, dtype=np.int64)
    if layout == "uniform":
        return torch.from_numpy((rows // 64) % M)
    if layout == "divergent":
        return torch.from_numpy(rows % M)
    return torch.from_numpy(np.random.default_rng(n + 1).integers(-1, M + 1, size=n).astype(np.int64))


def _models(dtype):
    """The numpy restatements of the six slots in ``dtype`` (None where there is no ground truth)."""
    out = []
    for s in SLOTS:
        if s is None:
            out.append(None)
        elif s == "custom":
            out.append(R.Principled(dtype=dtype, **CUSTOM))
        elif s >= 23:
            out.append(D.RoughDielectric({23: 0.2, 24: 0.3, 25: 0.5}[s], dtype=dtype))
        else:
            out.append(R.reference(s, dtype=dtype))
    return out


def single_material_calls(entries, w, tints):
    """Every call of every entry on ALL rows: {call: [per entry]}; ``tints[m]`` is entry m's tint (None: white)."""
    ref = {k: [] for k in ("o", "l", "w", "w_masked", "s", "s_masked", "p", "p_masked")}
    for m, e in enumerate(entries):
        if e is None:
            for k in ref:
                ref[k].append(None)
            continue
        t = tints[m]
        ref["o"].append(e.eval_t(w["wi"], w["wo"], tint=t))
        ref["l"].append(e.eval_t(w["wi"], w["wl"], tint=t))
        ref["w"].append(e.sample_weight(w["wi"], w["wo"], w["pdf"], tint=t))
        ref["w_masked"].append(e.sample_weight(w["wi"], w["wo"], w["pdf"], tint=t, active=w["active"]))
        ref["s"].append(e.sample_t(w["wi"], w["u"], tint=t))
        ref["s_masked"].append(e.sample_t(w["wi"], w["u"], tint=t, active=w["active"]))
        ref["p"].append(e.pdf_t(w["wi"], w["wo"]))
        ref["p_masked"].append(e.pdf_t(w["wi"], w["wo"], active=w["active"]))
    return ref


@pytest.fixture(scope="module")
def world():
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, Principled, reference_bsdf
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    entries = [None if s is None else Principled(**CUSTOM) if s == "custom" else reference_bsdf(s) for s in SLOTS]
    wi, wo, u, wl = make_rows()
    n = len(wi)
    g = np.random.default_rng(20)
    pdf = g.uniform(0.05, 5.0, size=n)
    pdf[g.uniform(size=n) < 0.1] = 1e-3                   # fireflies
    pdf[g.uniform(size=n) < 0.02] = 0.0
    w = dict(entries=entries, table=AnalyticTable(entries), tinted=AnalyticTable(entries, albedo=ALBEDO), n=n,
             wi=_cuda(wi), wo=_cuda(wo), wl=_cuda(wl), u=_cuda(u), pdf=_cuda(pdf.astype(np.float32)),
             active=torch.from_numpy(g.uniform(size=n) < 0.6).cuda())
    assert len(w["table"]) == M and n == SIZES[-1]
    w["ref"] = single_material_calls(entries, w, [TINT] * M)
    w["ref_white"] = single_material_calls(entries, w, [None] * M)
    # the effective tint of entry m: ONE fp32 product per channel, formed here in numpy's fp32
    eff = [tuple(float(v) for v in np.float32(TINT) * np.float32(a)) for a in ALBEDO]
    w["ref_albedo"] = single_material_calls(entries, w, eff)
    torch.cuda.synchronize()
    return w


def expected(refs, ids, n, part=None):
    """(values [n, ...] picked per row from the per-material references, has ground truth [n] bool)."""
    refs = [r if r is None or part is None else r[part] for r in refs]
    want = torch.full_like(next(r for r in refs if r is not None)[:n], float("nan"))
    gt = torch.zeros(n, dtype=torch.bool, device=want.device)
    for m, r in enumerate(refs):
        if r is not None:
            rows = ids == m
            want[rows] = r[:n][rows]
            gt |= rows
    return want, gt


def same_bits(got, want, gt, what=""):
    """``torch.equal`` where there is ground truth (no NaN occurs there), NaN in every channel elsewhere."""
    assert got.shape == want.shape and got.dtype == torch.float32, what
    assert not bool(torch.isnan(want[gt]).any()), what
    if not torch.equal(got[gt], want[gt]):
        d = (got[gt].view(torch.int32).long() - want[gt].view(torch.int32).long()).abs().reshape(int(gt.sum()), -1)
        rows = gt.nonzero()[:, 0][(d > 0).any(1)][:8].tolist()
        pytest.fail(f"{what}: {int((d > 0).any(1).sum())} of {int(gt.sum())} ground-truth rows differ, e.g. rows {rows}; "
                    f"largest distance {int(d.max())} ulp")
    assert bool(torch.isnan(got[~gt]).all()), f"{what}: a row without ground truth was not written as NaN"


def check_all_calls(w, table, ref, ids, n, tint, masked=False, what=""):
    """The four calls of ``table`` on the first n rows against ``ref``; -> has ground truth [n]."""
    wi, wo, wl, u, pdf = (w[k][:n] for k in ("wi", "wo", "wl", "u", "pdf"))
    act = w["active"][:n] if masked else None
    sfx = "_masked" if masked else ""
    want_o, gt = expected(ref["o"], ids, n)
    want_l, _ = expected(ref["l"], ids, n)
    f_o, f_l = table.eval_t(ids, wi, wo, wl, tint=tint)
    same_bits(f_o, want_o, gt, what + " f_o")
    same_bits(f_l, want_l, gt, what + " f_l")
    f = table.eval_t(ids, wi, wo, tint=tint)                      # wo alone
    assert isinstance(f, torch.Tensor)
    same_bits(f, want_o, gt, what + " f_o alone")
    weight, p = table.sample_weight(ids, wi, wo, pdf, tint=tint, active=act)
    same_bits(weight, expected(ref["w" + sfx], ids, n, 0)[0], gt, what + " weight")
    assert torch.equal(p[gt], expected(ref["w" + sfx], ids, n, 1)[0][gt]), what + " weight's pdf"
    assert torch.equal(p[~gt], pdf[~gt]), what + ": no ground truth, pdf_sa passes through"
    got = table.sample_t(ids, wi, u, tint=tint, active=act)
    for part, name in enumerate(("wo", "pdf", "weight")):
        same_bits(got[part], expected(ref["s" + sfx], ids, n, part)[0], gt, f"{what} sample {name}")
    same_bits(table.pdf_t(ids, wi, wo, active=act), expected(ref["p" + sfx], ids, n)[0], gt, what + " pdf")
    return gt


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_table_returns_the_bits_of_the_single_material_kernels(world, n, layout):
    ids = make_ids(layout, n).cuda()
    gt = check_all_calls(world, world["table"], world["ref"], ids, n, TINT, what=f"{layout} {n}")
    check_all_calls(world, world["table"], world["ref_white"], ids, n, None, what=f"{layout} {n} no tint")
    if n >= 197:   # the case is not vacuous: rows without ground truth, and rows of every entry (197 rows in runs of 64: of four)
        assert int((~gt).sum()) > 0 and all(int((ids == m).sum()) > 0 for m in range(4 if (n, layout) == (197, "uniform") else M))
    if n == SIZES[-1]:
        if layout == "random":
            assert int((ids < 0).sum()) > 0 and int((ids >= M).sum()) > 0
        # the references exercise what they are meant to: the firefly rule, failed samples, both sides of the surface
        p = world["table"].sample_weight(ids, world["wi"], world["wo"], world["pdf"], tint=TINT)[1]
        assert int((gt & (p == 0) & (world["pdf"] > 0)).sum()) > 0 and int((gt & (p > 0)).sum()) > 0
        wo, pdf, _ = world["table"].sample_t(ids, world["wi"], world["u"])
        assert int((gt & (pdf == 0)).sum()) > 0 and int((gt & (pdf > 0) & (wo[:, 2] * world["wi"][:, 2] < 0)).sum()) > 0


def test_uniform_and_divergent_waves_give_a_row_the_same_bits(world):
    """A row's value depends on its own id, not on what its wave-mates carry: rows in uniform waves and, after a permutation of
    the rows, the same rows with the same ids in divergent ones."""
    n, t = world["n"], world["table"]
    ids = make_ids("uniform", n).cuda()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    wi, wo, wl, u, pdf = (world[k] for k in ("wi", "wo", "wl", "u", "pdf"))
    ids_p, wi_p, wo_p, wl_p, u_p, pdf_p = (x[perm].contiguous() for x in (ids, wi, wo, wl, u, pdf))
    waves = ids_p[: 64 * (n // 64)].reshape(-1, 64)
    assert bool((waves.min(1).values != waves.max(1).values).all())  # every full wave is divergent now
    bits = lambda x: x.view(torch.int32)
    for a, b in zip(t.eval_t(ids, wi, wo, wl, tint=TINT), t.eval_t(ids_p, wi_p, wo_p, wl_p, tint=TINT)):
        assert torch.equal(bits(a[perm]), bits(b))
    for a, b in zip(t.sample_weight(ids, wi, wo, pdf, tint=TINT), t.sample_weight(ids_p, wi_p, wo_p, pdf_p, tint=TINT)):
        assert torch.equal(bits(a[perm]), bits(b))
    for a, b in zip(t.sample_t(ids, wi, u, tint=TINT), t.sample_t(ids_p, wi_p, u_p, tint=TINT)):
        assert torch.equal(bits(a[perm]), bits(b))
    assert torch.equal(bits(t.pdf_t(ids, wi, wo)[perm]), bits(t.pdf_t(ids_p, wi_p, wo_p)))
    # ... and directly: the "uniform" and the "divergent" layout give the rows both assign to the same entry the same bits
    ids_d = make_ids("divergent", n).cuda()
    both = ids == ids_d
    assert int(both.sum()) > 100
    assert torch.equal(bits(t.eval_t(ids, wi, wo, tint=TINT)[both]), bits(t.eval_t(ids_d, wi, wo, tint=TINT)[both]))


@pytest.mark.parametrize("layout", ["divergent", "random"])
def test_per_entry_albedo_is_one_fp32_product_with_the_tint(world, layout):
    """With an albedo per entry and a call tint, entry m's rows are its single-material call with
    tint = float32(tint) * float32(albedo[m]), bit for bit — entry 4's zero channel and entry 3's (1, 1, 1) included."""
    n = world["n"]
    ids = make_ids(layout, n).cuda()
    check_all_calls(world, world["tinted"], world["ref_albedo"], ids, n, TINT, what=f"albedo {layout}")
    check_all_calls(world, world["tinted"], world["ref_albedo"], ids, n, TINT, masked=True, what=f"albedo {layout} masked")
    # the albedo is in it: another table gives entry 0's rows other bits, and entry 3's (albedo 1) the same
    a = world["tinted"].eval_t(ids, world["wi"], world["wo"], tint=TINT)
    b = world["table"].eval_t(ids, world["wi"], world["wo"], tint=TINT)
    lit = (b > 1e-6).all(1)
    assert torch.equal(a[ids == 3], b[ids == 3]) and bool((a[(ids == 0) & lit] != b[(ids == 0) & lit]).all())
    assert bool((a[ids == 4][:, 0] == 0).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_masks_out_buffers_repeated_calls_and_a_side_stream(world, layout):
    n, t = world["n"], world["table"]
    ids = make_ids(layout, n).cuda()
    wi, wo, wl, u, pdf, mask = (world[k] for k in ("wi", "wo", "wl", "u", "pdf", "active"))
    # the masked references are the single-material kernels' own masked calls: unmasked rows keep their bits, masked rows are 0 ...
    gt = check_all_calls(world, t, world["ref"], ids, n, TINT, masked=True, what=f"masked {layout}")
    off, on = gt & ~mask, gt & mask
    assert int(off.sum()) > 0 and int(on.sum()) > 0 and int((~gt & ~mask).sum()) > 0
    out = (torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n,), SENTINEL, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda"))
    ret = t.sample_t(ids, wi, u, tint=TINT, active=mask, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))      # written in place
    full = t.sample_t(ids, wi, u, tint=TINT)
    for r, f in zip(ret, full):
        assert torch.equal(r[on], f[on]) and bool((r[off] == 0).all()) and bool(torch.isnan(r[~gt]).all())   # ... NaN without ground truth
    p_out = torch.full((n,), SENTINEL, device="cuda")
    assert t.pdf_t(ids, wi, wo, active=mask.to(torch.uint8), out=p_out).data_ptr() == p_out.data_ptr()
    p_full = t.pdf_t(ids, wi, wo)
    assert torch.equal(p_out[on], p_full[on]) and bool((p_out[off] == 0).all()) and bool(torch.isnan(p_out[~gt]).all())
    wgt, pk = t.sample_weight(ids, wi, wo, pdf, tint=TINT, active=mask)
    wgt_full, pk_full = t.sample_weight(ids, wi, wo, pdf, tint=TINT)
    assert torch.equal(wgt[on], wgt_full[on]) and torch.equal(pk[on], pk_full[on])
    assert bool((wgt[off] == 0).all()) and bool((pk[off] == 0).all())
    assert bool(torch.isnan(wgt[~gt]).all()) and torch.equal(pk[~gt], pdf[~gt])
    with pytest.raises(ValueError, match="active must be"):                  # a CPU mask is refused, not copied across
        t.sample_weight(ids, wi, wo, pdf, active=torch.ones(n, dtype=torch.bool))
    # eval_t into caller-supplied outputs, on a side stream
    want_o, _ = expected(world["ref"]["o"], ids, n)
    want_l, _ = expected(world["ref"]["l"], ids, n)
    out_o, out_l = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = t.eval_t(ids, wi, wo, wl, tint=TINT, out_o=out_o, out_l=out_l)
        s_side = t.sample_t(ids, wi, u, tint=TINT)
    side.synchronize()
    assert r[0] is out_o and r[1] is out_l
    same_bits(out_o, want_o, gt, "side stream f_o")
    same_bits(out_l, want_l, gt, "side stream f_l")
    for a, b in zip(s_side, full):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a second call into the SAME outputs agrees with the first; a third with other ids leaves nothing of it
    keep_o, keep_l = out_o.clone(), out_l.clone()
    t.eval_t(ids, wi, wo, wl, tint=TINT, out_o=out_o, out_l=out_l)
    assert torch.equal(out_o.view(torch.int32), keep_o.view(torch.int32)) and torch.equal(out_l.view(torch.int32), keep_l.view(torch.int32))
    ids2 = torch.roll(ids, 97)
    want_o2, gt2 = expected(world["ref"]["o"], ids2, n)
    want_l2, _ = expected(world["ref"]["l"], ids2, n)
    t.eval_t(ids2, wi, wo, wl, tint=TINT, out_o=out_o, out_l=out_l)
    same_bits(out_o, want_o2, gt2, "other ids f_o")
    same_bits(out_l, want_l2, gt2, "other ids f_l")


def _err(got, ref):
    """Per-row error against fp64: relative to max(|ref|, 1e-6 of the column's largest)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max(0))


def _held_to_yardstick(label, got, yard):
    fig = {q: dict(gpu_p99=np.percentile(got[q], 99), yard_p99=np.percentile(yard[q], 99), gpu_max=got[q].max(), yard_max=yard[q].max())
           for q in got}
    msg = label + ": " + "; ".join(f"{q} p99 gpu {f['gpu_p99']:.3e} yardstick {f['yard_p99']:.3e}, max gpu {f['gpu_max']:.3e} "
                                   f"yardstick {f['yard_max']:.3e}" for q, f in fig.items())
    print(msg)
    for q, f in fig.items():
        assert f["gpu_p99"] <= 4 * f["yard_p99"], msg
        assert f["gpu_max"] <= 4 * f["yard_max"], msg


def test_table_matches_fp64_within_the_fp32_yardstick(world):
    """The table's own numbers — not by way of the single-material kernels — against tests/principled_ref.py and
    tests/dielectric_ref.py in fp64, ids drawn per lane: eval of both directions and the pdf, on the rows that have ground truth,
    each row's error taken within its own material (relative to that material's column maximum), the percentiles over all of
    them; the yardstick is the same references in fp32 on the same rows (4x at p99 and at the maximum)."""
    n, t = world["n"], world["table"]
    ids = make_ids("random", n).cuda()
    wi, wo, wl = (world[k] for k in ("wi", "wo", "wl"))
    f_o, f_l = (x.cpu().numpy() for x in t.eval_t(ids, wi, wo, wl, tint=TINT))
    p = t.pdf_t(ids, wi, wo).cpu().numpy()
    ids_h, wi_h, wo_h, wl_h = ids.cpu().numpy(), wi.cpu().numpy(), wo.cpu().numpy(), wl.cpu().numpy()
    got = {"eval": [], "eval wl": [], "pdf": []}
    yard = {k: [] for k in got}
    for m, (r64, r32) in enumerate(zip(_models(np.float64), _models(np.float32))):
        rows = ids_h == m
        if r64 is None:
            assert np.isnan(f_o[rows]).all() and np.isnan(f_l[rows]).all() and np.isnan(p[rows]).all()
            continue
        assert rows.sum() > 300
        a, b, c = wi_h[rows], wo_h[rows], wl_h[rows]
        ref = {"eval": r64.eval(a, b, TINT), "eval wl": r64.eval(a, c, TINT), "pdf": r64.pdf(a, b)}
        y = {"eval": r32.eval(a, b, TINT), "eval wl": r32.eval(a, c, TINT), "pdf": r32.pdf(a, b)}
        g = {"eval": f_o[rows], "eval wl": f_l[rows], "pdf": p[rows]}
        assert all(np.isfinite(v).all() and (v >= 0).all() for v in g.values())
        fig = []
        for q in got:
            eg, ey = _err(g[q], ref[q]), _err(y[q], ref[q])
            eg, ey = (eg.max(1), ey.max(1)) if eg.ndim == 2 else (eg, ey)
            got[q].append(eg)
            yard[q].append(ey)
            fig.append(f"{q} max gpu {eg.max():.3e} yardstick {ey.max():.3e}")
        print(f"slot {m} ({SLOTS[m]}, {int(rows.sum())} rows): " + "; ".join(fig))
    _held_to_yardstick("table, ids per lane", {q: np.concatenate(v) for q, v in got.items()},
                       {q: np.concatenate(v) for q, v in yard.items()})


def test_bad_arguments_are_refused_without_touching_the_device(world):
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, reference_bsdf
    L, t = _lib.lib(), world["table"]._t
    ids = make_ids("divergent", 64).cuda()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    wi, wo, wl, u, pdf = (world[k][:64] for k in ("wi", "wo", "wl", "u", "pdf"))
    out, out2, out1 = torch.full((64, 3), SENTINEL, device="cuda"), torch.full((64, 3), SENTINEL, device="cuda"), torch.full((64,), SENTINEL, device="cuda")

    def einval(rc, expect):
        with pytest.raises(RuntimeError, match="bsdfd error 1: .*" + expect):
            _lib.check(rc)
    einval(L.bsdfd_analytic_eval_table(None, ptr(ids), ptr(wi), ptr(wo), None, 64, None, ptr(out), None, None), "null analytic table")
    einval(L.bsdfd_analytic_sample_table(None, ptr(ids), ptr(wi), ptr(u), None, 64, None, ptr(out), ptr(out1), None, None), "null analytic table")
    einval(L.bsdfd_analytic_eval_table(t, ptr(ids), ptr(wi), ptr(wo), None, -1, None, ptr(out), None, None), "N must be >= 0")
    einval(L.bsdfd_analytic_pdf_table(t, ptr(ids), ptr(wi), ptr(wo), None, -5, ptr(out1), None), "N must be >= 0")
    einval(L.bsdfd_analytic_sample_weight_table(t, ptr(ids), ptr(wi), ptr(wo), ptr(pdf), None, 2 ** 32, None, 3.5, ptr(out), ptr(out1), None),
           "N too large")
    einval(L.bsdfd_analytic_eval_table(t, ptr(ids), ptr(wi), ptr(wo), None, 64, None, ptr(out), ptr(out2), None), "both NULL or both given")
    einval(L.bsdfd_analytic_eval_table(t, ptr(ids), ptr(wi), ptr(wo), ptr(wl), 64, None, ptr(out), None, None), "both NULL or both given")
    einval(L.bsdfd_analytic_eval_table(t, None, ptr(wi), ptr(wo), None, 64, None, ptr(out), None, None), "null pointer")
    einval(L.bsdfd_analytic_sample_table(t, ptr(ids), ptr(wi), None, None, 64, None, ptr(out), ptr(out1), None, None), "null pointer")
    einval(L.bsdfd_analytic_pdf_table(t, ptr(ids), ptr(wi), ptr(wo), None, 64, None, None), "null pointer")
    # N == 0 launches nothing, whatever the pointers
    assert L.bsdfd_analytic_eval_table(t, None, None, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in (out, out2, out1))          # a rejected call writes nothing
    with pytest.raises(ValueError, match="out_l without wl"):
        world["table"].eval_t(ids, wi, wo, out_l=out2)
    with pytest.raises(ValueError, match="u must be"):
        world["table"].sample_t(ids, wi, u[:, :2].contiguous())
    with pytest.raises(ValueError, match="material_id must be"):
        world["table"].pdf_t(ids.int(), wi, wo)
    # create: a table without any ground truth, and a descriptor the single-material launcher refuses, written into the C struct
    with pytest.raises(RuntimeError, match="bsdfd error 1: .*at least one"):
        AnalyticTable([None, None])
    recs = (_lib.AnalyticEntry * 2)()
    for r in recs:
        r.kind, r.albedo, r.desc.principled = _lib.ANALYTIC_PRINCIPLED, (C.c_float * 3)(1, 1, 1), reference_bsdf(13)._desc
    recs[1].desc.principled.eta = 0.9
    made = C.c_void_p()
    einval(L.bsdfd_analytic_table_create(recs, 2, C.byref(made)), "entry 1: bsdfd_principled.eta")
    assert not made.value
    recs[1].desc.principled.eta = 1.5
    assert L.bsdfd_analytic_table_create(recs, 2, C.byref(made)) == 0 and made.value
    L.bsdfd_analytic_table_destroy(made)
