"""GPU: the fold of an anisotropic measured file onto its stored ``phi_i`` range (csrc/measured_dev.h: ``fold_wi``, called by
measured_f, measured_sample and measured_pdf) on a file for every stored range — the quadrants [-pi, -pi/2] and [0, pi/2]
(reduction 4), the half-planes [-pi, 0] and [0, pi] (reduction 2), the full circle (reduction 1) — at random rows and at rows
ON the symmetry planes (tests/measured_fold_rows.py): ``eval_t``, ``pdf_t`` and ``sample_t`` of ``MeasuredBSDF`` and ``MeasuredTable``.

Against the fp64 run of tests/measured_sampling_ref.py (which tests/test_measured_fold_cpu.py holds to the fold rule and to
oracle/measured_oracle.py) by the rule of tests/test_gpu_measured_sampling.py: the kernels may be 4x worse than the same numpy
code run in fp32, at the 99th percentile and at the maximum.  A wrong slice or a wrong flip is an O(0.1) error on these smooth
random tables.  And bit for bit: the sign of a zero, and the file's symmetry group, change no bit.

Before ``fold_wi`` a zero component kept its sign: (x, +0, z) in the quadrant [-pi, -pi/2], (-x, +0, z) in the half-plane
[-pi, 0] and (-x, -0, z) in [0, pi] had the azimuth +-pi outside the stored range, which was clamped to the range's FAR end;
those kernels fail the hand rows of these three files (eval off by up to 0.5 of the value, pdf by a factor) and no random row."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import measured_fold_rows as rows_of  # noqa: E402
import measured_sampling_ref as R  # noqa: E402
from measured_sampling_ref import held_to_yardstick as _held_to_yardstick, sample_errors as _sample_errors  # noqa: E402

NAMES = tuple(rows_of.FILES)
FOLDED = tuple(k for k, v in rows_of.FILES.items() if v[2] >= 2)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chm_orange_rgb.bsdf")
TINT = (0.9, 0.8, 0.7)
SENTINEL = 123.25


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def rows():
    """Random rows first, hand rows after them: fp32 arrays, their device copies, and which rows are which."""
    wi_r, wo_r, u_r = rows_of.random_rows()
    wi_h, wo_h, u_h, kind, axis = rows_of.hand_rows()
    wi, wo, u = np.concatenate([wi_r, wi_h]), np.concatenate([wo_r, wo_h]), np.concatenate([u_r, u_h])
    hand = np.arange(len(wi)) >= len(wi_r)
    pad = np.full(len(wi_r), -9)
    return dict(wi=wi, wo=wo, u=u, hand=hand, kind=np.concatenate([pad, kind]), axis=np.concatenate([pad, axis]),
                wi_d=_cuda(wi), wo_d=_cuda(wo), u_d=_cuda(u))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    paths = rows_of.write_files(tmp_path_factory.mktemp("measured_fold_gpu"))
    b = {k: MeasuredBSDF(p) for k, p in paths.items()}
    for k, (_, n_phi, reduction, _) in rows_of.FILES.items():
        assert (b[k].isotropic, b[k].reduction, b[k].n_phi, b[k].jacobian, b[k].has_luminance) == (False, reduction, n_phi, True, True)
    return b


@pytest.fixture(scope="module")
def case(gpu, rows):
    """Per file, computed once and shared (read-only): eval / pdf / sample of the fp64 reference, of its fp32 run (the yardstick)
    and of the kernels, on every row."""
    cache = {}

    def get(name):
        if name not in cache:
            c = {}
            for tag, dt in (("ref", np.float64), ("yard", np.float32)):
                r = R.MeasuredSampler(gpu[name].path, dt)
                c[tag] = dict(r=r, eval=r.eval(rows["wi"], rows["wo"], TINT), pdf=r.pdf(rows["wi"], rows["wo"]),
                              sample=r.sample(rows["wi"], rows["u"], TINT))
            got_d = dict(eval=gpu[name].eval_t(rows["wi_d"], rows["wo_d"], tint=TINT), pdf=gpu[name].pdf_t(rows["wi_d"], rows["wo_d"]),
                         sample=gpu[name].sample_t(rows["wi_d"], rows["u_d"], tint=TINT))
            c["got_d"] = got_d
            c["got"] = dict(eval=got_d["eval"].cpu().numpy(), pdf=got_d["pdf"].cpu().numpy(),
                            sample=tuple(t.cpu().numpy() for t in got_d["sample"]))
            cache[name] = c
        return cache[name]
    return get


def _eval_err(res, ref, sel):
    res, ref = np.asarray(res, dtype=np.float64)[sel], ref[sel]
    return {"eval": np.abs(res - ref).max(1) / (np.abs(ref).max(1) + 1e-3)}


def _pdf_err(res, ref, sel):
    """Relative where the reference is positive; where it is zero the flags were compared exactly."""
    res, ref = np.asarray(res, dtype=np.float64)[sel], ref[sel]
    return {"pdf": np.where(ref > 0, np.abs(res - ref) / np.where(ref > 0, ref, 1), 0.0)}


@pytest.mark.parametrize("name", NAMES)
def test_eval_matches_fp64_within_the_fp32_yardstick(case, rows, name):
    c = case(name)
    got, ref, yard = c["got"]["eval"], c["ref"]["eval"], c["yard"]["eval"]
    assert np.isfinite(got).all()
    dead = (rows["wi"][:, 2] <= 0) | (rows["wo"][:, 2] <= 0)
    assert ((got == 0).all(1) == dead).all() and ((ref == 0).all(1) == dead).all() and dead.sum() >= 8
    _held_to_yardstick(name + " eval_t, random rows", _eval_err(got, ref, ~rows["hand"] & ~dead), _eval_err(yard, ref, ~rows["hand"] & ~dead))
    _held_to_yardstick(name + " eval_t, hand rows", _eval_err(got, ref, rows["hand"]), _eval_err(yard, ref, rows["hand"]))


@pytest.mark.parametrize("name", NAMES)
def test_pdf_matches_fp64_within_the_fp32_yardstick(case, rows, name):
    c = case(name)
    got, ref, yard = c["got"]["pdf"].astype(np.float64), c["ref"]["pdf"], c["yard"]["pdf"].astype(np.float64)
    assert np.isfinite(got).all() and ((got == 0) == (ref == 0)).all() and (got[rows["wo"][:, 2] <= 0] == 0).all()
    rnd = ~rows["hand"] & (ref > 0)
    assert rnd.sum() > 0.9 * (~rows["hand"]).sum()
    _held_to_yardstick(name + " pdf_t, random rows", _pdf_err(got, ref, rnd), _pdf_err(yard, ref, rnd))
    _held_to_yardstick(name + " pdf_t, hand rows", _pdf_err(got, ref, rows["hand"]), _pdf_err(yard, ref, rows["hand"]))


@pytest.mark.parametrize("name", NAMES)
def test_sample_matches_fp64_within_the_fp32_yardstick(case, rows, name):
    c = case(name)
    got, ref, yard = c["got"]["sample"], c["ref"]["sample"], c["yard"]["sample"]
    wo_r, pdf_r, _ = ref
    assert all(np.isfinite(a).all() for a in got)
    scored = wo_r[:, 2] > 1e-4
    rnd = ~rows["hand"]
    assert 1 - scored[rnd].mean() <= 0.35, 1 - scored[rnd].mean()
    assert (pdf_r[scored & rnd] > 0).all()
    clear = ~scored & (np.abs(wo_r[:, 2]) > 1e-4)                # wo safely below the horizon: the zero flags agree exactly
    assert ((got[1] == 0) == (pdf_r == 0))[clear].all()
    assert (got[2][got[1] == 0] == 0).all()
    _held_to_yardstick(name + " sample_t, random rows", _sample_errors(got, ref, scored & rnd), _sample_errors(yard, ref, scored & rnd))
    hand = scored & rows["hand"]
    assert hand.sum() >= 0.5 * rows["hand"].sum() and (pdf_r[hand] > 0).all()
    _held_to_yardstick(name + " sample_t, hand rows", _sample_errors(got, ref, hand), _sample_errors(yard, ref, hand))


@pytest.mark.parametrize("name", NAMES)
def test_sample_pdf_and_eval_agree_on_the_device(gpu, case, rows, name):
    """tests/test_gpu_measured_sampling.py's statement, on every row: pdf_t of the sampled direction against the sampler's pdf,
    weight * pdf against eval_t * tint."""
    c = case(name)
    wo_d = c["got_d"]["sample"][0]
    wo, pdf, w = c["got"]["sample"]
    wo_y, pdf_y, w_y = c["yard"]["sample"]
    scored = c["ref"]["sample"][0][:, 2] > 1e-4
    assert np.abs(np.linalg.norm(wo.astype(np.float64), axis=1) - 1)[scored].max() <= 1e-5
    sel = scored & (pdf > 0) & (pdf_y > 0)
    assert sel.sum() >= 0.99 * scored.sum()
    back = gpu[name].pdf_t(rows["wi_d"], wo_d).cpu().numpy().astype(np.float64)
    f = gpu[name].eval_t(rows["wi_d"], wo_d, tint=TINT).cpu().numpy().astype(np.float64)
    r32 = c["yard"]["r"]
    back_y, f_y = r32.pdf(rows["wi"], wo_y).astype(np.float64), r32.eval(rows["wi"], wo_y, TINT).astype(np.float64)
    pdf, pdf_y = np.where(sel, pdf, 1.0).astype(np.float64), np.where(sel, pdf_y, 1.0).astype(np.float64)
    got = {"round trip": (np.abs(back - pdf) / pdf)[sel],
           "weight*pdf": (np.abs(w.astype(np.float64) * pdf[:, None] - f).max(1) / (np.abs(f).max(1) + 1e-3))[sel]}
    yard = {"round trip": (np.abs(back_y - pdf_y) / pdf_y)[sel],
            "weight*pdf": (np.abs(w_y.astype(np.float64) * pdf_y[:, None] - f_y).max(1) / (np.abs(f_y).max(1) + 1e-3))[sel]}
    _held_to_yardstick(name + " self-consistency", got, yard, maxima=False)


@pytest.mark.parametrize("name", FOLDED)
def test_the_sign_of_a_zero_changes_no_bit(gpu, case, rows, name):
    """On a plane (exactly one zero component in wi), with a wo without zero components: eval_t, pdf_t and sample_t's three
    outputs have the bits of the row with the other zero."""
    sel = ((rows["axis"] == 0) | (rows["axis"] == 1)) & (rows["kind"] >= 0) & (rows["kind"] < 4)
    assert sel.sum() == 16 * 4 and (rows["wo"][sel][:, :2] != 0).all()
    wi = rows["wi"][sel].copy()
    zero = wi == 0
    assert (zero.sum(1) == 1).all()
    wi[zero] = -wi[zero]
    assert (np.signbit(wi) != np.signbit(rows["wi"][sel]))[zero].all()
    wi_d, wo_d = _cuda(wi), _cuda(rows["wo"][sel])
    at = torch.from_numpy(sel).cuda()
    c = case(name)
    assert torch.equal(_bits(gpu[name].eval_t(wi_d, wo_d, tint=TINT)), _bits(c["got_d"]["eval"][at]))
    assert torch.equal(_bits(gpu[name].pdf_t(wi_d, wo_d)), _bits(c["got_d"]["pdf"][at]))
    assert bool((c["got_d"]["pdf"][at] > 0).any())
    # sample_t reads no wo: every plane row, with all eight of its variate pairs
    sel = (rows["axis"] == 0) | (rows["axis"] == 1)
    wi = rows["wi"][sel].copy()
    wi[wi == 0] = -wi[wi == 0]
    at = torch.from_numpy(sel).cuda()
    for a, b in zip(gpu[name].sample_t(_cuda(wi), _cuda(rows["u"][sel]), tint=TINT), c["got_d"]["sample"]):
        assert torch.equal(_bits(a), _bits(b[at]))
    assert bool((c["got_d"]["sample"][1][at] > 0).any())
    # normal incidence: the four signed versions of (+-0, +-0, 1) on the same wo / variates
    first = np.flatnonzero(rows["axis"] == 2)[:8]
    assert (rows["wi"][first] == [0, 0, 1]).all()
    wo_d, u_d = _cuda(np.tile(rows["wo"][first][:4], (4, 1))), _cuda(np.tile(rows["u"][first], (4, 1)))
    normals = np.float32([[0.0, 0.0, 1], [0.0, -0.0, 1], [-0.0, 0.0, 1], [-0.0, -0.0, 1]])
    f = gpu[name].eval_t(_cuda(np.repeat(normals, 4, 0)), wo_d, tint=TINT).reshape(4, 4, 3)
    p = gpu[name].pdf_t(_cuda(np.repeat(normals, 4, 0)), wo_d).reshape(4, 4)
    s = [t.reshape(4, 8, -1) for t in gpu[name].sample_t(_cuda(np.repeat(normals, 8, 0)), u_d, tint=TINT)]
    for t in [f, p] + s:
        assert all(torch.equal(_bits(t[k]), _bits(t[0])) for k in range(1, 4))
    assert bool((p > 0).all()) and bool((s[1] > 0).any())


@pytest.mark.parametrize("name", FOLDED)
def test_the_symmetry_group_changes_no_bit(gpu, case, rows, name):
    """Off the planes (the random rows and the rows 2^-100 off a plane): for every member G of the file's group — the four sign
    pairs of x and y for reduction 4, the identity and the point reflection for reduction 2 — eval_t(G wi, G wo) and pdf_t(G wi,
    G wo) are the bits of (wi, wo), and sample_t(G wi, u) returns G wo with the same pdf and weight."""
    sel = ~rows["hand"] | (rows["axis"] == -1)
    assert (rows["wi"][sel][:, :2] != 0).all() and sel.sum() == rows_of.N_RANDOM + 16 * 8
    at = torch.from_numpy(sel).cuda()
    wi_d, wo_d, u_d = rows["wi_d"][at], rows["wo_d"][at], rows["u_d"][at].contiguous()
    c = case(name)
    f, p = c["got_d"]["eval"][at], c["got_d"]["pdf"][at]
    s_wo, s_pdf, s_w = (t[at] for t in c["got_d"]["sample"])
    group = [(1, 1), (-1, 1), (1, -1), (-1, -1)] if gpu[name].reduction == 4 else [(1, 1), (-1, -1)]
    for gx, gy in group:
        G = torch.tensor([gx, gy, 1], dtype=torch.float32, device="cuda")
        g_wi, g_wo = (wi_d * G).contiguous(), (wo_d * G).contiguous()
        assert torch.equal(_bits(gpu[name].eval_t(g_wi, g_wo, tint=TINT)), _bits(f)), (name, gx, gy)
        assert torch.equal(_bits(gpu[name].pdf_t(g_wi, g_wo)), _bits(p)), (name, gx, gy)
        wo, pdf, w = gpu[name].sample_t(g_wi, u_d, tint=TINT)
        assert torch.equal(_bits(wo), _bits(s_wo * G)) and torch.equal(_bits(pdf), _bits(s_pdf)) and torch.equal(_bits(w), _bits(s_w)), (name, gx, gy)


def test_table_and_row_list_return_the_bits_of_the_single_material_calls(gpu, case, rows):
    """A MeasuredTable of the five files and the shipped isotropic one, ids interleaved so that every wave is mixed, on every row
    (the hand rows included): eval_t, sample_t and pdf_t return the bits of each material's own call; eval_t's ``rows=`` form does
    on a shuffled list, and leaves the rows outside the list untouched."""
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable
    fixture = MeasuredBSDF(FIXTURE)
    entries = [gpu[k] for k in NAMES] + [fixture]
    tab = MeasuredTable(entries)
    n = len(rows["wi"])
    ids = (torch.arange(n) % len(entries)).cuda()
    wi_d, wo_d, u_d = rows["wi_d"], rows["wo_d"], rows["u_d"]
    single = [case(k)["got_d"] for k in NAMES] + [dict(eval=fixture.eval_t(wi_d, wo_d, tint=TINT), pdf=fixture.pdf_t(wi_d, wo_d),
                                                       sample=fixture.sample_t(wi_d, u_d, tint=TINT))]

    def want(pick):
        out = torch.empty_like(pick(single[0]))
        for m, s in enumerate(single):
            out[ids == m] = pick(s)[ids == m]
        return out
    assert torch.equal(_bits(tab.eval_t(ids, wi_d, wo_d, tint=TINT)), _bits(want(lambda s: s["eval"])))
    assert torch.equal(_bits(tab.pdf_t(ids, wi_d, wo_d)), _bits(want(lambda s: s["pdf"])))
    for j, t in enumerate(tab.sample_t(ids, wi_d, u_d, tint=TINT)):
        assert torch.equal(_bits(t), _bits(want(lambda s: s["sample"][j]))), j
    # the list form: a shuffled two thirds of the rows, the hand rows among them
    g = np.random.default_rng(5)
    listed = np.concatenate([g.permutation(rows_of.N_RANDOM)[: rows_of.N_RANDOM // 3 * 2], np.flatnonzero(rows["hand"])])
    listed = torch.from_numpy(g.permutation(listed)).cuda()
    out = torch.full((n, 3), SENTINEL, device="cuda")
    assert tab.eval_t(ids, wi_d, wo_d, tint=TINT, out_o=out, rows=listed) is out
    inside = torch.zeros(n, dtype=torch.bool, device="cuda")
    inside[listed] = True
    assert torch.equal(_bits(out[inside]), _bits(want(lambda s: s["eval"])[inside]))
    assert bool((out[~inside] == SENTINEL).all()) and int((~inside).sum()) > 1000
