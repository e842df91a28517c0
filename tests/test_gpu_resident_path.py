"""The register-resident fast path of the disk net's plain plugin sample / pdf call (csrc/flow32.hip, flow_kernel32<.., ROP>; selected by
run() in csrc/bsdfd.hip at T = 8, 16, 32, ...) against the general kernel: the same statements in the same order, so the results are
held to it BIT FOR BIT.  The general kernel is reached for the same work through an identity ``row_index`` (pdf) and an identity
``row_index`` + ``rng_index`` (sample: the Philox counter is ``offset + index`` either way, so the draws are the same).  Which kernel
a call ran is read from the profiling interface (``profile_read_op("sample_resident" | "pdf_resident")``)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from conftest import load_case  # noqa: E402

STEM = "aniso_miro_7_rgb_disk"
SIZES = (1, 31, 32, 33, 4129)   # a lone query, the ragged last tile on both sides of a tile boundary, more tiles than one round of waves
SEEDS = ((3, 7), (0x9E3779B97F4A7C15, 123457))   # (seed, offset): the offset is non-zero


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _dirs(rng, n):
    """Unit directions over BOTH hemispheres, a quarter of them grazing (|z| < 0.1): the pdf's wi_z / wo_z guards fire on the lower
    ones, the sample's r^2 < 0.995 guard on flows that end at the rim of the disk."""
    z = np.where(rng.uniform(size=n) < 0.25, rng.uniform(-0.1, 0.1, size=n), rng.uniform(-1.0, 1.0, size=n))
    ph = rng.uniform(0, 2 * np.pi, size=n)
    r = np.sqrt(1 - z * z)
    return torch.from_numpy(np.stack([r * np.cos(ph), r * np.sin(ph), z], 1).astype(np.float32)).to(_dev())


@pytest.fixture(scope="module")
def smp():
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    _, fw = load_case(STEM)
    s = FlowSampler(fw)
    assert s.tile == 32
    yield s
    s.close()


def _ran(s, call):
    """(result, {kind: launches}) of one call through the profiling handle."""
    s.set_profiling(True)
    out = call()
    n = {k: s.profile_read_op(k)[0] for k in ("sample", "pdf", "sample_resident", "pdf_resident", "samples_only", "sample_pdf")}
    s.set_profiling(False)
    return out, n


@pytest.mark.parametrize("T", (8, 16))
@pytest.mark.parametrize("n", SIZES)
def test_fast_path_equals_the_general_kernel_bit_for_bit(smp, n, T):
    rng = np.random.default_rng(1000 * n + T)
    ident = torch.arange(n, dtype=torch.int64, device=_dev())
    clamped = zeros = 0
    for seed, offset in SEEDS:
        wi, wo_q = _dirs(rng, n), _dirs(rng, n)
        (wo_f, ps_f), ran = _ran(smp, lambda: smp.plugin_sample(wi, None, T=T, seed=seed, offset=offset))
        assert (ran["sample"], ran["sample_resident"]) == (1, 1), ran
        (wo_g, ps_g), ran = _ran(smp, lambda: smp.plugin_sample(wi, None, T=T, seed=seed, offset=offset, row_index=ident, rng_index=ident))
        assert (ran["sample"], ran["sample_resident"]) == (1, 0), ran
        assert torch.isfinite(wo_f).all() and torch.isfinite(ps_f).all()
        assert torch.equal(wo_f, wo_g) and torch.equal(ps_f, ps_g), (n, T, seed, (wo_f - wo_g).abs().max().item(), (ps_f - ps_g).abs().max().item())
        pq_f, ran = _ran(smp, lambda: smp.plugin_pdf(wi, wo_q, T=T))
        assert (ran["pdf"], ran["pdf_resident"]) == (1, 1), ran
        pq_g, ran = _ran(smp, lambda: smp.plugin_pdf(wi, wo_q, T=T, row_index=ident))
        assert (ran["pdf"], ran["pdf_resident"]) == (1, 0), ran
        assert torch.isfinite(pq_f).all() and torch.equal(pq_f, pq_g), (n, T, (pq_f - pq_g).abs().max().item())
        # ... and the pdf of the directions the sampler produced (upper hemisphere by construction)
        pp_f, pp_g = smp.plugin_pdf(wi, wo_f, T=T), smp.plugin_pdf(wi, wo_f, T=T, row_index=ident)
        assert torch.equal(pp_f, pp_g)
        clamped += int(((wo_f[:, 0] == 0) & (wo_f[:, 1] == 0)).sum().item())
        zeros += int(((pq_f == 0) & ((wi[:, 2] <= 0) | (wo_q[:, 2] <= 0))).sum().item())
        live = (wi[:, 2] > 0) & (wo_q[:, 2] > 0)
        assert bool((pq_f[~live] == 0).all())
    if n == SIZES[-1]:   # both epilogue guards were exercised, and so was the unguarded branch
        print(f"n={n} T={T}: {clamped} samples clamped by r^2 >= 0.995, {zeros} pdfs zeroed by the hemisphere guards")
        assert clamped > 0 and zeros > 0 and bool((pq_f[live] > 0).any()) and bool((ps_f > 0).any())


def test_only_the_plain_call_at_power_of_two_steps_from_eight_takes_the_fast_path(smp):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    n = 1000
    rng = np.random.default_rng(5)
    wi, wo = _dirs(rng, n), _dirs(rng, n)

    def kinds(call, s=smp):
        ran = _ran(s, call)[1]
        return ran["sample"], ran["sample_resident"], ran["pdf"], ran["pdf_resident"]

    for T in (8, 16, 32):
        assert kinds(lambda: smp.plugin_sample(wi, None, T=T, seed=1)) == (1, 1, 0, 0)
        assert kinds(lambda: smp.plugin_pdf(wi, wo, T=T)) == (0, 0, 1, 1)
    for T in (4, 12, 1, 2, 7, 24):                                      # below the threshold, or no power of two
        assert kinds(lambda: smp.plugin_sample(wi, None, T=T, seed=1)) == (1, 0, 0, 0), T
        assert kinds(lambda: smp.plugin_pdf(wi, wo, T=T)) == (0, 0, 1, 0), T
    ctx = smp.new_context(n)                                            # a per-query context, written and read
    assert kinds(lambda: smp.plugin_sample(wi, None, T=8, seed=1, ctx_out=ctx)) == (1, 0, 0, 0)
    assert kinds(lambda: smp.plugin_pdf(wi, wo, T=8, ctx_in=ctx)) == (0, 0, 1, 0)
    assert kinds(lambda: smp.plugin_sample(wi, None, T=8, seed=1, ctx_in=ctx)) == (1, 0, 0, 0)
    assert kinds(lambda: smp.plugin_pdf(wi, wo, T=8, ctx_out=ctx)) == (0, 0, 1, 0)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.6).to(_dev())      # a masked call: the live rows arrive as a row_index
    assert kinds(lambda: smp.plugin_sample(wi, None, T=8, seed=1, active=mask)) == (1, 0, 0, 0)
    assert kinds(lambda: smp.plugin_pdf(wi, wo, T=8, active=mask)) == (0, 0, 1, 0)
    x0 = torch.from_numpy(rng.normal(size=(n, 2)).astype(np.float32) * 0.3).to(_dev())   # an injected base point
    assert kinds(lambda: smp.plugin_sample(wi, x0, T=8)) == (1, 0, 0, 0)
    assert kinds(lambda: smp.plugin_sample_pdf(wi, wo, None, T=8, seed=1)) == (0, 0, 0, 0)   # the fused call: its own kernel
    assert kinds(lambda: smp.network_sampling(wi[:, :2].contiguous(), None, T=8, seed=1)) == (1, 0, 0, 0)   # operator io
    assert kinds(lambda: smp.network_pdf(wo[:, :2].contiguous(), wi[:, :2].contiguous(), T=8)) == (0, 0, 1, 0)
    # a segmented (MaterialTable) launch is recorded on the handle of its first bucket
    mt = MaterialTable([STEM, "chm_orange_rgb_disk"])
    mid = torch.from_numpy((np.arange(n) % 2).astype(np.int32)).to(_dev())
    first = mt.samplers[0]
    assert kinds(lambda: mt.sample(mid, wi, seed=1, T=8), first) == (1, 0, 0, 0)
    assert kinds(lambda: mt.pdf(mid, wi, wo, T=8), first) == (0, 0, 1, 0)
    # the spherical nets have no such kernel
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    sph = FlowSampler(load_case("aniso_miro_7_rgb_spherical")[1])
    assert kinds(lambda: sph.plugin_sample(wi, None, T=8, seed=1), sph) == (1, 0, 0, 0)
    assert kinds(lambda: sph.plugin_pdf(wi, wo, T=8), sph) == (0, 0, 1, 0)
    sph.close()
    # a handle on 16-query tiles neither
    s16 = FlowSampler(load_case(STEM)[1], tile=16)
    assert kinds(lambda: s16.plugin_sample(wi, None, T=8, seed=1), s16) == (1, 0, 0, 0)
    s16.close()
