"""The register-resident fast path (csrc/flow32.hip, flow_kernel32<.., ROP>) where ONE WAVE RUNS SEVERAL TILES in sequence — the
shapes tests/test_gpu_resident_path.py does not reach.  The weight fragments stay in registers across tiles and Euler steps, so
anything a tile leaves behind (a stale accumulator, a state register, the determinant product) would show in the next tile of the
same wave.  Held BIT FOR BIT to the general kernel, reached through an identity ``row_index`` (and ``rng_index`` for sample), as in
that file; the kernel a call ran is read from ``profile_read_op``.

  * N = 2^18 + 33, T = 8: 8 194 tiles — on 256 CUs more than one round of the capped grid, so some waves take a second trip of the
    tile loop; the last tile is ragged (one live query of 32).
  * N = 2^19 + 33, T = 8: the host hands out two-tile chunks (chunk_log2 = 1): consecutive trips of one wave.
  * T = 32 at N = 33 and N = 4 129: the longest Euler loop the fast path is selected for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from conftest import load_case  # noqa: E402

STEM = "aniso_miro_7_rgb_disk"
SHAPES = (((1 << 18) + 33, 8), ((1 << 19) + 33, 8), (33, 32), (4129, 32))   # (N, T)
SEED, OFFSET = 0x9E3779B97F4A7C15, 123457


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _dirs(rng, n):
    """Unit directions over both hemispheres, a quarter of them grazing (test_gpu_resident_path._dirs)."""
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
    """(result, (launches of the op, of them resident)) of one call through the profiling handle."""
    s.set_profiling(True)
    out = call()
    n = {k: s.profile_read_op(k)[0] for k in ("sample", "pdf", "sample_resident", "pdf_resident")}
    s.set_profiling(False)
    return out, n


def _first_diff(a, b):
    d = (a != b).reshape(a.shape[0], -1).any(1).nonzero()
    return None if d.numel() == 0 else (int(d[0]), int(d.numel()))


@pytest.mark.parametrize("n,T", SHAPES)
def test_resident_equals_general_where_a_wave_runs_several_tiles(smp, n, T):
    rng = np.random.default_rng(77 * n + T)
    ident = torch.arange(n, dtype=torch.int64, device=_dev())
    wi, wo_q = _dirs(rng, n), _dirs(rng, n)

    (wo_f, ps_f), ran = _ran(smp, lambda: smp.plugin_sample(wi, None, T=T, seed=SEED, offset=OFFSET))
    assert (ran["sample"], ran["sample_resident"]) == (1, 1), ran
    (wo_g, ps_g), ran = _ran(smp, lambda: smp.plugin_sample(wi, None, T=T, seed=SEED, offset=OFFSET, row_index=ident, rng_index=ident))
    assert (ran["sample"], ran["sample_resident"]) == (1, 0), ran
    assert torch.isfinite(wo_f).all() and torch.isfinite(ps_f).all()
    assert torch.equal(wo_f, wo_g) and torch.equal(ps_f, ps_g), ("sample", n, T, _first_diff(wo_f, wo_g), _first_diff(ps_f, ps_g))

    for what, wo in (("pdf at fresh directions", wo_q), ("pdf at the produced directions", wo_f)):
        p_f, ran = _ran(smp, lambda: smp.plugin_pdf(wi, wo, T=T))
        assert (ran["pdf"], ran["pdf_resident"]) == (1, 1), ran
        p_g, ran = _ran(smp, lambda: smp.plugin_pdf(wi, wo, T=T, row_index=ident))
        assert (ran["pdf"], ran["pdf_resident"]) == (1, 0), ran
        assert torch.isfinite(p_f).all() and torch.equal(p_f, p_g), (what, n, T, _first_diff(p_f, p_g))
        live = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        assert bool((p_f[~live] == 0).all()) and bool((p_f[live] > 0).any())
    # the ragged last tile holds this query alone
    assert bool(ps_f[-1] >= 0) and bool(torch.isfinite(wo_f[-1]).all())
