"""The host layer issues every plugin-level call through the library's ``*_ex`` entry points, with ``opts = NULL`` when no option
is set (sampler.py, materials.py).  That stands on one property of the C ABI, pinned here straight through ``_lib.lib()``: a
plain entry point, its ``_ex`` twin with ``opts = NULL`` and the twin with an all-null ``bsdfd_opts`` are the same call.  Both
sides run the same kernel on the same inputs, so every comparison is BITWISE.

Sizes: 1 and 33 are a lone partial tile and a tile boundary of both tilings, 4097 is more than one workgroup's chunk plus a
ragged tail."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from conftest import load_case  # noqa: E402

STEMS = ["chm_orange_rgb_disk", "aniso_miro_7_rgb_spherical"]
SIZES = [1, 33, 4097]
SEED, OFFSET = 11, 5


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _dirs(n, seed, lo=0.05):
    g = torch.Generator().manual_seed(seed)
    z = lo + (0.95 - lo) * torch.rand(n, generator=g)
    ph = 6.2831853 * torch.rand(n, generator=g)
    r = torch.sqrt(1 - z * z)
    return torch.stack([r * torch.cos(ph), r * torch.sin(ph), z], 1).float().to(_dev())


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("stem", STEMS)
def test_plain_entry_points_are_their_ex_twins_without_options(stem, tile, n):
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    _, fw = load_case(stem)
    a, b = FlowSampler(fw, tile=tile, binding="ctypes"), FlowSampler(fw, tile=tile, binding="ctypes")
    L, T, var = _lib.lib(), 4 if fw.domain == 0 else 8, _lib.PLUGIN_MEASURED
    wi, wl = _dirs(n, 1), _dirs(n, 2, 0.02)
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hs, ends = (C.c_void_p * 2)(a._h, b._h), (C.c_int64 * 2)(n // 2, n)   # two handles: rows [0, n/2) and [n/2, n)

    def outs():   # (wo, pdf, pdf2) with a filling no kernel produces
        return [torch.full((n, 3), -7.0, device=_dev()), torch.full((n,), -7.0, device=_dev()), torch.full((n,), -7.0, device=_dev())]

    def run(call):
        """[outputs of the plain call, of the _ex call with opts = NULL, of the _ex call with an all-null bsdfd_opts]"""
        res = []
        for opts in ((), (None,), (C.byref(_lib.Opts()),)):
            o = outs()
            _lib.check(call(o, opts))
            res.append(o)
        torch.cuda.synchronize()
        assert not (res[0][1] == -7.0).any()          # (every call writes a pdf)
        return res

    with torch.cuda.device(_dev()):
        calls = {
            "sample": run(lambda o, opts: (L.bsdfd_plugin_sample_ex if opts else L.bsdfd_plugin_sample)(
                a._h, var, p(wi), None, SEED, OFFSET, n, T, p(o[0]), p(o[1]), *opts, st)),
            "pdf": run(lambda o, opts: (L.bsdfd_plugin_pdf_ex if opts else L.bsdfd_plugin_pdf)(
                a._h, var, p(wi), p(wl), n, T, p(o[1]), *opts, st)),
            "sample_pdf": run(lambda o, opts: (L.bsdfd_plugin_sample_pdf_ex if opts else L.bsdfd_plugin_sample_pdf)(
                a._h, var, p(wi), None, p(wl), SEED, OFFSET, n, T, p(o[0]), p(o[1]), p(o[2]), *opts, st)),
            "sample_multi": run(lambda o, opts: (L.bsdfd_plugin_sample_multi_ex if opts else L.bsdfd_plugin_sample_multi)(
                hs, 2, ends, var, p(wi), None, SEED, OFFSET, T, p(o[0]), p(o[1]), *opts, st)),
            "pdf_multi": run(lambda o, opts: (L.bsdfd_plugin_pdf_multi_ex if opts else L.bsdfd_plugin_pdf_multi)(
                hs, 2, ends, var, p(wi), p(wl), T, p(o[1]), *opts, st)),
            "sample_pdf_multi": run(lambda o, opts: (L.bsdfd_plugin_sample_pdf_multi_ex if opts else L.bsdfd_plugin_sample_pdf_multi)(
                hs, 2, ends, var, p(wi), None, p(wl), SEED, OFFSET, T, p(o[0]), p(o[1]), p(o[2]), *opts, st)),
        }
    for name, (plain, ex_null, ex_empty) in calls.items():
        assert _same_bits(plain, ex_null), f"{name}: the _ex call with opts = NULL differs from the plain call"
        assert _same_bits(plain, ex_empty), f"{name}: the _ex call with an all-null bsdfd_opts differs from the plain call"
    a.close()
    b.close()


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("stem", STEMS)
def test_fused_call_writes_the_callers_buffers_through_either_binding(stem, tile, n, binding):
    """``plugin_sample_pdf(out=)``: the tensors passed come back, holding the bits of the allocating call — through the binding
    the sampler was created with (the operator library has a buffer-writing form of the fused call of its own)."""
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    _, fw = load_case(stem)
    s = FlowSampler(fw, tile=tile, binding=binding)
    T = 4 if fw.domain == 0 else 8
    wi, wl = _dirs(n, 1), _dirs(n, 2, 0.02)
    ref = s.plugin_sample_pdf(wi, wl, T=T, seed=SEED, offset=OFFSET)
    out = (torch.full((n, 3), -7.0, device=_dev()), torch.full((n,), -7.0, device=_dev()), torch.full((n,), -7.0, device=_dev()))
    got = s.plugin_sample_pdf(wi, wl, T=T, seed=SEED, offset=OFFSET, out=out)
    assert len(got) == 3 and all(g is o for g, o in zip(got, out))
    assert _same_bits(got, ref)
    s.close()
