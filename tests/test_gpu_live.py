"""`active` masks (ABI 8): bsdfd_compact_live (csrc/live.hip) turns a mask into the ascending row list of the live lanes, the
plugin-level calls run the flow on those rows through bsdfd_opts.row_index, and the masks of the plugin protocol
(rendering/brdf_measured_disk.py:59,112) and of the wavefront harness reach them.  Everything here is BIT-EXACT: a masked call
returns, on its live lanes, the bits of the unmasked call, and 0 on its dead lanes."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from conftest import load_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4096                                                         # rows per block of csrc/live.hip (LV_CHUNK)
Z_PALETTE = [0.0, -0.0, float("nan"), -0.5, -1e-30, 1e-30, 0.3, 1.0]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _compact(active, wi, dr, flags, n, zero=(None, None, None)):
    """bsdfd_compact_live through the C ABI with a workspace full of 0xFF bytes -> (rows [max(n, 1)], count)."""
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    dev = _dev()
    ws = torch.full((int(L.bsdfd_live_workspace_bytes(n)),), 0xFF, dtype=torch.uint8, device=dev)
    rows = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev)
    if n == 0:   # (torch gives empty tensors a NULL pointer; the entry point wants the arrays its flags name even at N = 0)
        wi, dr = (None if t is None else torch.zeros((1, 3), device=dev) for t in (wi, dr))
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    _lib.check(L.bsdfd_compact_live(_ptr(active), _ptr(wi), _ptr(dr), flags, n, _ptr(rows), _ptr(count), *[_ptr(z) for z in zero],
                                    _ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return rows, int(count.item())


def _vectors(n, seed):
    """[n, 3] with z components drawn from the palette (+0, -0, NaN, negatives, positives)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n + 1, 3, generator=g)
    v[:, 2] = torch.tensor(Z_PALETTE)[torch.randint(0, len(Z_PALETTE), (n + 1,), generator=g)]
    return v.to(_dev())[:n]


def _masks(n):
    g = torch.Generator().manual_seed(1000 + n)
    first, last = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if n:
        first[0], last[n - 1] = True, True
    return {"all_live": torch.ones(n, dtype=torch.bool), "all_dead": torch.zeros(n, dtype=torch.bool),
            "bernoulli": torch.rand(n, generator=g) < 0.4, "first": first, "last": last,
            "alternating": (torch.arange(n) % 2) == 0}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17, 200_003])
def test_compaction_equals_torch_nonzero(n):
    dev = _dev()
    wi, dr = _vectors(n, 1), _vectors(n, 2)
    for name, mask in _masks(n).items():
        mask = mask.to(dev)
        for flags in (0, 1, 2, 3):
            live = mask.clone()
            if flags & 1:
                live &= wi[:, 2] > 0
            if flags & 2:
                live &= dr[:, 2] > 0
            want = torch.nonzero(live).flatten()
            wo, pdf, pdf2 = (torch.full((n, 3), -7.0, device=dev), torch.full((n,), -7.0, device=dev),
                             torch.full((n,), -7.0, device=dev))
            # uint8 and bool masks, NULL mask for the all-live case
            act = None if name == "all_live" and flags else (mask.to(torch.uint8) * 3 if flags == 1 else mask)
            rows, k = _compact(act, wi if flags & 1 else None, dr if flags & 2 else None, flags, n, (wo, pdf, pdf2))
            assert k == want.numel(), (name, flags, k, want.numel())
            assert torch.equal(rows[:k], want), (name, flags)
            assert (wo[~live] == 0).all() and (pdf[~live] == 0).all() and (pdf2[~live] == 0).all(), (name, flags)
            assert (wo[live] == -7).all() and (pdf[live] == -7).all() and (pdf2[live] == -7).all(), (name, flags)
            rows2, k2 = _compact(act, wi if flags & 1 else None, dr if flags & 2 else None, flags, n)   # no arrays to zero
            assert k2 == k and torch.equal(rows2[:k], rows[:k]), (name, flags)


def test_live_rows_host_wrapper():
    from bsdf_diffusion_sampling_amd import live
    dev = _dev()
    n = 3 * B + 17
    wi, dr = _vectors(n, 3), _vectors(n, 4)
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.4).to(dev)
    pdf = torch.full((n,), -7.0, device=dev)
    rows = live.live_rows(mask, wi=wi, dir=dr, flags=live.LIVE_WI_UPPER | live.LIVE_DIR_UPPER, zero=(None, pdf))
    keep = mask & (wi[:, 2] > 0) & (dr[:, 2] > 0)
    assert torch.equal(rows, torch.nonzero(keep).flatten()) and (pdf[~keep] == 0).all() and (pdf[keep] == -7).all()
    assert torch.equal(live.live_rows(None, wi=wi, flags=live.LIVE_WI_UPPER), torch.nonzero(wi[:, 2] > 0).flatten())
    assert live.live_rows(torch.zeros(0, dtype=torch.bool, device=dev)).numel() == 0
    with pytest.raises(ValueError):
        live.live_rows(mask, wi=wi[:-1].contiguous(), flags=1)
    with pytest.raises(ValueError):
        live.live_rows(mask.float())


def _dirs(n, seed):
    """Unit vectors from BOTH hemispheres."""
    g = torch.Generator().manual_seed(seed)
    z = (0.03 + 0.92 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.7, 1.0, -1.0)
    ph = 6.2831853 * torch.rand(n, generator=g)
    r = torch.sqrt(1 - z * z)
    return torch.stack([r * torch.cos(ph), r * torch.sin(ph), z], 1).float().to(_dev())


def _launches(s):
    return s.profile_read()[0]


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
@pytest.mark.parametrize("tile", [32, 16])
@pytest.mark.parametrize("stem,variant", [("chm_orange_rgb_disk", 0), ("aniso_miro_7_rgb_spherical", 0), ("bsdf_3_spherical", 1)])
def test_masked_calls_equal_unmasked_calls_on_live_rows(stem, variant, tile, binding):
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    dev = _dev()
    _, fw = load_case(stem)
    s = FlowSampler(fw, tile=tile, binding=binding)
    T = 4 if fw.domain == 0 else 8
    m = 5000
    wi, wl = _dirs(m, 1), _dirs(m, 2)
    mask = (torch.rand(m, generator=torch.Generator().manual_seed(3)) < 0.4).to(dev)
    dead = ~mask
    sent = lambda *shape: torch.full(shape, -7.0, device=dev)   # noqa: E731
    # ---- sample
    wo_u, pdf_u = s.plugin_sample(wi, None, T=T, variant=variant, seed=9, offset=100)
    wo, pdf = s.plugin_sample(wi, None, T=T, variant=variant, seed=9, offset=100, active=mask)
    assert torch.equal(wo[mask], wo_u[mask]) and torch.equal(pdf[mask], pdf_u[mask])
    assert (wo[dead] == 0).all() and (pdf[dead] == 0).all()
    wo_b, pdf_b = sent(m, 3), sent(m)
    r = s.plugin_sample(wi, None, T=T, variant=variant, seed=9, offset=100, out=(wo_b, pdf_b), active=mask.to(torch.uint8))
    assert r[0] is wo_b and r[1] is pdf_b and torch.equal(wo_b, wo) and torch.equal(pdf_b, pdf)
    # ---- pdf: equal on EVERY row whose mask is set, the rows the hemisphere flags culled included
    p_u = s.plugin_pdf(wi, wl, T=T, variant=variant)
    p = s.plugin_pdf(wi, wl, T=T, variant=variant, active=mask)
    assert torch.equal(p[mask], p_u[mask]) and (p[dead] == 0).all()
    p_b = sent(m)
    s.plugin_pdf(wi, wl, T=T, variant=variant, out=p_b, active=mask)
    assert torch.equal(p_b, p)
    if variant == 0:
        culled = mask & ((wi[:, 2] <= 0) | (wl[:, 2] <= 0))
        assert int(culled.sum()) > 100 and (p_u[culled] == 0).all()
    # ---- fused sample + pdf: in-kernel draw, then an injected x0
    x0 = 0.3 * torch.randn(m, 2, generator=torch.Generator().manual_seed(4)).to(dev)
    for x, kw in ((None, dict(seed=9, offset=100)), (x0, {})):
        f_u = s.plugin_sample_pdf(wi, wl, x, T=T, variant=variant, **kw)
        f = s.plugin_sample_pdf(wi, wl, x, T=T, variant=variant, active=mask, **kw)
        f_b = s.plugin_sample_pdf(wi, wl, x, T=T, variant=variant, active=mask, out=(sent(m, 3), sent(m), sent(m)), **kw)
        for a, b, u in zip(f, f_b, f_u):
            assert torch.equal(a[mask], u[mask]) and (a[dead] == 0).all() and torch.equal(a, b)
    # ---- an all-live mask is the plain call
    ones = torch.ones(m, dtype=torch.bool, device=dev)
    a = s.plugin_sample(wi, None, T=T, variant=variant, seed=9, offset=100, active=ones)
    assert torch.equal(a[0], wo_u) and torch.equal(a[1], pdf_u)
    if variant == 1:   # (the measured variants cull by hemisphere on top of the mask: covered above)
        assert torch.equal(s.plugin_pdf(wi, wl, T=T, variant=variant, active=ones), p_u)
    else:
        up = _dirs(m, 6).abs().contiguous()
        assert torch.equal(s.plugin_pdf(up, up.flip(0).contiguous(), T=T, variant=variant, active=ones),
                           s.plugin_pdf(up, up.flip(0).contiguous(), T=T, variant=variant))
    a = s.plugin_sample_pdf(wi, wl, None, T=T, variant=variant, seed=9, offset=100, active=ones)
    u = s.plugin_sample_pdf(wi, wl, None, T=T, variant=variant, seed=9, offset=100)
    assert all(torch.equal(x, y) for x, y in zip(a, u))
    # ---- an all-dead mask: zeros, and no flow kernel is launched
    none = torch.zeros(m, dtype=torch.bool, device=dev)
    s.set_profiling(True)
    before = _launches(s)
    z = s.plugin_sample(wi, None, T=T, variant=variant, seed=9, active=none, out=(sent(m, 3), sent(m)))
    zp = s.plugin_pdf(wi, wl, T=T, variant=variant, active=none, out=sent(m))
    zf = s.plugin_sample_pdf(wi, wl, None, T=T, variant=variant, seed=9, active=none, out=(sent(m, 3), sent(m), sent(m)))
    assert _launches(s) == before
    s.plugin_pdf(wi, wl, T=T, variant=variant, active=mask)
    assert _launches(s) == before + 1                      # (the counter does move when a flow kernel runs)
    s.set_profiling(False)
    assert all((t == 0).all() for t in (*z, zp, *zf))
    # ---- a mask cannot be combined with what is indexed by the call's own rows
    idx = torch.arange(m, device=dev)
    ctx = s.new_context(m)
    with pytest.raises(ValueError):
        s.plugin_sample(wi, None, T=T, variant=variant, active=mask, row_index=idx)
    with pytest.raises(ValueError):
        s.plugin_sample(wi, None, T=T, variant=variant, active=mask, ctx_out=ctx)
    with pytest.raises(ValueError):
        s.plugin_sample(wi, None, T=T, variant=variant, active=mask, ctx_in=ctx)
    with pytest.raises(ValueError):
        s.plugin_pdf(wi, wl, T=T, variant=variant, active=mask, row_index=idx)
    with pytest.raises(ValueError):
        s.plugin_pdf(wi, wl, T=T, variant=variant, active=mask, ctx_in=ctx)
    with pytest.raises(ValueError):
        s.plugin_pdf(wi, wl, T=T, variant=variant, active=mask, ctx_out=ctx)
    with pytest.raises(ValueError):
        s.plugin_sample_pdf(wi, wl, None, T=T, variant=variant, active=mask, row_index=idx)
    with pytest.raises(RuntimeError):
        s.plugin_sample(wi, None, T=T, variant=variant, active=mask[:-1])            # wrong length
    with pytest.raises(RuntimeError):
        s.plugin_sample(wi, None, T=T, variant=variant, active=mask.cpu())           # host tensor
    s.close()


@pytest.mark.parametrize("stem,variant", [("chm_orange_rgb_disk", 0), ("aniso_miro_7_rgb_spherical", 0), ("bsdf_3_spherical", 1)])
def test_single_handle_fused_ex_entry_point(stem, variant):
    """bsdfd_plugin_sample_pdf_ex: NULL opts = bsdfd_plugin_sample_pdf; with a row_index = the one-handle _multi_ex call."""
    from bsdf_diffusion_sampling_amd import _lib
    from bsdf_diffusion_sampling_amd.sampler import FlowSampler
    dev = _dev()
    _, fw = load_case(stem)
    s = FlowSampler(fw, binding="ctypes")
    L = _lib.lib()
    T = 4 if fw.domain == 0 else 8
    m, n = 5000, 3217
    wi, wl = _dirs(m, 1), _dirs(m, 2)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    outs = lambda: (torch.full((m, 3), -7.0, device=dev), torch.full((m,), -7.0, device=dev), torch.full((m,), -7.0, device=dev))  # noqa: E731
    a, b = outs(), outs()
    _lib.check(L.bsdfd_plugin_sample_pdf(s._h, variant, _ptr(wi), None, _ptr(wl), 9, 100, m, T, *[_ptr(t) for t in a], st))
    _lib.check(L.bsdfd_plugin_sample_pdf_ex(s._h, variant, _ptr(wi), None, _ptr(wl), 9, 100, m, T, *[_ptr(t) for t in b], None, st))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(3))[:n].to(dev)
    o = _lib.opts(row_index=rows)
    a, b = outs(), outs()
    hs, ends = (C.c_void_p * 1)(s._h), (C.c_int64 * 1)(n)
    _lib.check(L.bsdfd_plugin_sample_pdf_multi_ex(hs, 1, ends, variant, _ptr(wi), None, _ptr(wl), 9, 100, T, *[_ptr(t) for t in a],
                                                  C.byref(o), st))
    _lib.check(L.bsdfd_plugin_sample_pdf_ex(s._h, variant, _ptr(wi), None, _ptr(wl), 9, 100, n, T, *[_ptr(t) for t in b],
                                            C.byref(o), st))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert (b[1][rows] != -7).all() and int((b[1] == -7).sum()) == m - n
    # ... and through both host bindings' row_index argument
    for binding in ("ctypes", "torch"):
        s2 = FlowSampler(fw, binding=binding)
        c = s2.plugin_sample_pdf(wi, wl, None, T=T, variant=variant, seed=9, offset=100, out=outs(), row_index=rows)
        assert all(torch.equal(x, y) for x, y in zip(b, c))
        s2.close()
    # inherited rules: no per-query context, N >= 0
    ctx = s.new_context(m)
    o2 = _lib.opts(ctx_out=ctx)
    assert L.bsdfd_plugin_sample_pdf_ex(s._h, variant, _ptr(wi), None, _ptr(wl), 9, 100, m, T, *[_ptr(t) for t in b],
                                        C.byref(o2), st) == 1
    assert L.bsdfd_plugin_sample_pdf_ex(s._h, variant, _ptr(wi), None, _ptr(wl), 9, 100, -1, T, *[_ptr(t) for t in b], None, st) == 1
    s.close()


def _plugin(kind, **extra):
    if kind == "disk":
        from bsdf_diffusion_sampling_amd.brdf_measured_disk import MyBSDF
    else:
        from bsdf_diffusion_sampling_amd.brdf_measured_spherical import MyBSDF
    return MyBSDF({"filename": "chm_orange_rgb", "albedo": [0.8, 0.7, 0.6], "measured_dir": os.path.join(ROOT, "tests", "golden"),
                   **extra})


@pytest.mark.parametrize("kind", ["disk", "spherical"])
def test_plugin_methods_honour_active(kind):
    from bsdf_diffusion_sampling_amd.plugin_base import SurfaceInteraction
    dev = _dev()
    n = 5000
    plug, legacy = _plugin(kind), _plugin(kind, compact_active=False)
    assert plug.compact_active and not legacy.compact_active and plug._fused_gt() is not None
    si, wo_q = SurfaceInteraction(_dirs(n, 1)), _dirs(n, 2)
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.4).to(dev)
    dead = ~mask
    bs_u, w_u = plug.sample(None, si, seed=21)
    bs, w = plug.sample(None, si, active=mask, seed=21)
    for a, u in ((w, w_u), (bs.pdf, bs_u.pdf), (bs.wo, bs_u.wo)):
        assert torch.equal(a[mask], u[mask]) and (a[dead] == 0).all()
    assert int((bs.pdf[mask] > 0).sum()) > 100 and int((w[mask] > 0).any(1).sum()) > 100     # (not vacuous)
    p_u = plug.pdf(None, si, wo_q)
    p = plug.pdf(None, si, wo_q, active=mask)
    assert torch.equal(p[mask], p_u[mask]) and (p[dead] == 0).all() and int((p[mask] > 0).sum()) > 100
    e, p2 = plug.eval_pdf(None, si, wo_q, active=mask)
    assert torch.equal(p2, p) and torch.equal(e, plug.eval(None, si, wo_q))
    # active=True is the call without a mask; a Python False kills every lane
    assert torch.equal(plug.pdf(None, si, wo_q, active=True), p_u)
    assert (plug.pdf(None, si, wo_q, active=False) == 0).all()
    # props["compact_active"] = False: the flow runs on every lane, the mask reaches the weight pass only (as before)
    bs_l, w_l = legacy.sample(None, si, active=mask, seed=21)
    w_ref, pdf_ref = legacy.bsdf.sample_weight(si.wi, bs_u.wo, legacy.sample_t(si.wi, seed=21)[1], tint=legacy.albedo,
                                               firefly_threshold=legacy.FIREFLY, active=mask)
    assert torch.equal(bs_l.wo, bs_u.wo) and torch.equal(bs_l.pdf, pdf_ref) and torch.equal(w_l, w_ref)
    assert torch.equal(w_l[mask], w_u[mask]) and (w_l[dead] == 0).all() and (bs_l.wo[dead] != 0).any()
    assert torch.equal(legacy.pdf(None, si, wo_q, active=mask), p_u)
    # the tensor core takes the mask directly, fused call included
    f_u = plug.sample_pdf_t(si.wi, wo_q, seed=21)
    f = plug.sample_pdf_t(si.wi, wo_q, seed=21, active=mask)
    for a, u in zip(f, f_u):
        assert torch.equal(a[mask], u[mask]) and (a[dead] == 0).all()


@pytest.mark.parametrize("kind", ["disk", "spherical"])
@pytest.mark.parametrize("gt", [False, True])
def test_renderer_skip_misses_gives_the_same_film(kind, gt):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    plug = _plugin(kind) if gt else _plugin(kind, measured=False)
    cam = WF.Camera(width=64, height=48)
    films = {}
    for skip in (False, True):
        r = WF.WavefrontRenderer(plug, cam, skip_misses=skip)
        if skip:
            b = r.primary(0, cam.height, 4, seed=7, pass_idx=0)
            hit = b["mat"] == 0
            assert 0.05 < float(hit.float().mean()) < 0.95                       # the frame has hits AND misses
            assert torch.equal(hit, (b["nrm"] != 0).any(1))
        films[skip] = r.render(passes=2, spp=4, seed=7)
    torch.cuda.synchronize()
    assert torch.isfinite(films[False]).all() and films[False].abs().sum() > 0
    assert torch.equal(films[True], films[False])
