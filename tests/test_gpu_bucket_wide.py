"""bsdfd_bucket_by_material_wide (ABI 7; csrc/bucket_wide.hip): the stable sort of a wavefront by material id for up to 65536
materials — the batched form of one `mybsdf` instance per material dispatched lane by lane.  The oracle is EXACT: the valid
rows in torch.argsort(stable=True) order, and torch.bincount of their ids."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd.sharding import bucket_by_material, bucket_by_material_native  # noqa: E402

EINVAL = 1   # BSDFD_EINVAL
WIDTHS = [65, 79, 256, 257, 4095, 4096, 4097, 65536]   # digit boundaries of a 6-bit and of an 8-bit radix
N_PATTERN = 3 * 4096 + 17                              # three full blocks of the 4096-row chunking and a ragged one


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def _expected(ids, m):
    """(perm over the valid rows, counts) on the CPU."""
    valid = (ids >= 0) & (ids < m)
    kept = ids[valid]
    return torch.nonzero(valid)[:, 0][torch.argsort(kept, stable=True)], torch.bincount(kept, minlength=m)


def _check(ids, m, run=bucket_by_material_native):
    perm, counts = run(ids.to(_dev()), m)
    exp_perm, exp_counts = _expected(ids, m)
    assert perm.dtype == torch.int64 and counts.dtype == torch.int64
    assert perm.shape == ids.shape and counts.shape == (m,)
    assert torch.equal(counts.cpu(), exp_counts)
    assert int(counts.sum()) == exp_perm.shape[0]
    assert torch.equal(perm.cpu()[: exp_perm.shape[0]], exp_perm)


def _raw(ids_dev, m, perm=None, ws=None, stream=None):
    """The C entry point through ctypes, on caller-made buffers."""
    L = _lib.lib()
    n = ids_dev.shape[0]
    need = L.bsdfd_bucket_wide_workspace_bytes(n, m)
    assert need > 0
    perm = torch.empty(n, dtype=torch.int64, device=ids_dev.device) if perm is None else perm
    ws = torch.empty(need, dtype=torch.uint8, device=ids_dev.device) if ws is None else ws
    counts = torch.empty(m, dtype=torch.int64, device=ids_dev.device)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = L.bsdfd_bucket_by_material_wide(C.c_void_p(ids_dev.data_ptr()), n, m, C.c_void_p(perm.data_ptr()),
                                         C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                         C.c_void_p(st.cuda_stream))
    assert rc == 0, L.bsdfd_last_error().decode()
    return perm, counts


def _uniform(n, m, seed=0):
    return torch.randint(0, m, (n,), generator=torch.Generator().manual_seed(seed + n + m))


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, N_PATTERN])
def test_wide_bucketing_equals_stable_argsort(n, m):
    _check(_uniform(n, m), m)


def test_wide_bucketing_of_1Mi_rows_over_65536_materials():
    _check(_uniform((1 << 20) + 3, 65536), 65536)


def _patterns(m):
    n = N_PATTERN
    top = 64 ** (2 if m > 4096 else 1)                       # weight of the highest 6-bit digit of an id below m
    hi = (m - 1) // top * top
    lo = min(5, m - 1 - hi)
    runs = _uniform(n, m, 1)
    runs[: n // 3] = m - 1
    return {
        "all_zero": torch.zeros(n, dtype=torch.int64),
        "all_last": torch.full((n,), m - 1, dtype=torch.int64),
        "descending": (m - 1 - torch.arange(n) % m),
        "two_ids_highest_digit": torch.where(_uniform(n, 2, 2) == 1, torch.tensor(hi + lo), torch.tensor(lo)),
        "long_run": runs,
    }


@pytest.mark.parametrize("pattern", ["all_zero", "all_last", "descending", "two_ids_highest_digit", "long_run"])
@pytest.mark.parametrize("m", WIDTHS)
def test_wide_bucketing_patterns(m, pattern):
    ids = _patterns(m)[pattern]
    assert ids.dtype == torch.int64 and int(ids.min()) >= 0 and int(ids.max()) < m
    if pattern == "two_ids_highest_digit":
        assert ids.unique().numel() == 2
    _check(ids, m)


@pytest.mark.parametrize("m", WIDTHS)
def test_rows_outside_the_table_are_left_out(m):
    """About one row in ten carries an id outside [0, m), among them ids whose low bits alias a valid one."""
    n = N_PATTERN
    g = torch.Generator().manual_seed(m)
    ids = _uniform(n, m, 3)
    bad = torch.tensor([-1, m, m + 64, 2 ** 31, 2 ** 40 + 3, -2 ** 40])
    out = torch.rand(n, generator=g) < 0.1
    ids[out] = bad[torch.randint(0, bad.numel(), (int(out.sum()),), generator=g)]
    assert 0 < int(((ids < 0) | (ids >= m)).sum()) < n
    _check(ids, m)
    none_valid = bad[torch.randint(0, bad.numel(), (n,), generator=g)]
    _, counts = bucket_by_material_native(none_valid.to(_dev()), m)
    assert torch.equal(counts.cpu(), torch.zeros(m, dtype=torch.int64))


@pytest.mark.parametrize("m", [79, 4097])
def test_raw_entry_point_is_independent_of_workspace_and_perm_contents(m):
    n = N_PATTERN
    ids = _uniform(n, m, 4)
    ids[::7] = -1
    ids_dev = ids.to(_dev())
    need = _lib.lib().bsdfd_bucket_wide_workspace_bytes(n, m)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=_dev())
    perm = torch.full((n,), -1, dtype=torch.int64, device=_dev())      # 0xFF in every byte
    p1, c1 = _raw(ids_dev, m, perm=perm, ws=ws)
    p1, c1 = p1.clone(), c1.clone()
    p2, c2 = _raw(ids_dev, m, perm=perm, ws=ws)                        # ... and on what the first run left behind
    exp_perm, exp_counts = _expected(ids, m)
    k = exp_perm.shape[0]
    assert torch.equal(c1.cpu(), exp_counts) and torch.equal(c2.cpu(), exp_counts)
    assert torch.equal(p1.cpu()[:k], exp_perm) and torch.equal(p2.cpu()[:k], exp_perm)


def test_raw_entry_point_rejects_bad_sizes():
    L = _lib.lib()
    n = 5000
    ids = _uniform(n, 79).to(_dev())
    need = L.bsdfd_bucket_wide_workspace_bytes(n, 79)
    perm = torch.empty(n, dtype=torch.int64, device=_dev())
    counts = torch.empty(65537, dtype=torch.int64, device=_dev())
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())

    def call(m, nbytes):
        return L.bsdfd_bucket_by_material_wide(C.c_void_p(ids.data_ptr()), n, m, C.c_void_p(perm.data_ptr()),
                                               C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, None)
    assert call(79, need - 1) == EINVAL and "workspace" in L.bsdfd_last_error().decode()
    assert call(0, need) == EINVAL and "n_materials" in L.bsdfd_last_error().decode()
    assert call(65537, need) == EINVAL and "n_materials" in L.bsdfd_last_error().decode()
    assert call(79, need) == 0
    with pytest.raises(ValueError, match="n_materials"):
        bucket_by_material_native(ids, 65537)
    # the dispatcher hands a table wider than its native limit to torch, same contract
    perm_t, counts_t = bucket_by_material(ids, 65537)
    assert torch.equal(perm_t.cpu(), torch.argsort(ids.cpu(), stable=True)) and int(counts_t.sum()) == n


def test_side_stream_needs_no_host_sync():
    """Everything is enqueued on the caller's stream: the next kernel on that stream reads perm / counts, no synchronise between."""
    dev = _dev()
    n, m = (1 << 18) + 5, 4097
    ids = _uniform(n, m, 5)
    ids_dev = ids.to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        perm, counts = _raw(ids_dev, m, stream=side)
        sorted_ids = ids_dev[perm]                    # enqueued behind the sort on the same stream
        total = counts.sum()
    side.synchronize()
    assert int(total) == n
    assert torch.equal(sorted_ids.cpu(), torch.sort(ids, stable=True).values)
    assert torch.equal(perm.cpu(), torch.argsort(ids, stable=True))


def test_table_of_all_77_shipped_sets_with_two_extra_bins():
    """MaterialTable over every parsable shipped set (27 disk + 25 measured spherical + 25 bsdf_*) with floor / miss bins: 79
    ids, past the one-pass sort.  sample() and pdf() through the table, gathered and direct, equal a loop over the materials
    that calls each FlowSampler on its lanes, bit for bit; the lanes of the extra bins come back zero."""
    from bsdf_diffusion_sampling_amd import weights as W
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    dev = _dev()
    tab = MaterialTable(W.list_shipped("disk") + W.list_shipped("spherical"))
    assert len(tab) == 77 and sum(s.startswith("bsdf_") for s in tab.stems) == 25
    n, extra = 8192, 2
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, len(tab) + extra, (n,), generator=g)
    z = 0.05 + 0.9 * torch.rand(n, generator=g)
    ph = 6.2831853 * torch.rand(n, generator=g)
    r = torch.sqrt(1 - z * z)
    wi = torch.stack([r * torch.cos(ph), r * torch.sin(ph), z], 1).float().to(dev)
    x0 = (0.3 * torch.randn(n, 2, generator=g)).to(dev)
    ids_dev = ids.to(dev)
    plan = tab.bucket(ids_dev, extra)
    exp_perm, exp_counts = _expected(ids, len(tab) + extra)
    assert torch.equal(plan[0].cpu(), exp_perm) and plan[1] == exp_counts.tolist()
    # the loop the table replaces: one plugin call per material on its lanes
    wo_ref = torch.zeros(n, 3, device=dev)
    pdf_ref = torch.zeros(n, device=dev)
    p_ref = torch.zeros(n, device=dev)
    for m, s in enumerate(tab.samplers):
        rows = (ids_dev == m).nonzero()[:, 0]
        assert rows.numel() > 0
        wo_m, pdf_m = s.plugin_sample(wi[rows].contiguous(), x0[rows].contiguous(), T=tab.T[m], variant=tab.variant[m])
        wo_ref[rows], pdf_ref[rows] = wo_m, pdf_m
        p_ref[rows] = s.plugin_pdf(wi[rows].contiguous(), wo_m, T=tab.T[m], variant=tab.variant[m])

    def same_bits(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    for direct in (False, True):
        wo, pdf = tab.sample(plan, wi, x0=x0, direct=direct)
        p = tab.pdf(plan, wi, wo_ref, direct=direct)
        assert same_bits(wo, wo_ref) and same_bits(pdf, pdf_ref) and same_bits(p, p_ref), f"direct={direct}"
    no_material = ids_dev >= len(tab)
    assert int(no_material.sum()) > 0
    assert (wo[no_material] == 0).all() and (pdf[no_material] == 0).all() and (p[no_material] == 0).all()
