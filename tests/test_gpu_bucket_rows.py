"""GPU tests of ``bsdfd_bucket_rows`` (csrc/bucket.hip): the one-pass stable counting sort over a row list, exactly the numpy
statement of tests/test_pathtrace_compact_cpu.py (``bucket_rows_ref``).  The sort's block is 4096 rows: the list lengths sit
around it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_pathtrace_compact_cpu import bucket_rows_ref  # noqa: E402

N_IDS = 20000
LENGTHS = (0, 1, 255, 4095, 4096, 4097, 2 * 4096 + 17)
N_MATERIALS = (1, 7, 34, 64)


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda")


def _ids(n_materials, seed=5):
    """20 000 ids, about a third of them outside [0, n_materials): negatives, n_materials and beyond, 2^40 + 3."""
    rng = np.random.default_rng(seed + n_materials)
    ids = rng.integers(0, n_materials, N_IDS).astype(np.int64)
    out = rng.random(N_IDS) < 1 / 3
    ids[out] = rng.choice(np.array([-1, -7, -(1 << 40), n_materials, n_materials + 1, 255, 256, (1 << 40) + 3, (1 << 32) + 1],
                                   dtype=np.int64), int(out.sum()))
    assert 0.25 < out.mean() < 0.42 and (ids == (1 << 40) + 3).any() and (ids < 0).any()
    return ids


def _rows(length, shuffled, seed=3):
    rng = np.random.default_rng(seed + length)
    rows = rng.permutation(N_IDS)[:length].astype(np.int64)
    return rows if shuffled else np.sort(rows)


def _pattern(fill):
    """The int64 that ``perm`` is pre-filled with for the byte ``fill``."""
    return (fill * 0x0101010101010101) & 0x7FFFFFFFFFFFFFFF


def _sort(ids_d, rows, n_materials, fill):
    """One call of the entry point with ``perm`` and the workspace pre-filled with the byte ``fill`` -> (perm, counts)."""
    from bsdf_diffusion_sampling_amd import _lib
    L, dev = _lib.lib(), ids_d.device
    p = lambda t: C.c_void_p(t.data_ptr())
    rows_d = torch.from_numpy(rows).to(dev)
    n = len(rows)
    perm = torch.full((max(n, 1),), _pattern(fill), dtype=torch.int64, device=dev)
    counts = torch.full((n_materials,), -5, dtype=torch.int64, device=dev)
    ws = torch.full((max(int(L.bsdfd_bucket_workspace_bytes(n, n_materials)), 1),), fill, dtype=torch.uint8, device=dev)
    rc = L.bsdfd_bucket_rows(p(ids_d), p(rows_d), n, n_materials, p(perm), p(counts), p(ws), ws.numel(), None)
    assert rc == 0, L.bsdfd_last_error()
    torch.cuda.synchronize()
    return perm.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("n_materials", N_MATERIALS)
def test_bucket_rows_is_the_numpy_statement(n_materials, shuffled):
    dev = _gpu()
    ids = _ids(n_materials)
    ids_d = torch.from_numpy(ids).to(dev)
    for length in LENGTHS:
        rows = _rows(length, shuffled)
        want_perm, want_counts = bucket_rows_ref(ids, rows, n_materials)
        for fill in (0x00, 0xA5):                        # the result does not depend on what perm and the workspace held
            perm, counts = _sort(ids_d, rows, n_materials, fill)
            assert np.array_equal(counts, want_counts), (length, fill)
            assert np.array_equal(perm[: counts.sum()], want_perm), (length, fill)   # (entries past sum(counts): unspecified)
        if length >= 255:
            assert 0 < want_counts.sum() < length         # some kept, some left out
    assert np.array_equal(ids_d.cpu().numpy(), ids)


def test_an_ascending_list_of_every_lane_is_the_full_plan_s_kept_prefix():
    from bsdf_diffusion_sampling_amd.sharding import bucket_by_material_native
    dev = _gpu()
    ids = _ids(7)
    ids_d = torch.from_numpy(ids).to(dev)
    full_perm, full_counts = bucket_by_material_native(ids_d, 7)
    perm, counts = _sort(ids_d, np.arange(N_IDS, dtype=np.int64), 7, 0x5A)
    assert np.array_equal(counts, full_counts.cpu().numpy())
    assert np.array_equal(perm[: counts.sum()], full_perm.cpu().numpy()[: counts.sum()])


def test_a_list_whose_ids_are_all_out_of_range():
    dev = _gpu()
    ids = _ids(34)
    rows = np.flatnonzero((ids < 0) | (ids >= 34))[:5000].astype(np.int64)
    assert len(rows) == 5000
    perm, counts = _sort(torch.from_numpy(ids).to(dev), rows, 34, 0xFF)
    assert not counts.any() and (perm == _pattern(0xFF)).all()                   # perm untouched: nothing was kept


def test_material_table_bucket_rows():
    """``MaterialTable.bucket_rows``: perm cut to the kept rows, counts on the host; a plan ``sample_pdf(out=)`` accepts."""
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    dev = _gpu()
    table = MaterialTable(["chm_orange_rgb_disk", "aniso_miro_7_rgb_spherical", "vch_silk_blue_rgb_disk"])
    ids = _ids(5)                                       # 3 materials + the floor + ended paths, and ids beyond
    rows = _rows(4097, True)
    want_perm, want_counts = bucket_rows_ref(ids, rows, 4)
    perm, counts = table.bucket_rows(torch.from_numpy(ids).to(dev), torch.from_numpy(rows).to(dev), extra_bins=1)
    assert isinstance(counts, list) and counts == want_counts.tolist() and perm.shape[0] == sum(counts)
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    with pytest.raises(ValueError, match="64"):
        table.bucket_rows(torch.from_numpy(ids).to(dev), torch.from_numpy(rows).to(dev), extra_bins=62)
    with pytest.raises(ValueError):
        table.bucket_rows(torch.from_numpy(ids).to(dev), torch.from_numpy(rows.astype(np.int32)).to(dev))
    with pytest.raises(ValueError):
        table.bucket_rows(torch.from_numpy(ids).to(dev), torch.from_numpy(rows))      # on the host
    with pytest.raises(ValueError):
        table.bucket_rows(torch.from_numpy(ids[:100]).to(dev), torch.from_numpy(rows).to(dev))   # longer than N


def test_errors():
    from bsdf_diffusion_sampling_amd import _lib
    dev = _gpu()
    L, p = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    ids = torch.from_numpy(_ids(7)).to(dev)
    rows = torch.arange(100, dtype=torch.int64, device=dev)
    perm = torch.full((100,), -9, dtype=torch.int64, device=dev)
    counts = torch.full((64,), -9, dtype=torch.int64, device=dev)
    need = int(L.bsdfd_bucket_workspace_bytes(100, 7))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    call = lambda rows_p, n, m, ws_bytes: L.bsdfd_bucket_rows(p(ids), rows_p, n, m, p(perm), p(counts), p(ws), ws_bytes, None)
    for m in (0, 65):
        assert call(p(rows), 100, m, need) == 1 and b"n_materials must be in [1, 64]" in L.bsdfd_last_error()
    assert call(p(rows), 100, 7, need - 1) == 1 and b"workspace" in L.bsdfd_last_error()
    assert call(None, 100, 7, need) == 1 and b"null rows" in L.bsdfd_last_error()
    assert call(p(rows), -1, 7, need) == 1
    torch.cuda.synchronize()
    assert (perm == -9).all() and (counts == -9).all()                              # nothing ran
    assert call(None, 0, 7, 0) == 0                                                 # an empty list only zeroes counts
    torch.cuda.synchronize()
    assert (counts[:7] == 0).all() and (counts[7:] == -9).all() and (perm == -9).all()
