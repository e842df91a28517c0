"""bsdfd_bucket_by_material_wide (ABI 7; csrc/bucket_wide.hip) — what is decided on the host: the workspace size and the
argument checks, all of which come before any HIP call, and the dispatch of ``sharding.bucket_by_material``."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from bsdf_diffusion_sampling_amd import _lib  # noqa: E402
from bsdf_diffusion_sampling_amd.sharding import bucket_by_material, bucket_by_material_native  # noqa: E402

EINVAL = 1   # BSDFD_EINVAL


def test_workspace_bytes():
    size = _lib.lib().bsdfd_bucket_wide_workspace_bytes
    ns = [0, 1, 4095, 4096, 4097, 1 << 20, (1 << 24) + 3]
    ms = [1, 64, 65, 79, 4096, 4097, 65536]
    for m in ms:
        got = [size(n, m) for n in ns]
        assert min(got) > 0 and got == sorted(got), (m, got)
    for n in ns:
        got = [size(n, m) for m in ms]
        assert got == sorted(got), (n, got)
    # a spare permutation is part of it as soon as there are two passes
    assert size(1 << 20, 65) >= (1 << 20) * 8
    for n, m in [(-1, 79), (10, 0), (10, -5), (10, 65537)]:
        assert size(n, m) == 0


@pytest.mark.parametrize("args,names", [
    (dict(n=-1), "N"),
    (dict(m=0), "n_materials"),
    (dict(m=65537), "n_materials"),
    (dict(counts=None), "counts"),
    (dict(n=0, counts=None), "counts"),
    (dict(ids=None), "material_id"),
    (dict(perm=None), "perm"),
    (dict(ws=None), "workspace"),
])
def test_bad_arguments_are_rejected_before_any_hip_call(args, names):
    """The pointers are never dereferenced: every case returns before the first HIP call, so host buffers (or none) will do."""
    L = _lib.lib()
    n, m = args.get("n", 100), args.get("m", 79)
    buf = (C.c_int64 * 1024)()
    addr = C.addressof(buf)
    p = {k: C.c_void_p(addr) if args.get(k, 1) is not None else None for k in ("ids", "perm", "counts", "ws")}
    rc = L.bsdfd_bucket_by_material_wide(p["ids"], n, m, p["perm"], p["counts"], p["ws"], 1 << 40, None)
    assert rc == EINVAL
    assert names in L.bsdfd_last_error().decode()


def test_short_or_misaligned_workspace_is_rejected_before_any_hip_call():
    L = _lib.lib()
    buf = (C.c_int64 * 16)()
    a = C.c_void_p(C.addressof(buf))
    need = L.bsdfd_bucket_wide_workspace_bytes(100, 79)
    assert L.bsdfd_bucket_by_material_wide(a, 100, 79, a, a, a, need - 1, None) == EINVAL
    assert "workspace" in L.bsdfd_last_error().decode()
    assert L.bsdfd_bucket_by_material_wide(a, 100, 79, a, a, C.c_void_p(C.addressof(buf) + 4), need, None) == EINVAL
    assert "aligned" in L.bsdfd_last_error().decode()


def test_cpu_tensors_take_the_torch_path():
    ids = torch.randint(0, 100, (5000,), generator=torch.Generator().manual_seed(0))
    perm, counts = bucket_by_material(ids, 100)
    assert perm.dtype == torch.int64 and counts.dtype == torch.int64
    assert torch.equal(perm, torch.argsort(ids, stable=True)) and torch.equal(counts, torch.bincount(ids, minlength=100))


def test_the_native_wrapper_does_not_fall_back():
    ids = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError, match="CUDA"):
        bucket_by_material_native(ids, 100)
    with pytest.raises(ValueError, match="CUDA"):
        bucket_by_material_native(ids, 5)
