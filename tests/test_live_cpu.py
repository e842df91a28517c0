"""bsdfd_compact_live (csrc/live.hip, ABI 8) without a GPU: the workspace size and every argument check — the entry point
refuses bad arguments before its first HIP call, so host buffers are enough (nothing is dereferenced)."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")


def _lib():
    from bsdf_diffusion_sampling_amd import _lib
    return _lib, _lib.lib()


def test_live_workspace_bytes():
    _, L = _lib()
    sizes = [0, 1, 63, 64, 65, 4095, 4096, 4097, 200_003, 1 << 20, 1 << 24, (1 << 31) + 5]
    got = [int(L.bsdfd_live_workspace_bytes(n)) for n in sizes]
    assert all(b > 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[-2] > got[-3] > got[0]
    assert L.bsdfd_live_workspace_bytes(-1) == 0 and L.bsdfd_live_workspace_bytes(-(1 << 40)) == 0


def test_compact_live_argument_checks():
    lib, L = _lib()
    n = 100
    need = int(L.bsdfd_live_workspace_bytes(n))
    ws = (C.c_uint64 * (need // 8 + 2))()                      # 8-byte aligned host scratch
    rows, count = (C.c_int64 * n)(), (C.c_int64 * 1)()
    act = (C.c_ubyte * n)()
    vec = (C.c_float * (3 * n))()
    p = lambda a, off=0: C.c_void_p(C.addressof(a) + off)      # noqa: E731
    good = dict(active=p(act), wi=p(vec), dir=p(vec), flags=3, n=n, rows=p(rows), count=p(count), zw=None, zp=None, zp2=None,
                ws=p(ws), ws_bytes=need, stream=None)

    def call(**kw):
        a = {**good, **kw}
        rc = L.bsdfd_compact_live(a["active"], a["wi"], a["dir"], a["flags"], a["n"], a["rows"], a["count"], a["zw"], a["zp"],
                                  a["zp2"], a["ws"], a["ws_bytes"], a["stream"])
        return rc, L.bsdfd_last_error().decode()

    EINVAL = 1
    for kw, word in ((dict(n=-1), "N"), (dict(rows=None), "rows"), (dict(count=None), "count"), (dict(ws=None), "workspace"),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace"), (dict(ws=p(ws, 4)), "workspace"),
                     (dict(ws=p(ws, 1)), "aligned"), (dict(flags=4), "flags"), (dict(flags=-1), "flags"), (dict(flags=1 << 20), "flags"),
                     (dict(flags=1, wi=None), "wi"), (dict(flags=3, wi=None), "wi"), (dict(flags=2, dir=None), "dir"),
                     (dict(flags=3, dir=None), "dir")):
        rc, msg = call(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    # a workspace sized for fewer rows than the call's is short
    rc, msg = call(n=1 << 20)
    assert rc == EINVAL and "workspace" in msg


def test_live_rows_refuses_cpu_tensors():
    from bsdf_diffusion_sampling_amd.live import live_rows
    with pytest.raises(ValueError, match="CUDA"):
        live_rows(torch.ones(8, dtype=torch.bool))
    with pytest.raises(ValueError, match="CUDA"):
        live_rows(None, wi=torch.zeros(8, 3), flags=1)
    with pytest.raises(ValueError):
        live_rows(None)


def test_abi_8_symbols_are_bound():
    lib, L = _lib()
    assert lib.ABI_VERSION == 8 and L.bsdfd_abi_version() == 8
    for name in ("bsdfd_live_workspace_bytes", "bsdfd_compact_live", "bsdfd_plugin_sample_pdf_ex"):
        assert name in lib.EXPORTS and getattr(L, name).argtypes
    from bsdf_diffusion_sampling_amd import torch_ext
    assert "plugin_sample_pdf_ex_out" in torch_ext.OPS
