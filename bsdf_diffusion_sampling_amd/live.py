"""Live lanes of a wavefront as a row list (``bsdfd_compact_live``, csrc/live.hip).

Every plugin method of the Mitsuba protocol takes an ``active`` mask (rendering/brdf_measured_disk.py:59,64,101,112); the
flow kernels evaluate the rows a ``row_index`` names, bit for bit as the full call does.  ``live_rows`` is the step between
the two: mask (and, on request, the upper-hemisphere tests of the ``measured`` plugins' pdf) -> ascending row numbers of the
live lanes, with the dead rows of the callers' result arrays zeroed in the same pass.  There is no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Sequence

import torch

from . import _lib

LIVE_WI_UPPER, LIVE_DIR_UPPER = _lib.LIVE_WI_UPPER, _lib.LIVE_DIR_UPPER

_workspace = {}                 # device -> uint8 scratch, grown on demand
_lock = threading.Lock()        # one compaction at a time per process: the scratch is shared (the call ends in a read-back)


def _f32(t, shape, name, dev):
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape
            or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 tensor of shape {list(shape)} on {dev}")
    return C.c_void_p(t.data_ptr())


def live_rows(active: Optional[torch.Tensor], wi: Optional[torch.Tensor] = None, dir: Optional[torch.Tensor] = None,
              flags: int = 0, zero: Sequence[Optional[torch.Tensor]] = (None, None, None)) -> torch.Tensor:
    """Ascending row numbers (int64, on the inputs' device) of the lanes with ``active[i] != 0`` (``active``: bool / uint8
    [N], or None = every lane) that also pass the tests ``flags`` asks for: ``LIVE_WI_UPPER`` — ``wi[i, 2] > 0``,
    ``LIVE_DIR_UPPER`` — ``dir[i, 2] > 0`` (NaN and +-0 are dead, as in the kernels' own guards).  ``zero = (wo [N,3],
    pdf [N], pdf2 [N])``, each optional: their DEAD rows are set to 0 in the same pass, their live rows are left alone.
    One native pass on the current stream plus one read-back of the live count (the call synchronises that stream)."""
    first = next((t for t in (active, wi, dir) if t is not None), None)
    if not isinstance(first, torch.Tensor):
        raise ValueError("live_rows needs a mask or a direction array")
    if not first.is_cuda:
        raise ValueError("live_rows needs CUDA (HIP) tensors: there is no host path")
    dev, n = first.device, first.shape[0]
    if active is not None:
        if (not isinstance(active, torch.Tensor) or active.device != dev or active.dtype not in (torch.bool, torch.uint8)
                or active.dim() != 1):
            raise ValueError(f"active must be a bool / uint8 tensor of shape [N] on {dev}")
        active = active.contiguous()
    wi_p, dir_p = _f32(wi, (n, 3), "wi", dev), _f32(dir, (n, 3), "dir", dev)
    zero = tuple(zero) + (None,) * (3 - len(zero))
    z_p = (_f32(zero[0], (n, 3), "zero[0] (wo)", dev), _f32(zero[1], (n,), "zero[1] (pdf)", dev),
           _f32(zero[2], (n,), "zero[2] (pdf2)", dev))
    L = _lib.lib()
    need = int(L.bsdfd_live_workspace_bytes(n))
    rows = torch.empty((n,), dtype=torch.int64, device=dev)
    if n == 0:
        return rows
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    with _lock, torch.cuda.device(dev):
        ws = _workspace.get(dev)
        if ws is None or ws.numel() < need:
            ws = _workspace[dev] = torch.empty((need,), dtype=torch.uint8, device=dev)
        _lib.check(L.bsdfd_compact_live(None if active is None else C.c_void_p(active.data_ptr()), wi_p, dir_p, int(flags), n,
                                        C.c_void_p(rows.data_ptr()), C.c_void_p(count.data_ptr()), *z_p,
                                        C.c_void_p(ws.data_ptr()), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        k = int(count.item())
    for t in zero:   # written through raw pointers
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return rows[:k]
