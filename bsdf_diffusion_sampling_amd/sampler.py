"""``FlowSampler`` — packed device-side handle of one (material, domain) flow sampler.

Thin host object over the C ABI (include/bsdfd.h).  PyTorch is used only for device
memory and the current HIP stream; all arithmetic happens in the HIP kernels of
csrc/bsdfd.hip.  Checks mirror the contiguity/dtype/device checks of the reference's
only native binding (tiny-cuda-nn/bindings/torch/tinycudann/bindings.cpp:54-73).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import weights as W


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i64(v: int) -> int:
    """uint64 seed / offset -> the int64 the operator schema carries (same 64 bits)."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def default_binding() -> str:
    """'torch' (the operator library torch.ops.bsdfd.*, csrc/torch_ops.cpp) when it has been built, else 'ctypes';
    $BSDFD_HOST_BINDING overrides.  Both are host shims over the same C ABI and the same kernels."""
    import os
    from . import torch_ext
    b = os.environ.get("BSDFD_HOST_BINDING")
    if b:
        if b not in ("ctypes", "torch"):
            raise RuntimeError(f"BSDFD_HOST_BINDING must be 'ctypes' or 'torch', got {b!r}")
        return b
    return "torch" if torch_ext.available() else "ctypes"


class FlowSampler:
    def __init__(self, fw: "W.FlowWeights | str", precision: str = "default", device: Optional[int] = None,
                 binding: Optional[str] = None, tile: int = 0):
        """``binding``: 'ctypes' or 'torch' — which host shim the per-call entry points go through (default:
        ``default_binding()``).  The handle is created through the C ABI either way and is the same object.
        ``tile``: bsdfd_desc.tile — 0 (default), 16 or 32 queries per wave tile.  With 0, ``$BSDFD_TILE=16`` / ``=32`` select the
        16- / 32-query kernels (A/B runs of one build; the LIBRARY reads no environment variable — this host maps it onto the
        field; 32 also selects the opt-in 32-query kernel of the 64 x 6 net and falls back to the default where none exists).
        An explicit ``tile=32`` ARGUMENT for a net / precision without a 32-query kernel raises."""
        if not torch.cuda.is_available():
            raise RuntimeError("FlowSampler needs an MI355X (torch.cuda is unavailable); there is no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        if isinstance(fw, str):
            fw = W.load(fw)
        self.weights = fw.validate()
        self.domain = fw.domain
        L = _lib.lib()
        d = _lib.Desc()
        d.domain, d.width, d.n_hidden, d.pe_bands = fw.domain, fw.width, fw.n_hidden, fw.pe_bands
        d.base_hidden, d.base_pe_bands = fw.base_hidden, fw.base_pe_bands
        d.precision = _lib.PRECISIONS[precision] if isinstance(precision, str) else int(precision)
        d.tile = int(tile)
        env_tile = 0
        if d.tile == 0:
            env_tile = {"16": 16, "32": 32}.get(os.environ.get("BSDFD_TILE", "").strip(), 0)
            d.tile = env_tile   # (32 from the ENVIRONMENT is a preference: also selects the opt-in 32-query kernels, falls back below)
        keep = []
        for name in ("w_in", "w_hidden", "w_out", "base_w1", "base_b1", "base_w2", "base_b2"):
            a = np.ascontiguousarray(getattr(fw, name), dtype=np.float32)
            keep.append(a)
            setattr(d, name, a.ctypes.data_as(C.POINTER(C.c_float)))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = L.bsdfd_create(C.byref(d), C.byref(h))
            if rc != 0 and env_tile == 32 and int(tile) == 0 and b"tile = 32" in L.bsdfd_last_error():
                d.tile = 0   # this net / precision has no 32-query kernel: $BSDFD_TILE=32 then means the library's default
                rc = L.bsdfd_create(C.byref(d), C.byref(h))
            _lib.check(rc)
        self._h = h
        self._L = L
        self.binding = binding or default_binding()
        if self.binding not in ("ctypes", "torch"):
            raise RuntimeError(f"binding must be 'ctypes' or 'torch', got {self.binding!r}")
        self._ops = None
        if self.binding == "torch":
            from . import torch_ext
            self._ops = torch_ext.load()
            self._hi = int(h.value)
        p = C.c_int32()
        _lib.check(L.bsdfd_get_info(h, None, None, None, C.byref(p)))
        self.precision = {v: k for k, v in _lib.PRECISIONS.items()}[p.value]
        _lib.check(L.bsdfd_get_tile(h, 0, C.byref(p)))
        self.tile = int(p.value)               # queries per wave tile of the sample / pdf kernels in effect (16 | 32)
        _lib.check(L.bsdfd_get_tile(h, 2, C.byref(p)))
        self.tile_samples_only = int(p.value)  # ... and of the kernel behind flow_samples_only

    def close(self):
        if getattr(self, "_h", None):
            self._L.bsdfd_destroy(self._h)
            self._h = None
            self._hi = 0  # the operator library rejects a null handle (TORCH_CHECK) instead of touching freed memory

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def _chk(self, t: Optional[torch.Tensor], cols: int, name: str, n: Optional[int] = None):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA (HIP) tensor")
        if t.device != self.device:
            raise RuntimeError(f"{name} is on {t.device}, the sampler on {self.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != cols:
            raise RuntimeError(f"{name} must have shape [N, {cols}], got {tuple(t.shape)}")
        if n is not None and t.shape[0] != n:
            raise RuntimeError(f"{name} has {t.shape[0]} rows, expected {n}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
        return t

    def _dev_chk(self, t, name: str):
        """torch binding: dtype / shape / contiguity are checked in C++ (csrc/torch_ops.cpp); the one thing the
        operator cannot know is which device the HANDLE lives on."""
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise RuntimeError(f"{name} must be a tensor on {self.device} (the sampler's device)")

    def _chk1(self, t: torch.Tensor, n: int, name: str):
        """A caller-supplied 1-D output (pdf [N]): the kernel writes N floats through its raw pointer."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.device:
            raise RuntimeError(f"{name} must be a CUDA (HIP) tensor on {self.device}")
        if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous float32 tensor of shape [{n}], got {t.dtype} {tuple(t.shape)}")
        return t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- per-query context (bsdfd_context_bytes / bsdfd_plugin_{sample,pdf}_ctx) ----
    def context_floats(self, n: int, n_segments: int = 1) -> int:
        """Size (in float32 elements) of the opaque per-query context of an n-query call."""
        if not getattr(self, "_h", None):
            raise RuntimeError("bsdfd: null handle")
        b = int(self._L.bsdfd_context_bytes(self._h, n, n_segments))
        if b < 0:
            raise RuntimeError("bsdfd_context_bytes: bad arguments")
        return b // 4

    def new_context(self, n: int, n_segments: int = 1) -> torch.Tensor:
        """Device buffer a ``plugin_sample(..., ctx_out=)`` call fills and ``plugin_pdf(..., ctx_in=)`` reads."""
        return torch.empty((self.context_floats(n, n_segments),), dtype=torch.float32, device=self.device)

    def _chk_ctx(self, ctx: torch.Tensor, n: int, n_segments: int = 1) -> torch.Tensor:
        need = self.context_floats(n, n_segments)
        if (not isinstance(ctx, torch.Tensor) or ctx.device != self.device or ctx.dtype != torch.float32 or ctx.dim() != 1
                or not ctx.is_contiguous() or ctx.numel() < need or ctx.data_ptr() % 16):
            raise RuntimeError(f"context must be a contiguous, 16-byte aligned float32 tensor of >= {need} elements on "
                               f"{self.device} (FlowSampler.new_context)")
        return ctx

    def flops_per_query(self, T: int) -> int:
        return int(self._L.bsdfd_flops_per_query(self._h, T))

    def set_profiling(self, on: bool):
        _lib.check(self._L.bsdfd_set_profiling(self._h, 1 if on else 0))

    def profile_read(self):
        """(launches, total kernel ms) since ``set_profiling(True)`` — HIP events on the launch stream."""
        n, ms = C.c_int64(), C.c_double()
        _lib.check(self._L.bsdfd_profile_read(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_read_op(self, op: str):
        """(launches, total kernel ms) of ONE kind of launch since ``set_profiling(True)``: ``op`` is "sample", "pdf",
        "samples_only" or "sample_pdf" (bsdfd_profile_read_op); "sample_resident" / "pdf_resident": those of the sample / pdf
        launches that ran the register-resident fast-path kernel."""
        n, ms = C.c_int64(), C.c_double()
        code = {"sample": 0, "pdf": 1, "samples_only": 2, "sample_pdf": 3, "sample_resident": 4, "pdf_resident": 5}[op]
        _lib.check(self._L.bsdfd_profile_read_op(self._h, code, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_clock_mhz(self) -> float:
        """Shader clock (MHz) the chip sustained under THIS handle's launches since ``set_profiling(True)``: the waves' own
        shader-cycle / wall-clock counters (bsdfd_profile_clock_mhz); 0 if none were recorded."""
        mhz = C.c_double()
        _lib.check(self._L.bsdfd_profile_clock_mhz(self._h, C.byref(mhz)))
        return mhz.value

    def last_kernel_ms(self) -> float:
        return float(self._L.bsdfd_last_kernel_ms(self._h))

    # ---- operator level (rendering/utils/mlp_brdf_sampling.py) -------
    def network_sampling(self, omega_i, x0=None, T: int = 4, seed: int = 0, offset: int = 0
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._ops is not None:
            self._dev_chk(omega_i, "omega_i")
            return self._ops.network_sampling(self._hi, omega_i, x0, _i64(seed), _i64(offset), T)
        omega_i = self._chk(omega_i, 2, "omega_i")
        n = omega_i.shape[0]
        x0 = self._chk(x0, 2, "x0", n)
        x = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        pdf = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.bsdfd_network_sampling(self._h, _ptr(omega_i), _ptr(x0), seed, offset, n, T,
                                                      _ptr(x), _ptr(pdf), self._stream()))
        return x, pdf

    def network_pdf(self, omega_o, omega_i, T: int = 4) -> torch.Tensor:
        if self._ops is not None:
            self._dev_chk(omega_i, "omega_i")
            return self._ops.network_pdf(self._hi, omega_o, omega_i, T)
        omega_i = self._chk(omega_i, 2, "omega_i")
        n = omega_i.shape[0]
        omega_o = self._chk(omega_o, 2, "omega_o", n)
        pdf = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.bsdfd_network_pdf(self._h, _ptr(omega_o), _ptr(omega_i), n, T, _ptr(pdf),
                                                 self._stream()))
        return pdf

    def flow_samples_only(self, omega_i, x0, T: int) -> torch.Tensor:
        if self._ops is not None:
            self._dev_chk(omega_i, "omega_i")
            return self._ops.flow_samples_only(self._hi, omega_i, x0, T)
        omega_i = self._chk(omega_i, 2, "omega_i")
        n = omega_i.shape[0]
        x0 = self._chk(x0, 2, "x0", n)
        x = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.bsdfd_flow_samples_only(self._h, _ptr(omega_i), _ptr(x0), n, T, _ptr(x),
                                                       self._stream()))
        return x

    # ---- plugin level (tensor core of MyBSDF.sample / MyBSDF.pdf) ----
    # Every plain entry point of the library is its *_ex twin with no option set (opts = NULL), so each operation has ONE ctypes
    # call site (*_ex) and one buffer-writing operator (*_ex_out); _prepare() is the one path from the arguments to either.
    def _chk_index(self, idx, n, name="rng_index"):
        if idx is None:
            return None
        if (not isinstance(idx, torch.Tensor) or idx.device != self.device or idx.dtype != torch.int64 or idx.dim() != 1
                or (n is not None and idx.shape[0] != n) or not idx.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous int64 tensor" + (f" of shape [{n}]" if n is not None else "") +
                               f" on {self.device}")
        return idx

    def _rows(self, row_index, m):
        """Rows a call processes: all m of the arrays, or the rows a row_index names."""
        if row_index is None:
            return m
        self._chk_index(row_index, None, "row_index")
        if row_index.shape[0] > m:
            raise RuntimeError(f"row_index names {row_index.shape[0]} rows, the arrays have {m}")
        if row_index.numel() and os.environ.get("BSDFD_CHECK_INDEX", "0") not in ("", "0"):
            # debugging aid (one device->host sync per call): the library cannot check this, it does not know the arrays' lengths
            lo, hi = int(row_index.min()), int(row_index.max())
            if lo < 0 or hi >= m:
                raise RuntimeError(f"row_index entries span [{lo}, {hi}], the arrays have rows [0, {m})")
            if int(torch.unique(row_index).numel()) != row_index.numel():
                raise RuntimeError("row_index names a row more than once")
        return row_index.shape[0]

    def _outputs(self, out, m, names, row_index=None, check=True):
        """The outputs of a call on m-row arrays, as a tuple laid out like ``names`` = (wo [m,3] or None, pdf [m], ...): fresh
        ones (zeros under a ``row_index``: the rows it does not name stay untouched; empty otherwise) or the caller's, checked."""
        if out is None:
            mk = torch.empty if row_index is None else torch.zeros
            return ((None if names[0] is None else mk((m, 3), dtype=torch.float32, device=self.device),) +
                    tuple(mk((m,), dtype=torch.float32, device=self.device) for _ in names[1:]))
        if check:
            if names[0] is not None:
                self._chk(out[0], 3, names[0], m)
            for t, name in zip(out[1:], names[1:]):
                self._chk1(t, m, name)
        return tuple(out)

    def _live_rows(self, active, wi, out, names, dir=None, flags=0):
        """``active`` mask -> (outputs with their dead rows zeroed, ascending rows of the live lanes).  The mask is compacted
        before the launch that would check ``wi``, so the row count and the outputs are settled here, for either binding.
        ``flags``: BSDFD_LIVE_* hemisphere tests on ``wi`` and on ``dir`` = (tensor, columns, name), applied on top of the mask."""
        from .live import live_rows
        if self._ops is not None:
            self._dev_chk(wi, "wi")
            if wi.dim() != 2:
                raise RuntimeError(f"wi must have shape [N, 3], got {tuple(wi.shape)}")
        else:
            self._chk(wi, 3, "wi")
        m = wi.shape[0]
        out = self._outputs(out, m, names)
        if flags:   # the hemisphere tests read the direction arrays themselves
            wi, dir = self._chk(wi, 3, "wi"), self._chk(*dir, m)
        if (not isinstance(active, torch.Tensor) or active.device != self.device or active.dtype not in (torch.bool, torch.uint8)
                or active.dim() != 1 or active.shape[0] != m):
            raise RuntimeError(f"active must be a bool / uint8 tensor of shape [{m}] on {self.device}")
        return out, live_rows(active, wi if flags else None, dir if flags else None, flags, zero=(out + (None,))[:3])

    def _prepare(self, wi, ins, out, names, ctx_out=None, ctx_in=None, rng_index=None, row_index=None, active=None, cull=0):
        """Arguments of a plugin-level call -> (n, out, opts, row_index): the rows the launch processes (None: a mask without a
        live lane — ``out`` is the result, nothing is launched), the outputs (None: torch binding, no buffers and no option —
        the allocating operator serves the call), the ``bsdfd_opts*`` of the ctypes call (None when no option is set) and the
        ``row_index`` in effect.  ``ins``: the inputs besides ``wi`` as (tensor, columns, name); ``names``: see _outputs;
        ``cull``: BSDFD_LIVE_* hemisphere tests on wi / ins[0] that a masked call applies on top of the mask."""
        if active is not None:
            if row_index is not None or rng_index is not None or ctx_in is not None or ctx_out is not None:
                raise ValueError("active= cannot be combined with row_index, rng_index or a per-query context: those are indexed "
                                 "by the call's own rows (compact the mask with live.live_rows and pass row_index instead)")
            out, rows = self._live_rows(active, wi, out, names, ins[0], cull)
            if rows.shape[0] == 0:
                return None, out, None, None
            if rows.shape[0] < wi.shape[0]:   # (every lane live: the ordinary call)
                row_index = rows
        if ctx_out is not None and ctx_in is not None:
            raise RuntimeError("a call either writes a per-query context (ctx_out) or reads one (ctx_in), not both")
        ctx = ctx_out if ctx_in is None else ctx_in
        plain = ctx is None and rng_index is None and row_index is None
        if self._ops is not None:   # dtype / shape / contiguity of the arrays: checked by the operator
            self._dev_chk(wi, "wi")
            if plain:
                return 0, out, None, None
            m = wi.shape[0]
        else:
            m = self._chk(wi, 3, "wi").shape[0]
        n = self._rows(row_index, m)
        if self._ops is None:
            for t, cols, name in ins:
                self._chk(t, cols, name, m)
        if ctx is not None:
            self._chk_ctx(ctx, n)
        if rng_index is not None:
            self._chk_index(rng_index, n)
        out = self._outputs(out, m, names, row_index, check=self._ops is None)
        if plain or self._ops is not None:
            return n, out, None, row_index
        return n, out, C.byref(_lib.opts(ctx_out=ctx_out, ctx_in=ctx_in, rng_index=rng_index, row_index=row_index)), row_index

    def plugin_sample(self, wi, x0=None, T: int = 4, variant: int = _lib.PLUGIN_MEASURED, seed: int = 0,
                      offset: int = 0, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      ctx_out: Optional[torch.Tensor] = None, rng_index: Optional[torch.Tensor] = None,
                      ctx_in: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None,
                      active: Optional[torch.Tensor] = None):
        """``ctx_out`` (``new_context(N)``): also write the per-query context a later ``plugin_pdf(wi, ., ctx_in=)`` /
        ``plugin_sample(wi, ctx_in=)`` for the SAME ``wi`` reads instead of recomputing the prologue (identical results);
        ``ctx_in``: read the context an earlier call (``plugin_pdf(..., ctx_out=)`` or ``plugin_sample(..., ctx_out=)``) wrote
        for this very ``wi``.  At most one of the two.
        ``rng_index`` (int64 [N]): the Philox counter of row i is ``offset + rng_index[i]`` instead of ``offset + i``
        (a bucketed wavefront passes the rows' original lane indices: draws independent of the bucketing).
        ``row_index`` (int64 [n], n <= N, distinct entries < N): the call processes n rows; row i reads ``wi`` / ``x0`` at row
        ``row_index[i]`` and writes ``wo`` / ``pdf`` there (bsdfd_opts.row_index: the gather / scatter of a bucketed wavefront
        inside the kernel's own loads and stores); rows it does not name are left as they are (zeros when ``out`` is None).
        Its Philox counter is ``offset + row_index[i]`` unless ``rng_index`` is given.
        ``active`` (bool / uint8 [N]): the ``active`` mask of the plugin protocol (rendering/brdf_measured_disk.py:59) — the flow
        runs on the lanes it selects only (``live.live_rows``, then the ``row_index`` path: the live rows get exactly the bits
        of the unmasked call), the dead rows of ``wo`` / ``pdf`` are 0, also in ``out=`` buffers.  One read-back of the live
        count per call.  Not together with ``row_index``, ``rng_index`` or a context (those are indexed by the call's own rows:
        whoever wants both passes ``row_index`` themselves)."""
        n, out, o, row_index = self._prepare(wi, ((x0, 2, "x0"),), out, ("out wo", "out pdf"), ctx_out, ctx_in, rng_index,
                                             row_index, active)
        if n is None:
            return out
        if self._ops is None:
            with torch.cuda.device(self.device):
                _lib.check(self._L.bsdfd_plugin_sample_ex(self._h, variant, _ptr(wi), _ptr(x0), seed, offset, n, T,
                                                          _ptr(out[0]), _ptr(out[1]), o, self._stream()))
        elif out is None:
            return self._ops.plugin_sample(self._hi, variant, wi, x0, _i64(seed), _i64(offset), T)
        else:
            self._ops.plugin_sample_ex_out(self._hi, variant, wi, x0, _i64(seed), _i64(offset), T, out[0], out[1],
                                           ctx_out if ctx_in is None else ctx_in, rng_index, ctx_in is not None, row_index)
        return out

    def plugin_sample_pdf(self, wi, wl, x0=None, T: int = 4, variant: int = _lib.PLUGIN_MEASURED, seed: int = 0,
                          offset: int = 0, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                          rng_index: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None,
                          active: Optional[torch.Tensor] = None):
        """sample(wi) and pdf(wi, wl) of the same intersections in ONE launch (the per-query prologue is
        shared): -> (wo [N,3], pdf(wo) [N], pdf(wl) [N]), identical to plugin_sample + plugin_pdf(wi, wl).
        ``rng_index`` / ``row_index`` / ``active``: as in ``plugin_sample`` (the fused call takes no
        per-query context).  A masked call culls by the mask alone: ``wo`` / ``pdf(wo)`` are defined below the horizon too."""
        n, out, o, row_index = self._prepare(wi, ((wl, 3, "wl"), (x0, 2, "x0")), out, ("out wo", "out pdf(wo)", "out pdf(wl)"),
                                             rng_index=rng_index, row_index=row_index, active=active)
        if n is None:
            return out
        if self._ops is None:
            with torch.cuda.device(self.device):
                _lib.check(self._L.bsdfd_plugin_sample_pdf_ex(self._h, variant, _ptr(wi), _ptr(x0), _ptr(wl), seed, offset, n, T,
                                                              _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), o, self._stream()))
        elif out is None:
            return self._ops.plugin_sample_pdf(self._hi, variant, wi, wl, x0, _i64(seed), _i64(offset), T)
        else:
            self._ops.plugin_sample_pdf_ex_out(self._hi, variant, wi, wl, x0, _i64(seed), _i64(offset), T, out[0], out[1], out[2],
                                               rng_index, row_index)
        return out

    def plugin_pdf(self, wi, wo, T: int = 4, variant: int = _lib.PLUGIN_MEASURED,
                   out: Optional[torch.Tensor] = None, ctx_in: Optional[torch.Tensor] = None,
                   ctx_out: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None,
                   active: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``ctx_in``: the context an earlier ``plugin_sample`` / ``plugin_pdf`` call wrote (``ctx_out=``) for this very ``wi``
        array; ``ctx_out`` (``new_context(N)``): write it here (the call order of Mitsuba's path integrator: eval_pdf() for the
        emitter sample first, sample() second — rendering/brdf_measured_disk.py:126,59).  At most one of the two.
        ``row_index``: as in ``plugin_sample`` (row i reads wi / wo at row ``row_index[i]`` and writes pdf there).
        ``active``: as in ``plugin_sample`` (rendering/brdf_measured_disk.py:112).  For ``PLUGIN_MEASURED`` the lanes with
        ``wi.z <= 0`` or ``wo.z <= 0`` are culled as well: their pdf is exactly 0 in the unmasked call too."""
        n, out, o, row_index = self._prepare(wi, ((wo, 3, "wo"),), None if out is None else (None, out), (None, "out pdf"),
                                             ctx_out, ctx_in, row_index=row_index, active=active,
                                             cull=_lib.LIVE_WI_UPPER | _lib.LIVE_DIR_UPPER if variant == _lib.PLUGIN_MEASURED else 0)
        if n is None:
            return out[1]
        if self._ops is None:
            with torch.cuda.device(self.device):
                _lib.check(self._L.bsdfd_plugin_pdf_ex(self._h, variant, _ptr(wi), _ptr(wo), n, T, _ptr(out[1]), o,
                                                       self._stream()))
        elif out is None:
            return self._ops.plugin_pdf(self._hi, variant, wi, wo, T)
        else:
            self._ops.plugin_pdf_ex_out(self._hi, variant, wi, wo, T, out[1], ctx_in if ctx_out is None else ctx_out,
                                        ctx_out is not None, row_index)
        return out[1]
