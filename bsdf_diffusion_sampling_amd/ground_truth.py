"""The host layer the native ground-truth evaluators share: ``measured.MeasuredBSDF``, ``measured.MeasuredTable``,
``analytic.RoughDielectric``, ``analytic.Principled`` and ``analytic.AnalyticTable``.

In ``libbsdfd.so`` each is four kernels over rows (eval, the tail of the plugins' sample(), sample, pdf) behind entry points of one
shape.  That shape is written once here; a class says which entry points are its own, what their leading argument is, how many
variates its sampler takes and where its firefly rule cuts.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib


def launch(name: str, device, *args):
    """One launch of the library's ``name`` on ``device``'s current stream, with that device current: tensors go as their data
    pointers, None as NULL, everything else as it is; the stream is the last argument."""
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args],
                                             stream))


def check(who: str, tensors, material_id: Optional[torch.Tensor] = None, active=None, coerce_active: bool = False):
    """The checks of every tensor call, ``who`` in the messages, over ``tensors`` = (name, tensor, columns; 0 = [N]) each: dtype and
    shape, then the row counts against the tensor that fixes N (``material_id`` int64 [N], else the first), then ``active``, then
    device and layout.  -> ``active`` as a contiguous uint8 [N] (None = every lane); ``coerce_active`` copies any mask across."""
    n, n_name = None, tensors[0][0]
    if material_id is not None:
        if material_id.dtype != torch.int64 or material_id.dim() != 1:
            raise ValueError(f"{who}: material_id must be an int64 tensor [N]")
        n, n_name = material_id.shape[0], "material_id"
    for name, t, cols in tensors:
        if t.dtype != torch.float32 or ((t.dim() != 2 or t.shape[1] != cols) if cols else t.dim() != 1):
            raise ValueError(f"{who}: {name} must be an fp32 tensor [N{',' + str(cols) if cols else ''}]")
        if n is None:
            n = t.shape[0]
        elif t.shape[0] != n:
            raise ValueError(f"{who}: {name} has {t.shape[0]} rows, {n_name} has {n}")
    device = tensors[0][1].device if material_id is None else material_id.device
    if active is not None:
        if coerce_active:
            active = active.to(device=device, dtype=torch.uint8)
        if not (isinstance(active, torch.Tensor) and active.shape == (n,) and active.device == device
                and active.dtype in (torch.bool, torch.uint8)):
            raise ValueError(f"{who}: active must be a bool or uint8 tensor [N] on the device of wi")
        active = active.to(torch.uint8).contiguous()
    if material_id is not None and not (material_id.is_cuda and material_id.is_contiguous()):
        raise ValueError(f"{who}: material_id must be a contiguous CUDA tensor, all on one device")
    for name, t, _ in tensors:
        if not (t.is_cuda and t.is_contiguous() and t.device == device):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor, all on one device")
    return active


def tint3(tint):
    """``tint`` (None, or three numbers in anything that iterates) as the ``const float[3]`` of the entry points."""
    if tint is None:
        return None
    vals = [float(v) for v in (tint.tolist() if hasattr(tint, "tolist") else tint)]
    return (C.c_float * 3)(*vals)


def sample_out(wi: torch.Tensor, out, who: str):
    """(wo, pdf, weight) to write into: the caller's ``out`` triple (``check`` it), or fresh tensors."""
    if out is None:
        return torch.empty_like(wi), torch.empty(wi.shape[0], dtype=torch.float32, device=wi.device), torch.empty_like(wi)
    if len(out) != 3:
        raise ValueError(f"{who}: out is a (wo [N,3], pdf [N], weight [N,3]) triple")
    return tuple(out)


def mask_of(active, wi: torch.Tensor):
    """Mitsuba's ``active`` argument (True, a bool, a mask, a DrJit mask) as the ``active`` of the tensor calls."""
    if active is True or active is None:
        return None
    if isinstance(active, bool):
        return torch.zeros(wi.shape[0], dtype=torch.uint8, device=wi.device)
    if not isinstance(active, torch.Tensor):
        active = active.torch()
    return active.to(device=wi.device, dtype=torch.uint8).contiguous()


class RowKernels:
    """The tensor calls that have one shape with and without a ``material_id`` per lane, written over both."""

    NAME = "RowKernels"         # the class, in messages
    ENTRY: dict = {}            # call -> entry point of the library; ``_lead()`` is its leading argument
    U_COLS = 2                  # variates per lane of sample_t
    FIREFLY = 30.0              # sample_weight's default threshold
    COERCE_ACTIVE = False       # sample_weight copies any mask across devices and dtypes

    def _front(self, material_id):
        return (self._lead(),) if material_id is None else (self._lead(), material_id)

    def _sample_weight(self, material_id, wi, wo, pdf_sa, tint, firefly_threshold, active):
        act = check(self.NAME + ".sample_weight", (("wi", wi, 3), ("wo", wo, 3), ("pdf_sa", pdf_sa, 0)), material_id, active,
                    self.COERCE_ACTIVE)
        weight, pdf = torch.empty_like(wi), torch.empty_like(pdf_sa)
        launch(self.ENTRY["sample_weight"], wi.device, *self._front(material_id), wi, wo, pdf_sa, act, wi.shape[0], tint3(tint),
               float(self.FIREFLY if firefly_threshold is None else firefly_threshold), weight, pdf)
        return weight, pdf

    def _sample_t(self, material_id, wi, u, tint, active, out):
        who = self.NAME + ".sample_t"
        wo, pdf, weight = sample_out(wi, out, who)
        act = check(who, (("wi", wi, 3), ("u", u, self.U_COLS), ("wo", wo, 3), ("pdf", pdf, 0), ("weight", weight, 3)),
                    material_id, active)
        launch(self.ENTRY["sample"], wi.device, *self._front(material_id), wi, u, act, wi.shape[0], tint3(tint), wo, pdf, weight)
        return wo, pdf, weight

    def _eval_table(self, material_id, wi, wo, wl, tint, out_o, out_l, rows=None):
        """``eval_t`` of the two tables: f_o [N,3] or, with ``wl``, (f_o, f_l).  ``rows`` (int64 [n_rows], contiguous, on the
        device, at most N entries, distinct and in [0, N)): the ``_rows`` entry point — only the listed rows are evaluated and
        written, every other row of ``out_o`` / ``out_l`` keeps what it held."""
        who = self.NAME + ".eval_t"
        if out_l is not None and wl is None:
            raise ValueError(f"{who}: out_l without wl")
        given = (("wi", wi), ("wo", wo), ("wl", wl), ("out_o", out_o), ("out_l", out_l))
        check(who, [(k, t, 3) for k, t in given if t is not None], material_id)
        if rows is not None and not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.dim() == 1
                                     and rows.is_contiguous() and rows.device == wi.device and rows.shape[0] <= wi.shape[0]):
            raise ValueError(f"{who}: rows must be a contiguous int64 tensor [n_rows <= N] on the device of wi")
        if out_o is None:
            out_o = torch.empty_like(wi)
        if wl is not None and out_l is None:
            out_l = torch.empty_like(wi)
        args = (self._lead(), material_id, wi, wo, wl, wi.shape[0], tint3(tint), out_o, out_l)
        if rows is None:
            launch(self.ENTRY["eval"], wi.device, *args)
        else:
            launch(self.ENTRY["eval"] + "_rows", wi.device, *args, rows, rows.shape[0])
        return out_o if wl is None else (out_o, out_l)

    def _pdf_t(self, material_id, wi, wo, active, out):
        if out is None:
            out = torch.empty(wi.shape[0], dtype=torch.float32, device=wi.device)
        act = check(self.NAME + ".pdf_t", (("wi", wi, 3), ("wo", wo, 3), ("out", out, 0)), material_id, active)
        launch(self.ENTRY["pdf"], wi.device, *self._front(material_id), wi, wo, act, wi.shape[0], out)
        return out


class GroundTruth(RowKernels):
    """An evaluator of ONE material: the tensor calls, and over them the call shapes of ``mi.BSDF`` as the reference's plugins use
    them (rendering/brdf_measured_disk.py:59,96,107,112)."""

    def eval_t(self, wi: torch.Tensor, wo: torch.Tensor, out: Optional[torch.Tensor] = None, tint=None) -> torch.Tensor:
        """f(wi, wo) cos(theta_o) [* tint] -> [N,3] (which lanes are zero: the class)."""
        if out is None:
            out = torch.empty_like(wi)
        check(self.NAME + ".eval_t", (("wi", wi, 3), ("wo", wo, 3), ("out", out, 3)))
        launch(self.ENTRY["eval"], wi.device, self._lead(), wi, wo, wi.shape[0], tint3(tint), out)
        return out

    def sample_weight(self, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, *, tint=None,
                      firefly_threshold: Optional[float] = None, active: Optional[torch.Tensor] = None):
        """The tail of a plugin's sample() in one launch -> (weight [N,3], pdf [N]): value = f * tint / pdf_sa, pdf := 0 where value
        reaches ``firefly_threshold`` (None = the class's ``FIREFLY``), weight = value where pdf > 0; zeros where ``active`` is false."""
        return self._sample_weight(None, wi, wo, pdf_sa, tint, firefly_threshold, active)

    def sample_t(self, wi: torch.Tensor, u: torch.Tensor, tint=None, active: Optional[torch.Tensor] = None, out=None):
        """The model's own importance sampler at the variates ``u`` [N,U_COLS] in [0,1) -> (wo [N,3], pdf [N], weight [N,3]),
        weight = f cos [* tint] / pdf; zeros on lanes with ``active`` false.  ``out`` = (wo, pdf, weight) buffers to write into."""
        return self._sample_t(None, wi, u, tint, active, out)

    def pdf_t(self, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Solid-angle density with which ``sample_t(wi, .)`` returns ``wo`` -> [N]; 0 on lanes with ``active`` false."""
        return self._pdf_t(None, wi, wo, active, out)

    # ---- the call shapes of ``mi.BSDF`` -------------------------------------------------------------------------------------
    def _variates(self, sample1, sample2) -> torch.Tensor:
        """``u`` of ``sample_t`` from Mitsuba's two samples: ``sample1`` is ignored (one lobe)."""
        from .plugin_base import _vec
        return _vec(sample2)

    def _bsdf_sample(self, wi, wo, pdf):
        from .plugin_base import BSDFSample3f
        return BSDFSample3f(wo=wo, pdf=pdf)

    def eval(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        return self.eval_t(_wi_of(si), _vec(wo))

    def sample(self, ctx, si, sample1, sample2, active=True):
        """``mi.BSDF.sample``: -> (BSDFSample3f, weight [N,3])."""
        from .plugin_base import _wi_of
        wi = _wi_of(si)
        wo, pdf, weight = self.sample_t(wi, self._variates(sample1, sample2), active=mask_of(active, wi))
        return self._bsdf_sample(wi, wo, pdf), weight

    def pdf(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        wi = _wi_of(si)
        return self.pdf_t(wi, _vec(wo), active=mask_of(active, wi))

    def eval_pdf(self, ctx, si, wo, active=True):
        return self.eval(ctx, si, wo, active), self.pdf(ctx, si, wo, active)
