"""Ground-truth evaluator for the plugins' ``eval()``, and the measured BSDF's own sampler: the RGL model on the GPU.

The reference builds Mitsuba's ``measured`` BSDF (``mi.load_dict({'type': 'measured', 'filename':
'measuredbsdfs/<name>.bsdf'})``, rendering/brdf_measured_disk.py:36-42) and calls its ``eval`` for the
sample weight and the firefly rule.  Mitsuba has no AMD GPU variant; ``MeasuredBSDF`` is the same
model (Dupuy & Jakob 2018) over ``libbsdfd.so`` (csrc/measured.hip) with the call shape the plugins
use: ``eval(ctx, si, wo) -> [N,3]`` = f * cos(theta_o), zero on the lower hemispheres.  Only the
``*_rgb.bsdf`` flavour is supported (the one the reference's scenes name).  No CPU fallback.
``sample`` / ``pdf`` / ``eval_pdf`` (``sample_t`` / ``pdf_t`` on tensors) are the importance sampler that ships inside every
tensor file — the baseline the neural samplers compete with, and the way to sample a material that has no trained nets.  Like
``eval`` it restates the published model and is parity-unpinned against Mitsuba.

``MeasuredTable`` serves a wavefront whose lanes carry DIFFERENT materials (one id per lane) in one launch
(csrc/measured_table.hip): the same numbers as ``MeasuredBSDF`` per material, bit for bit.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import _lib


def find_measured_file(material: str, directory: Optional[str] = None) -> Optional[str]:
    """``<dir>/<material>.bsdf`` in: the argument, $BSDFD_MEASURED_DIR, ./measuredbsdfs (the reference's
    CWD-relative convention, brdf_measured_disk.py:39) — first hit, else None."""
    for d in (directory, os.environ.get("BSDFD_MEASURED_DIR"), "measuredbsdfs"):
        if d:
            p = os.path.join(d, material + ".bsdf")
            if os.path.exists(p):
                return p
    return None


def _launch(name: str, device, *args):
    """One launch of the library's ``name`` on ``device``'s current stream, with that device current: tensors go as their data
    pointers, None as NULL, everything else as it is; the stream is the last argument."""
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args],
                                             stream))


class MeasuredBSDF:
    def __init__(self, path: str):
        self.path = path
        self._h = C.c_void_p()
        _lib.check(_lib.lib().bsdfd_measured_create_from_file(path.encode(), C.byref(self._h)))
        info = [C.c_int32() for _ in range(5)]
        _lib.check(_lib.lib().bsdfd_measured_get_info(self._h, *[C.byref(i) for i in info]))
        self.n_phi, self.n_theta, iso, jac, self.reduction = (i.value for i in info)
        self.isotropic, self.jacobian = bool(iso), bool(jac)
        lum = C.c_int32()
        _lib.check(_lib.lib().bsdfd_measured_has_luminance(self._h, C.byref(lum)))
        self.has_luminance = bool(lum.value)   # the file carries the sampler's luminance warp (without it that pdf is 1)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.lib().bsdfd_measured_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def _check(**tensors):
        ref = None
        for name, (t, cols) in tensors.items():
            shape_ok = (t.dim() == 2 and t.shape[1] == cols) if cols else t.dim() == 1
            if not (t.is_cuda and t.dtype == torch.float32 and shape_ok and t.is_contiguous()):
                raise ValueError(f"MeasuredBSDF: {name} must be a contiguous fp32 CUDA tensor "
                                 f"[N{',' + str(cols) if cols else ''}]")
            if ref is not None and t.shape[0] != ref:
                raise ValueError(f"MeasuredBSDF: {name} has {t.shape[0]} rows, expected {ref}")
            ref = t.shape[0]

    @staticmethod
    def _tint(tint):
        if tint is None:
            return None
        vals = [float(v) for v in (tint.tolist() if hasattr(tint, "tolist") else tint)]
        return (C.c_float * 3)(*vals)

    def eval_t(self, wi: torch.Tensor, wo: torch.Tensor, out: Optional[torch.Tensor] = None, tint=None) -> torch.Tensor:
        """f(wi, wo) cos(theta_o) [* tint] -> [N,3]; zero on the lower hemispheres."""
        self._check(wi=(wi, 3), wo=(wo, 3))
        if out is None:
            out = torch.empty_like(wi)
        _launch("bsdfd_measured_eval", wi.device, self._h, wi, wo, wi.shape[0], self._tint(tint), out)
        return out

    def sample_weight(self, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, tint=None,
                      firefly_threshold: float = 30.0, active: Optional[torch.Tensor] = None):
        """The tail of the plugins' sample() in one launch (brdf_measured_disk.py:89-101): -> (weight [N,3],
        pdf [N]) with value = f * tint / pdf_sa, the firefly rule pdf := 0 where lum(value) >= threshold,
        and weight = 0 on lanes that are inactive, have pdf 0 or leave through the lower hemisphere."""
        self._check(wi=(wi, 3), wo=(wo, 3), pdf_sa=(pdf_sa, 0))
        act = None
        if active is not None:
            act = active.to(device=wi.device, dtype=torch.uint8).contiguous()
            if act.shape != (wi.shape[0],):
                raise ValueError("MeasuredBSDF.sample_weight: active must be [N]")
        weight, pdf = torch.empty_like(wi), torch.empty_like(pdf_sa)
        _launch("bsdfd_measured_sample_weight", wi.device, self._h, wi, wo, pdf_sa, act, wi.shape[0], self._tint(tint),
                float(firefly_threshold), weight, pdf)
        return weight, pdf

    @staticmethod
    def _active(active, n: int, device, who: str):
        """``active`` as a contiguous uint8 [N] on ``device`` (None = every lane)."""
        if active is None:
            return None
        if not (isinstance(active, torch.Tensor) and active.shape == (n,) and active.device == device
                and active.dtype in (torch.bool, torch.uint8)):
            raise ValueError(f"{who}: active must be a bool or uint8 tensor [N] on the device of wi")
        return active.to(torch.uint8).contiguous()

    @staticmethod
    def _sample_out(wi, out, who: str):
        """(wo, pdf, weight) to write into: the caller's ``out`` triple, checked, or fresh tensors."""
        if out is None:
            return torch.empty_like(wi), torch.empty(wi.shape[0], dtype=torch.float32, device=wi.device), torch.empty_like(wi)
        if len(out) != 3:
            raise ValueError(f"{who}: out is a (wo [N,3], pdf [N], weight [N,3]) triple")
        return tuple(out)

    def sample_t(self, wi: torch.Tensor, u: torch.Tensor, tint=None, active: Optional[torch.Tensor] = None, out=None):
        """The file's own importance sampler (Dupuy & Jakob: luminance warp, VNDF warp, reflection about the half vector) at the
        variates ``u`` [N,2] in [0,1)^2 -> (wo [N,3], pdf [N], weight [N,3]), weight = f cos [* tint] / pdf.  Lanes with
        wi.z <= 0 or ``active`` false get zeros; pdf = weight = 0 where wo leaves through the lower hemisphere (wo is still
        written).  ``out`` = (wo, pdf, weight) buffers to write into."""
        wo, pdf, weight = self._sample_out(wi, out, "MeasuredBSDF.sample_t")
        self._check(wi=(wi, 3), u=(u, 2), wo=(wo, 3), pdf=(pdf, 0), weight=(weight, 3))
        act = self._active(active, wi.shape[0], wi.device, "MeasuredBSDF.sample_t")
        _launch("bsdfd_measured_sample", wi.device, self._h, wi, u, act, wi.shape[0], self._tint(tint), wo, pdf, weight)
        return wo, pdf, weight

    def pdf_t(self, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Solid-angle density with which ``sample_t(wi, .)`` returns ``wo`` -> [N]; 0 on the lower hemispheres and on lanes
        with ``active`` false."""
        if out is None:
            out = torch.empty(wi.shape[0], dtype=torch.float32, device=wi.device)
        self._check(wi=(wi, 3), wo=(wo, 3), out=(out, 0))
        act = self._active(active, wi.shape[0], wi.device, "MeasuredBSDF.pdf_t")
        _launch("bsdfd_measured_pdf", wi.device, self._h, wi, wo, act, wi.shape[0], out)
        return out

    # the call shapes of ``mi.BSDF`` as the reference's plugins use them (brdf_measured_disk.py:59,96,107,112)
    def eval(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        return self.eval_t(_wi_of(si), _vec(wo))

    @staticmethod
    def _mask_of(active, wi):
        """Mitsuba's ``active`` argument (True, a bool, or a mask) as the ``active`` of the tensor calls."""
        if active is True or active is None:
            return None
        if isinstance(active, bool):
            return torch.zeros(wi.shape[0], dtype=torch.uint8, device=wi.device)
        if not isinstance(active, torch.Tensor):
            active = active.torch()
        return active.to(device=wi.device, dtype=torch.uint8).contiguous()

    def sample(self, ctx, si, sample1, sample2, active=True):
        """``mi.BSDF.sample``: -> (BSDFSample3f(wo, pdf), weight [N,3]).  ``sample1`` is ignored (one lobe)."""
        from .plugin_base import BSDFSample3f, _vec, _wi_of
        wi = _wi_of(si)
        wo, pdf, weight = self.sample_t(wi, _vec(sample2), active=self._mask_of(active, wi))
        return BSDFSample3f(wo=wo, pdf=pdf), weight

    def pdf(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        wi = _wi_of(si)
        return self.pdf_t(wi, _vec(wo), active=self._mask_of(active, wi))

    def eval_pdf(self, ctx, si, wo, active=True):
        return self.eval(ctx, si, wo, active), self.pdf(ctx, si, wo, active)


class MeasuredTable:
    """``eval()`` for a mixed-material wavefront: ``entries[m]`` (a ``MeasuredBSDF``, or None = no ground truth) serves the lanes
    whose ``material_id`` is m.  One launch for the whole wavefront in LANE order (``bsdfd_measured_eval_table``), where
    ``MeasuredBSDF.eval_t`` takes one launch per material on gathered slices; lanes with ground truth get that evaluator's
    result bit for bit, every other lane (None entry, id negative or >= len(entries): a renderer's floor hits and misses) NaN.
    The table keeps the entries alive: it borrows their tensor data.  The native table is created here, on the entries' device
    (the launches then neither allocate nor synchronise); only a table without any ground truth, which the library refuses,
    is left to fail at its first launch."""

    MAX_MATERIALS = 65536

    def __init__(self, entries: Sequence[Optional[MeasuredBSDF]]):
        self.entries = list(entries)
        if not 1 <= len(self.entries) <= self.MAX_MATERIALS:
            raise ValueError(f"MeasuredTable: 1..{self.MAX_MATERIALS} entries")
        if any(e is not None and not isinstance(e, MeasuredBSDF) for e in self.entries):
            raise ValueError("MeasuredTable: entries are MeasuredBSDF objects or None")
        self._t = C.c_void_p()
        if any(e is not None for e in self.entries):
            self._table()

    def __len__(self):
        return len(self.entries)

    def __del__(self):
        try:
            if getattr(self, "_t", None) is not None and self._t.value:
                _lib.lib().bsdfd_measured_table_destroy(self._t)
                self._t = C.c_void_p()
        except Exception:
            pass

    def _table(self):
        """The native table (created with the entries' device current — the library checks that it is)."""
        if not self._t.value:
            handles = (C.c_void_p * len(self.entries))(*[None if e is None else e._h.value for e in self.entries])
            _lib.check(_lib.lib().bsdfd_measured_table_create(handles, len(self.entries), C.byref(self._t)))
        return self._t

    @staticmethod
    def _check(material_id: torch.Tensor, **tensors):
        """``MeasuredBSDF._check`` plus the ids: dtype and shape, then the row counts, then device and layout."""
        if material_id.dtype != torch.int64 or material_id.dim() != 1:
            raise ValueError("MeasuredTable: material_id must be an int64 tensor [N]")
        n = material_id.shape[0]
        for name, (t, cols) in tensors.items():
            if t.dtype != torch.float32 or not ((t.dim() == 2 and t.shape[1] == cols) if cols else t.dim() == 1):
                raise ValueError(f"MeasuredTable: {name} must be an fp32 tensor [N{',' + str(cols) if cols else ''}]")
            if t.shape[0] != n:
                raise ValueError(f"MeasuredTable: {name} has {t.shape[0]} rows, material_id has {n}")
        for name, t in [("material_id", material_id)] + [(k, t) for k, (t, _) in tensors.items()]:
            if not (t.is_cuda and t.is_contiguous() and t.device == material_id.device):
                raise ValueError(f"MeasuredTable: {name} must be a contiguous CUDA tensor, all on one device")

    def eval_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, wl: Optional[torch.Tensor] = None,
               tint=None, out_o: Optional[torch.Tensor] = None, out_l: Optional[torch.Tensor] = None):
        """f(wi, wo) cos(theta_o) [* tint] of each lane's material -> f_o [N,3]; with ``wl`` also f(wi, wl) cos(theta_l) ->
        (f_o, f_l), both evaluations in the same launch.  NaN rows = no ground truth for that lane."""
        if out_l is not None and wl is None:
            raise ValueError("MeasuredTable.eval_t: out_l without wl")
        given = dict(wi=(wi, 3), wo=(wo, 3))
        given.update({k: (t, 3) for k, t in (("wl", wl), ("out_o", out_o), ("out_l", out_l)) if t is not None})
        self._check(material_id, **given)
        if out_o is None:
            out_o = torch.empty_like(wi)
        if wl is not None and out_l is None:
            out_l = torch.empty_like(wi)
        _launch("bsdfd_measured_eval_table", wi.device, self._table(), material_id, wi, wo, wl, wi.shape[0],
                MeasuredBSDF._tint(tint), out_o, out_l)
        return out_o if wl is None else (out_o, out_l)

    def sample_weight(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, tint=None,
                      active: Optional[torch.Tensor] = None, firefly_threshold: float = 30.0):
        """``MeasuredBSDF.sample_weight`` of each lane's material in one launch -> (weight [N,3], pdf [N]); lanes without
        ground truth get weight NaN and pdf = pdf_sa."""
        self._check(material_id, wi=(wi, 3), wo=(wo, 3), pdf_sa=(pdf_sa, 0))
        act = None
        if active is not None:
            if active.shape != (wi.shape[0],) or active.device != wi.device or active.dtype not in (torch.bool, torch.uint8):
                raise ValueError("MeasuredTable.sample_weight: active must be a bool or uint8 tensor [N] on the device of wi")
            act = active.to(torch.uint8).contiguous()
        weight, pdf = torch.empty_like(wi), torch.empty_like(pdf_sa)
        _launch("bsdfd_measured_sample_weight_table", wi.device, self._table(), material_id, wi, wo, pdf_sa, act, wi.shape[0],
                MeasuredBSDF._tint(tint), float(firefly_threshold), weight, pdf)
        return weight, pdf

    def sample_t(self, material_id: torch.Tensor, wi: torch.Tensor, u: torch.Tensor, tint=None,
                 active: Optional[torch.Tensor] = None, out=None):
        """``MeasuredBSDF.sample_t`` of each lane's material in one launch -> (wo [N,3], pdf [N], weight [N,3]); lanes without
        ground truth get NaN in all three."""
        wo, pdf, weight = MeasuredBSDF._sample_out(wi, out, "MeasuredTable.sample_t")
        self._check(material_id, wi=(wi, 3), u=(u, 2), wo=(wo, 3), pdf=(pdf, 0), weight=(weight, 3))
        act = MeasuredBSDF._active(active, wi.shape[0], wi.device, "MeasuredTable.sample_t")
        _launch("bsdfd_measured_sample_table", wi.device, self._table(), material_id, wi, u, act, wi.shape[0],
                MeasuredBSDF._tint(tint), wo, pdf, weight)
        return wo, pdf, weight

    def pdf_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``MeasuredBSDF.pdf_t`` of each lane's material in one launch -> [N]; NaN = no ground truth for that lane."""
        if out is None:
            out = torch.empty(material_id.shape[0], dtype=torch.float32, device=material_id.device)
        self._check(material_id, wi=(wi, 3), wo=(wo, 3), out=(out, 0))
        act = MeasuredBSDF._active(active, wi.shape[0], wi.device, "MeasuredTable.pdf_t")
        _launch("bsdfd_measured_pdf_table", wi.device, self._table(), material_id, wi, wo, act, wi.shape[0], out)
        return out
