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
from .ground_truth import GroundTruth, RowKernels


def find_measured_file(material: str, directory: Optional[str] = None) -> Optional[str]:
    """``<dir>/<material>.bsdf`` in: the argument, $BSDFD_MEASURED_DIR, ./measuredbsdfs (the reference's
    CWD-relative convention, brdf_measured_disk.py:39) — first hit, else None."""
    for d in (directory, os.environ.get("BSDFD_MEASURED_DIR"), "measuredbsdfs"):
        if d:
            p = os.path.join(d, material + ".bsdf")
            if os.path.exists(p):
                return p
    return None


class MeasuredBSDF(GroundTruth):
    """One RGL material.  ``eval_t`` is zero on the lower hemispheres.  ``sample_weight`` is the tail of the measured plugins'
    sample() (brdf_measured_disk.py:89-101): the firefly rule reads lum(value), and weight = 0 also on lanes that leave through
    the lower hemisphere.  ``sample_t`` is the file's own importance sampler (Dupuy & Jakob: luminance warp, VNDF warp, reflection
    about the half vector) at ``u`` in [0,1)^2: lanes with wi.z <= 0 get zeros, pdf = weight = 0 where wo leaves through the lower
    hemisphere (wo is still written); ``pdf_t`` is 0 on the lower hemispheres."""

    NAME = "MeasuredBSDF"
    ENTRY = dict(eval="bsdfd_measured_eval", sample_weight="bsdfd_measured_sample_weight", sample="bsdfd_measured_sample",
                 pdf="bsdfd_measured_pdf")
    COERCE_ACTIVE = True        # the plugins and the Mitsuba adapter hand sample_weight masks of any dtype, wherever they live

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

    def _lead(self):
        return self._h

class MeasuredTable(RowKernels):
    """``eval()`` for a mixed-material wavefront: ``entries[m]`` (a ``MeasuredBSDF``, or None = no ground truth) serves the lanes
    whose ``material_id`` is m.  One launch for the whole wavefront in LANE order (``bsdfd_measured_eval_table``), where
    ``MeasuredBSDF.eval_t`` takes one launch per material on gathered slices; lanes with ground truth get that evaluator's
    result bit for bit, every other lane (None entry, id negative or >= len(entries): a renderer's floor hits and misses) NaN.
    The table keeps the entries alive: it borrows their tensor data.  The native table is created here, on the entries' device
    (the launches then neither allocate nor synchronise); only a table without any ground truth, which the library refuses,
    is left to fail at its first launch."""

    NAME = "MeasuredTable"
    ENTRY = dict(eval="bsdfd_measured_eval_table", sample_weight="bsdfd_measured_sample_weight_table",
                 sample="bsdfd_measured_sample_table", pdf="bsdfd_measured_pdf_table")
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

    _lead = _table

    def eval_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, wl: Optional[torch.Tensor] = None,
               tint=None, out_o: Optional[torch.Tensor] = None, out_l: Optional[torch.Tensor] = None,
               rows: Optional[torch.Tensor] = None):
        """f(wi, wo) cos(theta_o) [* tint] of each lane's material -> f_o [N,3]; with ``wl`` also f(wi, wl) cos(theta_l) ->
        (f_o, f_l), both evaluations in the same launch.  NaN rows = no ground truth for that lane.  ``rows`` (int64 [n_rows]):
        only the listed rows are evaluated and written (``bsdfd_measured_eval_table_rows``); every other row keeps what it held."""
        return self._eval_table(material_id, wi, wo, wl, tint, out_o, out_l, rows)

    def sample_weight(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, *, tint=None,
                      firefly_threshold: Optional[float] = None, active: Optional[torch.Tensor] = None):
        """``MeasuredBSDF.sample_weight`` of each lane's material in one launch -> (weight [N,3], pdf [N]); lanes without
        ground truth get weight NaN and pdf = pdf_sa.  A mask on another device is refused, not copied across."""
        return self._sample_weight(material_id, wi, wo, pdf_sa, tint, firefly_threshold, active)

    def sample_t(self, material_id: torch.Tensor, wi: torch.Tensor, u: torch.Tensor, tint=None,
                 active: Optional[torch.Tensor] = None, out=None):
        """``MeasuredBSDF.sample_t`` of each lane's material in one launch -> (wo [N,3], pdf [N], weight [N,3]); lanes without
        ground truth get NaN in all three."""
        return self._sample_t(material_id, wi, u, tint, active, out)

    def pdf_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``MeasuredBSDF.pdf_t`` of each lane's material in one launch -> [N]; NaN = no ground truth for that lane."""
        return self._pdf_t(material_id, wi, wo, active, out)
