"""Analytic ground truth of the full-sphere plugin: the rough dielectric on the GPU.

The reference's full-sphere plugin takes its ``eval()``, sample weight and firefly rule from an analytic Mitsuba BSDF out of a
list (rendering/utils/bsdf_dict.py; rendering/bsdf_myresult.py:97-110).  Entries 23..25 of that list are ``roughdielectric``
(Beckmann, alpha 0.2 / 0.3 / 0.5, bk7 in air); Mitsuba has no AMD GPU variant, so ``RoughDielectric`` is the same published
model (Walter et al. 2007; Mitsuba's defaults: visible-normal sampling, radiance transport) over ``libbsdfd.so``
(csrc/dielectric.hip, csrc/dielectric_dev.h): ``eval`` = f |cos theta_o| on both sides of the surface, its own importance
sampler (``sample`` / ``pdf``) and the fused tail of the plugin's ``sample()`` (``sample_weight``).  Restated from the
publication, PARITY-UNPINNED against Mitsuba, like ``measured.MeasuredBSDF``.  Entries 0..22 are ``principled`` BSDFs and have no
native counterpart.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .ground_truth import GroundTruth

# Mitsuba's named indices of refraction, as far as the reference's list uses them
IOR = {"bk7": 1.5046, "air": 1.000277, "vacuum": 1.0}
DISTRIBUTIONS = {"beckmann": 0}

# rendering/utils/bsdf_dict.py: the three roughdielectric entries (int_ior = bk7, ext_ior = air)
REFERENCE_ROUGHDIELECTRIC = {23: 0.2, 24: 0.3, 25: 0.5}
N_REFERENCE_MATERIALS = 26


def _ior(v) -> float:
    if isinstance(v, str):
        if v not in IOR:
            raise ValueError(f"RoughDielectric: unknown index of refraction {v!r} (known: {sorted(IOR)})")
        return IOR[v]
    return float(v)


class RoughDielectric(GroundTruth):
    """``eval_t`` = f |cos theta_o|, grey: reflection and (radiance-mode) transmission, either side.  ``sample_weight`` is the tail
    of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = 0 where pdf_sa <= 0, the firefly rule reads
    value.x, no cosine masks.  ``sample_t`` takes ``u`` [N,3] in [0,1)^3 (columns 0..1: Mitsuba's sample2, the visible normal;
    column 2: sample1, reflection iff u2 <= F); weight is 0 where the pdf is 0 or wo ends up on the wrong side for its lobe, and
    rows with wi.z == 0 get zeros.  ``sample`` fills eta and sampled_type per lobe; ``sample1`` [N] picks the lobe."""

    NAME = "RoughDielectric"
    ENTRY = dict(eval="bsdfd_dielectric_eval", sample_weight="bsdfd_dielectric_sample_weight", sample="bsdfd_dielectric_sample",
                 pdf="bsdfd_dielectric_pdf")
    U_COLS = 3
    FIREFLY = 3.5

    def __init__(self, alpha: float, int_ior="bk7", ext_ior="air", distribution: str = "beckmann"):
        if distribution not in DISTRIBUTIONS:
            raise ValueError(f"RoughDielectric: distribution {distribution!r} is not built (only 'beckmann')")
        self.alpha = float(alpha)
        self.int_ior, self.ext_ior = _ior(int_ior), _ior(ext_ior)
        if not (self.alpha > 0 and self.int_ior > 0 and self.ext_ior > 0):
            raise ValueError("RoughDielectric: alpha and the indices of refraction must be positive")
        self.distribution = distribution
        self.eta = self.int_ior / self.ext_ior
        self._desc = _lib.Dielectric(self.alpha, self.eta, DISTRIBUTIONS[distribution], 0)

    def __repr__(self):
        return f"RoughDielectric(alpha={self.alpha}, int_ior={self.int_ior}, ext_ior={self.ext_ior}, distribution={self.distribution!r})"

    def _lead(self):
        return C.byref(self._desc)

    def _variates(self, sample1, sample2):
        from .plugin_base import _vec
        return torch.cat([_vec(sample2).reshape(-1, 2), _vec(sample1).reshape(-1, 1)], 1).contiguous()

    def _bsdf_sample(self, wi, wo, pdf):
        from .plugin_base import FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, BSDFSample3f
        refl = wi[:, 2] * wo[:, 2] > 0
        eta = torch.where(refl, 1.0, torch.where(wi[:, 2] > 0, self.eta, 1.0 / self.eta))
        # (Mitsuba's flags are Glossy*; the reference's plugin reports the Diffuse pair, which is what plugin_base defines)
        return BSDFSample3f(wo=wo, pdf=pdf, eta=eta, sampled_type=torch.where(refl, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION),
                            sampled_component=torch.where(refl, 0, 1))


def reference_material(idx: int) -> RoughDielectric:
    """Entry ``idx`` of the reference's analytic material list (rendering/utils/bsdf_dict.py) as a native evaluator: 23 / 24 / 25
    are its three rough dielectrics; 0..22 are ``principled`` BSDFs, which are not built."""
    idx = int(idx)
    if idx in REFERENCE_ROUGHDIELECTRIC:
        return RoughDielectric(REFERENCE_ROUGHDIELECTRIC[idx], int_ior="bk7", ext_ior="air")
    if 0 <= idx < N_REFERENCE_MATERIALS:
        raise NotImplementedError(f"material {idx} of the reference's list is a Mitsuba `principled` BSDF: only the "
                                  "roughdielectric entries 23..25 have a native evaluator")
    raise IndexError(f"the reference's material list has entries 0..{N_REFERENCE_MATERIALS - 1}, not {idx}")
