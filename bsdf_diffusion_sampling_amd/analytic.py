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
from typing import Optional

import torch

from . import _lib
from .measured import MeasuredBSDF, _launch

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


class RoughDielectric:
    WHO = "RoughDielectric"

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

    @classmethod
    def _check(cls, **tensors):
        try:
            MeasuredBSDF._check(**tensors)
        except ValueError as e:
            raise ValueError(str(e).replace("MeasuredBSDF", cls.WHO)) from None

    def _d(self):
        return C.byref(self._desc)

    # ---- tensor calls ---------------------------------------------------------------------------------------------------
    def eval_t(self, wi: torch.Tensor, wo: torch.Tensor, out: Optional[torch.Tensor] = None, tint=None) -> torch.Tensor:
        """f(wi, wo) |cos theta_o| [* tint] -> [N,3], grey; reflection and (radiance-mode) transmission, either side."""
        if out is None:
            out = torch.empty_like(wi)
        self._check(wi=(wi, 3), wo=(wo, 3), out=(out, 3))
        _launch("bsdfd_dielectric_eval", wi.device, self._d(), wi, wo, wi.shape[0], MeasuredBSDF._tint(tint), out)
        return out

    def sample_weight(self, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, tint=None, firefly_threshold: float = 3.5,
                      active: Optional[torch.Tensor] = None):
        """The tail of the full-sphere plugin's sample() in one launch (rendering/bsdf_myresult.py:97-104) -> (weight [N,3],
        pdf [N]): value = f * tint / pdf_sa (0 where pdf_sa <= 0), pdf = pdf_sa where value.x < threshold else 0, weight = value
        where pdf > 0.  No cosine masks.  Rows with ``active`` false get zeros."""
        self._check(wi=(wi, 3), wo=(wo, 3), pdf_sa=(pdf_sa, 0))
        act = MeasuredBSDF._active(active, wi.shape[0], wi.device, self.WHO + ".sample_weight")
        weight, pdf = torch.empty_like(wi), torch.empty_like(pdf_sa)
        _launch("bsdfd_dielectric_sample_weight", wi.device, self._d(), wi, wo, pdf_sa, act, wi.shape[0], MeasuredBSDF._tint(tint),
                float(firefly_threshold), weight, pdf)
        return weight, pdf

    def sample_t(self, wi: torch.Tensor, u: torch.Tensor, tint=None, active: Optional[torch.Tensor] = None, out=None):
        """The model's own importance sampler at the variates ``u`` [N,3] in [0,1)^3 (columns 0..1: Mitsuba's sample2, the
        visible normal; column 2: sample1, reflection iff u2 <= F) -> (wo [N,3], pdf [N], weight [N,3]), weight = f |cos| [*
        tint] / pdf, 0 where the pdf is 0 or wo ends up on the wrong side for its lobe.  Rows with wi.z == 0 or ``active`` false
        get zeros.  ``out`` = (wo, pdf, weight) buffers to write into."""
        wo, pdf, weight = MeasuredBSDF._sample_out(wi, out, self.WHO + ".sample_t")
        self._check(wi=(wi, 3), u=(u, 3), wo=(wo, 3), pdf=(pdf, 0), weight=(weight, 3))
        act = MeasuredBSDF._active(active, wi.shape[0], wi.device, self.WHO + ".sample_t")
        _launch("bsdfd_dielectric_sample", wi.device, self._d(), wi, u, act, wi.shape[0], MeasuredBSDF._tint(tint), wo, pdf, weight)
        return wo, pdf, weight

    def pdf_t(self, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Solid-angle density with which ``sample_t(wi, .)`` returns ``wo`` -> [N]; 0 on rows with ``active`` false."""
        if out is None:
            out = torch.empty(wi.shape[0], dtype=torch.float32, device=wi.device)
        self._check(wi=(wi, 3), wo=(wo, 3), out=(out, 0))
        act = MeasuredBSDF._active(active, wi.shape[0], wi.device, self.WHO + ".pdf_t")
        _launch("bsdfd_dielectric_pdf", wi.device, self._d(), wi, wo, act, wi.shape[0], out)
        return out

    # ---- the call shapes of ``mi.BSDF`` -----------------------------------------------------------------------------------
    def eval(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        return self.eval_t(_wi_of(si), _vec(wo))

    def sample(self, ctx, si, sample1, sample2, active=True):
        """``mi.BSDF.sample``: -> (BSDFSample3f(wo, pdf, eta, sampled_type), weight [N,3]); ``sample1`` [N] picks the lobe."""
        from .plugin_base import FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, BSDFSample3f, _vec, _wi_of
        wi = _wi_of(si)
        u = torch.cat([_vec(sample2).reshape(-1, 2), _vec(sample1).reshape(-1, 1)], 1).contiguous()
        wo, pdf, weight = self.sample_t(wi, u, active=MeasuredBSDF._mask_of(active, wi))
        refl = wi[:, 2] * wo[:, 2] > 0
        eta = torch.where(refl, 1.0, torch.where(wi[:, 2] > 0, self.eta, 1.0 / self.eta))
        # (Mitsuba's flags are Glossy*; the reference's plugin reports the Diffuse pair, which is what plugin_base defines)
        return BSDFSample3f(wo=wo, pdf=pdf, eta=eta, sampled_type=torch.where(refl, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION),
                            sampled_component=torch.where(refl, 0, 1)), weight

    def pdf(self, ctx, si, wo, active=True):
        from .plugin_base import _vec, _wi_of
        wi = _wi_of(si)
        return self.pdf_t(wi, _vec(wo), active=MeasuredBSDF._mask_of(active, wi))

    def eval_pdf(self, ctx, si, wo, active=True):
        return self.eval(ctx, si, wo, active), self.pdf(ctx, si, wo, active)


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
