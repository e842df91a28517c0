"""Full-sphere analytic-BSDF plugin (transmission) — mirror of rendering/bsdf_myresult.py:41-139.

Same spherical operators, different post-processing:
  ctor   (:43-57)   props["idx"] selects ``bsdf_<idx>_spherical`` weights, props["albedo"];
                    flags Diffuse | FrontSide | BackSide.
  sample (:59-104)  only the sin(theta_o) > 5e-5 guard (no cos guard: theta in [0, pi]);
                    pdf_sa = pdf * clamp(1/|sin theta_o|, 1, FLT_MAX);
                    eta = 1 above / 1.788 below the surface, sampled_type 8 / 16 (:89-90);
                    weight = f * albedo / pdf * sin(theta_o) (:97); pdf := 0 where weight.x >= 3.5 (:100-103).
  pdf    (:115-133) no guards, no cos masks: pdf * clamp(1/|sin theta_o|, 1, FLT_MAX).
  eval   (:106-113) ground truth from the analytic BSDF list, no cos masks.

The list is rendering/utils/bsdf_dict.py.  Its entries 23..25 are rough dielectrics, which ``analytic.RoughDielectric`` evaluates
natively: for those ``idx`` the plugin has its ground truth by default (``props["analytic"] = False`` turns that off, ``props["bsdf"]``
overrides it) — eval() is one launch and sample()'s weight and firefly rule another.  Entries 0..22 are Mitsuba ``principled``
BSDFs, which ``analytic.Principled`` evaluates natively; that one is opt-in: ``props["analytic"] = "all"`` gives every ``idx`` its
native evaluator (``analytic.reference_bsdf``).  By default ``self.bsdf`` stays None there unless ``props["bsdf"]`` is given,
sample() returns ``(bs, None)`` and eval() raises.
"""
from __future__ import annotations

import torch

from . import _lib
from . import weights as W
from .plugin_base import (FLAG_BACK_SIDE, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, FLAG_FRONT_SIDE,
                          BSDFSample3f, NeuralBSDFCore)


class MyBSDF(NeuralBSDFCore):
    DOMAIN = W.DOMAIN_SPHERICAL
    DOMAIN_NAME = "spherical"
    VARIANT = _lib.PLUGIN_FULLSPHERE
    T = 8
    FIREFLY = 3.5
    FUSED_GT = "analytic.FullSphereGroundTruth"
    WEIGHT_TAKES_ACTIVE = False  # as in the reference: ``active`` reaches the flow only

    def __init__(self, props):
        super().__init__(props)
        self.idx = int(self._get("idx"))
        self.m_flags = FLAG_DIFFUSE_REFLECTION | FLAG_DIFFUSE_TRANSMISSION | FLAG_FRONT_SIDE | FLAG_BACK_SIDE
        self.m_components = [self.m_flags]
        analytic = self._get("analytic", True)
        if isinstance(analytic, str) and analytic != "all":
            raise ValueError(f"props['analytic'] is True, False or 'all', not {analytic!r}")
        if self.bsdf is None and analytic:
            from .analytic import REFERENCE_ROUGHDIELECTRIC, reference_bsdf
            if analytic == "all" or self.idx in REFERENCE_ROUGHDIELECTRIC:
                self.bsdf = reference_bsdf(self.idx)

    def _material_name(self) -> str:
        return f"bsdf_{int(self._get('idx'))}"

    def _ckpt_tag(self) -> str:
        return str(int(self._get("idx")))

    def _bsdf_sample(self, wo, pdf_sa):
        up = wo[:, 2] > 0
        return BSDFSample3f(wo=wo, pdf=pdf_sa, eta=torch.where(up, 1.0, 1.788),
                            sampled_type=torch.where(up, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION),
                            sampled_component=2)

    def _weight_lines(self, value, wi, bs, act):
        # value = f * albedo / pdf * sin(theta_o) with pdf_sa = pdf / sin(theta_o) wherever the clamp is inactive
        value = torch.where((bs.pdf > 0)[:, None], value, torch.zeros_like(value))
        bs.pdf = self.apply_firefly_clamp(bs.pdf, value[:, 0], self.FIREFLY)
        return torch.where((bs.pdf > 0)[:, None], value, torch.zeros_like(value))

    def _eval_lines(self, ctx, si, wo, wi, wo_t):
        return self.eval_unmasked(ctx, si, wo)  # no cos masks
