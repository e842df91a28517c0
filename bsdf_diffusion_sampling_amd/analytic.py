"""Analytic ground truth of the full-sphere plugin: the rough dielectric and the principled BSDF on the GPU.

The reference's full-sphere plugin takes its ``eval()``, sample weight and firefly rule from an analytic Mitsuba BSDF out of a
list (rendering/utils/bsdf_dict.py; rendering/bsdf_myresult.py:97-110).  Mitsuba has no AMD GPU variant, so both kinds of entry are
restated from their publications over ``libbsdfd.so``, PARITY-UNPINNED against Mitsuba, like ``measured.MeasuredBSDF``:

* entries 23..25 are ``roughdielectric`` (Beckmann, alpha 0.2 / 0.3 / 0.5, bk7 in air): ``RoughDielectric`` (Walter et al. 2007;
  Mitsuba's defaults: visible-normal sampling, radiance transport; csrc/dielectric.hip, csrc/dielectric_dev.h);
* entries 0..22 are ``principled``: ``Principled`` (Burley 2012 / 2015 with Mitsuba's choices: diffuse + retro-reflection + fake
  subsurface + sheen, a GTR1 clearcoat, specular transmission and reflection over anisotropic GGX, Fresnel mixed with Schlick
  terms; visible normals as in Heitz 2018; csrc/principled.hip, csrc/principled_dev.h).

Each is ``eval`` = f |cos theta_o| on both sides of the surface, its own importance sampler (``sample`` / ``pdf``) and the fused
tail of the plugin's ``sample()`` (``sample_weight``).  ``reference_bsdf(idx)`` builds any entry of the list.  No CPU fallback.

``AnalyticTable`` serves a MIXED-material wavefront — one material id per lane, as a renderer's primary rays write them — in one
launch per call (csrc/analytic_table.hip), where the classes above take one launch per material on gathered slices: every lane
gets the bits of its own material's single-material call, and lanes without ground truth NaN.  Each entry carries an ``albedo``
of its own, the per-ball colour of the reference's array scenes (rendering/bsdf_myresult.py:97,112), multiplied into the call's
tint.  It is what ``wavefront.ArrayRenderer`` and ``pathtrace.PathArrayRenderer`` shade with when their ``ground_truth`` is
analytic; ``ground_truth_for(names)`` builds that dict for the materials named ``bsdf_<idx>``.  Under occlusion those renderers drop
a BSDF sample below the surface unless ``PathArrayRenderer(..., transmission=True)`` follows it through the ball — the vertices
inside are then sampled here, by the models themselves (``AnalyticTable.sample_inside``) —, and without occlusion such a direction
looks the environment up weighted with the transmission lobe's ``f |cos|``.  Measured against the per-material
loop it replaces: profiles/analytic_table.json (tools/analytic_table_bench.py).
"""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Optional, Sequence

import torch

from . import _lib
from .ground_truth import GroundTruth, RowKernels

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


class FullSphereGroundTruth(GroundTruth):
    """What the full-sphere plugin fuses with (``bsdf_myresult.MyBSDF.FUSED_GT``): an analytic model of both sides of the surface whose
    ``sample_weight`` is the tail of that plugin's sample() (rendering/bsdf_myresult.py:97-104) — value = 0 where pdf_sa <= 0, the
    firefly rule reads value.x at 3.5, no cosine masks — and whose sampler takes ``u`` [N,3]: Mitsuba's sample2, then its sample1."""

    U_COLS = 3
    FIREFLY = 3.5

    def _lead(self):
        return C.byref(self._desc)

    def _variates(self, sample1, sample2):
        from .plugin_base import _vec
        return torch.cat([_vec(sample2).reshape(-1, 2), _vec(sample1).reshape(-1, 1)], 1).contiguous()


class RoughDielectric(FullSphereGroundTruth):
    """``eval_t`` = f |cos theta_o|, grey: reflection and (radiance-mode) transmission, either side.  ``sample_weight`` is the tail
    of the full-sphere plugin's sample() (rendering/bsdf_myresult.py:97-104): value = 0 where pdf_sa <= 0, the firefly rule reads
    value.x, no cosine masks.  ``sample_t`` takes ``u`` [N,3] in [0,1)^3 (columns 0..1: Mitsuba's sample2, the visible normal;
    column 2: sample1, reflection iff u2 <= F); weight is 0 where the pdf is 0 or wo ends up on the wrong side for its lobe, and
    rows with wi.z == 0 get zeros.  ``sample`` fills eta and sampled_type per lobe; ``sample1`` [N] picks the lobe."""

    NAME = "RoughDielectric"
    ENTRY = dict(eval="bsdfd_dielectric_eval", sample_weight="bsdfd_dielectric_sample_weight", sample="bsdfd_dielectric_sample",
                 pdf="bsdfd_dielectric_pdf")

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

    def _bsdf_sample(self, wi, wo, pdf):
        from .plugin_base import FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, BSDFSample3f
        refl = wi[:, 2] * wo[:, 2] > 0
        eta = torch.where(refl, 1.0, torch.where(wi[:, 2] > 0, self.eta, 1.0 / self.eta))
        # (Mitsuba's flags are Glossy*; the reference's plugin reports the Diffuse pair, which is what plugin_base defines)
        return BSDFSample3f(wo=wo, pdf=pdf, eta=eta, sampled_type=torch.where(refl, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION),
                            sampled_component=torch.where(refl, 0, 1))


def eta_of_specular(specular: float) -> float:
    """Mitsuba's ``specular`` parameter as a relative index of refraction (1 -> 1.78885, the 1.788 of the reference's plugin)."""
    return 2.0 / (1.0 - math.sqrt(0.08 * float(specular))) - 1.0


class Principled(FullSphereGroundTruth):
    """``eval_t`` = f |cos theta_o| per channel: diffuse (+ retro-reflection, fake subsurface, sheen) and clearcoat above the
    surface, specular reflection and (radiance-mode) transmission on either side.  The parameters are Mitsuba's, each in [0, 1];
    the interface is given as ``specular`` OR ``eta`` (>= 1; neither: Mitsuba's specular = 0.5, eta 1.5).  ``sample_t`` takes ``u``
    [N,3] in [0,1)^3 (columns 0..1: Mitsuba's sample2; column 2: sample1, which picks the lobe on the cumulative order diffuse,
    clearcoat, transmission, reflection); a failed sample is zeros in wo, pdf and weight.  ``sample`` fills eta, sampled_type and
    sampled_component (Mitsuba's 0..3, in that order)."""

    NAME = "Principled"
    ENTRY = dict(eval="bsdfd_principled_eval", sample_weight="bsdfd_principled_sample_weight", sample="bsdfd_principled_sample",
                 pdf="bsdfd_principled_pdf")
    UNIT = ("roughness", "anisotropic", "metallic", "spec_trans", "spec_tint", "sheen", "sheen_tint", "flatness", "clearcoat",
            "clearcoat_gloss")

    def __init__(self, base_color=(1.0, 1.0, 1.0), roughness=0.5, anisotropic=0.0, metallic=0.0, spec_trans=0.0, specular=None,
                 eta=None, spec_tint=0.0, sheen=0.0, sheen_tint=0.0, flatness=0.0, clearcoat=0.0, clearcoat_gloss=0.0):
        if specular is not None and eta is not None:
            raise ValueError("Principled: give specular or eta, not both")
        given = dict(roughness=roughness, anisotropic=anisotropic, metallic=metallic, spec_trans=spec_trans, spec_tint=spec_tint,
                     sheen=sheen, sheen_tint=sheen_tint, flatness=flatness, clearcoat=clearcoat, clearcoat_gloss=clearcoat_gloss)
        self.base_color = tuple(float(c) for c in base_color)
        for k in self.UNIT:
            setattr(self, k, float(given[k]))
        if len(self.base_color) != 3 or not all(0.0 <= v <= 1.0 for v in self.base_color + tuple(getattr(self, k) for k in self.UNIT)):
            raise ValueError("Principled: base_color (3 channels) and every parameter but eta must lie in [0, 1]")
        if specular is not None and not 0.0 <= float(specular) <= 1.0:
            raise ValueError("Principled: specular must lie in [0, 1]")
        self.eta = float(eta) if eta is not None else eta_of_specular(0.5 if specular is None else specular)
        if not (self.eta >= 1.0 and math.isfinite(self.eta)):
            raise ValueError("Principled: eta must be finite and >= 1")
        if self.eta == 1.0 and self.spec_trans > 0.0:
            raise ValueError("Principled: eta == 1 (no interface) needs spec_trans == 0")
        # derived, as csrc/principled.hip forms them (there in fp32): the GGX roughness pair, the lobe weights and the two
        # constant thresholds of the lobe choice
        aspect = math.sqrt(1.0 - 0.9 * self.anisotropic)
        self.ax, self.ay = max(1e-3, self.roughness ** 2 / aspect), max(1e-3, self.roughness ** 2 * aspect)
        self.brdf, self.bsdf = (1.0 - self.metallic) * (1.0 - self.spec_trans), (1.0 - self.metallic) * self.spec_trans
        total = 1.0 + 0.25 * self.clearcoat + self.brdf
        self.cum_d, self.cum_c = self.brdf / total, (self.brdf + 0.25 * self.clearcoat) / total
        self._desc = _lib.Principled((C.c_float * 3)(*self.base_color), self.roughness, self.anisotropic, self.metallic,
                                     self.spec_trans, self.eta, self.spec_tint, self.sheen, self.sheen_tint, self.flatness,
                                     self.clearcoat, self.clearcoat_gloss)

    def __repr__(self):
        return (f"Principled(base_color={self.base_color}, eta={self.eta}, "
                + ", ".join(f"{k}={getattr(self, k)}" for k in self.UNIT) + ")")

    def _bsdf_sample(self, wi, wo, pdf):
        from .plugin_base import FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION, BSDFSample3f
        refl = wi[:, 2] * wo[:, 2] > 0
        eta = torch.where(refl, 1.0, torch.where(wi[:, 2] > 0, self.eta, 1.0 / self.eta))
        # (Mitsuba's flags are Glossy* / Diffuse*; the reference's plugin reports the Diffuse pair, which is what plugin_base defines)
        return BSDFSample3f(wo=wo, pdf=pdf, eta=eta, sampled_type=torch.where(refl, FLAG_DIFFUSE_REFLECTION, FLAG_DIFFUSE_TRANSMISSION),
                            sampled_component=torch.where(refl, 3, 2))

    def sample(self, ctx, si, sample1, sample2, active=True):
        """``mi.BSDF.sample``: -> (BSDFSample3f, weight [N,3]); ``sampled_component`` 0..3 = diffuse, clearcoat, transmission,
        reflection: sample1 against the two constant thresholds (0 from inside), then the side of wo."""
        from .plugin_base import _vec, _wi_of
        bs, weight = super().sample(ctx, si, sample1, sample2, active)
        front, u2 = _wi_of(si)[:, 2] > 0, _vec(sample1).reshape(-1)
        bs.sampled_component = torch.where(u2 < torch.where(front, self.cum_d, 0.0), 0,
                                           torch.where(u2 < torch.where(front, self.cum_c, 0.0), 1, bs.sampled_component))
        return bs, weight


# rendering/utils/bsdf_dict.py: the 23 principled entries as (metallic, specular, roughness, anisotropic); everything else is common
# to them (sheen_tint: 0.3 at idx 7).  The file defines dict4_principled twice: the second definition wins, which is row 3.
REFERENCE_PRINCIPLED = {
    0: (.1, 1, .2, .5), 1: (.3, .7, .5, .5), 2: (1, .8, .1, .5), 3: (.2, .3, .3, .7), 4: (.1, .8, .3, .7), 5: (.1, 1, .1, .7),
    6: (.9, .7, .3, .7), 7: (.5, .8, .3, .7), 8: (.1, .8, .3, .7), 9: (.3, .2, .1, .7), 10: (0, 1, .1, .7), 11: (.8, .2, .1, .7),
    12: (.6, .2, .3, .7), 13: (.3, .2, .7, .7), 14: (.9, .2, .5, .7), 15: (.9, .2, .3, .7), 16: (.9, .2, .6, .7), 17: (.9, .2, .9, .7),
    18: (.1, .8, .1, .7), 19: (.1, .5, .4, .7), 20: (.1, .8, .3, .7), 21: (.1, .5, .7, .7), 22: (.1, .3, .8, .7),
}
REFERENCE_PRINCIPLED_COMMON = dict(base_color=(1.0, 1.0, 1.0), spec_tint=0.5, sheen=0.5, sheen_tint=0.5, clearcoat=0.5,
                                   clearcoat_gloss=0.5, spec_trans=0.9, flatness=1.0)


def reference_bsdf(idx: int):
    """Entry ``idx`` of the reference's analytic material list (rendering/utils/bsdf_dict.py) as a native evaluator: a
    ``Principled`` for 0..22, a ``RoughDielectric`` for 23..25."""
    idx = int(idx)
    if idx in REFERENCE_ROUGHDIELECTRIC:
        return RoughDielectric(REFERENCE_ROUGHDIELECTRIC[idx], int_ior="bk7", ext_ior="air")
    if idx in REFERENCE_PRINCIPLED:
        metallic, specular, roughness, anisotropic = REFERENCE_PRINCIPLED[idx]
        params = dict(REFERENCE_PRINCIPLED_COMMON, metallic=metallic, specular=specular, roughness=roughness, anisotropic=anisotropic)
        if idx == 7:
            params["sheen_tint"] = 0.3
        return Principled(**params)
    raise IndexError(f"the reference's material list has entries 0..{N_REFERENCE_MATERIALS - 1}, not {idx}")


def reference_material(idx: int) -> RoughDielectric:
    """The rough dielectrics of the reference's list, 23 / 24 / 25, as native evaluators — what the full-sphere plugin builds by
    default.  0..22 are ``principled`` BSDFs, which this call keeps refusing: ``reference_bsdf`` builds every entry."""
    idx = int(idx)
    if idx in REFERENCE_ROUGHDIELECTRIC:
        return reference_bsdf(idx)
    if 0 <= idx < N_REFERENCE_MATERIALS:
        raise NotImplementedError(f"material {idx} of the reference's list is a Mitsuba `principled` BSDF, which this call does not "
                                  "build: reference_bsdf(idx) does (analytic.Principled)")
    raise IndexError(f"the reference's material list has entries 0..{N_REFERENCE_MATERIALS - 1}, not {idx}")


class AnalyticTable(RowKernels):
    """The analytic models for a mixed-material wavefront: ``entries[m]`` (a ``Principled``, a ``RoughDielectric``, or None = no
    ground truth) serves the lanes whose ``material_id`` is m, in ONE launch on the wavefront in LANE order, call for call what
    ``measured.MeasuredTable`` is for the measured materials.  Lanes with ground truth get that entry's single-material result bit
    for bit, every other lane (None entry, id negative or >= len(entries): a renderer's floor hits and misses) NaN.
    ``albedo``: None, or one RGB triple per entry, finite and >= 0: lane by lane the tint is ``float32(tint) * float32(albedo[m])``.
    The native table is created here, on the current device; it copies what it needs from the entries."""

    NAME = "AnalyticTable"
    ENTRY = dict(eval="bsdfd_analytic_eval_table", sample_weight="bsdfd_analytic_sample_weight_table",
                 sample="bsdfd_analytic_sample_table", pdf="bsdfd_analytic_pdf_table")
    U_COLS = 3
    FIREFLY = 3.5
    MAX_MATERIALS = 65536

    def __init__(self, entries: Sequence[Optional[FullSphereGroundTruth]], albedo=None):
        self.entries = list(entries)
        if not 1 <= len(self.entries) <= self.MAX_MATERIALS:
            raise ValueError(f"AnalyticTable: 1..{self.MAX_MATERIALS} entries")
        if any(e is not None and not isinstance(e, (Principled, RoughDielectric)) for e in self.entries):
            raise ValueError("AnalyticTable: entries are Principled or RoughDielectric objects, or None")
        self.albedo = [(1.0, 1.0, 1.0)] * len(self.entries) if albedo is None else \
            [tuple(float(v) for v in (a.tolist() if hasattr(a, "tolist") else a)) for a in albedo]
        if len(self.albedo) != len(self.entries) or any(len(a) != 3 for a in self.albedo):
            raise ValueError("AnalyticTable: albedo is None or one RGB triple per entry")
        self._t = C.c_void_p()
        recs = (_lib.AnalyticEntry * len(self.entries))()
        for r, e, a in zip(recs, self.entries, self.albedo):
            r.albedo = (C.c_float * 3)(*a)
            if isinstance(e, Principled):
                r.kind, r.desc.principled = _lib.ANALYTIC_PRINCIPLED, e._desc
            elif isinstance(e, RoughDielectric):
                r.kind, r.desc.dielectric = _lib.ANALYTIC_DIELECTRIC, e._desc
        _lib.check(_lib.lib().bsdfd_analytic_table_create(recs, len(self.entries), C.byref(self._t)))

    def __len__(self):
        return len(self.entries)

    def __del__(self):
        try:
            if getattr(self, "_t", None) is not None and self._t.value:
                _lib.lib().bsdfd_analytic_table_destroy(self._t)
                self._t = C.c_void_p()
        except Exception:
            pass

    def _lead(self):
        return self._t

    def eval_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, wl: Optional[torch.Tensor] = None,
               tint=None, out_o: Optional[torch.Tensor] = None, out_l: Optional[torch.Tensor] = None,
               rows: Optional[torch.Tensor] = None):
        """f(wi, wo) |cos theta_o| * tint * albedo of each lane's material -> f_o [N,3]; with ``wl`` also f(wi, wl) |cos theta_l|
        -> (f_o, f_l), both evaluations in the same launch.  NaN rows = no ground truth for that lane.  ``rows`` (int64 [n_rows]):
        only the listed rows are evaluated and written (``bsdfd_analytic_eval_table_rows``); every other row keeps what it held."""
        return self._eval_table(material_id, wi, wo, wl, tint, out_o, out_l, rows)

    def sample_weight(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, pdf_sa: torch.Tensor, *, tint=None,
                      firefly_threshold: Optional[float] = None, active: Optional[torch.Tensor] = None):
        """``sample_weight`` of each lane's material in one launch -> (weight [N,3], pdf [N]); lanes without ground truth get
        weight NaN and pdf = pdf_sa."""
        return self._sample_weight(material_id, wi, wo, pdf_sa, tint, firefly_threshold, active)

    def sample_t(self, material_id: torch.Tensor, wi: torch.Tensor, u: torch.Tensor, tint=None,
                 active: Optional[torch.Tensor] = None, out=None):
        """``sample_t`` of each lane's material (``u`` [N,3]) in one launch -> (wo [N,3], pdf [N], weight [N,3]); lanes without
        ground truth get NaN in all three."""
        return self._sample_t(material_id, wi, u, tint, active, out)

    def pdf_t(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, active: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pdf_t`` of each lane's material in one launch -> [N]; NaN = no ground truth for that lane."""
        return self._pdf_t(material_id, wi, wo, active, out)

    def sample_inside(self, material_id: torch.Tensor, wi: torch.Tensor, wl: torch.Tensor, bounce: int, seed: int, pass_idx: int,
                      path_offset: int, out, rows: Optional[torch.Tensor] = None):
        """The sampler's answer for a path tracer's vertices INSIDE a ball, in place: on every lane with ``0 <= material_id <
        len(self)`` and ``wi.z < 0``, ``out`` = (wo [N,3], pdf_o [N], pdf_l [N]) receives ``sample_t(wi, u)``'s direction and
        density and ``pdf_t(wi, wl)``, bit for bit, at variates of the lane's own: ``u_k = (word k >> 8) * 2^-24`` of
        philox(key = seed, counter = (path_offset + lane, pass_idx, "Insd" + bounce)) — but ``pdf_o = 0`` where ``sample_t``'s weight
        is 0 in every channel (a failed sample: the bounce, which weights with ``f(wi, wo) / pdf_o`` of the pair, must drop it).  A
        None entry gets zeros.  Every other lane
        keeps what it held.  ``rows`` (int64 [n_rows], distinct lanes): only the listed lanes are looked at
        (``bsdfd_wf_sample_inside_rows``).  -> ``out``."""
        from .ground_truth import check, launch
        who = self.NAME + ".sample_inside"
        if out is None or len(out) != 3:
            raise ValueError(f"{who}: out is a (wo [N,3], pdf_o [N], pdf_l [N]) triple, written in place")
        wo, pdf_o, pdf_l = out
        check(who, (("wi", wi, 3), ("wl", wl, 3), ("wo", wo, 3), ("pdf_o", pdf_o, 0), ("pdf_l", pdf_l, 0)), material_id)
        if rows is not None and not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.dim() == 1
                                     and rows.is_contiguous() and rows.device == wi.device and rows.shape[0] <= wi.shape[0]):
            raise ValueError(f"{who}: rows must be a contiguous int64 tensor [n_rows <= N] on the device of wi")
        m64 = 0xFFFFFFFFFFFFFFFF
        args = (self._lead(), int(bounce), int(seed) & m64, int(pass_idx) & m64, int(path_offset) & m64, wi.shape[0], material_id,
                wi, wl, wo, pdf_o, pdf_l)
        if rows is None:
            launch("bsdfd_wf_sample_inside", wi.device, *args)
        else:
            launch("bsdfd_wf_sample_inside_rows", wi.device, *args, rows, rows.shape[0])
        torch.autograd.graph.increment_version([wo, pdf_o, pdf_l])
        return out


def ground_truth_for(names) -> dict:
    """{i: reference_bsdf(idx)} for every ``names[i]`` of the form ``bsdf_<idx>`` or ``bsdf_<idx>_spherical`` (what
    ``wavefront.scene_from_matpreview_xml`` calls the ``mybsdf idx = N`` balls): the ``ground_truth`` of the array renderers.
    Other names (the measured materials) are left out; an idx the reference's list does not have raises ``IndexError``."""
    out = {}
    for i, name in enumerate(names):
        m = re.fullmatch(r"bsdf_(\d+)(_spherical)?", str(name))
        if m:
            out[i] = reference_bsdf(int(m.group(1)))
    return out
