"""Importance sampling of a lat-long environment map (csrc/pathenv.hip, csrc/env_dev.h; C ABI ``bsdfd_env_sample`` /
``bsdfd_env_pdf``, and ``bsdfd_wf_sample_env`` / ``bsdfd_wf_bounce_env`` in ``pathtrace.PathArrayRenderer``).

The reference's ``envmap`` scenes (matpreview/disney_bsdf_array{0,1}_envmap.xml, disney_bsdf_array2_spherical_envmap.xml,
scene_measured.xml) are lit by Mitsuba's ``envmap`` emitter, which draws directions in proportion to the map's luminance:
a bilinear ``Hierarchical2D`` over luminance x sin(theta).  The distribution here is simpler and is **not pinned to Mitsuba's**
(like the evaluator of the environment itself, ``env_lookup``): piecewise constant over the unit square of ``env_lookup``'s own
parameterisation, ``u = atan2(x, -z) / 2pi`` (wrapped), ``v = theta / pi``, cell (j, i) = ``[i/W, (i+1)/W) x [j/H, (j+1)/H)``:

    lum[j, i]  Rec. 709 luminance of texel (j, i)
    B[j, i]    the maximum of lum over the 3x3 neighbourhood, wrapped in x and clamped in y.  ``env_lookup`` is bilinear about
               the texel centres: inside cell (j, i) it reads only texels j-1..j+1, i-1..i+1, so the density is positive wherever
               the looked-up radiance is, and radiance / density stays bounded
    weight     B[j, i] * (cos(pi j / H) - cos(pi (j+1) / H)), the row's exact share of the solid angle
    pdf_uv     weight / sum(weights) * W * H;  per solid angle: pdf_uv[cell] / (2 pi^2 max(sin theta, 1e-6))

The tables are built once per map in fp64 (as the RGL loader builds its warps) and rounded to fp32 for the device.  There is no
CPU fallback for the sampling itself: ``sample_t`` / ``pdf_t`` run the kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

REC709 = (0.2126, 0.7152, 0.0722)


def build_tables(env) -> dict:
    """env [H, W, 3] (anything ``np.asarray`` takes) -> dict(marginal [H+1], conditional [H, W+1], pdf_uv [H, W]), fp32 rounded
    from an fp64 build.  First CDF entries are exactly 0, last exactly 1; a row without weight gets a uniform conditional (it is
    never chosen: its marginal cell has no width).  ``ValueError`` for a map without positive finite luminance."""
    env = np.asarray(env, dtype=np.float64)
    if env.ndim != 3 or env.shape[2] != 3 or env.shape[0] < 1 or env.shape[1] < 1:
        raise ValueError("env must be [H,W,3]")
    h, w = env.shape[:2]
    lum = env @ np.asarray(REC709)
    if not np.isfinite(lum).all() or (lum < 0).any():
        raise ValueError("the environment map's luminance must be finite and non-negative")
    rows = np.clip(np.arange(-1, 2)[:, None] + np.arange(h)[None, :], 0, h - 1)      # clamped in y
    big = np.max([np.roll(lum[r], s, axis=1) for r in rows for s in (-1, 0, 1)], axis=0)   # wrapped in x
    edges = np.cos(np.pi * np.arange(h + 1) / h)
    weight = big * (edges[:-1] - edges[1:])[:, None]
    row = weight.sum(1)
    total = row.sum()
    if not total > 0.0:
        raise ValueError("the environment map is black: there is nothing to sample")
    marginal = np.concatenate([[0.0], np.cumsum(row)])
    marginal /= marginal[-1]
    conditional = np.concatenate([np.zeros((h, 1)), np.cumsum(weight, axis=1)], axis=1)
    empty = conditional[:, -1] <= 0.0
    conditional[empty] = np.arange(w + 1, dtype=np.float64)[None, :]
    conditional /= conditional[:, -1:]
    out = dict(marginal=marginal.astype(np.float32), conditional=conditional.astype(np.float32),
               pdf_uv=(weight / total * (w * h)).astype(np.float32))
    out["marginal"][0], out["marginal"][-1] = 0.0, 1.0
    out["conditional"][:, 0], out["conditional"][:, -1] = 0.0, 1.0
    return out


class EnvDistribution:
    """The sampling distribution of an environment map [H, W, 3] (a torch tensor or an array).  ``tables`` are the host's fp32
    arrays; the device copies are made on first use on a device and kept."""

    def __init__(self, env):
        if hasattr(env, "detach"):
            env = env.detach().cpu().numpy()
        self.tables = build_tables(env)
        self.height, self.width = self.tables["pdf_uv"].shape
        self._dev = {}

    def struct(self, device) -> _lib.EnvDist:
        """The ``bsdfd_env_dist`` of the tables on ``device`` (uploaded once; the struct points into tensors this object keeps)."""
        import torch
        device = torch.device(device)
        if device not in self._dev:
            t = {k: torch.from_numpy(v).to(device).contiguous() for k, v in self.tables.items()}
            s = _lib.EnvDist()
            s.marginal, s.conditional, s.pdf_uv = (t[k].data_ptr() for k in ("marginal", "conditional", "pdf_uv"))
            s.width, s.height = self.width, self.height
            self._dev[device] = (s, t)
        return self._dev[device][0]

    @staticmethod
    def _rows(t, cols: int, name: str):
        import torch
        if t.dim() != 2 or t.shape[1] != cols or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{name} must be a float32 [N,{cols}] tensor on a GPU")
        return t.contiguous()

    def sample_t(self, u):
        """u [N,2] in [0,1) (column 0 picks the row, column 1 the column) -> (dir [N,3] world, y up; pdf [N] per solid angle)."""
        import torch
        u = self._rows(u, 2, "u")
        n = u.shape[0]
        d = torch.empty((n, 3), dtype=torch.float32, device=u.device)
        pdf = torch.empty((n,), dtype=torch.float32, device=u.device)
        with torch.cuda.device(u.device):
            _lib.check(_lib.lib().bsdfd_env_sample(C.byref(self.struct(u.device)), n, C.c_void_p(u.data_ptr()),
                                                   C.c_void_p(d.data_ptr()), C.c_void_p(pdf.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(u.device).cuda_stream)))
        return d, pdf

    def pdf_t(self, d):
        """d [N,3] unit, world -> the density [N] per solid angle with which ``sample_t`` returns it."""
        import torch
        d = self._rows(d, 3, "d")
        n = d.shape[0]
        pdf = torch.empty((n,), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            _lib.check(_lib.lib().bsdfd_env_pdf(C.byref(self.struct(d.device)), n, C.c_void_p(d.data_ptr()),
                                                C.c_void_p(pdf.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(d.device).cuda_stream)))
        return pdf
