"""Path tracer for the array scene: occlusion and further bounces (csrc/pathtrace.hip, C ABI ``bsdfd_wf_path_begin`` /
``bsdfd_wf_bounce`` / ``bsdfd_wf_resolve``).

The reference renders its 12-ball array scenes with Mitsuba's ``path`` integrator at unbounded depth
(matpreview/disney_bsdf_array*_envmap.xml, scene_measured.xml: ``max_depth = -1``): balls shadow the floor and each
other, light reflected by one measured material lands on the next, and every further vertex calls the plugin's
``sample()`` / ``pdf()`` again.  ``ArrayRenderer`` stops after one bounce and traces no secondary ray; this class adds
the loop that feeds a shrinking wavefront through the same pieces bounce after bounce:

    primary -> path_begin (org, beta = 1, rad = env for a miss)
    per bounce k:  table.bucket(mat)            ended paths carry the "miss" id and sort behind the materials
                   table.sample_pdf(plan, ...)  flow evaluations for the lanes that carry a material only
                   measured_table.eval_t(...)   when there is ground truth
                   bounce(k, last = k == max_depth - 1)
    resolve -> film tile += mean_spp of rad

The geometry is at most 32 analytic spheres and one plane, intersected by brute force like the primary rays.  Only the
environment emits.  There is no Russian roulette: a path ends when it escapes, when its BSDF sample is invalid, or at
``max_depth``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from .wavefront import ArrayRenderer

_M64 = 0xFFFFFFFFFFFFFFFF


class PathArrayRenderer(ArrayRenderer):
    """``ArrayRenderer`` with ``max_depth`` vertices per path and, with ``occlusion``, shadow rays.

    ``max_depth=1, occlusion=False`` (the defaults) is ``ArrayRenderer``'s estimator through the path kernels.
    ``occlusion=None`` means ``max_depth > 1``: a deeper path must know what its BSDF sample hit, so ``max_depth > 1`` with
    ``occlusion=False`` is refused (it would count the environment through the balls at every depth).
    Bounce 0 draws with ``ArrayRenderer.render_pass``'s sampler key; bounce k > 0 with ``key ^ (k * 0xD1B54A32D192ED03)``.
    ``stats["lanes_per_bounce"]``: the material lanes served at each bounce of the last pass — the compaction is the
    bucketing itself, no mask machinery."""

    def __init__(self, *args, max_depth: int = 1, occlusion: Optional[bool] = None, **kwargs):
        max_depth = int(max_depth)
        if max_depth < 1:
            raise ValueError("max_depth must be >= 1")
        occlusion = max_depth > 1 if occlusion is None else bool(occlusion)
        if max_depth > 1 and not occlusion:
            raise ValueError("max_depth > 1 needs occlusion: without it every vertex would see the environment through the balls")
        super().__init__(*args, **kwargs)
        if self.use_ground_truth and self.measured_table is None:
            raise ValueError("PathArrayRenderer evaluates the ground truth on the lane-ordered wavefront (fused_ground_truth=True)")
        self.max_depth, self.occlusion = max_depth, occlusion
        self.stats = {"lanes_per_bounce": []}

    def _buffers(self, n: int):
        b = super()._buffers(n)
        if "org" not in b:
            for name in ("org", "beta", "rad"):
                b[name] = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        return b

    # -- the three path kernels ----------------------------------------------------------------------
    def path_begin(self, b):
        """org, beta, rad of the first vertices from what ``primary`` wrote into ``b``."""
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_wf_path_begin(C.byref(self.scene), p(self.env), b["mat"].shape[0], p(b["dir"]),
                                                      p(b["nrm"]), p(b["mat"]), p(b["org"]), p(b["beta"]), p(b["rad"]),
                                                      self._stream()))

    def bounce(self, b, bounce: int, last: bool, seed: int, pass_idx: int, path_offset: int, occlusion: Optional[bool] = None):
        """Shade the vertices in ``b`` (``wo``, ``pdf_o``, ``pdf_l`` [, ``f_o``, ``f_l``] from the sampler) and move the paths on."""
        p = lambda t: C.c_void_p(t.data_ptr())
        occlusion = self.occlusion if occlusion is None else occlusion
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_wf_bounce(
                C.byref(self.scene), p(self.env), bounce, int(bool(last)), int(bool(occlusion)), seed, pass_idx, path_offset,
                b["mat"].shape[0], p(b["org"]), p(b["nrm"]), p(b["wi"]), p(b["wl"]), p(b["mat"]), p(b["beta"]), p(b["rad"]),
                p(b["wo"]), p(b["pdf_o"]), p(b["pdf_l"]), p(b["f_o"]) if "f_o" in b else None,
                p(b["f_l"]) if "f_l" in b else None, self._stream()))
        # written through raw pointers: tell torch (the plugin cores key their per-query context cache on wi._version)
        torch.autograd.graph.increment_version([b["wi"], b["wl"], b["nrm"], b["org"], b["mat"], b["beta"], b["rad"]])

    def resolve(self, row_begin: int, row_end: int, spp: int, b, film: torch.Tensor):
        """film [row_end-row_begin, width, 3] += the pass' estimate."""
        if film.shape != (row_end - row_begin, self.camera.width, 3) or film.dtype != torch.float32 \
                or not film.is_contiguous() or film.device != self.device:
            raise ValueError("film must be a contiguous fp32 [rows, width, 3] tensor on the renderer's device")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_wf_resolve(C.byref(self.scene), row_begin, row_end, spp, C.c_void_p(b["rad"].data_ptr()),
                                                   C.c_void_p(film.data_ptr()), self._stream()))

    # -- one pass over a tile ------------------------------------------------------------------------
    def render_pass(self, film: torch.Tensor, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int,
                    x0: Optional[torch.Tensor] = None):
        n = (row_end - row_begin) * self.camera.width * spp
        if n == 0:
            return
        from .materials import WavefrontPipeline
        b = self.primary(row_begin, row_end, spp, seed, pass_idx)
        self.path_begin(b)
        offset = row_begin * self.camera.width * spp
        skey = (seed * 0x9E3779B97F4A7C15 + pass_idx + 1) & _M64
        n_balls = len(self.table)
        lanes = []
        for k in range(self.max_depth):
            plan = self.table.bucket(b["mat"], extra_bins=2)      # floor vertices and ended paths behind the materials
            counts = plan[1]                                      # (already on the host)
            n_mat = sum(counts[:n_balls])
            if n_mat + counts[n_balls] == 0:
                break
            lanes.append(n_mat)
            if n_mat:
                key = skey if k == 0 else skey ^ ((k * 0xD1B54A32D192ED03) & _M64)
                b["wo"], b["pdf_o"], b["pdf_l"] = self.table.sample_pdf(plan, b["wi"], b["wl"], seed=key, offset=offset,
                                                                        direct=n <= WavefrontPipeline.DIRECT_MAX_LANES)
                if self.use_ground_truth:
                    self.measured_table.eval_t(b["mat"], b["wi"], b["wo"], b["wl"], tint=self.plugin.albedo, out_o=b["f_o"],
                                               out_l=b["f_l"])
            # (no material lane: only floor vertices are left, which read neither the sampler's nor the evaluator's arrays)
            self.bounce(b, k, k == self.max_depth - 1, seed, pass_idx, offset)
        self.stats["lanes_per_bounce"] = lanes
        self.resolve(row_begin, row_end, spp, b, film)
