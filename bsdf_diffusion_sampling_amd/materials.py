"""Mixed-material batches (BASELINE.json configs[3]: "all paper measured BSDFs, mixed queries").

The reference binds one plugin instance per material and Mitsuba dispatches each wavefront
lane to its instance (one `sample()` call per material per bounce,
rendering/matpreview/disney_bsdf_array0_envmap.xml: 12 `mybsdf` instances).  Here a
``MaterialTable`` holds one packed device handle per material and serves a batch whose
queries carry a material id: queries are bucketed (stable sort by id) and results are
scattered back to the callers' order.  All disk nets together are ~160 KB of fp16 fragments
— the whole LDS — so keeping every material resident in every workgroup is not an option
(SURVEY.md §7 "mixed-material batches").  Instead ONE segmented launch
(the ``bsdfd_plugin_*_multi_ex`` entry points) serves all buckets whose handles share a kernel signature
(domain, width, depth, precision; up to 64 per launch): workgroups are dealt to the buckets
in proportion to their sizes and each loads only its own material's 16 KB image.  The 52
measured materials are 2 launches (27 disk + 25 spherical) instead of 52.
``segmented=False`` falls back to one launch per bucket (used by the tests as the
reference for the segmented path).
"""
from __future__ import annotations

import ctypes as C
from itertools import accumulate
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import weights as W
from .sampler import FlowSampler
from .sharding import bucket_by_material


class MaterialTable:
    def __init__(self, stems: Sequence[str], precision: str = "default", tile: int = 0):
        """``stems`` are shipped weight-set names such as ``aniso_miro_7_rgb_disk`` or
        ``chm_orange_rgb_spherical`` (mixing domains is allowed: the domain, T and plugin
        variant are per material).  ``tile``: bsdfd_desc.tile for every material (0 = library default)."""
        self.stems = list(stems)
        self.samplers: List[FlowSampler] = []
        self.T: List[int] = []
        self.variant: List[int] = []
        for stem in self.stems:
            fw = W.load(W.shipped_path(*self._split(stem)))
            self.samplers.append(FlowSampler(fw, precision=precision, tile=tile))
            disk = fw.domain == W.DOMAIN_DISK
            self.T.append(4 if disk else 8)  # plugin defaults, brdf_measured_disk.py:68 / _spherical.py:78
            self.variant.append(_lib.PLUGIN_FULLSPHERE if stem.startswith("bsdf_") else _lib.PLUGIN_MEASURED)

    @staticmethod
    def _split(stem: str) -> Tuple[str, str]:
        for dom in ("disk", "spherical"):
            if stem.endswith("_" + dom):
                return stem[: -len(dom) - 1], dom
        raise ValueError(f"cannot parse weight-set name {stem!r}")

    @classmethod
    def all_measured(cls, precision: str = "default") -> "MaterialTable":
        """27 disk + 25 spherical measured materials (config 4)."""
        stems = W.list_shipped("disk") + [s for s in W.list_shipped("spherical")
                                          if not s.startswith("bsdf_") and not s.endswith("_complex")]
        return cls([s for s in stems if not s.endswith("_complex")], precision)

    def __len__(self):
        return len(self.samplers)

    def _groups(self):
        """Indices of materials grouped by kernel signature + plugin defaults (T, variant)."""
        groups = {}
        for m, s in enumerate(self.samplers):
            fw = s.weights
            key = (fw.domain, fw.width, fw.n_hidden, s.precision, self.T[m], self.variant[m])
            groups.setdefault(key, []).append(m)
        return groups

    def _multi(self, which, members, seg_end_all, T, variant, ins, outs, seed, offset, ctx=None,
               gkey=None, rng_rows=None, ctx_fill=None, direct_rows=None):
        """``ins`` / ``outs``: the arrays of the call as ``FlowSampler.plugin_<which>`` takes and returns them — (wi, x0 or None) ->
        (wo, pdf), (wi, wo) -> (pdf,), (wi, wl, x0 or None) -> (wo, pdf(wo), pdf(wl)).

        ``direct_rows`` (int64 [n_mat], the bucket permutation): the arrays are the CALLERS' lane-ordered ones and every launch
        reads and writes its rows through ``bsdfd_opts.row_index`` — no gathered copy, no scatter (``direct=True`` of the public
        calls).  The Philox counter is then ``offset + original lane`` by construction.

        ``ctx`` (a dict, or None): per-query contexts (include/bsdfd.h, bsdfd_context_bytes) of the runs of this
        wavefront — the FILLING call (``ctx_fill``; default: "sample" fills, "pdf" reads) writes one buffer per (kernel
        signature, run), the other call on the same bucketed ``wi`` reads them instead of recomputing the per-query prologue.
        The dict keeps ONE buffer per (kernel signature, run number), grown to the largest wavefront seen, together with the
        bucket layout it was last filled for; a reading call whose layout differs is refused.

        Segmented launch(es) for the materials `members` of one kernel signature.  The bucketed arrays
        are ordered by material id, so a group's buckets may be interleaved with other groups'; each
        maximal run of ADJACENT buckets becomes one segmented call on the run's row range."""
        L = _lib.lib()
        rc = 0
        stream = C.c_void_p(torch.cuda.current_stream(ins[0].device).cuda_stream)
        # the C ABI takes cumulative ends; non-adjacent buckets are issued as separate runs
        run_h, run_end, base = [], [], None
        run_no = 0
        fill = (which == "sample") if ctx_fill is None else bool(ctx_fill)
        def flush():
            nonlocal run_h, run_end, base, run_no
            if not run_h:
                return 0
            k = len(run_h)
            arr_h = (C.c_void_p * k)(*run_h)
            arr_e = (C.c_int64 * k)(*[e - base for e in run_end])
            cbuf = None
            if ctx is not None and which in ("sample", "pdf"):
                ckey, layout = (gkey, run_no), (base, tuple(run_end))
                run_no += 1
                ent = ctx.get(ckey)
                if fill:
                    nbytes = int(L.bsdfd_context_bytes(run_h[0], run_end[-1] - base, k))
                    if ent is None or ent["buf"].numel() * 4 < nbytes or ent["buf"].device != ins[0].device:
                        ent = ctx[ckey] = {"buf": torch.empty((nbytes // 4,), dtype=torch.float32, device=ins[0].device)}
                    ent["layout"] = layout
                elif ent is None or ent.get("layout") != layout:
                    raise ValueError("a context-reading call needs the context a filling call of the SAME bucketed wavefront "
                                     "(same plan, same wi array) wrote: sample(ctx=) before pdf(ctx=), or pdf(ctx=, "
                                     "ctx_fill=True) before sample(ctx=, ctx_fill=False)")
                cbuf = ent["buf"]
            c_out, c_in = (cbuf, None) if fill else (None, cbuf)
            # Where a run starts: in the INDEX array (direct: the data pointers stay at row 0 of the lane-ordered arrays) or in the
            # bucketed arrays themselves (pointers advanced to the run's first row).  A lane index, supplied either way, carries
            # the Philox counter (offset + ORIGINAL lane); without one the counter is offset + row in the bucketed array.
            row0, off, o = base, offset, None
            if direct_rows is not None:
                row0, o = 0, _lib.opts(ctx_out=c_out, ctx_in=c_in, row_index=direct_rows, byte_offset_row=base * 8)
            elif cbuf is not None or rng_rows is not None:
                o = _lib.opts(ctx_out=c_out, ctx_in=c_in, rng_index=rng_rows, byte_offset_rng=base * 8)
            if direct_rows is None and rng_rows is None:
                off = offset + base
            o = None if o is None else C.byref(o)

            def at(t, row_bytes):
                return None if t is None else C.c_void_p(t.data_ptr() + row0 * row_bytes)
            if which == "sample":
                r = L.bsdfd_plugin_sample_multi_ex(arr_h, k, arr_e, variant, at(ins[0], 12), at(ins[1], 8), seed, off, T,
                                                   at(outs[0], 12), at(outs[1], 4), o, stream)
            elif which == "pdf":
                r = L.bsdfd_plugin_pdf_multi_ex(arr_h, k, arr_e, variant, at(ins[0], 12), at(ins[1], 12), T, at(outs[0], 4), o, stream)
            else:
                r = L.bsdfd_plugin_sample_pdf_multi_ex(arr_h, k, arr_e, variant, at(ins[0], 12), at(ins[2], 8), at(ins[1], 12), seed,
                                                       off, T, at(outs[0], 12), at(outs[1], 4), at(outs[2], 4), o, stream)
            run_h, run_end, base = [], [], None
            return r
        prev_end = None
        for m in members:
            b, e = seg_end_all[m - 1] if m else 0, seg_end_all[m]
            if prev_end is not None and b != prev_end:
                rc = rc or flush()
            if base is None:
                base = b
            run_h.append(self.samplers[m]._h)
            run_end.append(e)
            prev_end = e
        rc = rc or flush()
        _lib.check(rc)

    def _buckets(self, material_id, extra_bins: int = 0):
        if isinstance(material_id, tuple):  # a plan from bucket(): (perm, counts)
            perm, counts = material_id
            if (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or perm.dim() != 1
                    or len(counts) < len(self) or sum(counts) != perm.shape[0] or min(counts, default=0) < 0):
                raise ValueError("not a bucketing plan of this table: expected (perm int64 [N], counts) from bucket()")
            return perm, list(counts)
        if material_id.dtype != torch.int64:
            material_id = material_id.long()
        perm, counts = bucket_by_material(material_id, len(self) + extra_bins)
        counts = counts.cpu().tolist()
        if sum(counts) != material_id.shape[0]:
            raise ValueError(f"material ids must be in [0, {len(self) + extra_bins})")
        return perm, counts

    def _plan(self, material_id, n_rows: Optional[int] = None):
        """(rows, counts, seg_end): `rows` = the bucketed order of the lanes that carry a material (lanes of the
        plan's extra bins sort behind them and are not evaluated), `counts` per material.  ``n_rows``: the rows of the
        lane-ordered batch the plan must cover; None for arrays that are in bucket order already, which only a plan describes."""
        if n_rows is None and not isinstance(material_id, tuple):
            raise ValueError("bucketed=True needs a plan from bucket()")
        perm, counts = self._buckets(material_id)
        if n_rows is not None and perm.shape[0] != n_rows:
            raise ValueError(f"the bucketing plan covers {perm.shape[0]} rows, the batch has {n_rows}")
        counts = counts[: len(self)]
        n_mat = sum(counts)
        return perm if n_mat == perm.shape[0] else perm[:n_mat], counts, list(accumulate(counts))

    def _chk_in(self, t, cols, name, n=None):
        return self.samplers[0]._chk(t, cols, name, n)

    # -- bucketed flow: a renderer keeps a wavefront in bucket order across its sample() and pdf() calls and scatters
    # once at the end, instead of gathering the inputs and scattering the outputs in every call -----------------------
    def gather(self, plan, *tensors):
        """Rows of the lanes that carry a material, in bucket order (what ``bucketed=True`` calls take and return).
        A single fp32 [N,3] array (the wavefront's ``wi``) goes through the native one-pass kernel."""
        rows, _, _ = self._plan(plan)
        if (len(tensors) == 1 and tensors[0].is_cuda and tensors[0].dtype == torch.float32 and tensors[0].dim() == 2
                and tensors[0].shape[1] == 3 and tensors[0].is_contiguous() and rows.is_contiguous()):
            wi = tensors[0]
            out = torch.empty((rows.shape[0], 3), dtype=torch.float32, device=wi.device)
            with torch.cuda.device(wi.device):
                _lib.check(_lib.lib().bsdfd_gather_lanes(C.c_void_p(rows.data_ptr()), rows.shape[0], C.c_void_p(wi.data_ptr()),
                                                         C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream(wi.device).cuda_stream)))
            return out
        out = tuple(t[rows].contiguous() for t in tensors)
        return out[0] if len(out) == 1 else out

    def scatter(self, plan, *tensors):
        """Inverse of ``gather``: bucket-ordered results back to the callers' lane order (lanes without a material: 0).
        The usual triple of a wavefront — (wo [n,3], pdf [n], pdf [n]) or (wo, pdf) — is written in ONE native pass."""
        perm, _ = plan
        rows, _, _ = self._plan(plan)
        n, k = perm.shape[0], rows.shape[0]
        mk = torch.empty if k == n else torch.zeros

        def f32c(t, *shape):
            return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        if (len(tensors) in (2, 3) and f32c(tensors[0], k, 3) and all(f32c(t, k) for t in tensors[1:]) and rows.is_contiguous()):
            dev = tensors[0].device
            full = [mk((n, 3), dtype=torch.float32, device=dev)] + [mk((n,), dtype=torch.float32, device=dev) for _ in tensors[1:]]
            p = [C.c_void_p(t.data_ptr()) for t in tensors] + [None] * (3 - len(tensors))
            q = [C.c_void_p(t.data_ptr()) for t in full] + [None] * (3 - len(tensors))
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().bsdfd_scatter_lanes(C.c_void_p(rows.data_ptr()), k, p[0], p[1], p[2], q[0], q[1], q[2],
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            return tuple(full)
        out = []
        for t in tensors:
            full = mk((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            full[rows] = t
            out.append(full)
        return out[0] if len(out) == 1 else tuple(out)

    def bucket(self, material_id: torch.Tensor, extra_bins: int = 0):
        """Bucket a wavefront once and reuse the plan for its sample() and pdf() calls (a renderer asks both
        for the same intersections): pass the returned value in place of ``material_id``.  The stable sort
        of 16 Mi ids costs 0.2 ms natively (1.7 ms with torch.argsort).  ``extra_bins``: ids len(self) ..
        len(self)+extra_bins-1 are lanes that carry no material (a renderer's floor hits and misses); they
        sort behind the materials, are not evaluated, and their outputs are zero."""
        return self._buckets(material_id, extra_bins)

    def bucket_rows(self, material_id: torch.Tensor, rows: torch.Tensor, extra_bins: int = 0):
        """``bucket`` over a list of lanes: (perm, counts) of the lanes ``rows`` (int64 [n_rows], distinct, in [0, N)) by
        ``material_id[rows]``, ``perm`` holding LANE numbers, bucket by bucket, stable in list order, cut to the kept lanes: a lane
        whose id is outside [0, len(self) + extra_bins) is left out (a path tracer's ended paths), so ``perm`` is the next list.
        As a plan it serves ``sample_pdf(..., direct=True, out=)``.  Native only (``bsdfd_bucket_rows``): at most 64 ids."""
        n_ids = len(self) + extra_bins
        if n_ids > 64:
            raise ValueError(f"bucket_rows sorts at most 64 ids natively, got {n_ids}")
        for name, t in (("material_id", material_id), ("rows", rows)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 1 and t.is_cuda and t.is_contiguous()):
                raise ValueError(f"bucket_rows: {name} must be a contiguous int64 CUDA tensor [N]")
        if rows.device != material_id.device or rows.shape[0] > material_id.shape[0]:
            raise ValueError("bucket_rows: rows must be on the device of material_id and no longer than it")
        L, dev, n = _lib.lib(), material_id.device, rows.shape[0]
        perm = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(n_ids, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(L.bsdfd_bucket_workspace_bytes(n, n_ids)), 1), dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(L.bsdfd_bucket_rows(p(material_id), p(rows), n, n_ids, p(perm), p(counts), p(ws), ws.numel(),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        counts = counts.cpu().tolist()
        return perm[: sum(counts)], counts

    def _serve(self, which, material_id, ins, seed=0, offset=0, T=None, segmented=True, form="gathered", rng="lane",
               ctx=None, ctx_fill=None, out=None):
        """The skeleton of sample() / pdf() / sample_pdf(): ``ins`` (``wi`` first, in the order ``FlowSampler.plugin_<which>`` takes
        them) -> (results, (bucket-ordered inputs, bucket-ordered results, rows, seg_end)).  ``form``: how the launches see the
        arrays — "gathered": bucket-ordered copies, the results scattered back to lane order; "bucketed": the arrays are in
        bucket order already and the results stay in it; "direct": the lane-ordered arrays themselves, read and written through
        the bucket permutation.  ``out`` (direct only): the lane-ordered result arrays to write into, with no fill — the plan may
        then cover fewer rows than ``wi`` has (``bucket_rows``), and rows it does not list keep what they held."""
        if ctx is not None and not segmented:
            raise ValueError("ctx= is a feature of the segmented path (segmented=False issues one plain call per bucket)")
        if rng not in ("lane", "bucketed"):
            raise ValueError("rng must be 'lane' or 'bucketed'")
        wi = ins[0]
        n, dev = wi.shape[0], wi.device
        rows, counts, seg_end = self._plan(material_id, None if form == "bucketed" or out is not None else n)
        if form == "bucketed" and n != rows.shape[0]:
            raise ValueError(f"bucketed wi has {n} rows, the plan has {rows.shape[0]} material lanes")
        rows = rows.contiguous()
        direct, full = form == "direct", rows.shape[0] == n   # (not full: lanes without a material, their results are zeros)
        ins_s = tuple(None if t is None else t[rows].contiguous() for t in ins) if form == "gathered" else tuple(ins)

        def new(mk, k):
            return tuple(mk((k, 3) if cols == 3 else (k,), dtype=torch.float32, device=dev)
                         for cols in {"sample": (3, 1), "pdf": (1,), "sample_pdf": (3, 1, 1)}[which])
        outs_s = tuple(out) if out is not None else new(torch.zeros if direct and not full else torch.empty, ins_s[0].shape[0])
        # the Philox counter of a row: offset + its ORIGINAL lane (what the direct form draws by construction), or + its bucketed row
        rng_rows = rows if rng == "lane" and which != "pdf" and not direct else None
        with torch.cuda.device(dev):
            if segmented:
                for (dom, w, nh, prec, Tm, var), members in self._groups().items():
                    self._multi(which, members, seg_end, Tm if T is None else T, var, ins_s, outs_s, seed, offset, ctx=ctx,
                                gkey=(dom, w, nh, prec, var), rng_rows=rng_rows, ctx_fill=ctx_fill,
                                direct_rows=rows if direct else None)
            else:   # one call per bucket, same Philox keying as the segmented path
                lo = 0
                for m, c in enumerate(counts):
                    if c == 0:
                        continue
                    sl = slice(lo, lo + c)
                    if direct:
                        a, o, kw = ins_s, outs_s, dict(row_index=rows[sl])
                    else:
                        a, o, kw = [None if t is None else t[sl] for t in ins_s], tuple(t[sl] for t in outs_s), {}
                    if which != "pdf":
                        kw.update(seed=seed, offset=offset if direct or rng_rows is not None else offset + lo,
                                  rng_index=None if rng_rows is None else rng_rows[sl])
                    getattr(self.samplers[m], "plugin_" + which)(*a, T=self.T[m] if T is None else T, variant=self.variant[m],
                                                                 out=o[0] if which == "pdf" else o, **kw)
                    lo += c
        outs = outs_s
        if form == "gathered":
            outs = new(torch.empty if full else torch.zeros, n)
            for t, t_s in zip(outs, outs_s):
                t[rows] = t_s
        return outs, (ins_s, outs_s, rows, seg_end)

    def sample(self, material_id: torch.Tensor, wi: torch.Tensor, seed: int = 0, offset: int = 0,
               T: Optional[int] = None, x0: Optional[torch.Tensor] = None, segmented: bool = True,
               bucketed: bool = False, ctx: Optional[dict] = None, rng: str = "lane", ctx_fill: bool = True,
               direct: bool = False):
        """wi [N,3], material_id [N] -> (wo [N,3], pdf_sa [N]) in the callers' order.
        ``rng``: ``"lane"`` (default) — the Philox counter of a query is ``offset + its ORIGINAL lane index``, so the base
        draws depend on neither the bucketing nor how the wavefront is sharded over calls / GPUs (a shard passes its
        first lane's global index as ``offset``); ``"bucketed"`` — ``offset + row in the bucketed
        array`` (what a caller that keeps no lane order would use).
        ``ctx``: a dict this call fills with the wavefront's per-query contexts; hand the same dict (and the same
        plan and ``wi``) to ``pdf(..., ctx=)`` and it skips the per-query prologue (identical results).  The other order
        works too: ``pdf(..., ctx=d, ctx_fill=True)`` first, then ``sample(..., ctx=d, ctx_fill=False)``.  Segmented path only.
        Identical for the segmented and the per-bucket path.  ``bucketed=True``: ``material_id`` is a
        plan, ``wi`` / ``x0`` are already in bucket order (``gather(plan, wi)``) and the results stay in it.
        ``direct=True``: no gathered copies at all — the launches read ``wi`` / ``x0`` and write the results in the callers' lane
        order THROUGH the bucket permutation (``bsdfd_opts.row_index``); same results bit for bit (``rng="lane"`` only)."""
        wi = self._chk_in(wi, 3, "wi")
        x0 = self._chk_in(x0, 2, "x0", wi.shape[0])
        if direct and (bucketed or rng != "lane"):
            raise ValueError("direct=True takes lane-ordered arrays and draws with rng='lane'")
        return self._serve("sample", material_id, (wi, x0), seed, offset, T, segmented,
                           "direct" if direct else "bucketed" if bucketed else "gathered", rng, ctx, ctx_fill)[0]

    def sample_pdf(self, material_id, wi: torch.Tensor, wl: torch.Tensor, seed: int = 0, offset: int = 0,
                   T: Optional[int] = None, x0: Optional[torch.Tensor] = None, return_bucketed: bool = False,
                   rng: str = "lane", direct: bool = False, out=None):
        """sample(wi) and pdf(wi, wl) for the same material-tagged intersections, one launch per kernel
        signature -> (wo [N,3], pdf(wo) [N], pdf(wl) [N]) in the callers' order.
        ``out`` = (wo, pdf_o, pdf_l), with ``direct=True``: the results are written into these lane-ordered arrays, which are
        returned, and nothing N rows long is allocated or filled.  The plan may then cover fewer rows than ``wi`` has (a plan of
        ``bucket_rows``): only its material rows are written, every other row keeps what it held.  Without ``out`` a plan that
        does not cover the batch is refused."""
        wi = self._chk_in(wi, 3, "wi")
        wl = self._chk_in(wl, 3, "wl", wi.shape[0])
        x0 = self._chk_in(x0, 2, "x0", wi.shape[0])
        if direct and (return_bucketed or rng != "lane"):
            raise ValueError("direct=True returns lane-ordered arrays only and draws with rng='lane'")
        if out is not None:
            if not direct:
                raise ValueError("out= is written through the bucket permutation: it needs direct=True")
            if len(out) != 3:
                raise ValueError("out is a (wo [N,3], pdf_o [N], pdf_l [N]) triple")
            if out[0] is None:
                raise ValueError("out[0] (wo) is missing")
            out = (self._chk_in(out[0], 3, "out[0]", wi.shape[0]),) + tuple(self.samplers[0]._chk1(t, wi.shape[0], f"out[{k + 1}]")
                                                                          for k, t in enumerate(out[1:]))
        outs, (ins_s, outs_s, rows, seg_end) = self._serve("sample_pdf", material_id, (wi, wl, x0), seed, offset, T,
                                                           form="direct" if direct else "gathered", rng=rng, out=out)
        if return_bucketed:  # the bucket-ordered arrays too (material m = rows seg_end[m-1] .. seg_end[m]) and `rows`
            return outs + (dict(wi=ins_s[0], wl=ins_s[1], wo=outs_s[0], pdf_o=outs_s[1], pdf_l=outs_s[2], rows=rows,
                                seg_end=seg_end),)
        return outs

    def pdf(self, material_id: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, T: Optional[int] = None,
            segmented: bool = True, bucketed: bool = False, ctx: Optional[dict] = None, ctx_fill: bool = False,
            direct: bool = False):
        wi = self._chk_in(wi, 3, "wi")
        wo = self._chk_in(wo, 3, "wo", wi.shape[0])
        if direct and bucketed:
            raise ValueError("direct=True takes lane-ordered arrays")
        return self._serve("pdf", material_id, (wi, wo), T=T, segmented=segmented,
                           form="direct" if direct else "bucketed" if bucketed else "gathered", ctx=ctx, ctx_fill=ctx_fill)[0][0]


class _Wavefront:
    """One wavefront in flight through a ``WavefrontPipeline``: ``result()`` orders the calling stream behind its scatter
    and returns (wo [N,3], pdf(wo) by sample() [N], pdf(wo) by pdf() [N]) in the callers' lane order."""

    def __init__(self):
        self.plan = self.wi_b = self.bucketed = self.out = None
        self.prep_done = self.flow_done = self.scatter_done = None

    def result(self):
        cur = torch.cuda.current_stream(self.out[0].device)
        cur.wait_event(self.scatter_done)
        for t in self.out:
            t.record_stream(cur)
        return self.out


class WavefrontPipeline:
    """sample() + pdf() of a STREAM of independent material-tagged wavefronts (the passes of a render, the tiles of a film),
    software-pipelined over three HIP streams: the bucketing + gather of wavefront k run on a side stream under the flow
    kernels of wavefront k-1 (the host's wait for the bucket counts included), its scatter on another under the flow
    kernels of wavefront k+1.  The flow kernels — the only compute-bound part — then run back to back on the calling
    stream; the streaming passes around them use the HBM bandwidth the flow kernels leave idle.  Results are those of
    ``bucket -> gather -> sample(bucketed) -> pdf(bucketed) -> scatter`` issued one after the other, bit for bit.

    ``push()`` returns a ``_Wavefront``; at most two are in flight: the buffers of wavefront k are reused by wavefront k+2,
    so take ``result()`` of a wavefront before pushing the second one after it."""

    # Largest wavefront (lanes) served through the bucket permutation when ``direct`` is left to the pipeline.  Measured, 52 materials,
    # steady state, alternating (profiles/r06_ab/mixed_row_index_vs_gather_by_size.jsonl): wall time of the direct form over the
    # gather form 0.92 (256 Ki lanes), 0.97 (1 Mi), 1.00 (2 Mi), 0.93 (4 Mi), 0.95 (8 Mi), 1.05 (16 Mi).  Why it turns: a row-indexed
    # 12-byte access touches a whole line that ~10 tiles of OTHER buckets touch at other times; while the lane-ordered arrays sit in
    # the 256 MiB Infinity Cache that is free, beyond it every touch is an HBM access — at 16 Mi lanes the direct form moves 8.7 GB
    # per wavefront on the HBM side against 6.1 GB (1.07 GB algorithmic; rocprofv3 FETCH_SIZE / WRITE_SIZE,
    # profiles/r06_ab/mixed_16Mi_row_index_vs_gather_pmc.json): it reads wi through the index twice and writes AND re-reads wo through
    # it, the gather form pays each amplified pass once.
    DIRECT_MAX_LANES = 8 << 20

    def __init__(self, table: MaterialTable, direct: Optional[bool] = None):
        """``direct``: the flow kernels read ``wi`` and write the results in lane order through the bucket permutation
        (``bsdfd_opts.row_index``, round 6) — only the bucketing itself (count, scan, permutation) is left on the side stream, the
        gather of ``wi`` and the scatter of (wo, pdf, pdf) are gone.  ``False``: the round-4 form (gather on the side stream,
        bucket-ordered launches, scatter on a third stream).  ``None`` (default): by wavefront size — direct up to
        ``DIRECT_MAX_LANES`` lanes, the gather form beyond.  Identical results either way, bit for bit."""
        self.tab = table
        self.direct = direct
        self.pre = self.post = None
        self.slots = [_Wavefront(), _Wavefront()]
        self.k = 0

    def push(self, material_id: torch.Tensor, wi: torch.Tensor, seed: int = 0, offset: int = 0,
             ctx: Optional[dict] = None, extra_bins: int = 0, ready=None) -> _Wavefront:
        """``material_id`` / ``wi`` are read on a side stream.  ``ready`` orders that stream behind their producer:

        * ``None`` (default, always safe): an event recorded NOW on the calling stream — whatever the caller enqueued there to
          produce the inputs is waited for.  It is also ordered behind the previous wavefronts' flow kernels on that stream,
          so a caller that produces its inputs on the calling stream gets no overlap of the bucketing with them;
        * a ``torch.cuda.Event`` the producer recorded right behind its last write (e.g. on its own stream): full overlap;
        * ``False``: the inputs are complete already (resident arrays, a host-synchronised producer): no wait at all."""
        tab, dev = self.tab, wi.device
        direct = self.direct if self.direct is not None else wi.shape[0] <= self.DIRECT_MAX_LANES
        main = torch.cuda.current_stream(dev)
        if self.pre is None or self.pre.device != dev:
            self.pre, self.post = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        w = self.slots[self.k % 2]
        self.k += 1
        if ready is None:
            ready = main.record_event()
        with torch.cuda.stream(self.pre):
            if ready is not False:
                self.pre.wait_event(ready)
            if w.flow_done is not None:
                self.pre.wait_event(w.flow_done)       # the flow kernels of wavefront k-2 have read the buffers reused here
            plan = tab.bucket(material_id, extra_bins)  # (the host waits for the counts on THIS stream only)
            wi_b = None if direct else tab.gather(plan, wi)
            for t in (plan[0], wi_b):
                if t is not None:
                    t.record_stream(main)
            w.plan, w.wi_b = plan, wi_b
            w.prep_done = self.pre.record_event()
        main.wait_event(w.prep_done)
        if direct:
            if w.scatter_done is not None:
                main.wait_event(w.scatter_done)   # (a slot last used by the gather form: its scatter reads the slot's buffers)
            wo, pdf = tab.sample(plan, wi, seed=seed, offset=offset, ctx=ctx, direct=True)
            p2 = tab.pdf(plan, wi, wo, ctx=ctx, direct=True)
            w.bucketed = None
            w.out = (wo, pdf, p2)
            w.flow_done = w.scatter_done = main.record_event()
            return w
        if w.scatter_done is not None:
            main.wait_event(w.scatter_done)
        wo_b, pdf_b = tab.sample(plan, wi_b, seed=seed, offset=offset, bucketed=True, ctx=ctx)
        p_b = tab.pdf(plan, wi_b, wo_b, bucketed=True, ctx=ctx)
        for t in (wo_b, pdf_b, p_b, plan[0]):
            t.record_stream(self.post)
        w.bucketed = (wo_b, pdf_b, p_b)
        w.flow_done = main.record_event()
        with torch.cuda.stream(self.post):
            self.post.wait_event(w.flow_done)
            w.out = tab.scatter(plan, wo_b, pdf_b, p_b)
            w.scatter_done = self.post.record_event()
        return w
