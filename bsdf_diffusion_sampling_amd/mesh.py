"""Triangle meshes for the array scenes: the reference renders ``matpreview.serialized`` (a plane, an interior and a shell),
instanced 25 times per ``disney_bsdf_array*.xml``; this module reads that container, builds the scene the native ray caster walks
(csrc/mesh.hip: a threaded BVH per mesh, instances under affine transforms, ``bsdfd_mesh_intersect`` / ``_occluded`` /
``_primary``) and renders it through ``ArrayRenderer``'s own pipeline (``MeshArrayRenderer``: only ``primary()`` differs) or
through ``PathArrayRenderer``'s (``MeshPathArrayRenderer``: shadows, interreflection, point lights and Russian roulette, with
``bsdfd_mesh_path_primary`` / ``_sample_emitter`` / ``_bounce`` in the place of the sphere kernels).

Limits of the path tracer on meshes: no geometric-normal test — a BSDF sample above the shading normal but below the triangle's
plane enters the shell and is followed there; the shell's inside is shaded like its outside; no transmission and no importance
sampling of the environment on meshes yet.  ``CompactMeshPathArrayRenderer`` is the same renderer with the bounces behind the first
on a live-lane list (``bsdfd_mesh_sample_emitter_rows`` / ``bsdfd_mesh_bounce_rows``): the same film bit for bit.  Like everything at this level it is PARITY-UNPINNED against
Mitsuba: image handedness, which checker colour lands on which cell and the v0.5-to-v3 scene upgrade rules are this module's
reading of the files, not a comparison with Mitsuba's images.

There is no CPU fallback for the rays: every one goes through libbsdfd.so.  The reader, the XML parser and the BVH builder
(``bsdfd_mesh_bvh_build``, pure host code) need no device.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import struct
import zlib
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .pathtrace import PathArrayRenderer, _Geometry, _p
from .wavefront import ArrayRenderer

FLAG_NORMALS, FLAG_UV, FLAG_COLORS, FLAG_DOUBLE = 0x1, 0x2, 0x8, 0x2000   # the flags word of a serialized shape
FILE_MAGIC = 0x041C
NOTHING = 3.0e38                                                          # t of a miss (wf_dev::Hit's "nothing")
NODE_DTYPE = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("skip", np.int32), ("tris", np.int32)])   # bsdfd_mesh_node
# z-up (the reference's scenes) -> y-up (this project's sky and camera): (x, y, z) -> (x, z, -y), as wavefront.ARRAY0_LAYOUT
TO_Y_UP = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


class TriMesh:
    """Positions [nv,3] fp32, indices [nt,3] uint32 and optional vertex normals [nv,3] / uv [nv,2]: plain numpy.  Refuses
    out-of-range indices and non-finite vertices."""

    def __init__(self, positions, indices, normals=None, uvs=None, name: str = ""):
        self.positions = np.ascontiguousarray(positions, dtype=np.float32)
        idx = np.asarray(indices)
        if self.positions.ndim != 2 or self.positions.shape[1] != 3 or self.positions.shape[0] < 1:
            raise ValueError("positions must be [nv,3] with nv >= 1")
        if idx.ndim != 2 or idx.shape[1] != 3 or idx.shape[0] < 1:
            raise ValueError("indices must be [nt,3] with nt >= 1")
        if not np.isfinite(self.positions).all():
            raise ValueError("non-finite vertex")
        if idx.min() < 0 or idx.max() >= self.positions.shape[0]:
            raise ValueError(f"vertex index out of range: {int(idx.min())} .. {int(idx.max())} with {self.positions.shape[0]} vertices")
        self.indices = np.ascontiguousarray(idx, dtype=np.uint32)
        nv = self.positions.shape[0]
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32)
        if self.normals is not None and self.normals.shape != (nv, 3):
            raise ValueError("normals must be [nv,3]")
        if self.uvs is not None and self.uvs.shape != (nv, 2):
            raise ValueError("uvs must be [nv,2]")
        self.name = name

    @property
    def n_vertices(self) -> int:
        return self.positions.shape[0]

    @property
    def n_triangles(self) -> int:
        return self.indices.shape[0]


def load_serialized(path: str):
    """The shapes of a Mitsuba ``.serialized`` container -> [TriMesh].  The trailer holds the shape count (last 4 bytes) behind
    one offset per shape (32-bit in version 3, 64-bit in version 4); every shape is a 0x041C header, the version and a zlib stream
    of: flags, [name, version 4 only], vertex and triangle counts, positions, [normals], [uv], [colours, skipped], uint32 indices."""
    data = open(path, "rb").read()
    if len(data) < 8:
        raise ValueError(f"{path}: too short for a serialized mesh file")
    magic, version = struct.unpack_from("<HH", data, 0)
    if magic != FILE_MAGIC or version not in (3, 4):
        raise ValueError(f"{path}: not a serialized mesh file (header {magic:#06x}, version {version})")
    count = struct.unpack_from("<I", data, len(data) - 4)[0]
    width = 8 if version == 4 else 4
    if count < 1 or 4 + count * width + 4 > len(data):
        raise ValueError(f"{path}: shape count {count} does not fit the file (truncated?)")
    offsets = struct.unpack_from("<" + str(count) + ("Q" if version == 4 else "I"), data, len(data) - 4 - count * width)
    return [_read_shape(path, data, int(off), k) for k, off in enumerate(offsets)]


def _read_shape(path, data, off, k):
    if off + 4 > len(data):
        raise ValueError(f"{path}: shape {k} starts behind the end of the file")
    magic, version = struct.unpack_from("<HH", data, off)
    if magic != FILE_MAGIC or version not in (3, 4):
        raise ValueError(f"{path}: shape {k} has header {magic:#06x}, version {version}")
    z = zlib.decompressobj()
    try:
        raw = z.decompress(data[off + 4:])
    except zlib.error as exc:
        raise ValueError(f"{path}: shape {k}: {exc}") from None
    if not z.eof:
        raise ValueError(f"{path}: shape {k}: the compressed stream is truncated")
    pos = 0

    def take(n):
        nonlocal pos
        if pos + n > len(raw):
            raise ValueError(f"{path}: shape {k}: the stream ends inside its arrays")
        pos += n
        return raw[pos - n:pos]

    flags = struct.unpack("<I", take(4))[0]
    name = ""
    if version == 4:
        end = raw.find(b"\0", pos)
        if end < 0:
            raise ValueError(f"{path}: shape {k}: unterminated name")
        name = take(end - pos + 1)[:-1].decode("utf-8", "replace")
    nv, nt = struct.unpack("<QQ", take(16))
    real = np.dtype("<f8" if flags & FLAG_DOUBLE else "<f4")

    def reals(cols):
        return np.frombuffer(take(nv * cols * real.itemsize), dtype=real).reshape(nv, cols).astype(np.float32)

    positions = reals(3)
    normals = reals(3) if flags & FLAG_NORMALS else None
    uvs = reals(2) if flags & FLAG_UV else None
    if flags & FLAG_COLORS:
        take(nv * 3 * real.itemsize)
    indices = np.frombuffer(take(nt * 12), dtype="<u4").reshape(nt, 3)
    try:
        return TriMesh(positions, indices, normals, uvs, name=name)
    except ValueError as exc:
        raise ValueError(f"{path}: shape {k}: {exc}") from None


def build_bvh(mesh: TriMesh):
    """``bsdfd_mesh_bvh_build`` on a TriMesh -> (nodes [n_nodes] of NODE_DTYPE, order int32 [nt]): the threaded BVH the scene
    uploads (depth-first, an inner node's left child is i + 1, ``skip`` the first node behind the subtree; a leaf has
    ``tris = first * 8 + count`` into the reordered triangles, ``order[first + k]`` the file's triangle index)."""
    nt = mesh.n_triangles
    nodes = np.zeros(2 * nt, dtype=NODE_DTYPE)
    order = np.zeros(nt, dtype=np.int32)
    n = C.c_int64()
    _lib.check(_lib.lib().bsdfd_mesh_bvh_build(mesh.positions.ctypes.data, mesh.n_vertices, mesh.indices.ctypes.data, nt,
                                               nodes.ctypes.data, nodes.shape[0], order.ctypes.data, C.byref(n)))
    return nodes[: n.value].copy(), order


def bvh_stats(nodes) -> dict:
    """nodes, leaves and depth (a lone leaf has depth 1) of a threaded BVH."""
    depth, stack = 0, []   # the skips of the open subtrees
    for i in range(nodes.shape[0]):
        while stack and stack[-1] <= i:
            stack.pop()
        stack.append(int(nodes["skip"][i]))
        depth = max(depth, len(stack))
    return {"nodes": int(nodes.shape[0]), "leaves": int((nodes["tris"] != 0).sum()), "depth": depth}


@dataclasses.dataclass
class Instance:
    """One instance: a mesh index, a 3x4 (or 4x4) affine ``to_world`` and ONE of ``material`` (a lane of the material table),
    ``diffuse`` (a constant reflectance) or ``checker`` = (color0, color1, uscale, vscale) over the mesh's own uv."""
    mesh: int
    to_world: Sequence
    material: Optional[int] = None
    diffuse: Optional[float] = None
    checker: Optional[Sequence[float]] = None

    def matrix(self) -> np.ndarray:
        m = np.asarray(self.to_world, dtype=np.float64)
        if m.shape == (4, 4):
            if not np.allclose(m[3], (0.0, 0.0, 0.0, 1.0)):
                raise ValueError("to_world must be affine")
            m = m[:3]
        if m.shape != (3, 4):
            raise ValueError("to_world must be 3x4 or 4x4")
        return m


class MeshScene:
    """Meshes and up to 64 instances of them.  The native scene (``bsdfd_mesh_scene_create``) is made on the first call that needs
    a device, once per device; everything else here is host data.  ``intersect`` / ``occluded`` / ``primary`` take and return
    torch tensors on the current device."""

    def __init__(self, meshes, instances):
        self.meshes = list(meshes)
        self.instances = list(instances)
        if not self.meshes or not all(isinstance(m, TriMesh) for m in self.meshes):
            raise ValueError("meshes: a non-empty list of TriMesh")
        if not 1 <= len(self.instances) <= _lib.MESH_MAX_INSTANCES:
            raise ValueError(f"1..{_lib.MESH_MAX_INSTANCES} instances")
        for k, inst in enumerate(self.instances):
            if not 0 <= inst.mesh < len(self.meshes):
                raise ValueError(f"instance {k}: mesh index out of range")
            if sum(v is not None for v in (inst.material, inst.diffuse, inst.checker)) != 1:
                raise ValueError(f"instance {k}: exactly one of material, diffuse, checker")
            if inst.material is not None and inst.material < 0:
                raise ValueError(f"instance {k}: negative material index")
            if inst.checker is not None and (len(inst.checker) != 4 or self.meshes[inst.mesh].uvs is None):
                raise ValueError(f"instance {k}: checker = (color0, color1, uscale, vscale) on a mesh with uv")
            m = inst.matrix()
            if not np.isfinite(m).all() or abs(np.linalg.det(m[:, :3])) <= 1e-12 * np.abs(m[:, :3]).max() ** 3:
                raise ValueError(f"instance {k}: singular to_world")
        self._handles = {}
        self._bvh = {}

    def __del__(self):
        for h in getattr(self, "_handles", {}).values():
            try:
                _lib.lib().bsdfd_mesh_scene_destroy(h)
            except Exception:
                pass

    @property
    def material_indices(self):
        return sorted({i.material for i in self.instances if i.material is not None})

    def bvh(self, k: int):
        if k not in self._bvh:
            self._bvh[k] = build_bvh(self.meshes[k])
        return self._bvh[k]

    @property
    def stats(self):
        """Per mesh: {"nodes", "leaves", "depth", "triangles"} of the BVH the library builds."""
        return [dict(bvh_stats(self.bvh(k)[0]), triangles=m.n_triangles) for k, m in enumerate(self.meshes)]

    def _records(self):
        descs = (_lib.MeshDesc * len(self.meshes))()
        for d, m in zip(descs, self.meshes):
            d.positions, d.indices = m.positions.ctypes.data, m.indices.ctypes.data
            d.normals = None if m.normals is None else m.normals.ctypes.data
            d.uvs = None if m.uvs is None else m.uvs.ctypes.data
            d.n_vertices, d.n_triangles = m.n_vertices, m.n_triangles
        recs = (_lib.MeshInstance * len(self.instances))()
        for r, inst in zip(recs, self.instances):
            r.mesh = inst.mesh
            if inst.material is not None:
                r.surface, r.material = _lib.MESH_MATERIAL, int(inst.material)
            elif inst.diffuse is not None:
                r.surface, r.color0 = _lib.MESH_DIFFUSE, float(inst.diffuse)
            else:
                r.surface = _lib.MESH_CHECKER
                r.color0, r.color1, r.uscale, r.vscale = (float(v) for v in inst.checker)
            r.to_world = (C.c_float * 12)(*[float(v) for v in inst.matrix().reshape(-1)])
        return descs, recs

    def handle(self):
        """The native scene on the current device."""
        import torch
        dev = torch.cuda.current_device()
        if dev not in self._handles:
            descs, recs = self._records()
            h = C.c_void_p()
            _lib.check(_lib.lib().bsdfd_mesh_scene_create(descs, len(self.meshes), recs, len(self.instances), C.byref(h)))
            self._handles[dev] = h
        return self._handles[dev]

    @staticmethod
    def _rays(org, dir, tmax, skip):
        import torch
        n = org.shape[0]
        for name, a, shape, dt in (("org", org, (n, 3), torch.float32), ("dir", dir, (n, 3), torch.float32),
                                   ("tmax", tmax, (n,), torch.float32), ("skip", skip, (n, 2), torch.int32)):
            if a is None:
                continue
            if a.shape != shape or a.dtype != dt or not a.is_contiguous() or not a.is_cuda or a.device != org.device:
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on the rays' device")
        return n

    def intersect(self, org, dir, tmax=None, skip=None):
        """Closest hit of org + t dir with 0 < t <= tmax, the primitive ``skip`` = (instance, triangle) excepted ->
        (t [N], prim int32 [N,2], bary [N,2]); a miss is (3.0e38, (-1, -1), 0)."""
        import torch
        n = self._rays(org, dir, tmax, skip)
        t = torch.empty(n, dtype=torch.float32, device=org.device)
        prim = torch.empty((n, 2), dtype=torch.int32, device=org.device)
        bary = torch.empty((n, 2), dtype=torch.float32, device=org.device)
        with torch.cuda.device(org.device):
            _lib.check(_lib.lib().bsdfd_mesh_intersect(self.handle(), n, _p(org), _p(dir), _p(tmax), _p(skip), _p(t), _p(prim), _p(bary),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return t, prim, bary

    def occluded(self, org, dir, tmax=None, skip=None):
        """uint8 [N]: 1 where ``intersect`` would report a hit."""
        import torch
        n = self._rays(org, dir, tmax, skip)
        out = torch.empty(n, dtype=torch.uint8, device=org.device)
        with torch.cuda.device(org.device):
            _lib.check(_lib.lib().bsdfd_mesh_occluded(self.handle(), n, _p(org), _p(dir), _p(tmax), _p(skip), _p(out),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def primary(self, wf_scene, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int, b):
        """``bsdfd_wf_primary`` on this scene: fills b["wi"], b["wl"], b["nrm"], b["dir"] ([N,3] fp32) and b["mat"] (int64 [N], if
        present) for the camera, film and material count (1 + n_extra_spheres) of the ``_lib.WfScene``."""
        import torch
        dev = b["wi"].device
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bsdfd_mesh_primary(self.handle(), C.byref(wf_scene), row_begin, row_end, spp, seed, pass_idx,
                                                     _p(b["wi"]), _p(b["wl"]), _p(b["nrm"]), _p(b["dir"]),
                                                     _p(b["mat"]) if "mat" in b else None,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.autograd.graph.increment_version([b["wi"], b["wl"], b["nrm"], b["dir"]])
        return b


# ---- the reference's scene files ----
def _floats(s):
    return [float(v) for v in s.replace(",", " ").split()]


def transform_from_xml(node) -> np.ndarray:
    """The 4x4 matrix of a <transform>: its children ``matrix / scale / translate / rotate / lookAt`` in document order, each new
    one multiplied from the LEFT (Mitsuba applies them to a point in the order they are written)."""
    m = np.eye(4)
    for c in node:
        t = np.eye(4)
        tag = c.tag.lower()
        if tag == "matrix":
            v = _floats(c.get("value"))
            if len(v) != 16:
                raise ValueError("<matrix> needs 16 values")
            t = np.array(v).reshape(4, 4)
        elif tag == "scale":
            if c.get("value") is not None:
                s = [float(c.get("value"))] * 3
            else:
                s = [float(c.get(a, 1.0)) for a in "xyz"]
            t = np.diag(s + [1.0])
        elif tag == "translate":
            t[:3, 3] = [float(c.get(a, 0.0)) for a in "xyz"]
        elif tag == "rotate":
            ax = np.array([float(c.get(a, 0.0)) for a in "xyz"])
            ax /= np.linalg.norm(ax)
            ang = math.radians(float(c.get("angle")))
            k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            t[:3, :3] = np.eye(3) + math.sin(ang) * k + (1 - math.cos(ang)) * (k @ k)   # Rodrigues
        elif tag == "lookat":
            raise ValueError("<lookAt> is read by the sensor only")
        else:
            raise ValueError(f"unknown transform element <{c.tag}>")
        m = t @ m
    return m


def _grey(node, what):
    v = _floats(node.get("value"))
    if len(v) not in (1, 3) or any(abs(x - v[0]) > 1e-6 for x in v):
        raise ValueError(f"{what}: only grey reflectances are supported, got {node.get('value')!r}")
    return v[0]


def _diffuse_surface(bsdf, by_id, what):
    """(diffuse, checker) of a <bsdf type="diffuse">: a constant, or its checkerboard texture (nested or referenced)."""
    if bsdf.get("type") != "diffuse":
        raise ValueError(f"{what}: bsdf type {bsdf.get('type')!r} is not supported (mybsdf or diffuse)")
    for c in bsdf:
        if c.get("name") != "reflectance":
            continue
        tex = by_id.get(c.get("id")) if c.tag == "ref" else c if c.tag == "texture" else None
        if tex is None and c.tag in ("rgb", "spectrum", "float"):
            return _grey(c, what), None
        if tex is None or tex.get("type") != "checkerboard":
            raise ValueError(f"{what}: reflectance must be a constant or a checkerboard texture")
        prm = {"color0": 0.4, "color1": 0.2, "uscale": 1.0, "vscale": 1.0}   # Mitsuba's defaults
        for q in tex:
            if q.get("name") in ("color0", "color1"):
                prm[q.get("name")] = _grey(q, what)
            elif q.get("name") in ("uscale", "vscale"):
                prm[q.get("name")] = float(q.get("value"))
            elif q.get("name") in ("uoffset", "voffset") and float(q.get("value")) != 0.0:
                raise ValueError(f"{what}: uv offsets are not supported")
        return None, (prm["color0"], prm["color1"], prm["uscale"], prm["vscale"])
    return 0.5, None   # Mitsuba's default reflectance


def mesh_scene_from_matpreview_xml(xml_path: str, mesh_path: Optional[str] = None, width: int = 683, height: int = 512):
    """(material names, camera, MeshScene, ball_albedo) from a reference scene file (rendering/matpreview/disney_bsdf_array*.xml):
    every <shape type="serialized"> with its ``shapeIndex``, its ``toWorld`` and its bsdf — a nested ``mybsdf`` (material k, in
    the order of ``wavefront.parse_matpreview_xml``) or a referenced / nested ``diffuse`` with a constant or a ``checkerboard``
    reflectance — and the sensor's ``lookAt`` and ``fov`` (``fovAxis = smaller`` converted as ``wavefront.array0_scene`` does).
    Every transform and the camera go through the change of basis z-up -> y-up, (x, y, z) -> (x, z, -y), so the sky and the Philox
    streams keep their meaning.  ``mesh_path``: the ``.serialized`` file (default: the shapes' ``filename``, relative to the XML).
    Parity-unpinned against Mitsuba (see the module docstring)."""
    import xml.etree.ElementTree as ET
    from . import wavefront as WF
    root = ET.parse(xml_path).getroot()
    by_id = {e.get("id"): e for e in root.iter() if e.get("id") is not None and e.tag != "ref"}
    entries = WF.parse_matpreview_xml(xml_path)
    names = [str(p["filename"]) if "filename" in p else f"bsdf_{int(p['idx'])}" for p, _ in entries]
    files, slots, meshes, instances = {}, {}, [], []
    n_mat = 0
    for shape in root.iter("shape"):
        what = f"{xml_path}: shape {shape.get('id')!r}"
        mybsdf = next((b for b in shape.findall("bsdf") if b.get("type") == "mybsdf"), None)
        if shape.get("type") != "serialized":
            if mybsdf is not None:
                raise ValueError(f"{what}: a mybsdf shape that is no serialized mesh")
            continue
        fn = next((c.get("value") for c in shape.findall("string") if c.get("name") == "filename"), None)
        path = mesh_path or os.path.join(os.path.dirname(os.path.abspath(xml_path)), fn or "")
        if path not in files:
            files[path] = load_serialized(path)
        index = next((int(c.get("value")) for c in shape.findall("integer") if c.get("name") == "shapeIndex"), 0)
        if not 0 <= index < len(files[path]):
            raise ValueError(f"{what}: shapeIndex {index} of {len(files[path])}")
        if (path, index) not in slots:
            slots[(path, index)] = len(meshes)
            meshes.append(files[path][index])
        tr = next((t for t in shape.findall("transform") if t.get("name") == "toWorld"), None)
        to_world = TO_Y_UP @ (np.eye(4) if tr is None else transform_from_xml(tr))
        kw = {}
        if mybsdf is not None:
            kw["material"] = n_mat
            n_mat += 1
        else:
            bsdf = next(iter(shape.findall("bsdf")), None)
            if bsdf is None:
                ref = next((r for r in shape.findall("ref") if r.get("id") in by_id and by_id[r.get("id")].tag == "bsdf"), None)
                bsdf = None if ref is None else by_id[ref.get("id")]
            if bsdf is None:
                raise ValueError(f"{what}: no bsdf")
            kw["diffuse"], kw["checker"] = _diffuse_surface(bsdf, by_id, what)
        instances.append(Instance(slots[(path, index)], to_world[:3], **kw))
    if n_mat != len(names) or not names:
        raise ValueError(f"{xml_path}: {n_mat} serialized mybsdf shapes, {len(names)} mybsdf shapes in all")
    sensor = next(iter(root.iter("sensor")), None)
    if sensor is None:
        raise ValueError(f"{xml_path}: no sensor")
    look = next((c for t in sensor.findall("transform") for c in t if c.tag.lower() == "lookat"), None)
    if look is None:
        raise ValueError(f"{xml_path}: the sensor's toWorld must be a <lookAt>")
    y_up = lambda name: tuple(float(v) for v in TO_Y_UP[:3, :3] @ np.array(_floats(look.get(name))))
    fov = next((float(c.get("value")) for c in sensor.findall("float") if c.get("name") == "fov"), None)
    if fov is None:
        raise ValueError(f"{xml_path}: the sensor has no fov")
    axis = next((c.get("value") for c in sensor.findall("string") if c.get("name") == "fovAxis"), "x")
    if axis == "smaller":
        fov = 2 * math.degrees(math.atan(math.tan(math.radians(fov) / 2) * max(width / height, 1.0)))
    elif axis != "x":
        raise ValueError(f"{xml_path}: fovAxis {axis!r} is not supported (x or smaller)")
    cam = WF.Camera(origin=y_up("origin"), target=y_up("target"), up=y_up("up"), fov_deg=fov, width=width, height=height)
    return names, cam, MeshScene(meshes, instances), WF.albedos_from_matpreview_xml(xml_path)


class MeshArrayRenderer(ArrayRenderer):
    """``ArrayRenderer`` on a ``MeshScene``: the base class gets one placeholder sphere per material — they are never intersected;
    they keep ``n_sph = len(table)``, so that the diffuse id and the miss id are where ``shade_kernel`` and the bucketing expect
    them — and ``primary()`` calls ``bsdfd_mesh_primary`` on the same buffers.  ``render_pass``, the bucketing, the direct and
    gathered sampler forms, both ground-truth tables and ``shade`` are the base class's.  The instances' material indices must be
    exactly 0 .. len(table) - 1.  One bounce, unoccluded (``MeshPathArrayRenderer`` traces the rest); parity-unpinned against
    Mitsuba."""

    def __init__(self, table, mesh_scene: MeshScene, camera=None, env=None, albedo=(1.0, 1.0, 1.0), ground_truth=None,
                 ball_albedo=None, device=None, fused_ground_truth: bool = True):
        _check_mesh_scene(table, mesh_scene)
        n = len(table)
        super().__init__(table, [(0.0, 0.0, 0.0)] * n, [1.0] * n, camera=camera, env=env, floor=False, albedo=albedo,
                         ground_truth=ground_truth, device=device, fused_ground_truth=fused_ground_truth, ball_albedo=ball_albedo)
        self.mesh_scene = mesh_scene

    def primary(self, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int, out=None):
        """-> dict(wi, wl, nrm, dir [, mat]) of the mesh scene's closest hits; ``dir`` and ``wl`` are the base class's bits."""
        n = (row_end - row_begin) * self.camera.width * spp
        b = out or self._buffers(n)
        return self.mesh_scene.primary(self.scene, row_begin, row_end, spp, seed, pass_idx, b)


def _check_mesh_scene(table, mesh_scene):
    if not isinstance(mesh_scene, MeshScene):
        raise ValueError("mesh_scene must be a mesh.MeshScene")
    if mesh_scene.material_indices != list(range(len(table))):
        raise ValueError(f"the instances' material indices {mesh_scene.material_indices} must cover 0 .. {len(table) - 1} exactly")


class MeshPathArrayRenderer(PathArrayRenderer):
    """``PathArrayRenderer`` on a ``MeshScene``: the base class gets one placeholder sphere per material, as ``MeshArrayRenderer``
    gives its own, and the stages that touch geometry go to the mesh entry points:

    * ``primary`` calls ``bsdfd_mesh_path_primary``, which writes the first vertex of the path as well (``org``, ``prim``, ``beta``,
      ``rad``), so ``path_begin`` has nothing left to do;
    * ``sample_emitter`` and ``bounce`` are the base class's methods; ``_geometry`` sends them to ``bsdfd_mesh_sample_emitter`` and
      ``bsdfd_mesh_bounce`` with the scene's handle in front and ``prim`` behind;
    * the path state has one more array, ``prim`` int32 [N,2]: the (instance, triangle) a vertex lies on, which its rays skip.

    ``render_pass``, the bucketing, the sampler launches, both ground-truth tables, ``resolve`` and ``stats`` are inherited, and
    ``max_depth``, ``occlusion``, ``lights``, ``rr_depth`` and ``DEPTH_CAP`` mean what they mean there.  ``env_sampling`` other than
    ``"cosine"`` and ``transmission=True`` are refused: not on meshes yet.  ``sample_emitter`` and ``bounce`` take a live-lane list
    (``rows=``: ``bsdfd_mesh_sample_emitter_rows`` / ``bsdfd_mesh_bounce_rows``; an empty list returns without a launch, and an
    ``env_dist`` is a ``ValueError``); the renderer that runs its deep bounces on one is
    ``CompactMeshPathArrayRenderer``, and ``compact=True`` here is refused and points there.  Limits: the module docstring's.
    Parity-unpinned against Mitsuba."""

    def __init__(self, table, mesh_scene: MeshScene, camera=None, env=None, *, max_depth: Optional[int] = 1,
                 occlusion: Optional[bool] = None, lights=None, rr_depth: Optional[int] = None, albedo=(1.0, 1.0, 1.0),
                 ground_truth=None, ball_albedo=None, device=None, fused_ground_truth: bool = True, env_sampling: str = "cosine",
                 compact: bool = False, transmission: bool = False):
        if env_sampling != "cosine":
            raise ValueError(f"env_sampling={env_sampling!r}: importance sampling of the environment is not on meshes yet")
        if compact:
            raise ValueError("compact=True is not on meshes yet as an argument: the live-lane list is mesh.CompactMeshPathArrayRenderer")
        if transmission:
            raise ValueError("transmission=True: transmitted paths are not on meshes yet")
        if not isinstance(mesh_scene, MeshScene):
            raise ValueError("mesh_scene must be a mesh.MeshScene: other geometry is not on meshes yet")
        _check_mesh_scene(table, mesh_scene)
        n = len(table)
        super().__init__(table, [(0.0, 0.0, 0.0)] * n, [1.0] * n, camera, env, max_depth=max_depth, occlusion=occlusion, lights=lights,
                         rr_depth=rr_depth, floor=False, albedo=albedo, ground_truth=ground_truth, device=device,
                         fused_ground_truth=fused_ground_truth, ball_albedo=ball_albedo)
        self.mesh_scene = mesh_scene

    def _buffers(self, n: int):
        import torch
        b = super()._buffers(n)
        if "prim" not in b:
            b["prim"] = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        return b

    def primary(self, row_begin: int, row_end: int, spp: int, seed: int, pass_idx: int, out=None):
        """-> dict(wi, wl, nrm, dir, mat, org, prim, beta, rad): the mesh scene's closest hits as ``MeshArrayRenderer.primary``
        writes them, and the first vertex of every path."""
        import torch
        n = (row_end - row_begin) * self.camera.width * spp
        b = out or self._buffers(n)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bsdfd_mesh_path_primary(
                self.mesh_scene.handle(), C.byref(self.scene), row_begin, row_end, spp, seed, pass_idx, _p(b["wi"]), _p(b["wl"]),
                _p(b["nrm"]), _p(b["dir"]), _p(b["mat"]), _p(self.env), _p(b["org"]), _p(b["prim"]), _p(b["beta"]), _p(b["rad"]),
                self._stream()))
        torch.autograd.graph.increment_version([b[k] for k in ("wi", "wl", "nrm", "dir", "mat", "org", "prim", "beta", "rad")])
        return b

    def path_begin(self, b):
        """Nothing: ``primary`` has written ``org``, ``prim``, ``beta`` and ``rad`` (the hit's t is known there and nowhere else)."""

    def _geometry(self, b, env_dist=None) -> _Geometry:
        """The mesh scene's part of the two stages: its handle in front, ``prim`` behind — the shadow rays and the continuation rays
        skip it, and the bounce moves it on with the vertex.  An empty list returns without a launch."""
        if env_dist is not None:
            raise ValueError("env_dist: the environment's importance sampling is not on meshes yet")
        return _Geometry("bsdfd_mesh_", True, [self.mesh_scene.handle()], [_p(b["prim"])], [b["prim"]])


class CompactMeshPathArrayRenderer(MeshPathArrayRenderer):
    """``MeshPathArrayRenderer`` with ``PathArrayRenderer``'s ``compact=True``: bounce 0 runs over all N lanes as before; from
    bounce 1 on ``sample_emitter`` and ``bounce`` run over the live-lane list the bucketing of the bounce before left (the front of
    ``bucket_rows``' permutation: sorted by material, stable in lane order, ended paths left out), through
    ``bsdfd_mesh_sample_emitter_rows`` and ``bsdfd_mesh_bounce_rows``, and the sampler and the ground-truth table serve the list's
    material prefix.  ``render_pass`` is inherited unchanged — it forms the list and hands ``rows=`` on wherever ``self.compact``
    is set.  The film, the path state and ``stats`` are the plain renderer's bit for bit (a lane's Philox counters are keyed by the
    lane, never by the thread); ``stats["list_per_bounce"]`` holds the list lengths.  What it buys (profiles/mesh_path_compact.json,
    tools/mesh_bench.py --path --compact; the fixture scene): 1.16x at ``max_depth=2`` and 1.20x at 4 — while more than ~5 % of
    the lanes live, fewer waves walk — and 1.39x SLOWER at ``max_depth=None``: a short list packs 64 unrelated rays into a wave
    whose walk lasts ~2 ms, where the full-width launch runs the same rays one to a wave, side by side.  Use it at fixed depths.

    The constructor's arguments are ``MeshPathArrayRenderer``'s without ``compact``, and so are its refusals.  A class of its own,
    not an argument: ``MeshPathArrayRenderer(..., compact=True)`` keeps its refusal."""

    def __init__(self, table, mesh_scene: MeshScene, camera=None, env=None, *, max_depth: Optional[int] = 1,
                 occlusion: Optional[bool] = None, lights=None, rr_depth: Optional[int] = None, albedo=(1.0, 1.0, 1.0),
                 ground_truth=None, ball_albedo=None, device=None, fused_ground_truth: bool = True, env_sampling: str = "cosine",
                 transmission: bool = False):
        super().__init__(table, mesh_scene, camera, env, max_depth=max_depth, occlusion=occlusion, lights=lights, rr_depth=rr_depth,
                         albedo=albedo, ground_truth=ground_truth, ball_albedo=ball_albedo, device=device,
                         fused_ground_truth=fused_ground_truth, env_sampling=env_sampling, transmission=transmission)
        self.compact = True
