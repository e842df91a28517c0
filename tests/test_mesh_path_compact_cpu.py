"""CPU side of the live-lane list of the path tracer on meshes (csrc/mesh.hip: bsdfd_mesh_sample_emitter_rows / _bounce_rows;
``mesh.CompactMeshPathArrayRenderer``): the C ABI stays version 8 with two more symbols, which take their full-width sibling's
arguments with (rows, n_rows) in front of the stream; the entry points refuse what needs no device to refuse; ``rows=`` is an
argument of the two stages; and the new class refuses what its parent refuses, before a device is touched."""
import ctypes as C
import inspect
import os

import pytest

import mesh_bounce_ref as MB
from bsdf_diffusion_sampling_amd import _lib, mesh as M
from test_mesh_path_cpu import HANDLE, ROOT, _bounce_args, _scene

SYMBOLS = ("bsdfd_mesh_sample_emitter_rows", "bsdfd_mesh_bounce_rows")


def test_library_exports_the_list_forms_without_a_new_abi():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
        sibling = getattr(L, name[:-len("_rows")]).argtypes
        assert getattr(L, name).argtypes == sibling[:-1] + [C.c_void_p, C.c_int64, sibling[-1]]
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert all(name + "()" in note for name in SYMBOLS)
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr


def _rows_args(args, rows, n_rows):
    """A full-width argument list with (rows, n_rows) in front of the stream."""
    return args[:-1] + [rows, n_rows, args[-1]]


def test_list_forms_refuse_without_a_device():
    L = _lib.lib()
    sc, fake = _scene(), C.c_void_p(0x2000)
    lights = _lib.WfLights()
    lights.n_lights = 1
    err = lambda: L.bsdfd_last_error().decode()

    def bounce(handle, n, fill, rows, n_rows, **kw):
        return L.bsdfd_mesh_bounce_rows(*_rows_args(_bounce_args(handle, sc, n, fill, **kw), rows, n_rows))

    def emitter(handle, n, fill, rows, n_rows):
        return L.bsdfd_mesh_sample_emitter_rows(handle, C.byref(sc), C.byref(lights), 0, 1, 1, 0, 0, n, *[fill] * 7, fill, rows, n_rows, None)
    for call in (bounce, emitter):
        # a null scene, whatever the list
        for n, n_rows in ((64, 10), (64, 0), (0, 0), (-1, 0)):
            assert call(None, n, fake, fake, n_rows) == 1 and err() == "null mesh scene"
        # the list against N, and a list without a pointer
        assert call(HANDLE, 64, fake, fake, -1) == 1 and "n_rows" in err()
        assert call(HANDLE, 64, fake, fake, 65) == 1 and "n_rows" in err()
        assert call(HANDLE, -1, fake, fake, 0) == 1                        # (N < 0: no list fits)
        assert call(HANDLE, 64, fake, None, 10) == 1 and "rows" in err()
        # a list too large for one launch (and so is its wavefront)
        assert call(HANDLE, 2 ** 40, fake, fake, 2 ** 40) == 1 and "too large" in err()
        # an empty list and an empty wavefront are no-ops, whatever the pointers
        assert call(HANDLE, 64, None, None, 0) == 0
        assert call(HANDLE, 64, fake, fake, 0) == 0
        assert call(HANDLE, 0, None, None, 0) == 0
        # null arrays are refused before the scene is looked at
        assert call(HANDLE, 64, None, fake, 10) == 1 and err() in ("null pointer", "null environment map")
    # what the full-width bounce refuses: lpdf or dist (also with an empty list), a negative rr_depth, prim
    dist = _lib.EnvDist()
    for kw in (dict(lpdf=fake), dict(dist=C.byref(dist))):
        for n_rows in (10, 0):
            assert bounce(HANDLE, 64, fake, fake, n_rows, **kw) == 1
            assert "not on meshes yet" in err() and "lpdf and dist must be NULL" in err()
    assert bounce(HANDLE, 64, fake, fake, 10, rr_depth=-1) == 1 and "rr_depth" in err()
    args = _rows_args(_bounce_args(HANDLE, sc, 64, fake), fake, 10)
    args[-4] = None                                                        # prim
    assert L.bsdfd_mesh_bounce_rows(*args) == 1 and err() == "null pointer"
    bad = _lib.WfLights()                                                  # no light at all
    assert L.bsdfd_mesh_sample_emitter_rows(HANDLE, C.byref(sc), C.byref(bad), 0, 1, 1, 0, 0, 64, *[fake] * 8, fake, 10, None) == 1
    assert "point lights" in err()


def test_rows_is_the_last_parameter_of_both_stages():
    for cls in (M.MeshPathArrayRenderer, M.CompactMeshPathArrayRenderer):
        for method in (cls.sample_emitter, cls.bounce):
            name, prm = list(inspect.signature(method).parameters.items())[-1]
            assert name == "rows" and prm.default is None
    assert M.CompactMeshPathArrayRenderer.render_pass is M.MeshPathArrayRenderer.render_pass
    assert "compact" not in inspect.signature(M.CompactMeshPathArrayRenderer.__init__).parameters
    theirs = [p for p in inspect.signature(M.MeshPathArrayRenderer.__init__).parameters if p != "compact"]
    assert list(inspect.signature(M.CompactMeshPathArrayRenderer.__init__).parameters) == theirs


def test_compact_constructor_refuses_what_its_parent_refuses():
    """Before any device is touched: a list stands in for the material table."""
    geom = MB.kernel_scene(M)
    scene = M.MeshScene(geom["meshes"], geom["instances"])
    table = [None, None]
    for kw in (dict(env_sampling="importance"), dict(transmission=True)):
        with pytest.raises(ValueError, match="not on meshes yet"):
            M.CompactMeshPathArrayRenderer(table, scene, **kw)
    with pytest.raises(TypeError):
        M.CompactMeshPathArrayRenderer(table, scene, compact=True)
    with pytest.raises(ValueError, match="not on meshes yet"):
        M.CompactMeshPathArrayRenderer(table, [(0.0, 0.0, 0.0)] * 2)
    with pytest.raises(ValueError, match="cover"):
        M.CompactMeshPathArrayRenderer([None] * 3, scene)
    with pytest.raises(ValueError, match="needs occlusion"):
        M.CompactMeshPathArrayRenderer(table, scene, max_depth=2, occlusion=False)
    with pytest.raises(ValueError, match="needs rr_depth"):
        M.CompactMeshPathArrayRenderer(table, scene, max_depth=None)
    # the argument stays refused on the plain class, and says where the list is
    with pytest.raises(ValueError, match="not on meshes yet.*CompactMeshPathArrayRenderer"):
        M.MeshPathArrayRenderer(table, scene, compact=True)
