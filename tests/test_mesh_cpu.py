"""CPU tests of the mesh layer (bsdf_diffusion_sampling_amd/mesh.py, the host code of csrc/mesh.hip): the ``.serialized`` reader,
the threaded-BVH builder (``bsdfd_mesh_bvh_build``, no HIP call), the fp64 walk of that BVH against fp64 brute force
(tests/mesh_ref.py) — which pins the culling and the skip links before any GPU is involved — and the scene-file parser."""
import os
import struct
import zlib

import numpy as np
import pytest

import mesh_ref as R
from bsdf_diffusion_sampling_amd import _lib, mesh as M
from bsdf_diffusion_sampling_amd import wavefront as WF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESH_FILE = os.path.join(GOLDEN, "matpreview.serialized")
SCENE_FILE = os.path.join(GOLDEN, "disney_bsdf_array2_spherical_envmap.xml")
COUNTS = [(289, 512), (2078, 3936), (29439, 57152)]   # plane, interior, shell: (vertices, triangles)


@pytest.fixture(scope="module")
def shapes():
    return M.load_serialized(MESH_FILE)


# ---- reader ----
def write_serialized(path, meshes, version, double, with_normals, with_uv):
    real = "<f8" if double else "<f4"
    blob, offsets = b"", []
    for k, m in enumerate(meshes):
        flags = (M.FLAG_DOUBLE if double else 0x1000) | (M.FLAG_NORMALS if with_normals else 0) | (M.FLAG_UV if with_uv else 0)
        raw = struct.pack("<I", flags)
        if version == 4:
            raw += f"shape{k}".encode() + b"\0"
        raw += struct.pack("<QQ", m.n_vertices, m.n_triangles) + m.positions.astype(real).tobytes()
        if with_normals:
            raw += m.normals.astype(real).tobytes()
        if with_uv:
            raw += m.uvs.astype(real).tobytes()
        raw += m.indices.astype("<u4").tobytes()
        offsets.append(len(blob))
        blob += struct.pack("<HH", M.FILE_MAGIC, version) + zlib.compress(raw)
    blob += struct.pack("<" + str(len(offsets)) + ("Q" if version == 4 else "I"), *offsets) + struct.pack("<I", len(offsets))
    with open(path, "wb") as f:
        f.write(blob)


@pytest.mark.parametrize("version", [3, 4])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("attrs", [(False, False), (True, False), (False, True), (True, True)])
def test_reader_round_trips_a_file_the_test_wrote(tmp_path, version, double, attrs):
    small = [R.grid_mesh(2, 3, M.TriMesh), R.grid_mesh(1, 1, M.TriMesh, z=0.5)]
    path = str(tmp_path / "small.serialized")
    write_serialized(path, small, version, double, *attrs)
    back = M.load_serialized(path)
    assert len(back) == 2
    for a, b in zip(small, back):
        assert np.array_equal(a.positions, b.positions) and np.array_equal(a.indices, b.indices)
        assert (b.normals is not None) == attrs[0] and (b.uvs is not None) == attrs[1]
        assert b.normals is None or np.array_equal(a.normals, b.normals)
        assert b.uvs is None or np.array_equal(a.uvs, b.uvs)
    assert [b.name for b in back] == (["shape0", "shape1"] if version == 4 else ["", ""])


def test_fixture_holds_the_three_meshes_of_the_issue(shapes):
    assert [(m.n_vertices, m.n_triangles) for m in shapes] == COUNTS
    assert all(m.normals is not None and m.uvs is not None for m in shapes)
    assert os.path.getsize(MESH_FILE) == 857057


def test_truncated_file_and_index_out_of_range_are_refused(tmp_path):
    data = open(MESH_FILE, "rb").read()
    for cut in (3, 1000, len(data) // 2, len(data) - 5):
        p = str(tmp_path / f"cut{cut}.serialized")
        open(p, "wb").write(data[:cut])
        with pytest.raises(ValueError):
            M.load_serialized(p)
    g = R.grid_mesh(1, 1, M.TriMesh)
    bad = M.TriMesh(g.positions, g.indices)
    bad.indices = bad.indices.copy()
    bad.indices[1, 2] = 4                      # behind the reader's back: the file then carries an index == nv
    p = str(tmp_path / "bad.serialized")
    write_serialized(p, [bad], 4, False, False, False)
    with pytest.raises(ValueError, match="out of range"):
        M.load_serialized(p)
    with pytest.raises(ValueError, match="out of range"):
        M.TriMesh(g.positions, [[0, 1, 4]])
    with pytest.raises(ValueError, match="non-finite"):
        M.TriMesh([[0, 0, 0], [1, 0, np.nan], [0, 1, 0]], [[0, 1, 2]])


# ---- builder ----
def one_triangle():
    return M.TriMesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def five_triangles():
    """A fan of five triangles: one inner node over two leaves."""
    pos = [[0, 0, 0]] + [[np.cos(a), np.sin(a), 0.1 * k] for k, a in enumerate(np.linspace(0, 2.5, 6))]
    return M.TriMesh(pos, [[0, k + 1, k + 2] for k in range(5)], normals=np.tile([0.0, 0.0, 1.0], (7, 1)))


def check_bvh(mesh, nodes, order):
    n, nt = nodes.shape[0], mesh.n_triangles
    skip, tris = nodes["skip"].astype(np.int64), nodes["tris"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(nt))                  # a permutation
    assert (skip > np.arange(n)).all() and skip[0] == n
    leaves = np.nonzero(tris)[0]
    first, count = tris[leaves] >> 3, tris[leaves] & 7
    assert (count >= 1).all() and (count <= 4).all()
    slots = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)])
    assert np.array_equal(np.sort(slots), np.arange(nt))                  # every triangle in exactly one leaf
    assert (skip[leaves] == leaves + 1).all()
    V = mesh.positions[mesh.indices.astype(np.int64)]                     # [nt,3,3]

    def subtree(i):
        """(end, lo, hi) of the subtree at i, checking it is exactly [i, skip[i]) and that every box holds its vertices."""
        if tris[i]:
            v = V[order[(tris[i] >> 3):(tris[i] >> 3) + (tris[i] & 7)]].reshape(-1, 3)
            end = i + 1
        else:
            e1, lo1, hi1 = subtree(i + 1)
            assert e1 < skip[i], "an inner node has two children"
            end, lo2, hi2 = subtree(e1)
            v = np.stack([lo1, hi1, lo2, hi2])
        assert end == skip[i]
        lo, hi = v.min(0), v.max(0)
        assert (nodes["lo"][i] <= lo).all() and (nodes["hi"][i] >= hi).all()
        return end, lo, hi

    assert subtree(0)[0] == n
    return leaves.size


@pytest.mark.parametrize("which", ["one", "five", "plane", "interior"])
def test_builder_invariants(shapes, which):
    mesh = {"one": one_triangle, "five": five_triangles, "plane": lambda: shapes[0], "interior": lambda: shapes[1]}[which]()
    nodes, order = M.build_bvh(mesh)
    leaves = check_bvh(mesh, nodes, order)
    st = M.bvh_stats(nodes)
    assert st["nodes"] == nodes.shape[0] and st["leaves"] == leaves and st["nodes"] == 2 * leaves - 1
    if which == "one":
        assert nodes.shape[0] == 1 and nodes["tris"][0] == 1 and st["depth"] == 1
    if which == "five":
        assert nodes.shape[0] == 3 and nodes["tris"][0] == 0 and st["depth"] == 2


def test_builder_terminates_where_every_centroid_coincides():
    # 37 triangles around one centre, each the point reflection pattern of one shape: equal centroids
    g = np.random.default_rng(3)
    pos, idx = [], []
    for k in range(37):
        a, b = g.normal(size=3), g.normal(size=3)
        pos += [a, b, -a - b]                     # centroid exactly representable? -> rounded: make them identical below
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    pos = np.round(np.array(pos) * 256) / 256     # dyadic: the three sum to exactly 0 in fp32
    mesh = M.TriMesh(pos, idx)
    nodes, order = M.build_bvh(mesh)
    check_bvh(mesh, nodes, order)


def test_builder_refuses_what_it_cannot_index():
    L = _lib.lib()
    pos = np.zeros((3, 3), dtype=np.float32)
    idx = np.array([[0, 1, 3]], dtype=np.uint32)
    nodes, order, n = np.zeros(2, dtype=M.NODE_DTYPE), np.zeros(1, dtype=np.int32), _lib.C.c_int64()
    call = lambda p, i, cap: L.bsdfd_mesh_bvh_build(p.ctypes.data, 3, i.ctypes.data, 1, nodes.ctypes.data, cap, order.ctypes.data,
                                                   _lib.C.byref(n))
    assert call(pos, idx, 2) == 1 and "out of range" in L.bsdfd_last_error().decode()
    idx[0, 2] = 2
    pos[1, 1] = np.inf
    assert call(pos, idx, 2) == 1 and "non-finite" in L.bsdfd_last_error().decode()
    pos[1, 1] = 0.0
    assert call(pos, idx, 0) == 1 and "node_cap" in L.bsdfd_last_error().decode()
    assert call(pos, idx, 2) == 0 and n.value == 1
    assert L.bsdfd_mesh_bvh_build(None, 3, idx.ctypes.data, 1, nodes.ctypes.data, 2, order.ctypes.data, _lib.C.byref(n)) == 1


def test_entry_points_are_declared_and_need_a_scene():
    L = _lib.lib()
    hdr = open(os.path.join(_lib.INCLUDE_DIR, "bsdfd.h")).read()
    for name in ("bsdfd_mesh_bvh_build", "bsdfd_mesh_scene_create", "bsdfd_mesh_intersect", "bsdfd_mesh_occluded", "bsdfd_mesh_primary"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    assert "void bsdfd_mesh_scene_destroy(" in hdr and "bsdfd_mesh_scene_destroy" in _lib.EXPORTS
    csrc = os.path.join(os.path.dirname(_lib.SRC_PATH))
    assert _lib.SRC_PATHS[-1] == os.path.join(csrc, "mesh.hip") and os.path.join(csrc, "mesh_dev.h") in _lib.DEP_PATHS
    assert _lib.C.sizeof(_lib.MeshNode) == 32 == M.NODE_DTYPE.itemsize
    for n in (0, 64, -1):
        assert L.bsdfd_mesh_intersect(None, n, None, None, None, None, None, None, None, None) == 1
        assert L.bsdfd_last_error().decode() == "null mesh scene"
        assert L.bsdfd_mesh_occluded(None, n, None, None, None, None, None, None) == 1
    assert L.bsdfd_mesh_intersect(_lib.C.c_void_p(0x1000), -1, None, None, None, None, None, None, None, None) == 1
    assert L.bsdfd_last_error().decode() == "N must be >= 0"
    assert L.bsdfd_mesh_intersect(_lib.C.c_void_p(0x1000), 0, None, None, None, None, None, None, None, None) == 0


# ---- the fp64 walk against fp64 brute force ----
def test_bvh_walk_equals_brute_force_on_every_ray(shapes):
    interior = shapes[1]
    inst = [M.Instance(0, t, diffuse=0.18) for t in R.transforms()]
    org, d = R.rays_at(R.instance_boxes([interior], inst), 2048, seed=11)
    bf = R.brute_force([interior], inst, org, d)
    tmax = np.where(np.arange(2048) % 10 == 0, 0.5 * bf["t"], np.inf)      # cut some hits off
    skip = np.where((np.arange(2048) % 7 == 0)[:, None], bf["prim"], -1)   # ... and skip some of the first hits
    bvhs = [M.build_bvh(interior)]
    for kw in ({}, {"tmax": tmax}, {"skip": skip}):
        a, b = R.brute_force([interior], inst, org, d, **kw) if kw else bf, R.bvh_walk([interior], inst, bvhs, org, d, **kw)
        assert np.array_equal(a["prim"], b["prim"])
        hit = a["t"] < R.NOTHING
        assert 0.3 < hit.mean() < 0.95 and len(set(a["prim"][hit, 0])) == 3
        assert np.array_equal(a["t"] < R.NOTHING, b["t"] < R.NOTHING)
        # the walk intersects in object space, brute force in world space: the same real numbers, rounded differently in fp64
        assert np.allclose(a["t"], b["t"], rtol=1e-11, atol=0) and np.allclose(a["bary"], b["bary"], rtol=0, atol=1e-10)
        assert np.array_equal(a["marginal"], b["marginal"])
        R.assert_marginal_cap(a)


# ---- scene files ----
def test_transform_children_compose_in_document_order_from_the_left(tmp_path):
    import xml.etree.ElementTree as ET
    node = ET.fromstring('<transform name="toWorld"><matrix value="1 0 0 1  0 1 0 2  0 0 1 3  0 0 0 1"/>'
                         '<scale x="2" y="3" z="4"/><rotate z="1" angle="90"/><translate x="10"/><scale value="0.5"/></transform>')
    m = M.transform_from_xml(node)
    p = np.array([1.0, 1.0, 1.0, 1.0])
    # by hand: +(1,2,3) -> (2,3,4); *(2,3,4) -> (4,9,16); rotate 90 deg about z: (x,y) -> (-y,x) -> (-9,4,16); +10 x -> (1,4,16); /2
    assert np.allclose(m @ p, [0.5, 2.0, 8.0, 1.0])
    assert np.allclose(m[3], [0, 0, 0, 1])
    with pytest.raises(ValueError):
        M.transform_from_xml(ET.fromstring('<transform><shear x="1"/></transform>'))


def test_change_of_basis_is_the_array_layouts():
    assert np.allclose(M.TO_Y_UP @ [1.0, 2.0, 3.0, 1.0], [1.0, 3.0, -2.0, 1.0])   # (x, y, z) -> (x, z, -y)
    x, y, _ = WF.ARRAY0_LAYOUT[0]
    _, centers, _ = WF.array0_scene()
    assert np.allclose((M.TO_Y_UP @ [x, y, 0.33, 1.0])[:3], centers[0])


def test_fixture_scene():
    names, cam, scene, albedo = M.mesh_scene_from_matpreview_xml(SCENE_FILE, MESH_FILE, 64, 48)
    entries = WF.parse_matpreview_xml(SCENE_FILE)
    assert names == [f"bsdf_{int(p['idx'])}" for p, _ in entries] and len(names) == 12
    assert albedo == WF.albedos_from_matpreview_xml(SCENE_FILE)
    inst = scene.instances
    assert len(inst) == 25 and len(scene.meshes) == 3
    mats = [i for i in inst if i.material is not None]
    const = [i for i in inst if i.diffuse is not None]
    chk = [i for i in inst if i.checker is not None]
    assert [i.material for i in mats] == list(range(12)) and scene.material_indices == list(range(12))
    assert len(const) == 12 and all(i.diffuse == 0.18 for i in const)
    assert len(chk) == 1 and tuple(chk[0].checker) == (0.4, 0.2, 8.0, 16.0)
    tri = {i.mesh: scene.meshes[i.mesh].n_triangles for i in inst}
    assert {tri[i.mesh] for i in mats} == {57152} and {tri[i.mesh] for i in const} == {3936} and tri[chk[0].mesh] == 512
    # the first shell: matrix, then scale 0.5, then two translations, then the change of basis — its last <translate> is
    # parse_matpreview_xml's ball position
    (x, y, _), m0 = entries[0][1], mats[0].matrix()
    assert np.allclose(m0 @ [0, 0, 0, 1], M.TO_Y_UP[:3, :3] @ [-1.78814e-07 * 0.5 + x, 2.08616e-07 * 0.5 + y, 1.02569 * 0.5 + 0.01])
    assert np.isclose(abs(np.linalg.det(m0[:, :3])), 0.614046 ** 2 * 2 * 0.868393 / 8, rtol=1e-4)
    # the camera: the file's lookAt under the change of basis, fov on the smaller axis converted as array0_scene does
    assert np.allclose(cam.origin, (3.89558, 3.25463, 3.46243)) and np.allclose(cam.target, (3.24072, 2.80939, 2.85176))
    assert np.allclose(cam.up, (-0.317366, 0.895346, -0.312466))
    assert np.isclose(cam.fov_deg, WF.array0_scene(64, 48)[0].fov_deg) and (cam.width, cam.height) == (64, 48)
    st = scene.stats
    assert [s["triangles"] for s in st] == [scene.meshes[k].n_triangles for k in range(3)]
    assert all(s["nodes"] == 2 * s["leaves"] - 1 and 2 ** (s["depth"] - 1) >= s["leaves"] for s in st)


def test_scene_refusals(shapes):
    plane = shapes[0]
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    with pytest.raises(ValueError, match="singular"):
        M.MeshScene([plane], [M.Instance(0, np.zeros((3, 4)), diffuse=0.5)])
    with pytest.raises(ValueError, match="exactly one"):
        M.MeshScene([plane], [M.Instance(0, eye, diffuse=0.5, material=0)])
    with pytest.raises(ValueError, match="mesh index"):
        M.MeshScene([plane], [M.Instance(1, eye, diffuse=0.5)])
    with pytest.raises(ValueError, match="instances"):
        M.MeshScene([plane], [M.Instance(0, eye, diffuse=0.5)] * 65)
    with pytest.raises(ValueError, match="checker"):
        M.MeshScene([one_triangle()], [M.Instance(0, eye, checker=(0.4, 0.2, 8, 16))])
    M.MeshScene([plane], [M.Instance(0, np.diag([-1.0, 1.0, 1.0, 1.0]), material=0)])   # a mirroring one is fine
