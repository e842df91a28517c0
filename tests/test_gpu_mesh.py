"""GPU: the mesh ray caster (csrc/mesh.hip: bsdfd_mesh_intersect / _occluded / _primary) against the fp64 reference of
tests/mesh_ref.py, and ``mesh.MeshArrayRenderer``.

What is held to what:
* ``prim`` and the hit flag equal fp64 brute force (the fp64 BVH walk on the fixture scene, which tests/test_mesh_cpu.py pins to
  brute force) on every ray the reference does not mark MARGINAL (mesh_ref: within barycentric 1e-5 of an edge of a triangle whose
  plane it crosses at 0 < t <= t_best (1 + 1e-5)); at most 1 % of any set of 100 rays or more may be marginal — asserted first;
* ``t`` (relative) and ``bary`` (absolute) to 4 x the worst error of mesh_ref's numpy fp32 restatement of the kernel's formulas on
  the same case's rays against fp64 — the factor covers contraction and operation order, which the compiler is free to choose;
* ``occluded`` equals ``intersect``'s t < 3e38 exactly, on every set, with and without tmax and skip.
Every figure is printed before it is asserted."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import mesh_ref as R  # noqa: E402
from bsdf_diffusion_sampling_amd import _lib, mesh as M  # noqa: E402
from bsdf_diffusion_sampling_amd import wavefront as WF  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESH_FILE = os.path.join(GOLDEN, "matpreview.serialized")
SCENE_FILE = os.path.join(GOLDEN, "disney_bsdf_array2_spherical_envmap.xml")
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)
N_MAX = max(SIZES)
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch.device("cuda", 0)


def up(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype).contiguous()


def cast(scene, org, d, tmax=None, skip=None):
    """-> (t, prim, bary, occluded) as numpy."""
    o, dd, tm, sk = up(org), up(d), up(tmax), up(skip, torch.int32)
    t, prim, bary = scene.intersect(o, dd, tm, sk)
    occ = scene.occluded(o, dd, tm, sk)
    torch.cuda.synchronize()
    return t.cpu().numpy(), prim.cpu().numpy().astype(np.int64), bary.cpu().numpy(), occ.cpu().numpy()


@pytest.fixture(scope="module")
def shapes():
    return M.load_serialized(MESH_FILE)


def one_triangle():
    return M.TriMesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def five_triangles():
    pos = [[0, 0, 0]] + [[np.cos(a), np.sin(a), 0.1 * k] for k, a in enumerate(np.linspace(0, 2.5, 6))]
    return M.TriMesh(pos, [[0, k + 1, k + 2] for k in range(5)], normals=np.tile([0.0, 0.0, 1.0], (7, 1)))


CASES = ("one", "five", "plane", "interior3")
_case_cache = {}


def case(name, shapes):
    """A scene, its N_MAX rays, their fp64 brute-force answers and the fp32 restatement's error: made once per module."""
    if name in _case_cache:
        return _case_cache[name]
    if name == "interior3":
        meshes, inst = [shapes[1]], [M.Instance(0, t, diffuse=0.18) for t in R.transforms()]
    else:
        meshes = [{"one": one_triangle, "five": five_triangles, "plane": lambda: shapes[0]}[name]()]
        inst = [M.Instance(0, EYE, diffuse=0.5)]
    boxes = R.instance_boxes(meshes, inst)
    boxes = [(lo - 0.05 * np.linalg.norm(hi - lo), hi + 0.05 * np.linalg.norm(hi - lo)) for lo, hi in boxes]   # flat meshes too
    org, d = R.rays_at(boxes, N_MAX, seed=20 + CASES.index(name))
    ref = R.brute_force(meshes, inst, org, d)
    et, eb = R.fp32_restatement_error(meshes, inst, org, d, ref)
    print(f"[{name}] fp32 restatement against fp64 on {N_MAX} rays: t rel {et:.3e}, bary abs {eb:.3e}; "
          f"hits {np.mean(ref['t'] < R.NOTHING):.3f}, marginal {ref['marginal'].sum()}")
    _case_cache[name] = dict(meshes=meshes, inst=inst, scene=M.MeshScene(meshes, inst), org=org, d=d, ref=ref, et=et, eb=eb)
    return _case_cache[name]


def compare(got, ref, et, eb, what):
    """(t, prim, bary) of the GPU against a reference dict on its unmarginal rays."""
    t, prim, bary = got
    R.assert_marginal_cap(ref)
    ok = ~ref["marginal"]
    hit = ref["t"] < R.NOTHING
    assert np.array_equal((t < R.NOTHING)[ok], hit[ok]), f"{what}: hit flags"
    bad = np.nonzero(ok & (prim != ref["prim"]).any(1))[0]
    assert bad.size == 0, f"{what}: prim differs on rays {bad[:8]}: {prim[bad[:4]]} vs {ref['prim'][bad[:4]]}"
    s = ok & hit
    rel = np.abs(t[s] - ref["t"][s]) / ref["t"][s] if s.any() else np.zeros(1)
    db = np.abs(bary[s] - ref["bary"][s]) if s.any() else np.zeros(1)
    print(f"{what}: t rel err {rel.max():.3e} (bound {4 * et:.3e}), bary abs err {db.max():.3e} (bound {4 * eb:.3e}), "
          f"{int(s.sum())} hits, {int(ref['marginal'].sum())} marginal")
    assert rel.max() <= 4 * et and db.max() <= 4 * eb, what
    miss = ~(t < R.NOTHING)                       # every miss, marginal or not, is written as specified
    assert (t[miss] == np.float32(3.0e38)).all() and (prim[miss] == -1).all() and (bary[miss] == 0).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_intersect_equals_fp64_brute_force(shapes, name, n):
    c = case(name, shapes)
    ref = {k: v[:n] for k, v in c["ref"].items()}
    org, d = c["org"][:n], c["d"][:n]
    hit = ref["t"] < R.NOTHING
    if n >= 255:
        assert hit.any() and (~hit).any()
    t, prim, bary, occ = cast(c["scene"], org, d)
    compare((t, prim, bary), ref, c["et"], c["eb"], f"{name} N={n}")
    assert np.array_equal(occ, (t < R.NOTHING).astype(np.uint8))
    # tmax: half the distance cuts the hit off (nothing is nearer), twice the distance keeps it
    k = np.arange(n) % 10
    tmax = np.where(hit & (k == 0), 0.5 * ref["t"], np.where(hit & (k == 1), 2.0 * ref["t"], np.inf)).astype(np.float32)
    cut = hit & (k == 0)
    ref2 = dict(t=np.where(cut, R.NOTHING, ref["t"]), prim=np.where(cut[:, None], -1, ref["prim"]),
                bary=np.where(cut[:, None], 0.0, ref["bary"]), marginal=ref["marginal"])
    t2, prim2, bary2, occ2 = cast(c["scene"], org, d, tmax=tmax)
    compare((t2, prim2, bary2), ref2, c["et"], c["eb"], f"{name} N={n} tmax")
    assert np.array_equal(occ2, (t2 < R.NOTHING).astype(np.uint8))
    # skip = the first hit (GPU against GPU: the any-hit form must agree exactly, and the skipped primitive is never reported)
    t3, prim3, _, occ3 = cast(c["scene"], org, d, skip=prim.astype(np.int32))
    assert np.array_equal(occ3, (t3 < R.NOTHING).astype(np.uint8))
    assert not ((prim3 == prim).all(1) & (prim[:, 0] >= 0)).any()
    t4, prim4, _, occ4 = cast(c["scene"], org, d, tmax=tmax, skip=prim.astype(np.int32))
    assert np.array_equal(occ4, (t4 < R.NOTHING).astype(np.uint8))
    assert (t4[t4 < R.NOTHING] <= tmax[t4 < R.NOTHING]).all()


def test_skip_against_brute_force_and_no_skip_is_null(shapes):
    c = case("interior3", shapes)
    n = 257
    org, d = c["org"][:n], c["d"][:n]
    first = c["ref"]["prim"][:n]
    ref = R.brute_force(c["meshes"], c["inst"], org, d, skip=first)
    assert (ref["t"] < R.NOTHING).sum() > 20                      # a second surface behind the first, on many rays
    t, prim, bary, occ = cast(c["scene"], org, d, skip=first.astype(np.int32))
    compare((t, prim, bary), ref, c["et"], c["eb"], "interior3 skip")
    a = cast(c["scene"], org, d)
    b = cast(c["scene"], org, d, skip=np.full((n, 2), -1, dtype=np.int32))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_a_ray_leaving_a_triangle_does_not_report_it(shapes):
    # from points ON the triangles of the interior (fp32-rounded hit points), back out along the incoming ray and onwards through
    # the mesh: with skip = the triangle it starts on, never that triangle; a single triangle with nothing behind: a miss
    c = case("interior3", shapes)
    ref = c["ref"]
    s = np.nonzero((ref["t"] < R.NOTHING) & ~ref["marginal"])[0][:512]
    x = (c["org"][s].astype(np.float64) + ref["t"][s, None] * c["d"][s]).astype(np.float32)
    for d in (c["d"][s], -c["d"][s]):
        t, prim, _, occ = cast(c["scene"], x, d, skip=ref["prim"][s].astype(np.int32))
        assert not (prim == ref["prim"][s]).all(1).any()
        assert np.array_equal(occ, (t < R.NOTHING).astype(np.uint8))
    assert (t < R.NOTHING).mean() < 0.5 and (cast(c["scene"], x, c["d"][s], skip=ref["prim"][s].astype(np.int32))[0] < R.NOTHING).any()
    one = case("one", shapes)
    g = np.random.default_rng(5)
    b = g.dirichlet([1, 1, 1], 64)
    x = (b[:, 1:2] * [1, 0, 0] + b[:, 2:3] * [0, 1, 0]).astype(np.float32)
    d = g.normal(size=(64, 3)).astype(np.float32)
    t, prim, _, occ = cast(one["scene"], x, d, skip=np.zeros((64, 2), dtype=np.int32))
    assert (t == np.float32(3.0e38)).all() and (prim == -1).all() and not occ.any()


def on_triangle(c, org, d, t, prim, tol=1e-4):
    """The reported hit point lies on the reported triangle (fp64 barycentrics within tol), for the hits."""
    V, I, T = R.world_triangles(c["meshes"], c["inst"])
    first = np.searchsorted(I, np.arange(len(c["inst"])))
    h = prim[:, 0] >= 0
    v = V[first[prim[h, 0]] + prim[h, 1]]
    tt, u, w, ok = R._moller_trumbore(v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], org[h].astype(np.float64), d[h].astype(np.float64))
    return ok.all() and (np.minimum(np.minimum(u, w), 1 - u - w) > -tol).all() and np.allclose(tt, t[h], rtol=1e-4)


@pytest.mark.parametrize("transform", ["plain", "mirrored"])
def test_closed_mesh_is_watertight(transform):
    mesh, edges = R.octahedron(2, M.TriMesh)
    assert mesh.n_triangles == 128
    Tm = dict(zip(("plain", "scaled", "mirrored"), R.transforms()))[transform]
    inst = [M.Instance(0, Tm, diffuse=0.5)]
    scene = M.MeshScene([mesh], inst)
    Mw = R.instance_matrix(inst[0])
    g = np.random.default_rng(9)
    o = g.normal(size=(64, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    P = mesh.positions.astype(np.float64)
    targets = np.concatenate([P, 0.5 * (P[edges[:, 0]] + P[edges[:, 1]])])
    nv = P.shape[0]
    # A target is aimed at from the origins that see EVERY triangle around it from the front, with a margin: a ray that grazes the
    # convex corner at a vertex enters and leaves the mesh within an ulp of it — front and back side share the vertex — and
    # missing both is then no crack but the silhouette.  Every vertex and every edge is still aimed at, from several origins.
    idx = mesh.indices.astype(np.int64)
    ng = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    ng[(ng * P[idx].mean(1)).sum(1) < 0] *= -1                          # outward (the mesh is convex around the origin)
    around = [np.nonzero((idx == j).any(1))[0] for j in range(nv)] + \
             [np.nonzero((idx == a).any(1) & (idx == b).any(1))[0] for a, b in edges]
    assert all(len(a) >= 4 for a in around[:nv]) and all(len(a) == 2 for a in around[nv:])   # closed
    pairs = []
    for j in range(targets.shape[0]):
        w = o - targets[j]
        front = (ng[around[j]] @ (w / np.linalg.norm(w, axis=1, keepdims=True)).T > 0.1).all(0)
        assert front.sum() >= 4, j
        pairs += [(i, j) for i in np.nonzero(front)[0]]
    oi, tj = np.array(pairs).T
    org = (o[oi] @ Mw[:, :3].T + Mw[:, 3]).astype(np.float32)
    tgt = (targets[tj] @ Mw[:, :3].T + Mw[:, 3]).astype(np.float32)     # rounded to fp32
    d = tgt - org
    assert org.shape[0] > 3000
    ref = R.brute_force([mesh], inst, org, d)
    # fp64 Moeller-Trumbore is not watertight itself: on a few of these rays it falls between two triangles and reports the back
    # side; the front side is then the nearest plane crossing next to an edge
    t_ref = np.minimum(ref["t"], ref["edge_t"])
    assert np.isfinite(t_ref).all() and ref["marginal"].mean() > 0.9 and np.abs(t_ref - 1).max() < 1e-5
    et, eb = R.fp32_restatement_error([mesh], inst, org, d, dict(ref, marginal=np.zeros_like(ref["marginal"])))
    t, prim, bary, occ = cast(scene, org, d)
    rel = np.abs(t - t_ref) / t_ref
    print(f"watertight {transform}: {org.shape[0]} rays, misses {int((t >= R.NOTHING).sum())}, t rel err {rel.max():.3e} "
          f"(bound {4 * et:.3e}), worst rays {np.argsort(rel)[-3:].tolist()}: t {t[np.argsort(rel)[-3:]].tolist()}")
    assert (t < R.NOTHING).all() and occ.all()                          # no ray slips through
    assert rel.max() <= 4 * et                                          # the front side (the back is tens of per cent away)
    tri = mesh.indices[prim[:, 1]].astype(np.int64)
    is_vertex = tj < nv
    at_vertex = (tri == tj[:, None]).any(1)
    e = edges[np.where(is_vertex, 0, tj - nv)]
    at_edge = (tri == e[:, 0:1]).any(1) & (tri == e[:, 1:2]).any(1)
    assert np.where(is_vertex, at_vertex, at_edge).all()                # incident to the vertex / the edge aimed at


def test_degenerate_directions(shapes):
    c = case("plane", shapes)
    nodes, _ = c["scene"].bvh(0)
    leaf = nodes[nodes["tris"] != 0]
    xs = np.unique(np.concatenate([leaf["lo"][:, 0], leaf["hi"][:, 0]]))
    ys = np.unique(np.concatenate([leaf["lo"][:, 1], leaf["hi"][:, 1]]))
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    n = gx.size
    down = np.stack([gx.ravel(), gy.ravel(), np.full(n, 5.0)], 1).astype(np.float32)      # origins exactly in the leaves' planes
    zs = np.unique(np.concatenate([leaf["lo"][:, 2], leaf["hi"][:, 2]]))
    gy2, gz = np.meshgrid(ys, zs[:64], indexing="ij")
    along = np.stack([np.full(gy2.size, -5.0), gy2.ravel(), gz.ravel()], 1).astype(np.float32)
    org = np.concatenate([down, along])
    d = np.concatenate([np.tile([0.0, 0.0, -1.0], (n, 1)), np.tile([1.0, 0.0, 0.0], (gy2.size, 1))]).astype(np.float32)
    d[1::4, 1] = -0.0                                                   # a negative zero is a zero too
    ref = R.brute_force(c["meshes"], c["inst"], org, d)
    t, prim, bary, occ = cast(c["scene"], org, d)
    hit = ref["t"] < R.NOTHING
    print(f"degenerate: {org.shape[0]} rays, {int(hit.sum())} hits, {int(ref['marginal'].sum())} through an edge or a vertex")
    assert hit.sum() > 100 and (~hit).sum() > 10
    # these rays run THROUGH the vertices and edges the boxes are made of, so most are marginal by construction.  Off the edges
    # everything must agree.  On them the kernel may not miss where fp64 hits — fp64 Moeller-Trumbore itself is not watertight and
    # falls between two triangles on a few of these rays, so the converse is held to the geometry instead: the front-most plane
    # crossing next to an edge is then the reference for t, and the reported triangle must contain the point.
    got = t < R.NOTHING
    ok = ~ref["marginal"]
    assert np.array_equal(got[ok], hit[ok]) and np.array_equal(prim[ok], ref["prim"][ok])
    assert not (hit & ~got).any() and np.array_equal(occ, got.astype(np.uint8))
    t_ref = np.where(ok, ref["t"], np.minimum(ref["t"], ref["edge_t"]))
    assert np.isfinite(t_ref[got]).all()
    rel = np.abs(t[got] - t_ref[got]) / t_ref[got]
    print(f"  fp64 falls between triangles on {int((got & ~hit).sum())} rays; t rel err {rel.max():.3e} (bound {4 * c['et']:.3e})")
    assert rel.max() <= 4 * c["et"], rel.max()
    assert on_triangle(c, org, d, t, prim)
    # a ray in the plane of a triangle reports no hit on it
    one = case("one", shapes)
    o = np.array([[-1.0, 0.25, 0.0], [0.25, -1.0, 0.0], [2.0, 2.0, 0.0]], dtype=np.float32)
    dd = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.0]], dtype=np.float32)
    t, prim, _, occ = cast(one["scene"], o, dd)
    assert (t == np.float32(3.0e38)).all() and (prim == -1).all() and not occ.any()


def test_outputs_beyond_n_are_kept_and_misuse_is_refused(shapes):
    c = case("five", shapes)
    L, h = _lib.lib(), None
    n, pad = 100, 29
    o, d = up(c["org"][:n + pad]), up(c["d"][:n + pad])
    t = torch.full((n + pad,), -7.0, device=dev())
    prim = torch.full((n + pad, 2), -7, dtype=torch.int32, device=dev())
    bary = torch.full((n + pad, 2), -7.0, device=dev())
    occ = torch.full((n + pad,), 7, dtype=torch.uint8, device=dev())
    with torch.cuda.device(dev()):
        h = c["scene"].handle()
    p = lambda a: C.c_void_p(a.data_ptr())
    assert L.bsdfd_mesh_intersect(h, n, p(o), p(d), None, None, p(t), p(prim), p(bary), None) == 0
    assert L.bsdfd_mesh_occluded(h, n, p(o), p(d), None, None, p(occ), None) == 0
    torch.cuda.synchronize()
    assert (t[n:] == -7).all() and (prim[n:] == -7).all() and (bary[n:] == -7).all() and (occ[n:] == 7).all()
    assert (t[:n] != -7).all() and (occ[:n] != 7).all()
    # N = 0 is a no-op, whatever the pointers; null arrays and a negative N are errors
    assert L.bsdfd_mesh_intersect(h, 0, None, None, None, None, None, None, None, None) == 0
    assert L.bsdfd_mesh_occluded(h, 0, None, None, None, None, None, None) == 0
    for args in ((None, p(d), p(t), p(prim), p(bary)), (p(o), None, p(t), p(prim), p(bary)), (p(o), p(d), None, p(prim), p(bary)),
                 (p(o), p(d), p(t), None, p(bary)), (p(o), p(d), p(t), p(prim), None)):
        assert L.bsdfd_mesh_intersect(h, n, args[0], args[1], None, None, args[2], args[3], args[4], None) == 1
        assert L.bsdfd_last_error().decode() == "null pointer"
    assert L.bsdfd_mesh_occluded(h, n, p(o), p(d), None, None, None, None) == 1
    assert L.bsdfd_mesh_intersect(h, -1, p(o), p(d), None, None, p(t), p(prim), p(bary), None) == 1
    assert L.bsdfd_mesh_intersect(h, 2 ** 40, p(o), p(d), None, None, p(t), p(prim), p(bary), None) == 1
    assert "too large" in L.bsdfd_last_error().decode()
    with pytest.raises(ValueError):
        c["scene"].intersect(o.double(), d)
    # scene_create's refusals that need the C side: 65 instances, a singular transform, a checker on a mesh without uv
    desc, recs = c["scene"]._records()
    out = C.c_void_p()
    assert L.bsdfd_mesh_scene_create(desc, 1, recs, 0, C.byref(out)) == 1 and L.bsdfd_mesh_scene_create(desc, 1, recs, 65, C.byref(out)) == 1
    recs[0].to_world = (C.c_float * 12)(*([1, 0, 0, 0] * 3))
    assert L.bsdfd_mesh_scene_create(desc, 1, recs, 1, C.byref(out)) == 1 and "singular" in L.bsdfd_last_error().decode()
    desc, recs = c["scene"]._records()
    recs[0].surface = _lib.MESH_CHECKER
    assert L.bsdfd_mesh_scene_create(desc, 1, recs, 1, C.byref(out)) == 1 and "uv" in L.bsdfd_last_error().decode()


# ---- primary ----
def wf_scene(cam, n_materials):
    """The bsdfd_wf_scene ``ArrayRenderer`` builds for n_materials balls (here: out of sight) and this camera."""
    r, u, f = cam.basis()
    sc = _lib.WfScene()
    for name, val in (("cam_origin", cam.origin), ("cam_right", r), ("cam_up", u), ("cam_forward", f),
                      ("sphere_center", (0.0, -1e6, 0.0)), ("albedo", (1.0, 1.0, 1.0))):
        setattr(sc, name, (C.c_float * 3)(*[float(x) for x in val]))
    sc.tan_half_fov = math.tan(math.radians(cam.fov_deg) * 0.5)
    sc.width, sc.height, sc.sphere_radius, sc.env_height, sc.env_width = cam.width, cam.height, 1.0, 8, 16
    sc.n_extra_spheres = n_materials - 1
    for k in range(1, n_materials):
        sc.extra_spheres[k - 1] = (C.c_float * 4)(0.0, -1e6, 0.0, 1.0)
    return sc


def buffers(n):
    mk = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev())
    return dict(wi=mk(n, 3), wl=mk(n, 3), nrm=mk(n, 3), dir=mk(n, 3), mat=torch.full((n,), -7, dtype=torch.int64, device=dev()))


@pytest.fixture(scope="module")
def primary_case(shapes):
    """The checkered plane, two interiors carrying materials 0 and 1 (one of them mirrored and non-uniform) and a diffuse one,
    seen from a camera that also sees past them; W x H x SPP = 64 x 48 x 4."""
    plain, scaled, mirrored = R.transforms()
    lift = lambda t, dy: np.hstack([t[:, :3], t[:, 3:] + [[0.0], [dy], [0.0]]])
    y_up = M.TO_Y_UP[:3, :3]
    inst = [M.Instance(1, np.hstack([y_up @ (4.0 * np.eye(3)), [[0.0], [-1.0], [0.0]]]), checker=(0.4, 0.2, 8.0, 16.0)),
            M.Instance(0, np.hstack([y_up, [[0.0], [0.0], [0.0]]]), material=0),
            M.Instance(0, lift(np.hstack([y_up @ mirrored[:, :3], mirrored[:, 3:]]), 0.5), material=1),
            M.Instance(0, lift(np.hstack([y_up @ scaled[:, :3], scaled[:, 3:]]), 0.3), diffuse=0.18)]
    meshes = [shapes[1], shapes[0]]
    cam = WF.Camera(origin=(1.0, 2.5, 9.0), target=(0.0, 0.8, 0.0), fov_deg=50.0, width=64, height=48)
    return dict(meshes=meshes, inst=inst, scene=M.MeshScene(meshes, inst), cam=cam, n_mat=2)


@pytest.mark.parametrize("rows", [(0, 48), (5, 17)])
def test_primary(primary_case, rows):
    pc = primary_case
    spp, seed, pas = 4, 77, 3
    sc = wf_scene(pc["cam"], pc["n_mat"])
    n = (rows[1] - rows[0]) * 64 * spp
    b, w = buffers(n + 11), buffers(n)
    pc["scene"].primary(sc, rows[0], rows[1], spp, seed, pas, b)
    p = lambda a: C.c_void_p(a.data_ptr())
    _lib.check(_lib.lib().bsdfd_wf_primary(C.byref(sc), rows[0], rows[1], spp, seed, pas, p(w["wi"]), p(w["wl"]), p(w["nrm"]),
                                           p(w["dir"]), p(w["mat"]), None))
    torch.cuda.synchronize()
    for k in ("wi", "wl", "nrm", "dir", "mat"):
        assert (b[k][n:] == -7).all(), k                                 # nothing behind the tile is written
    g = {k: v[:n].cpu().numpy() for k, v in b.items()}
    # dir and wl: bsdfd_wf_primary's bits
    for k in ("dir", "wl"):
        assert np.array_equal(g[k].view(np.uint32), w[k].cpu().numpy().view(np.uint32)), k
    assert (w["mat"] == pc["n_mat"] + 1).all()                           # (its balls are out of sight)
    org = np.tile(np.asarray(pc["cam"].origin, dtype=np.float32), (n, 1))
    ref = R.bvh_walk(pc["meshes"], pc["inst"], [pc["scene"].bvh(0), pc["scene"].bvh(1)], org, g["dir"])
    R.assert_marginal_cap(ref)
    et, eb = R.fp32_restatement_error(pc["meshes"], pc["inst"], org, g["dir"], ref)
    want = R.primary_arrays(pc["meshes"], pc["inst"], pc["n_mat"], g["dir"], ref, bary_tol=4 * eb)
    ok = ~ref["marginal"] & ~want["fragile"]
    print(f"primary rows {rows}: {n} paths, marginal {int(ref['marginal'].sum())}, fragile {int(want['fragile'].sum())}, "
          f"materials {np.bincount(g['mat'], minlength=4).tolist()}, bary bound {4 * eb:.3e}")
    assert want["fragile"].mean() <= 0.03                                # (a condition on this test's own scene and camera)
    assert np.array_equal(g["mat"][ok], want["material"][ok])
    counts = np.bincount(g["mat"], minlength=pc["n_mat"] + 2)
    if rows == (0, 48):
        assert (counts > 0).all()                                        # both materials, diffuse lanes and misses
    assert counts[:2].sum() > 0 and (counts[2:] > 0).all()               # (the tile: a material, diffuse lanes and misses)
    # nrm: a barycentric error e_b moves the mixed normal by at most 3 e_b |n_v| / |mix| before normalisation (the vertex normals
    # are unit vectors to 5e-5), fp32 rounding of the 3x3 product, the mix and the normalisation adds ~10 ulp: bound both
    tol_n = 2 * 3 * (4 * eb) / want["mix_len"].min() + 16 * 2.0 ** -24
    hit = g["mat"] <= pc["n_mat"]
    dn = np.abs(g["nrm"] - want["nrm"])[ok & hit]
    print(f"  nrm abs err {dn.max():.3e} (bound {tol_n:.3e})")
    assert dn.max() <= tol_n
    assert np.abs(np.linalg.norm(g["nrm"][hit].astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24
    lanes = g["mat"] < pc["n_mat"]
    assert (g["wi"][lanes, 2] > 0).all()                                 # every material lane, marginal or not
    # wi = -(d . s, d . t, d . n): the frame's s, t have derivatives bounded by 3 in n (|sign + n.z| >= 1), d is a unit vector
    dw = np.abs(g["wi"] - want["wi"])[ok & lanes]
    print(f"  wi abs err {dw.max():.3e} (bound {4 * tol_n:.3e})")
    assert dw.max() <= 4 * tol_n
    diffuse = g["mat"] == pc["n_mat"]
    assert (g["wi"][diffuse, 0:1] == g["wi"][diffuse]).all()              # the reflectance in all three slots
    assert np.array_equal(g["wi"][ok & diffuse], want["wi"][ok & diffuse].astype(np.float32))
    seen = set(np.unique(g["wi"][diffuse, 0]))
    assert seen <= {np.float32(0.4), np.float32(0.2), np.float32(0.18)} and {np.float32(0.4), np.float32(0.2)} <= seen   # both parities
    assert rows != (0, 48) or np.float32(0.18) in seen
    miss = g["mat"] == pc["n_mat"] + 1
    assert (g["nrm"][miss] == 0).all() and not (g["nrm"][~miss] == 0).all(1).any()
    if rows != (0, 48):                                                  # a tile is the rows of the whole film
        full = buffers(48 * 64 * spp)
        pc["scene"].primary(sc, 0, 48, spp, seed, pas, full)
        torch.cuda.synchronize()
        lo = rows[0] * 64 * spp
        for k in ("wi", "wl", "nrm", "dir", "mat"):
            assert torch.equal(full[k][lo:lo + n], b[k][:n]), k
    # an instance whose material is not below n_materials is refused
    with pytest.raises(RuntimeError, match="n_materials"):
        pc["scene"].primary(wf_scene(pc["cam"], 1), rows[0], rows[1], spp, seed, pas, b)


def test_fixture_scene_against_the_fp64_walk():
    names, cam, scene, _ = M.mesh_scene_from_matpreview_xml(SCENE_FILE, MESH_FILE, 64, 48)
    assert len(scene.instances) == 25
    sc = wf_scene(cam, len(names))
    n = 64 * 48
    b = buffers(n)
    scene.primary(sc, 0, 48, 1, 5, 0, b)
    d = b["dir"].cpu().numpy()
    org = np.tile(np.asarray(cam.origin, dtype=np.float32), (n, 1))
    t, prim, bary, occ = cast(scene, org, d)
    ref = R.bvh_walk(scene.meshes, scene.instances, [scene.bvh(k) for k in range(3)], org, d)
    et, eb = R.fp32_restatement_error(scene.meshes, scene.instances, org, d, ref)
    print(f"fixture scene: hits per instance {np.bincount(ref['prim'][:, 0] + 1, minlength=26).tolist()}")
    compare((t, prim, bary), ref, et, eb, "fixture scene 64x48x1")
    assert np.array_equal(occ, (t < R.NOTHING).astype(np.uint8))
    kinds = np.array([0 if i.material is not None else 1 for i in scene.instances])
    seen = kinds[ref["prim"][ref["prim"][:, 0] >= 0, 0]]
    assert (seen == 0).sum() > 100 and (seen == 1).sum() > 100           # shells and the floor are both in the picture
    mat = b["mat"].cpu().numpy()
    ok = ~ref["marginal"]
    want = np.array([i.material if i.material is not None else len(names) for i in scene.instances] + [len(names) + 1])
    assert np.array_equal(mat[ok], want[ref["prim"][ok, 0]])


# ---- the renderer ----
@pytest.fixture(scope="module")
def two_shells():
    names, _, full, albedo = M.mesh_scene_from_matpreview_xml(SCENE_FILE, MESH_FILE, 64, 48)
    shells = [i for i in full.instances if i.material is not None][:2]
    plane = next(i for i in full.instances if i.checker is not None)
    inst = [M.Instance(s.mesh, s.to_world, material=k) for k, s in enumerate(shells)] + [plane]
    cam = WF.Camera(origin=(1.0, 1.05, -1.5), target=(-3.5, 0.75, -1.5), fov_deg=40.0, width=64, height=48)
    return dict(scene=M.MeshScene(full.meshes, inst), cam=cam, env=WF.make_sky(64, 128, seed=5), albedo=albedo[:2])


@pytest.mark.parametrize("table", ["disk", "analytic"])
def test_mesh_array_renderer(two_shells, table):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    ts = two_shells
    dev()
    kw = {}
    if table == "disk":
        tab = MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS[:2]])
    else:
        from bsdf_diffusion_sampling_amd.analytic import ground_truth_for
        stems = ["bsdf_13", "bsdf_24"]
        tab = MaterialTable([s + "_spherical" for s in stems])
        kw = dict(ground_truth=ground_truth_for(stems), ball_albedo=ts["albedo"])
    r = M.MeshArrayRenderer(tab, ts["scene"], camera=ts["cam"], env=ts["env"], **kw)
    film = r.render(1, 4, seed=3)
    tile = r.render(1, 4, seed=3, rows=(5, 17))
    torch.cuda.synchronize()
    f = film.cpu().numpy()
    assert f.shape == (48, 64, 3) and np.isfinite(f).all() and (f >= 0).all() and f.max() > 0
    assert np.array_equal(tile.cpu().numpy().view(np.uint32), f[5:17].view(np.uint32))   # a tile is the rows of the whole film
    b = r.primary(0, 48, 4, 3, 0)
    mat = b["mat"].clone()
    plan = tab.bucket(mat, extra_bins=2)
    counts = plan[1]
    print(f"renderer [{table}]: bucket counts {counts}")
    assert len(counts) == 4 and all(c > 0 for c in counts)               # both shells, then floor lanes, then misses
    # pixels whose four paths all miss: what ArrayRenderer writes for the same camera with nothing in sight
    sky = WF.ArrayRenderer(tab, [(0.0, -1e6, 0.0)] * 2, [1.0] * 2, camera=ts["cam"], env=ts["env"], floor=False).render(1, 4, seed=3)
    torch.cuda.synchronize()
    all_miss = (mat.view(48, 64, 4) == 3).all(2).cpu().numpy()
    assert all_miss.sum() > 50 and (~all_miss).sum() > 500
    assert np.array_equal(f[all_miss].view(np.uint32), sky.cpu().numpy()[all_miss].view(np.uint32))


def test_mesh_array_renderer_refusals(two_shells):
    from bsdf_diffusion_sampling_amd.materials import MaterialTable
    dev()
    ts = two_shells
    with pytest.raises(ValueError, match="cover"):
        M.MeshArrayRenderer(MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS[:3]]), ts["scene"], camera=ts["cam"])
    tab = MaterialTable([m + "_disk" for m in WF.ARRAY0_MATERIALS[:2]])
    with pytest.raises(ValueError, match="MeshScene"):
        M.MeshArrayRenderer(tab, [(0, 0, 0)] * 2, camera=ts["cam"])
    inst = ts["scene"].instances
    gap = M.MeshScene(ts["scene"].meshes, [M.Instance(inst[0].mesh, inst[0].to_world, material=1), inst[2]])
    with pytest.raises(ValueError, match="cover"):
        M.MeshArrayRenderer(tab, gap, camera=ts["cam"])
    with pytest.raises(ValueError, match="ball_albedo"):
        M.MeshArrayRenderer(tab, ts["scene"], camera=ts["cam"], ball_albedo=ts["albedo"])
