"""CPU side of transmission through the balls of the array scene (``PathArrayRenderer(transmission=True)``:
``bsdfd_wf_bounce_transmit``, ``bsdfd_wf_sample_inside`` / ``_rows``): the three symbols without a new ABI, the constructor's
refusals before any device work, and the numpy references the GPU tests hold the kernels to (tests/bounce_transmit_ref.py) held
to themselves — the transmitting bounce in two precisions, the chord against the quadratic's far root, the inside sampler's
variates against the Philox counters the header documents."""
import os

import numpy as np
import pytest

import bounce_ref as B
import bounce_transmit_ref as T
import pathtrace_ref as R
from oracle.wavefront_oracle import philox4x32
from test_pathtrace_cpu import STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bsdfd_wf_bounce_transmit", "bsdfd_wf_sample_inside", "bsdfd_wf_sample_inside_rows")
SEED, PASS, OFFSET = 0x1234567890ABCDEF, 3, (1 << 32) - 2000


def test_library_exports_the_transmission_entry_points_without_a_new_abi():
    import ctypes as C
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr and name + "()" in note
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert L.bsdfd_wf_bounce_transmit.argtypes == L.bsdfd_wf_bounce_rows.argtypes
    inside = L.bsdfd_wf_sample_inside.argtypes
    assert inside == [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64] + [C.c_void_p] * 7
    assert L.bsdfd_wf_sample_inside_rows.argtypes == inside[:-1] + [C.c_void_p, C.c_int64, C.c_void_p]
    # none of them belongs to the four families whose launchers tests/test_launch_contract_cpu.py counts
    assert not any(name.startswith(p) for name in SYMBOLS
                   for p in ("bsdfd_analytic_", "bsdfd_measured_", "bsdfd_dielectric_", "bsdfd_principled_"))


def test_the_constructor_refuses_what_transmission_cannot_serve():
    """Every refusal, before the constructor touches a device (no table, no camera: nothing here could be built)."""
    from bsdf_diffusion_sampling_amd.analytic import Principled, RoughDielectric
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    glass, opaque = RoughDielectric(0.3), Principled(roughness=0.5)
    centers, radii = [(-0.7, 0.33, 0.0), (0.05, 0.33, 0.1)], [0.33, 0.33]
    table = [None, None]        # (only its length is read before the first refusal)
    ok = dict(max_depth=4, transmission=True, ground_truth={0: glass, 1: opaque})
    with pytest.raises(ValueError, match="needs ground truth"):                       # no ground truth at all
        PathArrayRenderer(table, centers, radii, **dict(ok, ground_truth=None))
    with pytest.raises(ValueError, match="needs ground truth"):
        PathArrayRenderer(table, centers, radii, **dict(ok, ground_truth={}))
    with pytest.raises(ValueError, match="AnalyticTable"):                            # a measured table's entries
        PathArrayRenderer(table, centers, radii, **dict(ok, ground_truth={0: object()}))
    with pytest.raises(ValueError, match="AnalyticTable"):                            # no lane-ordered table at all
        PathArrayRenderer(table, centers, radii, **dict(ok, fused_ground_truth=False))
    with pytest.raises(ValueError, match="max_depth > 1"):
        PathArrayRenderer(table, centers, radii, **dict(ok, max_depth=1))
    with pytest.raises(ValueError, match="occlusion"):                                # occlusion off
        PathArrayRenderer(table, centers, radii, **dict(ok, occlusion=False))
    touching = [(0.0, 0.33, 0.0), (0.66, 0.33, 0.0)]                                  # |c_i - c_j| == r_i + r_j
    with pytest.raises(ValueError, match="balls 0 and 1 touch or intersect"):
        PathArrayRenderer(table, touching, radii, **ok)
    with pytest.raises(ValueError, match="balls 0 and 1 touch or intersect"):
        PathArrayRenderer(table, [(0.0, 0.33, 0.0), (0.3, 0.5, 0.1)], radii, **ok)
    with pytest.raises(ValueError, match="ball 1 reaches below the floor"):
        PathArrayRenderer(table, [(-0.7, 0.33, 0.0), (0.05, 0.3299, 0.1)], radii, **ok)
    with pytest.raises(ValueError, match="ball 1 reaches below the floor"):           # ... given by position too
        PathArrayRenderer(table, [(-0.7, 0.33, 0.0), (0.05, 0.3299, 0.1)], radii, None, None, True, **ok)
    with pytest.raises(ValueError, match="max_depth must be >= 1"):                   # (the earlier checks still come first)
        PathArrayRenderer(table, touching, radii, **dict(ok, max_depth=0))


def test_inside_variates_are_the_documented_philox_words():
    """u_k = (word k >> 8) 2^-24 of philox(key = seed, counter = (path lo, path hi, pass, "Insd" + bounce)): exact fp32 numbers in
    [0, 1), keyed by the path, with the path index crossing 2^32 inside the wavefront."""
    assert T.TAG_INSIDE == int.from_bytes(b"Insd", "big") and T.TAG_INSIDE != B.TAG
    n, bounce = 4096, 2
    u = T.inside_variates(SEED, PASS, bounce, OFFSET, n)
    assert u.dtype == np.float32 and u.shape == (n, 3) and (u >= 0).all() and (u < 1).all()
    gp = np.uint64(OFFSET) + np.arange(n, dtype=np.uint64)
    assert (gp >> np.uint64(32)).min() == 0 and (gp >> np.uint64(32)).max() == 1
    w = philox4x32(SEED & 0xFFFFFFFF, SEED >> 32, gp & np.uint64(0xFFFFFFFF), gp >> np.uint64(32), PASS, T.TAG_INSIDE + bounce)
    for k in range(3):
        ints = (u[:, k].astype(np.float64) * 2.0 ** 24)
        assert np.array_equal(ints, (w[k] >> np.uint32(8)).astype(np.float64))
    # a draw of its own: another tag, another bounce, another pass all give other words
    assert not np.array_equal(u[:, 0], B.variates(SEED, PASS, bounce, OFFSET, n))
    assert not np.array_equal(u, T.inside_variates(SEED, PASS, bounce + 1, OFFSET, n))
    assert not np.array_equal(u, T.inside_variates(SEED, PASS + 1, bounce, OFFSET, n))
    assert np.array_equal(u[7:], T.inside_variates(SEED, PASS, bounce, OFFSET + 7, n - 7))      # keyed by the path, not the row


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_chord_lands_on_the_far_side_of_the_ball(dtype):
    """Random entry points and inward directions, d . n from -1 (through the centre) to -1e-4 (a grazing chord): the next vertex
    lies on the sphere, its wi.z < 0 and equals d . n of the entry (a chord meets the sphere at equal angles), and
    t = -2 (x - c) . d is the far root of the quadratic.

    fp64: the entry point is on the sphere to fp64 rounding and everything is held to 1e-10.  fp32: the statements in the kernel's
    own arithmetic on what the kernel sees — fp32 arrays, the entry point c + r n rounded to fp32, i.e. up to 1e-7 off the sphere.
    The quadratic's far root moves by (that offset) / |d . n| then, 1e-3 at the grazing end, and below |d . n| ~ 5e-4 the ray from
    a point just outside misses the sphere altogether; the chord does not care: it is held to the sphere within 2e-5 r, to
    wi.z = (x - c) . d / r < 0 within 2e-5, and to the root within 2e-5 where the offset cannot move the root further
    (|d . n| >= 0.05)."""
    g = np.random.default_rng(11)
    n = 6000
    cosines = np.concatenate([np.full(1000, -1.0), np.full(1000, -1e-4), -np.exp(g.uniform(np.log(1e-4), 0.0, n - 2000))])
    nrm = R._sphere_dirs(g, n)
    s, t = R._onb(nrm)
    phi = g.uniform(0, 2 * np.pi, n)
    sin = np.sqrt(np.maximum(1 - cosines ** 2, 0.0))
    d = (sin * np.cos(phi))[:, None] * s + (sin * np.sin(phi))[:, None] * t + cosines[:, None] * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = g.uniform(-1, 1, (n, 3))
    r = g.uniform(0.2, 0.5, n)
    x = c + r[:, None] * nrm
    if dtype is np.float32:
        c, r, d, x = (a.astype(np.float32).astype(np.float64) for a in (c, r, d, x))
    tol = 1e-10 if dtype is np.float64 else 2e-5
    tt, xv, nv, wi = T.chord(c, r, x, d, dtype)
    want_t = T.far_root(c, r, x, d)
    bn = ((x - c) * d).sum(1) / r
    on_sphere = np.abs(np.linalg.norm(xv.astype(np.float64) - c, axis=1) - r) / r
    steep = bn <= (-0.05 if dtype is np.float32 else 0.0)
    print(f"{np.dtype(dtype).name}: |x' - c| / r - 1 max {on_sphere.max():.1e}; t against the far root max "
          f"{np.abs(tt - want_t)[steep].max():.1e} on {int(steep.sum())} rows (chords {tt.min():.1e} .. {tt.max():.2f}); "
          f"wi.z - (x - c) . d / r max {np.abs(wi[:, 2] - bn).max():.1e}")
    assert on_sphere.max() < tol
    assert (tt > 0).all() and (wi[:, 2] < 0).all() and steep.sum() >= 2000 and (bn > -2e-4).sum() >= 1000
    assert np.abs(tt - want_t)[steep].max() < tol
    assert np.abs(wi[:, 2] - bn).max() < tol
    assert np.abs((np.asarray(wi, np.float64) ** 2).sum(1) - 1).max() < max(tol, 1e-6)
    if dtype is np.float64:
        assert np.abs(bn - cosines).max() < 1e-10


@pytest.mark.parametrize("rr_depth", [None, 1])
@pytest.mark.parametrize("mode", ["cosine"])
def test_transmitting_reference_decides_the_same_in_fp32_and_fp64(mode, rr_depth):
    """On the synthetic wavefront of the GPU test the fp32 and the fp64 run of the transmitting reference decide the material id
    alike on all but 0.1 % of the rows — the cap the device is held to — and the wavefront holds what the GPU test needs: every
    class of row, and at least 300 rows that enter or stay inside."""
    v, cls = T.synthetic_vertices()
    env = R.synthetic_env()
    n, n_b = len(v["material"]), len(R.SYNTH_SCENE["spheres"])
    a, b = (T.bounce(R.SYNTH_SCENE, env, mode, 2, False, True, SEED, PASS, OFFSET, *[v[k] for k in STATE], rr_depth=rr_depth, dtype=dt)
            for dt in (np.float64, np.float32))
    plain = B.bounce(R.SYNTH_SCENE, env, mode, 2, False, True, SEED, PASS, OFFSET, *[v[k] for k in STATE], rr_depth=rr_depth)
    differ = int((a["material"] != b["material"]).sum())
    inside = a["enter"] & (a["material"] <= n_b)
    print(f"rr_depth = {rr_depth}: {differ} of {n} rows decide differently in fp32; classes "
          + ", ".join(f"{k} {int(m.sum())}" for k, m in cls.items()) + f"; {int(a['enter'].sum())} rows trigger the rule, "
          f"{int(inside.sum())} enter or stay inside")
    assert differ <= n // 1000
    assert np.array_equal(a["enter"], b["enter"])
    assert all(m.sum() >= 30 for m in cls.values())
    assert inside.sum() >= 300
    # the rule triggers exactly on the rows with ground truth; the others end as they did
    assert np.array_equal(a["enter"], cls["with_gt"])
    assert (a["material"][cls["without_gt"] | cls["opaque"]] == n_b + 1).all()
    # a row that enters stays on its ball, inside, on the sphere, with beta = beta_in f_o / pdf_o [/ q]
    assert np.array_equal(a["material"][inside], v["material"][inside]) and (a["wi"][inside, 2] < 0).all()
    scale = 1.0 if rr_depth is None else 1.0 / a["q"][inside, None]
    want_beta = v["beta"][inside].astype(np.float64) * v["f_o"][inside].astype(np.float64) / v["pdf_o"][inside, None].astype(np.float64) * scale
    assert np.abs(a["beta"][inside] - want_beta).max() < 1e-12
    cs = np.asarray([c for c, _ in R.SYNTH_SCENE["spheres"]], np.float32).astype(np.float64)[v["material"][inside]]
    rs = np.asarray([r for _, r in R.SYNTH_SCENE["spheres"]], np.float32).astype(np.float64)[v["material"][inside]]
    assert np.abs(np.linalg.norm(a["org"][inside] - cs, axis=1) - rs).max() < 1e-12
    # everywhere else the transmitting reference IS the plain one; rad is the plain one's on every row
    rest = ~a["enter"]
    for k in ("org", "nrm", "wi", "wl", "material", "beta"):
        assert np.array_equal(a[k][rest], plain[k][rest], equal_nan=True), k
    assert np.array_equal(a["rad"], plain["rad"], equal_nan=True)
    if rr_depth is not None:
        assert (a["killed"] & a["enter"]).sum() >= 30 and np.array_equal(a["killed"] & rest, plain["killed"] & rest)


def test_last_ends_the_rows_that_would_enter():
    v, _ = T.synthetic_vertices()
    a = T.bounce(R.SYNTH_SCENE, R.synthetic_env(), "cosine", 2, True, True, SEED, PASS, OFFSET, *[v[k] for k in STATE])
    live = v["material"] <= len(R.SYNTH_SCENE["spheres"])
    assert a["enter"].sum() >= 300 and (a["material"][live] == len(R.SYNTH_SCENE["spheres"]) + 1).all()
