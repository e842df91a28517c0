"""CPU side of Russian roulette and unbounded depth in the array-scene path tracer (bsdf_diffusion_sampling_amd/pathtrace.py,
csrc/bounce.hip): the export, the reader of the reference's integrator settings, the argument checks, and the reference rule of
tests/bounce_ref.py held to itself — unbiased on the variate grid, the same decisions in fp32 and fp64 on every row of a
test wavefront that exercises every outcome, and a mean that moves when the 1/q is left out."""
import os

import numpy as np
import pytest

import bounce_ref as B
import pass_replay as PR
import pathtrace_ref as R
import pathtrace_rr_ref as RR
from test_pass_replay_cpu import ORDER
from test_pathtrace_cpu import STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, PASS = 0x1234567890ABCDEF, 3
# The seed of ``pathtrace_rr_ref.rr_wavefront`` for the kernel tests.  With beta log-uniform in [1e-3, 2] the share of continuing
# rows whose q is clamped at 0.95 is 8 % in expectation over this wavefront (floor rows, reflectance 0.4 / 0.2, never are; a proxy
# ball row is with probability 0.11, a ground-truth one 0.09); of the seeds 0..1999 seven reach 10.4 %, 97 is the first of them
# (103 of 962 rows).  Every seed tried decides the same in fp32 and fp64 on every row.
WAVEFRONT_SEED = 97
# the unbiasedness test of tests/test_gpu_pathtrace_rr.py: the 5-ball scene from the low camera, 120x90, constant environment
UNBIASED = dict(w=120, h=90, spp=4, passes=64, max_depth=6, albedo=(0.5, 0.45, 0.4))


def rr_vertices(with_f=True):
    v = RR.rr_wavefront(R.synthetic_vertices(), WAVEFRONT_SEED)
    return v if with_f else {k: a for k, a in v.items() if k not in ("f_o", "f_l")}


def unbiasedness_scene(w=UNBIASED["w"], h=UNBIASED["h"]):
    """The oracle's scene dict of what tests/test_gpu_pathtrace_rr.py renders for the unbiasedness test."""
    from bsdf_diffusion_sampling_amd import wavefront as WF
    _, centers, radii = WF.array0_scene(w, h)
    cam = WF.Camera(origin=(1.5, 1.2, 3.0), target=(-1.8, 0.33, -1.8), fov_deg=40.0, width=w, height=h)
    return PR.scene_dict(cam, [centers[i] for i in ORDER], [radii[i] for i in ORDER], albedo=UNBIASED["albedo"])


def test_library_exports_bounce_rr_without_a_new_abi():
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    name = "bsdfd_wf_bounce_rr"
    assert name in _lib.EXPORTS and getattr(L, name).argtypes and f"int {name}(" in hdr
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert name + "()" in note
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr
    # bsdfd_wf_bounce_env's arguments, then rr_depth, then the stream
    env_args, rr_args = L.bsdfd_wf_bounce_env.argtypes, L.bsdfd_wf_bounce_rr.argtypes
    assert list(rr_args) == list(env_args[:-1]) + [_lib.C.c_int32, env_args[-1]] and len(rr_args) == 28
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    assert os.path.join(csrc, "bounce.hip") in _lib.SRC_PATHS and os.path.exists(os.path.join(csrc, "bounce.hip"))
    decl = hdr[hdr.index(f"int {name}("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl.endswith("const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth, void* hip_stream)")


XML = """<scene version="0.5.0">
    <integrator type="path">
        <integer name="{depth_name}" value="{depth}"/>{rr}
    </integrator>
    <sensor type="perspective"><integer name="maxDepth" value="77"/></sensor>
</scene>
"""
XML_DEFAULTS = """<scene version="3.0.0">
    <default name="spp" value="64"/>
    <default name="max_depth" value="-1"/>
    <integrator type="path">
        <integer name="max_depth" value="$max_depth"/>
    </integrator>
</scene>
"""


def test_integrator_from_matpreview_xml(tmp_path):
    from bsdf_diffusion_sampling_amd.pathtrace import integrator_from_matpreview_xml

    def read(text):
        p = tmp_path / "scene.xml"
        p.write_text(text)
        return integrator_from_matpreview_xml(str(p))
    assert read(XML.format(depth_name="maxDepth", depth=2, rr="")) == (1, 5)       # Mitsuba counts segments, the renderer vertices
    assert read(XML.format(depth_name="maxDepth", depth=-1, rr="")) == (None, 5)   # unbounded; rrDepth: Mitsuba's default
    assert read(XML.format(depth_name="maxDepth", depth=-1, rr='\n        <integer name="rrDepth" value="3"/>')) == (None, 3)
    assert read(XML.format(depth_name="max_depth", depth=7, rr='\n        <integer name="rr_depth" value="9"/>')) == (6, 9)
    assert read(XML_DEFAULTS) == (None, 5)                                         # scene_measured.xml's form
    assert read("<scene><integrator type='path'/></scene>") == (None, 5)           # Mitsuba's defaults
    for bad in (XML.format(depth_name="maxDepth", depth=1, rr=""), XML.format(depth_name="maxDepth", depth=0, rr=""),
                XML.format(depth_name="maxDepth", depth=4, rr='<integer name="rrDepth" value="0"/>'),
                XML_DEFAULTS.replace('<default name="max_depth" value="-1"/>', "")):
        with pytest.raises(ValueError):
            read(bad)


def test_renderer_argument_checks():
    """The constructor refuses its arguments before it touches a device."""
    from bsdf_diffusion_sampling_amd.pathtrace import PathArrayRenderer
    for bad in (0, -1):
        with pytest.raises(ValueError, match="rr_depth must be >= 1"):
            PathArrayRenderer(None, [], [], max_depth=4, rr_depth=bad)
    with pytest.raises(ValueError, match="needs rr_depth"):
        PathArrayRenderer(None, [], [], max_depth=None)
    with pytest.raises(ValueError, match="needs occlusion"):
        PathArrayRenderer(None, [], [], max_depth=None, rr_depth=5, occlusion=False)
    with pytest.raises(ValueError, match="max_depth must be >= 1"):
        PathArrayRenderer(None, [], [], max_depth=0, rr_depth=5)
    assert PathArrayRenderer.DEPTH_CAP == 1024


@pytest.mark.parametrize("q", [0.95, 0.5, 1.0 / 3.0, 0.1, 1e-3, 3e-6, float(np.float32(0.95)), 0.7071067811865476])
def test_rule_is_unbiased_on_the_variate_grid(q):
    """u = k 2^-24, k = 0 .. 2^24 - 1, survives iff u < q: ceil(q 2^24) of the 2^24 variates do, so the estimator's expectation
    P(survive) / q is within 2^-24 / q of 1 — and the reference's own comparison counts exactly that many."""
    p = np.ceil(q * 2.0 ** 24) / 2.0 ** 24
    assert abs(p / q - 1.0) <= 2.0 ** -24 / q
    k = int(np.ceil(q * 2.0 ** 24))
    u = (np.arange(max(k - 3, 0), min(k + 3, 1 << 24)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float64)
    assert np.array_equal(u < q, np.arange(max(k - 3, 0), min(k + 3, 1 << 24)) < k)


def test_variates_replay_philox_and_wrap_the_low_counter_word():
    from oracle.wavefront_oracle import philox4x32
    n = 256
    u = B.variates(SEED, PASS, 2, RR.OFFSET, n)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) > n - 4
    for row in (0, 99, 100, 255):           # row 100 is global path 2^32: low word 0, high word 1
        gp = RR.OFFSET + row
        w = philox4x32(SEED & 0xFFFFFFFF, SEED >> 32, np.array([gp & 0xFFFFFFFF], np.uint64), np.array([gp >> 32], np.uint64), PASS,
                       0x526F756C + 2)
        assert u[row] == np.float32(int(w[0][0]) >> 8) * np.float32(2.0 ** -24)
    assert (RR.OFFSET + 100) >> 32 == 1 and (RR.OFFSET + 99) >> 32 == 0
    assert not np.array_equal(u, B.variates(SEED, PASS, 3, RR.OFFSET, n))


@pytest.mark.parametrize("bounce", [0, 2])
def test_wavefront_is_fit_for_purpose_and_decides_the_same_in_fp32_and_fp64(bounce):
    """Among the rows of the test wavefront that would continue: >= 10 % clamped at 0.95, >= 10 % survive unclamped, >= 10 % are
    killed, some have q = 0; and the reference's fp32 run decides as its fp64 run does on EVERY row (with and without f)."""
    env = R.synthetic_env()
    for with_f in (True, False):
        v = rr_vertices(with_f)
        args = (R.SYNTH_SCENE, env, "cosine", bounce, False, True, SEED, PASS, RR.OFFSET, *[v.get(k) for k in STATE])
        a, b = B.bounce(*args, rr_depth=1), B.bounce(*args, rr_depth=1, dtype=np.float32)
        would, q = a["would"], a["q"]
        share = lambda rows: (would & rows).sum() / would.sum()
        clamped, free, killed = share(q == B.Q_MAX), share(a["survive"] & (q < B.Q_MAX)), share(a["killed"])
        zero = int((would & (q == 0)).sum())
        print(f"bounce {bounce} f={with_f}: {int(would.sum())} rows would continue: clamped {clamped:.3f}, survive unclamped {free:.3f}, "
              f"killed {killed:.3f}, q = 0 on {zero}")
        assert would.sum() > 900
        assert np.array_equal(a["would"], b["would"]) and np.array_equal(a["survive"], b["survive"])
        assert np.array_equal(a["material"], b["material"])
        assert np.abs(b["beta"][a["survive"]].astype(np.float64) - a["beta"][a["survive"]]).max() < 2e-6
        assert clamped >= 0.10 and free >= 0.10 and killed >= 0.10
        if with_f:
            assert zero >= 8 and a["killed"][would & (q == 0)].all()
        # killed rows keep their inputs, survivors carry beta thr / q, rad is the plain bounce's
        plain = B.bounce(*args)
        for k in RR.KEPT:
            assert np.array_equal(a[k][a["killed"]], v[k][a["killed"]].astype(np.float64)), k
        assert (a["material"][a["killed"]] == len(R.SYNTH_SCENE["spheres"]) + 1).all()
        assert np.array_equal(a["rad"], plain["rad"], equal_nan=True)
        s = a["survive"]
        assert np.allclose(a["beta"][s] * q[s, None], plain["beta"][s], rtol=1e-12, atol=0)
        for k in ("org", "nrm", "wi", "wl", "material"):
            assert np.array_equal(a[k][s], plain[k][s]), k
        assert np.isfinite(a["beta"][s]).all()


def test_roulette_is_inactive_before_rr_depth_and_at_last():
    env = R.synthetic_env()
    v = rr_vertices()
    tail = [v.get(k) for k in STATE]
    for rr_depth, bounce, last in ((4, 2, False), (1, 0, True), (3, 2, True)):
        a = B.bounce(R.SYNTH_SCENE, env, "cosine", bounce, last, True, SEED, PASS, RR.OFFSET, *tail, rr_depth=rr_depth)
        plain = B.bounce(R.SYNTH_SCENE, env, "cosine", bounce, last, True, SEED, PASS, RR.OFFSET, *tail)
        assert not a["killed"].any()
        for k in ("org", "nrm", "wi", "wl", "material", "beta", "rad"):
            assert np.array_equal(a[k], plain[k], equal_nan=True), k
    a = B.bounce(R.SYNTH_SCENE, env, "cosine", 2, False, True, SEED, PASS, RR.OFFSET, *tail, rr_depth=3)       # bounce + 1 == rr_depth: active
    assert a["killed"].sum() > 100


def test_leaving_out_the_division_moves_the_mean():
    """The power of the unbiasedness test of tests/test_gpu_pathtrace_rr.py, in the reference: its scene (albedo <= 0.5, floor 0.4 /
    0.2, unit environment), rr_depth = 1, max_depth = 6, the stand-in sampler of pass_replay.mock_answers.  The GPU test compares
    two runs of 64 passes at 4 spp with the tolerance 4 sqrt(se_a^2 + se_b^2), se = (standard deviation of the per-pass image
    means) / sqrt(64).  Here that standard deviation comes from 8 such passes, and the shift of the image mean from 8 passes at
    1 spp run twice on the same draws, with and without the 1/q (the shift does not depend on spp).  The shift must exceed ten
    times the tolerance.  The same experiment at full size (64 passes at 4 spp, both ways), run once: shift 5.1e-3 / 4.6e-3 /
    4.0e-3 per channel against a tolerance of 3.4e-4 / 3.3e-4 / 3.1e-4, a factor of 14.9 / 13.9 / 12.8.  (Eight passes estimate
    a standard deviation roughly: this test's tolerance comes out at 1.9e-4 / 1.7e-4 / 1.6e-4, a factor of 24 .. 27.)"""
    scene = unbiasedness_scene()
    env = np.ones((8, 16, 3), np.float32)

    def image_mean(p, spp, scale):
        out = PR.reference_pass(scene, env, "cosine", None, None, 0, scene["height"], spp, 4, p, UNBIASED["max_depth"], True,
                                PR.mock_answers(11 + p), rr_depth=1, scale=scale)
        return out["film"].reshape(-1, 3).mean(0)
    shift = np.mean([image_mean(p, 1, True) - image_mean(p, 1, False) for p in range(8)], axis=0)
    sd = np.std([image_mean(p, UNBIASED["spp"], True) for p in range(8)], axis=0, ddof=1)
    tolerance = 4.0 * np.sqrt(2.0) * sd / np.sqrt(UNBIASED["passes"])
    print(f"shift {shift}, tolerance of the GPU test {tolerance}, ratio {shift / tolerance}")
    assert (shift > 10.0 * tolerance).all()
