"""CPU tests of the measured BSDF's own importance sampler (csrc/measured_dev.h: measured_sample / measured_pdf): the numpy
restatement the GPU tests hold the kernels to (tests/measured_sampling_ref.py) against the fp64 oracle's warp, its round trip and
its Jacobian; the new symbols; the loader's handling of the optional ``luminance`` field."""
import ctypes as C
import os

import numpy as np
import pytest

from bsdf_diffusion_sampling_amd import measured_synth
from oracle import measured_oracle as M

import measured_sampling_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "chm_orange_rgb.bsdf")
SYMBOLS = ("bsdfd_measured_sample", "bsdfd_measured_pdf", "bsdfd_measured_sample_table", "bsdfd_measured_pdf_table")
EIO, EHIP = 3, 2


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("measured_sampling")
    aniso = measured_synth.write_anisotropic(str(d / "aniso_rgb.bsdf"))
    iso = measured_synth.write_isotropic(str(d / "iso_rgb.bsdf"))
    fields = dict(M.read_tensor_file(iso))
    no_lum = str(d / "iso_nolum_rgb.bsdf")
    measured_synth.write_tensor_file(no_lum, {k: v for k, v in fields.items() if k != "luminance"})
    rank3 = str(d / "iso_rank3_rgb.bsdf")
    measured_synth.write_tensor_file(rank3, {k: (v[0] if k == "luminance" else v) for k, v in fields.items()})
    return {"fixture": FIXTURE, "aniso": aniso, "iso": iso, "no_lum": no_lum, "rank3": rank3}


@pytest.mark.parametrize("which,field", [("fixture", "vndf"), ("fixture", "luminance"), ("aniso", "vndf"), ("aniso", "luminance")])
def test_warp_restates_the_oracle(files, which, field):
    """fp64: sample / invert / eval of the helper's warp agree with oracle.measured_oracle.Marginal2D to 1e-9."""
    t = M.read_tensor_file(files[which])
    phi_i, theta_i = t["phi_i"].astype(np.float64), t["theta_i"].astype(np.float64)
    mine = R.Warp(t[field], phi_i, theta_i, np.float64)
    orc = M.Marginal2D(t[field], (phi_i, theta_i), normalize=True, sampling=True)
    g = np.random.default_rng(3)
    n = 4096
    u = g.random((n, 2))
    param = (g.uniform(phi_i[0], phi_i[-1], n) if len(phi_i) > 1 else np.zeros(n), g.uniform(0.0, np.pi / 2, n))
    pos, pdf = mine.sample((u[:, 0], u[:, 1]), param)
    pos_o, pdf_o = orc.sample((u[:, 0], u[:, 1]), param)
    # The oracle's `sample` solves its quadratics with the cancelling root, which costs it up to 4e-9 of position on a few rows
    # per thousand of the fixture's luminance table (measured: 3 of these 4 096, and ITS OWN round trip invert(sample(u)) misses
    # u by the same amount there; the helper's round trip holds to 1e-14).  So sample-against-sample is held to 1e-9 on the rows
    # where the oracle agrees with itself, and on EVERY row the oracle's invert, which has no such root, must take the helper's
    # positions back to u to 1e-9.
    (b0, b1), _ = orc.invert(pos_o, param)
    sane = (np.abs(b0 - u[:, 0]) < 1e-10) & (np.abs(b1 - u[:, 1]) < 1e-10)
    assert sane.mean() > 0.99, sane.mean()
    assert np.abs(pos[0] - pos_o[0])[sane].max() < 1e-9 and np.abs(pos[1] - pos_o[1])[sane].max() < 1e-9
    assert np.abs(pdf - pdf_o)[sane].max() < 1e-9 * max(1.0, np.abs(pdf_o).max())
    (b0, b1), bpdf = orc.invert(pos, param)
    assert np.abs(b0 - u[:, 0]).max() < 1e-9 and np.abs(b1 - u[:, 1]).max() < 1e-9
    assert np.abs(bpdf - pdf).max() < 1e-9 * max(1.0, np.abs(pdf_o).max())
    s, ipdf = mine.invert((u[:, 0], u[:, 1]), param)
    s_o, ipdf_o = orc.invert((u[:, 0], u[:, 1]), param)
    assert np.abs(s[0] - s_o[0]).max() < 1e-9 and np.abs(s[1] - s_o[1]).max() < 1e-9
    assert np.abs(ipdf - ipdf_o).max() < 1e-9 * max(1.0, np.abs(ipdf_o).max())
    assert np.abs(mine.eval((u[:, 0], u[:, 1]), param) - orc.eval((u[:, 0], u[:, 1]), param)).max() < 1e-9 * max(1.0, np.abs(ipdf_o).max())
    # ... and the warp inverts itself
    back, _ = mine.invert(pos, param)
    assert np.abs(back[0] - u[:, 0]).max() < 1e-12 and np.abs(back[1] - u[:, 1]).max() < 1e-12


@pytest.mark.parametrize("which", ["fixture", "aniso", "iso", "no_lum"])
def test_pdf_of_a_sampled_direction_is_the_samplers_pdf(files, which):
    ref = R.MeasuredSampler(files[which], np.float64)
    g = np.random.default_rng(5)
    n = 4096
    wi, u = measured_synth.dirs(g, n, 0.02), g.random((n, 2))
    wo, pdf, weight = ref.sample(wi, u)
    back = ref.pdf(wi, wo)
    ok = pdf > 0
    assert ok.mean() > 0.5 and np.isfinite(wo).all() and np.isfinite(weight).all()
    assert (np.abs(back[ok] - pdf[ok]) / pdf[ok]).max() < 1e-9, (np.abs(back[ok] - pdf[ok]) / pdf[ok]).max()
    # weight * pdf is f cos at the sampled direction
    f = ref.eval(wi, wo)
    assert np.abs(weight[ok] * pdf[ok, None] - f[ok]).max() < 1e-9 * max(1.0, np.abs(f).max())
    assert (back[~ok & (wo[:, 2] <= 0)] == 0).all()


@pytest.mark.parametrize("which", ["fixture", "aniso", "iso"])
def test_pdf_is_the_inverse_area_of_the_map(files, which):
    """|(d wo/d u0 x d wo/d u1) . wo| * pdf = 1: the finite-difference area element of u -> wo against the stated density."""
    ref = R.MeasuredSampler(files[which], np.float64)
    g = np.random.default_rng(6)
    n, h = 4096, 1e-6
    wi, u = measured_synth.dirs(g, n, 0.3), g.uniform(0.02, 0.98, (n, 2))
    wo, pdf, _ = ref.sample(wi, u)
    d0 = (ref.sample(wi, u + [h, 0])[0] - ref.sample(wi, u - [h, 0])[0]) / (2 * h)
    d1 = (ref.sample(wi, u + [0, h])[0] - ref.sample(wi, u - [0, h])[0]) / (2 * h)
    area = np.abs((np.cross(d0, d1) * wo).sum(1))
    ok = pdf > 0
    assert abs(np.median(area[ok] * pdf[ok]) - 1.0) < 1e-4, np.median(area[ok] * pdf[ok])


def test_library_exports_and_binds_the_sampling_entry_points():
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    hdr = open(_lib.INCLUDE_DIR + "/bsdfd.h").read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and name + "(" in hdr
        assert getattr(L, name).argtypes, name
    assert len(L.bsdfd_measured_sample.argtypes) == 10 and len(L.bsdfd_measured_pdf.argtypes) == 7
    assert len(L.bsdfd_measured_sample_table.argtypes) == 11 and len(L.bsdfd_measured_pdf_table.argtypes) == 8
    assert L.bsdfd_abi_version() == 8 == _lib.ABI_VERSION
    # argument checks that run before any device work
    assert L.bsdfd_measured_sample(None, None, None, None, 0, None, None, None, None, None) == 1
    assert "null handle" in L.bsdfd_last_error().decode()
    assert L.bsdfd_measured_pdf_table(None, None, None, None, None, 0, None, None) == 1
    assert "null measured table" in L.bsdfd_last_error().decode()


def test_loader_takes_files_without_luminance_and_rejects_a_malformed_one(files):
    """The file checks come before the loader touches a device, so they run here: a file without the optional field passes them
    (the call then succeeds on a GPU machine and fails with a HIP error, not a file error, without one), a rank-3 `luminance`
    does not."""
    from bsdf_diffusion_sampling_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.bsdfd_measured_create_from_file(files["rank3"].encode(), C.byref(h))
    assert rc == EIO and not h.value and "luminance must be an fp32 field of rank 4" in L.bsdfd_last_error().decode()
    for which in ("no_lum", "iso"):
        rc = L.bsdfd_measured_create_from_file(files[which].encode(), C.byref(h))
        assert rc in (0, EHIP), (which, rc, L.bsdfd_last_error().decode())
        if rc == 0:
            lum = C.c_int32(-1)
            assert L.bsdfd_measured_has_luminance(h, C.byref(lum)) == 0 and lum.value == (which == "iso")
            L.bsdfd_measured_destroy(h)
            h = C.c_void_p()
    # wrong leading dimensions
    fields = dict(M.read_tensor_file(files["iso"]))
    fields["luminance"] = np.concatenate([fields["luminance"]] * 2, 1)
    bad = os.path.join(os.path.dirname(files["iso"]), "iso_badlum_rgb.bsdf")
    measured_synth.write_tensor_file(bad, fields)
    rc = L.bsdfd_measured_create_from_file(bad.encode(), C.byref(h))
    assert rc == EIO and "luminance does not match" in L.bsdfd_last_error().decode()


def test_python_calls_check_their_tensors():
    torch = pytest.importorskip("torch")
    from bsdf_diffusion_sampling_amd.measured import MeasuredBSDF, MeasuredTable
    v = torch.zeros(8, 3)
    bare = MeasuredBSDF.__new__(MeasuredBSDF)      # no file, no handle: the tensor checks come before the native call
    with pytest.raises(ValueError, match="must be a contiguous CUDA tensor"):
        bare.sample_t(v, torch.zeros(8, 2))
    with pytest.raises(ValueError, match="must be a contiguous CUDA tensor"):
        bare.pdf_t(v, v)
    tab = MeasuredTable([None, None])
    ids = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="u must be an fp32 tensor \\[N,2\\]"):
        tab.sample_t(ids, v, v)
    with pytest.raises(ValueError, match="u has 5 rows"):
        tab.sample_t(ids, v, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="wo has 5 rows"):
        tab.pdf_t(ids, v, v[:5])
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        tab.pdf_t(ids, v, v)


def test_pdf_matches_the_recorded_mitsuba_pdf():
    """The day a machine with Mitsuba records tests/golden/mitsuba_measured_eval.npz (tests/golden/make_mitsuba_golden.py), the
    restatement's pdf is pinned to Mitsuba's."""
    path = os.path.join(HERE, "golden", "mitsuba_measured_eval.npz")
    if not os.path.exists(path):
        pytest.skip("no Mitsuba golden recorded (tests/golden/make_mitsuba_golden.py needs Mitsuba)")
    z = np.load(path)
    ref = R.MeasuredSampler(FIXTURE, np.float64)
    got, want = ref.pdf(z["wi"], z["wo"]), z["pdf"]
    ok = want > 0
    assert (np.abs(got[ok] - want[ok]) / want[ok]).max() < 1e-4
