"""CPU tests of the mixed-material analytic table (csrc/analytic_table.hip, analytic.AnalyticTable): the symbols, the checks that
run before any device work, the two helpers that feed the array renderers, and the compiler's resource report of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from bsdf_diffusion_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bsdfd_analytic_table_create", "bsdfd_analytic_table_destroy", "bsdfd_analytic_eval_table",
           "bsdfd_analytic_sample_weight_table", "bsdfd_analytic_sample_table", "bsdfd_analytic_pdf_table")
KERNELS = ("analytic_eval_table_kernel", "analytic_weight_table_kernel", "analytic_sample_table_kernel", "analytic_pdf_table_kernel")
EINVAL = 1

SCENE = """<scene version="3.0.0">
  <integrator type="path"><integer name="max_depth" value="-1"/></integrator>
  <shape type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"/></shape>
  <shape type="obj">
    <transform name="to_world"><translate x="-4" y="1" z="0"/></transform>
    <bsdf type="mybsdf"><integer name='idx' value='21'/><vector name="albedo" value="0.1, 0.9, 0.9"/></bsdf>
  </shape>
  <shape type="obj">
    <transform name="to_world"><translate x="-3" y="2" z="0"/></transform>
    <bsdf type="mybsdf"><integer name='idx' value='25'/></bsdf>
  </shape>
  <shape type="obj">
    <transform name="to_world"><translate x="-2" y="3" z="0"/></transform>
    <bsdf type="mybsdf"><string name="filename" value="chm_orange_rgb"/><vector name="albedo" value="0.5 0.25 1"/></bsdf>
  </shape>
</scene>
"""


def test_library_declares_binds_and_exports_the_entry_points_without_a_new_abi():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bsdfd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes, name
        assert re.search(r"(int|void)\s+" + name + r"\(", hdr), name
    note = hdr[hdr.index("Added later WITHOUT a new version"):hdr.index("#define BSDFD_ABI_VERSION")]
    assert all(name + "()" in note for name in SYMBOLS)
    assert L.bsdfd_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define BSDFD_ABI_VERSION 8\n" in hdr
    for call in ("eval", "sample_weight", "sample", "pdf"):     # the measured table's argument lists
        assert list(getattr(L, f"bsdfd_analytic_{call}_table").argtypes) == list(getattr(L, f"bsdfd_measured_{call}_table").argtypes)
    # bsdfd_analytic_entry: kind, albedo[3], then the union of the two descriptors
    assert C.sizeof(_lib.AnalyticEntry) == 16 + 64 and _lib.AnalyticEntry.desc.offset == 16
    assert (_lib.ANALYTIC_NONE, _lib.ANALYTIC_PRINCIPLED, _lib.ANALYTIC_DIELECTRIC) == (0, 1, 2)
    for k, v in (("NONE", 0), ("PRINCIPLED", 1), ("DIELECTRIC", 2)):
        assert f"#define BSDFD_ANALYTIC_{k} {v}\n" in hdr
    csrc = os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc")
    src, host = os.path.join(csrc, "analytic_table.hip"), os.path.join(csrc, "analytic_host.h")
    assert src in _lib.SRC_PATHS and src not in _lib.FLOW_TUS and src not in _lib.KERNEL_SOURCES and os.path.exists(src)
    assert host in _lib.DEP_PATHS and host not in _lib.SRC_PATHS and os.path.exists(host)
    # the descriptor is derived in one place: neither single-material unit restates it
    for unit in ("principled.hip", "dielectric.hip", "analytic_table.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "analytic_host.h"' in text and "derive(const" not in text and "descriptor_error(const" not in text


def test_create_checks_its_arguments_before_any_device_work():
    from bsdf_diffusion_sampling_amd.analytic import reference_bsdf
    L = _lib.lib()
    t = C.c_void_p()

    def entries(*objs, albedo=(1.0, 1.0, 1.0)):
        recs = (_lib.AnalyticEntry * max(len(objs), 1))()
        for r, e in zip(recs, objs):
            r.albedo = (C.c_float * 3)(*albedo)
            if isinstance(e, _lib.Principled):
                r.kind, r.desc.principled = _lib.ANALYTIC_PRINCIPLED, e
            elif isinstance(e, _lib.Dielectric):
                r.kind, r.desc.dielectric = _lib.ANALYTIC_DIELECTRIC, e
            elif e is not None:
                r.kind = e
        return recs

    def refused(recs, n, word, out=t):
        rc = L.bsdfd_analytic_table_create(recs, n, None if out is None else C.byref(out))
        assert rc == EINVAL and word in L.bsdfd_last_error().decode(), (rc, L.bsdfd_last_error().decode())

    good = reference_bsdf(13)._desc
    refused(entries(good), 1, "null argument", out=None)
    refused(None, 1, "null entry array")
    refused(entries(good), 0, "[1, 65536]")
    refused(entries(good), 65537, "[1, 65536]")
    refused(entries(None, None), 2, "at least one")
    bad_eta = _lib.Principled((C.c_float * 3)(1, 1, 1), 0.5, 0.0, 0.0, 0.0, 0.9)
    refused(entries(good, None, bad_eta), 3, "entry 2: bsdfd_principled.eta")
    refused(entries(good, _lib.Dielectric(0.3, 1.5, 1, 0)), 2, "entry 1: bsdfd_dielectric.distribution")
    refused(entries(good, _lib.Dielectric(-0.3, 1.5, 0, 0)), 2, "entry 1: bsdfd_dielectric: alpha")
    refused(entries(good, 7), 2, "entry 1: kind")
    refused(entries(good, albedo=(1.0, -0.5, 1.0)), 1, "entry 0: albedo")
    refused(entries(good, albedo=(1.0, float("nan"), 1.0)), 1, "entry 0: albedo")
    refused(entries(good, albedo=(float("inf"), 1.0, 1.0)), 1, "entry 0: albedo")
    assert not t.value
    L.bsdfd_analytic_table_destroy(None)       # destroy(NULL) is a no-op
    # the launch calls refuse a null table before anything else
    assert L.bsdfd_analytic_eval_table(None, None, None, None, None, 0, None, None, None, None) == EINVAL
    assert L.bsdfd_analytic_pdf_table(None, None, None, None, None, 0, None, None) == EINVAL
    assert b"null analytic table" in L.bsdfd_last_error()


def test_python_table_refuses_wrong_entries_and_albedos_without_a_device():
    from bsdf_diffusion_sampling_amd.analytic import AnalyticTable, FullSphereGroundTruth, reference_bsdf
    from bsdf_diffusion_sampling_amd.ground_truth import RowKernels
    assert issubclass(AnalyticTable, RowKernels) and not issubclass(AnalyticTable, FullSphereGroundTruth)
    assert (AnalyticTable.U_COLS, AnalyticTable.FIREFLY, AnalyticTable.MAX_MATERIALS) == (3, 3.5, 65536)
    a, b = reference_bsdf(13), reference_bsdf(24)
    with pytest.raises(ValueError, match="entries are"):
        AnalyticTable([a, "bsdf_13"])
    with pytest.raises(ValueError, match="entries are"):
        AnalyticTable([a, a._desc])
    with pytest.raises(ValueError, match="entries"):
        AnalyticTable([])
    with pytest.raises(ValueError, match="entries"):
        AnalyticTable([a] * 65537)
    with pytest.raises(ValueError, match="albedo"):
        AnalyticTable([a, b], albedo=[(1, 1, 1)])
    with pytest.raises(ValueError, match="albedo"):
        AnalyticTable([a, b], albedo=[(1, 1, 1), (1, 1)])
    with pytest.raises(ValueError, match="albedo"):
        AnalyticTable([a, b], albedo=[(1, 1, 1), (1, 1, 1, 1)])
    # what only the library can tell: still an error, never a table
    with pytest.raises(RuntimeError, match="at least one"):
        AnalyticTable([None, None])
    with pytest.raises(RuntimeError, match="entry 1: albedo"):
        AnalyticTable([a, b], albedo=[(1, 1, 1), (1, -1, 1)])


def test_ground_truth_for_and_the_albedos_of_a_scene_file(tmp_path):
    from bsdf_diffusion_sampling_amd import wavefront as WF
    from bsdf_diffusion_sampling_amd.analytic import Principled, RoughDielectric, ground_truth_for
    path = tmp_path / "scene.xml"
    path.write_text(SCENE)
    names = WF.scene_from_matpreview_xml(str(path))[0]
    assert names == ["bsdf_21", "bsdf_25", "chm_orange_rgb"]
    assert WF.albedos_from_matpreview_xml(str(path)) == [(0.1, 0.9, 0.9), (1.0, 1.0, 1.0), (0.5, 0.25, 1.0)]
    assert [p for p, _ in WF.parse_matpreview_xml(str(path))] == [{"idx": 21}, {"idx": 25}, {"filename": "chm_orange_rgb"}]
    gt = ground_truth_for(names)
    assert sorted(gt) == [0, 1] and isinstance(gt[0], Principled) and isinstance(gt[1], RoughDielectric)
    assert (gt[0].roughness, gt[0].metallic) == (0.7, 0.1) and gt[1].alpha == 0.5
    gt = ground_truth_for(["bsdf_13_spherical", "bsdf_13_disk", "bsdf_x", "bsdf_24"])
    assert sorted(gt) == [0, 3] and gt[0].roughness == 0.7 and gt[3].alpha == 0.3
    assert ground_truth_for([]) == {}
    with pytest.raises(IndexError, match="0..25"):
        ground_truth_for(["bsdf_2", "bsdf_26_spherical"])
    bad = tmp_path / "bad.xml"
    bad.write_text(SCENE.replace('"0.5 0.25 1"', '"0.5 0.25"'))
    with pytest.raises(ValueError, match="RGB triple"):
        WF.albedos_from_matpreview_xml(str(bad))


def test_the_kernels_need_no_scratch():
    """Cross-compile csrc/analytic_table.hip for gfx950 and read the compiler's resource report: 0 bytes of scratch on all four."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    import tempfile
    with tempfile.TemporaryDirectory(prefix="analytic_table_cc_") as td:
        cmd = ["hipcc", *_lib.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-I", _lib.INCLUDE_DIR, "-c",
               os.path.join(ROOT, "bsdf_diffusion_sampling_amd", "csrc", "analytic_table.hip"), "-o", os.path.join(td, "analytic_table.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for block in text.split("Function Name: ")[1:]:
        name = next((k for k in KERNELS if re.search(r"\d+" + k + "E", block.split()[0])), None)
        if name:
            grab = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
            seen[name] = (grab(r" VGPRs"), grab(r"ScratchSize \[bytes/lane\]"), grab(r"Occupancy \[waves/SIMD\]"))
    print(", ".join(f"{k}: {v[0]} VGPRs, {v[1]} B scratch, {v[2]} waves/SIMD" for k, v in seen.items()))
    assert sorted(seen) == sorted(KERNELS)
    assert all(v[1] == 0 for v in seen.values()), seen
