"""CPU tests of the mixed-material ground-truth table (csrc/measured_table.hip, measured.MeasuredTable): the symbols, the
argument checks of the C entry point that run before any device work, and the tensor checks of the Python host."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from bsdf_diffusion_sampling_amd import _lib  # noqa: E402

SYMBOLS = ("bsdfd_measured_table_create", "bsdfd_measured_table_destroy", "bsdfd_measured_eval_table",
           "bsdfd_measured_sample_weight_table")
EINVAL = 1


def test_library_exports_the_table_entry_points():
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    hdr = open(_lib.INCLUDE_DIR + "/bsdfd.h").read()
    assert all(name + "(" in hdr for name in SYMBOLS)


def test_abi_version_is_unchanged():
    assert _lib.lib().bsdfd_abi_version() == 8 == _lib.ABI_VERSION


def test_table_create_rejects_bad_arguments():
    L = _lib.lib()

    def attempt(handles, n, expect):
        t = C.c_void_p(0xdead)
        rc = L.bsdfd_measured_table_create(handles, n, C.byref(t))
        msg = L.bsdfd_last_error().decode()
        assert rc == EINVAL and t.value is None and expect in msg, (rc, t.value, msg)

    some = (C.c_void_p * 4)(None, 0x1000, None, None)   # never dereferenced: the count is rejected first
    attempt(None, 4, "null handle array")
    attempt(some, 0, "n_materials")
    attempt(some, -1, "n_materials")
    attempt(some, 65537, "n_materials")
    attempt((C.c_void_p * 3)(None, None, None), 3, "at least one")
    attempt((C.c_void_p * 65536)(), 65536, "at least one")
    assert L.bsdfd_measured_table_create(some, 4, None) == EINVAL


def test_table_destroy_null_is_a_noop():
    _lib.lib().bsdfd_measured_table_destroy(None)
    _lib.lib().bsdfd_measured_table_destroy(C.c_void_p())


def test_launch_calls_reject_a_null_table_and_negative_n():
    L = _lib.lib()
    assert L.bsdfd_measured_eval_table(None, None, None, None, None, 0, None, None, None, None) == EINVAL
    assert "null measured table" in L.bsdfd_last_error().decode()
    assert L.bsdfd_measured_sample_weight_table(None, None, None, None, None, None, 0, None, 30.0, None, None, None) == EINVAL
    assert "null measured table" in L.bsdfd_last_error().decode()


def test_python_table_checks_its_entries():
    from bsdf_diffusion_sampling_amd import MeasuredTable
    from bsdf_diffusion_sampling_amd.measured import MeasuredTable as M2
    assert MeasuredTable is M2
    with pytest.raises(ValueError, match="entries"):
        MeasuredTable([])
    with pytest.raises(ValueError, match="MeasuredBSDF"):
        MeasuredTable([None, "chm_orange_rgb.bsdf"])
    assert len(MeasuredTable([None, None, None])) == 3


def test_eval_t_checks_its_tensors():
    """The tensor checks come before the native table is touched, so they run without a device."""
    from bsdf_diffusion_sampling_amd import MeasuredTable
    tab = MeasuredTable([None, None])
    n = 8
    ids, v = torch.zeros(n, dtype=torch.int64), torch.zeros(n, 3)
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):        # CPU tensors
        tab.eval_t(ids, v, v)
    with pytest.raises(ValueError, match="material_id must be an int64"):  # a float material_id
        tab.eval_t(ids.float(), v, v)
    with pytest.raises(ValueError, match="material_id must be an int64"):
        tab.eval_t(ids.to(torch.int32), v, v)
    with pytest.raises(ValueError, match="wo has 5 rows"):                 # a wrong row count
        tab.eval_t(ids, v, v[:5])
    with pytest.raises(ValueError, match="wi has 8 rows, material_id has 5"):
        tab.eval_t(ids[:5], v, v)
    with pytest.raises(ValueError, match="out_l has 3 rows"):
        tab.eval_t(ids, v, v, wl=v, out_l=v[:3])
    with pytest.raises(ValueError, match="wl must be an fp32 tensor"):
        tab.eval_t(ids, v, v, wl=v.double())
    with pytest.raises(ValueError, match="out_l without wl"):              # a lone out_l
        tab.eval_t(ids, v, v, out_l=v.clone())
    with pytest.raises(ValueError, match="pdf_sa must be an fp32 tensor \\[N\\]"):
        tab.sample_weight(ids, v, v, v)
