"""Issue order of the Euler-step loop of the two register-resident disk kernels (csrc/flow32.hip, flow_kernel32<.., ROP>), as
recorded in profiles/isa_mix_latest.json by ``tools/isa_mix.py --profile`` from the assembly of the committed kernel sources
(tests/test_host_cpu.py::test_committed_profiles_match_the_kernel_source ties that file to the sources).

At 2 waves per SIMD little else fills the shadow of an MFMA, so the loop is held to the spacing the general disk kernel had at
3 waves per SIMD when the resident kernels were scheduled by hand: at most 13 MFMAs with nothing of the wave's
own behind them (``mfma_bare``: followed directly by another MFMA or by an s_nop) and at most 39 cycles of s_nop pads
(``pad_cycles``).  The MFMA count is the floor of the formulation: four Jacobian matvecs and two state matvecs in three-product
split fp16, plus layer 1."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDENT = ("disk_1Mi_T8", "disk_1Mi_T8@pdf")   # ROP = OP_SAMPLE, OP_PDF


@pytest.fixture(scope="module")
def mix():
    return json.load(open(os.path.join(ROOT, "profiles", "isa_mix_latest.json")))


@pytest.mark.parametrize("workload", RESIDENT)
def test_resident_loop_keeps_its_mfma_count_and_spacing(mix, workload):
    m = mix[workload]
    assert m["kernel"].startswith("flow_kernel32ILi0ELb1ELb0ELb1ELi") and not m["kernel"].endswith("n1E"), m["kernel"]
    print(f"{workload}: n_mfma {m['n_mfma']}, mfma_bare {m['mfma_bare']}, pad_cycles {m['pad_cycles']}, longest MFMA run "
          f"{m['mfma_run_max']}, pads over 4 cycles {m['pads_over_4']}, VGPRs {m['meta']['vgpr_count']}")
    assert m["n_mfma"] == 37
    assert m["mfma_bare"] <= 13
    assert m["pad_cycles"] <= 39
    assert m["meta"]["vgpr_count"] <= 256 and m["meta"]["vgpr_spill_count"] == 0 and m["meta"]["private_segment_fixed_size"] == 0
