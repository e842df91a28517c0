#!/usr/bin/env python3
"""What the lit and env path kernels wrote before the three bounce kernels became one templated body:
``bounce_kernels_before_merge.npz``.

The arrays of ``recorded_arrays()`` in tests/test_gpu_pathtrace_lights.py and tests/test_gpu_envmap.py (the keys and cases are
described there), from the library ``BSDFD_LIB_PATH`` selects — a build of the commit to pin — driven by this tree's Python.

Usage (on an MI355X):  BSDFD_LIB_PATH=<build of the parent commit>/libbsdfd.so python tests/golden/make_bounce_merge_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_envmap as E  # noqa: E402
import test_gpu_pathtrace_lights as L  # noqa: E402


def main():
    out = dict(L.recorded_arrays(L.synthetic_inputs()), **E.recorded_arrays(E.synthetic_inputs()))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bounce_kernels_before_merge.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
