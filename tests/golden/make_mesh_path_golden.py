#!/usr/bin/env python3
"""What the mesh path kernels wrote before the sphere and mesh kernels got one __global__ template and one launcher per stage:
``mesh_path_before_unify.npz``.

The arrays of ``recorded_arrays()`` in tests/test_gpu_mesh_path.py (the keys and cases are described there), from the library
``BSDFD_LIB_PATH`` selects — a build of the commit to pin — driven by this tree's Python.

Usage (on an MI355X):  BSDFD_LIB_PATH=<build of the parent commit>/libbsdfd.so python tests/golden/make_mesh_path_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_mesh_path as T  # noqa: E402


def main():
    out = T.recorded_arrays(T.make_kernel_case(T.RECORDED_N))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mesh_path_before_unify.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
