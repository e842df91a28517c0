"""Synthetic RGL tensor files for the ground-truth evaluator's tests and tools: a minimal writer of Mitsuba's TensorFile layout
(the loader's inverse, as in tests/test_gpu_measured.py) and two families of smooth random tables — only one real file is at
hand (tests/golden/chm_orange_rgb.bsdf); every other branch of the evaluator is reached with these.  numpy only."""
import struct

import numpy as np


def write_tensor_file(path, fields):
    codes = {np.dtype(np.uint8): 1, np.dtype(np.float32): 10}
    header = b"tensor_file\x00" + bytes([1, 0]) + struct.pack("<I", len(fields))
    table_len = sum(2 + len(k) + 2 + 1 + 8 + 8 * v.ndim for k, v in fields.items())
    off = len(header) + table_len
    table, blobs = b"", b""
    for k, v in fields.items():
        v = np.ascontiguousarray(v)
        table += struct.pack("<H", len(k)) + k.encode() + struct.pack("<H", v.ndim) + bytes([codes[v.dtype]])
        table += struct.pack("<Q", off + len(blobs)) + struct.pack(f"<{v.ndim}Q", *v.shape)
        blobs += v.tobytes()
    with open(path, "wb") as f:
        f.write(header + table + blobs)


def _smooth(g, *shape):
    a = g.uniform(0.2, 1.0, size=shape)
    for ax in (-1, -2):
        a = (a + np.roll(a, 1, axis=ax) + np.roll(a, -1, axis=ax)) / 3
    return a.astype(np.float32)


def write_anisotropic(path, seed=7, vndf_hw=(12, 20), rgb_hw=(6, 10), ndf_hw=(9, 17), phi_range=(-np.pi, -np.pi / 2), n_phi=4,
                      closed=False):
    """Anisotropic, jacobian 1, phi_i in ``n_phi`` slices over ``phi_range``: a quadrant (reduction 4; the default is Mitsuba's, and
    the fields of test_gpu_measured.py's synthetic file), a half-plane (reduction 2) or the full circle (reduction 1), whose last
    slice and whose last azimuth row of ``sigma`` repeat the first, as an acquisition's do.  ``closed``: the tables over the
    half vector's azimuth (``vndf``, ``ndf``) and over the warped copy of it (``luminance``, ``rgb``: the VNDF warp takes the
    two ends of the azimuth to their two ends) also end with the row they start with, as a measured material's do — the evaluator
    wraps that azimuth at +pi onto -pi (Mitsuba's ``u - floor(u)``), where only such tables are continuous."""
    g = np.random.default_rng(seed)
    phi_i = np.linspace(phi_range[0], phi_range[1], n_phi).astype(np.float32)
    theta_i = np.linspace(0.0, np.pi / 2, 5).astype(np.float32)
    fields = {
        "version": np.array([1, 0], dtype=np.uint8), "description": np.frombuffer(b"synthetic anisotropic", dtype=np.uint8),
        "phi_i": phi_i, "theta_i": theta_i, "sigma": _smooth(g, *ndf_hw), "ndf": _smooth(g, *ndf_hw) * 3,
        "vndf": _smooth(g, n_phi, 5, *vndf_hw), "luminance": _smooth(g, n_phi, 5, *rgb_hw), "rgb": _smooth(g, n_phi, 5, 3, *rgb_hw),
        "jacobian": np.array([1], dtype=np.uint8)}
    if closed:
        for k in ("vndf", "ndf", "luminance", "rgb"):
            fields[k][..., -1, :] = fields[k][..., 0, :]
    if np.isclose(phi_range[1] - phi_range[0], 2 * np.pi):     # the full circle: phi_i ends on the angle it starts on
        for k in ("vndf", "luminance", "rgb"):
            fields[k][-1] = fields[k][0]
        fields["sigma"][-1] = fields["sigma"][0]
    write_tensor_file(path, fields)
    return path


def write_isotropic(path, seed=11, n_theta=3, vndf_hw=(10, 14), rgb_hw=(5, 7), ndf_hw=(7, 11), jacobian=0):
    """Isotropic with ONE azimuth slice (n_phi = 1) and, by default, jacobian = 0 (no NDF / sigma factor)."""
    g = np.random.default_rng(seed)
    theta_i = np.linspace(0.0, np.pi / 2, n_theta).astype(np.float32)
    write_tensor_file(path, {
        "version": np.array([1, 0], dtype=np.uint8), "description": np.frombuffer(b"synthetic isotropic", dtype=np.uint8),
        "phi_i": np.zeros(1, dtype=np.float32), "theta_i": theta_i, "sigma": _smooth(g, *ndf_hw), "ndf": _smooth(g, *ndf_hw) * 3,
        "vndf": _smooth(g, 1, n_theta, *vndf_hw), "luminance": _smooth(g, 1, n_theta, *rgb_hw),
        "rgb": _smooth(g, 1, n_theta, 3, *rgb_hw), "jacobian": np.array([jacobian], dtype=np.uint8)})
    return path


def dirs(g, n, zmin=0.02):
    """Unit vectors on the upper hemisphere (test_gpu_measured.py's `_dirs`)."""
    z, ph = g.uniform(zmin, 1.0, size=n), g.uniform(0, 2 * np.pi, size=n)
    r = np.sqrt(1 - z * z)
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], 1)
