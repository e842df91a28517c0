"""Helper (not a test): the five synthetic anisotropic files — one per stored ``phi_i`` range — and the rows on which
tests/test_measured_fold_cpu.py and tests/test_gpu_measured_fold.py question the fold of csrc/measured_dev.h (``fold_wi``): random
rows over all four quadrants, and hand-placed incident directions ON the symmetry planes (a zero component of either sign), at
normal incidence and 2^-100 off the planes, each paired with eight outgoing directions and eight variate pairs.  Fixed seeds;
fp32 values, as the kernels read them.  numpy only.
"""
import numpy as np

from bsdf_diffusion_sampling_amd import measured_synth

PI = np.pi
# name -> (stored phi_i range, slices, reduction, seed of the tables).  "quadrant_neg" is measured_synth's default file, byte for
# byte; the others close their half-vector tables over the azimuth (measured_synth.write_anisotropic: `closed`), which is what
# makes eval / pdf continuous in wi where the half vector's azimuth wraps from +pi to -pi.  A seed is changed (never a cap) if a
# file misses the caps of test_measured_fold_cpu.py::test_excluded_shares_from_the_reference_alone.
FILES = {
    "quadrant_neg": ((-PI, -PI / 2), 4, 4, 7),
    "quadrant_pos": ((0.0, PI / 2), 4, 4, 8),
    "half_neg": ((-PI, 0.0), 7, 2, 9),
    "half_pos": ((0.0, PI), 7, 2, 10),
    "circle": ((-PI, PI), 9, 1, 12),
}
N_RANDOM = 4096
OFF = 2.0 ** -100
TOP = np.float32(1 - 2.0 ** -24)


def write_files(directory):
    """{name: path} of the five files, written under ``directory``."""
    out = {}
    for name, (rng, n_phi, _, seed) in FILES.items():
        p = str(directory / f"{name}_rgb.bsdf")
        if name == "quadrant_neg":
            out[name] = measured_synth.write_anisotropic(p)
        else:
            out[name] = measured_synth.write_anisotropic(p, seed=seed, phi_range=rng, n_phi=n_phi, closed=True)
    return out


def random_rows():
    """(wi, wo, u) fp32, N_RANDOM rows: wi over all four quadrants with z >= 0.02; half of the wo within 0.05 of the mirror
    direction (tests/test_gpu_measured.py), a few below the horizon; u the variates of ``sample``.  No component is zero."""
    g = np.random.default_rng(41)
    wi, wo = measured_synth.dirs(g, N_RANDOM, 0.02), measured_synth.dirs(g, N_RANDOM, 0.02)
    k = N_RANDOM // 2
    wo[:k] = wi[:k] * [-1, -1, 1] + g.normal(size=(k, 3)) * 0.05
    wo[:k] /= np.linalg.norm(wo[:k], axis=1, keepdims=True)
    wo[::500, 2] *= -1
    wi, wo, u = wi.astype(np.float32), wo.astype(np.float32), g.random((N_RANDOM, 2)).astype(np.float32)
    assert (wi[:, :2] != 0).all() and (wo[:, :2] != 0).all()
    return wi, wo, u


def hand_wi():
    """(wi [36, 3] fp64, axis [36]): the hand-placed incident directions and, per row, which component is the (near-)zero one —
    0 / 1 for a plane row with EXACTLY one zero component (x / y), 2 for the four signed normal incidences, -1 for the rows
    2^-100 off a plane."""
    rows, axis = [], []
    for s, c in ((0.6, 0.8), (np.sqrt(1 - 0.02 ** 2), 0.02)):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                rows += [(sign * s, zero, c), (zero, sign * s, c)]
                axis += [1, 0]
    for zx in (0.0, -0.0):
        for zy in (0.0, -0.0):
            rows.append((zx, zy, 1.0))
            axis.append(2)
    for s, c in ((0.6, 0.8), (np.sqrt(1 - 0.02 ** 2), 0.02)):
        for sign in (1.0, -1.0):
            for off in (OFF, -OFF):
                rows += [(sign * s, off, c), (off, sign * s, c)]
                axis += [-1, -1]
    return np.array(rows, dtype=np.float64), np.array(axis)


WO_KINDS = ("random", "random", "random", "random", "mirror", "same", "y == 0", "x == 0")


def pair(wi):
    """Each row of ``wi`` [K, 3] with eight outgoing directions and eight variate pairs -> (wi [8K, 3], wo [8K, 3], u [8K, 2],
    kind [8K] = index into WO_KINDS), fp64 (the callers round).  Four random wo without zero components, the exact mirror
    direction and wo = wi — both formed FROM the row's wi, so that a row moved off its plane keeps its half vector on the pole /
    on wi —, one wo with wo.y == 0 and one with wo.x == 0; the four corners of the unit square and four random variate pairs.
    The random ones depend on K alone."""
    k = len(wi)
    g = np.random.default_rng(43)
    wo = np.empty((k, 8, 3))
    wo[:, :4] = measured_synth.dirs(g, 4 * k, 0.05).reshape(k, 4, 3)
    wo[:, 4] = wi * [-1, -1, 1]
    wo[:, 5] = wi
    on = measured_synth.dirs(g, 2 * k, 0.05).reshape(k, 2, 3)
    for j, comp in ((0, 1), (1, 0)):
        d = on[:, j].copy()
        d[:, comp] = 0.0
        wo[:, 6 + j] = d / np.linalg.norm(d, axis=1, keepdims=True)
    u = np.empty((k, 8, 2))
    u[:, :4] = [[0, 0], [0, TOP], [TOP, 0], [TOP, TOP]]
    u[:, 4:] = g.random((k, 4, 2))
    return np.repeat(wi, 8, 0), wo.reshape(-1, 3), u.reshape(-1, 2), np.tile(np.arange(8), k)


def hand_rows():
    """(wi, wo, u fp32 [288, ...], kind [288], axis [288]): ``pair`` of ``hand_wi``."""
    wi, axis = hand_wi()
    wi8, wo, u, kind = pair(wi)
    wo = wo.astype(np.float32)
    wo[kind == 4] = (wi8.astype(np.float32) * np.float32([-1, -1, 1]))[kind == 4]      # exact in fp32 too
    wo[kind == 5] = wi8.astype(np.float32)[kind == 5]
    return wi8.astype(np.float32), wo, u.astype(np.float32), kind, np.repeat(axis, 8)


def off_plane(wi, axis, fold, reduction, eps):
    """The plane rows ``wi`` (exactly one zero component, ``axis``) with the zero replaced by ``eps`` of the stored side's sign:
    the file's side (``fold`` = signs of x and y at the middle of its phi_i range) where the component is folded — y for
    reduction >= 2, x for reduction 4 —, else the zero's own sign (both sides are stored)."""
    out = np.array(wi, dtype=np.float64)
    for r, a in enumerate(axis):
        folded = reduction == 4 or (reduction == 2 and a == 1)
        out[r, a] = eps * (fold[a] if folded else np.copysign(1.0, wi[r, a]))
    return out
