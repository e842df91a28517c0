"""The synthetic wavefront the Russian roulette of the array-scene path tracer is checked on (``bsdfd_wf_bounce_rr``; the rule
itself is in tests/bounce_ref.py).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import pathtrace_ref as R

F = np.float32
OFFSET = (1 << 32) - 100    # the counter's low word wraps inside a wavefront that starts here
KEPT = ("org", "nrm", "wi", "wl", "beta")


def rr_wavefront(v: dict, seed: int, zero_rows: int = 32, scene: dict = R.SYNTH_SCENE):
    """The synthetic wavefront ``v`` (``pathtrace_ref.synthetic_vertices`` or one of its two descendants) made fit for roulette:
    ``beta`` per row and channel log-uniform in [1e-3, 2], and ``f_o`` = 0 on ``zero_rows`` of the ball rows that have ground truth
    (q = 0: the path must end).  Ended rows keep their NaN state."""
    g = np.random.default_rng(seed)
    n = len(v["material"])
    n_b = len(scene["spheres"])
    beta = np.exp(g.uniform(np.log(1e-3), np.log(2.0), (n, 3)))
    beta[v["material"] > n_b] = np.nan
    out = dict(v, beta=beta.astype(F))
    if "f_o" in v:
        f_o = v["f_o"].copy()
        rows = np.flatnonzero((v["material"] < n_b) & ~np.isnan(f_o[:, 0]) & np.isfinite(v["pdf_o"]) & (v["pdf_o"] > 0) & (v["wo"][:, 2] > 0))
        f_o[g.choice(rows, zero_rows, replace=False)] = 0.0
        out["f_o"] = f_o
    return out
