"""Helper (not a test): numpy restatement of the measured BSDF's own importance sampler — ``sample(wi, u)`` and ``pdf(wi, wo)`` of
Mitsuba 3's ``measured`` plugin (Dupuy & Jakob 2018), as csrc/measured_dev.h computes them — in a chosen float type.

fp64 is the reference of the GPU tests; the fp32 run of the SAME code is their yardstick: what the arithmetic as written costs in
single precision (the device's ``sincosf / atan2f / asinf`` and fused multiply-adds differ from numpy's, which is what the tests'
factor over the yardstick covers).  The tables are built in fp64 and then rounded to the working type, as the loader does.

Self-contained: its own warp class (``Warp``), with the cancellation-free root of the segment integral.  Only the tensor-file
reader comes from oracle/measured_oracle.py.  PARITY-UNPINNED against Mitsuba, like the evaluator.
"""
import numpy as np

from oracle.measured_oracle import read_tensor_file


def solve_segment(c0, a, rem):
    """t in [0,1] with t (c0 + a t / 2) = rem; 2 rem / (c0 + sqrt(c0^2 + 2 a rem)), 0 where the denominator is 0."""
    den = c0 + np.sqrt(np.maximum(c0 * c0 + 2 * a * rem, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0, 2 * rem / np.where(den > 0, den, 1), 0)
    return np.clip(t, 0, 1).astype(c0.dtype)


class Warp:
    """Bilinear table ``raw[n_phi, n_theta, H, W]`` over [0,1]^2, interpolated linearly over (phi_i, theta_i), each slice
    normalised; ``sample`` / ``invert`` / ``eval`` with densities per unit area of the unit square."""

    def __init__(self, raw, phi_i, theta_i, dtype=np.float64):
        self.dt = np.dtype(dtype)
        flat = np.asarray(raw, dtype=np.float64)
        self.h, self.w = flat.shape[-2:]
        seg = 0.5 * (flat[..., :-1] + flat[..., 1:])
        cond = np.concatenate([np.zeros_like(seg[..., :1]), np.cumsum(seg, -1)], -1)          # [.., H, W]
        row = cond[..., -1]
        mseg = 0.5 * (row[..., :-1] + row[..., 1:])
        marg = np.concatenate([np.zeros_like(mseg[..., :1]), np.cumsum(mseg, -1)], -1)        # [.., H]
        scale = 1.0 / marg[..., -1]
        self.data = (flat * scale[..., None, None]).astype(self.dt)
        self.cond = (cond * scale[..., None, None]).astype(self.dt)
        self.marg = (marg * scale[..., None]).astype(self.dt)
        self.params = [np.asarray(phi_i).astype(self.dt), np.asarray(theta_i).astype(self.dt)]
        self.area = self.dt.type((self.w - 1) * (self.h - 1))

    def slices(self, param):
        """[(weight [N], (i_phi [N], i_theta [N]))] over the <= 4 corner slices, in the evaluator's order."""
        one = self.dt.type(1)
        combos = [(np.ones(len(param[0]), dtype=self.dt), ())]
        for vals, p in zip(self.params, param):
            p = np.asarray(p, dtype=self.dt)
            if len(vals) == 1:
                combos = [(w, idx + (np.zeros(len(p), dtype=np.int64),)) for w, idx in combos]
                continue
            i = np.clip(np.searchsorted(vals, p, side="right") - 1, 0, len(vals) - 2)
            t = np.clip((p - vals[i]) / (vals[i + 1] - vals[i]), 0, 1).astype(self.dt)
            combos = [c for w, idx in combos for c in ((w * (one - t), idx + (i,)), (w * t, idx + (i + 1,)))]
        return combos

    def _mix(self, table, sl, *ij):
        acc = np.zeros(len(sl[0][0]), dtype=self.dt) if ij[0].ndim == 1 else np.zeros(ij[0].shape, dtype=self.dt)
        for w, idx in sl:
            pre = tuple(a.reshape(a.shape + (1,) * (ij[0].ndim - 1)) for a in idx)
            acc = acc + w.reshape(w.shape + (1,) * (ij[0].ndim - 1)) * table[pre + ij]
        return acc

    def _patch(self, pos):
        x = np.asarray(pos[0], dtype=self.dt) * self.dt.type(self.w - 1)
        y = np.asarray(pos[1], dtype=self.dt) * self.dt.type(self.h - 1)
        ix = np.clip(np.floor(x).astype(np.int64), 0, self.w - 2)
        iy = np.clip(np.floor(y).astype(np.int64), 0, self.h - 2)
        return ix, iy, (x - ix).astype(self.dt), (y - iy).astype(self.dt)

    def sample(self, s, param):
        """uniform variates (s0, s1) -> (position (x, y), density)."""
        sl = self.slices(param)
        sx, sy = (np.asarray(a, dtype=self.dt) for a in s)
        n, one = len(sx), self.dt.type(1)
        rows = np.arange(n)
        marg = self._mix(self.marg, sl, np.broadcast_to(np.arange(self.h), (n, self.h)))                  # [N, H]
        iy = np.clip((marg <= sy[:, None]).sum(1) - 1, 0, self.h - 2)
        last = np.full(n, self.w - 1)
        r0, r1 = self._mix(self.cond, sl, iy, last), self._mix(self.cond, sl, iy + 1, last)
        fy = solve_segment(r0, r1 - r0, sy - marg[rows, iy])
        target = sx * ((one - fy) * r0 + fy * r1)
        cols = np.broadcast_to(np.arange(self.w), (n, self.w))
        cond = ((one - fy)[:, None] * self._mix(self.cond, sl, np.broadcast_to(iy[:, None], cols.shape), cols)
                + fy[:, None] * self._mix(self.cond, sl, np.broadcast_to(iy[:, None] + 1, cols.shape), cols))
        ix = np.clip((cond <= target[:, None]).sum(1) - 1, 0, self.w - 2)
        v00, v10 = self._mix(self.data, sl, iy, ix), self._mix(self.data, sl, iy, ix + 1)
        v01, v11 = self._mix(self.data, sl, iy + 1, ix), self._mix(self.data, sl, iy + 1, ix + 1)
        c0, c1 = (one - fy) * v00 + fy * v01, (one - fy) * v10 + fy * v11
        fx = solve_segment(c0, c1 - c0, target - cond[rows, ix])
        pos = ((ix.astype(self.dt) + fx) / self.dt.type(self.w - 1), (iy.astype(self.dt) + fy) / self.dt.type(self.h - 1))
        return pos, ((one - fx) * c0 + fx * c1) * self.area

    def invert(self, pos, param):
        """position -> (the variates ``sample`` maps to it, density)."""
        sl = self.slices(param)
        ix, iy, fx, fy = self._patch(pos)
        one, half = self.dt.type(1), self.dt.type(0.5)
        v00, v10 = self._mix(self.data, sl, iy, ix), self._mix(self.data, sl, iy, ix + 1)
        v01, v11 = self._mix(self.data, sl, iy + 1, ix), self._mix(self.data, sl, iy + 1, ix + 1)
        c0, c1 = (one - fy) * v00 + fy * v01, (one - fy) * v10 + fy * v11
        part = fx * (c0 + half * fx * (c1 - c0))
        last = np.full_like(ix, self.w - 1)
        cdf0, cdf1 = self._mix(self.cond, sl, iy, ix), self._mix(self.cond, sl, iy + 1, ix)
        r0, r1 = self._mix(self.cond, sl, iy, last), self._mix(self.cond, sl, iy + 1, last)
        row = (one - fy) * r0 + fy * r1
        with np.errstate(divide="ignore", invalid="ignore"):
            s0 = np.where(row > 0, (part + (one - fy) * cdf0 + fy * cdf1) / np.where(row > 0, row, 1), 0).astype(self.dt)
        s1 = fy * (r0 + half * fy * (r1 - r0)) + self._mix(self.marg, sl, iy)
        return (s0, s1), ((one - fx) * c0 + fx * c1) * self.area

    def eval(self, pos, param):
        sl = self.slices(param)
        ix, iy, fx, fy = self._patch(pos)
        one = self.dt.type(1)
        v00, v10 = self._mix(self.data, sl, iy, ix), self._mix(self.data, sl, iy, ix + 1)
        v01, v11 = self._mix(self.data, sl, iy + 1, ix), self._mix(self.data, sl, iy + 1, ix + 1)
        return ((one - fy) * ((one - fx) * v00 + fx * v10) + fy * ((one - fx) * v01 + fx * v11)) * self.area


def _bilinear(table, pos, dt):
    """Plain (unnormalised, parameter-free) bilinear lookup of ``table[H, W]``."""
    h, w = table.shape
    x, y = pos[0] * dt.type(w - 1), pos[1] * dt.type(h - 1)
    ix = np.clip(np.floor(x).astype(np.int64), 0, w - 2)
    iy = np.clip(np.floor(y).astype(np.int64), 0, h - 2)
    fx, fy, one = (x - ix).astype(dt), (y - iy).astype(dt), dt.type(1)
    return ((one - fy) * ((one - fx) * table[iy, ix] + fx * table[iy, ix + 1])
            + fy * ((one - fx) * table[iy + 1, ix] + fx * table[iy + 1, ix + 1]))


class MeasuredSampler:
    """``sample`` / ``pdf`` / ``eval`` of one RGL rgb tensor file in ``dtype`` arithmetic."""

    def __init__(self, path, dtype=np.float64):
        self.dt = dt = np.dtype(dtype)
        t = read_tensor_file(path)
        phi_i, theta_i = t["phi_i"].astype(np.float64), t["theta_i"].astype(np.float64)
        self.isotropic = len(phi_i) <= 2
        self.jacobian = bool(t["jacobian"][0])
        self.reduction, self.fold = 0, (1.0, 1.0)
        if not self.isotropic:
            self.reduction = int(np.rint(2 * np.pi / (phi_i[-1] - phi_i[0])))
            mid = 0.5 * (phi_i[0] + phi_i[-1])
            self.fold = (-1.0 if np.cos(mid) < 0 else 1.0, -1.0 if np.sin(mid) < 0 else 1.0)
        self.vndf = Warp(t["vndf"], t["phi_i"], t["theta_i"], dt)
        self.luminance = Warp(t["luminance"], t["phi_i"], t["theta_i"], dt) if "luminance" in t else None
        self.ndf, self.sigma, self.rgb = t["ndf"].astype(dt), t["sigma"].astype(dt), t["rgb"].astype(dt)
        self.pi = dt.type(np.pi)

    # -- pieces -------------------------------------------------------------------------------------------------------
    def _fold(self, wi):
        """-> (wi folded onto the stored side, flip_x [N], flip_y [N]): csrc/measured_dev.h's fold_wi.  A component on the wrong
        side is negated (the flips are what the caller applies to wo); a zero component of either sign flips nothing and takes
        the stored side's sign, so that arctan2 answers inside [phi_i[0], phi_i[-1]]."""
        n = len(wi)
        fx = fy = np.zeros(n, dtype=bool)
        wif = wi.copy()
        if self.reduction >= 2:
            sx, sy = self.dt.type(self.fold[0]), self.dt.type(self.fold[1])
            fy = wi[:, 1] * sy < 0
            fx = (wi[:, 0] * sx < 0) if self.reduction == 4 else fy
            wif[:, 1] = np.copysign(wi[:, 1], sy)
            # (reduction 2 stores both sides of x: a zero x is read as +0)
            wif[:, 0] = np.copysign(wi[:, 0], sx) if self.reduction == 4 else np.where(fx, -wi[:, 0], wi[:, 0]) + self.dt.type(0)
        return wif, fx, fy

    def folded_azimuth(self, wi):
        """phi_i as every call forms it: the azimuth of the folded incident direction (the tests hold it to the stored range)."""
        return self._incident(self._fold(np.asarray(wi).astype(self.dt))[0])[1]

    @staticmethod
    def _flip(v, fx, fy):
        v = v.copy()
        v[:, 0] = np.where(fx, -v[:, 0], v[:, 0])
        v[:, 1] = np.where(fy, -v[:, 1], v[:, 1])
        return v

    def _elevation(self, d):
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + (d[:, 2] - self.dt.type(1)) ** 2)
        return self.dt.type(2) * np.arcsin(np.minimum(self.dt.type(0.5) * dist, self.dt.type(1)))

    def _incident(self, wi):
        theta_i, phi_i = self._elevation(wi), np.arctan2(wi[:, 1], wi[:, 0])
        u_wi = (np.sqrt(theta_i * (self.dt.type(2) / self.pi)), (phi_i + self.pi) * (self.dt.type(0.5) / self.pi))
        return theta_i, phi_i, u_wi

    def _jac(self, um_x, sin_theta_m, m_dot_wi):
        return np.maximum(self.dt.type(2) * self.pi * self.pi * um_x * sin_theta_m, self.dt.type(1e-6)) * self.dt.type(4) * m_dot_wi

    def _spectrum(self, s, u_m, u_wi, param):
        sl = self.vndf.slices(param)                       # the same slices and weights for every table of the file
        sh, sw = self.rgb.shape[-2:]
        out = np.zeros((len(s[0]), 3), dtype=self.dt)
        for w, (ip, it) in sl:
            for c in range(3):
                x, y = s[0] * self.dt.type(sw - 1), s[1] * self.dt.type(sh - 1)
                ix = np.clip(np.floor(x).astype(np.int64), 0, sw - 2)
                iy = np.clip(np.floor(y).astype(np.int64), 0, sh - 2)
                fx, fy, one = (x - ix).astype(self.dt), (y - iy).astype(self.dt), self.dt.type(1)
                tab = self.rgb[:, :, c]
                out[:, c] += w * ((one - fy) * ((one - fx) * tab[ip, it, iy, ix] + fx * tab[ip, it, iy, ix + 1])
                                  + fy * ((one - fx) * tab[ip, it, iy + 1, ix] + fx * tab[ip, it, iy + 1, ix + 1]))
        if self.jacobian:
            with np.errstate(divide="ignore", invalid="ignore"):
                out = out * (_bilinear(self.ndf, u_m, self.dt) / (self.dt.type(4) * _bilinear(self.sigma, u_wi, self.dt)))[:, None]
        return out.astype(self.dt)

    # -- the two calls ------------------------------------------------------------------------------------------------
    def sample(self, wi, u, tint=None):
        """-> (wo [N,3], pdf [N], weight [N,3]); zeros where wi.z <= 0; pdf = weight = 0 where wo.z <= 0 (wo as computed)."""
        dt, one = self.dt, self.dt.type(1)
        wi, u = np.asarray(wi).astype(dt), np.asarray(u).astype(dt)
        active = wi[:, 2] > 0
        wif, fx, fy = self._fold(wi)
        theta_i, phi_i, u_wi = self._incident(wif)
        param = (phi_i, theta_i)
        s = (u[:, 1].copy(), u[:, 0].copy())               # Mitsuba's swap
        lum_pdf = np.ones(len(wi), dtype=dt)
        if self.luminance is not None:
            s, lum_pdf = self.luminance.sample(s, param)
        u_m, vndf_pdf = self.vndf.sample(s, param)
        theta_m = u_m[0] * u_m[0] * (self.pi * dt.type(0.5))
        phi_m = (dt.type(2) * u_m[1] - one) * self.pi
        if self.isotropic:
            phi_m = phi_m + phi_i
        st, ct = np.sin(theta_m), np.cos(theta_m)
        m = np.stack([np.cos(phi_m) * st, np.sin(phi_m) * st, ct], 1).astype(dt)
        d = (m * wif).sum(1).astype(dt)
        wo = self._flip((dt.type(2) * d[:, None] * m - wif).astype(dt), fx, fy)
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = (vndf_pdf * lum_pdf / self._jac(u_m[0], st, d)).astype(dt)
        ok = active & (wo[:, 2] > 0) & (pdf > 0) & np.isfinite(pdf)
        with np.errstate(divide="ignore", invalid="ignore"):
            weight = self._spectrum(s, u_m, u_wi, param) / pdf[:, None]
        if tint is not None:
            weight = weight * np.asarray(tint).astype(dt)
        return (np.where(active[:, None], wo, 0).astype(dt), np.where(ok, pdf, 0).astype(dt),
                np.where(ok[:, None], weight, 0).astype(dt))

    def _half_vector(self, wi, wo):
        dt = self.dt
        wif, fx, fy = self._fold(wi)
        wof = self._flip(wo, fx, fy)
        m = wif + wof
        m = (m / np.maximum(np.sqrt((m * m).sum(1, keepdims=True)), dt.type(1e-30))).astype(dt)
        if self.reduction >= 2:                            # unsign_zeros: -0 -> +0, the pole (+-0, +-0) has the azimuth 0
            m[:, :2] = m[:, :2] + dt.type(0)
        theta_i, phi_i, u_wi = self._incident(wif)
        theta_m, phi_m = self._elevation(m), np.arctan2(m[:, 1], m[:, 0])
        um_y = ((phi_m - phi_i if self.isotropic else phi_m) + self.pi) * (dt.type(0.5) / self.pi)
        u_m = (np.sqrt(theta_m * (dt.type(2) / self.pi)), (um_y - np.floor(um_y)).astype(dt))
        return wif, m, theta_m, u_m, u_wi, (phi_i, theta_i)

    def pdf(self, wi, wo):
        dt = self.dt
        wi, wo = np.asarray(wi).astype(dt), np.asarray(wo).astype(dt)
        active = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        wif, m, theta_m, u_m, u_wi, param = self._half_vector(wi, wo)
        s, vndf_pdf = self.vndf.invert(u_m, param)
        lum_pdf = self.luminance.eval(s, param) if self.luminance is not None else np.ones(len(wi), dtype=dt)
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = (vndf_pdf * lum_pdf / self._jac(u_m[0], np.sin(theta_m), (m * wif).sum(1).astype(dt))).astype(dt)
        return np.where(active & (pdf > 0) & np.isfinite(pdf), pdf, 0).astype(dt)

    def eval(self, wi, wo, tint=None):
        """f(wi, wo) cos(theta_o), as the evaluator computes it (the spectral lookup at the inverted position)."""
        dt = self.dt
        wi, wo = np.asarray(wi).astype(dt), np.asarray(wo).astype(dt)
        active = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        wif, m, theta_m, u_m, u_wi, param = self._half_vector(wi, wo)
        s, _ = self.vndf.invert(u_m, param)
        f = self._spectrum(s, u_m, u_wi, param)
        if tint is not None:
            f = f * np.asarray(tint).astype(dt)
        return np.where(active[:, None], f, 0).astype(dt)


# -- the yardstick rule of the GPU tests (test_gpu_measured_sampling.py, test_gpu_measured_fold.py) -------------------------------
def sample_errors(res, ref, rows):
    """(wo, pdf, weight) against the fp64 reference on `rows` -> {quantity: per-row error}."""
    wo, pdf, w = (np.asarray(a, dtype=np.float64)[rows] for a in res)
    wo_r, pdf_r, w_r = (a[rows] for a in ref)
    return {"wo": np.abs(wo - wo_r).max(1), "pdf": np.abs(pdf - pdf_r) / pdf_r,
            "weight": np.abs(w - w_r).max(1) / (np.abs(w_r).max(1) + 1e-3)}


def held_to_yardstick(label, got, yard, maxima=True):
    """Each quantity's p99 (and max) of `got` is at most 4x the yardstick's; the message carries every figure."""
    fig = {q: dict(gpu_p99=np.percentile(got[q], 99), yard_p99=np.percentile(yard[q], 99), gpu_max=got[q].max(), yard_max=yard[q].max())
           for q in got}
    msg = label + ": " + "; ".join(f"{q} p99 gpu {f['gpu_p99']:.3e} yardstick {f['yard_p99']:.3e}, max gpu {f['gpu_max']:.3e} "
                                   f"yardstick {f['yard_max']:.3e}" for q, f in fig.items())
    print(msg)
    for q, f in fig.items():
        assert f["gpu_p99"] <= 4 * f["yard_p99"], msg
        if maxima:
            assert f["gpu_max"] <= 4 * f["yard_max"], msg
    return fig
