"""numpy restatement of the rough-dielectric model of csrc/dielectric_dev.h (Walter et al. 2007: Beckmann D, the rational Smith
G1, exact unpolarised Fresnel; radiance-mode transmission) and of its sampling map, statement for statement, parameterised by
dtype: fp64 is the reference of the tests, fp32 the yardstick (the same lines in the kernels' arithmetic).

Directions are rows of [N,3] arrays in the local shading frame; ``alpha`` and ``eta`` are rounded to fp32 first, as the
descriptor the kernels read (``bsdfd_dielectric``) carries them.

The sampling map (``sample_normal``): stretch s*wi by alpha, draw the two slopes of the alpha = 1 visible-normal distribution,
rotate them to the azimuth of wi, unstretch, normalise.  A slope is drawn by inverting

    C(x) = ct erfc(-x) / 2 + st exp(-x^2) / (2 sqrt(pi))          (st, ct: sine and cosine of the stretched direction)

on [-6, min(ct / st, 6)]: 20 bisections, then 2 Newton steps clamped to the last bracket — a fixed trip count.  The second
slope is independent of the first and of the direction: the same routine with (st, ct) = (0, 1)."""
import numpy as np

try:
    from scipy.special import erfc as _erfc
except ImportError:   # the same function, slower
    import math
    _erfc_scalar = np.vectorize(math.erfc, otypes=[np.float64])

    def _erfc(x):
        return _erfc_scalar(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)

IOR = {"bk7": 1.5046, "air": 1.000277, "vacuum": 1.0}
ETA_BK7_AIR = float(np.float32(IOR["bk7"] / IOR["air"]))
SLOPE_LIMIT, BISECTIONS, NEWTON_STEPS = 6.0, 20, 2
MIN_HALF_LEN2 = 1e-12


class RoughDielectric:
    def __init__(self, alpha, eta=ETA_BK7_AIR, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        f = self.dt
        self.alpha, self.eta0 = f(np.float32(alpha)), f(np.float32(eta))
        self.inv_eta0 = f(1) / self.eta0
        self.pi = f(np.pi)
        self.inv_sqrt_pi = f(1 / np.sqrt(np.pi))
        self.inv_2sqrt_pi = f(0.5 / np.sqrt(np.pi))

    def _a(self, x):
        return np.ascontiguousarray(x, dtype=self.dt)

    # ---- the terms ------------------------------------------------------------------------------------------------
    def half_vector(self, wi, wo):
        """-> (m [N,3], reflect, eta, ok): ok is False where the generalised half vector is undefined."""
        f = self.dt
        ci, co = wi[:, 2], wo[:, 2]
        refl = ci * co > 0
        eta = np.where(ci > 0, self.eta0, self.inv_eta0)
        k = np.where(refl, f(1), eta)
        hx, hy, hz = wi[:, 0] + wo[:, 0] * k, wi[:, 1] + wo[:, 1] * k, wi[:, 2] + wo[:, 2] * k
        len2 = hx * hx + hy * hy + hz * hz
        ok = len2 > f(MIN_HALF_LEN2)
        inv = np.where(ok, f(1) / np.sqrt(np.where(ok, len2, f(1))), f(0))
        inv = np.where(hz < 0, -inv, inv)
        m = np.stack([hx * inv, hy * inv, hz * inv], 1)
        return m, refl, eta, ok & (m[:, 2] > 0)

    def ndf(self, m):
        f = self.dt
        a2 = self.alpha * self.alpha
        cz2 = m[:, 2] * m[:, 2]
        d = np.exp(-(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) / (a2 * cz2)) / (self.pi * a2 * cz2 * cz2)
        return np.where(d * m[:, 2] > f(1e-20), d, f(0))

    def g1(self, v, dot_vm):
        f = self.dt
        ax, ay = self.alpha * v[:, 0], self.alpha * v[:, 1]
        xy = ax * ax + ay * ay
        a = f(1) / np.sqrt(xy / (v[:, 2] * v[:, 2]))
        a2 = a * a
        g = (f(3.535) * a + f(2.181) * a2) / (f(1) + f(2.276) * a + f(2.577) * a2)
        g = np.where(a >= f(1.6), f(1), g)
        g = np.where(xy == 0, f(1), g)
        return np.where(dot_vm * v[:, 2] <= 0, f(0), g)

    def fresnel_of(self, eta_it, ca, ct):
        """Unpolarised Fresnel reflectance from the two (absolute) cosines."""
        f = self.dt
        a_s = (eta_it * ct - ca) / (eta_it * ct + ca)
        a_p = (eta_it * ca - ct) / (eta_it * ca + ct)
        F = f(0.5) * (a_s * a_s + a_p * a_p)
        return np.where(ca == 0, f(1), F)

    def fresnel(self, c):
        """-> (F, signed cosine of the transmitted direction, eta_ti); the transmitted cosine by Snell's law."""
        f = self.dt
        outside = c >= 0
        eta_it = np.where(outside, self.eta0, self.inv_eta0)
        eta_ti = np.where(outside, self.inv_eta0, self.eta0)
        ct2 = f(1) - eta_ti * eta_ti * (f(1) - c * c)
        ct = np.sqrt(np.maximum(ct2, f(0)))
        return self.fresnel_of(eta_it, np.abs(c), ct), np.where(c > 0, -ct, ct), eta_ti

    def _terms(self, wi, wo):
        m, refl, eta, ok = self.half_vector(wi, wo)
        dwi = wi[:, 0] * m[:, 0] + wi[:, 1] * m[:, 1] + wi[:, 2] * m[:, 2]
        dwo = wo[:, 0] * m[:, 0] + wo[:, 1] * m[:, 1] + wo[:, 2] * m[:, 2]
        D = self.ndf(m)
        # across the surface the generalised half vector obeys Snell's law by construction: |wo . m| IS the transmitted cosine.
        # Reading it off the pair keeps 1 - F well conditioned next to the critical angle (and reciprocal to rounding).
        F = np.where(refl, self.fresnel(dwi)[0], self.fresnel_of(np.where(dwi >= 0, self.eta0, self.inv_eta0), np.abs(dwi), np.abs(dwo)))
        s = dwi + eta * dwo
        return m, refl, eta, ok, dwi, dwo, D, F, s

    # ---- eval / pdf ---------------------------------------------------------------------------------------------------
    def f_cos(self, wi, wo):
        """f(wi, wo) |cos theta_o| -> [N] (grey)."""
        f = self.dt
        wi, wo = self._a(wi), self._a(wo)
        with np.errstate(all="ignore"):
            m, refl, eta, ok, dwi, dwo, D, F, s = self._terms(wi, wo)
            ci, co = wi[:, 2], wo[:, 2]
            G = self.g1(wi, dwi) * self.g1(wo, dwo)
            vr = F * D * G / (f(4) * np.abs(ci))
            vt = np.abs((f(1) - F) * D * G * dwi * dwo / (ci * (s * s)))
            v = np.where(refl, vr, vt)
            return np.where(ok & (ci != 0) & (co != 0) & np.isfinite(v), v, f(0))

    def eval(self, wi, wo, tint=(1.0, 1.0, 1.0)):
        return self.f_cos(wi, wo)[:, None] * self._a(tint)[None, :]

    def pdf(self, wi, wo):
        f = self.dt
        wi, wo = self._a(wi), self._a(wo)
        with np.errstate(all="ignore"):
            m, refl, eta, ok, dwi, dwo, D, F, s = self._terms(wi, wo)
            ci, co = wi[:, 2], wo[:, 2]
            vis = D * self.g1(wi, dwi) * np.abs(dwi) / np.abs(ci)
            lobe = np.where(refl, F, f(1) - F)
            jac = np.where(refl, f(1) / (f(4) * np.abs(dwo)), eta * eta * np.abs(dwo) / (s * s))
            p = vis * lobe * jac
            return np.where(ok & (ci != 0) & (co != 0) & np.isfinite(p) & (p > 0), p, f(0))

    # ---- sampling -----------------------------------------------------------------------------------------------------
    def _cdf(self, ct, st, x):
        return self.dt(0.5) * ct * _erfc(-x) + st * self.inv_2sqrt_pi * np.exp(-x * x)

    def sample_slope(self, ct, st, u):
        f = self.dt
        lo = np.full_like(u, -SLOPE_LIMIT)
        hi = np.minimum(ct / st, f(SLOPE_LIMIT))
        t = u * self._cdf(ct, st, hi)
        for _ in range(BISECTIONS):
            mid = f(0.5) * (lo + hi)
            up = self._cdf(ct, st, mid) <= t
            lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
        x = f(0.5) * (lo + hi)
        for _ in range(NEWTON_STEPS):
            d = (ct - x * st) * self.inv_sqrt_pi * np.exp(-x * x)
            xn = np.minimum(np.maximum(x - (self._cdf(ct, st, x) - t) / d, lo), hi)
            x = np.where(d > 0, xn, x)
        return x

    def sample_normal(self, v, u0, u1):
        """v = s * wi (v.z > 0) -> the visible normal m [N,3]."""
        with np.errstate(all="ignore"):
            return self._sample_normal(self._a(v), self._a(u0), self._a(u1))

    def _sample_normal(self, v, u0, u1):
        f = self.dt
        sx, sy, sz = self.alpha * v[:, 0], self.alpha * v[:, 1], v[:, 2]
        inv = f(1) / np.sqrt(sx * sx + sy * sy + sz * sz)
        sx, sy, sz = sx * inv, sy * inv, sz * inv
        r = np.sqrt(sx * sx + sy * sy)
        flat = r > 0
        cphi = np.where(flat, sx / r, f(1))
        sphi = np.where(flat, sy / r, f(0))
        slope_x = self.sample_slope(sz, r, u0)
        slope_y = self.sample_slope(np.ones_like(u1), np.zeros_like(u1), u1)
        tx = (cphi * slope_x - sphi * slope_y) * self.alpha
        ty = (sphi * slope_x + cphi * slope_y) * self.alpha
        inv = f(1) / np.sqrt(tx * tx + ty * ty + f(1))
        return np.stack([-tx * inv, -ty * inv, inv], 1)

    def sample(self, wi, u, tint=(1.0, 1.0, 1.0), active=None, details=False):
        """-> (wo [N,3], pdf [N], weight [N,3]); with ``details`` also (reflect [N] bool, F [N])."""
        # (rows with wi.z == 0 or ``active`` false: zeros)
        f = self.dt
        wi, u = self._a(wi), self._a(u)
        with np.errstate(all="ignore"):
            ci = wi[:, 2]
            live = ci != 0
            if active is not None:
                live &= np.asarray(active) != 0
            s = np.where(ci > 0, f(1), f(-1))
            m = self.sample_normal(wi * s[:, None], u[:, 0], u[:, 1])
            c = wi[:, 0] * m[:, 0] + wi[:, 1] * m[:, 1] + wi[:, 2] * m[:, 2]
            F, ct, eta_ti = self.fresnel(c)
            refl = u[:, 2] <= F
            k = np.where(refl, f(2) * c, eta_ti * c + ct)
            e = np.where(refl, f(1), eta_ti)
            wo = m * k[:, None] - wi * e[:, None]
            wo = np.where(live[:, None], wo, f(0))
            pdf = np.where(live, self.pdf(wi, wo), f(0))
            side = np.where(refl, ci * wo[:, 2] > 0, ci * wo[:, 2] < 0)
            keep = live & side & (pdf > 0)
            fc = self.f_cos(wi, wo)[:, None] * self._a(tint)[None, :]
            w = np.where(keep[:, None], fc / np.where(keep, pdf, f(1))[:, None], f(0))
        return (wo, pdf, w, refl, F) if details else (wo, pdf, w)

    def sample_weight(self, wi, wo, pdf_sa, tint=(1.0, 1.0, 1.0), threshold=3.5, active=None):
        """The tail of the full-sphere plugin's sample(): -> (weight [N,3], pdf [N])."""
        f = self.dt
        pdf_sa = self._a(pdf_sa)
        act = np.ones(pdf_sa.shape, bool) if active is None else np.asarray(active) != 0
        live = act & (pdf_sa > 0)
        with np.errstate(all="ignore"):
            value = np.where(live[:, None], self.eval(wi, wo, tint) / np.where(live, pdf_sa, f(1))[:, None], f(0))
        pdf = np.where(act & (value[:, 0] < f(threshold)), pdf_sa, f(0))
        return np.where((pdf > 0)[:, None], value, f(0)), pdf


# ---- what the reference's material list holds at idx 23..25 ----------------------------------------------------------
REFERENCE_ALPHA = {23: 0.2, 24: 0.3, 25: 0.5}


def sphere_dirs(rng, n, dtype=np.float64):
    """n directions uniform on the sphere."""
    z = rng.uniform(-1, 1, n)
    ph = rng.uniform(-np.pi, np.pi, n)
    r = np.sqrt(1 - z * z)
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], 1).astype(dtype)


def wi_of(theta, phi=0.0, n=1, dtype=np.float64):
    return np.tile(np.array([[np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)]], dtype=dtype), (n, 1))
