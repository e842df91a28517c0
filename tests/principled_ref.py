"""numpy restatement of the principled model of csrc/principled_dev.h (Burley's 2012 / 2015 BSDF with the choices Mitsuba's
`principled` makes: anisotropic GGX with the separable Smith G, exact unpolarised Fresnel mixed with Schlick terms, a GTR1
clearcoat, diffuse + retro-reflection + fake subsurface, sheen, radiance-mode transmission) and of its sampling map, statement
for statement, parameterised by dtype: fp64 is the reference of the tests, fp32 the yardstick (the same lines in the kernels'
arithmetic).

Directions are rows of [N,3] arrays in the local shading frame (x: the tangent the anisotropy refers to); the parameters are
rounded to fp32 first, as the descriptor the kernels read (``bsdfd_principled``) carries them, and the derived values are formed
from those in ``dtype`` — on the device side the launcher forms them in fp32.

The sampling map: the visible normal ``m`` of s * wi from the GGX distribution of visible normals (Heitz 2018: stretch, a disk
point warped towards the visible half, unstretch) at (u0, u1); u2 picks the lobe on the cumulative order diffuse, clearcoat,
transmission, reflection, whose first two thresholds are constants of the material; the four candidate directions are formed
and one is selected; pdf and eval of the chosen pair are then those of ``pdf`` / ``eval``.  One line differs in form: the
azimuths are cos / sin(2 pi u) here and ``sincospif(2 u)`` in the kernels (the same function, one rounding fewer there)."""
import numpy as np

MIN_HALF_LEN2 = 1e-12
LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_TRANSMISSION, LOBE_REFLECTION = 0, 1, 2, 3
PARAMS = ("roughness", "anisotropic", "metallic", "spec_trans", "eta", "spec_tint", "sheen", "sheen_tint", "flatness", "clearcoat",
          "clearcoat_gloss")


def eta_of_specular(specular):
    return 2.0 / (1.0 - np.sqrt(0.08 * specular)) - 1.0


class Principled:
    def __init__(self, base_color=(1.0, 1.0, 1.0), roughness=0.5, anisotropic=0.0, metallic=0.0, spec_trans=0.0, eta=1.5,
                 spec_tint=0.0, sheen=0.0, sheen_tint=0.0, flatness=0.0, clearcoat=0.0, clearcoat_gloss=0.0, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        f = self.dt
        given = dict(roughness=roughness, anisotropic=anisotropic, metallic=metallic, spec_trans=spec_trans, eta=eta,
                     spec_tint=spec_tint, sheen=sheen, sheen_tint=sheen_tint, flatness=flatness, clearcoat=clearcoat,
                     clearcoat_gloss=clearcoat_gloss)
        for k in PARAMS:
            setattr(self, k, f(np.float32(given[k])))
        self.base = np.array([f(np.float32(c)) for c in base_color], dtype=self.dt)
        self.pi = f(np.pi)
        self.inv_pi = f(1 / np.pi)
        # ---- derived, wave-uniform (principled_dev.h: derive()) ----
        self.inv_eta = f(1) / self.eta
        aspect = np.sqrt(f(1) - f(0.9) * self.anisotropic)
        r2 = self.roughness * self.roughness
        self.ax = np.maximum(f(1e-3), r2 / aspect)
        self.ay = np.maximum(f(1e-3), r2 * aspect)
        self.inv_ax, self.inv_ay = f(1) / self.ax, f(1) / self.ay
        self.d_norm = f(1) / (self.pi * self.ax * self.ay)
        a_cc = (f(1) - self.clearcoat_gloss) * f(0.1) + self.clearcoat_gloss * f(0.001)
        self.a2_cc = a_cc * a_cc
        self.ln_a2_cc = np.log(self.a2_cc)
        self.brdf = (f(1) - self.metallic) * (f(1) - self.spec_trans)
        self.bsdf = (f(1) - self.metallic) * self.spec_trans
        lum = f(0.212671) * self.base[0] + f(0.715160) * self.base[1] + f(0.072169) * self.base[2]
        self.c_tint = np.array([c / lum if lum > 0 else f(1) for c in self.base], dtype=self.dt)
        self.sqrt_base = np.sqrt(self.base)
        r0 = (self.eta - f(1)) / (self.eta + f(1))
        self.r0_eta = r0 * r0
        self.p_c = f(0.25) * self.clearcoat
        self.inv_sum = f(1) / (f(1) + self.p_c + self.brdf)
        self.cum_d = self.brdf * self.inv_sum
        self.cum_c = (self.brdf + self.p_c) * self.inv_sum

    def _a(self, x):
        return np.ascontiguousarray(x, dtype=self.dt)

    # ---- the terms ----------------------------------------------------------------------------------------------------
    def half_vector(self, wi, wo):
        """-> (h [N,3] with h.z >= 0, reflect, eta_path, ok): ok is False where the generalised half vector is undefined."""
        f = self.dt
        ci, co = wi[:, 2], wo[:, 2]
        refl = ci * co > 0
        eta = np.where(ci > 0, self.eta, self.inv_eta)
        k = np.where(refl, f(1), eta)
        hx, hy, hz = wi[:, 0] + wo[:, 0] * k, wi[:, 1] + wo[:, 1] * k, wi[:, 2] + wo[:, 2] * k
        len2 = hx * hx + hy * hy + hz * hz
        ok = len2 > f(MIN_HALF_LEN2)
        inv = np.where(ok, f(1) / np.sqrt(np.where(ok, len2, f(1))), f(0))
        inv = np.where(hz < 0, -inv, inv)
        return np.stack([hx * inv, hy * inv, hz * inv], 1), refl, eta, ok

    def ggx_d(self, h):
        f = self.dt
        x, y = h[:, 0] * self.inv_ax, h[:, 1] * self.inv_ay
        t = x * x + y * y + h[:, 2] * h[:, 2]
        d = self.d_norm / (t * t)
        return np.where(d * h[:, 2] > f(1e-20), d, f(0))

    def g1(self, v, dot_vh, ax, ay):
        """The separable Smith term of one direction for the roughness pair (ax, ay)."""
        f = self.dt
        x, y = ax * v[:, 0], ay * v[:, 1]
        xy = x * x + y * y
        g = f(2) / (f(1) + np.sqrt(f(1) + xy / (v[:, 2] * v[:, 2])))
        g = np.where(xy == 0, f(1), g)
        return np.where(dot_vh * v[:, 2] <= 0, f(0), g)

    def gtr1(self, hz):
        return (self.a2_cc - self.dt(1)) / (self.pi * self.ln_a2_cc * (self.dt(1) + (self.a2_cc - self.dt(1)) * hz * hz))

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
        eta_it = np.where(outside, self.eta, self.inv_eta)
        eta_ti = np.where(outside, self.inv_eta, self.eta)
        ct2 = f(1) - eta_ti * eta_ti * (f(1) - c * c)
        ct = np.sqrt(np.maximum(ct2, f(0)))
        return self.fresnel_of(eta_it, np.abs(c), ct), np.where(c > 0, -ct, ct), eta_ti

    def sw(self, c):
        """Schlick's weight clamp(1 - c, 0, 1)^5."""
        f = self.dt
        x = np.minimum(np.maximum(f(1) - c, f(0)), f(1))
        x2 = x * x
        return x2 * x2 * x

    def schlick_general(self, r0, c):
        """The Schlick term as Mitsuba states it for either sign of c.  The model only takes it at c >= 0 (the front side), where
        it is r0 + (1 - r0) sw(c) — the form the lobes below use; kept for the test that says so."""
        f = self.dt
        eta_it = np.where(c >= 0, self.eta, self.inv_eta)
        cos_t = np.sqrt(np.maximum(f(0), f(1) - (f(1) - c * c) / (eta_it * eta_it)))
        return r0 + (f(1) - r0) * self.sw(np.where(eta_it > 1, np.abs(c), cos_t))

    def _terms(self, wi, wo):
        f = self.dt
        h, refl, eta, ok = self.half_vector(wi, wo)
        ci, co = wi[:, 2], wo[:, 2]
        dwi = wi[:, 0] * h[:, 0] + wi[:, 1] * h[:, 1] + wi[:, 2] * h[:, 2]
        dwo = wo[:, 0] * h[:, 0] + wo[:, 1] * h[:, 1] + wo[:, 2] * h[:, 2]
        # across the surface the generalised half vector obeys Snell's law by construction: |wo . h| IS the transmitted cosine
        F = np.where(refl, self.fresnel(dwi)[0], self.fresnel_of(np.where(dwi >= 0, self.eta, self.inv_eta), np.abs(dwi), np.abs(dwo)))
        front = ci > 0
        s_dwi, s_dwo = np.where(front, dwi, -dwi), np.where(front, dwo, -dwo)
        t = dict(h=h, reflect=refl, refract=ci * co < 0, eta=eta, ok=ok & (ci != 0), front=front, dwi=dwi, dwo=dwo, F=F,
                 s=dwi + eta * dwo, D=self.ggx_d(h), compat_r=(s_dwi > 0) & (s_dwo > 0), compat_t=(s_dwi > 0) & (s_dwo < 0),
                 Dcc=self.gtr1(h[:, 2]))
        return t

    # ---- eval / pdf ---------------------------------------------------------------------------------------------------
    def eval(self, wi, wo, tint=(1.0, 1.0, 1.0)):
        """f(wi, wo) |cos theta_o| * tint -> [N,3]."""
        f = self.dt
        wi, wo = self._a(wi), self._a(wo)
        tint = self._a(tint)
        with np.errstate(all="ignore"):
            t = self._terms(wi, wo)
            ci, co = wi[:, 2], wo[:, 2]
            aci, aco = np.abs(ci), np.abs(co)
            F, D, dwi, dwo, front, refl = t["F"], t["D"], t["dwi"], t["dwo"], t["front"], t["reflect"]
            G = self.g1(wi, dwi, self.ax, self.ay) * self.g1(wo, dwo, self.ax, self.ay)
            m_spec = refl & t["compat_r"] & (F > 0)
            m_trans = (self.bsdf > 0) & t["refract"] & t["compat_t"] & (F < 1)
            m_front = refl & front
            spec = np.where(m_spec, D * G / (f(4) * aci), f(0))
            trans = np.where(m_trans, self.bsdf * np.abs((f(1) - F) * D * G * dwi * dwo / (ci * (t["s"] * t["s"]))), f(0))
            sch = self.sw(np.abs(dwi))
            Gcc = self.g1(wi, dwi, f(0.25), f(0.25)) * self.g1(wo, dwo, f(0.25), f(0.25))
            cc = np.where(m_front & (self.clearcoat > 0), self.p_c * (f(0.04) + f(0.96) * sch) * t["Dcc"] * Gcc * aco, f(0))
            Fo, Fi = self.sw(aco), self.sw(aci)
            f_d = (f(1) - f(0.5) * Fi) * (f(1) - f(0.5) * Fo)
            Rr = f(2) * self.roughness * dwo * dwo
            f_r = Rr * (Fo + Fi + Fo * Fi * (Rr - f(1)))
            Fss = (f(1) + (f(0.5) * Rr - f(1)) * Fo) * (f(1) + (f(0.5) * Rr - f(1)) * Fi)
            f_ss = f(1.25) * (Fss * (f(1) / (aco + aci) - f(0.5)) + f(0.5))
            diff = np.where(m_front & (self.brdf > 0),
                            self.brdf * aco * self.inv_pi * ((f(1) - self.flatness) * (f_d + f_r) + self.flatness * f_ss), f(0))
            sheen = np.where(m_front & (self.sheen > 0) & (self.metallic < 1),
                             self.sheen * (f(1) - self.metallic) * self.sw(np.abs(dwo)) * aco, f(0))
            out = []
            for k in range(3):
                base, ctint = self.base[k], self.c_tint[k]
                r0c = ctint * self.r0_eta
                Fp = ((f(1) - self.metallic) * (f(1) - self.spec_tint) * F + self.metallic * (base + (f(1) - base) * sch)
                      + (f(1) - self.metallic) * self.spec_tint * (r0c + (f(1) - r0c) * sch))
                Fp = np.where(front, Fp, self.bsdf * F)
                v = (Fp * spec + self.sqrt_base[k] * trans + cc + base * diff
                     + (f(1) + (ctint - f(1)) * self.sheen_tint) * sheen)
                out.append(np.where(t["ok"] & np.isfinite(v), v, f(0)) * tint[k])
            return np.stack(out, 1)

    def pdf(self, wi, wo):
        f = self.dt
        wi, wo = self._a(wi), self._a(wo)
        with np.errstate(all="ignore"):
            t = self._terms(wi, wo)
            ci, co = wi[:, 2], wo[:, 2]
            F, dwi, dwo, front, refl = t["F"], t["dwi"], t["dwo"], t["front"], t["reflect"]
            vis = t["D"] * self.g1(wi, dwi, self.ax, self.ay) * np.abs(dwi) / np.abs(ci)
            p_t = np.where(front, self.bsdf * (f(1) - F) * self.inv_sum, f(1) - F)
            p_r = np.where(front, (f(1) - self.bsdf * (f(1) - F)) * self.inv_sum, F)
            p_c = np.where(front, self.p_c * self.inv_sum, f(0))
            p_d = np.where(front, self.cum_d, f(0))
            jac = np.where(refl, f(1) / (f(4) * np.abs(dwo)), np.abs(t["eta"] * t["eta"] * dwo / (t["s"] * t["s"])))
            on_r = np.where(refl & t["compat_r"], (p_r * vis + p_c * t["Dcc"] * t["h"][:, 2]) * jac, f(0))
            on_t = np.where(t["refract"] & t["compat_t"], p_t * vis * jac, f(0))
            p = on_r + on_t + np.where(refl, p_d * np.maximum(co, f(0)) * self.inv_pi, f(0))
            live = t["ok"] & (front | (self.bsdf > 0))
            return np.where(live & np.isfinite(p) & (p > 0), p, f(0))

    # ---- sampling -----------------------------------------------------------------------------------------------------
    def sample_normal(self, v, u0, u1):
        """v = s * wi (v.z > 0) -> the visible normal m [N,3] (Heitz 2018)."""
        f = self.dt
        v, u0, u1 = self._a(v), self._a(u0), self._a(u1)
        with np.errstate(all="ignore"):
            sx, sy, sz = self.ax * v[:, 0], self.ay * v[:, 1], v[:, 2]
            inv = f(1) / np.sqrt(sx * sx + sy * sy + sz * sz)
            sx, sy, sz = sx * inv, sy * inv, sz * inv
            len2 = sx * sx + sy * sy
            flat = len2 > 0
            il = np.where(flat, f(1) / np.sqrt(np.where(flat, len2, f(1))), f(0))
            t1x, t1y = np.where(flat, -sy * il, f(1)), np.where(flat, sx * il, f(0))
            t2x, t2y, t2z = -sz * t1y, sz * t1x, sx * t1y - sy * t1x          # cross(Vh, T1), T1.z = 0
            r = np.sqrt(u0)
            phi = f(2) * self.pi * u1
            p1, p2 = r * np.cos(phi), r * np.sin(phi)
            s = f(0.5) * (f(1) + sz)
            p2 = (f(1) - s) * np.sqrt(np.maximum(f(1) - p1 * p1, f(0))) + s * p2
            p3 = np.sqrt(np.maximum(f(1) - p1 * p1 - p2 * p2, f(0)))
            nx = p1 * t1x + p2 * t2x + p3 * sx
            ny = p1 * t1y + p2 * t2y + p3 * sy
            nz = p2 * t2z + p3 * sz
            mx, my, mz = self.ax * nx, self.ay * ny, np.maximum(nz, f(0))
            inv = f(1) / np.sqrt(mx * mx + my * my + mz * mz)
            return np.stack([mx * inv, my * inv, mz * inv], 1)

    def candidates(self, wi, u):
        """-> (m, F at wi . m, the four candidate directions [4,N,3] in lobe order, m_cc)."""
        f = self.dt
        ci = wi[:, 2]
        s = np.where(ci > 0, f(1), f(-1))
        m = self.sample_normal(wi * s[:, None], u[:, 0], u[:, 1])
        c = wi[:, 0] * m[:, 0] + wi[:, 1] * m[:, 1] + wi[:, 2] * m[:, 2]
        F, ct, eta_ti = self.fresnel(c)
        wo_r = m * (f(2) * c)[:, None] - wi
        wo_t = m * (eta_ti * c + ct)[:, None] - wi * eta_ti[:, None]
        # GTR1 normal of the clearcoat
        cos2 = (f(1) - np.exp((f(1) - u[:, 1]) * self.ln_a2_cc)) / (f(1) - self.a2_cc)
        cos2 = np.minimum(np.maximum(cos2, f(0)), f(1))
        cth, sth = np.sqrt(cos2), np.sqrt(f(1) - cos2)
        phi = f(2) * self.pi * u[:, 0]
        mcc = np.stack([sth * np.cos(phi), sth * np.sin(phi), cth], 1)
        ccc = wi[:, 0] * mcc[:, 0] + wi[:, 1] * mcc[:, 1] + wi[:, 2] * mcc[:, 2]
        wo_c = mcc * (f(2) * ccc)[:, None] - wi
        # cosine hemisphere, always +z
        r = np.sqrt(u[:, 0])
        phi = f(2) * self.pi * u[:, 1]
        wo_d = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(f(1) - u[:, 0])], 1)
        return m, F, np.stack([wo_d, wo_c, wo_t, wo_r]), mcc

    def thresholds(self, wi, F):
        """Cumulative lobe thresholds (diffuse, clearcoat, transmission) per row."""
        f = self.dt
        front = wi[:, 2] > 0
        cum_d = np.where(front, self.cum_d, f(0))
        cum_c = np.where(front, self.cum_c, f(0))
        cum_t = cum_c + np.where(front, self.bsdf * (f(1) - F) * self.inv_sum, f(1) - F)
        return cum_d, cum_c, cum_t

    def sample(self, wi, u, tint=(1.0, 1.0, 1.0), active=None, details=False):
        """-> (wo [N,3], pdf [N], weight [N,3]); a failed sample is all zeros.  With ``details`` also a dict: lobe [N], F [N],
        candidates [4,N,3], thresholds (cum_d, cum_c, cum_t)."""
        f = self.dt
        wi, u = self._a(wi), self._a(u)
        with np.errstate(all="ignore"):
            ci = wi[:, 2]
            live = (ci != 0) & ((ci > 0) | (self.bsdf > 0))
            if active is not None:
                live &= np.asarray(active) != 0
            m, F, cand, mcc = self.candidates(wi, u)
            cum_d, cum_c, cum_t = self.thresholds(wi, F)
            u2 = u[:, 2]
            lobe = np.where(u2 < cum_d, LOBE_DIFFUSE, np.where(u2 < cum_c, LOBE_CLEARCOAT, np.where(u2 < cum_t, LOBE_TRANSMISSION,
                                                                                                   LOBE_REFLECTION)))
            wo = np.where((lobe == 0)[:, None], cand[0], np.where((lobe == 1)[:, None], cand[1],
                                                                  np.where((lobe == 2)[:, None], cand[2], cand[3])))
            n = np.where((lobe == LOBE_CLEARCOAT)[:, None], mcc, m)        # the normal the compat test reads
            s = np.where(ci > 0, f(1), f(-1))
            dn_i = s * (wi[:, 0] * n[:, 0] + wi[:, 1] * n[:, 1] + wi[:, 2] * n[:, 2])
            dn_o = s * (wo[:, 0] * n[:, 0] + wo[:, 1] * n[:, 1] + wo[:, 2] * n[:, 2])
            trans = lobe == LOBE_TRANSMISSION
            side = np.where(trans, ci * wo[:, 2] < 0, ci * wo[:, 2] > 0)
            compat = (lobe == LOBE_DIFFUSE) | ((dn_i > 0) & np.where(trans, dn_o < 0, dn_o > 0))
            good = live & side & compat
            wo = np.where(good[:, None], wo, f(0))
            pdf = np.where(good, self.pdf(wi, wo), f(0))
            good &= pdf > 0
            wo = np.where(good[:, None], wo, f(0))
            fc = self.eval(wi, wo, tint)
            w = np.where(good[:, None], fc / np.where(good, pdf, f(1))[:, None], f(0))
        if details:
            return wo, pdf, w, dict(lobe=lobe, F=F, candidates=cand, thresholds=(cum_d, cum_c, cum_t), ok=good)
        return wo, pdf, w

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


# ---- what the reference's material list holds at idx 0..22: (metallic, specular, roughness, anisotropic) -------------
REFERENCE_ROWS = {
    0: (.1, 1, .2, .5), 1: (.3, .7, .5, .5), 2: (1, .8, .1, .5), 3: (.2, .3, .3, .7), 4: (.1, .8, .3, .7), 5: (.1, 1, .1, .7),
    6: (.9, .7, .3, .7), 7: (.5, .8, .3, .7), 8: (.1, .8, .3, .7), 9: (.3, .2, .1, .7), 10: (0, 1, .1, .7), 11: (.8, .2, .1, .7),
    12: (.6, .2, .3, .7), 13: (.3, .2, .7, .7), 14: (.9, .2, .5, .7), 15: (.9, .2, .3, .7), 16: (.9, .2, .6, .7), 17: (.9, .2, .9, .7),
    18: (.1, .8, .1, .7), 19: (.1, .5, .4, .7), 20: (.1, .8, .3, .7), 21: (.1, .5, .7, .7), 22: (.1, .3, .8, .7),
}
REFERENCE_COMMON = dict(base_color=(1.0, 1.0, 1.0), spec_tint=0.5, sheen=0.5, sheen_tint=0.5, clearcoat=0.5, clearcoat_gloss=0.5,
                        spec_trans=0.9, flatness=1.0)


def reference_params(idx):
    metallic, specular, roughness, anisotropic = REFERENCE_ROWS[idx]
    p = dict(REFERENCE_COMMON, metallic=metallic, roughness=roughness, anisotropic=anisotropic, eta=eta_of_specular(specular))
    if idx == 7:
        p["sheen_tint"] = 0.3
    return p


def reference(idx, dtype=np.float64):
    return Principled(dtype=dtype, **reference_params(idx))


def sphere_dirs(rng, n, dtype=np.float64):
    """n directions uniform on the sphere."""
    z = rng.uniform(-1, 1, n)
    ph = rng.uniform(-np.pi, np.pi, n)
    r = np.sqrt(1 - z * z)
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], 1).astype(dtype)


def wi_of(theta, phi=0.0, n=1, dtype=np.float64):
    return np.tile(np.array([[np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)]], dtype=dtype), (n, 1))
