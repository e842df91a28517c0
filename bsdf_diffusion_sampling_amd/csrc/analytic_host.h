// analytic_host.h — host side of the two analytic descriptors: their checks and what is derived from them, once per call
// (principled.hip, dielectric.hip) or once per table (analytic_table.hip).  One statement of each, so that a table row is handed
// the very descriptor the single-material kernel gets.  (The device side the three share: analytic_rows.h; the count checks and
// the launch: rows.h.)
#pragma once
#include <cmath>

#include "bsdfd.h"
#include "dielectric_dev.h"
#include "principled_dev.h"

namespace dielectric_dev {

// the first complaint about a descriptor, or null
inline const char* descriptor_error(const bsdfd_dielectric& desc) {
    if (desc.distribution != 0) return "bsdfd_dielectric.distribution: only 0 (Beckmann) is built";
    if (!(desc.alpha > 0.0f && std::isfinite(desc.alpha) && desc.eta > 0.0f && std::isfinite(desc.eta)))
        return "bsdfd_dielectric: alpha and eta must be positive and finite";
    return nullptr;
}

inline DielectricDev derive(const bsdfd_dielectric& desc) { return DielectricDev{desc.alpha, desc.eta, 1.0f / desc.eta}; }

}  // namespace dielectric_dev

namespace principled_dev {

// the first complaint about a descriptor, or null
inline const char* descriptor_error(const bsdfd_principled& desc) {
    const float unit[] = {desc.base_color[0], desc.base_color[1], desc.base_color[2], desc.roughness, desc.anisotropic,
                          desc.metallic, desc.spec_trans, desc.spec_tint, desc.sheen, desc.sheen_tint, desc.flatness,
                          desc.clearcoat, desc.clearcoat_gloss};
    for (float v : unit)
        if (!(v >= 0.0f && v <= 1.0f))   // (false for NaN)
            return "bsdfd_principled: every parameter but eta must be finite and in [0, 1]";
    if (!(desc.eta >= 1.0f && std::isfinite(desc.eta))) return "bsdfd_principled.eta must be finite and >= 1";
    if (desc.eta == 1.0f && desc.spec_trans != 0.0f) return "bsdfd_principled: eta == 1 (no interface) needs spec_trans == 0";
    return nullptr;
}

// what depends on the material alone, in fp32 (tests/principled_ref.py forms the same values in its dtype)
inline PrincipledDev derive(const bsdfd_principled& p) {
    PrincipledDev d{};
    const float lum = 0.212671f * p.base_color[0] + 0.715160f * p.base_color[1] + 0.072169f * p.base_color[2];
    for (int k = 0; k < 3; ++k) {
        d.base[k] = p.base_color[k];
        d.sqrt_base[k] = std::sqrt(p.base_color[k]);
        d.c_tint[k] = lum > 0.0f ? p.base_color[k] / lum : 1.0f;
    }
    d.roughness = p.roughness; d.metallic = p.metallic; d.spec_tint = p.spec_tint; d.sheen = p.sheen;
    d.sheen_tint = p.sheen_tint; d.flatness = p.flatness; d.clearcoat = p.clearcoat;
    d.eta = p.eta;
    d.inv_eta = 1.0f / p.eta;
    const float aspect = std::sqrt(1.0f - 0.9f * p.anisotropic);
    const float r2 = p.roughness * p.roughness;
    d.ax = std::fmax(1e-3f, r2 / aspect);
    d.ay = std::fmax(1e-3f, r2 * aspect);
    d.inv_ax = 1.0f / d.ax;
    d.inv_ay = 1.0f / d.ay;
    d.d_norm = 1.0f / (kPi * d.ax * d.ay);
    const float a_cc = (1.0f - p.clearcoat_gloss) * 0.1f + p.clearcoat_gloss * 0.001f;
    d.a2_cc = a_cc * a_cc;
    d.ln_a2_cc = std::log(d.a2_cc);
    d.brdf = (1.0f - p.metallic) * (1.0f - p.spec_trans);
    d.bsdf = (1.0f - p.metallic) * p.spec_trans;
    const float r0 = (p.eta - 1.0f) / (p.eta + 1.0f);
    d.r0_eta = r0 * r0;
    d.p_c = 0.25f * p.clearcoat;
    d.inv_sum = 1.0f / (1.0f + d.p_c + d.brdf);
    d.cum_d = d.brdf * d.inv_sum;
    d.cum_c = (d.brdf + d.p_c) * d.inv_sum;
    return d;
}

}  // namespace principled_dev
