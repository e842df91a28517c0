// measured.hip — ground-truth evaluator behind the plugins' eval(): the RGL measured-BSDF model.
//
// The reference's plugins build Mitsuba 3's `measured` BSDF on `measuredbsdfs/<name>.bsdf`
// (rendering/brdf_measured_disk.py:36-42) and call its eval() for the sample weight f/pdf and the
// firefly rule (:96-100, :107-110).  Mitsuba has no AMD GPU variant, so the drop-in carries its own
// evaluator of the published model (Dupuy & Jakob, SIGGRAPH Asia 2018):
//
//     f(wi, wo) cos(theta_o) = spec(s; phi_i, theta_i) * D(u_m) / (4 sigma(u_i)),
//     u = (sqrt(2 theta / pi), (phi + pi) / 2 pi),   s = VNDF^-1(u_m | phi_i, theta_i),
//
// every table a bilinear grid over [0,1]^2, linearly interpolated over the incident-direction
// parameters; VNDF^-1 is the inverse of the inverse-CDF warp of that interpolated density
// (marginal over azimuth rows, conditional over elevation columns).  The host part parses the
// tensor file and builds the normalised VNDF with its conditional / marginal CDFs in double;
// the kernel is one thread per (wi, wo) pair: ~60 gathers from tables that total < 1 MB (L2-resident),
// i.e. latency- not bandwidth-bound; it is not part of the neural hot path.
//
// The same files carry their own importance sampler (luminance warp, VNDF warp, reflection about the half vector):
// bsdfd_measured_sample / bsdfd_measured_pdf below; the device side of both is measured_dev.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "measured_dev.h"

using namespace measured_dev;

namespace {

struct Field {
    int dtype;
    std::vector<uint64_t> shape;
    const unsigned char* ptr;
    size_t count() const {
        size_t n = 1;
        for (auto s : shape) n *= (size_t)s;
        return n;
    }
    // element count with the shape fields validated: every dimension <= 2^26 and no wrap-around of the product (a
    // crafted shape that wraps to a small product would pass the "fits in the file" test and then index out of bounds)
    bool count_checked(size_t* out) const {
        size_t n = 1;
        for (auto s : shape) {
            if (s > (1ull << 26)) return false;
            if (__builtin_mul_overflow(n, (size_t)s, &n)) return false;
        }
        *out = n;
        return true;
    }
};

// One thread per row; the rows themselves are measured_dev.h's, shared with measured_table.hip.
// eval(): rgb_out = f cos * tint
__global__ __launch_bounds__(256) void measured_eval_kernel(MeasuredDev m, const float* __restrict__ wi,
                                                            const float* __restrict__ wo, long long n, Tint tint,
                                                            float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    eval_row(m, wi, wo, nullptr, q, tint, out, nullptr);
}

// the tail of the plugins' sample(): weight = f * tint / pdf with the firefly rule
__global__ __launch_bounds__(256) void measured_weight_kernel(MeasuredDev m, const float* __restrict__ wi,
                                                              const float* __restrict__ wo,
                                                              const float* __restrict__ pdf_in,
                                                              const unsigned char* __restrict__ active, long long n,
                                                              Tint tint, float thr, float* __restrict__ weight,
                                                              float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    weight_row(m, wi, wo, pdf_in, active, q, tint, thr, weight, pdf_out);
}

// sample(): the file's own importance sampler, one query per lane
__global__ __launch_bounds__(256) void measured_sample_kernel(MeasuredDev m, const float* __restrict__ wi,
                                                              const float* __restrict__ u,
                                                              const unsigned char* __restrict__ active, long long n,
                                                              Tint tint, float* __restrict__ wo_out,
                                                              float* __restrict__ pdf_out, float* __restrict__ weight_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    sample_row(m, wi, u, active, q, tint, wo_out, pdf_out, weight_out);
}

// pdf(): the density of that sampler at a given wo
__global__ __launch_bounds__(256) void measured_pdf_kernel(MeasuredDev m, const float* __restrict__ wi,
                                                           const float* __restrict__ wo,
                                                           const unsigned char* __restrict__ active, long long n,
                                                           float* __restrict__ pdf_out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    pdf_row(m, wi, wo, active, q, pdf_out);
}

int upload(bsdfd_measured_ctx* h, const std::vector<float>& v, const float** out) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(float)));
    h->allocs.push_back(p);
    HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = static_cast<const float*>(p);
    return BSDFD_OK;
}

std::vector<float> as_f32(const Field& f) {
    std::vector<float> v(f.count());
    std::memcpy(v.data(), f.ptr, v.size() * sizeof(float));
    return v;
}

// the host path of the four launchers: `kernel` over N rows of h's material, `args` behind the descriptor
template <class... P, class... A>
int measured_launch(bsdfd_measured_handle h, int64_t n, bool pointers_given, void (*kernel)(P...), void* stream, A... args) {
    if (!h) return bsdfd_fail_(BSDFD_EINVAL, "null handle");
    if (int rc = rows::launch_checks(n, rows::kMaxRowsSingle, "measured handle", &h->device)) return rc;
    return launch_rows(n, pointers_given ? nullptr : "null pointer", kernel, stream, h->dev, args...);
}

}  // namespace

extern "C" {

int bsdfd_measured_create_from_file(const char* path, bsdfd_measured_handle* out) {
    if (!path || !out) return bsdfd_fail_(BSDFD_EINVAL, "null argument");
    *out = nullptr;
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return bsdfd_fail_(BSDFD_EIO, std::string("cannot open ") + path);
    std::vector<unsigned char> raw;
    {
        std::fseek(fp, 0, SEEK_END);
        const long sz = std::ftell(fp);
        std::fseek(fp, 0, SEEK_SET);
        raw.resize(sz > 0 ? (size_t)sz : 0);
        const size_t got = raw.empty() ? 0 : std::fread(raw.data(), 1, raw.size(), fp);
        std::fclose(fp);
        if (got != raw.size()) return bsdfd_fail_(BSDFD_EIO, std::string("short read: ") + path);
    }
    // Mitsuba TensorFile: "tensor_file\0", u8 major, u8 minor, u32 n_fields, then per field:
    // u16 name_len, name, u16 ndim, u8 dtype, u64 offset, u64 shape[ndim]
    if (raw.size() < 18 || std::memcmp(raw.data(), "tensor_file", 12) != 0)
        return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": not a tensor file");
    if (raw[12] != 1 || raw[13] != 0) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": unsupported tensor file version");
    uint32_t nf;
    std::memcpy(&nf, raw.data() + 14, 4);
    size_t pos = 18;
    std::map<std::string, Field> fields;
    static const int dtype_size[12] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 2, 4, 8};
    for (uint32_t i = 0; i < nf; ++i) {
        auto need = [&](size_t k) { return pos + k <= raw.size(); };
        uint16_t nl, nd;
        if (!need(2)) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": truncated header");
        std::memcpy(&nl, raw.data() + pos, 2); pos += 2;
        if (!need((size_t)nl + 11)) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": truncated header");
        std::string name(reinterpret_cast<const char*>(raw.data() + pos), nl); pos += nl;
        std::memcpy(&nd, raw.data() + pos, 2); pos += 2;
        Field f;
        f.dtype = raw[pos]; pos += 1;
        uint64_t off;
        std::memcpy(&off, raw.data() + pos, 8); pos += 8;
        if (!need(8 * (size_t)nd)) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": truncated header");
        f.shape.resize(nd);
        std::memcpy(f.shape.data(), raw.data() + pos, 8 * (size_t)nd); pos += 8 * (size_t)nd;
        if (f.dtype < 1 || f.dtype > 11) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": bad dtype in field " + name);
        size_t cnt = 0, bytes = 0;
        if (!f.count_checked(&cnt) || __builtin_mul_overflow(cnt, (size_t)dtype_size[f.dtype], &bytes))
            return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": implausible shape in field " + name);
        if (off > raw.size() || bytes > raw.size() - off)
            return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": field " + name + " exceeds the file");
        f.ptr = raw.data() + off;
        fields[name] = f;
    }
    auto want = [&](const char* name, int dtype, size_t ndim) -> const Field* {
        auto it = fields.find(name);
        if (it == fields.end() || it->second.dtype != dtype || it->second.shape.size() != ndim) return nullptr;
        return &it->second;
    };
    const Field *phi = want("phi_i", 10, 1), *theta = want("theta_i", 10, 1), *sigma = want("sigma", 10, 2),
                *ndf = want("ndf", 10, 2), *vndf = want("vndf", 10, 4), *rgb = want("rgb", 10, 5),
                *jac = want("jacobian", 1, 1);
    // optional: the luminance warp of the file's own sampler (bsdfd_measured_sample); eval() does not read it
    const Field* lum = nullptr;
    if (auto it = fields.find("luminance"); it != fields.end()) {
        lum = &it->second;
        if (lum->dtype != 10 || lum->shape.size() != 4)
            return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": luminance must be an fp32 field of rank 4 [n_phi][n_theta][h][w]");
    }
    if (!phi || !theta || !sigma || !ndf || !vndf || !rgb || !jac)
        return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": expected fp32 fields phi_i, theta_i, sigma, ndf, vndf, rgb and u8 "
                                                           "jacobian (spectral files are not supported; use the *_rgb.bsdf flavour)");
    for (const Field* f : {phi, theta, sigma, ndf, vndf, rgb})  // table extents are used as int indices below
        for (auto dim : f->shape)
            if (dim < 1 || dim > (1u << 20))
                return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": table dimension out of range [1, 2^20]");
    if (lum)
        for (auto dim : lum->shape)
            if (dim < 1 || dim > (1u << 20))
                return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": table dimension out of range [1, 2^20]");
    if (jac->shape[0] < 1) return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": empty jacobian field");
    const int n_phi = (int)phi->shape[0], n_theta = (int)theta->shape[0];
    if ((int)vndf->shape[0] != n_phi || (int)vndf->shape[1] != n_theta || (int)rgb->shape[0] != n_phi ||
        (int)rgb->shape[1] != n_theta || rgb->shape[2] != 3 || vndf->shape[2] < 2 || vndf->shape[3] < 2 ||
        rgb->shape[3] < 2 || rgb->shape[4] < 2 || ndf->shape[0] < 2 || ndf->shape[1] < 2 || sigma->shape[0] < 2 ||
        sigma->shape[1] < 2)
        return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": inconsistent table shapes");
    if (lum && ((int)lum->shape[0] != n_phi || (int)lum->shape[1] != n_theta || lum->shape[2] < 2 || lum->shape[3] < 2))
        return bsdfd_fail_(BSDFD_EIO, std::string(path) + ": luminance does not match phi_i / theta_i (inconsistent table shapes)");

    int devid = -1;
    HIP_TRY(hipGetDevice(&devid));
    bsdfd_measured_ctx* h = new bsdfd_measured_ctx();
    h->device = devid;
    if (auto it = fields.find("description"); it != fields.end())
        h->description.assign(reinterpret_cast<const char*>(it->second.ptr), it->second.count());
    MeasuredDev& d = h->dev;
    d.n_phi = n_phi; d.n_theta = n_theta;
    d.isotropic = n_phi <= 2;
    d.jacobian = jac->ptr[0] ? 1 : 0;
    d.reduction = 0;
    const std::vector<float> phi_v = as_f32(*phi), theta_v = as_f32(*theta);
    d.fold_x = d.fold_y = 1.0f;
    if (!d.isotropic) {
        d.reduction = (int)std::lrint(2.0 * M_PI / ((double)phi_v[n_phi - 1] - (double)phi_v[0]));
        const double mid = 0.5 * ((double)phi_v[0] + (double)phi_v[n_phi - 1]);
        d.fold_x = std::cos(mid) < 0.0 ? -1.0f : 1.0f;
        d.fold_y = std::sin(mid) < 0.0 ? -1.0f : 1.0f;
    }

    // Warps (VNDF, luminance): per-slice normalisation and CDFs in double.  Integrals in patch units: a linear segment
    // integrates to the mean of its end points, a row of patches to the mean of its two vertex rows.
    auto build_warp = [&](const Field& f, std::vector<float>& data, std::vector<float>& cdf_cond, std::vector<float>& cdf_marg) {
        const int vh = (int)f.shape[2], vw = (int)f.shape[3];
        const std::vector<float> vraw = as_f32(f);
        data.resize(vraw.size()); cdf_cond.resize(vraw.size()); cdf_marg.resize((size_t)n_phi * n_theta * vh);
        std::vector<double> cond((size_t)vh * vw), marg(vh);
        for (int s = 0; s < n_phi * n_theta; ++s) {
            const float* src = vraw.data() + (size_t)s * vh * vw;
            for (int y = 0; y < vh; ++y) {
                double acc = 0.0;
                cond[(size_t)y * vw] = 0.0;
                for (int x = 1; x < vw; ++x) {
                    acc += 0.5 * ((double)src[(size_t)y * vw + x - 1] + (double)src[(size_t)y * vw + x]);
                    cond[(size_t)y * vw + x] = acc;
                }
            }
            double acc = 0.0;
            marg[0] = 0.0;
            for (int y = 1; y < vh; ++y) {
                acc += 0.5 * (cond[(size_t)(y - 1) * vw + vw - 1] + cond[(size_t)y * vw + vw - 1]);
                marg[y] = acc;
            }
            const double scale = acc > 0.0 ? 1.0 / acc : 0.0;
            for (size_t i = 0; i < (size_t)vh * vw; ++i) {
                data[(size_t)s * vh * vw + i] = (float)((double)src[i] * scale);
                cdf_cond[(size_t)s * vh * vw + i] = (float)(cond[i] * scale);
            }
            for (int y = 0; y < vh; ++y) cdf_marg[(size_t)s * vh + y] = (float)(marg[y] * scale);
        }
    };
    const int vh = (int)vndf->shape[2], vw = (int)vndf->shape[3];
    std::vector<float> vdata, vcond, vmarg, ldata, lcond, lmarg;
    build_warp(*vndf, vdata, vcond, vmarg);
    if (lum) build_warp(*lum, ldata, lcond, lmarg);
    int rc = BSDFD_OK;
    auto up = [&](const std::vector<float>& v, const float** dst) {
        if (rc == BSDFD_OK) rc = upload(h, v, dst);
    };
    up(phi_v, &d.phi_i);
    up(theta_v, &d.theta_i);
    up(as_f32(*ndf), &d.ndf.data);
    up(as_f32(*sigma), &d.sigma.data);
    up(vdata, &d.vndf.data);
    up(vcond, &d.vndf_cond);
    up(vmarg, &d.vndf_marg);
    up(as_f32(*rgb), &d.rgb.data);
    d.lum = Table{nullptr, 0, 0};
    d.lum_cond = d.lum_marg = nullptr;
    if (lum) {
        up(ldata, &d.lum.data);
        up(lcond, &d.lum_cond);
        up(lmarg, &d.lum_marg);
        d.lum.h = (int)lum->shape[2]; d.lum.w = (int)lum->shape[3];
    }
    d.ndf.h = (int)ndf->shape[0]; d.ndf.w = (int)ndf->shape[1];
    d.sigma.h = (int)sigma->shape[0]; d.sigma.w = (int)sigma->shape[1];
    d.vndf.h = vh; d.vndf.w = vw;
    d.rgb.h = (int)rgb->shape[3]; d.rgb.w = (int)rgb->shape[4];
    if (rc != BSDFD_OK) {
        for (void* p : h->allocs) (void)hipFree(p);
        delete h;
        return rc;
    }
    *out = h;
    return BSDFD_OK;
}

void bsdfd_measured_destroy(bsdfd_measured_handle h) {
    if (!h) return;
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
}

int bsdfd_measured_get_info(bsdfd_measured_handle h, int32_t* n_phi, int32_t* n_theta, int32_t* isotropic,
                            int32_t* jacobian, int32_t* reduction) {
    if (!h) return bsdfd_fail_(BSDFD_EINVAL, "null handle");
    if (n_phi) *n_phi = h->dev.n_phi;
    if (n_theta) *n_theta = h->dev.n_theta;
    if (isotropic) *isotropic = h->dev.isotropic;
    if (jacobian) *jacobian = h->dev.jacobian;
    if (reduction) *reduction = h->dev.reduction;
    return BSDFD_OK;
}

int bsdfd_measured_eval(bsdfd_measured_handle h, const float* wi, const float* wo, int64_t n, const float* tint,
                        float* rgb_out, void* stream) {
    return measured_launch(h, n, wi && wo && rgb_out, measured_eval_kernel, stream, wi, wo, (long long)n, TintArg{tint},
                           rgb_out);
}

int bsdfd_measured_has_luminance(bsdfd_measured_handle h, int32_t* has_luminance) {
    if (!h || !has_luminance) return bsdfd_fail_(BSDFD_EINVAL, "null argument");
    *has_luminance = h->dev.lum.data ? 1 : 0;
    return BSDFD_OK;
}

int bsdfd_measured_sample(bsdfd_measured_handle h, const float* wi, const float* u, const unsigned char* active, int64_t n,
                          const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* stream) {
    return measured_launch(h, n, wi && u && wo_out && pdf_out, measured_sample_kernel, stream, wi, u, active, (long long)n,
                           TintArg{tint}, wo_out, pdf_out, weight_out);
}

int bsdfd_measured_pdf(bsdfd_measured_handle h, const float* wi, const float* wo, const unsigned char* active, int64_t n,
                       float* pdf_out, void* stream) {
    return measured_launch(h, n, wi && wo && pdf_out, measured_pdf_kernel, stream, wi, wo, active, (long long)n, pdf_out);
}

int bsdfd_measured_sample_weight(bsdfd_measured_handle h, const float* wi, const float* wo, const float* pdf_sa,
                                 const unsigned char* active, int64_t n, const float* tint, float firefly_threshold,
                                 float* weight_out, float* pdf_out, void* stream) {
    return measured_launch(h, n, wi && wo && pdf_sa && weight_out && pdf_out, measured_weight_kernel, stream, wi, wo, pdf_sa,
                           active, (long long)n, TintArg{tint}, firefly_threshold, weight_out, pdf_out);
}

}  // extern "C"
