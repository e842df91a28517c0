// host.hip — the host side of the flow sampler: the handle (bsdfd_ctx), the launch routine run() / run_multi(), the flow entry points of
// include/bsdfd.h, the profiling ring, and the error plumbing every translation unit of libbsdfd.so links against (common.h).  No kernel:
// the two families (bsdfd.hip, flow32.hip) describe theirs through flow_kernels.h; nothing here enters the kernel-source fingerprint.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "flow_dev.h"
#include "flow_kernels.h"

#pragma clang diagnostic ignored "-Wc++20-designator"   // run()'s argument record is filled by field name

namespace {

thread_local std::string g_err;

inline int fail(int code, const std::string& msg) { return bsdfd_fail_(code, msg); }

}  // namespace

int bsdfd_fail_(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

struct bsdfd_ctx {
    int domain, width, n_hidden, precision, state_dim, in_dim;
    int device, num_cu;
    // launch slots: 0 .. 2 = the (no-Jacobian, Jacobian, Jacobian + fused sample/pdf) kernels of every call form; KF_RESIDENT + op =
    // the register-resident fast path of the plain plugin sample / pdf call (flow32.hip, flow_kernel32<.., ROP>; k[].fn = nullptr
    // where the net has none), chosen per call by run()
    static constexpr int KF_RESIDENT = 3, NKF = 5;
    FlowKernel k[NKF];   // slot m's kernel: 32-query tiles (flow32.hip) where bsdfd_create chose them, else 16 (bsdfd.hip)
    int per_cu[NKF];     // resident blocks per CU
    ImgLayout L;
    char* d_img;
    char* d_img32;   // the 32-query-tile kernels' weight image, if any slot runs them
    int ctx_v4_32;   // f32x4 records per 32-query tile of the per-query context (bsdfd_tile32_context_v4)
    const char* img_of[NKF];   // the image slot m's kernel reads, and its size (<= k[m].lds_bytes)
    int img_bytes[NKF];
    // profiling: a ring of HIP event pairs recorded on the launch stream around every launch.  Everything above this line is immutable
    // after create; the profiling state below is guarded by `prof_mu`, so the handle stays re-entrant across host threads / streams
    // with profiling on (launches that are being timed serialise on the mutex for the two hipEventRecord calls only).
    static constexpr int RING = 64;
    std::mutex prof_mu;
    bool profiling;
    hipEvent_t ev0[RING], ev1[RING];
    bool pending[RING];
    long long n_rec;       // launches recorded since profiling was enabled
    long long n_done;      // launches harvested
    double total_ms;
    float last_ms;
    int op_of[RING];       // which operation a recorded launch ran (OP_*, + BSDFD_OP_RESIDENT on the fast path): the per-operation
    long long n_op[8];     // totals of bsdfd_profile_read_op ([op]: every launch of the operation, [BSDFD_OP_RESIDENT + op]: the
    double ms_op[8];       // fast-path launches among them)
    unsigned long long* d_clk;  // CLK_SLOTS x 8 cumulative counters (KParams::clk), zeroed by bsdfd_set_profiling — NOT per launch: a memset in
                                // front of every profiled launch would put an inter-kernel boundary inside the event bracket
    double wall_khz;            // rate of the wall clock (hipDeviceAttributeWallClockRate)
};

namespace {

// queries per wave tile when the caller leaves bsdfd_desc.tile at 0 and $BSDFD_TILE is unset: the 32-query-tile kernels where they
// exist (round 5, within-run A/B on one box: kernel time 0.925-0.94 of the 16-query kernels' on disk T = 8 / T = 4 and spherical
// T = 8, sample and pdf, and 0.93 on the fused sample+pdf launches; profiles/r05_ab/)
constexpr int kDefaultTile = 32;
// extra dynamic LDS per workgroup: 0 in the product; a tools build (tools/tuning_knobs.h) reads $BSDFD_LDS_PAD to lower the
// number of resident workgroups per CU (occupancy sweeps of the same binary)
#ifdef BSDFD_TOOLS_LDS_PAD
inline size_t lds_pad() { BSDFD_TOOLS_LDS_PAD }
#else
constexpr size_t lds_pad() { return 0; }
#endif

hipError_t harvest(bsdfd_handle h, int slot) {
    hipError_t e = hipEventSynchronize(h->ev1[slot]);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, h->ev0[slot], h->ev1[slot]);
    if (e != hipSuccess) return e;
    h->pending[slot] = false;
    h->total_ms += ms;
    h->last_ms = ms;
    h->n_done++;
    h->n_op[h->op_of[slot] & 3]++;
    h->ms_op[h->op_of[slot] & 3] += ms;
    if (h->op_of[slot] & BSDFD_OP_RESIDENT) {
        h->n_op[h->op_of[slot] & 7]++;
        h->ms_op[h->op_of[slot] & 7] += ms;
    }
    return hipSuccess;
}

#ifndef BSDFD_T32_RESIDENT_MIN_T
#define BSDFD_T32_RESIDENT_MIN_T 8   // least T at which run() takes the register-resident fast path (A/B builds: 0 = never)
#endif

struct SegHost { bsdfd_handle h; long long q_begin, q_end; };   // one bucket of a segmented launch

struct CtxArg {  // optional arguments of a call (bsdfd_opts) and the bucket numbering base of segmented launches
    float* out = nullptr;
    const float* in = nullptr;
    int seg_base = 0;
    const long long *rng_index = nullptr, *row_index = nullptr;
    CtxArg() = default;
    explicit CtxArg(const bsdfd_opts* o) {
        if (!o) return;
        out = static_cast<float*>(o->ctx_out);
        in = static_cast<const float*>(o->ctx_in);
        rng_index = reinterpret_cast<const long long*>(o->rng_index);
        row_index = reinterpret_cast<const long long*>(o->row_index);
    }
};

struct Call {  // what an entry point asks of run() / run_multi(): filled by field name, in this order; what it leaves out is absent
    int op, io;
    const float *in_a, *in_b = nullptr, *in_c = nullptr;   // as in KParams: omega_i | wi, x0 | omega_o | wo, wl
    uint64_t seed = 0, offset = 0;
    int64_t N = 0;   // (run_multi: the last segment's end)
    int T;
    float *out_x = nullptr, *out_pdf = nullptr, *out_pdf2 = nullptr;
    void* stream;
    CtxArg ctx = CtxArg();
};

// plugin `variant` -> the kernels' io code; -1 with the error recorded: run() / run_multi() return BSDFD_EINVAL on it before any other check
int plugin_io(int32_t variant) {
    if (variant == BSDFD_PLUGIN_MEASURED) return IO_PLUGIN;
    if (variant == BSDFD_PLUGIN_FULLSPHERE) return IO_PLUGIN_FULLSPHERE;
    return fail(-1, "unknown plugin variant");
}

int run(bsdfd_handle h, const Call& c, const std::vector<SegHost>* segs = nullptr) {
    const auto& [op, io, in_a, in_b, in_c, seed, offset, N, T, out_x, out_pdf, out_pdf2, stream, ctx] = c;
    if (io < 0) return BSDFD_EINVAL;
    if (!h) return fail(BSDFD_EINVAL, "null handle");
    if (N < 0) return fail(BSDFD_EINVAL, "N must be >= 0");
    if (T < 1 || T > 4096) return fail(BSDFD_EINVAL, "T must be in [1, 4096]");
    if (N == 0) return BSDFD_OK;
    if (!in_a) return fail(BSDFD_EINVAL, "null input pointer");
    if (op == OP_PDF && !in_b) return fail(BSDFD_EINVAL, "pdf needs the outgoing directions");
    if (op == OP_SAMPLE_PDF && (io == IO_OPERATOR || !in_c || !out_pdf2))
        return fail(BSDFD_EINVAL, "sample_pdf is a plugin-level call and needs wl and a second pdf output");
    if (op == OP_SAMPLES_ONLY && !in_b) return fail(BSDFD_EINVAL, "flow_samples_only needs x0");
    if (op != OP_PDF && !out_x) return fail(BSDFD_EINVAL, "null output pointer");
    if (op != OP_SAMPLES_ONLY && !out_pdf) return fail(BSDFD_EINVAL, "null pdf output pointer");
    if (io == IO_PLUGIN_FULLSPHERE && h->domain != BSDFD_DOMAIN_SPHERICAL)
        return fail(BSDFD_EINVAL, "the full-sphere plugin variant needs a spherical-domain handle");
    if ((ctx.out || ctx.in) && op != OP_SAMPLE && op != OP_PDF)
        return fail(BSDFD_EINVAL, "a per-query context is written / read by the sample and pdf calls only");
    if (ctx.out && ctx.in)
        return fail(BSDFD_EINVAL, "a call either writes a per-query context (ctx_out) or reads one (ctx_in), not both");
    if (ctx.rng_index && (op == OP_PDF || op == OP_SAMPLES_ONLY))
        return fail(BSDFD_EINVAL, "rng_index applies to calls that draw base samples (sample, sample_pdf)");
    if (ctx.row_index && io == IO_OPERATOR)
        return fail(BSDFD_EINVAL, "row_index applies to the plugin-level calls (sample, pdf, sample_pdf)");
    if ((reinterpret_cast<uintptr_t>(ctx.out) | reinterpret_cast<uintptr_t>(ctx.in)) & 15u)
        return fail(BSDFD_EINVAL, "the per-query context buffer must be 16-byte aligned");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return fail(BSDFD_EINVAL, "handle was created on device " + std::to_string(h->device) +
                                                        " but device " + std::to_string(dev) + " is current");
    KParams kp;
    kp.L = h->L;
    kp.in_a = in_a; kp.in_b = in_b; kp.out_x = out_x; kp.out_pdf = out_pdf;
    kp.in_c = in_c; kp.out_pdf2 = out_pdf2;
    kp.N = N; kp.T = T; kp.n_hidden = h->n_hidden; kp.op = op; kp.io = io; kp.seed = seed; kp.offset = offset;
    kp.nseg = 0;
    kp.chunk_log2 = 3;
    kp.ctx_out = ctx.out; kp.ctx_in = ctx.in; kp.seg_base = ctx.seg_base; kp.rng_index = ctx.rng_index;
    kp.row_index = ctx.row_index;
    kp.clk = nullptr;

    const int mode = op == OP_SAMPLES_ONLY ? 0 : (op == OP_SAMPLE_PDF ? 2 : 1);
    // flow_kernel32w (the 64 x 6 f16 samples-only kernel, mode 0) reads neither segments, nor a context, nor rng_index / row_index:
    // all four are rejected for OP_SAMPLES_ONLY above and below — keep it that way if that validation is ever relaxed
    if (mode == 0 && (segs || ctx.out || ctx.in || ctx.rng_index || ctx.row_index))
        return fail(BSDFD_EINVAL, "flow_samples_only takes no segments, per-query context, rng_index or row_index");
    // The register-resident fast path (flow32.hip) serves exactly one call form: a single-material plugin sample / pdf of the
    // measured variant with nothing optional — no context, no index arrays (an `active` mask arrives as a row_index), no injected
    // base point — at T a power of two >= BSDFD_T32_RESIDENT_MIN_T, the step counts it is tested bit for bit against the general
    // kernel at (measurements: DESIGN.md §4.3, profiles/r07_ab/disk_resident_path.txt).  Everything else: the general kernel.
    int kf = mode;
    if (BSDFD_T32_RESIDENT_MIN_T > 0 && mode == 1 && (op == OP_SAMPLE || op == OP_PDF) && h->k[bsdfd_ctx::KF_RESIDENT + op].fn &&
        io == IO_PLUGIN && !segs && !ctx.out && !ctx.in && !ctx.rng_index && !ctx.row_index && (op == OP_PDF || !in_b) &&
        T >= BSDFD_T32_RESIDENT_MIN_T && (T & (T - 1)) == 0)
        kf = bsdfd_ctx::KF_RESIDENT + op;
    const FlowKernel& k = h->k[kf];
    const int threads = k.threads;
    const int waves = threads / 64;
    // grid: 4 rounds of the resident capacity (blocks per CU from the occupancy query of the
    // instantiated kernel: VGPR- or LDS-limited); block-granular dynamic balancing measured ~4 %
    // faster than an exactly-resident persistent grid (tools/tscan.py sweep)
    kp.img = h->img_of[kf];
    kp.L.total = h->img_bytes[kf];
    const int tile = k.tile;
    int per_cu = h->per_cu[kf];
    if (per_cu < 1) per_cu = 1;
    // grid-shape overrides of the tools builds (tools/tuning_knobs.h, force-included by tools/ab_build.sh for tools/tscan.py
    // and tools/nscan.py); the product build has none
#ifdef BSDFD_TOOLS_KNOBS
    BSDFD_TOOLS_KNOBS(per_cu)
#else
    constexpr int cl_override = -1;
#endif
    const long long cap = (long long)h->num_cu * per_cu * 4;
    // tiles per wave and chunk: 8 when that still leaves >= `min_chunks` workgroup-chunks, else fewer
    auto pick_cl = [&](long long ntiles, long long min_chunks) {
        if (cl_override >= 0 && cl_override <= 3) return cl_override;
        int cl = 3;
        while (cl > 0 && ntiles / ((long long)waves << cl) < min_chunks) --cl;
        return cl;
    };
    long long nblocks;
    if (!segs) {
        const long long ntiles = (N + tile - 1) / tile;
        kp.chunk_log2 = pick_cl(ntiles, 8LL * h->num_cu);
        const long long want = (ntiles + ((long long)waves << kp.chunk_log2) - 1) / ((long long)waves << kp.chunk_log2);
        nblocks = want < cap ? want : cap;
    } else {
        // workgroups are dealt to the buckets in proportion to their sizes (at least one each)
        long long total_want = 0;
        std::vector<long long> want(segs->size());
        for (size_t i = 0; i < segs->size(); ++i) {
            const long long nt = ((*segs)[i].q_end - (*segs)[i].q_begin + tile - 1) / tile;
            want[i] = (nt + waves - 1) / waves;
            total_want += want[i];
        }
        const double scale = total_want > cap ? (double)cap / (double)total_want : 1.0;
        int b = 0;
        for (size_t i = 0; i < segs->size(); ++i) {
            long long nb = (long long)(want[i] * scale);
            if (nb < 1) nb = 1;
            if (nb > want[i]) nb = want[i];
            KParams::Seg& sg = kp.seg[kp.nseg++];
            sg.img = (*segs)[i].h->img_of[mode];
            sg.q_begin = (*segs)[i].q_begin;
            sg.q_end = (*segs)[i].q_end;
            sg.blk_begin = b;
            b += (int)nb;
            sg.blk_end = b;
            sg.chunk_log2 = pick_cl(((*segs)[i].q_end - (*segs)[i].q_begin + tile - 1) / tile, 8LL * nb);
            sg.pad = 0;
        }
        nblocks = b;
    }
    dim3 grid((unsigned)nblocks), block(threads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    void* args[] = {const_cast<KParams*>(&kp)};
    std::unique_lock<std::mutex> prof_lock(h->prof_mu, std::defer_lock);
    int slot = -1;
    if (h->profiling) {  // (a racy read is fine: the flag is re-read under the lock)
        prof_lock.lock();
        if (h->profiling) {
            slot = (int)(h->n_rec % bsdfd_ctx::RING);
            if (h->pending[slot]) HIP_TRY(harvest(h, slot));
            kp.clk = h->d_clk;
            HIP_TRY(hipEventRecord(h->ev0[slot], s));
        }
    }
    hipError_t e = hipLaunchKernel(k.fn, grid, block, args, (size_t)k.lds_bytes + lds_pad(), s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(BSDFD_EHIP, std::string("kernel launch: ") + hipGetErrorString(e));
    if (slot >= 0) {
        HIP_TRY(hipEventRecord(h->ev1[slot], s));
        h->pending[slot] = true;
        h->op_of[slot] = op | (kf >= bsdfd_ctx::KF_RESIDENT ? BSDFD_OP_RESIDENT : 0);
        h->n_rec++;
    }
    return BSDFD_OK;
}

// multi-material launch: all handles must share the kernel signature (domain, width, depth, precision)
int run_multi(const bsdfd_handle* hs, int n, const int64_t* seg_end, Call c) {
    if (c.io < 0) return BSDFD_EINVAL;
    if (!hs || !seg_end || n < 1) return fail(BSDFD_EINVAL, "need at least one handle and its segment end");
    for (int i = 0; i < n; ++i) {
        if (!hs[i]) return fail(BSDFD_EINVAL, "null handle in the table");
        if (hs[i]->domain != hs[0]->domain || hs[i]->width != hs[0]->width || hs[i]->n_hidden != hs[0]->n_hidden ||
            hs[i]->precision != hs[0]->precision || hs[i]->device != hs[0]->device || hs[i]->k[0].tile != hs[0]->k[0].tile ||
            hs[i]->k[1].tile != hs[0]->k[1].tile || hs[i]->k[2].tile != hs[0]->k[2].tile)
            return fail(BSDFD_EINVAL, "handles of one multi-material launch must share domain, width, depth, "
                                      "precision, tile and device");
        if (seg_end[i] < (i ? seg_end[i - 1] : 0)) return fail(BSDFD_EINVAL, "segment ends must be non-decreasing");
    }
    c.N = seg_end[n - 1];
    if (c.N == 0) return BSDFD_OK;
    // chunks of MAX_SEG non-empty buckets per launch
    std::vector<SegHost> segs;
    int rc = BSDFD_OK;
    for (int i = 0; i < n && rc == BSDFD_OK; ++i) {
        const long long b = i ? seg_end[i - 1] : 0, e = seg_end[i];
        if (e > b) segs.push_back({hs[i], b, e});
        if ((int)segs.size() == MAX_SEG || (i == n - 1 && !segs.empty())) {
            rc = run(segs[0].h, c, &segs);
            c.ctx.seg_base += (int)segs.size();
            segs.clear();
        }
    }
    return rc;
}

}  // namespace

extern "C" {

int bsdfd_create(const bsdfd_desc* d, bsdfd_handle* out) {
    if (!d || !out) return fail(BSDFD_EINVAL, "null argument");
    *out = nullptr;
    if (d->domain != BSDFD_DOMAIN_DISK && d->domain != BSDFD_DOMAIN_SPHERICAL)
        return fail(BSDFD_EINVAL, "domain must be BSDFD_DOMAIN_DISK or BSDFD_DOMAIN_SPHERICAL");
    if (d->width != 32 && d->width != 64) return fail(BSDFD_EINVAL, "width must be 32 or 64");
    if (d->n_hidden < 1 || d->n_hidden > 16) return fail(BSDFD_EINVAL, "n_hidden must be in [1, 16]");
    if (d->pe_bands != PE_BANDS) return fail(BSDFD_EINVAL, "pe_bands must be 5 (the reference's velocity nets)");
    if (d->base_pe_bands != BASE_PE_BANDS || d->base_hidden != BASE_HIDDEN)
        return fail(BSDFD_EINVAL, "base net must be PE_3 -> 16 -> 4 (the reference's pretrain nets)");
    if (!d->w_in || !d->w_out || !d->base_w1 || !d->base_b1 || !d->base_w2 || !d->base_b2 ||
        (d->n_hidden > 1 && !d->w_hidden))
        return fail(BSDFD_EINVAL, "null weight pointer");
    if (d->tile != 0 && d->tile != 16 && d->tile != 32) return fail(BSDFD_EINVAL, "tile must be 0 (default), 16 or 32");
    int prec = d->precision == BSDFD_PREC_DEFAULT ? BSDFD_PREC_SPLIT3 : d->precision;
    if (prec != BSDFD_PREC_F32 && prec != BSDFD_PREC_SPLIT3 && prec != BSDFD_PREC_F16)
        return fail(BSDFD_EINVAL, "unknown precision");
    if (d->tile == 32 && !bsdfd_tile32_supported(*d, prec))
        return fail(BSDFD_EINVAL, "tile = 32 was asked for explicitly, but no 32-query-tile kernel exists for this net and precision "
                                  "(they serve the disk 32x3 / spherical 32x4 nets in split3 and f16 and the spherical 64x6 net in f16); "
                                  "pass 0 for the library's default or 16");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BSDFD_EINVAL, std::string("bsdfd is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName);
    bsdfd_ctx* h = new bsdfd_ctx();
    h->domain = d->domain; h->width = d->width; h->n_hidden = d->n_hidden; h->precision = prec;
    h->state_dim = d->domain == BSDFD_DOMAIN_DISK ? 2 : 3;
    h->in_dim = h->state_dim + 1 + 2 + 4 * PE_BANDS;
    h->device = dev; h->num_cu = prop.multiProcessorCount;
    h->profiling = false; h->d_img = nullptr; h->d_img32 = nullptr; h->d_clk = nullptr;
    h->n_rec = h->n_done = 0; h->total_ms = 0.0; h->last_ms = -1.0f;
    for (int i = 0; i < 8; ++i) { h->n_op[i] = 0; h->ms_op[i] = 0.0; }
    int khz = 0;
    h->wall_khz = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess ? (double)khz : 0.0;
    for (int i = 0; i < bsdfd_ctx::RING; ++i) { h->pending[i] = false; h->ev0[i] = nullptr; h->ev1[i] = nullptr; }
    std::vector<char> img = bsdfd_build_image16(*d, prec, h->L);
    if (h->L.total < 0) {
        delete h;
        return fail(BSDFD_EINVAL, "internal error: weight-image layout differs from the kernel's compile-time fragment offsets");
    }
    if (h->L.total > 160 * 1024 - 512) {
        delete h;
        return fail(BSDFD_EINVAL, "weight image does not fit the 160 KiB LDS; use fewer layers or BSDFD_PREC_F16");
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_img), img.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_img, img.data(), img.size(), hipMemcpyHostToDevice);
    // Tile: desc->tile alone decides (0 = the library's default; the library reads no environment variable — the Python hosts map
    // $BSDFD_TILE onto the field for A/B runs of one build).  The 32-query-tile kernels exist for the reference's two plugin nets in
    // split3 (every call) and for the samples-only call of those nets and of the 64 x 6 teacher in f16; everything else runs
    // 16-query tiles — silently under the default, with an error when 32 was asked for explicitly and cannot be honoured at all.
    const int want_tile = d->tile == 0 ? kDefaultTile : d->tile;
    const bool t32 = want_tile == 32 && bsdfd_tile32_supported(*d, prec);
    h->ctx_v4_32 = bsdfd_tile32_context_v4(*d, prec);
    std::vector<char> img32;
    if (t32 && e == hipSuccess) {
        img32 = bsdfd_build_image32(*d, prec);
        e = hipMalloc(reinterpret_cast<void**>(&h->d_img32), img32.size());
        if (e == hipSuccess) e = hipMemcpy(h->d_img32, img32.data(), img32.size(), hipMemcpyHostToDevice);
    }
    // every slot from one record: the 32-query kernel if it exists and (32 was asked for explicitly or it is not opt-in), else the
    // 16-query kernel; the fast path rides on slot 1's 32-query tiling (its own kernel and occupancy): its slots exist only then
    for (int m = 0; m < bsdfd_ctx::NKF; ++m) {
        const bool resident = m >= bsdfd_ctx::KF_RESIDENT;
        FlowKernel k32 = {};   // (fn == nullptr)
        if (resident && h->k[1].tile == 32) k32 = bsdfd_kernel32_resident(*d, prec, m - bsdfd_ctx::KF_RESIDENT);
        if (!resident && t32) k32 = bsdfd_kernel32(*d, prec, m);
        const bool use32 = k32.fn && (d->tile == 32 || !k32.opt_in);
        h->k[m] = use32 || resident ? k32 : bsdfd_kernel16(*d, prec, m, h->L);
        h->img_of[m] = use32 ? h->d_img32 : h->d_img;
        h->img_bytes[m] = use32 ? (int)img32.size() : h->L.total;
        h->per_cu[m] = 0;
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_clk), (size_t)CLK_SLOTS * 8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->d_clk, 0, (size_t)CLK_SLOTS * 8 * sizeof(unsigned long long));
    for (int i = 0; i < bsdfd_ctx::RING && e == hipSuccess; ++i) {
        e = hipEventCreate(&h->ev0[i]);
        if (e == hipSuccess) e = hipEventCreate(&h->ev1[i]);
    }
    for (int m = 0; m < bsdfd_ctx::NKF && e == hipSuccess; ++m) {
        const FlowKernel& k = h->k[m];
        if (!k.fn) continue;
        // dynamic LDS above the default cap needs the attribute (per function and device)
        e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes + (int)lds_pad());
        int nb = 0;
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, k.threads, (size_t)k.lds_bytes + lds_pad());
        h->per_cu[m] = nb;
    }
    if (e != hipSuccess) {
        bsdfd_destroy(h);   // (frees what exists of a half-built handle)
        return fail(BSDFD_EHIP, std::string("create: ") + hipGetErrorString(e));
    }
    *out = h;
    return BSDFD_OK;
}

int bsdfd_create_from_file(const char* path, int32_t precision, bsdfd_handle* out) {
    if (!path || !out) return fail(BSDFD_EINVAL, "null argument");
    *out = nullptr;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(BSDFD_EIO, std::string("cannot open ") + path);
    std::vector<char> raw;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + n);
    std::fclose(f);
    if (raw.size() < 104 || std::memcmp(raw.data(), "BSDFWT01", 8) != 0)
        return fail(BSDFD_EIO, std::string(path) + ": not a BSDFWT01 weight file");
    int32_t hdr[8];
    std::memcpy(hdr, raw.data() + 72, sizeof hdr);
    bsdfd_desc d;
    std::memset(&d, 0, sizeof d);
    d.domain = hdr[0]; d.width = hdr[1]; d.n_hidden = hdr[2]; d.pe_bands = hdr[3];
    d.base_hidden = hdr[4]; d.base_pe_bands = hdr[5]; d.precision = precision;
    if (d.width <= 0 || d.width > 4096 || d.n_hidden < 1 || d.n_hidden > 64 || d.pe_bands < 0 || d.pe_bands > 64 ||
        d.base_hidden <= 0 || d.base_hidden > 4096 || d.base_pe_bands < 0 || d.base_pe_bands > 64)
        return fail(BSDFD_EIO, std::string(path) + ": implausible header");
    const int sd = d.domain == BSDFD_DOMAIN_DISK ? 2 : 3;
    if (hdr[6] != sd) return fail(BSDFD_EIO, std::string(path) + ": state_dim inconsistent with domain");
    const size_t in_dim = sd + 1 + 2 + 4 * d.pe_bands, bin = 2 + 4 * d.base_pe_bands;
    const size_t cnt[7] = {(size_t)d.width * in_dim, (size_t)(d.n_hidden - 1) * d.width * d.width, (size_t)2 * d.width,
                           (size_t)d.base_hidden * bin, (size_t)d.base_hidden, (size_t)4 * d.base_hidden, 4};
    size_t total = 0;
    for (size_t c : cnt) total += c;
    if (raw.size() != 104 + 4 * total) return fail(BSDFD_EIO, std::string(path) + ": payload size mismatch");
    const float* p = reinterpret_cast<const float*>(raw.data() + 104);
    d.w_in = p; p += cnt[0];
    d.w_hidden = p; p += cnt[1];
    d.w_out = p; p += cnt[2];
    d.base_w1 = p; p += cnt[3];
    d.base_b1 = p; p += cnt[4];
    d.base_w2 = p; p += cnt[5];
    d.base_b2 = p;
    return bsdfd_create(&d, out);
}

void bsdfd_destroy(bsdfd_handle h) {
    if (!h) return;
    if (h->d_img) (void)hipFree(h->d_img);
    if (h->d_img32) (void)hipFree(h->d_img32);
    if (h->d_clk) (void)hipFree(h->d_clk);
    for (int i = 0; i < bsdfd_ctx::RING; ++i) {
        if (h->ev0[i]) (void)hipEventDestroy(h->ev0[i]);
        if (h->ev1[i]) (void)hipEventDestroy(h->ev1[i]);
    }
    delete h;
}

int bsdfd_get_info(bsdfd_handle h, int32_t* domain, int32_t* width, int32_t* n_hidden, int32_t* precision) {
    if (!h) return fail(BSDFD_EINVAL, "null handle");
    if (domain) *domain = h->domain;
    if (width) *width = h->width;
    if (n_hidden) *n_hidden = h->n_hidden;
    if (precision) *precision = h->precision;
    return BSDFD_OK;
}

int bsdfd_get_tile(bsdfd_handle h, int32_t op, int32_t* tile) {
    if (!h || !tile) return fail(BSDFD_EINVAL, "null argument");
    if (op < 0 || op > 3) return fail(BSDFD_EINVAL, "op must be one of BSDFD_OP_SAMPLE, _PDF, _SAMPLES_ONLY, _SAMPLE_PDF");
    *tile = h->k[op == OP_SAMPLES_ONLY ? 0 : (op == OP_SAMPLE_PDF ? 2 : 1)].tile;
    return BSDFD_OK;
}

int64_t bsdfd_flops_per_query(bsdfd_handle h, int32_t T) {
    if (!h) return -1;
    const int64_t w = h->width, nh = h->n_hidden;
    const int64_t fwd = (int64_t)h->in_dim * w + (nh - 1) * w * w + 2 * w;
    int64_t tang = 2 * ((nh - 1) * w * w + 2 * w);
    if (h->state_dim == 3) tang += 2 * w;
    const int64_t base = 2 * ((2 + 4 * BASE_PE_BANDS) * BASE_HIDDEN + 4 * BASE_HIDDEN);
    return (int64_t)T * 2 * (fwd + tang) + base;
}

int bsdfd_network_sampling(bsdfd_handle h, const float* omega_i, const float* x0, uint64_t seed, uint64_t offset,
                           int64_t N, int32_t T, float* x_out, float* pdf_out, void* stream) {
    return run(h, {.op = OP_SAMPLE, .io = IO_OPERATOR, .in_a = omega_i, .in_b = x0, .seed = seed, .offset = offset, .N = N, .T = T,
                   .out_x = x_out, .out_pdf = pdf_out, .stream = stream});
}

int bsdfd_network_pdf(bsdfd_handle h, const float* omega_o, const float* omega_i, int64_t N, int32_t T,
                      float* pdf_out, void* stream) {
    return run(h, {.op = OP_PDF, .io = IO_OPERATOR, .in_a = omega_i, .in_b = omega_o, .N = N, .T = T, .out_pdf = pdf_out, .stream = stream});
}

int bsdfd_flow_samples_only(bsdfd_handle h, const float* omega_i, const float* x0, int64_t N, int32_t T,
                            float* x_out, void* stream) {
    return run(h, {.op = OP_SAMPLES_ONLY, .io = IO_OPERATOR, .in_a = omega_i, .in_b = x0, .N = N, .T = T, .out_x = x_out, .stream = stream});
}

int64_t bsdfd_context_bytes(bsdfd_handle h, int64_t N, int32_t n_segments) {
    if (!h || N < 0 || n_segments < 1) return -1;
    // per 16-query tile: cacc[NM] per lane + bo per query, 16 B each; the 32-query-tile kernels store (4 x 64 + 32) x 16 B per tile
    if (h->k[1].tile == 32) return ((N + 31) / 32 + n_segments) * (int64_t)(h->ctx_v4_32 * 16);
    const int64_t per_tile = ((int64_t)(h->width / 16) * 64 + 16) * 16;
    return ((N + 15) / 16 + n_segments) * per_tile;
}

// The plugin-level calls.  A form without `opts` is its _ex form with none (CtxArg(nullptr) is the empty CtxArg).
int bsdfd_plugin_sample_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, uint64_t seed, uint64_t offset,
                           int64_t N, int32_t T, float* wo, float* pdf_sa, const bsdfd_opts* opts, void* stream) {
    return run(h, {.op = OP_SAMPLE, .io = plugin_io(variant), .in_a = wi, .in_b = x0, .seed = seed, .offset = offset, .N = N, .T = T,
                   .out_x = wo, .out_pdf = pdf_sa, .stream = stream, .ctx = CtxArg(opts)});
}

int bsdfd_plugin_pdf_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* wo, int64_t N, int32_t T,
                        float* pdf_sa, const bsdfd_opts* opts, void* stream) {
    return run(h, {.op = OP_PDF, .io = plugin_io(variant), .in_a = wi, .in_b = wo, .N = N, .T = T, .out_pdf = pdf_sa, .stream = stream,
                   .ctx = CtxArg(opts)});
}

int bsdfd_plugin_sample_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                                 const float* wi, const float* x0, uint64_t seed, uint64_t offset, int32_t T, float* wo,
                                 float* pdf_sa, const bsdfd_opts* opts, void* stream) {
    return run_multi(handles, n_handles, seg_end, {.op = OP_SAMPLE, .io = plugin_io(variant), .in_a = wi, .in_b = x0, .seed = seed,
                     .offset = offset, .T = T, .out_x = wo, .out_pdf = pdf_sa, .stream = stream, .ctx = CtxArg(opts)});
}

int bsdfd_plugin_pdf_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                              const float* wi, const float* wo, int32_t T, float* pdf_sa, const bsdfd_opts* opts, void* stream) {
    return run_multi(handles, n_handles, seg_end, {.op = OP_PDF, .io = plugin_io(variant), .in_a = wi, .in_b = wo, .T = T,
                     .out_pdf = pdf_sa, .stream = stream, .ctx = CtxArg(opts)});
}

int bsdfd_plugin_sample_pdf_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                                     const float* wi, const float* x0, const float* wl, uint64_t seed, uint64_t offset,
                                     int32_t T, float* wo, float* pdf_wo, float* pdf_wl, const bsdfd_opts* opts, void* stream) {
    const int io = plugin_io(variant);
    if (io >= 0 && opts && (opts->ctx_in || opts->ctx_out))   // (an unknown variant is reported first: run_multi)
        return fail(BSDFD_EINVAL, "the fused sample+pdf call shares the prologue in registers; it takes no per-query context");
    return run_multi(handles, n_handles, seg_end, {.op = OP_SAMPLE_PDF, .io = io, .in_a = wi, .in_b = x0, .in_c = wl, .seed = seed,
                     .offset = offset, .T = T, .out_x = wo, .out_pdf = pdf_wo, .out_pdf2 = pdf_wl, .stream = stream, .ctx = CtxArg(opts)});
}

int bsdfd_plugin_sample(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, uint64_t seed,
                        uint64_t offset, int64_t N, int32_t T, float* wo, float* pdf_sa, void* stream) {
    return bsdfd_plugin_sample_ex(h, variant, wi, x0, seed, offset, N, T, wo, pdf_sa, nullptr, stream);
}

int bsdfd_plugin_pdf(bsdfd_handle h, int32_t variant, const float* wi, const float* wo, int64_t N, int32_t T,
                     float* pdf_sa, void* stream) {
    return bsdfd_plugin_pdf_ex(h, variant, wi, wo, N, T, pdf_sa, nullptr, stream);
}

int bsdfd_plugin_sample_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                              const float* wi, const float* x0, uint64_t seed, uint64_t offset, int32_t T, float* wo, float* pdf_sa, void* stream) {
    return bsdfd_plugin_sample_multi_ex(handles, n_handles, seg_end, variant, wi, x0, seed, offset, T, wo, pdf_sa, nullptr, stream);
}

int bsdfd_plugin_pdf_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                           const float* wi, const float* wo, int32_t T, float* pdf_sa, void* stream) {
    return bsdfd_plugin_pdf_multi_ex(handles, n_handles, seg_end, variant, wi, wo, T, pdf_sa, nullptr, stream);
}

int bsdfd_plugin_sample_pdf_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end, int32_t variant,
                                  const float* wi, const float* x0, const float* wl, uint64_t seed, uint64_t offset,
                                  int32_t T, float* wo, float* pdf_wo, float* pdf_wl, void* stream) {
    return bsdfd_plugin_sample_pdf_multi_ex(handles, n_handles, seg_end, variant, wi, x0, wl, seed, offset, T, wo, pdf_wo, pdf_wl, nullptr, stream);
}

// the single-handle fused call is one ordinary launch, not a one-segment run_multi (its _ex form, live.hip, is)
int bsdfd_plugin_sample_pdf(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, const float* wl, uint64_t seed,
                            uint64_t offset, int64_t N, int32_t T, float* wo, float* pdf_wo, float* pdf_wl, void* stream) {
    return run(h, {.op = OP_SAMPLE_PDF, .io = plugin_io(variant), .in_a = wi, .in_b = x0, .in_c = wl, .seed = seed, .offset = offset,
                   .N = N, .T = T, .out_x = wo, .out_pdf = pdf_wo, .out_pdf2 = pdf_wl, .stream = stream});
}

int bsdfd_set_profiling(bsdfd_handle h, int32_t enable) {
    if (!h) return fail(BSDFD_EINVAL, "null handle");
    std::lock_guard<std::mutex> lock(h->prof_mu);
    for (int i = 0; i < bsdfd_ctx::RING; ++i)
        if (h->pending[i]) HIP_TRY(harvest(h, i));
    h->profiling = enable != 0;
    h->n_rec = h->n_done = 0;
    h->total_ms = 0.0;
    h->last_ms = -1.0f;
    for (int i = 0; i < 8; ++i) { h->n_op[i] = 0; h->ms_op[i] = 0.0; }
    HIP_TRY(hipMemset(h->d_clk, 0, (size_t)CLK_SLOTS * 8 * sizeof(unsigned long long)));  // (every pending launch was harvested above: nothing is in flight)
    // the memset runs on the legacy stream and is asynchronous to the host: a profiled launch issued right behind this call on a
    // NON-BLOCKING stream (torch side streams, the WavefrontPipeline streams) is not ordered behind it and its counters could be
    // wiped — wait for it here (this entry point synchronises anyway: see include/bsdfd.h)
    HIP_TRY(hipStreamSynchronize(nullptr));
    return BSDFD_OK;
}

int bsdfd_profile_read(bsdfd_handle h, int64_t* n_launches, double* total_ms) {
    if (!h) return fail(BSDFD_EINVAL, "null handle");
    std::lock_guard<std::mutex> lock(h->prof_mu);
    // harvest in launch order so last_ms is the most recent launch
    for (long long k = h->n_done; k < h->n_rec; ++k) {
        const int slot = (int)(k % bsdfd_ctx::RING);
        if (h->pending[slot]) HIP_TRY(harvest(h, slot));
    }
    if (n_launches) *n_launches = h->n_done;
    if (total_ms) *total_ms = h->total_ms;
    return BSDFD_OK;
}

int bsdfd_profile_read_op(bsdfd_handle h, int32_t op, int64_t* n_launches, double* total_ms) {
    if (op < 0 || op > BSDFD_OP_RESIDENT + OP_PDF)
        return fail(BSDFD_EINVAL, "op must be one of BSDFD_OP_SAMPLE, _PDF, _SAMPLES_ONLY, _SAMPLE_PDF, or BSDFD_OP_RESIDENT + _SAMPLE / _PDF");
    int rc = bsdfd_profile_read(h, nullptr, nullptr);
    if (rc != BSDFD_OK) return rc;
    std::lock_guard<std::mutex> lock(h->prof_mu);
    if (n_launches) *n_launches = h->n_op[op];
    if (total_ms) *total_ms = h->ms_op[op];
    return BSDFD_OK;
}

int bsdfd_profile_clock_mhz(bsdfd_handle h, double* mhz) {
    if (!mhz) return fail(BSDFD_EINVAL, "null argument");
    int rc = bsdfd_profile_read(h, nullptr, nullptr);
    if (rc != BSDFD_OK) return rc;
    std::lock_guard<std::mutex> lock(h->prof_mu);
    std::vector<unsigned long long> st((size_t)CLK_SLOTS * 8);   // (bsdfd_profile_read has synchronised on every recorded launch)
    HIP_TRY(hipMemcpy(st.data(), h->d_clk, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double cyc = 0.0, ticks = 0.0;
    for (int i = 0; i < CLK_SLOTS; ++i) { cyc += (double)st[(size_t)i * 8]; ticks += (double)st[(size_t)i * 8 + 1]; }
    *mhz = (ticks > 0.0 && h->wall_khz > 0.0) ? cyc / ticks * h->wall_khz * 1e-3 : 0.0;
    return BSDFD_OK;
}

float bsdfd_last_kernel_ms(bsdfd_handle h) {
    if (!h) return -1.0f;
    {
        std::lock_guard<std::mutex> lock(h->prof_mu);
        if (!h->profiling || h->n_rec == 0) return -1.0f;
    }
    if (bsdfd_profile_read(h, nullptr, nullptr) != BSDFD_OK) return -1.0f;
    std::lock_guard<std::mutex> lock(h->prof_mu);
    return h->last_ms;
}

const char* bsdfd_last_error(void) { return g_err.c_str(); }
#if defined(BSDFD_COMPILER_ONLY_BUILD)
#define BSDFD_VERIFIED_TAG "; COMPILER-ONLY BUILD (BSDFD_COMPILER_ONLY_BUILD=1): no inline-asm LDS reads or SDWA sigmoids, device assembly not inspected"
#elif defined(BSDFD_UNVERIFIED_BUILD)
#define BSDFD_VERIFIED_TAG "; UNVERIFIED BUILD: shipped with BSDFD_ALLOW_UNVERIFIED_BUILD=1 although the assembly checks failed"
#else
#define BSDFD_VERIFIED_TAG ""
#endif
const char* bsdfd_version(void) {   // (the variant words come from the unit the variant flags were applied to: bsdfd.hip)
    static const std::string v = std::string("bsdfd 0.6 (gfx950; ") + bsdfd_flow_variant() + BSDFD_VERIFIED_TAG ")";
    return v.c_str();
}
int32_t bsdfd_abi_version(void) { return BSDFD_ABI_VERSION; }

}  // extern "C"
