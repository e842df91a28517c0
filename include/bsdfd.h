/*
 * bsdfd.h — C ABI of the MI355X-native neural-BSDF flow sampler ("bsdfd").
 *
 * This is the drop-in boundary for the ONE hot path of fzy28/BSDF_diffusion_sampling:
 * the per-query rectified-flow sampler and its change-of-variables PDF behind the
 * Mitsuba plugin methods sample()/pdf().  Plain pointers and sizes only — no torch
 * types.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions (modelled on how the reference binds its only native library,
 * tiny-cuda-nn/bindings/torch/tinycudann/bindings.cpp:79-110):
 *   - all data pointers are DEVICE pointers to contiguous row-major fp32, caller-owned;
 *   - no allocation inside sample/pdf calls; any N >= 0 (ragged tail handled in-kernel);
 *   - work is enqueued on the HIP stream the caller passes (NULL = default stream)
 *     and the call returns without synchronising;
 *   - return value 0 = ok, otherwise a BSDFD_E* code; bsdfd_last_error() returns a
 *     thread-local message (the Python host raises RuntimeError with it);
 *   - a handle is immutable after create and bound to the device current at create;
 *     calls are re-entrant across host threads and streams (the optional launch-timing
 *     counters of bsdfd_set_profiling are the only mutable state and are mutex-guarded).
 */
#ifndef BSDFD_H
#define BSDFD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header: bumped whenever a struct grows or an entry point changes.  Structs (bsdfd_desc, bsdfd_opts,
 * bsdfd_wf_scene) may grow AT THE END between versions and MUST be zero-initialised by the caller (memset / `= {0}`): a zero
 * field always selects the behaviour of the version that did not have it.  A host checks bsdfd_abi_version() ==
 * BSDFD_ABI_VERSION once after loading the library (the Python hosts do: _lib.lib()).
 *   5: bsdfd_desc.reserved became bsdfd_desc.tile (values other than 0 / 16 / 32 are rejected, 0 = library default).
 *   6: bsdfd_opts.row_index appended; bsdfd_abi_version() added.
 *   7: bsdfd_bucket_wide_workspace_bytes() and bsdfd_bucket_by_material_wide() added.
 *   8: bsdfd_live_workspace_bytes(), bsdfd_compact_live() and bsdfd_plugin_sample_pdf_ex() added (`active` masks).
 *      Added later WITHOUT a new version (no struct or existing entry point changed; a host that needs them looks the symbols
 *      up): bsdfd_measured_table_create(), bsdfd_measured_table_destroy(), bsdfd_measured_eval_table() and
 *      bsdfd_measured_sample_weight_table() (eval() of a mixed-material wavefront in one launch);
 *      bsdfd_measured_sample(), bsdfd_measured_pdf(), bsdfd_measured_sample_table(), bsdfd_measured_pdf_table() and
 *      bsdfd_measured_has_luminance() (the measured BSDF's own importance sampler);
 *      bsdfd_wf_path_begin(), bsdfd_wf_bounce() and bsdfd_wf_resolve() (occlusion and further bounces in the array scene);
 *      bsdfd_wf_sample_emitter() and bsdfd_wf_bounce_lit(), which take a struct of their own, bsdfd_wf_lights: point emitters
 *      in the array scene;
 *      bsdfd_env_sample(), bsdfd_env_pdf(), bsdfd_wf_sample_env() and bsdfd_wf_bounce_env(), which take a struct of their own,
 *      bsdfd_env_dist: importance sampling of the environment map in the array scene;
 *      bsdfd_wf_bounce_rr(): Russian roulette inside the bounce of the array scene;
 *      bsdfd_dielectric_eval(), bsdfd_dielectric_sample_weight(), bsdfd_dielectric_sample() and bsdfd_dielectric_pdf(), which
 *      take a struct of their own, bsdfd_dielectric: the rough-dielectric ground truth of the full-sphere plugin;
 *      bsdfd_principled_eval(), bsdfd_principled_sample_weight(), bsdfd_principled_sample() and bsdfd_principled_pdf(), which
 *      take a struct of their own, bsdfd_principled: the principled ground truth of the full-sphere plugin;
 *      bsdfd_analytic_table_create(), bsdfd_analytic_table_destroy(), bsdfd_analytic_eval_table(),
 *      bsdfd_analytic_sample_weight_table(), bsdfd_analytic_sample_table() and bsdfd_analytic_pdf_table(), which take a struct
 *      of their own, bsdfd_analytic_entry: both analytic models for a mixed-material wavefront in one launch;
 *      bsdfd_bucket_rows(), bsdfd_wf_bounce_rows(), bsdfd_wf_sample_emitter_rows(), bsdfd_wf_sample_env_rows(),
 *      bsdfd_measured_eval_table_rows() and bsdfd_analytic_eval_table_rows(): the per-depth calls of the array scene over a
 *      live-lane list;
 *      bsdfd_wf_bounce_transmit(), bsdfd_wf_sample_inside() and bsdfd_wf_sample_inside_rows(): transmitted paths through the
 *      balls of the array scene;
 *      bsdfd_mesh_bvh_build(), bsdfd_mesh_scene_create(), bsdfd_mesh_scene_destroy(), bsdfd_mesh_intersect(),
 *      bsdfd_mesh_occluded() and bsdfd_mesh_primary(), which take structs of their own, bsdfd_mesh_desc and bsdfd_mesh_instance:
 *      ray casting on the array scenes' triangle meshes;
 *      bsdfd_mesh_path_primary(), bsdfd_mesh_sample_emitter() and bsdfd_mesh_bounce(): the path tracer of the array scene on
 *      those meshes;
 *      bsdfd_mesh_sample_emitter_rows() and bsdfd_mesh_bounce_rows(): its per-depth calls over a live-lane list. */
#define BSDFD_ABI_VERSION 8

#define BSDFD_OK 0
#define BSDFD_EINVAL 1   /* bad argument / unsupported architecture */
#define BSDFD_EHIP 2     /* a HIP runtime call failed */
#define BSDFD_EIO 3      /* weight file unreadable / malformed */

#define BSDFD_DOMAIN_DISK 0       /* state = 2-D point on the unit disk          */
#define BSDFD_DOMAIN_SPHERICAL 1  /* state = (theta, phi); net input [theta, sin phi, cos phi] */

/* Arithmetic of the dense layer contractions.  Activations, Jacobian determinant, base density and warps are fp32 VALU —
 * with ONE exception: bsdfd_flow_samples_only in BSDFD_PREC_F16 (both tilings) evaluates the hidden layers' sigmoids in
 * packed fp16 as well (see BSDFD_PREC_F16). */
#define BSDFD_PREC_DEFAULT 0  /* = BSDFD_PREC_SPLIT3 */
#define BSDFD_PREC_F32 1      /* v_mfma_f32_16x16x4_f32: exact fp32 FMA chains (validation mode) */
#define BSDFD_PREC_SPLIT3 2   /* fp16 MFMA, operands split hi+lo, 3 products, fp32 accumulate (<=1e-4 parity).
                               * Range: hidden activations and tangents must stay below fp16's 65504 (they are
                               * O(1..100) for the reference's nets and inputs); beyond it the result is inf/NaN,
                               * never a silently wrong finite number. BSDFD_PREC_F32 has fp32 range. */
#define BSDFD_PREC_F16 3      /* single fp16 MFMA pass (tcnn-class 1e-2 tolerance; reflow teacher sampling).  The kernels of
                               * bsdfd_flow_samples_only in this precision — 16- AND 32-query tiles — also evaluate the hidden
                               * layers' sigmoids in packed fp16 (the 16-query kernels: every hidden layer; the 32-query
                               * kernels keep the last hidden layer's in fp32): that call is its own fp16-class evaluation and
                               * does NOT walk the trajectory of bsdfd_network_sampling(BSDFD_PREC_F16) bit for bit (agreement
                               * ~2e-2, the class's tolerance).  Range: |pre-activation| must stay below ~4.5e4 (fp16's
                               * largest finite value); beyond it sigma evaluates inf * 0 = NaN, never a wrong finite number. */

/* Plugin post-processing variants (which MyBSDF the call mirrors). */
#define BSDFD_PLUGIN_MEASURED 0    /* rendering/brdf_measured_{disk,spherical}.py */
#define BSDFD_PLUGIN_FULLSPHERE 1  /* rendering/bsdf_myresult.py (spherical only) */

typedef struct bsdfd_ctx* bsdfd_handle;

/* The four kinds of flow-kernel launch (bsdfd_get_tile, bsdfd_profile_read_op). */
#define BSDFD_OP_SAMPLE 0        /* network_sampling, plugin_sample      */
#define BSDFD_OP_PDF 1           /* network_pdf, plugin_pdf              */
#define BSDFD_OP_SAMPLES_ONLY 2  /* flow_samples_only                    */
#define BSDFD_OP_SAMPLE_PDF 3    /* plugin_sample_pdf                    */
/* bsdfd_profile_read_op only: BSDFD_OP_RESIDENT + BSDFD_OP_SAMPLE / _PDF = those launches of the operation that ran the
 * register-resident fast-path kernel (plain single-material plugin sample / pdf of the disk net at T = 8, 16, 32, ...). */
#define BSDFD_OP_RESIDENT 4

/* Host pointers to fp32 row-major [out, in] matrices exactly as nn.Linear.weight
 * stores them (reference checkpoints: rendering/checkpoints_new/.../brdf_rectify_network*.pth
 * and brdf_pretrain_network*.pth, loaded at rendering/brdf_measured_disk.py:43-51).
 * The library copies and re-packs them; the caller may free them after create. */
typedef struct bsdfd_desc {
    int32_t domain;         /* BSDFD_DOMAIN_*                                            */
    int32_t width;          /* hidden width of the velocity net: 32 or 64                */
    int32_t n_hidden;       /* hidden layers: 3 (disk), 4 (spherical), 6 (64-wide teacher) */
    int32_t pe_bands;       /* positional-encoding bands of the velocity net (5)         */
    int32_t base_hidden;    /* hidden width of the base-density net (16)                 */
    int32_t base_pe_bands;  /* positional-encoding bands of the base net (3)             */
    int32_t precision;      /* BSDFD_PREC_*                                              */
    int32_t tile;           /* queries per wave64 tile: 0 = library default (32 where such a kernel exists), 16 = the
                             * 16x16x32-MFMA kernels (every net), 32 = the 32x32x16-MFMA kernels, which exist for
                             *   (1) the reference's two plugin nets — disk 32x3, spherical 32x4 — in BSDFD_PREC_SPLIT3 (all calls),
                             *   (2) bsdfd_flow_samples_only of the 64 x 6 spherical teacher in BSDFD_PREC_F16,
                             *   (3) bsdfd_flow_samples_only of those two 32-wide nets in BSDFD_PREC_F16,
                             *   (4) the Jacobian calls (sampling / pdf, operator and plugin level) of the 64 x 6 spherical net in
                             *       BSDFD_PREC_SPLIT3 — OPT-IN: served only when 32 is asked for explicitly (it measured 4 % slower
                             *       than the 16-query kernel, which stays this net's default).
                             * An explicit 32 for a (net, precision) with no such kernel at all is REJECTED by bsdfd_create
                             * (BSDFD_EINVAL); where only some calls have one — (2), (3), (4) — the others run 16-query tiles and
                             * bsdfd_get_tile says which.  Product behaviour depends on this field alone: the library reads
                             * no environment variable (the Python hosts map $BSDFD_TILE onto it for A/B runs).
                             * Both tilings implement the same operators to the same tolerance.  Was `reserved` before ABI 5:
                             * zero-initialise the struct. */
    const float* w_in;      /* [width, state_dim + 1 + 2 + 4*pe_bands], cols [state|alpha|PE(omega_i)] */
    const float* w_hidden;  /* [n_hidden-1, width, width]                                */
    const float* w_out;     /* [2, width]                                                */
    const float* base_w1;   /* [base_hidden, 2 + 4*base_pe_bands]                        */
    const float* base_b1;   /* [base_hidden]                                             */
    const float* base_w2;   /* [4, base_hidden]                                          */
    const float* base_b2;   /* [4]                                                       */
} bsdfd_desc;

/* Replaces MyBSDF.__init__'s network construction + load_state_dict
 * (rendering/brdf_measured_disk.py:43-51, brdf_measured_spherical.py:53-59,
 * bsdf_myresult.py:49-54). */
int bsdfd_create(const bsdfd_desc* desc, bsdfd_handle* out);

/* Same, from a neutral .bsdfw file (format: bsdf_diffusion_sampling_amd/weights.py);
 * replaces torch.load of the pickle checkpoints. precision = BSDFD_PREC_*. */
int bsdfd_create_from_file(const char* path, int32_t precision, bsdfd_handle* out);

void bsdfd_destroy(bsdfd_handle h);

/* Introspection (host side mirrors / bench): domain, width, n_hidden, precision in
 * effect; algorithmic flop per query for T Euler steps. */
int bsdfd_get_info(bsdfd_handle h, int32_t* domain, int32_t* width, int32_t* n_hidden,
                   int32_t* precision);
int64_t bsdfd_flops_per_query(bsdfd_handle h, int32_t T);
/* Queries per wave64 tile (16 or 32, see bsdfd_desc.tile) of the kernel this handle launches for `op` (BSDFD_OP_*).  For
 * BSDFD_OP_SAMPLE / _PDF it is the granularity of the opaque per-query context below.  (A handle may mix tilings: the 64 x 6 teacher
 * in BSDFD_PREC_F16 has a 32-query-tile kernel for bsdfd_flow_samples_only alone.)  No counterpart in the reference. */
int bsdfd_get_tile(bsdfd_handle h, int32_t op, int32_t* tile);

/* network_sampling_disk / network_sampling_spherical
 * (rendering/utils/mlp_brdf_sampling.py:17-51, :106-140).
 *   omega_i [N,2]  condition: disk coords of wi, or (theta_i, phi_i)
 *   x0      [N,2]  base draw, or NULL: drawn in-kernel from D_base with a Philox4x32-10
 *                  stream keyed (seed, offset + query index) — statistically, not
 *                  bit-wise, equal to torch's RNG
 *   x_out   [N,2]  flowed sample;  pdf_out [N]  p0(x0) * prod 1/det(I + J/T), signed. */
int bsdfd_network_sampling(bsdfd_handle h, const float* omega_i, const float* x0, uint64_t seed,
                           uint64_t offset, int64_t N, int32_t T, float* x_out, float* pdf_out,
                           void* hip_stream);

/* network_pdf_disk / network_pdf_spherical (mlp_brdf_sampling.py:69-103, :144-181). */
int bsdfd_network_pdf(bsdfd_handle h, const float* omega_o, const float* omega_i, int64_t N,
                      int32_t T, float* pdf_out, void* hip_stream);

/* Tensor core of MyBSDF.sample with the domain warp and guards fused
 * (rendering/brdf_measured_disk.py:59-82; brdf_measured_spherical.py:69-91;
 *  bsdf_myresult.py:59-84 when variant = BSDFD_PLUGIN_FULLSPHERE):
 *   wi [N,3] unit vectors in the local frame -> wo [N,3], pdf_sa [N] (solid-angle pdf).
 * The measured.eval()-dependent firefly rule (:97-100) is NOT applied here. */
int bsdfd_plugin_sample(bsdfd_handle h, int32_t variant, const float* wi, const float* x0,
                        uint64_t seed, uint64_t offset, int64_t N, int32_t T, float* wo,
                        float* pdf_sa, void* hip_stream);

/* Tensor core of MyBSDF.pdf (rendering/brdf_measured_disk.py:112-124;
 * brdf_measured_spherical.py:122-137; bsdf_myresult.py:115-133). */
int bsdfd_plugin_pdf(bsdfd_handle h, int32_t variant, const float* wi, const float* wo, int64_t N,
                     int32_t T, float* pdf_sa, void* hip_stream);

/* sample(wi) and pdf(wi, wl) for the SAME intersections in one launch: the per-query prologue
 * (positional encoding, conditioning term of layer 1, base-density net) is evaluated once and the flow
 * runs twice (forward from the base draw, reverse from wl).  This is the call pattern of a renderer
 * with next-event estimation (one sample() and one pdf() per path and bounce); results are identical
 * to bsdfd_plugin_sample followed by bsdfd_plugin_pdf(wi, wl). */
int bsdfd_plugin_sample_pdf(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, const float* wl,
                            uint64_t seed, uint64_t offset, int64_t N, int32_t T, float* wo, float* pdf_wo,
                            float* pdf_wl, void* hip_stream);

/* Per-query context: what the kernel derives from wi ALONE — the conditioning term of layer 1
 * (W1[:, PE(omega_i)] PE(omega_i), once per query instead of once per Euler step as rendering/utils/model.py:494
 * recomputes it) and the base-density net's four outputs (evaluated twice per sample() by
 * rendering/utils/mlp_brdf_sampling.py:20,24) — 144 B per query for the 32-wide nets, 272 B for 64-wide.
 * A renderer calls sample(si) and pdf(si, wl) for the SAME intersections (rendering/brdf_measured_disk.py:59,112 are
 * both driven by one `si`) — Mitsuba's path integrator in the order eval_pdf() (emitter sampling, :126 -> :112) first,
 * sample() (:59) second — so EITHER call may write the context while it runs (opts->ctx_out) and either may read it
 * (opts->ctx_in) instead of re-evaluating the prologue (cart_to_spher(wi), 22 sin/cos, the conditioning contraction and the
 * base net: 20 fp32 MFMAs per 16 queries).  A call takes at most one of the two.
 * Results are BIT-IDENTICAL to the calls without a context.  The buffer is opaque device memory of
 * bsdfd_context_bytes(h, N, n_segments) bytes (n_segments = 1 for single-material calls, = n_handles for *_multi
 * calls), 16-byte aligned, valid only for the handle(s), the wi array and — for *_multi — the seg_end layout it
 * was written with; T may differ between the two calls.  NULL context = the plain call. */
int64_t bsdfd_context_bytes(bsdfd_handle h, int64_t N, int32_t n_segments);

/* Optional arguments of the plugin-level calls (NULL pointer / all-zero struct = the plain call). */
typedef struct bsdfd_opts {
    void* ctx_out;             /* sample / pdf calls: also write the per-query context of this wi array here        */
    const void* ctx_in;        /* sample / pdf calls: read the context an earlier call wrote for the same wi array  */
    const int64_t* rng_index;  /* sample calls: device array [N]; the Philox counter of row i is offset +
                                * rng_index[i] instead of offset + i.  A wavefront that was bucketed by material
                                * passes the rows' ORIGINAL lane indices here: the base draws then depend on neither
                                * the bucketing nor the sharding / GPU count.                */
    const int64_t* row_index;  /* sample / pdf / sample_pdf calls (ABI 6): device array [N]; row i of the call READS its
                                * inputs (wi, x0, wo / wl) at row row_index[i] of the callers' arrays and WRITES its outputs
                                * there.  A wavefront bucketed by material hands over the bucket permutation
                                * (bsdfd_bucket_by_material's perm) with the callers' lane-ordered arrays: no gathered copy of
                                * the inputs, no scatter of the results (the dispatch it replaces: one plugin instance per
                                * material called on its lanes, rendering/matpreview/disney_bsdf_array0_envmap.xml +
                                * rendering/brdf_measured_disk.py:140).  seg_end, the per-query context and rng_index stay
                                * indexed by i; without rng_index the Philox counter of row i is offset + row_index[i].
                                * Rows not named by row_index are not touched.  Entries must be distinct and inside the
                                * callers' arrays; the library cannot check either (it is not told the arrays' lengths;
                                * the Python hosts do under BSDFD_CHECK_INDEX=1).                                      */
} bsdfd_opts;
int bsdfd_plugin_sample_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, uint64_t seed,
                           uint64_t offset, int64_t N, int32_t T, float* wo, float* pdf_sa, const bsdfd_opts* opts,
                           void* hip_stream);
int bsdfd_plugin_pdf_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* wo, int64_t N, int32_t T,
                        float* pdf_sa, const bsdfd_opts* opts, void* hip_stream);

/* Mixed-material batches (BASELINE.json configs[3]; the reference binds one plugin instance per material,
 * rendering/matpreview/disney_bsdf_array0_envmap.xml, and Mitsuba calls each instance on its lanes).
 * The query arrays are BUCKETED by material: bucket i = rows [seg_end[i-1], seg_end[i]) (seg_end is a HOST
 * array of n_handles cumulative ends; empty buckets allowed) is served by handles[i].  All handles must
 * share domain, width, depth, precision and device; ONE launch serves up to 64 buckets (workgroups are
 * dealt to buckets in proportion to their sizes, each loads its material's weight image into LDS).
 * The Philox counter of a row is offset + its row index in the bucketed array. */
int bsdfd_plugin_sample_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                              int32_t variant, const float* wi, const float* x0, uint64_t seed,
                              uint64_t offset, int32_t T, float* wo, float* pdf_sa, void* hip_stream);
int bsdfd_plugin_pdf_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                           int32_t variant, const float* wi, const float* wo, int32_t T, float* pdf_sa,
                           void* hip_stream);
/* bsdfd_plugin_sample_pdf over material buckets (same bucket layout as bsdfd_plugin_sample_multi) */
int bsdfd_plugin_sample_pdf_multi(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                                  int32_t variant, const float* wi, const float* x0, const float* wl,
                                  uint64_t seed, uint64_t offset, int32_t T, float* wo, float* pdf_wo,
                                  float* pdf_wl, void* hip_stream);

/* the *_multi calls with optional arguments (bsdfd_opts; a context spans n_segments = n_handles buckets) */
int bsdfd_plugin_sample_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                                 int32_t variant, const float* wi, const float* x0, uint64_t seed, uint64_t offset,
                                 int32_t T, float* wo, float* pdf_sa, const bsdfd_opts* opts, void* hip_stream);
int bsdfd_plugin_pdf_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                              int32_t variant, const float* wi, const float* wo, int32_t T, float* pdf_sa,
                              const bsdfd_opts* opts, void* hip_stream);
/* bsdfd_plugin_sample_pdf_multi with opts->rng_index (the fused call takes no context: its prologue stays in registers) */
int bsdfd_plugin_sample_pdf_multi_ex(const bsdfd_handle* handles, int32_t n_handles, const int64_t* seg_end,
                                     int32_t variant, const float* wi, const float* x0, const float* wl, uint64_t seed,
                                     uint64_t offset, int32_t T, float* wo, float* pdf_wo, float* pdf_wl,
                                     const bsdfd_opts* opts, void* hip_stream);
/* bsdfd_plugin_sample_pdf with optional arguments (ABI 8): the single-handle form of the call above, with its rules (rng_index
 * and row_index; no per-query context).  With the row list of bsdfd_compact_live() as opts->row_index it is the fused
 * sample() + pdf() of the lanes an `active` mask selects — the `active` argument of the reference's plugin methods
 * (rendering/brdf_measured_disk.py:59,112), i.e. Mitsuba calling an instance on its lanes only.  NULL opts = the plain call. */
int bsdfd_plugin_sample_pdf_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, const float* wl,
                               uint64_t seed, uint64_t offset, int64_t N, int32_t T, float* wo, float* pdf_wo,
                               float* pdf_wl, const bsdfd_opts* opts, void* hip_stream);

/* Reflow teacher sampling without the Jacobian: x <- x + v(x, t/T | omega_i)/T for T steps
 * (learning_repo_cleanup/spherical_domain_sampling.py:147-166, disk_domain_sampling.py:93-110 —
 * the reference's only tiny-cuda-nn call site). x0 [N,2] in, x_out [N,2] out. */
int bsdfd_flow_samples_only(bsdfd_handle h, const float* omega_i, const float* x0, int64_t N,
                            int32_t T, float* x_out, void* hip_stream);

/* Kernel timing with HIP events ON THE LAUNCH STREAM: while profiling is enabled every launch
 * through this handle is bracketed by an event pair recorded on the stream the kernel is
 * launched on (a ring of 64 pairs; no host synchronisation unless the ring wraps onto a launch
 * that is still running).  bsdfd_set_profiling resets the counters.
 * bsdfd_profile_read synchronises on the outstanding stop events and returns the number of
 * launches and the sum of their durations (ms) since profiling was enabled;
 * bsdfd_last_kernel_ms returns the duration of the most recent launch (negative if none).
 * bsdfd_set_profiling / bsdfd_profile_* synchronise and touch device memory from the host: not while a stream is being captured
 * (launches THROUGH a profiling handle are capture-safe only with profiling off: event records inside a capture become graph nodes). */
int bsdfd_set_profiling(bsdfd_handle h, int32_t enable);
int bsdfd_profile_read(bsdfd_handle h, int64_t* n_launches, double* total_ms);
float bsdfd_last_kernel_ms(bsdfd_handle h);
/* The same totals for ONE kind of launch (bench.py's sample / pdf split of the timed region itself): `op` is
 * BSDFD_OP_SAMPLE (network_sampling, plugin_sample), BSDFD_OP_PDF (network_pdf, plugin_pdf), BSDFD_OP_SAMPLES_ONLY
 * (flow_samples_only) or BSDFD_OP_SAMPLE_PDF (plugin_sample_pdf); BSDFD_OP_RESIDENT + BSDFD_OP_SAMPLE / _PDF: the part of that
 * operation's launches which took the fast-path kernel (which kernel a call ran).  No counterpart in the reference. */
int bsdfd_profile_read_op(bsdfd_handle h, int32_t op, int64_t* n_launches, double* total_ms);
/* Shader clock (MHz) the chip sustained UNDER THE PROFILED LAUNCHES THEMSELVES: while profiling is enabled every wave adds its
 * lifetime in shader cycles (s_memtime) and in ticks of the constant-rate wall clock (s_memrealtime,
 * hipDeviceAttributeWallClockRate) to two words of the handle — both read by the same wave, so counter offsets between CUs
 * cancel; the ratio of the sums x the wall-clock rate is the clock, averaged over the waves' lifetimes.  This is what
 * bench.py's issue-bound entry divides by (the stand-alone probe below runs a similar instruction mix, not the kernel itself,
 * and may draw a different clock: "DVFS give-back", MI355X_MICROARCH.md).  0 if nothing was recorded.  No counterpart in the
 * reference. */
int bsdfd_profile_clock_mhz(bsdfd_handle h, double* mhz);

/* Shader clock (MHz) the chip sustains under the flow kernel's instruction mix: a ~6 ms probe launch on every
 * CU, shader-cycle count of the LONGEST-lived wave (maximum over all waves) / HIP-event duration (csrc/clock.hip).
 * The probe allocates, copies back and SYNCHRONISES: it must not be called while a stream is being captured
 * (the rest of the API is capture-safe).  Measurement only: bench.py
 * uses it to state kernel time in shader cycles per (16-query tile x Euler step) next to the instruction-issue
 * model of that loop (the "issue-bound" roofline entry).  No counterpart in the reference. */
int bsdfd_shader_clock_mhz(double* mhz, void* hip_stream);

/* Stand-alone positional encoding = the reference's positional_encoding_1 (rendering/utils/model.py:9-57):
 * x [N,dim] -> out [N, dim * (include_input + 2 * bands)] = cat([x], sin(f_0 x), cos(f_0 x), ...), f = 2^b
 * (log_sampling) or linspace(1, 2^(bands-1), bands).  Fused (and free) inside the flow kernel; this
 * un-fused pass is the drop-in for the reference function and the HBM-bound "encoding pass". */
int bsdfd_positional_encoding(const float* x, int64_t N, int32_t dim, int32_t bands, int32_t include_input,
                              int32_t log_sampling, float* out, void* hip_stream);

/* ---- bucketing of a material-tagged wavefront (config 4) ---------------------------------------------
 * Stable counting sort of N lanes by material id (int64, 0 <= id < n_materials <= 64), on the device:
 * perm [N] gathers lanes into bucket order (torch.argsort(stable=True) semantics), counts [n_materials]
 * are the bucket sizes (device memory).  `workspace`: device scratch of bsdfd_bucket_workspace_bytes().
 * Lanes with an id outside the range are left out of perm (counts then sum to less than N). */
int64_t bsdfd_bucket_workspace_bytes(int64_t N, int32_t n_materials);
int bsdfd_bucket_by_material(const int64_t* material_id, int64_t N, int32_t n_materials, int64_t* perm,
                             int64_t* counts, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* The same sort for 1 <= n_materials <= 65536 (ABI 7): what the reference scene spells as one `mybsdf` instance per
 * material, each lane dispatched to its instance by Mitsuba, for scenes with more than 64 of them.  Same contract as
 * bsdfd_bucket_by_material: perm [N] in torch.argsort(stable=True) order, counts [n_materials] on the device; a lane whose
 * id — the full 64-bit value — is outside [0, n_materials) is left out, the kept lanes fill perm[0 .. sum(counts)) and the
 * rest of perm is unspecified.  One stable counting pass per 6-bit digit of the id (two passes up to 4096 materials, three
 * above).  Deterministic, independent of what `workspace` (device scratch of bsdfd_bucket_wide_workspace_bytes(), 8-byte
 * aligned) held before; allocates nothing and does not synchronise: everything is enqueued on hip_stream.  N == 0 only
 * zeroes counts.  bsdfd_bucket_wide_workspace_bytes() returns 0 for N < 0 or n_materials outside [1, 65536]. */
int64_t bsdfd_bucket_wide_workspace_bytes(int64_t N, int32_t n_materials);
int bsdfd_bucket_by_material_wide(const int64_t* material_id, int64_t N, int32_t n_materials, int64_t* perm,
                                  int64_t* counts, void* workspace, int64_t workspace_bytes, void* hip_stream);

/* Bucket order <-> lane order around a run of bucketed calls (a renderer keeps a wavefront in bucket order across its
 * sample() and pdf() calls): wi_b[i] = wi[perm[i]] for the first n entries of perm (the lanes that carry a material), and
 * the inverse for the results, all arrays of a wavefront in ONE pass (NULL = skip that array): wo[perm[i]] = wo_b[i],
 * pdf[perm[i]] = pdf_b[i], pdf2[perm[i]] = pdf2_b[i].  Lanes not named by perm[0..n) are left untouched. */
int bsdfd_gather_lanes(const int64_t* perm, int64_t n, const float* wi, float* wi_b, void* hip_stream);
int bsdfd_scatter_lanes(const int64_t* perm, int64_t n, const float* wo_b, const float* pdf_b, const float* pdf2_b,
                        float* wo, float* pdf, float* pdf2, void* hip_stream);

/* ---- live lanes of a wavefront (ABI 8) -------------------------------------------------------------------
 * Replaces the `active` argument of the reference's plugin methods (rendering/brdf_measured_disk.py:59,64,101,112: sample,
 * the DrJit select on its weight, eval, pdf), which Mitsuba uses to call an instance on its lanes only: an order-preserving
 * compaction of the N lanes of a wavefront into the row list the plugin-level calls take as bsdfd_opts.row_index.  Lane i is
 * live when `active` is NULL or active[i] != 0, and (BSDFD_LIVE_WI_UPPER unset or wi[3i+2] > 0), and (BSDFD_LIVE_DIR_UPPER
 * unset or dir[3i+2] > 0) — the comparisons of the kernels' own hemisphere guards, so NaN and +-0 are dead; the two flags
 * cull the lanes for which the pdf of the `measured` plugins is 0 anyway (:112-124).  rows[0 .. count) receives the live row
 * numbers in ascending order (rows holds up to N entries; the rest is unspecified), count is a DEVICE int64[1].  In the same
 * pass the DEAD rows of up to three result arrays are set to 0 — zero_wo [N,3], zero_pdf [N], zero_pdf2 [N], each may be
 * NULL; their live rows are not touched (the masked call writes them).  `workspace`: device scratch of
 * bsdfd_live_workspace_bytes() (0 for N < 0), 8-byte aligned; the result does not depend on what it held before.  Allocates
 * nothing and does not synchronise: everything is enqueued on hip_stream (no workgroup waits on another one).  N == 0 only
 * writes count = 0. */
#define BSDFD_LIVE_WI_UPPER 1
#define BSDFD_LIVE_DIR_UPPER 2
int64_t bsdfd_live_workspace_bytes(int64_t N);
int bsdfd_compact_live(const unsigned char* active, const float* wi, const float* dir, int32_t flags, int64_t N,
                       int64_t* rows, int64_t* count, float* zero_wo, float* zero_pdf, float* zero_pdf2,
                       void* workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- ground-truth evaluator for eval(): RGL measured BSDF (rgb tensor files) -----------------------
 * Replaces, for the plugins' eval() / sample-weight / firefly rule, the Mitsuba `measured` BSDF the
 * reference builds in rendering/brdf_measured_disk.py:36-42 (`mi.load_dict({'type': 'measured',
 * 'filename': 'measuredbsdfs/<name>.bsdf'})`) and evaluates at :96,107.  Model: Dupuy & Jakob 2018
 * (csrc/measured.hip).  rgb_out [N,3] = f(wi, wo) * cos(theta_o), 0 where cos(theta_i) <= 0 or
 * cos(theta_o) <= 0 — Mitsuba's eval() convention. */
typedef struct bsdfd_measured_ctx* bsdfd_measured_handle;
int bsdfd_measured_create_from_file(const char* path, bsdfd_measured_handle* out);
void bsdfd_measured_destroy(bsdfd_measured_handle h);
int bsdfd_measured_get_info(bsdfd_measured_handle h, int32_t* n_phi, int32_t* n_theta, int32_t* isotropic,
                            int32_t* jacobian, int32_t* reduction);
/* tint: host pointer to 3 floats (the plugin's albedo) or NULL */
int bsdfd_measured_eval(bsdfd_measured_handle h, const float* wi, const float* wo, int64_t N, const float* tint,
                        float* rgb_out, void* hip_stream);
/* The tail of the plugins' sample() in one pass (rendering/brdf_measured_disk.py:89-101,
 * brdf_measured_spherical.py:97-109): value = f * tint / pdf_sa on active lanes (cos(theta_i) > 0, and
 * active[q] != 0 if a mask is given) with pdf_sa > 0; firefly rule pdf_out = lum(value) < threshold ? pdf_sa : 0;
 * weight_out [N,3] = value where active, pdf_out > 0 and cos(theta_o) > 0, else 0. */
int bsdfd_measured_sample_weight(bsdfd_measured_handle h, const float* wi, const float* wo, const float* pdf_sa,
                                 const unsigned char* active, int64_t N, const float* tint, float firefly_threshold,
                                 float* weight_out, float* pdf_out, void* hip_stream);

/* eval() for a MIXED-material wavefront (csrc/measured_table.hip): one launch serves every material, where the calls above
 * take one launch per material on gathered slices.  The rows stay in lane order with their material ids, as bsdfd_wf_primary
 * writes them. */
typedef struct bsdfd_measured_table_ctx* bsdfd_measured_table;
/* handles[m] serves material id m; a NULL entry = "no ground truth for this material".  1 <= n_materials <= 65536,
 * at least one non-NULL handle, all on the current device.  The table copies the handles' device descriptors into one
 * device array; it borrows the handles' tensor data: the caller keeps the handles alive while the table lives. */
int  bsdfd_measured_table_create(const bsdfd_measured_handle* handles, int32_t n_materials, bsdfd_measured_table* out);
void bsdfd_measured_table_destroy(bsdfd_measured_table t);
/* eval() of a whole wavefront in LANE order, one launch: row i with 0 <= material_id[i] < n_materials (the full 64-bit
 * value) and a non-NULL handle gets f_o[i] = what bsdfd_measured_eval(handles[id], wi+3i, wo+3i, 1, tint, ...) writes, bit
 * for bit, and likewise f_l[i] from wl; every other row (floor, miss, NULL slot, id out of range or negative) gets a quiet
 * NaN in all three channels: the "use the proxy" value bsdfd_wf_shade reads.  wl and f_l are both NULL or both given. */
int  bsdfd_measured_eval_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                               const float* wl, int64_t N, const float* tint, float* f_o, float* f_l, void* hip_stream);
/* bsdfd_measured_sample_weight per lane's material: rows with ground truth get its weight_out / pdf_out bit for bit;
 * the others get weight_out = NaN and pdf_out = pdf_sa. */
int  bsdfd_measured_sample_weight_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi,
                                        const float* wo, const float* pdf_sa, const unsigned char* active, int64_t N,
                                        const float* tint, float firefly_threshold, float* weight_out, float* pdf_out,
                                        void* hip_stream);

/* ---- sample() / pdf() of the measured BSDF: the importance sampler every RGL file ships -------------------------------
 * Mitsuba's `measured` plugin draws with the file's `luminance` warp (optional field; without it that pdf is 1), then its VNDF
 * warp, then reflects wi about the sampled half vector (Dupuy & Jakob 2018).  Restated from the published model; PARITY-UNPINNED
 * against Mitsuba, like eval().  u [N,2] in [0,1)^2 are the caller's variates (Mitsuba's sample2).  Per row:
 *   wo_out [N,3]     the sampled direction (written as computed even where it leaves through the lower hemisphere),
 *   pdf_out [N]      its solid-angle density, 0 where wo.z <= 0 (or where the density is not a positive finite number),
 *   weight_out [N,3] f(wi, wo) cos(theta_o) * tint / pdf, 0 where pdf is 0 (may be NULL).
 * Rows with wi.z <= 0, and rows with active[i] == 0 when a mask is given (u8 [N] or NULL), get 0 in every output.
 * bsdfd_measured_pdf is the density of that sampler at a given wo: 0 unless wi.z > 0 and wo.z > 0.
 * All four calls are stream-ordered, allocate nothing and do not synchronise; N = 0 is a no-op. */
int bsdfd_measured_has_luminance(bsdfd_measured_handle h, int32_t* has_luminance);
int bsdfd_measured_sample(bsdfd_measured_handle h, const float* wi, const float* u, const unsigned char* active, int64_t N,
                          const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* hip_stream);
int bsdfd_measured_pdf(bsdfd_measured_handle h, const float* wi, const float* wo, const unsigned char* active, int64_t N,
                       float* pdf_out, void* hip_stream);
/* ... for a mixed-material wavefront in lane order: a row whose id names a non-NULL handle gets what the single-material call
 * writes for it, bit for bit (zeros where active[i] == 0 included); every other row gets a quiet NaN in every output. */
int bsdfd_measured_sample_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* u,
                                const unsigned char* active, int64_t N, const float* tint, float* wo_out, float* pdf_out,
                                float* weight_out, void* hip_stream);
int bsdfd_measured_pdf_table(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                             const unsigned char* active, int64_t N, float* pdf_out, void* hip_stream);

/* ---- analytic ground truth of the full-sphere plugin: the rough dielectric (csrc/dielectric.hip) -------------------------
 * The reference's full-sphere plugin takes eval(), the sample weight and the firefly rule from an analytic Mitsuba BSDF of its
 * material list (rendering/bsdf_myresult.py:97-110, rendering/utils/bsdf_dict.py); entries 23..25 of that list are
 * `roughdielectric` (Beckmann, alpha 0.2 / 0.3 / 0.5, bk7 in air).  Model: Walter et al. 2007 with Mitsuba's defaults — Beckmann
 * D, the rational Smith G1, exact unpolarised Fresnel, visible-normal sampling, radiance transport (the transmitted lobe carries
 * 1 / eta^2).  Restated from the publications; PARITY-UNPINNED against Mitsuba, like the measured model above.  fp32.
 * The material is this descriptor, read on the host at the call (zero-initialise it; it may grow at the end):
 *   alpha         Beckmann roughness (isotropic), > 0
 *   eta           int_ior / ext_ior, > 0
 *   distribution  0 = Beckmann; anything else is BSDFD_EINVAL
 * Directions are in the local shading frame; BOTH sides of the surface are served (wi.z < 0: from inside).  Per row:
 *   eval           rgb_out [N,3] = f(wi, wo) |cos theta_o| * tint (grey), 0 where wi.z == 0 or wo.z == 0, where the half vector is
 *                  undefined (|wi + k wo| < 1e-6) and where the value is not finite.
 *   sample_weight  the tail of the plugin's sample(): value = f |cos| * tint / pdf_sa (0 where pdf_sa <= 0); pdf_out = pdf_sa where
 *                  value.x < firefly_threshold, else 0; weight_out = value where pdf_out > 0, else 0.  No cosine masks.
 *   sample         u [N,3] in [0,1)^3: columns 0..1 are Mitsuba's sample2 (the visible normal), column 2 its sample1 (reflection
 *                  iff u2 <= F).  wo_out [N,3]; pdf_out [N] = what bsdfd_dielectric_pdf gives for (wi, wo_out), bit for bit;
 *                  weight_out [N,3] (may be NULL) = what bsdfd_dielectric_eval gives for that pair, divided by pdf_out — 0 where
 *                  pdf_out is 0 or wo_out is on the wrong side of the surface for the chosen lobe.  Rows with wi.z == 0 get zeros.
 *   pdf            the solid-angle density of that sampler at a given wo.
 * Rows with active[i] == 0, when a mask is given (u8 [N] or NULL), get 0 in every output.  tint: 3 floats on the host or NULL
 * (white).  All four calls are stream-ordered, allocate nothing and do not synchronise; N = 0 is a no-op. */
typedef struct {
    float alpha, eta;
    int32_t distribution, reserved;
} bsdfd_dielectric;
int bsdfd_dielectric_eval(const bsdfd_dielectric* desc, const float* wi, const float* wo, int64_t N, const float* tint,
                          float* rgb_out, void* hip_stream);
int bsdfd_dielectric_sample_weight(const bsdfd_dielectric* desc, const float* wi, const float* wo, const float* pdf_sa,
                                   const unsigned char* active, int64_t N, const float* tint, float firefly_threshold,
                                   float* weight_out, float* pdf_out, void* hip_stream);
int bsdfd_dielectric_sample(const bsdfd_dielectric* desc, const float* wi, const float* u, const unsigned char* active, int64_t N,
                            const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* hip_stream);
int bsdfd_dielectric_pdf(const bsdfd_dielectric* desc, const float* wi, const float* wo, const unsigned char* active, int64_t N,
                         float* pdf_out, void* hip_stream);

/* ---- analytic ground truth of the full-sphere plugin: the principled BSDF (csrc/principled.hip) ---------------------------
 * Entries 0..22 of the reference's material list (rendering/utils/bsdf_dict.py) are Mitsuba `principled` BSDFs.  Model: Burley
 * 2012 / 2015 with Mitsuba's choices — four sampled lobes (diffuse with retro-reflection, fake subsurface and sheen; a GTR1
 * clearcoat; specular transmission; specular reflection) over an anisotropic GGX distribution with the separable Smith G, exact
 * unpolarised Fresnel mixed with Schlick terms, radiance transport; visible normals drawn as in Heitz 2018.  Restated from the
 * publications; PARITY-UNPINNED against Mitsuba, like the two models above.  fp32.
 * The material is this descriptor, read on the host at the call (zero-initialise it; it may grow at the end).  Every parameter
 * but eta lies in [0, 1]; eta = int_ior / ext_ior >= 1, and eta == 1 (no interface) only with spec_trans == 0; anything else is
 * BSDFD_EINVAL.  (Mitsuba's `specular` is eta = 2 / (1 - sqrt(0.08 specular)) - 1.)
 * Directions are in the local shading frame, x the tangent the anisotropy refers to; BOTH sides of the surface are served
 * (wi.z < 0: from inside, where only the two specular lobes exist, and nothing at all without transmission).  Per row:
 *   eval           rgb_out [N,3] = f(wi, wo) |cos theta_o| * tint, 0 where wi.z == 0 or wo.z == 0, where the half vector is
 *                  undefined (|wi + k wo| < 1e-6) and, per channel, where the value is not finite.
 *   sample_weight  the tail of the plugin's sample(), as bsdfd_dielectric_sample_weight: value = f |cos| * tint / pdf_sa (0 where
 *                  pdf_sa <= 0); pdf_out = pdf_sa where value.x < firefly_threshold, else 0; weight_out = value where pdf_out > 0.
 *   sample         u [N,3] in [0,1)^3: columns 0..1 are Mitsuba's sample2, column 2 its sample1, which picks the lobe on the
 *                  cumulative order diffuse, clearcoat, transmission, reflection (Mitsuba's components 0..3).  wo_out [N,3];
 *                  pdf_out [N] = what bsdfd_principled_pdf gives for (wi, wo_out), bit for bit; weight_out [N,3] (may be NULL) =
 *                  what bsdfd_principled_eval gives for that pair, divided by pdf_out.  A failed sample (a direction on the
 *                  wrong side for its lobe, wi.z == 0, from inside without transmission, pdf 0) is zeros in all three.
 *   pdf            the solid-angle density of that sampler at a given wo: the mixture of the four lobes.
 * Rows with active[i] == 0, when a mask is given (u8 [N] or NULL), get 0 in every output.  tint: 3 floats on the host or NULL
 * (white).  All four calls are stream-ordered, allocate nothing and do not synchronise; N = 0 is a no-op. */
typedef struct {
    float base_color[3];
    float roughness, anisotropic, metallic, spec_trans, eta, spec_tint, sheen, sheen_tint, flatness, clearcoat, clearcoat_gloss;
    int32_t reserved[2];
} bsdfd_principled;
int bsdfd_principled_eval(const bsdfd_principled* desc, const float* wi, const float* wo, int64_t N, const float* tint,
                          float* rgb_out, void* hip_stream);
int bsdfd_principled_sample_weight(const bsdfd_principled* desc, const float* wi, const float* wo, const float* pdf_sa,
                                   const unsigned char* active, int64_t N, const float* tint, float firefly_threshold,
                                   float* weight_out, float* pdf_out, void* hip_stream);
int bsdfd_principled_sample(const bsdfd_principled* desc, const float* wi, const float* u, const unsigned char* active, int64_t N,
                            const float* tint, float* wo_out, float* pdf_out, float* weight_out, void* hip_stream);
int bsdfd_principled_pdf(const bsdfd_principled* desc, const float* wi, const float* wo, const unsigned char* active, int64_t N,
                         float* pdf_out, void* hip_stream);

/* ---- the two analytic models for a MIXED-material wavefront (csrc/analytic_table.hip) ---------------------------------------
 * One launch serves every material, where the calls above take one launch per material on gathered slices: the analytic
 * counterpart of bsdfd_measured_table.  The rows stay in lane order with their material ids, as bsdfd_wf_primary writes them.
 * entries[m] serves material id m (zero-initialise it; it may grow at the end):
 *   kind    BSDFD_ANALYTIC_NONE ("no ground truth for this material"), _PRINCIPLED or _DIELECTRIC: which member of desc is read
 *   albedo  the material's own RGB factor, finite and >= 0 (the `albedo` every `mybsdf` ball of the reference's array scenes
 *           carries: rendering/bsdf_myresult.py:97,112): a row's effective tint is tint[c] * albedo[m][c], one fp32 product,
 *           used exactly where the single-material calls use tint.  (1, 1, 1) leaves the call's tint as it is.
 * 1 <= n_materials <= 65536, at least one entry with ground truth; a descriptor the single-material call would refuse, a kind
 * that is none of the three and a bad albedo are BSDFD_EINVAL, the message naming the entry.  What depends on a material alone is
 * derived here, once, by the code the single-material calls run per call, and copied to the current device; the entries are not
 * needed afterwards. */
#define BSDFD_ANALYTIC_NONE 0
#define BSDFD_ANALYTIC_PRINCIPLED 1
#define BSDFD_ANALYTIC_DIELECTRIC 2
typedef struct {
    int32_t kind;
    float albedo[3];
    union {
        bsdfd_principled principled;
        bsdfd_dielectric dielectric;
    } desc;
} bsdfd_analytic_entry;
typedef struct bsdfd_analytic_table_ctx* bsdfd_analytic_table;
int  bsdfd_analytic_table_create(const bsdfd_analytic_entry* entries, int32_t n_materials, bsdfd_analytic_table* out);
void bsdfd_analytic_table_destroy(bsdfd_analytic_table t);
/* The four calls of a whole wavefront in LANE order, one launch each; argument lists as the bsdfd_measured_*_table calls (u is
 * [N,3], as for the single-material analytic samplers).  Row i with 0 <= material_id[i] < n_materials (the full 64-bit value)
 * and an entry with ground truth gets what the single-material call of that entry writes for the row with the effective tint,
 * bit for bit (zeros where active[i] == 0 included); eval_table writes f_o from wo and, when wl and f_l are given (both or
 * neither), f_l from wl in the same launch.  Every other row (floor, miss, NONE slot, id out of range or negative) gets a quiet
 * NaN in every output, whatever its mask says — the "use the proxy" value bsdfd_wf_shade reads — except that sample_weight_table
 * passes pdf_out = pdf_sa through.  Stream-ordered, no allocation, no synchronisation; N = 0 is a no-op. */
int  bsdfd_analytic_eval_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                               const float* wl, int64_t N, const float* tint, float* f_o, float* f_l, void* hip_stream);
int  bsdfd_analytic_sample_weight_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi,
                                        const float* wo, const float* pdf_sa, const unsigned char* active, int64_t N,
                                        const float* tint, float firefly_threshold, float* weight_out, float* pdf_out,
                                        void* hip_stream);
int  bsdfd_analytic_sample_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* u,
                                 const unsigned char* active, int64_t N, const float* tint, float* wo_out, float* pdf_out,
                                 float* weight_out, void* hip_stream);
int  bsdfd_analytic_pdf_table(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                              const unsigned char* active, int64_t N, float* pdf_out, void* hip_stream);

/* ---- wavefront harness ------------------------------------
 * The reference renders through Mitsuba 3 (rendering/brdf_measured_disk.py:146-155: passes of
 * `mi.render(scene, spp=4, seed)`), whose integrator calls the plugin's sample()/pdf() once per
 * wavefront; rendering/utils/mitsuba_helper.py:59-127 restates the primary-ray generation and
 * :130-137 the power-heuristic MIS weight.  These two streaming kernels are the part of that loop
 * around the plugin calls for a minimal scene of the harness' own: pinhole camera, one analytic
 * sphere carrying the material, a lat-long environment map (y up), one bounce.  Path index inside a
 * tile of rows [row_begin, row_end): ((row - row_begin) * width + col) * spp + s; the RNG counter is
 * the global path index, so an image does not depend on the row split over GPUs. */
typedef struct bsdfd_wf_scene {
    float cam_origin[3], cam_right[3], cam_up[3], cam_forward[3]; /* orthonormal camera basis */
    float tan_half_fov;                                            /* of the horizontal field of view */
    int32_t width, height;                                         /* film size in pixels */
    float sphere_center[3];
    float sphere_radius;
    float albedo[3];                                               /* props["albedo"] of the plugin */
    int32_t env_width, env_height;                                 /* environment map [H,W,3] fp32 */
    /* array scenes (matpreview/disney_bsdf_array*.xml: 12 balls with one `mybsdf` material each over a
     * checkerboard floor): ball 0 is the sphere above, balls 1..n_extra_spheres follow; ball k carries
     * material k.  All zero = the single-ball scene. */
    int32_t n_extra_spheres;                                       /* 0..31 */
    float extra_spheres[31][4];                                    /* centre xyz, radius */
    int32_t has_plane;                                             /* diffuse checkerboard floor y = plane_y */
    float plane_y, checker_scale, checker_color0, checker_color1;
} bsdfd_wf_scene;

/* Primary rays of rows [row_begin,row_end), spp jittered samples per pixel, pass index `pass`:
 * wi [N,3] local incoming direction ((0,0,1) for rays that miss the sphere), wl [N,3] cosine-weighted
 * light-sample direction (local), nrm [N,3] world normal (0 for a miss), dir [N,3] world ray direction,
 * material [N] (or NULL): ball index = material index, n_balls for the floor (its reflectance is then
 * in the wi slot), n_balls + 1 for a miss — the ids bsdfd_bucket_by_material sorts. */
int bsdfd_wf_primary(const bsdfd_wf_scene* scene, int32_t row_begin, int32_t row_end, int32_t spp,
                     uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir,
                     int64_t* material, void* hip_stream);
/* One-bounce MIS estimate: wo/pdf_o from plugin sample(), pdf_l = plugin pdf(wi, wl);
 * f_o / f_l [N,3] = plugin eval(wi, wo) / eval(wi, wl) (f cos, albedo included) or both NULL: then the
 * proxy f cos = albedo * pdf is used; a NaN in a path's f_o / f_l entry selects the proxy for that path.  wi / material: the arrays of bsdfd_wf_primary, needed (non-NULL)
 * for scenes with a floor.  film [row_end-row_begin, width, 3] += mean over the spp samples. */
int bsdfd_wf_shade(const bsdfd_wf_scene* scene, const float* env, int32_t row_begin, int32_t row_end,
                   int32_t spp, const float* wo, const float* pdf_o, const float* wl, const float* pdf_l,
                   const float* nrm, const float* dir, const float* f_o, const float* f_l, const float* wi,
                   const int64_t* material, float* film, void* hip_stream);

/* ---- path tracing in the array scene: occlusion and further bounces (csrc/pathtrace.hip) ----------
 * The reference renders its array scenes with Mitsuba's `path` integrator at unbounded depth: balls shadow the floor and
 * each other, and every further vertex calls the plugin's sample() / pdf() again.  These three kernels keep a path's state
 * in lane-ordered arrays between those calls; a host loops  bucket -> sample/pdf [-> eval] -> bounce  over a shrinking
 * wavefront.  Only the environment emits (point emitters: the section below).  All three are stream-ordered, allocate
 * nothing and do not synchronise; N = 0 is a no-op.  Row p of a tile is the global path  path_offset + p
 * (= row_begin * width * spp + p for a film tile).
 *
 * bsdfd_wf_path_begin: from dir / nrm / material as bsdfd_wf_primary wrote them -> org [N,3] world position of the first
 * vertex (ball k: centre_k + r_k * nrm; floor: the ray/plane point; miss: 0), beta [N,3] = 1 (throughput), rad [N,3] =
 * env(dir) for a miss, 0 otherwise (radiance gathered so far). */
int bsdfd_wf_path_begin(const bsdfd_wf_scene* scene, const float* env, int64_t N, const float* dir, const float* nrm,
                        const int64_t* material, float* org, float* beta, float* rad, void* hip_stream);
/* One vertex of every live path (material <= n_balls).  In/out: org, nrm, wi, wl, material, beta, rad.  In: wo / pdf_o /
 * pdf_l (and f_o / f_l, both NULL or both given; NaN = proxy) of the sampler, as bsdfd_wf_shade takes them.
 *   ball vertex : rad += beta * (the two MIS strategies of bsdfd_wf_shade).  With `occlusion`, a light sample wl that meets
 *                 geometry adds nothing, and the BSDF sample wo (followed only if wo.z > 0 and pdf_o is positive and finite)
 *                 adds its environment term only if it escapes; if it hits and `last` is 0 the path moves there: org, nrm,
 *                 wi (local incoming direction, or the checker reflectance for a floor hit — as bsdfd_wf_primary), material,
 *                 beta *= f_o / pdf_o (proxy: albedo), and a fresh cosine-weighted wl (Philox key and counter of
 *                 bsdfd_wf_primary with counter word 3 = 0x57617665 + bounce + 1).  Without `occlusion` no ray is traced
 *                 and the path ends: bsdfd_wf_shade's estimate.
 *   floor vertex: the one cosine-sampled direction wl serves both purposes — rad += beta * reflectance * env unless
 *                 (`occlusion`) it hits a ball; then beta *= reflectance and the path moves there, or ends when `last`.
 * A path that ends gets material = n_balls + 1 (the "miss" id: the next bucketing sorts it behind the materials); such a
 * lane is skipped by later calls.  A ray skips the surface it starts on (known from `material`): no epsilon offset.
 * `bounce` is the 0-based depth of the vertices being shaded. */
int bsdfd_wf_bounce(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                    uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                    float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                    const float* pdf_l, const float* f_o, const float* f_l, void* hip_stream);
/* film [row_end-row_begin, width, 3] += mean over the spp samples of rad [N,3] (bsdfd_wf_shade's accumulation order). */
int bsdfd_wf_resolve(const bsdfd_wf_scene* scene, int32_t row_begin, int32_t row_end, int32_t spp, const float* rad,
                     float* film, void* hip_stream);

/* ---- point emitters in the array scene (csrc/pathlights.hip) ---------------------------------------
 * Five of the reference's array scenes are lit by a Mitsuba `point` emitter (matpreview/disney_bsdf_array*_pointlight*.xml).
 * Every vertex takes ONE emitter sample, the emitter chosen uniformly among the n_e = n_lights + has_env emitters as
 * Mitsuba's sample_emitter_direction does:  pick = (u0 * n_e) >> 32  with u0 the first word of
 * philox4x32(key = seed, counter = (global path index lo, hi, pass, 0x4C697465 + bounce));  pick == n_lights is the
 * environment.  A host with lights runs, per depth,  sample_emitter -> bucket -> sample/pdf [-> eval] -> bounce_lit  in place
 * of  bucket -> sample/pdf [-> eval] -> bounce.  Both calls are stream-ordered, allocate nothing and do not synchronise; N = 0
 * is a no-op; a lane whose path has ended (material outside 0..n_balls) is not read into anything and not a byte of its
 * wl, lsel, emit or state moves. */
#define BSDFD_WF_MAX_LIGHTS 8
typedef struct bsdfd_wf_lights {
    int32_t n_lights;            /* 1..8 point emitters */
    int32_t has_env;             /* the environment map emits too and counts as one more emitter */
    float position[8][3];        /* world, y up like the rest of bsdfd_wf_scene */
    float intensity[8][3];       /* radiant intensity per channel (Mitsuba `point`: radiance f cos * I / d^2) */
} bsdfd_wf_lights;               /* 200 bytes */

/* The emitter sample of the vertices at depth `bounce` (org, nrm, wi, material as bsdfd_wf_path_begin / bsdfd_wf_bounce left
 * them) -> lsel [N] (the picked point emitter, -1 for the environment), emit [N,3], and wl [N,3] in/out:
 *   environment picked   : wl stays the cosine sample bsdfd_wf_primary / bsdfd_wf_bounce wrote; emit = 0.
 *   point k, ball vertex : wl = the local direction to the light in the vertex' frame (the sampler's pdf() and the evaluator
 *                          are asked about it next); emit = n_e * I_k / d^2, 0 where wl.z <= 0 and, with `occlusion`, where the
 *                          ray towards the light meets another surface before it (the vertex' own surface is skipped by id).
 *   point k, floor vertex: wl stays (the path continues along it); emit = n_e * (reflectance / pi) * cos * I_k / d^2, the whole
 *                          term, shadowed the same way. */
int bsdfd_wf_sample_emitter(const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                            uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                            const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit, void* hip_stream);
/* bsdfd_wf_bounce for vertices whose emitter sample is lsel / emit.  The path moves on exactly as there.  The estimate:
 *   ball vertex : a picked point adds emit * f cos(wl) (f_l, or the proxy albedo * pdf_l; a delta light has no MIS weight);
 *                 a picked environment adds bsdfd_wf_bounce's light term with the density (wl.z / pi) / n_e.  A BSDF sample that
 *                 escapes adds the environment weighted against (wo.z / pi) / n_e if has_env, else nothing.
 *   floor vertex: the environment along wl at full weight if has_env and the ray escapes, plus emit. */
int bsdfd_wf_bounce_lit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, void* hip_stream);

/* ---- importance sampling of the environment map in the array scene (csrc/pathenv.hip) ---------------
 * Four of the reference's array scenes (matpreview/disney_bsdf_array{0,1}_envmap.xml, disney_bsdf_array2_spherical_envmap.xml,
 * scene_measured.xml) are lit by a Mitsuba `envmap` emitter, whose sample_direction / pdf_direction draw directions in
 * proportion to the map's luminance (a bilinear Hierarchical2D over luminance x sin theta).  The distribution here is piecewise
 * constant over the unit square of the lookup's own parameterisation,  u = atan2(x, -z) / 2pi (wrapped),  v = theta / pi,  cell
 * (j, i) = [i/W, (i+1)/W) x [j/H, (j+1)/H), built by the host from the 3x3 maximum of the texel luminances (so that the density is
 * positive wherever the bilinear lookup is) times the row's solid angle; it is NOT pinned to Mitsuba's.  All tables are fp32 on
 * the device; first entries of the CDFs are 0, last entries 1.  A cell is the one with cdf[k] <= t < cdf[k+1] (a cell of zero
 * width is never chosen); inside it both coordinates are uniform with offset (t - cdf[k]) / (cdf[k+1] - cdf[k]).  The density of a
 * direction per solid angle is  pdf_uv[cell] / (2 pi^2 max(sin theta, 1e-6)). */
typedef struct bsdfd_env_dist {
    const float* marginal;       /* [height + 1]         CDF over the rows */
    const float* conditional;    /* [height][width + 1]  CDF over the columns of each row */
    const float* pdf_uv;         /* [height][width]      density per unit area of the (u, v) square: averages to 1 */
    int32_t width, height;
} bsdfd_env_dist;

/* Row-level access (Mitsuba envmap: sample_direction / pdf_direction).  u [N,2] in [0,1): u[.,0] picks the row, u[.,1] the
 * column -> dir [N,3] (world, y up, unit) and its density pdf [N];  dir [N,3] unit -> pdf [N].  N = 0 is a no-op. */
int bsdfd_env_sample(const bsdfd_env_dist* dist, int64_t N, const float* u, float* dir, float* pdf, void* hip_stream);
int bsdfd_env_pdf(const bsdfd_env_dist* dist, int64_t N, const float* dir, float* pdf, void* hip_stream);

/* The environment's emitter sample of the vertices at depth `bounce`, drawn from `dist` (of the environment map's size) instead
 * of the cosine-weighted wl: runs after bsdfd_wf_sample_emitter (if there are lights) and before the bucketing.  For every live
 * vertex with lsel == -1 — lsel NULL: every live vertex, and n_e must be 1 — a direction d from
 * philox4x32(key = seed, counter = (global path index lo, hi, pass, 0x456E766D + bounce)): word 0 >> 8 picks the row, word 1 >> 8
 * the column (times 2^-24).  With p_l = pdf(d) / n_e, E the bilinear lookup and V the visibility (`occlusion`: no surface along d;
 * the vertex' own is skipped by id):
 *   ball vertex : wl = d in the vertex' frame (it may be below the horizon), lpdf = p_l, emit = E V / p_l, 0 where wl.z <= 0.
 *   floor vertex: wl stays (the cosine direction is the floor's BSDF sample and the way on), lpdf = p_l,
 *                 emit = mis(p_l, cos / pi) (reflectance / pi) cos E V / p_l, the finished term.
 * Vertices that picked a point light, and ended paths: not a byte of their wl, lpdf or emit moves. */
int bsdfd_wf_sample_env(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int32_t n_e, int32_t bounce,
                        int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                        const float* nrm, const float* wi, const int64_t* material, const int32_t* lsel, float* wl, float* lpdf,
                        float* emit, void* hip_stream);
/* bsdfd_wf_bounce_lit for vertices whose environment sample is bsdfd_wf_sample_env's.  `lights` and `lsel` are both NULL (the
 * environment is the only emitter) or both given (has_env must be set; n_e = n_lights + 1).  The path moves on exactly as in
 * bsdfd_wf_bounce.  The estimate differs from bsdfd_wf_bounce_lit's in three places:
 *   ball vertex, environment picked: adds mis(lpdf, pdf_l) * emit * f cos(wl) (f_l, or the proxy albedo * pdf_l);
 *   a BSDF sample wo that escapes  : weighted mis(pdf_o, pdf(d) / n_e);
 *   floor vertex                   : its escaping cosine sample is weighted mis(cos / pi, pdf(d) / n_e), and emit is added. */
int bsdfd_wf_bounce_env(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                        uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                        float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                        const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                        const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, void* hip_stream);

/* ---- Russian roulette in the array scene (csrc/bounce.hip) ------------------------------------------
 * Six of the reference's array scenes are rendered by Mitsuba's `path` integrator at max_depth = -1 with its default rr_depth = 5.
 * Mitsuba's rule (the `path` integrator's `rr_depth` parameter): once  depth >= rr_depth  — depth = the surface vertices processed so far, here bounce + 1 —
 * a path continues with probability  q = min(max over the channels of throughput * eta^2, 0.95)  and its throughput is divided
 * by q.  This is that rule restated (eta = 1; the throughput is the one after this vertex, beta * f / pdf); it is NOT pinned to
 * Mitsuba's random stream or images.
 *
 * bsdfd_wf_bounce_rr is bsdfd_wf_bounce, bsdfd_wf_bounce_lit or bsdfd_wf_bounce_env with that rule inside the kernel:
 *   dist == NULL, lights == NULL : bsdfd_wf_bounce     (lsel, emit, lpdf are not read)
 *   dist == NULL, lights given   : bsdfd_wf_bounce_lit (lpdf is not read)
 *   dist given                   : bsdfd_wf_bounce_env
 * and every check of the chosen call applies; rr_depth >= 1.  While bounce + 1 < rr_depth, and whenever `last` is set, every
 * array is written exactly as by that call and no variate is drawn.  From then on a path that would continue draws
 * u = (word 0 >> 8) * 2^-24  of  philox4x32(key = seed, counter = (global path index lo, hi, pass, 0x526F756C + bounce))  and
 * continues iff q is a positive number and u < q, with beta *= (f_o / pdf_o) / q; otherwise it ends like a path that escaped:
 * material = n_balls + 1, nothing else written.  rad does not depend on the roulette, nor do org, nrm, wi, wl, material of a
 * path that survives. */
int bsdfd_wf_bounce_rr(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                       uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                       float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                       const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                       const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                       void* hip_stream);

/* ---- The per-depth calls of the array scene over a live-lane list (csrc/bucket.hip, bounce.hip, pathlights.hip, pathenv.hip,
 * measured_table.hip, analytic_table.hip) ----------------------------------------------------------------------------
 * A deep path tracer serves a few hundred lanes of a wavefront of a million; the calls above are launched over all N.  These are
 * their list forms: `rows` (int64 [n_rows], device) names the lanes to serve, the arrays keep their N rows and their lane order,
 * and thread t works on lane rows[t] exactly as the full-width call works on that lane — a lane's Philox counters are keyed by
 * path_offset + lane, never by the thread — so every listed lane gets the full-width call's result bit for bit.  For each of them:
 *   - the entries of `rows` are distinct and in [0, N);  0 <= n_rows <= N;
 *   - a row that is not listed keeps every byte of every array;
 *   - n_rows == 0 is a no-op (rows may then be NULL); otherwise every check of the full-width sibling applies.
 *
 * bsdfd_bucket_rows is bsdfd_bucket_by_material (n_materials <= 64) over the rows of a list: a row's id is
 * material_id[rows[r]] and perm receives rows[r], so perm holds LANE numbers, bucket by bucket, stable in list order.  Rows whose id
 * is outside [0, n_materials) are left out; the kept rows fill perm[0 .. sum(counts)), the rest of perm is unspecified.  The
 * workspace is bsdfd_bucket_workspace_bytes(n_rows, n_materials).  Allocates nothing, does not synchronise; n_rows == 0 only
 * zeroes counts.  (The front of the permutation a path tracer gets by leaving its "ended" id out of range is its next list.)
 *
 * bsdfd_wf_bounce_rows takes bsdfd_wf_bounce_rr's arguments and selects the call as it does; rr_depth == 0 means no roulette
 * (bsdfd_wf_bounce, _lit or _env), rr_depth >= 1 is bsdfd_wf_bounce_rr.  bsdfd_wf_sample_emitter_rows and bsdfd_wf_sample_env_rows
 * are bsdfd_wf_sample_emitter and bsdfd_wf_sample_env.  bsdfd_measured_eval_table_rows and bsdfd_analytic_eval_table_rows are the
 * two tables' eval(): f_o / f_l are written at the listed rows only, NaN where a listed row has no ground truth. */
int bsdfd_bucket_rows(const int64_t* material_id, const int64_t* rows, int64_t n_rows, int32_t n_materials, int64_t* perm,
                      int64_t* counts, void* workspace, int64_t workspace_bytes, void* hip_stream);
int bsdfd_wf_bounce_rows(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                         uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                         float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                         const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                         const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                         const int64_t* rows, int64_t n_rows, void* hip_stream);
int bsdfd_wf_sample_emitter_rows(const bsdfd_wf_scene* scene, const bsdfd_wf_lights* lights, int32_t bounce, int32_t occlusion,
                                 uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org, const float* nrm,
                                 const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit,
                                 const int64_t* rows, int64_t n_rows, void* hip_stream);
int bsdfd_wf_sample_env_rows(const bsdfd_wf_scene* scene, const float* env, const bsdfd_env_dist* dist, int32_t n_e, int32_t bounce,
                             int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                             const float* nrm, const float* wi, const int64_t* material, const int32_t* lsel, float* wl, float* lpdf,
                             float* emit, const int64_t* rows, int64_t n_rows, void* hip_stream);
int bsdfd_measured_eval_table_rows(bsdfd_measured_table t, const int64_t* material_id, const float* wi, const float* wo,
                                   const float* wl, int64_t N, const float* tint, float* f_o, float* f_l, const int64_t* rows,
                                   int64_t n_rows, void* hip_stream);
int bsdfd_analytic_eval_table_rows(bsdfd_analytic_table t, const int64_t* material_id, const float* wi, const float* wo,
                                   const float* wl, int64_t N, const float* tint, float* f_o, float* f_l, const int64_t* rows,
                                   int64_t n_rows, void* hip_stream);

/* ---- transmission through the balls of the array scene (no new ABI version: three more entry points) ----
 *
 * bsdfd_wf_bounce_transmit is the bounce with one rule changed.  Under occlusion a usable BSDF sample (pdf_o > 0) BELOW the surface
 * (wo.z < 0) at a vertex with ground truth (f_o not NaN) is followed into the ball instead of ending the path, if f_o / pdf_o is
 * positive in some channel: the next vertex is the far side of the SAME ball, at t = -2 (x - c) . d along the ray, written like any
 * other vertex — nrm stays the outward normal, so wi.z < 0 says "arrived from inside" — with beta *= f_o / pdf_o.  Nothing else
 * is intersected inside a ball: the caller guarantees that the balls are pairwise disjoint and above the plane.  Without ground
 * truth, or with f_o == 0 in every channel, such a sample ends the path as in the other bounces; a sample with wo.z > 0 leaves the
 * surface outward and is traced against everything but its own ball, whichever side wi is on.  It takes bsdfd_wf_bounce_rows'
 * arguments and selects the emitters as it does; rr_depth == 0 means no roulette; rows == NULL with n_rows == 0 serves every lane,
 * anything else is a list under the list contract above.  f_o is required.
 *
 * bsdfd_wf_sample_inside / _rows is the sampler's answer for the vertices inside a ball.  A lane with 0 <= material[p] <
 * n_materials of the table and wi.z < 0 gets, from its material's own importance sampler,
 *     wo[p], pdf_o[p] = sample(wi[p], u0, u1, u2)        pdf_l[p] = pdf(wi[p], wl[p])
 * bit for bit what bsdfd_analytic_sample_table / _pdf_table return for that row and those variates, which are
 *     u_k = (word k >> 8) * 2^-24  of  philox4x32(key = seed, counter = (path lo, path hi, pass, "Insd" + bounce)),
 * path = path_offset + p — except that pdf_o[p] = 0 where that sample's weight is 0 in every channel (the dielectric's wo on the
 * wrong side for the lobe that drew it): the bounce weights a sample with f(wi, wo) / pdf_o of the pair, which is not 0 there.
 * A record of kind BSDFD_ANALYTIC_NONE gets zeros in all three.  Either ends the path at the bounce.  Every
 * other lane keeps every byte.  The checks and the list contract are those of bsdfd_analytic_eval_table_rows. */
int bsdfd_wf_bounce_transmit(const bsdfd_wf_scene* scene, const float* env, int32_t bounce, int32_t last, int32_t occlusion,
                             uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm, float* wi,
                             float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                             const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                             const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                             const int64_t* rows, int64_t n_rows, void* hip_stream);
int bsdfd_wf_sample_inside(bsdfd_analytic_table t, int32_t bounce, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N,
                           const int64_t* material, const float* wi, const float* wl, float* wo, float* pdf_o, float* pdf_l,
                           void* hip_stream);
int bsdfd_wf_sample_inside_rows(bsdfd_analytic_table t, int32_t bounce, uint64_t seed, uint64_t pass, uint64_t path_offset,
                                int64_t N, const int64_t* material, const float* wi, const float* wl, float* wo, float* pdf_o,
                                float* pdf_l, const int64_t* rows, int64_t n_rows, void* hip_stream);

/* ---- ray casting on instanced triangle meshes (no new ABI version: six more entry points) ----
 *
 * The array scenes' real geometry: a few triangle meshes, instanced under affine transforms.  csrc/mesh.hip, csrc/mesh_dev.h.
 *
 * bsdfd_mesh_bvh_build is a pure host function (no HIP call): a binary BVH over the nt triangles of (positions [nv,3], indices
 * [nt,3]), split at the median of the triangle centroids along the longest axis of the centroid box, a leaf at <= 4 triangles,
 * stored THREADED: nodes in depth-first order, an inner node's left child is the next node, and every node carries `skip`, the
 * index of the first node behind its subtree (the root's is *n_nodes) — a traversal needs no stack.  A leaf has
 * tris = first * 8 + count into the reordered triangle array, order_out[first + k] being that triangle's index in `indices`; an
 * inner node has tris = 0.  node_cap >= 2 * nt - 1 always suffices; order_out is [nt].  nt must be in [1, 2^27]; an index >= nv
 * or a non-finite vertex is refused. */
typedef struct bsdfd_mesh_node {
    float lo[3], hi[3];
    int32_t skip;
    int32_t tris;
} bsdfd_mesh_node; /* 32 bytes */
int bsdfd_mesh_bvh_build(const float* positions, int64_t nv, const uint32_t* indices, int64_t nt, bsdfd_mesh_node* nodes_out,
                         int64_t node_cap, int32_t* order_out, int64_t* n_nodes);

/* A scene: each mesh is uploaded once with its BVH (host pointers; normals [nv,3] and uvs [nv,2] may be NULL), then up to
 * BSDFD_MESH_MAX_INSTANCES instances, each a mesh index, a 3x4 row-major affine to_world (inverted on the host in fp64; a singular
 * one is refused, a mirroring one is fine) and a surface record: BSDFD_MESH_MATERIAL (lane `material` of the material table),
 * BSDFD_MESH_DIFFUSE (constant reflectance color0) or BSDFD_MESH_CHECKER (color0 / color1 by the parity of
 * floor(2 uscale u) + floor(2 vscale v) over the mesh's own uv, odd = color1; the mesh must have uvs).  Created on the current
 * device; synchronises. */
#define BSDFD_MESH_MAX_INSTANCES 64
#define BSDFD_MESH_MATERIAL 0
#define BSDFD_MESH_DIFFUSE 1
#define BSDFD_MESH_CHECKER 2
typedef struct bsdfd_mesh_desc {
    const float* positions;
    const uint32_t* indices;
    const float* normals;
    const float* uvs;
    int64_t n_vertices, n_triangles;
} bsdfd_mesh_desc;
typedef struct bsdfd_mesh_instance {
    int32_t mesh, surface, material, reserved;
    float color0, color1, uscale, vscale;
    float to_world[12];
} bsdfd_mesh_instance;
typedef struct bsdfd_mesh_scene_ctx* bsdfd_mesh_scene;
int bsdfd_mesh_scene_create(const bsdfd_mesh_desc* meshes, int32_t n_meshes, const bsdfd_mesh_instance* instances,
                            int32_t n_instances, bsdfd_mesh_scene* scene);
void bsdfd_mesh_scene_destroy(bsdfd_mesh_scene scene);

/* One ray per lane, org + t dir with dir of any length (t is the parameter, not a distance).  All arrays are device pointers.
 *
 * bsdfd_mesh_intersect: the closest hit with 0 < t <= tmax[p] (tmax NULL: unbounded), the primitive skip[p] = (instance, triangle)
 * excepted — the primitive a secondary ray starts on; no epsilon; NULL or (-1, -1): none.  t [N], prim int32 [N,2] = (instance,
 * the file's triangle index), bary [N,2] = the weights of the triangle's second and third vertex.  A miss writes t = 3.0e38,
 * prim = (-1, -1), bary = 0.  Smaller t wins; on equal t the smaller (instance, triangle).  The ray/triangle test is watertight
 * at shared edges and vertices (Woop, Benthin, Wald 2013); a ray in a triangle's plane does not hit it.
 *
 * bsdfd_mesh_occluded: out[p] = 1 where bsdfd_mesh_intersect would report a hit, else 0 (uint8 [N]), leaving at the first one.
 *
 * bsdfd_mesh_primary is bsdfd_wf_primary on the mesh scene: the camera, film, tile and n_materials = 1 + n_extra_spheres of
 * `wf_scene` (its spheres and plane are not looked at), the same Philox key and counters, film position, ray and light sample, so
 * dir and wl are bsdfd_wf_primary's.  nrm is the shading normal: the barycentric mix of the vertex normals through the inverse
 * transpose, normalised, flipped into the hemisphere of the geometric normal (itself faced towards the ray); the geometric normal
 * where the mesh has no normals or where -dir . nrm <= 0.  A material instance writes wi in the onb(nrm) frame and its lane;
 * a diffuse one writes its reflectance in all three wi slots and n_materials; a miss writes a zero normal and n_materials + 1.
 * An instance whose material is >= n_materials is refused.
 *
 * All three: N (or the tile) == 0 is a no-op; nothing behind the N-th lane is written; no allocation, no synchronisation. */
int bsdfd_mesh_intersect(bsdfd_mesh_scene scene, int64_t N, const float* org, const float* dir, const float* tmax,
                         const int32_t* skip, float* t, int32_t* prim, float* bary, void* hip_stream);
int bsdfd_mesh_occluded(bsdfd_mesh_scene scene, int64_t N, const float* org, const float* dir, const float* tmax,
                        const int32_t* skip, uint8_t* out, void* hip_stream);
int bsdfd_mesh_primary(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, int32_t row_begin, int32_t row_end, int32_t spp,
                       uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material,
                       void* hip_stream);

/* ---- the path tracer of the array scene on the mesh scene (no new ABI version: three more entry points) ----
 *
 * The per-depth calls of the array scene (bsdfd_wf_path_begin / _sample_emitter / _bounce*) with the triangle meshes as their
 * geometry.  The path state gains one array, prim int32 [N,2]: the (instance, triangle) a path's vertex lies on.  A ray that
 * leaves the vertex skips that primitive — no epsilon, bsdfd_mesh_intersect's rule — and nothing else.  `wf_scene` gives the
 * camera, the film, the proxy albedo, the environment's size and n_materials = 1 + n_extra_spheres; its spheres and plane are not
 * looked at.  The diffuse and checker instances take the part of the floor (id n_materials, reflectance in the wi slots); the
 * miss id is n_materials + 1.  An instance whose material is >= n_materials is refused.
 *
 * bsdfd_mesh_path_primary is bsdfd_mesh_primary (the same kernel: wi, wl, nrm, dir and material are its bits; one walk per lane)
 * and, in a second small launch on the same stream, bsdfd_wf_path_begin: for a hit org = cam + t dir, prim = the hit, rad = 0; for a miss org = 0, prim = (-1, -1) and rad = the environment
 * along dir (env [env_height, env_width, 3]); beta = 1 on every lane.
 *
 * bsdfd_mesh_sample_emitter is bsdfd_wf_sample_emitter: the shadow ray to the picked point light is an any-hit walk bounded by the
 * distance to the light.  prim is read only.
 *
 * bsdfd_mesh_bounce is bsdfd_wf_bounce_rr's argument list, with lights, lsel and emit NULL where only the environment emits (the
 * cosine light strategy) and rr_depth = 0 for no roulette.  lpdf and dist must be NULL (BSDFD_EINVAL): the environment is not
 * importance-sampled on meshes yet; nor is there transmission (the live-lane list: below).  The estimate, the MIS weights, the roulette
 * and the Philox counters are those of the sphere kernels (one body, csrc/bounce_dev.h); the closest hit is one walk per lane,
 * the cosine strategy's shadow ray one unbounded any-hit walk, and the next vertex is written as bsdfd_mesh_primary writes the
 * first: org = x + t d, the shading-normal rule for a ray of direction d, prim = the hit.  A sample above the shading normal but
 * below the triangle's plane is followed into the mesh (no geometric-normal test), and a surface is shaded alike from both
 * sides.  A path that has ended keeps every byte of its state, prim included.
 *
 * All three: a null scene, a negative or too-large N and null arrays are refused before any device work; N (or the tile) == 0 is
 * a no-op; nothing behind the N-th lane is written; no allocation, no synchronisation. */
int bsdfd_mesh_path_primary(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, int32_t row_begin, int32_t row_end, int32_t spp,
                            uint64_t seed, uint64_t pass, float* wi, float* wl, float* nrm, float* dir, int64_t* material,
                            const float* env, float* org, int32_t* prim, float* beta, float* rad, void* hip_stream);
int bsdfd_mesh_sample_emitter(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const bsdfd_wf_lights* lights, int32_t bounce,
                              int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, const float* org,
                              const float* nrm, const float* wi, const int64_t* material, float* wl, int32_t* lsel, float* emit,
                              const int32_t* prim, void* hip_stream);
int bsdfd_mesh_bounce(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const float* env, int32_t bounce, int32_t last,
                      int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm,
                      float* wi, float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                      const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights, const int32_t* lsel,
                      const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth, int32_t* prim,
                      void* hip_stream);

/* ---- the same two per-depth calls over a live-lane list (no new ABI version: two more entry points) ----
 *
 * bsdfd_mesh_sample_emitter_rows and bsdfd_mesh_bounce_rows take their full-width sibling's arguments and, in front of the stream,
 * `rows` (int64 [n_rows], device) and n_rows, as bsdfd_wf_sample_emitter_rows and bsdfd_wf_bounce_rows do, under the contract of
 * those list forms: thread t serves lane rows[t] exactly as the full-width call serves that lane — prim is read and written at
 * rows[t], the Philox counters are keyed by path_offset + lane — so a listed lane gets the full-width call's result bit for bit;
 *   - the entries of `rows` are distinct and in [0, N) (an entry outside is skipped, not followed);  0 <= n_rows <= N;
 *   - a row that is not listed keeps every byte of every array, prim included;
 *   - n_rows == 0 is a no-op that returns BSDFD_OK whatever the pointers (rows may then be NULL); otherwise every check of the
 *     full-width sibling applies (lpdf and dist must be NULL here too).
 * A null scene, n_rows < 0, n_rows > N and rows == NULL with n_rows > 0 are refused before any device work.  The grid covers
 * n_rows threads, not N: a wave's two walks serve 64 listed lanes, where the full-width call's serve what is left alive among 64
 * neighbouring lanes.  Listed paths that have ended leave in front of the walks, as ended lanes do at full width. */
int bsdfd_mesh_sample_emitter_rows(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const bsdfd_wf_lights* lights,
                                   int32_t bounce, int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N,
                                   const float* org, const float* nrm, const float* wi, const int64_t* material, float* wl,
                                   int32_t* lsel, float* emit, const int32_t* prim, const int64_t* rows, int64_t n_rows,
                                   void* hip_stream);
int bsdfd_mesh_bounce_rows(bsdfd_mesh_scene scene, const bsdfd_wf_scene* wf_scene, const float* env, int32_t bounce, int32_t last,
                           int32_t occlusion, uint64_t seed, uint64_t pass, uint64_t path_offset, int64_t N, float* org, float* nrm,
                           float* wi, float* wl, int64_t* material, float* beta, float* rad, const float* wo, const float* pdf_o,
                           const float* pdf_l, const float* f_o, const float* f_l, const bsdfd_wf_lights* lights,
                           const int32_t* lsel, const float* emit, const float* lpdf, const bsdfd_env_dist* dist, int32_t rr_depth,
                           int32_t* prim, const int64_t* rows, int64_t n_rows, void* hip_stream);

const char* bsdfd_last_error(void);
const char* bsdfd_version(void);
/* BSDFD_ABI_VERSION the library was compiled with (see the top of this header). */
int32_t bsdfd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BSDFD_H */
