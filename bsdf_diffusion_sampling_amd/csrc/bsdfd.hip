// bsdfd.hip — MI355X (gfx950 / CDNA4) implementation of the neural-BSDF flow sampler on 16-QUERY TILES: the kernel, its weight image and
// its instantiation table (flow_kernels.h).  The handle, the launch routine and the entry points of include/bsdfd.h are in host.hip.
//
// One fused kernel per call evaluates, for every query, the whole hot path of
// fzy28/BSDF_diffusion_sampling (paths relative to the reference root):
//   positional encoding            rendering/utils/model.py:9-57
//   conditional base density       model.py:374-398 (disk), :277-317 (spherical)
//   velocity net, T Euler steps    model.py:479-501 / :422-446 / :449-477
//   2x2 Jacobian determinant       rendering/utils/mlp_brdf_sampling.py:17-51,:69-103,:106-181
//   domain warps and guards        rendering/brdf_measured_{disk,spherical}.py, bsdf_myresult.py
//
// Mapping to the hardware (DESIGN.md has the long version):
//   * a wave64 owns a tile of 16 queries; lane = (g = lane>>4, q = lane&15) holds, for
//     query q, hidden units {16m + 4g + r}.  That is exactly the C/D layout of the
//     16x16 MFMA shapes, and — because the K index of a contraction may be permuted
//     freely as long as A and B agree — also the B-operand layout of the NEXT layer:
//     the weights are pre-permuted on the host so activations never leave registers
//     between layers (no LDS round trip, no cross-lane traffic).
//   * the layer contraction is D[unit, query] = sum_k W[unit, k] * H[k, query]; the three
//     vectors that flow through every layer (activation h and the two Jacobian tangents
//     t0 = dh/dx0, t1 = dh/dx1 — forward-mode equivalent of the reference's two
//     backward() calls) share each weight fragment.
//   * the conditioning part of layer 1 (W1[:, PE(omega_i)]) is constant across the T
//     steps: it is computed once per query and used as the C-in accumulator of the
//     per-step layer-1 MFMA.
//   * weights live in LDS as ready-made MFMA A-fragments (one ds_read_b128 per use).
//   * the 2x2 Jacobian of the reference's two nets (disk 32x3, spherical 32x4) is formed by MEETING IN THE MIDDLE: the host
//     also packs the output-side folded matrices G_j = W_L^T diag(Wout[j, :]); per step two tangent layers' worth of hi/lo
//     splits, scalings and MFMAs are replaced by one fp32 2x2 bilinear form and a 5-swap cross-lane reduction (blocks
//     "MIM" / "MIMS" in the Euler step; other depths / widths run forward-mode tangents).
//   * a sample launch can write, and a pdf launch read, the per-query context (what depends on wi alone): bsdfd_opts.
//   * precision of the contractions: exact fp32 MFMA (16x16x4), or fp16 MFMA (16x16x32)
//     with hi+lo operand splitting (3 products, fp32 accumulate), or plain fp16.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "flow_dev.h"
#include "flow_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------
// The fused flow kernel.
//   DOMAIN : BSDFD_DOMAIN_*            NM : width/16 (2 or 4)
//   PREC   : BSDFD_PREC_F32 / SPLIT3 / F16      JAC : track the Jacobian determinant
// ---------------------------------------------------------------------------------------------
//   NH     : number of hidden layers when known at compile time (3 disk, 4 spherical; 32-wide nets: the
//            layer loop is then fully unrolled — no loop-carried register copies, `last` is static;
//            measured -3..4 % per Euler step), 0 = run-time p.n_hidden (any depth).
//   FUSED  : compiled with the two-phase OP_SAMPLE_PDF loop (its own instantiation: the loop costs the
//            single-op kernels 2-4 % when compiled into them)
// Waves per SIMD the register allocator is asked to make room for: 3 for the 32-wide nets (<= 168 VGPRs), 2 for the 64-wide.
// The one exception is the disk 32x3 split3 single-op kernel (the headline workload): asked for 2, the scheduler stops
// trading instruction-level parallelism for registers and still lands at 165 VGPRs = 3 waves/SIMD, 1.1 % faster than the
// 156-VGPR schedule it produces when asked for 3 (profiles/r03_ab/ab13).  tools/isa_mix.py --check-async (a CPU test) fails
// if a toolchain ever takes that kernel past 168 VGPRs, i.e. down to 2 waves/SIMD (which measured 4 % slower on the
// spherical kernel).
// The 64-wide kernels WITHOUT the Jacobian (the reflow teacher sampler, f16 / f32) need ~127 VGPRs in their loop = 4 waves/SIMD;
// the per-tile prologue they share with every other instantiation once grew past 128 and took the teacher from 4 to 3 waves
// (-4 %, round 4): they are pinned to 4.
// The output layer's A fragment holds rows {Wout_hi[0], Wout_hi[1], Wout_lo[0], Wout_lo[1]}.  Wout_lo = w - fp16(w) is at most 2^-11 |w|:
// for |w| < 2^-3 it would be an fp16 SUBNORMAL (absolute error 2^-25 whatever w is), a FIXED perturbation of the 64 weights that
// move the state directly — on materials with a narrow base density (cc_amber_citrine: pdf() at fresh directions) it was the whole
// distance between these kernels' p99 (1.05e-4) and the 32-query kernels' fp32 output layer (3.3e-5); round 6,
// tools/archive/r06_weight_repr_diag*.py.  The lo rows are separate output rows, so the host stores them x 2^11 (normal again,
// 11 good bits) and the sum e[o] + e[o + 2] becomes one fma with 2^-11: no instruction more.  (A/B knob: 1 = the old form.)
#ifndef BSDFD_WO_LO_SCALE
#define BSDFD_WO_LO_SCALE 2048
#endif
constexpr float kWoLoInv = 1.0f / (float)BSDFD_WO_LO_SCALE;
// (written without commas: __launch_bounds__ is a variadic macro)
#define BSDFD_MIN_WAVES \
    (NM != 2 ? ((!JAC && PREC != BSDFD_PREC_SPLIT3) ? 4 : 2) \
             : ((DOMAIN == BSDFD_DOMAIN_DISK && PREC == BSDFD_PREC_SPLIT3 && JAC && NH == 3 && !FUSED) ? 2 : 3))
template <int DOMAIN, int NM, int PREC, bool JAC, int NH, bool FUSED>
__global__ __launch_bounds__(NM == 2 ? 256 : 512, BSDFD_MIN_WAVES) void flow_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (p.clk) { clk_c0 = __builtin_readcyclecounter(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
    // this workgroup's share of the work: the whole batch, or one material's bucket
    const char* img = p.img;
    long long q_begin = 0, q_end = p.N;
    int blk = blockIdx.x, nblk = gridDim.x, cl = p.chunk_log2;
    int sidx = 0;
    if (p.nseg > 0) {
        for (int i = 1; i < p.nseg; ++i)
            if ((int)blockIdx.x >= p.seg[i].blk_begin) sidx = i;
        img = p.seg[sidx].img;
        q_begin = p.seg[sidx].q_begin;
        q_end = p.seg[sidx].q_end;
        blk = blockIdx.x - p.seg[sidx].blk_begin;
        nblk = p.seg[sidx].blk_end - p.seg[sidx].blk_begin;
        cl = p.seg[sidx].chunk_log2;
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(img);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (int i = threadIdx.x; i < p.L.total / 16; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();

    constexpr int KC = NM / 2;  // K chunks of 32 for the fp16 MFMA
    // FOLD_L1 (disk nets, fp16 MFMA paths): the layer-1 tangents are t_i = g (.) w_i with w_i = W1[:, i] CONSTANT, so
    // W2 t_i = (W2 diag(w_i)) g.  The host packs the two folded matrices (L.wf) and the first hidden layer splits ONE
    // vector (g) instead of two tangents: one hi/lo split and two multiplies per unit less, the same MFMA count.
    // Within-run A/B: -5.5 % (T = 8), -4.7 % (T = 4), -4.9 % (fused sample+pdf), accuracy unchanged (profiles/r02_ab/ab7).  The spherical analogue
    // (three folded matrices, d/dphi = cos(phi) F_sin g - sin(phi) F_cos g: +6 fp16 MFMAs, -2 fp32 MFMAs, one split less)
    // was built and measured at +-0.2 %: not kept.
    constexpr bool FOLD_L1 = JAC && NM == 2 && PREC != BSDFD_PREC_F32 && DOMAIN == BSDFD_DOMAIN_DISK && NH == 3;
    // MIM (same nets): the OUTPUT side of the Jacobian is folded as well and the two halves meet in the middle — see the
    // block in the Euler step.  History: with only the input side folded and every fragment register-resident the kernel
    // wanted 4 VGPRs more than 3 waves/SIMD allow; round 2 shipped a "PIN" arrangement (resident hi parts, the 4 folded lo
    // fragments fetched asynchronously per step: -3.7 %); MIM supersedes it (-5.7 % on top, profiles/r03_ab/).
    constexpr bool MIM = FOLD_L1 && KC == 1;
    // the spherical 26-32x4-2 nets: two regular tangent layers, then the same meeting in the middle (block "MIMS" below).
    // Round 4: also in the fused sample+pdf instantiation (-5.3 % kernel time, profiles/r04_ab/ab2*).  That kernel spills 16
    // VGPRs, all in the per-tile prologue and at the phase switch — none inside the Euler loop and none between an
    // asynchronous read and its wait, which is what tools/isa_mix.py --check-async verifies.
    constexpr bool MIMS = JAC && NM == 2 && PREC != BSDFD_PREC_F32 && DOMAIN == BSDFD_DOMAIN_SPHERICAL && NH == 4;
    // FOLDOUT (the depth-unrolled 64-wide instantiation, i.e. the reference's 64 x 6 nets; the run-time-depth kernels would carry
    // the 48 extra registers across loop iterations and spill): the OUTPUT side of the Jacobian folded as in MIM — the tangents stop in front of
    // the activation of the second-to-last hidden layer (U_i = their fp32 pre-activations there), R_j = G_j g_L with
    // G_j = W_L^T diag(Wout[j, :]) packed by the host, J_ji = sum_k R_j[k] g_{L-1}[k] U_i[k].  Per step two tangent vectors less to
    // scale and split (once at the second-to-last, once at the last layer) for one split of g_L, and 8 MFMAs fewer.
    // Within-run A/B (profiles/r04_ab/ab4_foldout_64wide.txt): -0.7 % (sample) / -1.8 % (pdf) on the 64 x 6 split3 kernel.
    constexpr bool FOLDOUT = JAC && NM == 4 && NH >= 2 && PREC != BSDFD_PREC_F32;
    // conditioning term of layer 1 on split-fp16 MFMAs: split3 builds of the DISK kernels (see the prologue).  Round 4,
    // all 77 shipped sets x 2048 queries (profiles/r04_ab/acc_sweep_*.json): the worst disk set's p99 pdf error goes from 2.4e-5
    // to 2.6e-5 (sample) and 2.3e-5 to 2.8e-5 (pdf) for -2.2 % kernel time at the plugin's T = 4 (-0.6 % at T = 8); the
    // spherical nets would gain 0.5 % and lose margin (golden chm_orange pdf p99 5.1e-5 -> 8.2e-5 of the 1e-4 contract): they
    // keep the exact-fp32 chains, as does every kernel in precision mode f32.
    // (the samples-only split3 kernel follows, so that it walks exactly the trajectory of the sampling kernel)
#ifndef BSDFD_SPLIT_PRO
#define BSDFD_SPLIT_PRO 1   // (A/B knob of tools/ab_build.sh; 0: the exact-fp32 chains everywhere)
#endif
    constexpr bool SPLIT_PRO = BSDFD_SPLIT_PRO && PREC == BSDFD_PREC_SPLIT3 && DOMAIN == BSDFD_DOMAIN_DISK;
    const int n_hidden = NH ? NH : p.n_hidden;
    const int lane_k = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;

    const float* Lwin = reinterpret_cast<const float*>(smem + p.L.win);
    const float* Lwc = reinterpret_cast<const float*>(smem + p.L.wc);
    const char* Lwh = smem + p.L.wh;
    const char* Lwh_lo = smem + p.L.wh_lo;
    const char* Lwo = smem + p.L.wo;
    const char* Lwf = smem + p.L.wf;
    const char* Lwf_lo = smem + p.L.wf_lo;
    const char* Lwg = smem + p.L.wg;
    const char* Lwg_lo = smem + p.L.wg_lo;
    const float* Lbw1 = reinterpret_cast<const float*>(smem + p.L.bw1);
    const float* Lbb1 = reinterpret_cast<const float*>(smem + p.L.bb1);
    const float* Lbw2 = reinterpret_cast<const float*>(smem + p.L.bw2);
    const float* Lbb2 = reinterpret_cast<const float*>(smem + p.L.bb2);
    const char* Lwcs = smem + p.L.wcs;
    const char* Lwcs_lo = smem + p.L.wcs_lo;
    const f32x4* Lwt0 = reinterpret_cast<const f32x4*>(smem + p.L.wt0);

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float win[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) win[m] = Lwin[m * 64 + lane_k];

    // layer-1 pre-activations of the constant tangents: d/dx0 (both domains), d/dx1 (disk)
    f32x4 zt0c[NM], zt1c[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        zt0c[m] = mfma4(win[m], (lane_k >> 4) == 0 ? 1.0f : 0.0f, zero4);
        zt1c[m] = mfma4(win[m], (lane_k >> 4) == 1 ? 1.0f : 0.0f, zero4);
    }

    const double invT_d = 1.0 / (double)p.T;
    const bool t_pow2 = (p.T & (p.T - 1)) == 0;
    const float invT = (float)invT_d;
    // OP_SAMPLE_PDF runs the flow twice per query (forward from the base draw, then reverse from wl) on ONE
    // evaluation of the per-query prologue (encoding, conditioning term, base net): the call pattern of a
    // renderer that asks sample() and pdf() for the same intersection
    const int nphase = FUSED ? 2 : 1;
    const bool reverse1 = (p.op == OP_PDF);  // single-op kernels: fixed for the launch
    const float cstep1 = reverse1 ? -invT : invT;
    const long long ntiles = (q_end - q_begin + 15) / 16;

    // Tile -> wave map: a workgroup takes CHUNKS of 2^cl x waves_per_block consecutive tiles, chunks
    // round-robin over the grid.  Consecutive tiles of a chunk stay on one CU (one XCD's L2), so the
    // 128-B lines of the query arrays are not fetched by two XCDs (a plain round-robin of single
    // tiles measured +35 % HBM reads), while the round-robin of chunks keeps the dynamic balance.
    // cl = 3 for large batches; the host lowers it for small ones so that every CU gets work
    // (64 Ki queries: 8-tile chunks would occupy 128 workgroups, 1-tile chunks 1024).
    const long long chunk = (long long)waves_per_block << cl;
    for (long long it = 0;; ++it) {
        const long long chunk_base = ((it >> cl) * nblk + blk) * chunk;
        if (chunk_base >= ntiles) break;
        const long long tile = chunk_base + (it & ((1 << cl) - 1)) * waves_per_block + wave;
        if (tile >= ntiles) continue;
        // The fused sample+pdf kernels (REMAT) re-derive the lane number per tile from an opaque copy, and the row of the
        // lane's query again at the phase switch and in the epilogue: otherwise everything computed from the lane number (LDS
        // addresses, half-wave selects) is hoisted out of the tile loop and the 64-bit row with every address derived from it is
        // carried across both Euler loops — the fused spherical split3 kernel spilled 16 VGPRs for that (round 4: 68 B of
        // scratch per lane).  The single-op kernels keep the plain values (same code as before).
        constexpr bool REMAT = FUSED;
        auto opaque = [](int x) -> int { if (REMAT) asm volatile("" : "+v"(x)); return x; };
        const int lane = opaque(lane_k);
        const int g = lane >> 4;
        const int q = lane & 15;
        const long long tile_q0 = q_begin + tile * 16;
        auto row_of = [&](int qq, bool& in_range) -> long long {
            const long long r = tile_q0 + qq;
            in_range = r < q_end;
            return in_range ? r : q_end - 1;
        };
        bool valid;
        const long long qi = row_of(q, valid);
        // row of the callers' arrays (bsdfd_opts.row_index; flow_dev.h, KParams) — re-read in the epilogue, not carried across the loop
        auto user_row = [&](long long r) -> long long { return p.row_index ? p.row_index[r] : r; };
        const long long qu = user_row(qi);

        // ---------------- inputs: condition (y0,y1) and, for pdf, the outgoing point -------------
        float y0 = 0.f, y1 = 0.f, wi_z = 1.0f;
        float xs0 = 0.f, xs1 = 0.f, wo_z = 1.0f, wo_sin = 1.0f;  // pdf: the point the reverse flow starts from
        bool wo_pole = false;                                    // spherical plugin pdf: the reference's sin(theta_o) guard fires
        float xi0 = 0.f, xi1 = 0.f;                              // sample: injected x0 (if any)
        // per-query context: a launch that is handed the context an earlier sample / pdf launch wrote for the SAME wi array
        // skips everything below that depends on wi alone (cart_to_spher(wi), encoding, conditioning term, base net)
        const bool have_ctx = !FUSED && p.ctx_in != nullptr;
        // plugin io: the direction whose pdf is asked -> start point of the reverse flow.  Disk: its xy; spherical: the arguments of
        // its two angles (evaluated below, one atan2f per lane, together with those of wi where both are needed)
        SphArgs ao = {};
        auto load_dir = [&](const float* dir, long long qi) {
            const float ox = dir[qi * 3 + 0], oy = dir[qi * 3 + 1], oz = dir[qi * 3 + 2];
            wo_z = oz;
            wo_sin = sqrtf(ox * ox + oy * oy);  // Mitsuba Frame3f::sin_theta
            if (DOMAIN == BSDFD_DOMAIN_DISK) {
                xs0 = ox; xs1 = oy;
            } else {
                ao = spher_args(ox, oy, oz);
                wo_pole = ao.ref_pole;
            }
        };
        auto angles_of = [&](const SphArgs& a, float& theta, float& phi) {   // two jobs: lanes g = 0, 2 theta, g = 1, 3 phi
            const float Y[2] = {a.s, a.y}, X[2] = {a.z, a.x};
            float r[2];
            atan2_by_lane<2>(Y, X, g, q, r);
            theta = r[0]; phi = r[1];
        };
        if (p.io == IO_OPERATOR) {
            const float2 c2 = reinterpret_cast<const float2*>(p.in_a)[qi];
            y0 = c2.x; y1 = c2.y;
            if (p.op == OP_PDF || p.in_b != nullptr) {
                const float2 b2 = reinterpret_cast<const float2*>(p.in_b)[qi];
                xs0 = b2.x; xs1 = b2.y;
            }
        } else {
            const float wx = p.in_a[qu * 3 + 0], wy = p.in_a[qu * 3 + 1], wz = p.in_a[qu * 3 + 2];
            wi_z = wz;
            if (DOMAIN == BSDFD_DOMAIN_DISK) {
                y0 = wx; y1 = wy;  // rendering/brdf_measured_disk.py:66-67
            }
            const bool need_o = !FUSED && p.op == OP_PDF;
            if (need_o) load_dir(p.in_b, qu);  // (the fused kernel loads wl at its phase switch: 4 registers less across phase 1)
            if (DOMAIN == BSDFD_DOMAIN_SPHERICAL) {  // cart_to_spher, rendering/brdf_measured_spherical.py:35-39 (wave-uniform branches)
                if (!have_ctx && need_o) {           // pdf(): four angles, one per lane of the query
                    const SphArgs ai = spher_args(wx, wy, wz);
                    const float Y[4] = {ai.s, ai.y, ao.s, ao.y}, X[4] = {ai.z, ai.x, ao.z, ao.x};
                    float r[4];
                    atan2_by_lane<4>(Y, X, g, q, r);
                    y0 = r[0]; y1 = r[1]; xs0 = r[2]; xs1 = r[3];
                } else if (!have_ctx) {
                    angles_of(spher_args(wx, wy, wz), y0, y1);
                } else if (need_o) {
                    angles_of(ao, xs0, xs1);
                }
            }
            if ((FUSED || p.op != OP_PDF) && p.in_b != nullptr) {  // injected base sample
                const float2 b2 = reinterpret_cast<const float2*>(p.in_b)[qu];
                if (FUSED) { xi0 = b2.x; xi1 = b2.y; } else { xs0 = b2.x; xs1 = b2.y; }
            }
        }

        f32x4 cacc[NM];
        f32x4 bo;
        // context slot of this tile: tiles of one bucket start 16 queries apart and a later bucket starts at or after the
        // end of the previous one, so floor(first query / 16) + bucket index is unique (bsdfd_context_bytes sizes for it)
        constexpr long long CTX_V4 = NM * 64 + 16;  // f32x4 per tile: cacc[NM] per lane + bo per query
        const long long ctx_slot = ((q_begin + tile * 16) >> 4) + p.seg_base + sidx;
        if (have_ctx) {
            const f32x4* c = reinterpret_cast<const f32x4*>(p.ctx_in) + ctx_slot * CTX_V4;
#pragma unroll
            for (int m = 0; m < NM; ++m) cacc[m] = c[m * 64 + lane];
            bo = c[NM * 64 + q];
        } else {
        // ---------------- positional encoding, distributed over the 4 lanes of a query -----------
        // lane g needs fn(2^b y_d) for dim d = g&1, fn = g>>1 ? cos : sin, b = 0..4: slab b of the K=4
        // contraction is [sin(2^b y0), sin(2^b y1), cos(2^b y0), cos(2^b y1)] = PE block b.  Lanes g and
        // g^2 (lane ^ 32) need the sin resp. cos of the SAME angles, so the sincos evaluations are
        // shared: the lower half-wave evaluates bands 0..2, the upper half bands 3..4, and three
        // v_permlane32_swap exchange the halves (3 sincosf per lane instead of 5).
        const float ysel = (g & 1) ? y1 : y0;
        float pe[PE_BANDS];
        {
            const bool upper = (g >> 1) != 0;  // lanes 32..63: want cos; evaluate bands 3, 4
            float sv[3], cv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) sincos_enc(ysel * (upper ? (float)(8 << k) : (float)(1 << k)), sv[k], cv[k]);
            // swap(vdst, src): vdst[32..63] <-> src[0..31].  vdst = upper-half sin of band 3+k, src =
            // lower-half cos of band k: afterwards the lower half finds sin(band 3+k) in `src` and
            // the upper half finds cos(band k) in `vdst`.
            unsigned got[3][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(sv[k]), __float_as_uint(cv[k]), false, false);
                got[k][0] = r[0];
                got[k][1] = r[1];
            }
            // lower half (sin): bands 0..2 own sv[k]; bands 3..4 arrived in r[1] of swaps 0, 1
            // upper half (cos): bands 3..4 own cv[0..1]; bands 0..2 arrived in r[0] of swaps 0..2
            pe[0] = upper ? __uint_as_float(got[0][0]) : sv[0];
            pe[1] = upper ? __uint_as_float(got[1][0]) : sv[1];
            pe[2] = upper ? __uint_as_float(got[2][0]) : sv[2];
            pe[3] = upper ? cv[0] : __uint_as_float(got[0][1]);
            pe[4] = upper ? cv[1] : __uint_as_float(got[1][1]);
        }
        const float yslab = g == 0 ? y0 : (g == 1 ? y1 : 0.0f);

        // conditioning part of layer 1 (constant across the Euler steps) and the base-density net
        // PE_3 -> 16 (SiLU) -> 4, once per query
        // c = W1[:, PE] PE(omega_i): exact fp32 MFMA chains (K = 4 slabs), except in the split3 disk kernels (SPLIT_PRO) — this
        // term enters z1 of all T steps, so its rounding error is systematic (the MFMA's fp16 adder tree is not an fp32 FMA
        // chain): see the accuracy sweep quoted at SPLIT_PRO.  The NM chains (and the base net's) are issued
        // slab-major so that consecutive MFMAs are independent (40-cycle dependent latency).
        // The base net (PE_3 -> 16 -> 4) also stays exact fp32: its outputs (loc, log sigma) are divided
        // by sigma ~ 1e-2 for peaked materials, so an fp16-split evaluation (measured) raised the p99
        // pdf error of aniso_miro_7 from 1.8e-5 to 2.9e-5.
        f32x4 bz = *reinterpret_cast<const f32x4*>(Lbb1 + lane * 4);
#pragma unroll
        for (int m = 0; m < NM; ++m) cacc[m] = zero4;
        if (SPLIT_PRO) {
            // split3: the lane's 5 encoded values and its raw coordinate ARE the 8 K-values (two zero pads) of one K = 32 B
            // fragment; the 22 x W conditioning contraction is 3 x NM fp16 MFMAs instead of 6 x NM exact-fp32 ones
            Frag ph, pl;
            const float p03[4] = {pe[0], pe[1], pe[2], pe[3]}, p47[4] = {pe[4], yslab, 0.0f, 0.0f};
            split_pack<true>(p03, ph.p[0], ph.p[1], pl.p[0], pl.p[1]);
            split_pack<true>(p47, ph.p[2], ph.p[3], pl.p[2], pl.p[3]);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const f16x8 ah = *reinterpret_cast<const f16x8*>(Lwcs + (m * 64 + lane) * 16);
                const f16x8 al = *reinterpret_cast<const f16x8*>(Lwcs_lo + (m * 64 + lane) * 16);
                cacc[m] = mfma16(ah, ph.v, zero4);
                cacc[m] = mfma16(ah, pl.v, cacc[m]);
                cacc[m] = mfma16(al, ph.v, cacc[m]);
            }
        }
#pragma unroll
        for (int s = 0; s < PE_SLABS; ++s) {
            const float b = s < PE_BANDS ? pe[s < PE_BANDS ? s : 0] : yslab;
            if (!SPLIT_PRO) {
#pragma unroll
                for (int m = 0; m < NM; ++m) cacc[m] = mfma4(Lwc[(m * PE_SLABS + s) * 64 + lane], b, cacc[m]);
            }
            if (s < BASE_PE_BANDS) bz = mfma4(Lbw1[s * 64 + lane], b, bz);
            if (s == PE_BANDS) bz = mfma4(Lbw1[BASE_PE_BANDS * 64 + lane], b, bz);
        }
        {
            const f32x4 w2 = *reinterpret_cast<const f32x4*>(Lbw2 + lane * 4);
            bo = *reinterpret_cast<const f32x4*>(Lbb2);
#pragma unroll
            for (int r = 0; r < 4; ++r) bo = mfma4(w2[r], silu(bz[r]), bo);
            // The result of an 8-pass MFMA may not be read by a VALU instruction for 10 wait states.  hipcc pads for that in
            // straight-line code but was caught (ROCm 7.2, round 4) leaving the padding out when the first reader sits in a
            // block reached by a TAKEN branch right behind the MFMA — here: the context store is skipped, softplus(bo[3]) / the
            // base density read bo two instructions later, and the kernel computed with the stale accumulator (the bias).  The
            // wait states are therefore spelled out; `_asmcheck.check_mfma_hazards_lines` verifies every MFMA of every
            // instantiation on the built assembly (a branch counted as one wait state) as part of `_lib.build()`.
            asm volatile("s_nop 7\n\ts_nop 1" : "+v"(bo));
        }
        if (!FUSED && p.ctx_out != nullptr) {  // one 1-KiB store per accumulator and wave, 16 B per query for bo
            f32x4* c = reinterpret_cast<f32x4*>(p.ctx_out) + ctx_slot * CTX_V4;
#pragma unroll
            for (int m = 0; m < NM; ++m) c[m * 64 + lane] = cacc[m];
            if (g == 0) c[NM * 64 + q] = bo;
        }
        }  // !have_ctx
        // bo = (loc0, loc1, ls0, ls1) disk | (loc, log_scale, mu, kappa_raw) spherical
        float kappa = 0.0f;
        if (DOMAIN == BSDFD_DOMAIN_SPHERICAL) kappa = softplus(bo[3]) + 1e-3f;

        int ph = 0;
    next_phase:  // FUSED: executed twice per tile (a goto, so that the single-op kernels contain no loop at all)
        {
        const int op = FUSED ? (ph ? OP_PDF : OP_SAMPLE) : p.op;
        const bool reverse = FUSED ? (ph != 0) : reverse1;
        const float cstep = FUSED ? (ph ? -invT : invT) : cstep1;
        float* const out_pdf = (FUSED && ph) ? p.out_pdf2 : p.out_pdf;
        // ---------------- initial state ------------------------------------------------------------
        if (FUSED && ph) {
            bool v2;
            load_dir(p.in_c, user_row(REMAT ? row_of(opaque(q), v2) : qi));
            if (DOMAIN == BSDFD_DOMAIN_SPHERICAL) angles_of(ao, xs0, xs1);
        }
        float x0 = (FUSED && !ph) ? xi0 : xs0, x1 = (FUSED && !ph) ? xi1 : xs1;
        if (op == OP_SAMPLE && p.in_b == nullptr) {  // draw x0 ~ D_base(. | omega_i) in-kernel
            const unsigned long long ctr = p.offset + (unsigned long long)(p.rng_index ? p.rng_index[qi] : qu);
            const unsigned k0 = (unsigned)p.seed, k1 = (unsigned)(p.seed >> 32);
            unsigned u[4];
            philox4x32(k0, k1, (unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0x476175u, u);  // "Gau"
            // Box-Muller on hardware transcendentals (v_log/v_sqrt/v_sin/v_cos; v_sin and v_cos take
            // revolutions, so sin(2 pi u) needs no range reduction).  The draw is statistically, never
            // bit-wise, comparable with torch's RNG, so ~1e-6 function error is immaterial here.
            const float rad = __builtin_amdgcn_sqrtf(-2.0f * kLn2 * __builtin_amdgcn_logf(u01_open(u[0])));
            const float rev = u01_open(u[1]);
            const float sn = __builtin_amdgcn_sinf(rev), cs = __builtin_amdgcn_cosf(rev);
            auto fexp0 = [](float x) -> float { return __builtin_amdgcn_exp2f(x * kLog2e); };
            if (DOMAIN == BSDFD_DOMAIN_DISK) {  // model.py:387-392
                x0 = bo[0] + rad * cs * fexp0(bo[2]);
                x1 = bo[1] + rad * sn * fexp0(bo[3]);
            } else {                            // model.py:298-307
                x0 = bo[0] + rad * cs * (fexp0(bo[1]) + 1e-3f);
                x1 = von_mises_sample(bo[2], kappa, k0, k1, (unsigned)ctr, (unsigned)(ctr >> 32), lane);
            }
        }

        // exp() below is v_exp_f32(x * log2 e): <= 2 ulp + |x| 2^-24 from the argument scaling, the same
        // conditioning the reference's own fp32 exp(logp) has; (x - loc) / exp(ls) is formed as
        // (x - loc) * exp(-ls).
        auto fexp = [](float x) -> float { return __builtin_amdgcn_exp2f(x * kLog2e); };
        auto base_pdf = [&](float a0, float a1) -> float {
            const float log2pi = 1.8378770664093453f;
            if (DOMAIN == BSDFD_DOMAIN_DISK) {  // model.py:393-398
                const float e0 = (a0 - bo[0]) * fexp(-bo[2]);
                const float e1 = (a1 - bo[1]) * fexp(-bo[3]);
                return fexp(-log2pi - (bo[2] + bo[3]) - 0.5f * (e0 * e0 + e1 * e1));
            } else {                            // model.py:308-317
                const float e = (a0 - bo[0]) * __builtin_amdgcn_rcpf(fexp(bo[1]) + 1e-3f);
                const float loggau = -0.5f * log2pi - bo[1] - 0.5f * e * e;
                float sd_, cd_;
                sincos_enc(a1 - bo[2], sd_, cd_);   // (bounded-argument kernel, 9e-8; libm beyond |arg| 1024)
                const float logvon = kappa * cd_ - log2pi - log_i0(kappa);
                return fexp(loggau + logvon);
            }
        };
        float p0 = 1.0f;
        if (op == OP_SAMPLE) p0 = base_pdf(x0, x1);

        // ---------------- T explicit Euler steps ---------------------------------------------------
        float acc = 1.0f;
        for (int t = 0; t < p.T; ++t) {
            // The depth-unrolled spherical kernel (4 hidden layers: 48 + 4 weight-fragment registers) spilled 11 VGPRs to
            // scratch at 3 waves/SIMD when the compiler hoisted every fragment load out of this loop (round 1: HBM traffic
            // 1.14x the algorithmic bytes).  Any asm statement in the loop body stops that hoisting, so for THIS
            // instantiation the fragments are re-read from LDS every step (13 conflict-free ds_read_b128 per step): 153
            // VGPRs, no scratch, traffic 1.0x, +0.9 % kernel time (profiles/r02_ab/ab2: variant r32, sph8).  The disk
            // kernel has no spills and keeps its fragments in registers (the same change costs it 2 %).  The depth-unrolled
            // 64 x 6 kernels could not hold 5 layers of 64-wide fragments in registers at all: same treatment.
            if ((DOMAIN == BSDFD_DOMAIN_SPHERICAL && ((NM == 2 && NH == 4 && JAC) || (NM == 4 && NH == 6))) || (FOLD_L1 && FUSED) || MIM || MIMS)
                asm volatile("s_nop 0");  // (the fused sample+pdf disk kernel: same treatment; MIM fetches its fragments explicitly.
                                          //  NOT an empty statement: hipcc's hazard recognizer counts every asm statement as one wait state)
            // alpha = float32(t/T) resp. float32(1 - t/T) as torch forms them (python double, then
            // cast); t * (1/T) in fp64 differs from t/T by < 1 ulp(fp64), invisible after the cast.
            float alpha;
            if (t_pow2) {  // t/T and 1 - t/T are exact in fp32 when T is a power of two: skip the fp64 ops
                const float tf = (float)t * invT;
                alpha = reverse ? 1.0f - tf : tf;
            } else {
                const double tf = (double)t * invT_d;
                alpha = (float)(reverse ? 1.0 - tf : tf);
            }
            f32x4 z[NM], zt0[NM], zt1[NM];
            if (DOMAIN == BSDFD_DOMAIN_DISK) {
                const float bs = sel4(g, x0, x1, alpha, 0.0f);
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    z[m] = mfma4(win[m], bs, cacc[m]);
                    zt0[m] = zt0c[m];
                    zt1[m] = zt1c[m];
                }
            } else {
                float sp, cp;
                sincos_enc(x1, sp, cp);
                const float bs = sel4(g, x0, sp, cp, alpha);
                const float bt = sel4(g, 0.0f, cp, -sp, 0.0f);  // d/dphi of the input
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    z[m] = mfma4(win[m], bs, cacc[m]);
                    if (!MIMS) zt0[m] = zt0c[m];
                    if (JAC) zt1[m] = mfma4(win[m], bt, zero4);
                }
            }

            f32x4 v = zero4, d0 = zero4, d1 = zero4;  // rows r=0,1: the two outputs
            // MIM / MIMS: J_ji = sum_k R_j[k] gm[k] U_i[k] over this lane's 8 units, then over the 4 lanes (g) of the query; det
            auto mim_finish = [&](const f32x4 (&R0)[NM], const f32x4 (&R1)[NM], const float (&gm)[NM][4], const f32x4 (&U0)[NM],
                                  const f32x4 (&U1)[NM]) {
                // (element pairs: the compiler emits v_pk_mul_f32 / v_pk_fma_f32 for the 2-vectors)
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                f32x2 ja2 = {0.f, 0.f}, jb2 = ja2, jc2 = ja2, jd2 = ja2;  // J00, J11, J01, J10
#pragma unroll
                for (int m = 0; m < NM; ++m)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x2 gg2 = {gm[m][2 * h], gm[m][2 * h + 1]};
                        const f32x2 r0 = {R0[m][2 * h], R0[m][2 * h + 1]}, r1 = {R1[m][2 * h], R1[m][2 * h + 1]};
                        const f32x2 u0 = gg2 * (f32x2){U0[m][2 * h], U0[m][2 * h + 1]};
                        const f32x2 u1 = gg2 * (f32x2){U1[m][2 * h], U1[m][2 * h + 1]};
                        ja2 = __builtin_elementwise_fma(r0, u0, ja2);
                        jc2 = __builtin_elementwise_fma(r0, u1, jc2);
                        jd2 = __builtin_elementwise_fma(r1, u0, jd2);
                        jb2 = __builtin_elementwise_fma(r1, u1, jb2);
                    }
                float ja = ja2[0] + ja2[1], jb = jb2[0] + jb2[1], jc = jc2[0] + jc2[1], jd = jd2[0] + jd2[1];
                // v_permlane32_swap(x, y): x[32..63] <-> y[0..31]; afterwards x + y holds, in the lower half-wave, x summed
                // over the lane pairs (l, l + 32) and, in the upper half, y summed over them.  v_permlane16_swap does the
                // same between the odd 16-lane rows of x and the even rows of y.  Two levels leave J00 | J01 | J11 | J10 in
                // rows 0 | 1 | 2 | 3 (row = g = lane >> 4), each summed over the query's 4 lanes.
                auto swap32 = [](float& x, float& y) {
                    const auto t_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                    x = __uint_as_float(t_[0]); y = __uint_as_float(t_[1]);
                };
                auto swap16 = [](float& x, float& y) {
                    const auto t_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                    x = __uint_as_float(t_[0]); y = __uint_as_float(t_[1]);
                };
                swap32(ja, jb);
                float sab = ja + jb;        // rows 0,1: J00 over (g, g+2) | rows 2,3: J11 over (g-2, g)
                swap32(jc, jd);
                float scd = jc + jd;        // rows 0,1: J01 | rows 2,3: J10
                swap16(sab, scd);
                const float tj = sab + scd; // row 0: J00, row 1: J01, row 2: J11, row 3: J10
                // w = 1 + c J on the diagonal rows (0, 2), c J on the others; det = w0 w2 - w1 w3 (mlp_brdf_sampling.py:44-46)
                float w = fmaf(cstep, tj, (g & 1) ? 0.0f : 1.0f), w2 = w;
                swap32(w, w2);              // w: rows (0,1,0,1) of the old w, w2: rows (2,3,2,3)
                float pr = w * w2, pr2 = pr;  // row 0: w0 w2, row 1: w1 w3
                swap16(pr, pr2);            // pr row 0 = old row 0, pr2 row 0 = old row 1
                const float det = pr - pr2; // valid in row 0 (g == 0), the lane that writes the query's results
                // forward: the reference divides (tmp_J /= J); v_rcp_f32 (1 ulp) * acc differs from the IEEE quotient by <= 2 ulp
                if (reverse) acc *= det; else acc *= __builtin_amdgcn_rcpf(det);
            };
            if (PREC == BSDFD_PREC_F32) {
                for (int layer = 0; layer < n_hidden; ++layer) {
                    const bool last = (layer == n_hidden - 1);
                    if (NH == 0) loop_head_pad<NM, JAC>(z, zt0, zt1);
                    float h[NM][4], t0[NM][4], t1[NM][4];
#pragma unroll
                    for (int m = 0; m < NM; ++m)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float gg;
                            silu_grad_scaled(z[m][r], h[m][r], gg);
                            if (JAC) {
                                t0[m][r] = zt0[m][r] * gg;
                                t1[m][r] = zt1[m][r] * gg;
                            }
                        }
                    if (!last) {
                        const char* base = Lwh + (size_t)layer * NM * NM * 64 * 16;
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) {
                            f32x4 a = zero4, a0 = zero4, a1 = zero4;
#pragma unroll
                            for (int m = 0; m < NM; ++m) {
                                const f32x4 w = *reinterpret_cast<const f32x4*>(base + ((mo * NM + m) * 64 + lane) * 16);
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    a = mfma4(w[r], h[m][r], a);
                                    if (JAC) {
                                        a0 = mfma4(w[r], t0[m][r], a0);
                                        a1 = mfma4(w[r], t1[m][r], a1);
                                    }
                                }
                            }
                            z[mo] = a; zt0[mo] = a0; zt1[mo] = a1;
                        }
                    } else {
#pragma unroll
                        for (int m = 0; m < NM; ++m) {
                            const f32x4 w = *reinterpret_cast<const f32x4*>(Lwo + (m * 64 + lane) * 16);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                v = mfma4(w[r], h[m][r], v);
                                if (JAC) {
                                    d0 = mfma4(w[r], t0[m][r], d0);
                                    d1 = mfma4(w[r], t1[m][r], d1);
                                }
                            }
                        }
                    }
                }
            } else if (MIM) {
                // ---- disk 25-32-32-32-2 nets: the 2x2 Jacobian by MEETING IN THE MIDDLE -------------------------------
                // J = Wout D3 W3 D2 W2 D1 W1[:, :2] (D_l = diag silu'(z_l)).  Forward mode carries two tangent vectors
                // through every layer: each needs a scaling by silu', a hi/lo split and its share of the MFMAs.  Here the
                // input side is folded as before (U_i = W2 D1 W1[:, i] = F_i g1, F_i = W2 diag(W1[:, i]) packed by the host)
                // and the OUTPUT side the same way, transposed: R_j = (Wout D3 W3)^T[:, j] = G_j g3 with
                // G_j = W3^T diag(Wout[j, :]).  Both are plain matrix x vector contractions of the per-unit factors g1, g3;
                // the middle factor D2 is applied in fp32: J_ji = sum_k R_j[k] g2[k] U_i[k].  Per step: 5 vectors split
                // instead of 8, no tangent scalings, 38 fp16 MFMAs instead of 42; the price is the 2x2 bilinear form
                // (24 packed FMAs) and one cross-lane reduction over the 4 lanes of a query (5 v_permlane swaps).
                constexpr bool SPLIT = (PREC == BSDFD_PREC_SPLIT3);
                // Weight fragments: 25 per step (W2, W3 hi/lo, Wout, F_0, F_1, G_0, G_1 hi/lo).  They do not fit the register
                // budget of 3 waves/SIMD next to the flow state, so each layer's fragments are requested from LDS with
                // asynchronous reads one phase ahead (behind the previous layer's MFMAs, in flight during this layer's activation
                // math; the lo parts, which feed a layer's last MFMAs, behind the wait for its hi parts) and waited for once.  The image layout of this instantiation is a
                // compile-time constant (build_image checks it), so every read is `lane base + immediate offset`.
                constexpr int FR = 64 * 16;                                         // bytes of one fragment
                constexpr int O_WH = NM * 64 * 4 + NM * PE_SLABS * 64 * 4;          // L.wh
                constexpr int O_WHL = O_WH + (NH - 1) * NM * FR;                    // L.wh_lo (split3)
                constexpr int O_WO = SPLIT ? O_WHL + (NH - 1) * NM * FR : O_WHL;    // L.wo
                constexpr int O_WF = O_WO + FR;                                     // L.wf
                constexpr int O_WFL = O_WF + 2 * NM * FR;                           // L.wf_lo
                constexpr int O_WG = SPLIT ? O_WFL + 2 * NM * FR : O_WFL;           // L.wg
                constexpr int O_WGL = O_WG + 2 * NM * FR;                           // L.wg_lo
                const unsigned lb = (unsigned)(uintptr_t)smem + (unsigned)lane * 16u;
                float hv[NM][4], gv[NM][4];
                Frag bh, bl, gh, gl;
                // Request points.  EARLY (single-op kernels): a layer's fragments are requested before the previous layer's MFMAs
                // and its lo parts together with the hi parts — measured 1 % faster than LATE.  LATE (fused sample+pdf kernel,
                // whose second phase keeps more state live): behind the previous layer's MFMAs, and the lo parts — which feed a
                // layer's last MFMAs — only behind the wait for its hi parts; this keeps the two-phase kernel free of spills.
                constexpr bool LATE = FUSED;
                f16x8 w2h[NM], w2l[NM], f0h[NM], f1h[NM], f0l[NM], f1l[NM], w3h[NM], w3l[NM], wo, g0h[NM], g1h[NM], g0l[NM], g1l[NM];
                auto req_A_lo = [&] {
                    if (!SPLIT) return;
                    lds_read_b128_async_at<O_WHL>(w2l[0], lb); lds_read_b128_async_at<O_WHL + FR>(w2l[1], lb);
                    lds_read_b128_async_at<O_WFL>(f0l[0], lb); lds_read_b128_async_at<O_WFL + FR>(f0l[1], lb);
                    lds_read_b128_async_at<O_WFL + 2 * FR>(f1l[0], lb); lds_read_b128_async_at<O_WFL + 3 * FR>(f1l[1], lb);
                };
                auto req_B = [&] {
                    lds_read_b128_async_at<O_WH + 2 * FR>(w3h[0], lb); lds_read_b128_async_at<O_WH + 3 * FR>(w3h[1], lb);
                    if (SPLIT) { lds_read_b128_async_at<O_WHL + 2 * FR>(w3l[0], lb); lds_read_b128_async_at<O_WHL + 3 * FR>(w3l[1], lb); }
                };
                auto req_C_hi = [&] {
                    lds_read_b128_async_at<O_WO>(wo, lb);
                    lds_read_b128_async_at<O_WG>(g0h[0], lb); lds_read_b128_async_at<O_WG + FR>(g0h[1], lb);
                    lds_read_b128_async_at<O_WG + 2 * FR>(g1h[0], lb); lds_read_b128_async_at<O_WG + 3 * FR>(g1h[1], lb);
                };
                auto req_C_lo = [&] {
                    if (!SPLIT) return;
                    lds_read_b128_async_at<O_WGL>(g0l[0], lb); lds_read_b128_async_at<O_WGL + FR>(g0l[1], lb);
                    lds_read_b128_async_at<O_WGL + 2 * FR>(g1l[0], lb); lds_read_b128_async_at<O_WGL + 3 * FR>(g1l[1], lb);
                };
                // -- hidden layer 1 -> z2, U0, U1
                lds_read_b128_async_at<O_WH>(w2h[0], lb); lds_read_b128_async_at<O_WH + FR>(w2h[1], lb);
                lds_read_b128_async_at<O_WF>(f0h[0], lb); lds_read_b128_async_at<O_WF + FR>(f0h[1], lb);
                lds_read_b128_async_at<O_WF + 2 * FR>(f1h[0], lb); lds_read_b128_async_at<O_WF + 3 * FR>(f1h[1], lb);
                if (!LATE) req_A_lo();
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) silu_grad_scaled(z[m][r], hv[m][r], gv[m][r]);
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                    split_pack<SPLIT>(gv[m], gh.p[2 * m], gh.p[2 * m + 1], gl.p[2 * m], gl.p[2 * m + 1]);
                }
                BSDFD_WAIT6(gh.v, w2h[0], w2h[1], f0h[0], f0h[1], f1h[0], f1h[1]);
                if (LATE) req_A_lo();
                else {
                    if (SPLIT) BSDFD_WAIT6(gl.v, w2l[0], w2l[1], f0l[0], f0l[1], f1l[0], f1l[1]);
                    req_B();
                }
                // z2 first (the next activation needs nothing else); the 12 MFMAs of U0, U1 are off the critical path — J is
                // formed at the end of the step — so they run in the matrix pipe under the next layer's activation math
                f32x4 U0[NM], U1[NM];
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w2h[mo], bh.v, zero4);
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w2h[mo], bl.v, z[mo]);
                    if (!LATE) {
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w2l[mo], bh.v, z[mo]);
                    }
                }
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) {
                    U0[mo] = mfma16(f0h[mo], gh.v, zero4);
                    U1[mo] = mfma16(f1h[mo], gh.v, zero4);
                }
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        U0[mo] = mfma16(f0h[mo], gl.v, U0[mo]);
                        U1[mo] = mfma16(f1h[mo], gl.v, U1[mo]);
                    }
                    if (LATE) {
                        BSDFD_WAIT6(U1[1], w2l[0], w2l[1], f0l[0], f0l[1], f1l[0], f1l[1]);
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w2l[mo], bh.v, z[mo]);
                    }
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        U0[mo] = mfma16(f0l[mo], gh.v, U0[mo]);
                        U1[mo] = mfma16(f1l[mo], gh.v, U1[mo]);
                    }
                }
                if (LATE) req_B();
                // -- hidden layer 2 -> z3 (its silu' stays in fp32: the middle factor of J)
                float g2[NM][4];
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) silu_grad_scaled(z[m][r], hv[m][r], g2[m][r]);
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                }
                if (SPLIT) BSDFD_WAIT4(bl.v, w3h[0], w3h[1], w3l[0], w3l[1]); else BSDFD_WAIT2(bh.v, w3h[0], w3h[1]);
                if (!LATE) { req_C_hi(); req_C_lo(); }
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w3h[mo], bh.v, zero4);
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w3h[mo], bl.v, z[mo]);
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(w3l[mo], bh.v, z[mo]);
                }
                if (LATE) req_C_hi();
                // -- hidden layer 3 -> v, R0, R1
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) silu_grad_scaled(z[m][r], hv[m][r], gv[m][r]);
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                    split_pack<SPLIT>(gv[m], gh.p[2 * m], gh.p[2 * m + 1], gl.p[2 * m], gl.p[2 * m + 1]);
                }
                BSDFD_WAIT5(gh.v, wo, g0h[0], g0h[1], g1h[0], g1h[1]);
                if (LATE) req_C_lo();  // (the lo parts feed the last 4 of the 14 MFMAs below)
                else if (SPLIT) BSDFD_WAIT4(gl.v, g0l[0], g0l[1], g1l[0], g1l[1]);
                f32x4 R0[NM], R1[NM];
                {
                    f32x4 e = mfma16(wo, bh.v, zero4);
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        R0[mo] = mfma16(g0h[mo], gh.v, zero4);
                        R1[mo] = mfma16(g1h[mo], gh.v, zero4);
                    }
                    if (SPLIT) {
                        e = mfma16(wo, bl.v, e);
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) {
                            R0[mo] = mfma16(g0h[mo], gl.v, R0[mo]);
                            R1[mo] = mfma16(g1h[mo], gl.v, R1[mo]);
                        }
                        if (LATE) BSDFD_WAIT4(R1[1], g0l[0], g0l[1], g1l[0], g1l[1]);
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) {
                            R0[mo] = mfma16(g0l[mo], gh.v, R0[mo]);
                            R1[mo] = mfma16(g1l[mo], gh.v, R1[mo]);
                        }
                    }
                    v[0] = fmaf(e[2], kWoLoInv, e[0]); v[1] = fmaf(e[3], kWoLoInv, e[1]);
                }
                mim_finish(R0, R1, g2, U0, U1);
            } else if (MIMS) {
                // ---- spherical 26-32-32-32-32-2 nets: J = [Wout D4 W4] D3 [W3 D2 W2 D1 W1 E] -----------------------------
                // E = d(theta, sin phi, cos phi)/d(theta, phi) depends on the state, so the input side is not foldable into the
                // weights: the two tangents go through hidden layers 1 and 2 in forward mode as before (zt3_i = W3 (g2 . W2 (g1 .
                // zt1_i)) = U_i, fp32 accumulators).  The output side is folded (R_j = G_j g4, G_j = W4^T diag(Wout[j, :])) and
                // J_ji = sum_k R_j[k] g3[k] U_i[k].  Per step 9 vectors are split instead of 12 and 56 fp16 MFMAs issue instead
                // of 60.  Fragments: asynchronous LDS reads one phase ahead, as in the disk block above.
                constexpr bool SPLIT = (PREC == BSDFD_PREC_SPLIT3);
                constexpr int FR = 64 * 16;
                constexpr int O_WH = NM * 64 * 4 + NM * PE_SLABS * 64 * 4;          // L.wh: W2, W3, W4 (2 fragments each)
                constexpr int O_WHL = O_WH + (NH - 1) * NM * FR;                    // L.wh_lo
                constexpr int O_WO = SPLIT ? O_WHL + (NH - 1) * NM * FR : O_WHL;    // L.wo
                constexpr int O_WG = O_WO + FR;                                     // L.wg
                constexpr int O_WGL = O_WG + 2 * NM * FR;                           // L.wg_lo
                const unsigned lb = (unsigned)(uintptr_t)smem + (unsigned)lane * 16u;
                float hv[NM][4], gv[NM][4], t0v[NM][4], t1v[NM][4];
                Frag bh, bl, b0h, b0l, b1h, b1l;
                f16x8 wAh[NM], wAl[NM], wBh[NM], wBl[NM];  // (W2 / W4 and W3: each set is requested behind the previous layer's MFMAs)
                // the constant d/dtheta pre-activations of layer 1 (column 0 of W1 in the accumulator layout) come from LDS every
                // step instead of living in 8 registers across the whole tile (ordinary loads: the compiler waits for them)
#pragma unroll
                for (int m = 0; m < NM; ++m) zt0[m] = Lwt0[m * 64 + lane];
                lds_read_b128_async_at<O_WH>(wAh[0], lb); lds_read_b128_async_at<O_WH + FR>(wAh[1], lb);
                if (SPLIT) { lds_read_b128_async_at<O_WHL>(wAl[0], lb); lds_read_b128_async_at<O_WHL + FR>(wAl[1], lb); }
                // -- hidden layer 1 (tangent pre-activations zt0 = W1 e_theta (constant), zt1 = W1 d(input)/d(phi))
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        silu_grad_scaled(z[m][r], hv[m][r], gv[m][r]);
                        t0v[m][r] = zt0[m][r] * gv[m][r];
                        t1v[m][r] = zt1[m][r] * gv[m][r];
                    }
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                    split_pack<SPLIT>(t0v[m], b0h.p[2 * m], b0h.p[2 * m + 1], b0l.p[2 * m], b0l.p[2 * m + 1]);
                    split_pack<SPLIT>(t1v[m], b1h.p[2 * m], b1h.p[2 * m + 1], b1l.p[2 * m], b1l.p[2 * m + 1]);
                }
                if (SPLIT) BSDFD_WAIT4(b1l.v, wAh[0], wAh[1], wAl[0], wAl[1]); else BSDFD_WAIT2(b1h.v, wAh[0], wAh[1]);
                f32x4 U0[NM], U1[NM];
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) {
                    z[mo] = mfma16(wAh[mo], bh.v, zero4);
                    U0[mo] = mfma16(wAh[mo], b0h.v, zero4);
                    U1[mo] = mfma16(wAh[mo], b1h.v, zero4);
                }
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        z[mo] = mfma16(wAh[mo], bl.v, z[mo]);
                        U0[mo] = mfma16(wAh[mo], b0l.v, U0[mo]);
                        U1[mo] = mfma16(wAh[mo], b1l.v, U1[mo]);
                    }
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        z[mo] = mfma16(wAl[mo], bh.v, z[mo]);
                        U0[mo] = mfma16(wAl[mo], b0h.v, U0[mo]);
                        U1[mo] = mfma16(wAl[mo], b1h.v, U1[mo]);
                    }
                }
                // next layer's fragments: requested behind this layer's MFMAs (so that the two sets are never live together),
                // in flight during the next activation math (~170 VALU instructions: several LDS latencies)
                lds_read_b128_async_at<O_WH + 2 * FR>(wBh[0], lb); lds_read_b128_async_at<O_WH + 3 * FR>(wBh[1], lb);
                if (SPLIT) { lds_read_b128_async_at<O_WHL + 2 * FR>(wBl[0], lb); lds_read_b128_async_at<O_WHL + 3 * FR>(wBl[1], lb); }
                // -- hidden layer 2
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        silu_grad_scaled(z[m][r], hv[m][r], gv[m][r]);
                        t0v[m][r] = U0[m][r] * gv[m][r];
                        t1v[m][r] = U1[m][r] * gv[m][r];
                    }
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                    split_pack<SPLIT>(t0v[m], b0h.p[2 * m], b0h.p[2 * m + 1], b0l.p[2 * m], b0l.p[2 * m + 1]);
                    split_pack<SPLIT>(t1v[m], b1h.p[2 * m], b1h.p[2 * m + 1], b1l.p[2 * m], b1l.p[2 * m + 1]);
                }
                if (SPLIT) BSDFD_WAIT4(b1l.v, wBh[0], wBh[1], wBl[0], wBl[1]); else BSDFD_WAIT2(b1h.v, wBh[0], wBh[1]);
                // z3 first; U_i = zt3_i are needed only when J is formed
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wBh[mo], bh.v, zero4);
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wBh[mo], bl.v, z[mo]);
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wBl[mo], bh.v, z[mo]);
                }
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) {
                    U0[mo] = mfma16(wBh[mo], b0h.v, zero4);
                    U1[mo] = mfma16(wBh[mo], b1h.v, zero4);
                }
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        U0[mo] = mfma16(wBh[mo], b0l.v, U0[mo]);
                        U1[mo] = mfma16(wBh[mo], b1l.v, U1[mo]);
                    }
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        U0[mo] = mfma16(wBl[mo], b0h.v, U0[mo]);
                        U1[mo] = mfma16(wBl[mo], b1h.v, U1[mo]);
                    }
                }
                lds_read_b128_async_at<O_WH + 4 * FR>(wAh[0], lb); lds_read_b128_async_at<O_WH + 5 * FR>(wAh[1], lb);
                if (SPLIT) { lds_read_b128_async_at<O_WHL + 4 * FR>(wAl[0], lb); lds_read_b128_async_at<O_WHL + 5 * FR>(wAl[1], lb); }
                // -- hidden layer 3 (its silu' stays in fp32: the middle factor of J)
                float g3[NM][4];
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) silu_grad_scaled(z[m][r], hv[m][r], g3[m][r]);
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                }
                if (SPLIT) BSDFD_WAIT4(bl.v, wAh[0], wAh[1], wAl[0], wAl[1]); else BSDFD_WAIT2(bh.v, wAh[0], wAh[1]);
#pragma unroll
                for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wAh[mo], bh.v, zero4);
                if (SPLIT) {
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wAh[mo], bl.v, z[mo]);
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) z[mo] = mfma16(wAl[mo], bh.v, z[mo]);
                }
                f16x8 wo, g0h[NM], g1h[NM], g0l[NM], g1l[NM];
                lds_read_b128_async_at<O_WO>(wo, lb);
                lds_read_b128_async_at<O_WG>(g0h[0], lb); lds_read_b128_async_at<O_WG + FR>(g0h[1], lb);
                lds_read_b128_async_at<O_WG + 2 * FR>(g1h[0], lb); lds_read_b128_async_at<O_WG + 3 * FR>(g1h[1], lb);
                // -- hidden layer 4 -> v, R0, R1
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) silu_grad_scaled(z[m][r], hv[m][r], gv[m][r]);
                    split_pack<SPLIT>(hv[m], bh.p[2 * m], bh.p[2 * m + 1], bl.p[2 * m], bl.p[2 * m + 1]);
                    split_pack<SPLIT>(gv[m], b0h.p[2 * m], b0h.p[2 * m + 1], b0l.p[2 * m], b0l.p[2 * m + 1]);
                }
                BSDFD_WAIT5(b0h.v, wo, g0h[0], g0h[1], g1h[0], g1h[1]);
                // (the lo parts of G are requested only now — they feed the last 4 of the 14 MFMAs below, ~150 cycles away —
                //  so that they are not live during the activation math: with them the kernel spilled 2 VGPRs)
                if (SPLIT) {
                    lds_read_b128_async_at<O_WGL>(g0l[0], lb); lds_read_b128_async_at<O_WGL + FR>(g0l[1], lb);
                    lds_read_b128_async_at<O_WGL + 2 * FR>(g1l[0], lb); lds_read_b128_async_at<O_WGL + 3 * FR>(g1l[1], lb);
                }
                f32x4 R0[NM], R1[NM];
                {
                    f32x4 e = mfma16(wo, bh.v, zero4);
#pragma unroll
                    for (int mo = 0; mo < NM; ++mo) {
                        R0[mo] = mfma16(g0h[mo], b0h.v, zero4);
                        R1[mo] = mfma16(g1h[mo], b0h.v, zero4);
                    }
                    if (SPLIT) {
                        e = mfma16(wo, bl.v, e);
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) {
                            R0[mo] = mfma16(g0h[mo], b0l.v, R0[mo]);
                            R1[mo] = mfma16(g1h[mo], b0l.v, R1[mo]);
                        }
                        BSDFD_WAIT4(R1[1], g0l[0], g0l[1], g1l[0], g1l[1]);
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) {
                            R0[mo] = mfma16(g0l[mo], b0h.v, R0[mo]);
                            R1[mo] = mfma16(g1l[mo], b0h.v, R1[mo]);
                        }
                    }
                    v[0] = fmaf(e[2], kWoLoInv, e[0]); v[1] = fmaf(e[3], kWoLoInv, e[1]);
                }
                mim_finish(R0, R1, g3, U0, U1);
            } else {
                // ---- fp16 MFMA path ----
                // Per layer: one sigmoid per unit -> (hs, g); tangents scaled by g; the lane's own 8
                // values per K chunk ARE the B fragment of the next contraction, split into hi + lo
                // (SPLIT3); the three products share one fp32 accumulator, and the MFMAs are issued
                // term-major over the 3 x NM accumulators so that no two consecutive MFMAs depend on
                // each other.  (A software-pipelined variant that interleaved the MFMAs of one vector
                // with the VALU work of the next measured no faster: on gfx950 a 16x16x32 MFMA hides
                // only ~3 VALU issues, tools/ubench/mfma_overlap.hip — MFMA and VALU time add.)
                constexpr bool SPLIT = (PREC == BSDFD_PREC_SPLIT3);
                constexpr bool TSPLIT = SPLIT && (kTangentPrec == 3);   // tangents: hi+lo operands
                constexpr bool TWLO = SPLIT && (kTangentPrec >= 2);     // tangents: W_lo product
                // NH > 0: fully unrolled.  NH == 0 (run-time depth) cannot be, and clang says so (-Wpass-failed,
                // silenced in the build line); an explicit `unroll 1` there measured 13 % slower on the 64-wide net
                const bool foldout = FOLDOUT && n_hidden >= 2;
                float gmid[NM][4];     // FOLDOUT: silu' of the second-to-last hidden layer, the fp32 middle factor of J
                f32x4 Uf0[NM], Uf1[NM], Rf0[NM], Rf1[NM];
#pragma unroll
                for (int layer = 0; layer < n_hidden; ++layer) {
                    const bool last = (layer == n_hidden - 1);
                    if (NH == 0) loop_head_pad<NM, JAC>(z, zt0, zt1);
                    // first hidden layer of a disk net: folded tangents (FOLD_L1 above) — split g, not t_0 and t_1
                    const bool fold = FOLD_L1 && layer == 0 && !last;
                    const bool pen = foldout && layer == n_hidden - 2;   // the tangents stop here (see FOLDOUT)
                    const bool lastf = foldout && last;                  // ... and g_L alone is split: b0h / b0l hold it
                    Frag bh[KC], bl[KC], b0h[KC], b0l[KC], b1h[KC], b1l[KC];
                    if (pen) {
#pragma unroll
                        for (int m = 0; m < NM; ++m) { Uf0[m] = zt0[m]; Uf1[m] = zt1[m]; }
                    }
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        if constexpr (!SPLIT && !JAC && PREC == BSDFD_PREC_F16) {
                            // precision f16, no Jacobian: two M-tiles' sigmoids in packed fp16 straight into the chunk's B fragment
                            // (flow_dev.h: act_pack8; round 5, as in the 32-query-tile kernels of csrc/flow32.hip)
                            if ((m & 1) == 0) {
                                const float z8[8] = {z[m][0], z[m][1], z[m][2], z[m][3], z[m + 1][0], z[m + 1][1], z[m + 1][2], z[m + 1][3]};
                                act_pack8(z8, bh[m >> 1]);
                            }
                            continue;
                        }
                        float hv[4], t0v[4], t1v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float gg;
                            silu_grad_scaled(z[m][r], hv[r], gg);
                            if (JAC) {
                                if (pen) gmid[m][r] = gg;
                                t0v[r] = (fold || lastf) ? gg : zt0[m][r] * gg;
                                if (!fold && !lastf) t1v[r] = zt1[m][r] * gg;
                            }
                        }
                        const int kc = m >> 1, q0 = 2 * (m & 1);
                        split_pack<SPLIT>(hv, bh[kc].p[q0], bh[kc].p[q0 + 1], bl[kc].p[q0], bl[kc].p[q0 + 1]);
                        if (JAC && pen) {
                            // nothing to split: the tangents are consumed in fp32 by the bilinear form
                        } else if (JAC && (fold || lastf)) {
                            split_pack<TSPLIT>(t0v, b0h[kc].p[q0], b0h[kc].p[q0 + 1], b0l[kc].p[q0], b0l[kc].p[q0 + 1]);
                        } else if (JAC) {
                            split_pack<TSPLIT>(t0v, b0h[kc].p[q0], b0h[kc].p[q0 + 1], b0l[kc].p[q0], b0l[kc].p[q0 + 1]);
                            split_pack<TSPLIT>(t1v, b1h[kc].p[q0], b1h[kc].p[q0 + 1], b1l[kc].p[q0], b1l[kc].p[q0 + 1]);
                        }
                    }
                    if (!last) {
                        const size_t lbase = (size_t)layer * NM * KC * 64 * 16;
                        f32x4 a[NM], a0[NM], a1[NM];
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) { a[mo] = zero4; a0[mo] = zero4; a1[mo] = zero4; }
#pragma unroll
                        for (int kc = 0; kc < KC; ++kc) {
                            f16x8 wh[NM], wl[NM];
#pragma unroll
                            for (int mo = 0; mo < NM; ++mo) {
                                const size_t off = lbase + ((size_t)(mo * KC + kc) * 64 + lane) * 16;
                                wh[mo] = *reinterpret_cast<const f16x8*>(Lwh + off);
                                if (SPLIT) wl[mo] = *reinterpret_cast<const f16x8*>(Lwh_lo + off);
                            }
                            if (JAC && fold) {
                                // tangent accumulators: folded matrices x g (the B fragments of g sit in b0h / b0l); issued
                                // term-major like the regular layers, so that consecutive MFMAs never share an accumulator
                                constexpr size_t fstride = (size_t)NM * KC * 64 * 16;
                                f16x8 f0h[NM], f0l[NM], f1h[NM], f1l[NM];
#pragma unroll
                                for (int mo = 0; mo < NM; ++mo) {
                                    const size_t foff = ((size_t)(mo * KC + kc) * 64 + lane) * 16;
                                    f0h[mo] = *reinterpret_cast<const f16x8*>(Lwf + foff);
                                    f1h[mo] = *reinterpret_cast<const f16x8*>(Lwf + fstride + foff);
                                    if (SPLIT) {
                                        f0l[mo] = *reinterpret_cast<const f16x8*>(Lwf_lo + foff);
                                        f1l[mo] = *reinterpret_cast<const f16x8*>(Lwf_lo + fstride + foff);
                                    }
                                }
#pragma unroll
                                for (int mo = 0; mo < NM; ++mo) {
                                    a[mo] = mfma16(wh[mo], bh[kc].v, a[mo]);
                                    a0[mo] = mfma16(f0h[mo], b0h[kc].v, a0[mo]);
                                    a1[mo] = mfma16(f1h[mo], b0h[kc].v, a1[mo]);
                                }
                                if (SPLIT) {
#pragma unroll
                                    for (int mo = 0; mo < NM; ++mo) {
                                        a[mo] = mfma16(wh[mo], bl[kc].v, a[mo]);
                                        if (TSPLIT) { a0[mo] = mfma16(f0h[mo], b0l[kc].v, a0[mo]); a1[mo] = mfma16(f1h[mo], b0l[kc].v, a1[mo]); }
                                    }
#pragma unroll
                                    for (int mo = 0; mo < NM; ++mo) {
                                        a[mo] = mfma16(wl[mo], bh[kc].v, a[mo]);
                                        if (TWLO) { a0[mo] = mfma16(f0l[mo], b0h[kc].v, a0[mo]); a1[mo] = mfma16(f1l[mo], b0h[kc].v, a1[mo]); }
                                    }
                                }
                                continue;
                            }
                            const bool tang = JAC && !pen;   // (FOLDOUT: no tangent contractions out of the second-to-last layer)
#pragma unroll
                            for (int mo = 0; mo < NM; ++mo) {
                                a[mo] = mfma16(wh[mo], bh[kc].v, a[mo]);
                                if (tang) { a0[mo] = mfma16(wh[mo], b0h[kc].v, a0[mo]); a1[mo] = mfma16(wh[mo], b1h[kc].v, a1[mo]); }
                            }
                            if (SPLIT) {
#pragma unroll
                                for (int mo = 0; mo < NM; ++mo) {
                                    a[mo] = mfma16(wh[mo], bl[kc].v, a[mo]);
                                    if (tang && TSPLIT) { a0[mo] = mfma16(wh[mo], b0l[kc].v, a0[mo]); a1[mo] = mfma16(wh[mo], b1l[kc].v, a1[mo]); }
                                }
#pragma unroll
                                for (int mo = 0; mo < NM; ++mo) {
                                    a[mo] = mfma16(wl[mo], bh[kc].v, a[mo]);
                                    if (tang && TWLO) { a0[mo] = mfma16(wl[mo], b0h[kc].v, a0[mo]); a1[mo] = mfma16(wl[mo], b1h[kc].v, a1[mo]); }
                                }
                            }
                        }
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) { z[mo] = a[mo]; zt0[mo] = a0[mo]; zt1[mo] = a1[mo]; }
                    } else if (lastf) {
                        // output layer for h as below; R_j = G_j g_L (fragments of G_0, G_1 behind L.wg, hi / lo)
                        f32x4 e = zero4;
#pragma unroll
                        for (int mo = 0; mo < NM; ++mo) { Rf0[mo] = zero4; Rf1[mo] = zero4; }
#pragma unroll
                        for (int kc = 0; kc < KC; ++kc) {
                            const f16x8 wo = *reinterpret_cast<const f16x8*>(Lwo + ((size_t)kc * 64 + lane) * 16);
                            e = mfma16(wo, bh[kc].v, e);
                            if (SPLIT) e = mfma16(wo, bl[kc].v, e);
                            constexpr size_t gstride = (size_t)NM * KC * 64 * 16;
#pragma unroll
                            for (int mo = 0; mo < NM; ++mo) {
                                const size_t goff = ((size_t)(mo * KC + kc) * 64 + lane) * 16;
                                const f16x8 g0h = *reinterpret_cast<const f16x8*>(Lwg + goff);
                                const f16x8 g1h = *reinterpret_cast<const f16x8*>(Lwg + gstride + goff);
                                Rf0[mo] = mfma16(g0h, b0h[kc].v, Rf0[mo]);
                                Rf1[mo] = mfma16(g1h, b0h[kc].v, Rf1[mo]);
                                if (TSPLIT) { Rf0[mo] = mfma16(g0h, b0l[kc].v, Rf0[mo]); Rf1[mo] = mfma16(g1h, b0l[kc].v, Rf1[mo]); }
                                if (TWLO) {
                                    const f16x8 g0l = *reinterpret_cast<const f16x8*>(Lwg_lo + goff);
                                    const f16x8 g1l = *reinterpret_cast<const f16x8*>(Lwg_lo + gstride + goff);
                                    Rf0[mo] = mfma16(g0l, b0h[kc].v, Rf0[mo]);
                                    Rf1[mo] = mfma16(g1l, b0h[kc].v, Rf1[mo]);
                                }
                            }
                        }
                        v[0] = fmaf(e[2], kWoLoInv, e[0]); v[1] = fmaf(e[3], kWoLoInv, e[1]);
                    } else {
                        // output layer: A rows (i&3) = {Wout_hi[0], Wout_hi[1], Wout_lo[0], Wout_lo[1]}, so
                        // e[0..1] = hi*hi + hi*lo and e[2..3] = (lo*hi + lo*lo) x BSDFD_WO_LO_SCALE: out = e[o] + e[o+2] / scale
                        f32x4 e = zero4, e0 = zero4, e1 = zero4;
#pragma unroll
                        for (int kc = 0; kc < KC; ++kc) {
                            const f16x8 wo = *reinterpret_cast<const f16x8*>(Lwo + ((size_t)kc * 64 + lane) * 16);
                            e = mfma16(wo, bh[kc].v, e);
                            if (JAC) { e0 = mfma16(wo, b0h[kc].v, e0); e1 = mfma16(wo, b1h[kc].v, e1); }
                            if (SPLIT) {
                                e = mfma16(wo, bl[kc].v, e);
                                if (JAC && TSPLIT) { e0 = mfma16(wo, b0l[kc].v, e0); e1 = mfma16(wo, b1l[kc].v, e1); }
                            }
                        }
                        v[0] = fmaf(e[2], kWoLoInv, e[0]); v[1] = fmaf(e[3], kWoLoInv, e[1]);
                        d0[0] = fmaf(e0[2], kWoLoInv, e0[0]); d0[1] = fmaf(e0[3], kWoLoInv, e0[1]);
                        d1[0] = fmaf(e1[2], kWoLoInv, e1[0]); d1[1] = fmaf(e1[3], kWoLoInv, e1[1]);
                    }
                }
                if (foldout) mim_finish(Rf0, Rf1, gmid, Uf0, Uf1);
            }

            // det(I + c*J) with the row convention of mlp_brdf_sampling.py:44-46; signed.
            if (JAC && !MIM && !MIMS && !(FOLDOUT && n_hidden >= 2)) {
                const float j00 = 1.0f + cstep * d0[0];
                const float j01 = cstep * d1[0];
                const float j10 = cstep * d0[1];
                const float j11 = 1.0f + cstep * d1[1];
                const float det = j00 * j11 - j01 * j10;
                // forward: the reference divides (tmp_J /= J); v_rcp_f32 (1 ulp) * acc differs from the
                // IEEE quotient by <= 2 ulp, far below the fp32 noise of det itself
                if (reverse) acc *= det; else acc *= __builtin_amdgcn_rcpf(det);
            }
            x0 += cstep * v[0];
            x1 += cstep * v[1];
        }

        // ---------------- epilogue: density, warp, guards, store ------------------------------------
        float pdf = 0.0f;
        if (op == OP_SAMPLE) pdf = p0 * acc;
        else if (op == OP_PDF) pdf = base_pdf(x0, x1) * acc;

        bool valid_e = valid;
        const long long qe_tile = REMAT ? row_of(opaque(q), valid_e) : qi;
        const long long qe = p.io == IO_OPERATOR ? qe_tile : user_row(qe_tile);
        const bool writer = valid_e && g == 0;
        if (p.io == IO_OPERATOR) {
            if (writer) {
                if (op != OP_PDF) reinterpret_cast<float2*>(p.out_x)[qe] = make_float2(x0, x1);
                if (op != OP_SAMPLES_ONLY) out_pdf[qe] = pdf;
            }
        } else if (op == OP_SAMPLE) {
            float ox, oy, oz, pdf_sa;
            if (DOMAIN == BSDFD_DOMAIN_DISK) {  // rendering/brdf_measured_disk.py:69-82
                const float r2 = x0 * x0 + x1 * x1;
                const bool ok = r2 < 0.995f;
                ox = ok ? x0 : 0.0f; oy = ok ? x1 : 0.0f;
                oz = sqrtf(fmaxf(1.0f - (ox * ox + oy * oy), 0.0f));
                pdf_sa = (ok ? pdf : 0.0f) * oz;
            } else {  // rendering/brdf_measured_spherical.py:79-91, bsdf_myresult.py:69-84
                float st, ct, sp, cp;
                sincos_enc(x0, st, ct);
                sincos_enc(x1, sp, cp);
                if (!(st > 0.00005f)) pdf = 0.0f;
                if (p.io == IO_PLUGIN && !(ct > 0.0f)) pdf = 0.0f;
                ox = cp * st; oy = sp * st; oz = ct;
                const float inv = fminf(fmaxf(1.0f / sqrtf(ox * ox + oy * oy), 1.0f), 3.402823466e+38f);
                pdf_sa = pdf * inv;
            }
            if (writer) {
                p.out_x[qe * 3 + 0] = ox; p.out_x[qe * 3 + 1] = oy; p.out_x[qe * 3 + 2] = oz;
                out_pdf[qe] = pdf_sa;
            }
        } else {
            float pdf_sa;
            if (DOMAIN == BSDFD_DOMAIN_DISK) {  // rendering/brdf_measured_disk.py:112-124
                pdf_sa = (wi_z > 0.0f && wo_z > 0.0f) ? pdf * wo_z : 0.0f;
            } else {
                const float inv = fminf(fmaxf(1.0f / wo_sin, 1.0f), 3.402823466e+38f);
                if (p.io == IO_PLUGIN) {  // rendering/brdf_measured_spherical.py:122-137
                    if (wo_pole) pdf = 0.0f;   // sin(theta_o) > 0.00005 as the reference's fp32 cart_to_spher decides it
                    pdf_sa = (wi_z > 0.0f && wo_z > 0.0f) ? pdf * inv : 0.0f;
                } else {                  // rendering/bsdf_myresult.py:115-133
                    pdf_sa = pdf * inv;
                }
            }
            if (writer) out_pdf[qe] = pdf_sa;
        }
        }
        if (FUSED && ++ph < nphase) goto next_phase;
    }
    if (p.clk) {
        const unsigned long long dc = (unsigned long long)__builtin_readcyclecounter() - clk_c0;
        const unsigned long long dr = (unsigned long long)__builtin_amdgcn_s_memrealtime() - clk_r0;
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* slot = p.clk + 8 * ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (CLK_SLOTS - 1));
            atomicAdd(slot, dc);
            atomicAdd(slot + 1, dr);
        }
    }
}

// ---- host side of these kernels (flow_kernels.h): their weight image and their instantiation table ----
inline uint16_t f32_to_f16_bits(float x) {
    const _Float16 h = (_Float16)x;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
inline float f16_round(float x) { return (float)(_Float16)x; }

// Build the weight image: every matrix is stored as ready-made MFMA A-fragments in the
// lane order the kernel reads them (see the kernel header for the unit <-> (m, g, r) map).
std::vector<char> build_image(const bsdfd_desc& d_in, int prec, ImgLayout& L) {
    // scaled pre-activation convention (see silu_grad_scaled): first layer x -log2(e), output layer x -ln 2
    bsdfd_desc d = d_in;
    const int sd_ = d.domain == BSDFD_DOMAIN_DISK ? 2 : 3;
    std::vector<float> w_in_s((size_t)d.width * (sd_ + 1 + 2 + 4 * PE_BANDS)), w_out_s((size_t)2 * d.width);
    for (size_t i = 0; i < w_in_s.size(); ++i) w_in_s[i] = (float)((double)d_in.w_in[i] * -1.4426950408889634);
    for (size_t i = 0; i < w_out_s.size(); ++i) w_out_s[i] = (float)((double)d_in.w_out[i] * -0.6931471805599453);
    d.w_in = w_in_s.data();
    d.w_out = w_out_s.data();
    const int W = d.width, NM = W / 16, NH = d.n_hidden, KC = NM / 2;
    const int SD = d.domain == BSDFD_DOMAIN_DISK ? 2 : 3;
    const int IN = SD + 1 + 2 + 4 * PE_BANDS;
    const int BIN = 2 + 4 * BASE_PE_BANDS;
    auto align16 = [](int x) { return (x + 15) & ~15; };
    int off = 0;
    L.win = off; off += NM * 64 * 4;
    L.wc = off; off += NM * PE_SLABS * 64 * 4;
    if (prec == BSDFD_PREC_F32) {
        L.wh = off; off += (NH - 1) * NM * NM * 64 * 16;
        L.wh_lo = L.wh;
        L.wo = off; off += NM * 64 * 16;
    } else {
        L.wh = off; off += (NH - 1) * NM * KC * 64 * 16;
        L.wh_lo = off;
        if (prec == BSDFD_PREC_SPLIT3) off += (NH - 1) * NM * KC * 64 * 16;
        L.wo = off; off += KC * 64 * 16;
    }
    L.wf = L.wf_lo = L.wg = L.wg_lo = 0;
    // folded layer-1 tangent matrices W2 diag(W1[:, i]), i = 0, 1, of the disk nets (FOLD_L1 in the kernel)
    const bool fold = d.domain == BSDFD_DOMAIN_DISK && prec != BSDFD_PREC_F32 && NH >= 2 && NM == 2;
    const int NFOLD = 2;
    // ... and the output side folded the same way (MIM in the kernel), with W_L the last hidden-to-hidden matrix:
    // G_j = W_L^T diag(Wout[j, :]), j = 0, 1, so that (Wout D_L W_L)^T[:, j] = G_j g_L
    // (disk 25-32x3-2 and spherical 26-32x4-2: the two nets the reference's plugins load)
    // (disk 25-32x3-2 and spherical 26-32x4-2: the two nets the reference's plugins load — compile-time fragment offsets; and
    //  the 64 x 6 spherical net, which has a depth-unrolled instantiation: FOLDOUT in the kernel, run-time offsets)
    const bool mim32 = prec != BSDFD_PREC_F32 && NM == 2 &&
                       ((d.domain == BSDFD_DOMAIN_DISK && NH == 3) || (d.domain == BSDFD_DOMAIN_SPHERICAL && NH == 4));
    const bool mim = mim32 || (prec != BSDFD_PREC_F32 && NM == 4 && NH == 6 && d.domain == BSDFD_DOMAIN_SPHERICAL);
    if (fold) {
        L.wf = off; off += NFOLD * NM * KC * 64 * 16;
        L.wf_lo = off;
        if (prec == BSDFD_PREC_SPLIT3) off += NFOLD * NM * KC * 64 * 16;
    }
    if (mim) {
        L.wg = off; off += NFOLD * NM * KC * 64 * 16;
        L.wg_lo = off;
        if (prec == BSDFD_PREC_SPLIT3) off += NFOLD * NM * KC * 64 * 16;
        // the MIM kernels address their fragments with compile-time offsets: keep the two in step
        if (mim32) {
        const int fr = 64 * 16, o_wh = NM * 64 * 4 + NM * PE_SLABS * 64 * 4, o_whl = o_wh + (NH - 1) * NM * fr;
        const bool sp = prec == BSDFD_PREC_SPLIT3;
        const int o_wo = sp ? o_whl + (NH - 1) * NM * fr : o_whl;
        const int o_wf = fold ? o_wo + fr : 0, o_wfl = fold ? o_wf + 2 * NM * fr : 0;
        const int o_wg = fold ? (sp ? o_wfl + 2 * NM * fr : o_wfl) : o_wo + fr, o_wgl = o_wg + 2 * NM * fr;
        if (L.wh != o_wh || L.wh_lo != o_whl || L.wo != o_wo || L.wf != o_wf || L.wf_lo != o_wfl || L.wg != o_wg ||
            L.wg_lo != o_wgl) {
            L.total = -1;  // reported by bsdfd_create as an error: never launch a kernel whose fragment offsets are wrong
            return {};
        }
        }
    }
    L.bw1 = off; off += (BASE_PE_BANDS + 1) * 64 * 4;
    L.bb1 = off; off += 64 * 16;
    L.bw2 = off; off += 64 * 16;
    L.bb2 = off; off += 16;
    // conditioning weights as fp16 hi / lo A-fragments (split3; SPLIT_PRO in the kernel): K slot (g, j) of lane group g =
    // encoded value (band j, fn g >> 1, dim g & 1) for j < 5, the raw coordinate y_g for j = 5 and g < 2, else zero.
    // Appended BEHIND everything else so that the MIM kernels' compile-time fragment offsets do not move.
    L.wcs = L.wcs_lo = 0;
    if (prec == BSDFD_PREC_SPLIT3) {
        L.wcs = off; off += NM * 64 * 16;
        L.wcs_lo = off; off += NM * 64 * 16;
    }
    // column 0 of the (scaled) layer-1 matrix in the MFMA accumulator layout: lane (g, q) holds units 16 m + 4 g + r (MIMS)
    L.wt0 = off; off += NM * 64 * 16;
    L.total = align16(off);
    std::vector<char> img(L.total, 0);
    auto F = [&](int o) { return reinterpret_cast<float*>(img.data() + o); };
    auto H = [&](int o) { return reinterpret_cast<uint16_t*>(img.data() + o); };

    // PE entry (band b, fn f, dim dd) sits at PE index 2 + 4b + 2f + dd (model.py:26-57)
    for (int l = 0; l < 64; ++l) {
        const int g = l >> 4, i = l & 15;
        for (int m = 0; m < NM; ++m) {
            const int unit = 16 * m + i;
            // state part: k = g -> disk [x0, x1, alpha, 0]; spherical [theta, sin, cos, alpha]
            F(L.win)[m * 64 + l] = (g < SD + 1) ? d.w_in[unit * IN + g] : 0.0f;
            for (int s = 0; s < PE_BANDS; ++s)
                F(L.wc)[(m * PE_SLABS + s) * 64 + l] = d.w_in[unit * IN + SD + 1 + 2 + 4 * s + 2 * (g >> 1) + (g & 1)];
            F(L.wc)[(m * PE_SLABS + PE_BANDS) * 64 + l] = g < 2 ? d.w_in[unit * IN + SD + 1 + g] : 0.0f;
        }
        // base net
        for (int s = 0; s < BASE_PE_BANDS; ++s)
            F(L.bw1)[s * 64 + l] = d.base_w1[i * BIN + 2 + 4 * s + 2 * (g >> 1) + (g & 1)];
        F(L.bw1)[BASE_PE_BANDS * 64 + l] = g < 2 ? d.base_w1[i * BIN + g] : 0.0f;
        for (int r = 0; r < 4; ++r) {
            F(L.bb1)[l * 4 + r] = d.base_b1[4 * g + r];
            F(L.bw2)[l * 4 + r] = d.base_w2[(i & 3) * BASE_HIDDEN + 4 * g + r];
        }
    }
    for (int r = 0; r < 4; ++r) F(L.bb2)[r] = d.base_b2[r];
    for (int m = 0; m < NM; ++m)
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) F(L.wt0)[(m * 64 + l) * 4 + r] = d.w_in[(16 * m + 4 * (l >> 4) + r) * IN + 0];
    if (prec == BSDFD_PREC_SPLIT3)
        for (int m = 0; m < NM; ++m)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int g = l >> 4, unit = 16 * m + (l & 15);
                    float w = 0.0f;
                    if (j < PE_BANDS) w = d.w_in[unit * IN + SD + 1 + 2 + 4 * j + 2 * (g >> 1) + (g & 1)];
                    else if (j == PE_BANDS && g < 2) w = d.w_in[unit * IN + SD + 1 + g];
                    const float hi = f16_round(w);
                    H(L.wcs)[((size_t)m * 64 + l) * 8 + j] = f32_to_f16_bits(w);
                    H(L.wcs_lo)[((size_t)m * 64 + l) * 8 + j] = f32_to_f16_bits(w - hi);
                }

    if (prec == BSDFD_PREC_F32) {
        for (int layer = 0; layer < NH - 1; ++layer)
            for (int mo = 0; mo < NM; ++mo)
                for (int m = 0; m < NM; ++m)
                    for (int l = 0; l < 64; ++l)
                        for (int r = 0; r < 4; ++r)
                            F(L.wh)[((((size_t)layer * NM + mo) * NM + m) * 64 + l) * 4 + r] =
                                d.w_hidden[((size_t)layer * W + 16 * mo + (l & 15)) * W + 16 * m + 4 * (l >> 4) + r];
        for (int m = 0; m < NM; ++m)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int o = (l & 15) & 3;
                    F(L.wo)[(m * 64 + l) * 4 + r] = o < 2 ? d.w_out[o * W + 16 * m + 4 * (l >> 4) + r] : 0.0f;
                }
    } else {
        for (int layer = 0; layer < NH - 1; ++layer)
            for (int mo = 0; mo < NM; ++mo)
                for (int kc = 0; kc < KC; ++kc)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int k = 16 * (2 * kc + (j >> 2)) + 4 * (l >> 4) + (j & 3);
                            const float w = d.w_hidden[((size_t)layer * W + 16 * mo + (l & 15)) * W + k];
                            const size_t idx = ((((size_t)layer * NM + mo) * KC + kc) * 64 + l) * 8 + j;
                            const float hi = f16_round(w);
                            H(L.wh)[idx] = f32_to_f16_bits(w);
                            if (prec == BSDFD_PREC_SPLIT3) H(L.wh_lo)[idx] = f32_to_f16_bits(w - hi);
                        }
        if (fold)
            for (int i = 0; i < NFOLD; ++i)
                for (int mo = 0; mo < NM; ++mo)
                    for (int kc = 0; kc < KC; ++kc)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 8; ++j) {
                                const int k = 16 * (2 * kc + (j >> 2)) + 4 * (l >> 4) + (j & 3);
                                // (W2 diag(w_i))[unit][k] in double; w_i = the scaled layer-1 column (what zt{0,1}c hold)
                                const double v = (double)d.w_hidden[((size_t)16 * mo + (l & 15)) * W + k] * (double)d.w_in[(size_t)k * IN + i];
                                const size_t idx = ((((size_t)i * NM + mo) * KC + kc) * 64 + l) * 8 + j;
                                const float hi = f16_round((float)v);
                                H(L.wf)[idx] = f32_to_f16_bits((float)v);
                                if (prec == BSDFD_PREC_SPLIT3) H(L.wf_lo)[idx] = f32_to_f16_bits((float)(v - (double)hi));
                            }
        if (mim)
            for (int i = 0; i < NFOLD; ++i)
                for (int mo = 0; mo < NM; ++mo)
                    for (int kc = 0; kc < KC; ++kc)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 8; ++j) {
                                const int k = 16 * (2 * kc + (j >> 2)) + 4 * (l >> 4) + (j & 3);  // unit of the LAST hidden layer (contraction index)
                                const int unit = 16 * mo + (l & 15);                                // unit of the layer before it (row of G_i)
                                // G_i[unit][k] = W_L[k][unit] * Wout[i][k], Wout already scaled by -ln 2 (d.w_out)
                                const double v = (double)d.w_hidden[((size_t)(NH - 2) * W + k) * W + unit] * (double)d.w_out[(size_t)i * W + k];
                                const size_t idx = ((((size_t)i * NM + mo) * KC + kc) * 64 + l) * 8 + j;
                                const float hi = f16_round((float)v);
                                H(L.wg)[idx] = f32_to_f16_bits((float)v);
                                if (prec == BSDFD_PREC_SPLIT3) H(L.wg_lo)[idx] = f32_to_f16_bits((float)(v - (double)hi));
                            }
        for (int kc = 0; kc < KC; ++kc)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * (2 * kc + (j >> 2)) + 4 * (l >> 4) + (j & 3);
                    const int o = (l & 15) & 3;
                    const float w = d.w_out[(o & 1) * W + k];
                    float val;
                    if (o < 2) val = w;
                    else val = (prec == BSDFD_PREC_SPLIT3) ? (w - f16_round(w)) * (float)BSDFD_WO_LO_SCALE : 0.0f;   // (see kWoLoInv)
                    H(L.wo)[((size_t)kc * 64 + l) * 8 + j] = f32_to_f16_bits(val);
                }
    }
    return img;
}

// kernel instantiation table: (domain, width/16, precision, Jacobian) x {generic depth, the reference's depths}
template <int DOMAIN, int NM, int NH>
const void* kernel_ptr_prec(int prec, int mode) {  // mode 0: no Jacobian, 1: Jacobian, 2: Jacobian + fused sample/pdf
#define BSDFD_K(P, H)                                                                                      \
    (mode == 0   ? reinterpret_cast<const void*>(flow_kernel<DOMAIN, NM, P, false, H, false>)                \
     : mode == 1 ? reinterpret_cast<const void*>(flow_kernel<DOMAIN, NM, P, true, H, false>)                 \
                 : reinterpret_cast<const void*>(flow_kernel<DOMAIN, NM, P, true, H, true>))
    switch (prec) {
        case BSDFD_PREC_F32: return BSDFD_K(BSDFD_PREC_F32, 0);
        case BSDFD_PREC_F16: return BSDFD_K(BSDFD_PREC_F16, NH);
        default: return BSDFD_K(BSDFD_PREC_SPLIT3, NH);
    }
#undef BSDFD_K
}
const void* kernel_ptr(int domain, int nm, int n_hidden, int prec, int mode) {
    if (domain == BSDFD_DOMAIN_DISK) {
        if (nm == 2) return n_hidden == 3 ? kernel_ptr_prec<BSDFD_DOMAIN_DISK, 2, 3>(prec, mode)
                                          : kernel_ptr_prec<BSDFD_DOMAIN_DISK, 2, 0>(prec, mode);
        return kernel_ptr_prec<BSDFD_DOMAIN_DISK, 4, 0>(prec, mode);
    }
    if (nm == 2) return n_hidden == 4 ? kernel_ptr_prec<BSDFD_DOMAIN_SPHERICAL, 2, 4>(prec, mode)
                                      : kernel_ptr_prec<BSDFD_DOMAIN_SPHERICAL, 2, 0>(prec, mode);
    // other 64-wide depths keep the run-time layer loop
    // the reference's 64 x 6 teacher (NN_cond_pos_spherical_complicate) gets a depth-unrolled instantiation too: with the
    // per-step LDS re-read of the fragments (see the Euler loop) it needs 121 (fp16) / 231 (split3) VGPRs and no scratch;
    // A/B against the run-time-depth kernel: teacher -1.4 %, split3 -0.2 .. -2 % (profiles/r02_ab/ab6)
    if (n_hidden == 6) return kernel_ptr_prec<BSDFD_DOMAIN_SPHERICAL, 4, 6>(prec, mode);
    return kernel_ptr_prec<BSDFD_DOMAIN_SPHERICAL, 4, 0>(prec, mode);
}
inline int threads_for(int nm) { return nm == 2 ? 256 : 512; }

}  // namespace

std::vector<char> bsdfd_build_image16(const bsdfd_desc& d, int prec, ImgLayout& L) { return build_image(d, prec, L); }
FlowKernel bsdfd_kernel16(const bsdfd_desc& d, int prec, int mode, const ImgLayout& L) {
    return {kernel_ptr(d.domain, d.width / 16, d.n_hidden, prec, mode), 16, threads_for(d.width / 16), L.total, false};
}

const char* bsdfd_flow_variant() { return BSDFD_LDS_VARIANT BSDFD_SIGMOID_VARIANT; }
