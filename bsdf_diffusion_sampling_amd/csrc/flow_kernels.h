// flow_kernels.h — what host.hip (the host side of the library) needs from the two flow-kernel translation units, bsdfd.hip (16-query
// tiles) and flow32.hip (32-query tiles): one record per kernel.  `mode` 0: no Jacobian (flow_samples_only), 1: Jacobian
// (network_sampling / network_pdf / plugin sample / plugin pdf), 2: fused sample+pdf.
#pragma once
#include <vector>

#include "bsdfd.h"

struct ImgLayout;   // flow_dev.h

// A launchable kernel: queries per wave tile, workgroup size, dynamic LDS (>= the weight image it reads).  fn == nullptr: no such kernel
// for this net / precision / mode.  opt_in: it serves its mode only when the caller asked for its tile size EXPLICITLY (bsdfd_desc.tile),
// not under the library's default — the 64 x 6 Jacobian kernel on 32-query tiles, which measured slower than its 16-query counterpart.
struct FlowKernel {
    const void* fn;
    int tile, threads, lds_bytes;
    bool opt_in;
};

// 16-query tiles: a kernel for every net the library accepts.  The weight image with its layout, and the kernel (its LDS = L.total).
std::vector<char> bsdfd_build_image16(const bsdfd_desc& d, int prec, ImgLayout& L);
FlowKernel bsdfd_kernel16(const bsdfd_desc& d, int prec, int mode, const ImgLayout& L);
const char* bsdfd_flow_variant();   // BSDFD_LDS_VARIANT BSDFD_SIGMOID_VARIANT as bsdfd.hip was compiled (bsdfd_version() reports them)

// 32-query tiles.  True where a kernel exists for SOME mode of this net: the reference's two plugin nets — disk 25-32x3-2 (rendering/
// utils/model.py:479-501), spherical 26-32x4-2 (:422-446) — in split3 (all modes); the 64 x 6 spherical teacher (:449-477) in f16 (mode 0)
bool bsdfd_tile32_supported(const bsdfd_desc& d, int prec);
// the weight image of those kernels (fragment order of v_mfma_f32_32x32x16_f16; compile-time offsets, see L32 / L32W in flow32.hip)
std::vector<char> bsdfd_build_image32(const bsdfd_desc& d, int prec);
FlowKernel bsdfd_kernel32(const bsdfd_desc& d, int prec, int mode);   // fn == nullptr: the 16-query-tile kernel serves the mode
// the register-resident fast path of the plain plugin sample / pdf call (op = OP_SAMPLE | OP_PDF), if any: the disk 25-32x3-2 net in
// split3.  Same image, LDS bytes and workgroup size as bsdfd_kernel32(d, prec, 1); 2 waves per SIMD.
FlowKernel bsdfd_kernel32_resident(const bsdfd_desc& d, int prec, int op);
// f32x4 records per 32-query tile of the per-query context the mode-1 kernel of this net writes / reads (bsdfd_context_bytes)
int bsdfd_tile32_context_v4(const bsdfd_desc& d, int prec);
