// live.hip — the live lanes of a wavefront as a row list (ABI 8).
//
// Every plugin method of the Mitsuba protocol takes an `active` mask (rendering/brdf_measured_disk.py:59,64,101,112) and a
// wavefront always carries dead lanes: rays that missed, paths that ended, back-facing wi.  The flow kernels evaluate the rows
// a row index names (bsdfd_opts.row_index), bit for bit as the full call does; this pass turns a mask into that index: an
// ORDER-PRESERVING compaction, three small kernels shaped like bucket.hip with a single bin, all HBM-streaming:
//   mark  : per 4096-row block, the liveness of 64 consecutive rows as one wave ballot (kept as a bit mask in the
//           workspace), the block's live count, and zeros into the dead rows of the callers' result arrays
//   scan  : exclusive scan of the per-block counts (bucket_scan.h with one bin); the total is `count`
//   write : each block re-reads its 64 masks (512 B instead of the mask and direction arrays), scans their popcounts in
//           LDS, ranks every live row inside its wave's mask (mbcnt) and writes its run of `rows` with coalesced stores
// No block waits on another one: the only ordering is the stream order of the three launches.
// 16 Mi lanes with both hemisphere tests: 16 MB + 2 x 192 MB read once, 2 MB of masks written and read, <= 128 MB written.
//
// Also here: bsdfd_plugin_sample_pdf_ex, the single-handle form of the fused sample+pdf call with optional arguments (what a
// masked sample_pdf call goes through).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "bucket_scan.h"
#include "common.h"

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_ROWS = 16;                          // rows per thread, LV_THREADS apart (coalesced loads)
constexpr int LV_CHUNK = LV_THREADS * LV_ROWS;       // rows per block
constexpr int LV_MASKS = LV_CHUNK / 64;              // wave ballots per block: mask k * 4 + wave covers rows k * 256 + wave * 64 ..

// The comparisons are the flow kernels' guards (flow32.hip: `wi_z > 0.0f && wo_z > 0.0f`): NaN and +-0 are dead.
__global__ __launch_bounds__(LV_THREADS) void live_mark_kernel(const unsigned char* __restrict__ active,
                                                               const float* __restrict__ wi, const float* __restrict__ dir,
                                                               int flags, long long n, unsigned long long* __restrict__ masks,
                                                               int* __restrict__ blockcnt, float* __restrict__ zero_wo,
                                                               float* __restrict__ zero_pdf, float* __restrict__ zero_pdf2) {
    __shared__ int wave_total[LV_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row0 = (long long)blockIdx.x * LV_CHUNK;
    int total = 0;
#pragma unroll
    for (int k = 0; k < LV_ROWS; ++k) {
        const long long r = row0 + k * LV_THREADS + threadIdx.x;
        bool live = false;
        if (r < n) {
            live = !active || active[r] != 0;
            if (flags & BSDFD_LIVE_WI_UPPER) live = live && wi[r * 3 + 2] > 0.0f;
            if (flags & BSDFD_LIVE_DIR_UPPER) live = live && dir[r * 3 + 2] > 0.0f;
            if (!live) {
                if (zero_wo) { zero_wo[r * 3 + 0] = 0.0f; zero_wo[r * 3 + 1] = 0.0f; zero_wo[r * 3 + 2] = 0.0f; }
                if (zero_pdf) zero_pdf[r] = 0.0f;
                if (zero_pdf2) zero_pdf2[r] = 0.0f;
            }
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) masks[(long long)blockIdx.x * LV_MASKS + k * (LV_THREADS / 64) + wave] = m;
        total += __popcll(m);
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < LV_THREADS / 64; ++w) s += wave_total[w];
        blockcnt[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(LV_THREADS) void live_write_kernel(const unsigned long long* __restrict__ masks,
                                                                const long long* __restrict__ offs,
                                                                long long* __restrict__ rows) {
    __shared__ unsigned long long smask[LV_MASKS];
    __shared__ int sbase[LV_MASKS + 1];              // live rows of the block before a mask; [LV_MASKS]: the block's total
    __shared__ unsigned short srow[LV_CHUNK];        // the block's live rows (local numbers) in ascending order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {  // LV_MASKS == 64: one mask per lane, popcounts scanned with shuffles
        const unsigned long long m = masks[(long long)blockIdx.x * LV_MASKS + lane];
        const int c = __popcll(m);
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        smask[lane] = m;
        sbase[lane] = incl - c;
        if (lane == 63) sbase[LV_MASKS] = incl;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LV_ROWS; ++k) {
        const int seg = k * (LV_THREADS / 64) + wave;
        const unsigned long long m = smask[seg];
        if ((m >> lane) & 1ull) {
            // rank inside the wave's mask: set bits below this lane
            const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            srow[sbase[seg] + below] = (unsigned short)(k * LV_THREADS + threadIdx.x);
        }
    }
    __syncthreads();
    const int total = sbase[LV_MASKS];
    const long long row0 = (long long)blockIdx.x * LV_CHUNK, out0 = offs[blockIdx.x];
    for (int j = threadIdx.x; j < total; j += LV_THREADS) rows[out0 + j] = row0 + srow[j];
}

static_assert(LV_MASKS == 64, "live_write_kernel scans one mask per lane of a wave");

// workspace: [offs: nblocks x i64][masks: nblocks x 64 x u64][blockcnt: nblocks x i32]
long long live_blocks(long long n) { return n > 0 ? (n + LV_CHUNK - 1) / LV_CHUNK : 1; }

}  // namespace

extern "C" {

int64_t bsdfd_live_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return live_blocks(n) * (long long)(sizeof(long long) + LV_MASKS * sizeof(unsigned long long) + sizeof(int)) + 64;
}

int bsdfd_compact_live(const unsigned char* active, const float* wi, const float* dir, int32_t flags, int64_t n, int64_t* rows,
                       int64_t* count, float* zero_wo, float* zero_pdf, float* zero_pdf2, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (!rows) return bsdfd_fail_(BSDFD_EINVAL, "null rows pointer");
    if (!count) return bsdfd_fail_(BSDFD_EINVAL, "null count pointer");
    if (!workspace) return bsdfd_fail_(BSDFD_EINVAL, "null workspace pointer");
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return bsdfd_fail_(BSDFD_EINVAL, "workspace must be 8-byte aligned");
    if (workspace_bytes < bsdfd_live_workspace_bytes(n))
        return bsdfd_fail_(BSDFD_EINVAL, "workspace smaller than bsdfd_live_workspace_bytes()");
    if (flags & ~(BSDFD_LIVE_WI_UPPER | BSDFD_LIVE_DIR_UPPER))
        return bsdfd_fail_(BSDFD_EINVAL, "unknown bits in flags (BSDFD_LIVE_WI_UPPER | BSDFD_LIVE_DIR_UPPER)");
    if ((flags & BSDFD_LIVE_WI_UPPER) && !wi) return bsdfd_fail_(BSDFD_EINVAL, "BSDFD_LIVE_WI_UPPER needs the wi array");
    if ((flags & BSDFD_LIVE_DIR_UPPER) && !dir) return bsdfd_fail_(BSDFD_EINVAL, "BSDFD_LIVE_DIR_UPPER needs the dir array");
    const long long nblocks = live_blocks(n);
    if (nblocks > 0x7fffffffLL) return bsdfd_fail_(BSDFD_EINVAL, "N too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count, 0, sizeof(int64_t), st));
        return BSDFD_OK;
    }
    long long* offs = static_cast<long long*>(workspace);
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(offs + nblocks);
    int* blockcnt = reinterpret_cast<int*>(masks + nblocks * LV_MASKS);
    const dim3 grid((unsigned)nblocks), block(LV_THREADS);
    hipLaunchKernelGGL(live_mark_kernel, grid, block, 0, st, active, wi, dir, (int)flags, (long long)n, masks, blockcnt, zero_wo,
                       zero_pdf, zero_pdf2);
    hipLaunchKernelGGL(bucket_scan_kernel, dim3(1), dim3(1024), 0, st, blockcnt, nblocks, offs, reinterpret_cast<long long*>(count));
    hipLaunchKernelGGL(live_write_kernel, grid, block, 0, st, masks, offs, reinterpret_cast<long long*>(rows));
    HIP_TRY(hipGetLastError());
    return BSDFD_OK;
}

int bsdfd_plugin_sample_pdf_ex(bsdfd_handle h, int32_t variant, const float* wi, const float* x0, const float* wl, uint64_t seed,
                               uint64_t offset, int64_t n, int32_t T, float* wo, float* pdf_wo, float* pdf_wl,
                               const bsdfd_opts* opts, void* stream) {
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    return bsdfd_plugin_sample_pdf_multi_ex(&h, 1, &n, variant, wi, x0, wl, seed, offset, T, wo, pdf_wo, pdf_wl, opts, stream);
}

}  // extern "C"
