// bucket_wide.hip — stable bucketing of a material-tagged wavefront over up to 65536 materials (the scene the reference
// writes as one `mybsdf` instance per material, dispatched lane by lane by Mitsuba: here one sort, then segmented launches).
//
// bucket.hip sorts in one counting pass because its per-thread LDS columns fit 64 bins.  The same pass, applied to one 6-bit
// digit of the id at a time from the lowest digit up (LSD radix sort; every pass is stable, so the whole is), covers
// 64^passes materials: two passes up to 4096, three up to 65536.  Per pass, as in bucket.hip:
//   count   : per 4096-row block, per-thread private columns of an LDS histogram of the digit (no atomics)
//   scan    : per digit value, exclusive scan of its per-block totals (bucket_scan.h)
//   scatter : each block recounts, sorts its rows locally in LDS and writes every (digit, block) run with coalesced stores
// The first pass tests the full 64-bit id against [0, n_materials), drops the rows that fail and writes, next to the
// permutation, the id of every surviving row as 16 bits; the later passes read those 2-byte keys (coalesced) instead of
// gathering 8-byte ids through the permutation, and take the number of surviving rows from the first pass's bin sizes in
// device memory.  The bucket sizes are read off the sorted keys: every run of equal keys adds -start and +end to its counter
// (two integer adds per non-empty bucket, so their order cannot show).
// 16 Mi ids, two passes: 128 MB read twice + 160 MB written, then 32 MB read twice + 128 MB read + 160 MB written.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "bsdfd.h"
#include "bucket_scan.h"
#include "common.h"

namespace {

constexpr int BW_THREADS = 256;
constexpr int BW_ROWS = 16;                         // consecutive rows per thread
constexpr int BW_CHUNK = BW_THREADS * BW_ROWS;      // rows per block
constexpr int BW_BITS = 6;                          // digit width: 64 bins of per-thread columns are what fits in LDS
constexpr int BW_BINS = 1 << BW_BITS;
constexpr int BW_MAX_MATERIALS = 65536;             // ids travel as 16-bit keys after the first pass
constexpr int BW_MAX_PASSES = 3;
// row strides of the per-bin LDS tables, padded as in bucket.hip (the per-bin serial scans fall into different banks)
constexpr int BW_CNT_STRIDE = BW_THREADS + 4;
constexpr int BW_BASE_STRIDE = BW_THREADS + 2;
constexpr unsigned char BW_DROPPED = 255;

__host__ __device__ constexpr size_t bw_scatter_lds(int bins) {
    return (size_t)BW_CHUNK + (size_t)bins * (BW_CNT_STRIDE + 2 * BW_BASE_STRIDE) + (size_t)BW_CHUNK * 4 +
           BW_BINS * sizeof(long long) + (BW_BINS + 1) * sizeof(int);
}

// Rows a pass sorts: all of them in the first pass (bincnt0 == nullptr), afterwards the rows the first pass kept.
__device__ __forceinline__ long long live_rows(const long long* __restrict__ bincnt0, int bins0, long long n) {
    if (!bincnt0) return n;
    long long s = 0;
    for (int b = 0; b < bins0; ++b) s += bincnt0[b];
    return s;
}

// Stage the block's digits into LDS with coalesced loads (u8; BW_DROPPED = not sorted), optionally the 16-bit keys too, then
// count: cnt[d][t] = number of rows with digit d among thread t's 16 consecutive rows (each thread owns its column).
// FIRST: the keys are the callers' int64 ids, tested in full; otherwise the previous pass's 16-bit keys, all valid.
template <bool FIRST>
__device__ __forceinline__ void stage_and_count(const long long* __restrict__ ids, const unsigned short* __restrict__ kin,
                                                long long n_live, long long row0, int M, int shift, int bins,
                                                unsigned char* lid, unsigned short* lkey, unsigned char* cnt) {
    for (int i = threadIdx.x; i < bins * BW_CNT_STRIDE / 4; i += BW_THREADS) reinterpret_cast<unsigned*>(cnt)[i] = 0u;
#pragma unroll
    for (int k = 0; k < BW_ROWS; ++k) {
        const int j = k * BW_THREADS + threadIdx.x;
        const long long r = row0 + j;
        bool ok;
        unsigned key;
        if (FIRST) {
            const long long m = r < n_live ? ids[r] : -1;
            ok = m >= 0 && m < M;
            key = (unsigned)m;
        } else {
            ok = r < n_live;
            key = ok ? kin[r] : 0u;
        }
        lid[j] = ok ? (unsigned char)((key >> shift) & (BW_BINS - 1)) : BW_DROPPED;
        if (lkey) lkey[j] = (unsigned short)key;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BW_ROWS; ++k) {
        const unsigned char d = lid[threadIdx.x * BW_ROWS + k];
        if (d != BW_DROPPED) cnt[d * BW_CNT_STRIDE + threadIdx.x]++;
    }
    __syncthreads();
}

template <bool FIRST>
__global__ __launch_bounds__(BW_THREADS) void wide_count_kernel(const long long* __restrict__ ids,
                                                                const unsigned short* __restrict__ kin, long long n,
                                                                const long long* __restrict__ bincnt0, int bins0, int M,
                                                                int shift, int bins, long long nblocks,
                                                                int* __restrict__ blockhist) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* lid = smem;
    unsigned char* cnt = smem + BW_CHUNK;
    stage_and_count<FIRST>(ids, kin, live_rows(bincnt0, bins0, n), (long long)blockIdx.x * BW_CHUNK, M, shift, bins, lid,
                           nullptr, cnt);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = wave; d < bins; d += BW_THREADS / 64) {  // four u8 counters per word, each <= 16
        const unsigned v = *reinterpret_cast<const unsigned*>(cnt + d * BW_CNT_STRIDE + lane * 4);
        int total = (int)((v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) total += __shfl_xor(total, o, 64);
        if (lane == 0) blockhist[(long long)d * nblocks + blockIdx.x] = total;
    }
}

// pin / pout: the permutation so far (unused in the first pass, where a row is its own source) and after this pass;
// kout: the keys in the order of pout.
template <bool FIRST>
__global__ __launch_bounds__(BW_THREADS) void wide_scatter_kernel(
    const long long* __restrict__ ids, const unsigned short* __restrict__ kin, const long long* __restrict__ pin, long long n,
    const long long* __restrict__ bincnt0, int bins0, int M, int shift, int bins, long long nblocks,
    const long long* __restrict__ offs, const long long* __restrict__ bincnt, long long* __restrict__ pout,
    unsigned short* __restrict__ kout) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* lid = smem;                                                            // [4096] staged digits
    unsigned char* cnt = lid + BW_CHUNK;                                                  // [bins][256]
    unsigned short* base = reinterpret_cast<unsigned short*>(cnt + bins * BW_CNT_STRIDE);  // [bins][256] -> local positions
    unsigned short* srow = base + bins * BW_BASE_STRIDE;                                  // [4096] rows in digit order
    unsigned short* lkey = srow + BW_CHUNK;                                               // [4096] staged keys
    long long* gbase = reinterpret_cast<long long*>(lkey + BW_CHUNK);                     // [bins] first slot of (digit, block)
    int* lstart = reinterpret_cast<int*>(gbase + BW_BINS);                                // [bins+1] local start of a digit
    const long long row0 = (long long)blockIdx.x * BW_CHUNK;
    const long long n_live = live_rows(bincnt0, bins0, n);
    if (row0 >= n_live) return;  // (uniform) a block behind the last surviving row has nothing to place
    stage_and_count<FIRST>(ids, kin, n_live, row0, M, shift, bins, lid, lkey, cnt);
    // exclusive scan of every digit's column counts over the 256 threads: one wave per digit at a time, a lane takes 4
    // adjacent columns (one LDS word) and the lanes' sums are scanned with shuffles
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = wave; d < bins; d += BW_THREADS / 64) {
        const unsigned v = *reinterpret_cast<const unsigned*>(cnt + d * BW_CNT_STRIDE + lane * 4);
        const unsigned c0 = v & 0xff, c1 = (v >> 8) & 0xff, c2 = (v >> 16) & 0xff, c3 = v >> 24;
        const unsigned tot = c0 + c1 + c2 + c3;
        unsigned incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const unsigned excl = incl - tot;
        unsigned short* b = base + d * BW_BASE_STRIDE + lane * 4;
        b[0] = (unsigned short)excl; b[1] = (unsigned short)(excl + c0);
        b[2] = (unsigned short)(excl + c0 + c1); b[3] = (unsigned short)(excl + c0 + c1 + c2);
        if (lane == 63) lstart[d + 1] = (int)incl;
    }
    if (wave == 0) {  // first slot of (digit, block) = bins before the digit + blocks before this one
        const long long c = lane < bins ? bincnt[lane] : 0;
        long long incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane < bins) gbase[lane] = incl - c + offs[(long long)lane * nblocks + blockIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lstart[0] = 0;
        for (int d = 0; d < bins; ++d) lstart[d + 1] += lstart[d];
    }
    __syncthreads();
    // locally sorted order (stable: threads own consecutive rows, columns were scanned in thread order)
#pragma unroll
    for (int k = 0; k < BW_ROWS; ++k) {
        const int j = threadIdx.x * BW_ROWS + k;
        const unsigned char d = lid[j];
        if (d != BW_DROPPED) srow[lstart[d] + base[d * BW_BASE_STRIDE + threadIdx.x]++] = (unsigned short)j;
    }
    __syncthreads();
    // coalesced write-out: consecutive local positions of a digit are consecutive slots of pout / kout
    const int total = lstart[bins];
    for (int j = threadIdx.x; j < total; j += BW_THREADS) {
        const int s = srow[j];
        const unsigned key = lkey[s];
        const int d = (key >> shift) & (BW_BINS - 1);
        const long long dst = gbase[d] + (j - lstart[d]);
        pout[dst] = FIRST ? row0 + s : pin[row0 + s];
        kout[dst] = (unsigned short)key;
    }
}

// Bucket sizes from the sorted keys (counts zeroed beforehand): the row that opens a run of equal keys subtracts its
// position, the row that closes it adds the position behind it.
__global__ __launch_bounds__(BW_THREADS) void wide_sizes_kernel(const unsigned short* __restrict__ keys, long long n,
                                                                const long long* __restrict__ bincnt0, int bins0,
                                                                unsigned long long* __restrict__ counts) {
    const long long k = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
    const long long n_live = live_rows(bincnt0, bins0, n);
    if (k >= n_live) return;
    const unsigned short key = keys[k];
    if (k == 0 || keys[k - 1] != key) atomicAdd(&counts[key], 0ull - (unsigned long long)k);
    if (k == n_live - 1 || keys[k + 1] != key) atomicAdd(&counts[key], (unsigned long long)k + 1ull);
}

int wide_passes(int n_materials) {
    int p = 1;
    while (p < BW_MAX_PASSES && (1 << (BW_BITS * p)) < n_materials) ++p;
    return p;
}

// workspace: [spare permutation: N x i64, two passes and up][offs: 64 x nblocks x i64][bin sizes: passes x 64 x i64]
//            [blockhist: 64 x nblocks x i32][keys: 2 x N x u16, each padded to 8 B]
struct WideLayout {
    long long nblocks, spare, table, keys;
    long long bytes() const {
        return spare * 8 + table * 8 + (long long)BW_MAX_PASSES * BW_BINS * 8 + table * 4 + 2 * keys;
    }
};
WideLayout wide_layout(long long n, int n_materials) {
    WideLayout w;
    w.nblocks = (n + BW_CHUNK - 1) / BW_CHUNK;
    w.spare = wide_passes(n_materials) > 1 ? n : 0;
    w.table = (long long)BW_BINS * (w.nblocks > 0 ? w.nblocks : 1);  // (a multiple of 64 entries: the keys stay 8-byte aligned)
    w.keys = (n * 2 + 7) / 8 * 8;
    return w;
}

}  // namespace

extern "C" {

int64_t bsdfd_bucket_wide_workspace_bytes(int64_t n, int32_t n_materials) {
    if (n < 0 || n_materials < 1 || n_materials > BW_MAX_MATERIALS) return 0;
    return wide_layout(n, n_materials).bytes() + 64;
}

int bsdfd_bucket_by_material_wide(const int64_t* material_id, int64_t n, int32_t n_materials, int64_t* perm, int64_t* counts,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (n < 0) return bsdfd_fail_(BSDFD_EINVAL, "N must be >= 0");
    if (n_materials < 1 || n_materials > BW_MAX_MATERIALS)
        return bsdfd_fail_(BSDFD_EINVAL, "n_materials must be in [1, 65536]");
    if (!counts) return bsdfd_fail_(BSDFD_EINVAL, "null counts pointer");
    if (n > 0) {
        if (!material_id) return bsdfd_fail_(BSDFD_EINVAL, "null material_id pointer");
        if (!perm) return bsdfd_fail_(BSDFD_EINVAL, "null perm pointer");
        if (!workspace) return bsdfd_fail_(BSDFD_EINVAL, "null workspace pointer");
        if (reinterpret_cast<uintptr_t>(workspace) % 8) return bsdfd_fail_(BSDFD_EINVAL, "workspace must be 8-byte aligned");
        if (workspace_bytes < bsdfd_bucket_wide_workspace_bytes(n, n_materials))
            return bsdfd_fail_(BSDFD_EINVAL, "workspace smaller than bsdfd_bucket_wide_workspace_bytes()");
    }
    const WideLayout w = wide_layout(n, n_materials);
    if (w.nblocks > 0x7fffffffLL / BW_ROWS) return bsdfd_fail_(BSDFD_EINVAL, "N too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * n_materials, st));
    if (n == 0) return BSDFD_OK;
    long long* spare = static_cast<long long*>(workspace);
    long long* offs = spare + w.spare;
    long long* bincnt = offs + w.table;
    int* blockhist = reinterpret_cast<int*>(bincnt + BW_MAX_PASSES * BW_BINS);
    unsigned short* keys[2] = {reinterpret_cast<unsigned short*>(blockhist + w.table), nullptr};
    keys[1] = keys[0] + w.keys / 2;
    const long long* ids = reinterpret_cast<const long long*>(material_id);
    long long* out = reinterpret_cast<long long*>(perm);
    // ~71 KB of dynamic LDS at 64 bins: above the default cap, needs the attribute (once per process)
    static const hipError_t attr_rc[2] = {
        hipFuncSetAttribute(reinterpret_cast<const void*>(wide_scatter_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bw_scatter_lds(BW_BINS)),
        hipFuncSetAttribute(reinterpret_cast<const void*>(wide_scatter_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bw_scatter_lds(BW_BINS))};
    HIP_TRY(attr_rc[0]);
    HIP_TRY(attr_rc[1]);
    const int passes = wide_passes(n_materials);
    const dim3 grid((unsigned)w.nblocks), block(BW_THREADS);
    int bins0 = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = BW_BITS * p;
        const int bins = p + 1 < passes ? BW_BINS : ((n_materials - 1) >> shift) + 1;  // the top digit may not use them all
        if (p == 0) bins0 = bins;
        long long* pout = (passes - 1 - p) % 2 == 0 ? out : spare;   // the last pass lands in perm
        const long long* pin = pout == out ? spare : out;
        long long* cnt_p = bincnt + p * BW_BINS;
        const size_t lds_count = (size_t)BW_CHUNK + (size_t)bins * BW_CNT_STRIDE;
        if (p == 0) {
            hipLaunchKernelGGL(wide_count_kernel<true>, grid, block, lds_count, st, ids, nullptr, (long long)n, nullptr, 0,
                               (int)n_materials, shift, bins, w.nblocks, blockhist);
            hipLaunchKernelGGL(bucket_scan_kernel, dim3((unsigned)bins), dim3(1024), 0, st, blockhist, w.nblocks, offs, cnt_p);
            hipLaunchKernelGGL(wide_scatter_kernel<true>, grid, block, bw_scatter_lds(bins), st, ids, nullptr, nullptr,
                               (long long)n, nullptr, 0, (int)n_materials, shift, bins, w.nblocks, offs, cnt_p, pout, keys[0]);
        } else {
            hipLaunchKernelGGL(wide_count_kernel<false>, grid, block, lds_count, st, nullptr, keys[(p - 1) & 1], (long long)n,
                               bincnt, bins0, (int)n_materials, shift, bins, w.nblocks, blockhist);
            hipLaunchKernelGGL(bucket_scan_kernel, dim3((unsigned)bins), dim3(1024), 0, st, blockhist, w.nblocks, offs, cnt_p);
            hipLaunchKernelGGL(wide_scatter_kernel<false>, grid, block, bw_scatter_lds(bins), st, nullptr, keys[(p - 1) & 1], pin,
                               (long long)n, bincnt, bins0, (int)n_materials, shift, bins, w.nblocks, offs, cnt_p, pout,
                               keys[p & 1]);
        }
    }
    hipLaunchKernelGGL(wide_sizes_kernel, dim3((unsigned)((n + BW_THREADS - 1) / BW_THREADS)), block, 0, st,
                       keys[(passes - 1) & 1], (long long)n, bincnt, bins0, reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return BSDFD_OK;
}

}  // extern "C"
