// bucket_scan.h — the scan step shared by the counting sorts of bucket.hip (<= 64 materials, one pass) and bucket_wide.hip
// (one pass per 6-bit digit): per-block bin totals -> every block's first slot inside its bin, and the bin sizes.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// one block per bin (material / digit value): exclusive scan of the bin's per-block totals (row-local), bucket size
__global__ __launch_bounds__(1024) void bucket_scan_kernel(const int* __restrict__ blockhist, long long nblocks,
                                                           long long* __restrict__ offs, long long* __restrict__ counts) {
    __shared__ long long part[1024];
    const int* row = blockhist + (long long)blockIdx.x * nblocks;
    long long* out = offs + (long long)blockIdx.x * nblocks;
    const long long per = (nblocks + 1023) / 1024;
    const long long b = min((long long)threadIdx.x * per, nblocks), e = min(b + per, nblocks);
    long long s = 0;
    for (long long i = b; i < e; ++i) s += row[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
        const long long v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long acc = part[threadIdx.x] - s;
    for (long long i = b; i < e; ++i) { out[i] = acc; acc += row[i]; }
    if (threadIdx.x == 1023) counts[blockIdx.x] = part[1023];
}

}  // namespace
