// material_table.h — a table of materials behind the row kernels, whatever the record: what measured_table.hip (records: the
// measured descriptors) and analytic_table.hip (records: a kind and that model's derived descriptor) share.  Device side: the
// wave-uniform pick of a row's record and the row of a list launch.  Host side: the opaque table, its upload and destruction,
// the checks of a launch and the launch.  Each unit keeps what really differs: its records, how create validates its entries,
// and its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "bsdfd.h"
#include "common.h"
#include "rows.h"

namespace material_table {

// The row's material, once: a wave whose live lanes all carry one id (the first live lane's, held as a scalar) addresses the
// record with that scalar and reads it through uniform loads, any other wave per lane.  `use(record)` serves a row whose id
// names a record that `has(record)` ground truth, `none()` every other.  Call with the dead lanes (rows past N) already retired.
// The range check and `has` share one condition per branch, so that each branch has one `use` and one `none`: `use` is the
// whole row, inlined, and a second copy per branch is a second copy of the model.
template <class Rec, class Has, class Use, class None>
__device__ __forceinline__ void with_entry(const Rec* __restrict__ table, int n_materials, long long id, Has has, Use use,
                                           None none) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)id & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)id >> 32));
    const long long first = (long long)(((unsigned long long)hi << 32) | lo);
    if (__ballot(id != first) == 0ull) {
        if (first >= 0 && first < n_materials && has(table[first])) use(table[first]);
        else none();
    } else {
        if (id >= 0 && id < n_materials && has(table[id])) use(table[id]);
        else none();
    }
}

// A launch over a row list: this thread's row q = rows[t] of the N-row arrays; false for a thread past the list and for an entry
// outside [0, N) (a contract violation: skipped, not followed).
__device__ __forceinline__ bool listed_row(const long long* __restrict__ rows, long long n_rows, long long n, long long& q) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows) return false;
    q = rows[t];
    return (unsigned long long)q < (unsigned long long)n;
}

// ---- host side ----
// what the two opaque table types of include/bsdfd.h derive from, each adding its `noun` ("measured table") for the messages
template <class Rec>
struct Ctx {
    Rec* dev;  // [n_materials] on the device
    int32_t n_materials;
    int device;
};

// the last step of a *_table_create, after its validation: the records go to the current device `devid` and are wrapped;
// `what` names them in the copy's error
template <class Table, class Rec>
int upload(const std::vector<Rec>& host, int devid, const char* what, Table** out) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, host.size() * sizeof(Rec)));
    const hipError_t e = hipMemcpy(p, host.data(), host.size() * sizeof(Rec), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return bsdfd_fail_(BSDFD_EHIP, std::string("hipMemcpy of the material ") + what + ": " + hipGetErrorString(e));
    }
    *out = new Table{{static_cast<Rec*>(p), (int32_t)host.size(), devid}};
    return BSDFD_OK;
}

template <class Table>
void destroy(Table* t) {
    if (!t) return;
    (void)hipFree(t->dev);
    delete t;
}

// The host path of every table launcher: the checks of the table and of N, then `kernel` over n_rows threads — one per row
// (n_rows = N), or one per entry of a row list — with the table (as the record type K the kernel reads it through), the ids of
// the N rows and `args` behind them.
template <class Table, class K, class... P, class... A>
int launch(const Table* t, int64_t n, int64_t n_rows, const int64_t* material_id, const char* bad,
           void (*kernel)(const K*, P...), void* stream, A... args) {
    if (!t) return bsdfd_fail_(BSDFD_EINVAL, std::string("null ") + Table::noun);
    if (int rc = rows::launch_checks(n, rows::kMaxRowsTable, Table::noun, &t->device)) return rc;
    if (n_rows < 0 || n_rows > n) return bsdfd_fail_(BSDFD_EINVAL, "n_rows must be in [0, N]");
    return rows::launch_rows(n_rows, bad, kernel, stream, reinterpret_cast<const K*>(t->dev), (int)t->n_materials,
                             reinterpret_cast<const long long*>(material_id), args...);
}

}  // namespace material_table
