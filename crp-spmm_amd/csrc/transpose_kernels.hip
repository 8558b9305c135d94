// transpose_kernels.hip -- A^T of a CSR on the device, and the C entry point crp_csr_transpose (include/crpspmm_hip.h).
//
// Output rule: row c of A^T lists the rows of A that hold column c, ascending, duplicates of one (row, column) pair in
// their original order -- a stable sort of the nonzeros by column.  Every entry carries the 64-bit key
// (source row << 32 | source position): the keys are distinct, so the order inside an output row is unique and the device
// agrees with the host (csr_transpose.cpp) bit for bit.  Values are moved, never added; the only atomics are on integers.
//
//   pass 1  (one thread per row and per nonzero) the checks that make the later passes safe -- rowptr never decreases,
//           every column lies in [0, ncol) -- and the column counts (atomicAdd on ints: a sum does not depend on the
//           order) into rowptr_t.  A bad input ends the call here: rowptr_t holds counts, nothing else was written.
//   pass 2  output rows longer than one wave are listed by tier; exclusive scan of the counts in place -> rowptr_t
//           (scan_sort.h, shared with permute_kernels.hip).
//   pass 3  fill: one wave per source row, every nonzero takes the next free slot of its column (an atomic cursor) and
//           leaves its key there -- the slots of a column are handed out in whatever order the waves arrive.
//   pass 4  per output row, by length, the keys are sorted and the order becomes the unique one:
//           L <= 64          one wave, one key per lane, bitonic sort across the lanes;
//           64 < L <= 4096   one workgroup, keys in LDS (32 KiB);
//           L > 4096         one workgroup per row at a time, keys in a scratch buffer (padded to a power of two): a dense
//                            column is one output row of nrow entries.
//           Then colidx_t = the key's row, tmap = its position, val_t = val[position].
// Cost: about 44 B per nonzero (4 B read twice, the 8-byte key written and read, 4 + 4 + 8 B written, 8 B gathered).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "crpspmm_hip.h"
#include "csr_transpose.h"
#include "scan_sort.h"

namespace crp {

namespace {

using namespace devsort;
enum { F_PTR = 1, F_COL = 2 };

struct Census
{
    int flags, n_mid, n_long, max_long;
};

// ---- pass 1
__global__ void k_check_count(int nrow, int ncol, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colidx, int *count,
                              Census *cs)
{
    const long long span = nrow > nnz ? nrow : nnz;
    int flags = 0;
    for (long long x = (long long) blockIdx.x * blockDim.x + threadIdx.x; x < span; x += (long long) gridDim.x * blockDim.x)
    {
        if (x < nrow && rowptr[x + 1] < rowptr[x]) flags |= F_PTR;
        if (x < nnz)
        {
            const int c = colidx[x];
            if (c < 0 || c >= ncol) flags |= F_COL;
            else atomicAdd(&count[c], 1);
        }
    }
    if (flags) atomicOr(&cs->flags, flags);
}

// ---- pass 2: the tiers of the output rows (mid rows from the front of lists, long rows from its back)
__global__ void k_tiers(int ncol, const int *__restrict__ count, int *lists, Census *cs)
{
    for (long long x = (long long) blockIdx.x * blockDim.x + threadIdx.x; x < ncol; x += (long long) gridDim.x * blockDim.x)
    {
        const int len = count[x];
        if (len > LDS_PAIRS)
        {
            lists[ncol - 1 - atomicAdd(&cs->n_long, 1)] = (int) x;
            atomicMax(&cs->max_long, len);
        }
        else if (len > WAVE)
            lists[atomicAdd(&cs->n_mid, 1)] = (int) x;
    }
}

// ---- pass 3: keys into the slots of their columns, one wave per source row
__global__ void __launch_bounds__(256) k_fill_keys(int nrow, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                   const int *__restrict__ rowptr_t, int *cursor, uint64_t *keys)
{
    const int lane = threadIdx.x % WAVE, waves = blockDim.x / WAVE;
    for (long long i = (long long) blockIdx.x * waves + threadIdx.x / WAVE; i < nrow; i += (long long) gridDim.x * waves)
    {
        const int p0 = rowptr[i], p1 = rowptr[i + 1];
        for (int p = p0 + lane; p < p1; p += WAVE)
        {
            const int c = colidx[p];
            keys[rowptr_t[c] + atomicAdd(&cursor[c], 1)] = ((uint64_t) (uint32_t) i << 32) | (uint32_t) p;
        }
    }
}

// ---- pass 4
__device__ inline void emit(uint64_t key, int q, const double *val, int *colidx_t, double *val_t, int *tmap)
{
    const int p = (int) (uint32_t) key;
    colidx_t[q] = (int) (key >> 32);
    if (tmap) tmap[q] = p;
    if (val_t) val_t[q] = val[p];
}

// output rows of 1 .. 64 entries: one wave per row, one key per lane
__global__ void __launch_bounds__(256) k_sort_short(int ncol, const int *__restrict__ rowptr_t, const uint64_t *__restrict__ keys,
                                                    const double *__restrict__ val, int *colidx_t, double *val_t, int *tmap)
{
    const int lane = threadIdx.x % WAVE, waves = blockDim.x / WAVE;
    for (long long c = (long long) blockIdx.x * waves + threadIdx.x / WAVE; c < ncol; c += (long long) gridDim.x * waves)
    {
        const int out = rowptr_t[c], len = rowptr_t[c + 1] - out;
        if (len == 0 || len > WAVE) continue;                       // (wave-uniform)
        uint64_t key = lane < len ? keys[out + lane] : PAD;
        key = wave_bitonic(key, lane, pow2_at_least(len));
        if (lane < len) emit(key, out + lane, val, colidx_t, val_t, tmap);
    }
}

__device__ inline void sort_row_in(uint64_t *s, int c, const int *rowptr_t, const uint64_t *keys, const double *val, int *colidx_t,
                                   double *val_t, int *tmap)
{
    const int out = rowptr_t[c], len = rowptr_t[c + 1] - out, np2 = pow2_at_least(len);
    for (int t = threadIdx.x; t < np2; t += blockDim.x) s[t] = t < len ? keys[out + t] : PAD;
    __syncthreads();
    block_bitonic(s, np2);
    for (int t = threadIdx.x; t < len; t += blockDim.x) emit(s[t], out + t, val, colidx_t, val_t, tmap);
    __syncthreads();
}

// output rows of 65 .. LDS_PAIRS entries: one workgroup per row, keys in LDS
__global__ void __launch_bounds__(MID_THREADS) k_sort_mid(const int *__restrict__ list, const int *__restrict__ rowptr_t,
                                                          const uint64_t *__restrict__ keys, const double *__restrict__ val,
                                                          int *colidx_t, double *val_t, int *tmap)
{
    __shared__ uint64_t s[LDS_PAIRS];
    sort_row_in(s, list[blockIdx.x], rowptr_t, keys, val, colidx_t, val_t, tmap);
}

// longer output rows: workgroup b sorts rows b, b + grid, ... in its own scratch slice of `slice` keys
__global__ void __launch_bounds__(LONG_THREADS) k_sort_long(int n_long, const int *__restrict__ list, uint64_t *scratch, long long slice,
                                                            const int *__restrict__ rowptr_t, const uint64_t *__restrict__ keys,
                                                            const double *__restrict__ val, int *colidx_t, double *val_t, int *tmap)
{
    uint64_t *s = scratch + (long long) blockIdx.x * slice;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) sort_row_in(s, list[-r], rowptr_t, keys, val, colidx_t, val_t, tmap);
}

#define TR_TRY(expr)                                            \
    do                                                          \
    {                                                           \
        const hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) { rc = (int) e__; goto done; }   \
    } while (0)

}  // namespace

int csr_transpose_dev(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t, int *colidx_t,
                      double *val_t, int *tmap, void *stream)
{
    const hipStream_t st = (hipStream_t) stream;
    int rc = 0, ends[2] = {0, 0};
    Census cs = {0, 0, 0, 0};
    char *work = nullptr;
    uint64_t *scratch = nullptr, *keys = nullptr;
    const int nb = scan_tiles(ncol + 1);
    int *cursor = nullptr, *lists = nullptr, *bsum = nullptr;
    Census *dcs = nullptr;
    long long span = 0;
    int nnz = 0;

    TR_TRY(hipMemcpyAsync(&ends[0], rowptr, sizeof(int), hipMemcpyDeviceToHost, st));
    TR_TRY(hipMemcpyAsync(&ends[1], rowptr + nrow, sizeof(int), hipMemcpyDeviceToHost, st));
    TR_TRY(hipStreamSynchronize(st));
    if (ends[0] != 0 || ends[1] < 0) return CRP_CSR_T_EPTR;
    nnz = ends[1];
    if (nnz > 0 && (colidx == nullptr || colidx_t == nullptr || (val_t != nullptr && val == nullptr))) return CRP_CSR_T_EARG;

    // work: keys[nnz] | cursor[ncol] | lists[ncol] | bsum[nb] | census
    {
        const size_t kb = sizeof(uint64_t) * (size_t) nnz;
        const size_t bytes = kb + sizeof(int) * ((size_t) ncol * 2 + (size_t) nb) + sizeof(Census);
        TR_TRY(hipMalloc(&work, bytes));
        keys = (uint64_t *) work;
        cursor = (int *) (work + kb);
        lists = cursor + ncol;
        bsum = lists + ncol;
        dcs = (Census *) (bsum + nb);
        if (ncol > 0) TR_TRY(hipMemsetAsync(cursor, 0, sizeof(int) * (size_t) ncol, st));
        TR_TRY(hipMemsetAsync(dcs, 0, sizeof(Census), st));
        TR_TRY(hipMemsetAsync(rowptr_t, 0, sizeof(int) * ((size_t) ncol + 1), st));
    }
    // ---- pass 1 and its verdict
    span = nrow > nnz ? nrow : nnz;
    if (span > 0)
    {
        const long long blocks = std::min<long long>((span + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_check_count, dim3((unsigned) blocks), dim3(256), 0, st, nrow, ncol, nnz, rowptr, colidx, rowptr_t, dcs);
        TR_TRY(hipGetLastError());
    }
    // ---- pass 2 (the tier lists are of no use after a bad input, and do no harm)
    if (ncol > 0 && nnz > 0)
    {
        const long long blocks = std::min<long long>(((long long) ncol + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_tiers, dim3((unsigned) blocks), dim3(256), 0, st, ncol, rowptr_t, lists, dcs);
        TR_TRY(hipGetLastError());
    }
    TR_TRY(hipMemcpyAsync(&cs, dcs, sizeof(Census), hipMemcpyDeviceToHost, st));
    TR_TRY(hipStreamSynchronize(st));
    if (cs.flags)
    {
        rc = (cs.flags & F_PTR) ? CRP_CSR_T_EPTR : CRP_CSR_T_ECOL;     // (the host's order)
        goto done;
    }
    TR_TRY(exclusive_scan_inplace(ncol + 1, rowptr_t, bsum, st));
    if (nnz > 0)
    {
        // ---- pass 3
        {
            const long long blocks = std::min<long long>(((long long) nrow + 3) / 4, 1 << 20);
            hipLaunchKernelGGL(k_fill_keys, dim3((unsigned) blocks), dim3(256), 0, st, nrow, rowptr, colidx, rowptr_t, cursor, keys);
            TR_TRY(hipGetLastError());
        }
        // ---- pass 4
        {
            const long long blocks = std::min<long long>(((long long) ncol + 3) / 4, 1 << 20);
            hipLaunchKernelGGL(k_sort_short, dim3((unsigned) blocks), dim3(256), 0, st, ncol, rowptr_t, keys, val, colidx_t, val_t, tmap);
            TR_TRY(hipGetLastError());
        }
        if (cs.n_mid > 0)
        {
            hipLaunchKernelGGL(k_sort_mid, dim3(cs.n_mid), dim3(MID_THREADS), 0, st, lists, rowptr_t, keys, val, colidx_t, val_t, tmap);
            TR_TRY(hipGetLastError());
        }
        if (cs.n_long > 0)
        {
            long long slice = LDS_PAIRS;
            while (slice < cs.max_long) slice <<= 1;
            const long long budget = (long long) 256 << 20;             // bytes of scratch the call allows itself
            const int grid = (int) std::max<long long>(1, std::min<long long>({(long long) cs.n_long, 256, budget / (slice * 8)}));
            TR_TRY(hipMalloc(&scratch, sizeof(uint64_t) * (size_t) slice * (size_t) grid));
            hipLaunchKernelGGL(k_sort_long, dim3(grid), dim3(LONG_THREADS), 0, st, cs.n_long, lists + ncol - 1, scratch, slice, rowptr_t,
                               keys, val, colidx_t, val_t, tmap);
            TR_TRY(hipGetLastError());
        }
    }
    TR_TRY(hipStreamSynchronize(st));
done:
    if (work || scratch) (void) hipStreamSynchronize(st);
    if (scratch) (void) hipFree(scratch);
    if (work) (void) hipFree(work);
    return rc;
}

}  // namespace crp

extern "C" int crp_csr_transpose(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t,
                                 int *colidx_t, double *val_t, int *tmap, void *stream)
{
    if (nrow < 0 || ncol < 0 || rowptr == nullptr || rowptr_t == nullptr) return CRP_CSR_T_EARG;
    const void *ptrs[7] = {rowptr, colidx, val, rowptr_t, colidx_t, val_t, tmap};
    int ndev = 0, nhost = 0;
    for (const void *p : ptrs)
    {
        if (p == nullptr) continue;
        int is_dev = 0;
        crp_dev_ptr_is_device(p, &is_dev);
        (is_dev ? ndev : nhost)++;
    }
    if (ndev > 0 && nhost > 0) return CRP_CSR_T_EMIXED;
    if (ndev == 0) return crp::csr_transpose_host(nrow, ncol, rowptr, colidx, val, rowptr_t, colidx_t, val_t, tmap);
    return crp::csr_transpose_dev(nrow, ncol, rowptr, colidx, val, rowptr_t, colidx_t, val_t, tmap, stream);
}
