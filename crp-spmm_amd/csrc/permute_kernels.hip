// permute_kernels.hip -- the symmetric permutation P A P^T of a square CSR on the device (include/crp_part.h), and
// the C entry points crp_csr_permute_sym / crp_graph_row_partition.
//
// Output rule: row perm[i] receives row i's entries with columns perm[c], ascending inside the row, duplicate
// columns in their original order.  Every entry is sorted by the 64-bit key (perm[c] << 32 | position in the row):
// the keys of a row are distinct, so the order is unique and the device agrees with the host (graph_part.cpp) bit
// for bit.  The values follow their keys after the sort.
//
//   pass 1  (one thread per row and per nonzero): row lengths scattered to len1[perm[i]] -- kept in rowptr1 --
//           with the checks that make the later passes safe: rowptr never decreases, every target of perm is hit
//           exactly once, every column lies in [0, nrow).  Rows longer than one wave are listed by tier.  The flags
//           and the tier counts go back to the host; a bad input ends the call here, nothing else is read.
//   pass 2  exclusive scan of len1 in place -> rowptr1 (tile sums, one workgroup over the tile sums, tiles again).
//   pass 3  per row, by length:
//           L <= 64          one wave, one key per lane, bitonic sort across the lanes (__shfl_xor);
//           64 < L <= 4096   one workgroup, keys in LDS (32 KiB), bitonic sort;
//           L > 4096         one workgroup per row at a time, keys in a scratch buffer in device memory that the
//                            call allocates (padded to a power of two) and frees.
// Cost: about 24-30 B per nonzero (12 B read, 12 B written, the 4-byte perm gathers) plus the sorts' on-chip work.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "crp_part.h"
#include "crpspmm_hip.h"
#include "graph_part.h"
#include "scan_sort.h"

namespace crp {

namespace {

using namespace devsort;                // scan_sort.h: the tier limits, the scan, the sorts' building blocks
enum { F_PTR = 1, F_PERM = 2, F_COL = 4 };

struct Census
{
    int flags, n_mid, n_long, max_long;
};

__device__ inline uint64_t row_key(const int *perm, const int *colidx, int in, int t)
{
    return ((uint64_t) (uint32_t) perm[colidx[in + t]] << 32) | (uint32_t) t;
}

// ---- pass 1
__global__ void k_scatter_lengths(int nrow, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                  const int *__restrict__ perm, int *len1, int *hit, int *lists, Census *cs)
{
    const long long span = nrow > nnz ? nrow : nnz;
    int flags = 0;
    for (long long x = (long long) blockIdx.x * blockDim.x + threadIdx.x; x < span; x += (long long) gridDim.x * blockDim.x)
    {
        if (x < nrow)
        {
            const int i = (int) x, len = rowptr[i + 1] - rowptr[i], t = perm[i];
            if (len < 0) flags |= F_PTR;
            if (t < 0 || t >= nrow) flags |= F_PERM;
            else
            {
                if (atomicAdd(&hit[t], 1) != 0) flags |= F_PERM;
                len1[t] = len;
            }
            if (len > LDS_PAIRS)
            {
                lists[nrow - 1 - atomicAdd(&cs->n_long, 1)] = i;
                atomicMax(&cs->max_long, len);
            }
            else if (len > WAVE)
                lists[atomicAdd(&cs->n_mid, 1)] = i;
        }
        if (x < nnz)
        {
            const int c = colidx[x];
            if (c < 0 || c >= nrow) flags |= F_COL;
        }
    }
    if (flags) atomicOr(&cs->flags, flags);
}

// ---- pass 2: the exclusive scan of scan_sort.h

// ---- pass 3
// rows of 1 .. 64 entries: one wave per row, one key per lane
__global__ void __launch_bounds__(256) k_sort_short(int nrow, const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                    const double *__restrict__ val, const int *__restrict__ perm,
                                                    const int *__restrict__ rowptr1, int *colidx1, double *val1)
{
    const int lane = threadIdx.x % WAVE, waves = blockDim.x / WAVE;
    for (long long i0 = (long long) blockIdx.x * waves + threadIdx.x / WAVE; i0 < nrow; i0 += (long long) gridDim.x * waves)
    {
        const int i = (int) i0, in = rowptr[i], len = rowptr[i + 1] - in;
        if (len == 0 || len > WAVE) continue;                       // (wave-uniform)
        const int out = rowptr1[perm[i]], np2 = pow2_at_least(len);
        uint64_t key = lane < len ? row_key(perm, colidx, in, lane) : PAD;
        key = wave_bitonic(key, lane, np2);
        if (lane < len)
        {
            colidx1[out + lane] = (int) (key >> 32);
            val1[out + lane] = val[in + (int) (uint32_t) key];
        }
    }
}

__device__ inline void sort_row_in(uint64_t *s, int i, const int *rowptr, const int *colidx, const double *val, const int *perm,
                                   const int *rowptr1, int *colidx1, double *val1)
{
    const int in = rowptr[i], len = rowptr[i + 1] - in, out = rowptr1[perm[i]], np2 = pow2_at_least(len);
    for (int t = threadIdx.x; t < np2; t += blockDim.x) s[t] = t < len ? row_key(perm, colidx, in, t) : PAD;
    __syncthreads();
    block_bitonic(s, np2);
    for (int t = threadIdx.x; t < len; t += blockDim.x)
    {
        const uint64_t key = s[t];
        colidx1[out + t] = (int) (key >> 32);
        val1[out + t] = val[in + (int) (uint32_t) key];
    }
    __syncthreads();
}

// rows of 65 .. LDS_PAIRS entries: one workgroup per row, keys in LDS
__global__ void __launch_bounds__(MID_THREADS) k_sort_mid(const int *__restrict__ list, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colidx, const double *__restrict__ val,
                                                          const int *__restrict__ perm, const int *__restrict__ rowptr1,
                                                          int *colidx1, double *val1)
{
    __shared__ uint64_t s[LDS_PAIRS];
    sort_row_in(s, list[blockIdx.x], rowptr, colidx, val, perm, rowptr1, colidx1, val1);
}

// rows of more than LDS_PAIRS entries: workgroup b sorts rows b, b + grid, ... in its own scratch slice of `slice` keys
__global__ void __launch_bounds__(LONG_THREADS) k_sort_long(int n_long, const int *__restrict__ list, uint64_t *scratch,
                                                            long long slice, const int *__restrict__ rowptr,
                                                            const int *__restrict__ colidx, const double *__restrict__ val,
                                                            const int *__restrict__ perm, const int *__restrict__ rowptr1,
                                                            int *colidx1, double *val1)
{
    uint64_t *s = scratch + (long long) blockIdx.x * slice;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x)
        sort_row_in(s, list[-r], rowptr, colidx, val, perm, rowptr1, colidx1, val1);
}

#define PERM_TRY(expr)                                          \
    do                                                          \
    {                                                           \
        const hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) { rc = (int) e__; goto done; }   \
    } while (0)

int csr_permute_sym_dev(int nrow, const int *rowptr, const int *colidx, const double *val, const int *perm, int *rowptr1,
                        int *colidx1, double *val1, hipStream_t st)
{
    int rc = 0, ends[2] = {0, 0};
    Census cs = {0, 0, 0, 0};
    char *work = nullptr;
    uint64_t *scratch = nullptr;
    const int nb = scan_tiles(nrow + 1);
    int *hit = nullptr, *lists = nullptr, *bsum = nullptr;
    Census *dcs = nullptr;
    long long span = 0;
    int nnz = 0;

    PERM_TRY(hipMemcpyAsync(&ends[0], rowptr, sizeof(int), hipMemcpyDeviceToHost, st));
    PERM_TRY(hipMemcpyAsync(&ends[1], rowptr + nrow, sizeof(int), hipMemcpyDeviceToHost, st));
    PERM_TRY(hipStreamSynchronize(st));
    if (ends[0] != 0 || ends[1] < 0) return CRP_PART_EPTR;
    nnz = ends[1];
    if (nnz > 0 && (colidx == nullptr || val == nullptr || colidx1 == nullptr || val1 == nullptr)) return CRP_PART_EARG;
    if (nrow == 0)
    {
        PERM_TRY(hipMemsetAsync(rowptr1, 0, sizeof(int), st));
        PERM_TRY(hipStreamSynchronize(st));
        return 0;
    }

    // work: hit[nrow] | lists[nrow] | bsum[nb] | census
    {
        const size_t bytes = sizeof(int) * ((size_t) nrow * 2 + (size_t) nb) + sizeof(Census);
        PERM_TRY(hipMalloc(&work, bytes));
        hit = (int *) work;
        lists = hit + nrow;
        bsum = lists + nrow;
        dcs = (Census *) (bsum + nb);
        PERM_TRY(hipMemsetAsync(hit, 0, sizeof(int) * (size_t) nrow, st));
        PERM_TRY(hipMemsetAsync(dcs, 0, sizeof(Census), st));
        PERM_TRY(hipMemsetAsync(rowptr1 + nrow, 0, sizeof(int), st));
    }
    // ---- pass 1 and its verdict
    span = nrow > nnz ? nrow : nnz;
    {
        const long long blocks = std::min<long long>((span + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_scatter_lengths, dim3((unsigned) blocks), dim3(256), 0, st, nrow, nnz, rowptr, colidx, perm,
                           rowptr1, hit, lists, dcs);
        PERM_TRY(hipGetLastError());
    }
    PERM_TRY(hipMemcpyAsync(&cs, dcs, sizeof(Census), hipMemcpyDeviceToHost, st));
    PERM_TRY(hipStreamSynchronize(st));
    if (cs.flags)
    {
        rc = (cs.flags & F_PTR) ? CRP_PART_EPTR : (cs.flags & F_COL) ? CRP_PART_ECOL : CRP_PART_EPERM;     // (the host's order)
        goto done;
    }
    // ---- pass 2
    PERM_TRY(exclusive_scan_inplace(nrow + 1, rowptr1, bsum, st));
    // ---- pass 3
    {
        const long long blocks = std::min<long long>((nrow + 3) / 4, 1 << 20);
        hipLaunchKernelGGL(k_sort_short, dim3((unsigned) blocks), dim3(256), 0, st, nrow, rowptr, colidx, val, perm, rowptr1,
                           colidx1, val1);
        PERM_TRY(hipGetLastError());
    }
    if (cs.n_mid > 0)
    {
        hipLaunchKernelGGL(k_sort_mid, dim3(cs.n_mid), dim3(MID_THREADS), 0, st, lists, rowptr, colidx, val, perm, rowptr1,
                           colidx1, val1);
        PERM_TRY(hipGetLastError());
    }
    if (cs.n_long > 0)
    {
        long long slice = LDS_PAIRS;
        while (slice < cs.max_long) slice <<= 1;
        const long long budget = (long long) 256 << 20;             // bytes of scratch the call allows itself
        const int grid = (int) std::max<long long>(1, std::min<long long>({(long long) cs.n_long, 256, budget / (slice * 8)}));
        PERM_TRY(hipMalloc(&scratch, sizeof(uint64_t) * (size_t) slice * (size_t) grid));
        hipLaunchKernelGGL(k_sort_long, dim3(grid), dim3(LONG_THREADS), 0, st, cs.n_long, lists + nrow - 1, scratch, slice,
                           rowptr, colidx, val, perm, rowptr1, colidx1, val1);
        PERM_TRY(hipGetLastError());
    }
    PERM_TRY(hipStreamSynchronize(st));
done:
    if (work || scratch) (void) hipStreamSynchronize(st);
    if (scratch) (void) hipFree(scratch);
    if (work) (void) hipFree(work);
    return rc;
}

}  // namespace

}  // namespace crp

extern "C" {

int crp_csr_permute_sym(int nrow, const int *rowptr, const int *colidx, const double *val, const int *perm, int *rowptr1,
                        int *colidx1, double *val1, void *stream)
{
    if (nrow < 0 || rowptr == nullptr || perm == nullptr || rowptr1 == nullptr) return CRP_PART_EARG;
    const void *ptrs[7] = {rowptr, colidx, val, perm, rowptr1, colidx1, val1};
    int ndev = 0, nhost = 0;
    for (const void *p : ptrs)
    {
        if (p == nullptr) continue;
        int is_dev = 0;
        crp_dev_ptr_is_device(p, &is_dev);
        (is_dev ? ndev : nhost)++;
    }
    if (ndev > 0 && nhost > 0) return CRP_PART_EMIXED;
    if (ndev == 0) return crp::csr_permute_sym_host(nrow, rowptr, colidx, val, perm, rowptr1, colidx1, val1);
    return crp::csr_permute_sym_dev(nrow, rowptr, colidx, val, perm, rowptr1, colidx1, val1, (hipStream_t) stream);
}

int crp_graph_row_partition(int nrow, int nproc, int *rowptr, int *colidx, double *val, int *perm, int *row_displs, int where)
{
    if (where < -1 || where > 1) return CRP_PART_EARG;
    int rc = crp::graph_row_order(nrow, nproc, rowptr, colidx, perm, row_displs);
    if (rc != 0) return rc;
    const int nnz = rowptr[nrow];
    bool on_dev = where == 1;
    if (where == -1)
    {
        int count = 0, dev = -1;
        on_dev = hipGetDeviceCount(&count) == hipSuccess && count > 0 && hipGetDevice(&dev) == hipSuccess && dev >= 0;
        (void) hipGetLastError();
    }
    if (!on_dev)
    {
        std::vector<int> rowptr1((size_t) nrow + 1), colidx1((size_t) nnz + 1);
        std::vector<double> val1((size_t) nnz + 1);
        rc = crp::csr_permute_sym_host(nrow, rowptr, colidx, val, perm, rowptr1.data(), colidx1.data(), val1.data());
        if (rc != 0) return rc;
        memcpy(rowptr, rowptr1.data(), sizeof(int) * ((size_t) nrow + 1));
        if (nnz > 0)
        {
            memcpy(colidx, colidx1.data(), sizeof(int) * (size_t) nnz);
            memcpy(val, val1.data(), sizeof(double) * (size_t) nnz);
        }
        return 0;
    }
    // staged through the current device: inputs up, P A P^T down into the caller's arrays
    const size_t ib = sizeof(int) * ((size_t) nrow + 1), cb = sizeof(int) * ((size_t) nnz + 1), vb = sizeof(double) * ((size_t) nnz + 1);
    char *d = nullptr;
    const hipError_t e = hipMalloc(&d, 2 * ib + 2 * cb + 2 * vb + ib);
    if (e != hipSuccess) return (int) e;
    double *dval = (double *) d, *dval1 = (double *) (d + vb);
    int *drow = (int *) (d + 2 * vb), *drow1 = (int *) (d + 2 * vb + ib), *dcol = (int *) (d + 2 * vb + 2 * ib),
        *dcol1 = (int *) (d + 2 * vb + 2 * ib + cb), *dperm = (int *) (d + 2 * vb + 2 * ib + 2 * cb);
    hipError_t he = hipMemcpy(drow, rowptr, ib, hipMemcpyHostToDevice);
    if (he == hipSuccess && nnz > 0) he = hipMemcpy(dcol, colidx, sizeof(int) * (size_t) nnz, hipMemcpyHostToDevice);
    if (he == hipSuccess && nnz > 0) he = hipMemcpy(dval, val, sizeof(double) * (size_t) nnz, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(dperm, perm, sizeof(int) * (size_t) nrow, hipMemcpyHostToDevice);
    rc = (int) he;
    if (rc == 0) rc = crp::csr_permute_sym_dev(nrow, drow, dcol, dval, dperm, drow1, dcol1, dval1, nullptr);
    if (rc == 0) rc = (int) hipMemcpy(rowptr, drow1, ib, hipMemcpyDeviceToHost);
    if (rc == 0 && nnz > 0) rc = (int) hipMemcpy(colidx, dcol1, sizeof(int) * (size_t) nnz, hipMemcpyDeviceToHost);
    if (rc == 0 && nnz > 0) rc = (int) hipMemcpy(val, dval1, sizeof(double) * (size_t) nnz, hipMemcpyDeviceToHost);
    (void) hipFree(d);
    return rc;
}

}  // extern "C"
