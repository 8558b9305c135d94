// dropout_kernels.hip -- the attention-dropout mask of dropout.h over a CSR handle, as (nnz, heads) keep flags: what the fused
// GAT / GATv2 calls re-form in registers, written out for callers who run the chain of separate calls and for the tests.
// One wave per row; lane l takes the (entry, head) pairs l, l + 64, ... of the row.  transposed: the handle holds A^T, so the
// entry's column index is the row r of the draw and the handle's row (after its row map) the column code c.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace crp {

__global__ __launch_bounds__(256) void dropout_mask_kernel(const int nrow, const int heads, const int *__restrict__ rowptr,
                                                           const int *__restrict__ colidx, const int *__restrict__ rowmap,
                                                           const bool transposed, const uint32_t seed_lo, const uint32_t seed_hi,
                                                           const uint32_t thr, uint8_t *__restrict__ mask, const int *__restrict__ out_pos)
{
    const int64_t row = (int64_t) blockIdx.x * 4 + threadIdx.x / 64;
    if (row >= nrow) return;
    const int lane = threadIdx.x % 64;
    const int pb = rowptr[row], pe = rowptr[row + 1];
    const uint32_t mrow = (uint32_t) (rowmap ? rowmap[row] : (int) row);
    const int64_t n = (int64_t) (pe - pb) * heads;
    for (int64_t t = lane; t < n; t += 64)
    {
        const int p = pb + (int) (t / heads);
        const uint32_t h = (uint32_t) (t % heads);
        const uint32_t code = (uint32_t) colidx[p];
        const bool k = transposed ? dropout_keep(seed_lo, seed_hi, code, mrow, h, thr) : dropout_keep(seed_lo, seed_hi, mrow, code, h, thr);
        mask[(int64_t) (out_pos ? out_pos[p] : p) * heads + h] = k ? 1 : 0;
    }
}

hipError_t dropout_mask_csr(int nrow, int heads, const int *rowptr, const int *colidx, const int *rowmap, bool transposed, double drop,
                            unsigned long long seed, uint8_t *mask, const int *out_pos, hipStream_t s)
{
    if (nrow <= 0) return hipSuccess;
    const int64_t blocks = ((int64_t) nrow + 3) / 4;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned) blocks), dim3(256), 0, s, nrow, heads, rowptr, colidx, rowmap, transposed,
                       (uint32_t) seed, (uint32_t) (seed >> 32), dropout_threshold(drop), mask, out_pos);
    return hipGetLastError();
}

}  // namespace crp
