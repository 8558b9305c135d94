// csr_transpose.cpp -- host path of crp_csr_transpose (include/crpspmm_hip.h): a counting sort of the nonzeros by column.
// The nonzeros are placed in input order, so inside an output row they stand in ascending (row, position) order: the
// stable sort the contract names, and what the device path (transpose_kernels.hip) reproduces bit for bit.
#include <stddef.h>
#include <vector>
#include "crpspmm_hip.h"
#include "csr_transpose.h"

namespace crp {

int csr_transpose_host(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t, int *colidx_t,
                       double *val_t, int *tmap)
{
    // ---- checks first: nothing is written before the input is known to be good
    if (rowptr[0] != 0) return CRP_CSR_T_EPTR;
    for (int i = 0; i < nrow; i++)
        if (rowptr[i + 1] < rowptr[i]) return CRP_CSR_T_EPTR;
    const int nnz = rowptr[nrow];
    if (nnz > 0 && (colidx == NULL || colidx_t == NULL || (val_t != NULL && val == NULL))) return CRP_CSR_T_EARG;
    for (int p = 0; p < nnz; p++)
        if (colidx[p] < 0 || colidx[p] >= ncol) return CRP_CSR_T_ECOL;
    // ---- column counts, offsets
    for (int c = 0; c <= ncol; c++) rowptr_t[c] = 0;
    for (int p = 0; p < nnz; p++) rowptr_t[colidx[p] + 1]++;
    for (int c = 0; c < ncol; c++) rowptr_t[c + 1] += rowptr_t[c];
    // ---- fill in input order
    std::vector<int> cursor(rowptr_t, rowptr_t + ncol);
    for (int i = 0; i < nrow; i++)
        for (int p = rowptr[i]; p < rowptr[i + 1]; p++)
        {
            const int q = cursor[(size_t) colidx[p]]++;
            colidx_t[q] = i;
            if (val_t) val_t[q] = val[p];
            if (tmap) tmap[q] = p;
        }
    return 0;
}

}  // namespace crp
