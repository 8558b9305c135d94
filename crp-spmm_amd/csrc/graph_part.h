// graph_part.h -- k-way row partition of a square CSR and the symmetric permutation P A P^T on the host (internal;
// see graph_part.cpp; the C ABI is include/crp_part.h).
#pragma once

namespace crp {

// perm[i] = new index of original row i; row_displs[q] .. row_displs[q + 1] - 1 = the new rows of part q (nproc + 1
// entries).  Returns 0 or a negative CRP_PART_E* code (include/crp_part.h).
int graph_row_order(int nrow, int nproc, const int *rowptr, const int *colidx, int *perm, int *row_displs);

// rowptr1 / colidx1 / val1 := P A P^T (the output rule of include/crp_part.h), all host arrays, after the checks of
// the device path (rowptr monotone, columns in range, perm a bijection).  0 or CRP_PART_E*.
int csr_permute_sym_host(int nrow, const int *rowptr, const int *colidx, const double *val, const int *perm, int *rowptr1,
                         int *colidx1, double *val1);

}  // namespace crp
