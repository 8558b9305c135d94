// csr_transpose.h -- the two paths of crp_csr_transpose (include/crpspmm_hip.h): host (csr_transpose.cpp) and device
// (transpose_kernels.hip).  Both take checked-for-NULL arguments from the C entry point and return its codes.
#pragma once

namespace crp {

int csr_transpose_host(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t, int *colidx_t,
                       double *val_t, int *tmap);
// every pointer a device pointer; runs on `stream` (a hipStream_t) and synchronises it
int csr_transpose_dev(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t, int *colidx_t,
                      double *val_t, int *tmap, void *stream);

}  // namespace crp
