/*
 * crp_part.h -- graph-based 1D row partitioning (part-method 1 of the example programs) and the symmetric permutation
 * P A P^T of a square CSR, on the host or on the device.
 *
 * The partition: row groups (consecutive rows with identical column lists) form the vertices of the graph of the
 * pattern of A + A^T; the vertices are cut by recursive bisection along breadth-first orders from pseudo-peripheral
 * roots, a part meant for k ranks at the weighted floor(k/2)/k point, vertex weight = row nonzeros.  Every part holds
 * at most nnz / nproc + (largest row nnz) nonzeros; inside a part the rows keep their original relative order.  The
 * result does not depend on the thread count.
 *
 * The permutation: row perm[i] of the output receives row i's entries with columns perm[c], ascending inside the row;
 * duplicate columns keep their original order.  The result is unique: host and device outputs agree bit for bit.
 *
 * Return values: 0 on success, < 0 for an argument error (CRP_PART_E*), > 0 for a HIP error (hipError_t).
 */
#ifndef CRP_PART_H
#define CRP_PART_H

#ifdef __cplusplus
extern "C" {
#endif

#define CRP_PART_EARG   (-1)   /* null pointer, negative size, nproc < 1 */
#define CRP_PART_EPERM  (-2)   /* perm is not a bijection of [0, nrow) */
#define CRP_PART_ECOL   (-3)   /* a column index outside [0, nrow) */
#define CRP_PART_EPTR   (-4)   /* rowptr does not start at 0 or decreases */
#define CRP_PART_EMIXED (-5)   /* host and device pointers mixed in one call */

/* k-way row partition only: perm[i] = new index of original row i (nrow entries), row_displs = nproc + 1 cuts of the
 * permuted rows.  Host arrays; the pattern need not be symmetric (the graph is A + A^T). */
int crp_graph_row_order(int nrow, int nproc, const int *rowptr, const int *colidx, int *perm, int *row_displs);

/* rowptr1 / colidx1 / val1 := P A P^T.  Either every pointer is a host pointer (host threads) or every pointer is a
 * device pointer (HIP kernels on `stream`, which the call synchronises); the inputs are checked first (perm a
 * bijection, columns in range, rowptr monotone) and a bad input returns its code without writing colidx1 / val1. */
int crp_csr_permute_sym(int nrow, const int *rowptr, const int *colidx, const double *val, const int *perm, int *rowptr1,
                        int *colidx1, double *val1, void *stream);

/* The contract of METIS_row_partition in the reference's examples: host arrays, the partition into perm / row_displs
 * and P A P^T written back into rowptr / colidx / val.  where = 0: host; 1: device, staged through the current HIP
 * device; -1: the device when one is current, the host otherwise. */
int crp_graph_row_partition(int nrow, int nproc, int *rowptr, int *colidx, double *val, int *perm, int *row_displs,
                            int where);

#ifdef __cplusplus
}
#endif
#endif
