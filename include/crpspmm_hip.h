/*
 * crpspmm_hip.h -- device-level C ABI of the MI355X (gfx950) CRP-SpMM hot path.
 *
 * These are the entry points a host binding (cgo / JNI / ctypes / the MPI
 * facade in rowpara_spmm.h) calls for the work the reference does inside
 * rp_spmm_exec():
 *
 *   reference call site (under /root/reference)        replaced by
 *   -------------------------------------------------  -------------------------
 *   src/rowpara_spmm.c:388-408  mkl_sparse_d_create_csr
 *        + mkl_sparse_d_mm + mkl_sparse_destroy         crp_csr_dev_create (once)
 *                                                       + crp_spmm_csr_f64
 *   src/rowpara_spmm.c:232-262  pack B rows (OpenMP)    crp_gather_rows_f64
 *   src/rowpara_spmm.c:313-344  unpack B rows           crp_scatter_rows_f64
 *   src/rowpara_spmm.c:348-384  self-to-self copy       eliminated (two-source
 *                                                       column index, see below)
 *   deprecated/src/cuda_proxy.cu:53-118 mem/copy shims  crp_dev_* helpers
 *
 * Plain pointers and sizes only; no torch / MPI types.  Every function
 * returns 0 on success or a hipError_t value (> 0) / negative argument
 * error; nothing here falls back to the CPU.
 *
 * Two-source column index: a column index c >= 0 addresses row c of the
 * caller's local B block (B0, leading dimension ldB0); c < 0 addresses row
 * (~c) of the compact buffer of rows received from peers (B1, ldB1).  With
 * one rank every index is >= 0 and B1 may be NULL.
 *
 * Streams.  Every call that takes a `stream` is asynchronous on that stream, taken literally (NULL = the null
 * stream): in steady state it enqueues all of its device work there and nowhere else, allocates nothing, waits
 * for nothing and touches no other stream, so it may be captured into a graph on that stream.  The calls that
 * may block are these and no others:
 *   - The first call that builds state on a handle blocks: what it builds is complete on return.  State a handle
 *     builds lazily -- a derived format (row panels, team streams, the row-owner kernel's C rows after a new row
 *     map) and the fp32 copies of the values -- is built by the first call that needs it, on that call's stream,
 *     and the call waits once for what it enqueued there.  Later calls on ANY stream therefore find it complete;
 *     they never wait, and the library keeps no event for it.  Such a first call is not capturable.
 *   - With a host pointer crp_csr_dev_update_values blocks until the values have left the caller's array.  With
 *     a device pointer it is asynchronous and refreshes every format and copy built so far on `stream`.
 *   - crp_csr_transpose with device pointers (it sizes its work from counts it reads back), and the calls marked
 *     Blocking below.
 * Two calls on one handle that run on different streams are the caller's to order whenever one of them writes
 * the handle's values (crp_csr_dev_update_values) or a row map; calls that only read the handle -- the products,
 * the SDDMM, the attention calls, the row softmax -- need no ordering among themselves.
 * The multi-head attention calls (crp_attention_mh_csr_*, crp_attention_bwd_q_mh_csr_*, crp_attention_bwd_kv_mh_csr_*) are
 * attention calls in every sentence above: asynchronous on `stream`, taken literally; in steady state they enqueue all of their
 * device work there and nowhere else, allocate nothing, wait for nothing and touch no other stream, so they may be captured;
 * the only state they may build is the handle's fp32 copy of the values (fp32, bias = 1), by the first call that needs it.
 * The same holds, word for word, for the GAT attention calls (crp_gat_attention_csr_*, crp_gat_attention_bwd_row_csr_*,
 * crp_gat_attention_bwd_col_csr_*), for the GATv2 attention calls (crp_gatv2_attention_csr_*, crp_gatv2_attention_bwd_row_csr_*,
 * crp_gatv2_attention_bwd_col_csr_*), for the _drop_ forms of both families (crp_gat_attention_drop_*, crp_gatv2_attention_drop_*)
 * and for crp_dropout_mask_csr, which reads the handle's pattern only and builds no state at all.  crp_col_sum_* take no handle
 * and work in the caller's scratch: all of their device work on `stream`, nothing else.
 */
#ifndef CRPSPMM_HIP_H
#define CRPSPMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRP_LAYOUT_ROW_MAJOR 0
#define CRP_LAYOUT_COL_MAJOR 1

/* Opaque device-resident sparse matrix (CSR arrays + launch schedule). */
typedef struct crp_csr_dev *crp_csr_dev_p;

/* ---- device management --------------------------------------------------- */
int crp_hip_device_count(int *count);
int crp_hip_set_device(int dev);
int crp_hip_get_device(int *dev);
/* name must hold >= 256 bytes; cu_count / hbm_bytes may be NULL. */
int crp_hip_device_info(int dev, char *name, int *cu_count, size_t *hbm_bytes);

/* PCI bus id of the current device ("0000:c1:00.0"): tells whether two ranks share a GPU. len >= 16. */
int crp_hip_device_bus_id(char *out, size_t len);

int crp_dev_malloc(void **ptr, size_t bytes);
int crp_dev_free(void *ptr);
int crp_dev_memset(void *ptr, int value, size_t bytes, void *stream);
/* kind: 0 host->device, 1 device->host, 2 device->device.  Asynchronous on
 * `stream` when the host side is pinned; crp_stream_sync() to wait. */
int crp_dev_memcpy(void *dst, const void *src, size_t bytes, int kind, void *stream);
/* strided copy of `height` rows of `width_bytes` bytes (hipMemcpy2DAsync); pitches in bytes. */
int crp_dev_memcpy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes,
                     size_t height, int kind, void *stream);
/* pinned host memory (hipHostMalloc / hipHostFree) */
int crp_host_malloc(void **ptr, size_t bytes);
int crp_host_free(void *ptr);
/* returns 1 in *is_dev when ptr is device memory, 0 for host memory. */
int crp_dev_ptr_is_device(const void *ptr, int *is_dev);

int crp_stream_create(void **stream);
int crp_stream_destroy(void *stream);
int crp_stream_sync(void *stream);
int crp_event_create(void **event);
int crp_event_destroy(void *event);
int crp_event_record(void *event, void *stream);
int crp_event_sync(void *event);
int crp_stream_wait_event(void *stream, void *event);
int crp_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---- device-resident CSR -------------------------------------------------- */
/* Upload a host CSR (0-based rowptr[0] == 0, int32 indices, fp64 values).
 * colidx may carry the two-source encoding described above; ncol is the row
 * count of B0 (used for argument checking only).  Blocking. */
int crp_csr_dev_create(int nrow, int ncol, const int *rowptr, const int *colidx,
                       const double *val, crp_csr_dev_p *out);
/* The same, for a matrix whose VALUES already sit in device memory (a row panel replicated between GPUs,
 * /root/reference/src/para2d_spmm.c:56-86): val_host is still read (the derived formats are built on the host), but the
 * device CSR takes its values from val_dev instead of a second upload.  src_start = NULL: val_dev holds the nnz values in
 * order; else row t's values start at val_dev[src_start[t]] (host array of nrow entries: a row subset of a larger matrix). */
int crp_csr_dev_create_dv(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val_host,
                          const double *val_dev, const int *src_start, crp_csr_dev_p *out);
int crp_csr_dev_destroy(crp_csr_dev_p *A);
/* New values for the same sparsity pattern (val in the order given at create; host or device
 * pointer): refreshes the CSR copy and every derived format on `stream`. */
int crp_csr_dev_update_values(crp_csr_dev_p A, const double *val, void *stream);
/* Row-subset matrices: row i of A writes row rowmap[i] of C (0 <= rowmap[i] < c_nrow; host array of
 * nrow entries, copied).  Lets a product be split into row subsets that run at different times
 * (rows with no remote column while the B exchange is in flight, the rest after it) without
 * touching the per-row summation order.  rowmap = NULL restores the identity.  Blocking. */
int crp_csr_dev_set_rowmap(crp_csr_dev_p A, const int *rowmap, int c_nrow);
int crp_csr_dev_nrow(crp_csr_dev_p A);
long long crp_csr_dev_nnz(crp_csr_dev_p A);
/* bytes of HBM the kernel must touch for A itself: 12*nnz + 4*(nrow+1). */
long long crp_csr_dev_bytes(crp_csr_dev_p A);
/* csr_mat_row_part_comm_size (/root/reference/src/spmat_part.c:38-64; include/spmat_part.h) evaluated ON THE DEVICE for a
 * matrix that is device-resident already -- re-planning a grid for other widths or rank counts without touching the host CSR:
 * comm_sizes[b] = distinct columns the rows rblk_ptr[b] .. rblk_ptr[b + 1] name outside [x_displs[b], x_displs[b + 1]),
 * *total_size their sum; bit-exact against the host function.  One bitmap of ncol bits per block in HBM (nblk * ncol / 8
 * bytes, temporary).  Only for matrices with plain column indices (no two-source encoding): -2 otherwise. */
int crp_csr_dev_row_part_comm_size(crp_csr_dev_p A, int nblk, const int *rblk_ptr, const int *x_displs, int *comm_sizes,
                                   int *total_size);

/* ---- transpose of a CSR, and handles for A^T ------------------------------------
 * rowptr_t / colidx_t / val_t / tmap := A^T for the nrow x ncol CSR (rowptr, colidx, val).  Row c of the output lists the
 * rows of A that hold column c in ascending row order; duplicates of one (row, column) pair keep their original order;
 * tmap[q] = position in the input of output entry q and val_t[q] = val[tmap[q]] -- a stable sort of the nonzeros by
 * column, so the result is unique and host and device outputs agree bit for bit.  rowptr_t holds ncol + 1 entries,
 * colidx_t / val_t / tmap nnz; val_t and tmap may be NULL (val may be NULL when val_t is).  Either every pointer is a host
 * pointer (host code) or every pointer is a device pointer (HIP kernels on `stream`, which the call synchronises; column
 * counts by integer atomics, the order inside a row by a sort, values moved and never added).  The inputs are checked
 * first -- rowptr[0] == 0, rowptr never decreases, every column in [0, ncol): a negative column (the two-source
 * encoding) is refused -- and a bad input returns its code before colidx_t, val_t or tmap is written.
 * Returns 0, a CRP_CSR_T_E* code (< 0), or a HIP error (> 0). */
#define CRP_CSR_T_EARG   (-1)   /* null pointer, negative size */
#define CRP_CSR_T_ECOL   (-3)   /* a column index outside [0, ncol) */
#define CRP_CSR_T_EPTR   (-4)   /* rowptr does not start at 0 or decreases */
#define CRP_CSR_T_EMIXED (-5)   /* host and device pointers mixed in one call */
int crp_csr_transpose(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val,
                      int *rowptr_t, int *colidx_t, double *val_t, int *tmap, void *stream);
/* A device-resident handle for A^T from A's host CSR (arguments as crp_csr_dev_create, plain column indices only): A's
 * arrays go up once, are transposed on the device (crp_csr_transpose) and come back for the host-side format builders;
 * tmap stays in device memory.  crp_csr_dev_nrow() of the result is ncol.  Everything else applies to it as to any other
 * handle: it IS the handle crp_csr_dev_create would give for the transposed arrays.  crp_csr_dev_update_values() keeps
 * its contract -- values in the order given at create, which is A's order; the handle gathers them through tmap.
 * Returns 0, a CRP_CSR_T_E* code for a bad CSR, -3 out of host memory, or a HIP error (> 0).  Blocking. */
int crp_csr_dev_create_t(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, crp_csr_dev_p *out);
/* 1 for a handle made by crp_csr_dev_create_t, 0 for any other, -1 for NULL */
int crp_csr_dev_is_transposed(crp_csr_dev_p A);

/* what variant 0 resolves to for this matrix: 1 csr-rowgroup, 2 rowpanel-R4, 3 rowpanel-R8
 * (chosen at create time from how many columns the rows of a panel share;
 * CRPSPMM_SPMM_VARIANT=1|2|3 overrides). */
/* The fp32 value path (BASELINE configs[3]; the reference itself is fp64-only, src/rowpara_spmm.h:28): the same
 * product with A's values, B and C in fp32 and fp32 FMAs, row-major operands.  A is the matrix created from fp64
 * values; its fp32 copies are derived on first use and follow crp_csr_dev_update_values.  variant 0 = auto (the
 * fp32 instance of the team kernel from 32 columns on (from 65 on mostly-hole panels) where teams share columns and the operands are 16-byte
 * aligned with n, ldB, ldC multiples of 4; else the fp32 CSR row-group kernel), 1 = row-group, 5 = team kernel.
 * Parity is defined against the fp64 product: relative Frobenius error <= 1e-5 (tests/test_gpu_parity.py). */
int crp_spmm_csr_f32(crp_csr_dev_p A, int n, const float *B0, long long ldB0, const float *B1, long long ldB1, float *C,
                     long long ldC, int variant, void *stream);

int crp_csr_dev_auto_variant(crp_csr_dev_p A);
/* 1 when the derived formats (row panels, teams) hold the rows in the locality order of csrc/locality.cpp
 * instead of the caller's order (taken at create time when it lets the rows of a panel share more columns;
 * CRPSPMM_REORDER=0|1 overrides).  Results do not depend on it: C rows are written through a row map and
 * every row's products are still summed in the kernel variant's own order. */
int crp_csr_dev_reordered(crp_csr_dev_p A);
/* the variant that a variant-0 (auto) row-major fp64 product of n columns launches on this matrix when B0 and C are 16-byte aligned
 * with ldB0 = ldC = n and there is no B1 (csrc/dispatch.cpp, resolve_f64: the rules crp_spmm_csr_f64 follows; after such a
 * product it equals crp_csr_dev_last_variant()).  The create-time choice (crp_csr_dev_auto_variant), replaced for even n by 5
 * (team2-R8) where 64 consecutive rows share columns: from 96 columns on (from 33 when the row-panel format would ask for more than
 * 12 B row slices per row of A, from 48 when the matrix has no stride lattice; from 33 when fewer than 35 % of the (row, entry) pairs
 * of the R = 8 panels exist; for 61 .. 64 columns otherwise); else by 7 (team2r-R8: lane groups own rows, csrc/team2r_kernel.hip) at
 * 24 <= n <= 32 when fewer than 35 % of those pairs exist (CRPSPMM_TEAM2R=0|1 forces, then up to 64 columns); and by 1 below 24
 * columns.  Once a variant-0 product found the row-owner streams too large (past their 32-bit offsets), 7 is no longer chosen: 3
 * under CRPSPMM_TEAM2R=1, the choice without it otherwise.  Other operands may fall back further (5 -> 3 -> 1).  Variants 4 and 6
 * (the round-1 LDS team kernel, the narrow team kernel of round 3) were measured slower than what auto picks at every width and
 * removed in round 4: asking for them returns -1. */
int crp_csr_dev_resolved_variant(crp_csr_dev_p A, int n);
/* the variant the last crp_spmm_csr_f64 / _f32 on this matrix launched (after every fallback), or 0 before the first */
int crp_csr_dev_last_variant(crp_csr_dev_p A);
/* the kernel instance that product launched, named by its launcher from its own template arguments: "rowgroup<LPR,VW,NV>", "cm"
 * (column-major), "panel<R,NV,VW,a32|a64,b0|b1>", "narrow<b0|b1,o32|o64,compact|full>", "team2r<G,b0|b1>",
 * "team2<f64|f32,NVH|NV1|NV2,b0|b1,compact|full>", "rowgroup_f32<LPR,VW>"; "" before the first product and after one that launched
 * nothing (an empty matrix, n = 0, an error before the launch).  The string lives as long as the library. */
const char *crp_csr_dev_last_kernel(crp_csr_dev_p A);
/* 1 when the team formats built so far found the two nested strides of a mesh numbered along its lines (their
 * teams are then blocks of neighbouring mesh lines), 0 otherwise / not built yet. */
int crp_csr_dev_lattice(crp_csr_dev_p A);
/* 1 when the team format (variant 5) of this matrix holds compact value blocks (only the values that exist), 0 when it holds 8 values
 * per part, -1 before it is built (csrc/dispatch.cpp, team2_compact: fixed by whichever product builds it first). */
int crp_csr_dev_team2_compact(crp_csr_dev_p A);
/* Host-only: build the row-panel format the rowpanel kernels consume (R = 4 or 8)
 * and return malloc'd copies (caller frees).  Panel p owns entries pptr[p] .. pptr[p+1]
 * (padded to multiples of 8 with mask-0 entries); entry q has column pcol[q] (two-source
 * encoding), row-presence mask byte (pmask4[q/4] >> 8*(q%4)) & 0xFF and values
 * pval[q*R .. q*R+R-1].  The entries of a panel are in column order, except under the team schedule
 * (below) where they are in the order the panel's wave meets them.
 * porder (optional) receives the processing order: *norder positions, position s is the panel the
 * s-th wave takes (4 consecutive positions = one workgroup), -1 = none.  Which order:
 *   - matrices with two nested far strides (3D meshes in natural order), R = 8: the TEAM SCHEDULE --
 *     the four waves of a workgroup take a 2 x 2 block of tooth-mate panels (panels that read the
 *     same B rows through different bands), every panel's entries are re-ordered so that the four
 *     waves reach a shared row after the same number of entries, and the workgroups sweep the
 *     teeth in lockstep per XCD; norder = 4 * teams;
 *   - the same matrices with R = 4: the stride-lattice order of single panels; norder = npanel;
 *   - otherwise groups of consecutive panels visited breadth-first over shared B rows.
 * CRPSPMM_PANEL_ORDER=0|1|2|3 forces natural / breadth-first / lattice / team schedule,
 * CRPSPMM_PANEL_GROUP sets the breadth-first group size.  Used by the CPU tests of the format. */
int crp_panel_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int R,
                          int *npanel, int **pptr, int **pcol, unsigned **pmask4, double **pval,
                          long long *real_entries, int **porder, int *norder);

/* Host-only: the team format variant 4 ("team-R8") consumes, built on the R = 8 panels: team g owns
 * panels tpanel[4g .. 4g+3] (-1 = none), one per wave of a workgroup, and union entries
 * tptr[g] .. tptr[g+1] (padded to multiples of 8 with mask-0 entries): column tcol[q], and in
 * tmask[q] byte w the row mask of wave w's panel for that column (0: wave w skips the entry).  Every
 * wave meets its own panel's entries in that panel's own order.  torder = processing order of
 * the teams; *lattice = 1 when the teams are 2 x 2 blocks of a stride lattice, 0 for four consecutive
 * panels.  malloc'd copies (caller frees).  Used by the CPU tests of the format. */
int crp_team_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int *nteam, int *lattice,
                         int **tpanel, int **tptr, int **tcol, unsigned **tmask, int **torder);

/* Host-only: the streams variant 5 ("team2-R8", csrc/team2_kernel.hip) consumes: teams of 8 panels of 8 rows
 * (one per wave of a 512-thread workgroup; tpanel, -1 = none), the union of whose columns is walked in rounds
 * of up to 8 slots.  tinfo[4g] = rounds of team g, [4g+1] = its first record block, [4g+2] = parts of all its
 * waves, [4g+3] = filled slots.  trec = record blocks of 8 rounds x 8 waves x 4 words (csrc/panel_format.h, Team2Host):
 * word 0 = part count | ring slots | flags | value position of part 0; word 1 = ranges (6 bits per part: first * 8 + len
 * - 1) | value position of part 1 | size class of round r+3's value block; word 2 = offset of round r+3's value block in
 * the wave's stream (20 bits, units of 4 values) | value positions of parts 2 and 3; word 3 = column this wave fetches for
 * round r+3.  tpro[((3g + d)*8 + w)*2 ..] = {column, value offset} of round d < 3.  Values are compact:
 * a part of len rows holds len values; a round's parts form one block (padded to 4 values) of the wave's stream, which
 * starts at tval[4 * tvoff[8g + w]]; part i's first value sits (position_i - 7 + first_i) values into the block.
 * vmap[nz] = index in tval of CSR nonzero nz.  *nvalent = values in tval.  malloc'd copies (caller frees).  Used by the
 * CPU tests, which replay the streams in numpy. */
int crp_team2_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int *nteam, int *lattice,
                          int **tpanel, int **tinfo, int **tpro, unsigned **trec, long long *nrecwords,
                          long long **tvoff, double **tval, long long *nvalent, int **torder, unsigned **vmap);
/* The launch grid of the streams crp_team2_format_host() built last (process-wide, planning / test helper only): 8 runs
 * of *ngrid / 8 entries, run x = the teams XCD x processes, in order (-1 = none); a generation = 64 consecutive
 * entries of a run.  Slots of a round that hold no B row name a row of the team (fetched, not read). */
int crp_team2_format_host_grid(int **tgrid, int *ngrid);
/* 1 when the value blocks of those streams are compact (a part of len rows holds len values), 0 when every part holds 8
 * values, row r of part i at 8 i + r of the round's block (panels filled to 40 % and more; CRPSPMM_TEAM2_COMPACT=0|1 forces) */
int crp_team2_format_host_compact(void);

/* Host-only: the streams variant 7 ("team2r-R8", csrc/team2r_kernel.hip: the row-owner team kernel for operands of 24 .. 64 fp64
 * columns) consumes.  Teams as variant 5.  A round has 8 G d ring slots of 1024 / G bytes (G = 4: n <= 32, 2: n <= 64; d = 2 row DMA
 * instructions per wave and round); wave w fetches slots G d w .. G d (w + 1) - 1.  Round r (from tinfo[2g + 1] on, tinfo[2g] rounds), wave w owns trec[(r * 8 + w) * 16 ..]: [0] Lp =
 * steps (multiple of 2, <= 12); [1] first 16-byte unit of its block inside the wave's stream, which starts at byte 16 * tvoff[8g + w]
 * of tval; [2 .. 2 + G d) the columns of the slots the wave fetches for this round.  A block = [8 rows][Lp] doubles, then
 * [8 rows][Lp] uint16, then a 64-byte header = the record of round r + 2 of the same team and wave (zeros past the last round):
 * step s of row i multiplies the value with the B row slice at that byte offset of the round's ring set (slot * 1024 / G);
 * 8192 d = the slice of zeros (padding, value 0.0).  vmap[nz] = 8-byte word of tval that holds CSR nonzero nz.
 * tent (may be NULL): per entry e of tgrid and wave w 32 words at tent[(e * 8 + w) * 32]: [0] rounds (0: no team), [1] panel, [2], [3]
 * tvoff, [4 .. 14) record of round 0, [14 .. 24) of round 1, [24 .. 32) 0xFFFFFFFF (the C rows, filled on the device).
 * stats (4, may be NULL): rounds, steps (sum of Lp), filled slots, nonzeros.  malloc'd copies (caller frees). */
int crp_team2r_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int G, int *nteam, int *lattice, int **tpanel,
                           int **tinfo, unsigned **trec, long long *nrecwords, long long **tvoff, double **tval, long long *nwords,
                           int **tgrid, int *ngrid, unsigned **vmap, long long *stats, unsigned **tent);

/* Host-only: the processing order of the rows of a square A that crp_csr_dev_create() applies for B-row
 * locality (csrc/locality.cpp: row groups with identical column lists, `nparts` slabs by breadth-first
 * bisection, reverse Cuthill-McKee inside every slab).  perm[i] = row processed at position i (caller provides
 * nrow ints).  Returns 0, or 1 when the matrix does not qualify (not square, two-source indices, too small):
 * perm is then the identity.  info (4 doubles, may be NULL): row groups, parts, mean |pos(col) - pos(row)| before, after. */
int crp_locality_order_host(int nrow, int ncol, const int *rowptr, const int *colidx, int nparts, int *perm, double *info);
/* Host-only: the kernel choice of crp_csr_dev_create and crp_spmm_csr_f64 / _f32 for this matrix, without a device (the CPU tests
 * of csrc/dispatch.cpp).  For every width widths[i] the variant a product with `variant` launches (f32: the fp32 path) into
 * resolved[i], for the operand shape 0 = B0 and C 16-byte aligned with ld = n, 1 = ld = n + 1, 2 = as 0 with a B1, 3 = as 0 with
 * B0 only 8-byte aligned.  info (5 ints, may be NULL): auto variant, reordered (crp_csr_dev_reordered), the team kernel's
 * first width, whether teams share columns, whether the R = 8 panels are mostly holes.  Reads the CRPSPMM_* knobs as the
 * product does.  Returns 0, or -1 on bad arguments. */
int crp_spmm_plan_host(int nrow, int ncol, const int *rowptr, const int *colidx, int nwidth, const int *widths, int variant, int f32,
                       int shape, int *resolved, int *info);

/* ---- the hot kernel --------------------------------------------------------
 * C[nrow x n] := A * B (alpha = 1, beta = 0; C is overwritten, never read),
 * the arithmetic of mkl_sparse_d_mm as called at src/rowpara_spmm.c:403-406:
 * C[i][j] = sum_p val[p] * B[col[p]][j]; every product is formed once (absent pairs are skipped,
 * never multiplied by zero) and a row's products are summed one after the other with FMAs -- in
 * ascending p, except under the team schedule / variant 4 where the order is the team's schedule
 * (fixed at create time, so repeated calls are bit-identical).
 * layout 0: B0/B1/C row-major (ld >= n); layout 1: column-major
 * (ldB0 >= rows of B0, ldB1 >= rows of B1, ldC >= nrow).  All pointers are
 * device pointers; the launch is asynchronous on `stream`.  `variant` picks a
 * kernel (0 = automatic); see crp_spmm_variant_name(). */
int crp_spmm_csr_f64(crp_csr_dev_p A, int layout, int n,
                     const double *B0, long long ldB0,
                     const double *B1, long long ldB1,
                     double *C, long long ldC, int variant, void *stream);
const char *crp_spmm_variant_name(int variant);
int crp_spmm_variant_count(void);

/* ---- sampled dense-dense product over A's pattern (SDDMM) ---------------------
 * out[p] = < X[i][0:n], Y[c][0:n] > for every nonzero p = (i, c) of A; mode 1: times A's current value of that nonzero
 * (the fp32 form multiplies by the fp32 copy of the value, derived on first use and kept current by
 * crp_csr_dev_update_values).  Row-major operands: X has a row per row of A (row rowmap[t] for row t of a handle with a
 * row map, crp_csr_dev_set_rowmap), Y0 / Y1 are the two sources of the column code (c >= 0: row c of Y0, c < 0: row ~c
 * of Y1; a source no code names may be NULL -- Y0 when every code is negative or A has no nonzero, Y1 when none is -- and
 * its leading dimension is then not read).  Nonzero p of the handle writes out[out_pos[p]] (out_pos: device
 * int32 array of nnz entries), out[p] when out_pos is NULL: nnz entries, or the entries out_pos names, and nothing
 * else.  p counts in the handle's own CSR order -- for a handle made by crp_csr_dev_create the order of the values
 * given at create, which is the order crp_csr_dev_update_values takes, so out may be passed to it as it is; for a
 * handle made by crp_csr_dev_create_t the order of the transposed arrays.  Only pairs of the pattern are formed: a Y
 * row no column names and the X row of an empty row are never read.  All pointers are device pointers; the launch is
 * asynchronous on `stream`.  Returns 0, a HIP error (> 0), or a negative argument error, before which nothing is
 * written: -1 for a NULL handle, X or out, for Y0 = NULL on a handle with a code >= 0, for Y1 = NULL on a handle with
 * negative codes, for n < 1 and for a mode other than 0 or 1; -4 for a leading dimension below n (of X, or of a source
 * that is not NULL).
 * Fixed order: column j belongs to lane (j / W) % L of a group of L lanes (W = elements per 16 bytes; L = 8, 16, 32 or
 * 64, picked from n), every lane adds its products in ascending j with FMAs, and the lanes' sums meet in the balanced
 * binary tree over the lane number.  Assignment and tree are a function of (dtype, n) ONLY -- not of operand alignment
 * or leading dimensions (operands that cannot be read in 16-byte pieces are read by elements into the same
 * assignment), of the source a Y row comes from, of the handle (full matrix or row subset), or of the entry's position
 * in its row.  Repeated calls are therefore bit-identical, and a row-subset handle reproduces the full matrix's entries
 * bit for bit. */
int crp_sddmm_csr_f64(crp_csr_dev_p A, int n, const double *X, long long ldX,
                      const double *Y0, long long ldY0, const double *Y1, long long ldY1,
                      double *out, const int *out_pos, int mode, void *stream);
int crp_sddmm_csr_f32(crp_csr_dev_p A, int n, const float *X, long long ldX,
                      const float *Y0, long long ldY0, const float *Y1, long long ldY1,
                      float *out, const int *out_pos, int mode, void *stream);

/* ---- fused sparse attention over A's pattern -----------------------------------
 * For every row i of the handle with entries p = (i, c_p), p in the handle's CSR order:
 *   s_p = scale * < Q[i][0:nk], K[c_p][0:nk] >      (bias = 1: + A's current value of p; the fp32 form adds the fp32 copy
 *                                                    of the value that crp_sddmm_csr_f32 mode 1 uses)
 *   O[i][0:nv] = sum_p softmax_p(s) * V[c_p][0:nv]
 * -- crp_sddmm_csr_*, a scale, crp_row_softmax_*, a value update and crp_spmm_csr_* in one trip over the row, without the
 * nnz-sized intermediates and without touching A's values.  Row-major operands: Q and O have a row per row of A (row
 * rowmap[t] for row t of a handle with a row map); K0 / V0 and K1 / V1 are the two sources of the column code, as Y0 / Y1
 * of the SDDMM (a source no code names may be NULL).  The fp32 form takes scale as a double and rounds it to float once.
 * Optional outputs, each skipped when NULL: lse[i] = m + log(l) per row, indexed like the rows of O (m = the row's maximum
 * score, l = sum_p exp(s_p - m)); p_out = the probabilities exp(s_p - m) / l, nonzero p written to p_out[out_pos[p]]
 * (p_out[p] when out_pos is NULL), as the SDDMM writes -- the order crp_csr_dev_update_values and crp_row_softmax_bwd_*
 * take, so the existing calls form the backward pass from it.  Only what is named is written: O[i][0:nv] of every row,
 * lse of every row, the nnz entries of p_out.  All pointers are device pointers; the launch is asynchronous on `stream`.
 * Special cases: an empty row writes +0 to O[i][0:nv] and lse = -inf; a one-entry row with a finite score gives O[i] =
 * V[c] bit for bit; a score of -inf (a bias value or a product) is a masked edge that contributes exactly nothing, p_out =
 * 0 (its V row may still be read; V is taken to be finite); an all-masked row gives zeros, lse = -inf; a row with NaN or
 * +inf among its scores has unspecified outputs in that row only.
 * Fixed order: a group of L lanes owns a row; with W = elements per 16 bytes and G(n) = 8, 16, 32 or 64 for n <= 8 W, 16 W,
 * 32 W, else, L = max(G(nk), G(nv)); column j of Q / K and of V / O belongs to lane (j / W) % L.  The dot of an entry is
 * formed as crp_sddmm_csr_* forms it for (dtype, nk), so the bits before `* scale` are the SDDMM's; s = dot * scale (one
 * rounding; bias: + value, one more).  The row goes in batches of 8 entries in ascending p with an online softmax:
 * m' = max(m, batch), f = exp(m - m'), e_u = exp(s_u - m'); l = l * f, then l = l + e_u in ascending u; acc[j] = acc[j] * f,
 * then acc[j] = fma(e_u, V[c_u][j], acc[j]) in ascending u; after the row O = acc / l (IEEE).  The maximum is never
 * deferred.  A row's bits depend on (dtype, nk, nv, scale, bias) and the row's entries in CSR order ONLY: not on alignment,
 * leading dimensions (operands that cannot be accessed in 16-byte pieces are accessed by elements in the same assignment),
 * the source a K / V row comes from, the handle (full matrix or row subset), the optional outputs or the other rows.
 * Error bound: DESIGN.md 5j.
 * Returns 0 (also for a handle without rows, for which nothing is launched), a HIP error (> 0), or a negative argument
 * error, before which nothing is written: -1 for a NULL handle, Q or O, for a NULL K or V source that a code names, for
 * nk < 1 or nv < 1, for a bias other than 0 or 1 and for a non-finite scale; -4 for a leading dimension below its width
 * (nk for Q and K, nv for V and O; of a source that is not NULL). */
int crp_attention_csr_f64(crp_csr_dev_p A, int nk, int nv, double scale, int bias,
                          const double *Q, long long ldQ,
                          const double *K0, long long ldK0, const double *K1, long long ldK1,
                          const double *V0, long long ldV0, const double *V1, long long ldV1,
                          double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream);
int crp_attention_csr_f32(crp_csr_dev_p A, int nk, int nv, double scale, int bias,
                          const float *Q, long long ldQ,
                          const float *K0, long long ldK0, const float *K1, long long ldK1,
                          const float *V0, long long ldV0, const float *V1, long long ldV1,
                          float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream);

/* ---- the fused backward of crp_attention_csr_* ------------------------------------
 * Inputs: Q, K, V, scale and bias as in the forward, O and lse as the forward wrote them, and the upstream gradient dO (a row
 * per row of O).  For every nonzero p = (i, c):
 *   s_p  = scale * < Q[i][0:nk], K[c][0:nk] >      (bias = 1: + the handle's current value of p, as the forward forms it)
 *   p_p  = exp(s_p - lse[i]),   dP_p = < dO[i][0:nv], V[c][0:nv] >,   D_i = < dO[i][0:nv], O[i][0:nv] >,   dS_p = p_p (dP_p - D_i)
 *   dQ[i] = scale * sum over row i of dS_p K[c_p]
 *   dK[c] = scale * sum over column c of dS_p Q[i_p],     dV[c] = sum over column c of p_p dO[i_p]
 * in two calls that re-form the probabilities from lse instead of reading stored ones.  Nothing nnz-sized is written unless
 * ds_out is given, and the handles' values are not touched.
 *   crp_attention_bwd_q_csr_*, over a handle of A (two-source column codes for K and V, a row map selects the Q / O / dO / dQ /
 *   lse / delta row, all as in the forward): writes dQ[i][0:nk] and delta[i] = D_i of every row -- delta is required, one entry
 *   per row, indexed like lse -- and, when ds_out is not NULL, ds_out[out_pos[p]] = dS_p (ds_out[p] when out_pos is NULL): the
 *   gradient of the bias, i.e. of A's values, in the order crp_csr_dev_update_values takes.
 *   crp_attention_bwd_kv_csr_*, over a handle of A^T (crp_csr_dev_create_t: its rows are A's columns, its entries the rows of A
 *   in the stable transposed order; a row map selects the K / V / dK / dV row): one source -- a handle whose codes name a second
 *   source returns -1.  Takes delta as the row side wrote it and writes dK[c][0:nk], dV[c][0:nv] of every row of the handle.
 *   With bias = 1 the value added to s_p is this handle's own current value of the entry.
 * Width cap: a lane keeps the whole of K[c] and V[c], so nk and nv are at most 4 * 64 * W columns each (W = elements per 16
 * bytes): 512 in fp64, 1024 in fp32.  Wider operands return CRP_ATTN_BWD_EWIDTH with nothing written; the chain of the existing
 * calls (p_out, crp_row_softmax_bwd_*, value updates and products) serves those widths.
 * Aliasing: bwd_kv allows dK == K and dV == V exactly (same pointer, same leading dimension): a lane group reads its row of K
 * and V whole before it writes it, and no other group reads that row.  bwd_q allows no output to alias an input.
 * Special cases: lse[i] = -inf (an empty or all-masked row) makes every p and dS of that row +0 and dQ[i] = +0; s_p = -inf
 * gives p = dS = +0 exactly; an empty row of either handle writes +0 to its outputs (delta[i] is still written: a plain dot);
 * NaN or +inf among a row's scores leaves that row's outputs unspecified, and for bwd_kv those of the columns it touches.
 * Fixed order: the lane group and the column-to-lane assignment are the forward's, L = max(G(nk), G(nv)); both dots of an entry
 * and D_i are formed as crp_sddmm_csr_* forms them for (dtype, nk) and (dtype, nv), on both sides, so s, p, dP and dS have the
 * same bits in both calls; s = dot * scale (+ value), p = exp(s - lse), dS = p * (dP - D) (p == 0: +0); entries go in batches
 * of 8 in the handle's CSR order with acc[j] = fma(dS_u, K[c_u][j], acc[j]) (kv: fma(dS_u, Q[i_u][j], .) and fma(p_u,
 * dO[i_u][j], .)) from +0, and dQ = acc * scale (dK likewise; dV = acc).  A row's bits depend on (dtype, nk, nv, scale, bias)
 * and its entries in the handle's CSR order ONLY: not on alignment or leading dimensions, the source a row comes from, the
 * handle (full matrix or row subset), the optional output or the other rows.  Error bound: DESIGN.md 5l.
 * The fp32 forms take scale as a double and round it to float once.  All pointers are device pointers; the launches are
 * asynchronous on `stream`.  Returns 0 (also for a handle without rows, for which nothing is launched), a HIP error (> 0), or
 * a negative argument error, before which nothing is written: -1 for a NULL handle or a NULL required pointer (bwd_q: Q, O, dO,
 * lse, dQ, delta and a K or V source that a code names; bwd_kv: K, V, dK, dV, and Q, dO, lse, delta when the handle has a
 * nonzero), for nk < 1 or nv < 1, a bias other than 0 or 1, a non-finite scale, and for bwd_kv on a handle with negative
 * codes; -4 for a leading dimension below its width; CRP_ATTN_BWD_EWIDTH for nk or nv over the cap. */
#define CRP_ATTN_BWD_EWIDTH (-6)   /* nk or nv above 4 * 64 * (elements per 16 bytes) */
int crp_attention_bwd_q_csr_f64(crp_csr_dev_p A, int nk, int nv, double scale, int bias,
                                const double *Q, long long ldQ,
                                const double *K0, long long ldK0, const double *K1, long long ldK1,
                                const double *V0, long long ldV0, const double *V1, long long ldV1,
                                const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                double *dQ, long long lddQ, double *delta, double *ds_out, const int *out_pos, void *stream);
int crp_attention_bwd_q_csr_f32(crp_csr_dev_p A, int nk, int nv, double scale, int bias,
                                const float *Q, long long ldQ,
                                const float *K0, long long ldK0, const float *K1, long long ldK1,
                                const float *V0, long long ldV0, const float *V1, long long ldV1,
                                const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
                                float *dQ, long long lddQ, float *delta, float *ds_out, const int *out_pos, void *stream);
int crp_attention_bwd_kv_csr_f64(crp_csr_dev_p At, int nk, int nv, double scale, int bias,
                                 const double *K, long long ldK, const double *V, long long ldV,
                                 const double *Q, long long ldQ, const double *dO, long long lddO,
                                 const double *lse, const double *delta,
                                 double *dK, long long lddK, double *dV, long long lddV, void *stream);
int crp_attention_bwd_kv_csr_f32(crp_csr_dev_p At, int nk, int nv, double scale, int bias,
                                 const float *K, long long ldK, const float *V, long long ldV,
                                 const float *Q, long long ldQ, const float *dO, long long lddO,
                                 const float *lse, const float *delta,
                                 float *dK, long long lddK, float *dV, long long lddV, void *stream);

/* ---- Multi-head: the fused attention and its backward over `heads` heads side by side ----------------------------
 * heads = H >= 1 heads of dk columns of Q / K / dQ / dK and dv columns of V / O / dO / dV: the operands have H dk and H dv
 * columns, and head h owns columns [h dk, (h + 1) dk) and [h dv, (h + 1) dv).  For every row i, head h and entry p = (i, c_p):
 *   s_{p,h} = scale * < Q[i]_h, K[c_p]_h >   (bias = 1: + A's value of p, one value per nonzero, shared by the heads)
 *   O[i]_h  = sum_p softmax_p(s_{.,h}) * V[c_p]_h
 * and the backward of the section above per head.  Per-row scalars are (rows, H) row-major -- lse[i H + h], delta[i H + h], with
 * i the row of O (through the row map) -- and per-nonzero outputs (nnz, H): p_out[pos H + h], ds_out[pos H + h] with pos =
 * out_pos[p], or p when out_pos is NULL (out_pos keeps nnz entries).  The gradient of A's value of p is the caller's sum of
 * ds_out[pos H + h] over h.
 * Bit contract: head h of every output equals, bit for bit, the single-head call above with nk = dk and nv = dv on the column
 * views of head h (pointers advanced by h dk / h dv, the same leading dimensions): the instance, the order of the dots, the
 * batches of 8, the rescales and the special cases (an empty row: +0 and lse = -inf for every head; masked edges; all-masked
 * rows, per head) are those of (dtype, dk, dv), so the error bounds of DESIGN.md 5j and 5l hold with nk -> dk, nv -> dv.
 * A group of L(dk, dv) lanes owns the unit (row, head); consecutive groups hold consecutive heads of a row.  The 16-byte path
 * needs the single-head call's conditions and dk, dv multiples of W (they are the unit's nk, nv), so that every head's slice
 * is aligned; else elements, in the same assignment.  bwd_kv keeps dK == K and dV == V legal: a group reads its own slice of
 * the row whole before it writes it, and no other group reads that slice.
 * Errors, all before anything is written: those of the single-head calls, with -1 also for heads < 1, -4 for a leading
 * dimension below heads * dk or heads * dv, and CRP_ATTN_BWD_EWIDTH for a PER-HEAD width dk or dv over the cap (the total
 * width is not capped).  rows * heads units that do not fit one launch (about 2^31 blocks) return a HIP error (> 0). */
int crp_attention_mh_csr_f64(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias,
                             const double *Q, long long ldQ,
                             const double *K0, long long ldK0, const double *K1, long long ldK1,
                             const double *V0, long long ldV0, const double *V1, long long ldV1,
                             double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream);
int crp_attention_mh_csr_f32(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias,
                             const float *Q, long long ldQ,
                             const float *K0, long long ldK0, const float *K1, long long ldK1,
                             const float *V0, long long ldV0, const float *V1, long long ldV1,
                             float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream);
int crp_attention_bwd_q_mh_csr_f64(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias,
                                   const double *Q, long long ldQ,
                                   const double *K0, long long ldK0, const double *K1, long long ldK1,
                                   const double *V0, long long ldV0, const double *V1, long long ldV1,
                                   const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                   double *dQ, long long lddQ, double *delta, double *ds_out, const int *out_pos, void *stream);
int crp_attention_bwd_q_mh_csr_f32(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias,
                                   const float *Q, long long ldQ,
                                   const float *K0, long long ldK0, const float *K1, long long ldK1,
                                   const float *V0, long long ldV0, const float *V1, long long ldV1,
                                   const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
                                   float *dQ, long long lddQ, float *delta, float *ds_out, const int *out_pos, void *stream);
int crp_attention_bwd_kv_mh_csr_f64(crp_csr_dev_p At, int heads, int dk, int dv, double scale, int bias,
                                    const double *K, long long ldK, const double *V, long long ldV,
                                    const double *Q, long long ldQ, const double *dO, long long lddO,
                                    const double *lse, const double *delta,
                                    double *dK, long long lddK, double *dV, long long lddV, void *stream);
int crp_attention_bwd_kv_mh_csr_f32(crp_csr_dev_p At, int heads, int dk, int dv, double scale, int bias,
                                    const float *K, long long ldK, const float *V, long long ldV,
                                    const float *Q, long long ldQ, const float *dO, long long lddO,
                                    const float *lse, const float *delta,
                                    float *dK, long long lddK, float *dV, long long lddV, void *stream);

/* ---- fused GAT attention: additive LeakyReLU scores over A's pattern, forward and backward --------------------------
 * The score of a graph attention layer in place of the scaled dot product: two scalars per node and head, and no K.  For every
 * row i of the handle, head h < heads and entry p = (i, c_p), p in the handle's CSR order:
 *   z = el[i][h] + er[c_p][h]                    (one rounding)
 *   a = z > 0 ? z : slope * z                    (one rounding: torch.nn.functional.leaky_relu)
 *   s = a        (bias = 1: s = a + A's current value of p, one more rounding; the value is shared by the heads, and the fp32
 *                 form adds the fp32 copy that crp_sddmm_csr_f32 mode 1 uses)
 *   O[i]_h = sum_p softmax_p(s) * V[c_p]_h
 * Every step is rounded on its own: slope * z + value is never contracted into an FMA.  slope is any finite double; the fp32
 * form rounds it to float once; slope = 1 is the plain additive score.
 * Operands (row-major device pointers): V / O / dO / dV have heads * dv columns, head h owns columns [h dv, (h + 1) dv).  el is
 * (rows of O, heads) with ldel >= heads, read through the handle's row map like Q of crp_attention_csr_*; er0 / er1 are the two
 * sources of the column code exactly as V0 / V1 (lder >= heads; a source no code names may be NULL).  Per-row scalars lse,
 * delta, d_el are (rows, heads) -- lse and delta contiguous, entry i heads + h with i the row of O -- and the per-nonzero
 * outputs p_out, ds_out are (nnz, heads): entry pos heads + h with pos = out_pos[p], or p when out_pos is NULL.
 * Forward: from the scores on this is crp_attention_mh_csr_* verbatim -- batches of 8 entries in ascending p, m' = max(m,
 * batch), f = exp(m - m'), e_u = exp(s_u - m'), l = l f then l + e_u in ascending u, acc = acc f then fma(e_u, V[c_u][j], acc) in
 * ascending u, O = acc / l, lse = m + log l, p_out = exp(s - m) / l, the maximum never deferred -- so O, lse and p_out are bit
 * for bit what that order gives for these scores and (dtype, dv).  A group of G(dv) lanes owns the unit (row, head); each lane
 * forms the score of entry (lane & 7) of a batch from one scalar load of er.  Special cases as there: an empty row writes +0
 * and lse = -inf for every head; a one-entry row gives O = V[c] bit for bit; s = -inf (a bias value of -inf, or z = -inf with
 * slope > 0) is a masked edge; an all-masked row gives zeros; NaN or +inf among a row's scores (slope = 0 with an infinite z is
 * this case) leaves that row's outputs unspecified.
 * Backward, from el, er, V, O, lse and dO, with s re-formed exactly as above:  p = exp(s - lse[i][h]),  dP = < dO[i]_h, V[c]_h >,
 * D = < dO[i]_h, O[i]_h > (both as crp_sddmm_csr_* forms a dot for (dtype, dv)),  dS = p (dP - D) (p == 0: +0),  dZ = dS g with
 * g = z > 0 ? 1 : slope (one rounding).
 *   crp_gat_attention_bwd_row_csr_*, over a handle of A (two sources, row map and out_pos as in crp_attention_bwd_q_mh_csr_*):
 *   writes delta[i][h] = D and d_el[i][h] = the sum of the row's dZ -- one IEEE addition per entry from +0 in ascending p -- both
 *   required, and, when ds_out is not NULL, ds_out[(pos, h)] = dS: the gradient of A's values per head.
 *   crp_gat_attention_bwd_col_csr_*, over a handle of A^T (crp_csr_dev_create_t; one source: negative codes return -1; the row
 *   map selects the er / V / d_er / dV row): takes delta as the row side wrote it and writes d_er[c][h] = the sum of the column's
 *   dZ, from +0 in the handle's CSR order, and dV[c]_h with acc = fma(p_u, dO[i_u][j], acc) from +0 in that order.  With bias = 1
 *   the value added is this handle's own value of the entry.  dV == V with the same pointer and leading dimension is legal; no
 *   other aliasing is.
 * s, p, dP, dS and dZ have the same bits on both sides.  Rows with lse = -inf give +0 everywhere; delta is still written.  The
 * per-head width cap is the attention backward's: dv <= 4 * 64 * W, else CRP_ATTN_BWD_EWIDTH with nothing written.
 * Error bounds: DESIGN.md 5o.  Asynchronous on `stream`.  Returns 0 (also for a handle without rows: nothing is launched), a
 * HIP error (> 0; rows * heads units that do not fit one launch among them), or a negative argument error before which nothing
 * is written: -1 for a NULL handle or required pointer (forward: el, O and an er or V source that a code names; row side also
 * dO, lse, d_el, delta; column side: er, V, d_er, dV, and el, dO, lse, delta when the handle has a nonzero), heads < 1, dv < 1, a
 * bias other than 0 or 1, a non-finite slope; -4 for a leading dimension below its width (heads, or heads * dv). */
int crp_gat_attention_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                              const double *el, long long ldel,
                              const double *er0, long long lder0, const double *er1, long long lder1,
                              const double *V0, long long ldV0, const double *V1, long long ldV1,
                              double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream);
int crp_gat_attention_bwd_row_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                      const double *el, long long ldel,
                                      const double *er0, long long lder0, const double *er1, long long lder1,
                                      const double *V0, long long ldV0, const double *V1, long long ldV1,
                                      const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                      double *d_el, long long ldd_el, double *delta, double *ds_out, const int *out_pos, void *stream);
int crp_gat_attention_bwd_col_csr_f64(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
                                      const double *er, long long lder, const double *V, long long ldV,
                                      const double *el, long long ldel, const double *dO, long long lddO,
                                      const double *lse, const double *delta,
                                      double *d_er, long long ldd_er, double *dV, long long lddV, void *stream);
int crp_gat_attention_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                              const float *el, long long ldel,
                              const float *er0, long long lder0, const float *er1, long long lder1,
                              const float *V0, long long ldV0, const float *V1, long long ldV1,
                              float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream);
int crp_gat_attention_bwd_row_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                      const float *el, long long ldel,
                                      const float *er0, long long lder0, const float *er1, long long lder1,
                                      const float *V0, long long ldV0, const float *V1, long long ldV1,
                                      const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
                                      float *d_el, long long ldd_el, float *delta, float *ds_out, const int *out_pos, void *stream);
int crp_gat_attention_bwd_col_csr_f32(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
                                      const float *er, long long lder, const float *V, long long ldV,
                                      const float *el, long long ldel, const float *dO, long long lddO,
                                      const float *lse, const float *delta,
                                      float *d_er, long long ldd_er, float *dV, long long lddV, void *stream);

/* ---- fused GATv2 attention: a LeakyReLU inside the dot with a, over A's pattern, forward and backward ----------------
 * The score of a GATv2 layer.  For every row i of the handle, head h < heads and entry p = (i, c_p), p in the handle's CSR order:
 *   z_j = XT[i]_h[j] + XS[c_p]_h[j]              (one rounding)
 *   r_j = z_j > 0 ? z_j : slope * z_j            (one rounding, never contracted with anything)
 *   s   = sum_j a_h[j] r_j                       (as crp_sddmm_csr_* forms a dot for (dtype, dv): per lane fma(a_j, r_j, acc) in
 *                                                 ascending j from +0 in the SDDMM's column-to-lane assignment for G(dv) lanes,
 *                                                 then the balanced binary tree over the lane number)
 *   bias = 1: s = s + A's current value of p, one more rounding (shared by the heads; fp32: the fp32 copy of crp_sddmm_csr_f32)
 *   O[i]_h = sum_p softmax_p(s) * XS[c_p]_h
 * The gathered row XS[c] is the score operand and the value operand.  slope is any finite double; the fp32 form rounds it to
 * float once.
 * Operands (row-major device pointers): XT / O / dO / dXT / da_part / dXS have heads * dv columns, head h owns columns
 * [h dv, (h + 1) dv).  XT is (rows of O, heads * dv), read through the handle's row map like Q of crp_attention_csr_*; XS0 / XS1
 * are the two sources of the column code exactly as V0 / V1 of crp_gat_attention_csr_* (a source no code names may be NULL); a is
 * heads * dv contiguous elements.  lse and delta are (rows, heads), contiguous; p_out and ds_out are (nnz, heads): entry
 * pos heads + h with pos = out_pos[p], or p when out_pos is NULL.
 * Forward: from s on this is crp_attention_mh_csr_* verbatim (batches of 8 in ascending p, the maximum taken at every batch,
 * O = acc / l, lse = m + log l, p_out = exp(s - m) / l, acc = fma(e_u, XS[c_u][j], acc)): O, lse and p_out are bit for bit what
 * that order gives for these scores and (dtype, dv).  Special cases as there and as crp_gat_attention_csr_*: an empty row writes
 * +0 and lse = -inf for every head; a one-entry row gives O = XS[c] bit for bit; s = -inf is a masked edge; an all-masked row
 * writes zeros; NaN or +inf among a row's scores leaves that row's outputs unspecified.  XS is taken to be finite.
 * Backward, with s re-formed exactly as above:  p = exp(s - lse[i][h]),  dP = < dO[i]_h, XS[c]_h >,  D = < dO[i]_h, O[i]_h > (both
 * the SDDMM's dot for (dtype, dv)),  dS = p (dP - D) (p == 0: +0),  ag_j = z_j > 0 ? a_j : as_j with as_j = fl(a_j slope).
 *   crp_gatv2_attention_bwd_row_csr_*, over a handle of A (two sources, row map, out_pos): writes delta[i][h] = D,
 *   dXT[i]_h[j] with acc = fma(dS_p, ag_pj, acc) and da_part[i]_h[j] with acc = fma(dS_p, r_pj, acc), both from +0 in ascending p
 *   -- da_part (rows, heads * dv) is the row's share of the gradient of a: crp_col_sum_* of it over the rows is da, nothing
 *   nnz-sized is stored; all three required -- and, when ds_out is not NULL, ds_out[(pos, h)] = dS.  A row-subset handle writes
 *   the rows its map names and no others.
 *   crp_gatv2_attention_bwd_col_csr_*, over a handle of A^T (crp_csr_dev_create_t; one source: negative codes return -1; the
 *   row map selects the XS / dXS row): takes delta as the row side wrote it, keeps accZ = fma(dS, ag, accZ) and
 *   accV = fma(p, dO[i][j], accV) from +0 in that handle's CSR order and writes dXS[c]_h = accZ + accV, one addition.  With
 *   XT = 0 and slope = 1 the two are the bits of crp_attention_bwd_kv_mh_csr_*'s dK and dV for Q = a in every row, K = V = XS.
 *   With bias = 1 the value added is this handle's own value of the entry.  dXS == XS with the same pointer and leading
 *   dimension is legal; no other aliasing is.
 * s, p, dP and dS have the same bits on both sides.  Rows with lse = -inf give +0 everywhere; delta is still written.
 * Width cap, both directions: a lane keeps its pieces of XT (or XS[c]), a and as for the unit, so dv <= 4 * 64 * W per head (512
 * in fp64, 1024 in fp32); wider heads return CRP_GATV2_EWIDTH with nothing written.
 * Error bounds: DESIGN.md 5p.  Asynchronous on `stream`; the stream contract of the attention calls holds word for word.
 * Returns 0 (also for a handle without rows: nothing is launched), a HIP error (> 0), or a negative argument error before which
 * nothing is written: -1 for a NULL handle or required pointer (forward: XT, a, O and a source that a code names; row side also
 * dO, lse, dXT, da_part, delta; column side: XS, a, dXS, and XT, dO, lse, delta when the handle has a nonzero), heads < 1,
 * dv < 1, a bias other than 0 or 1, a non-finite slope, negative column codes on the column side; -4 for a leading dimension
 * below heads * dv; CRP_GATV2_EWIDTH. */
#define CRP_GATV2_EWIDTH (-6)      /* dv above 4 * 64 * (elements per 16 bytes): the value of CRP_ATTN_BWD_EWIDTH */
int crp_gatv2_attention_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                const double *XT, long long ldXT,
                                const double *XS0, long long ldXS0, const double *XS1, long long ldXS1, const double *a,
                                double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream);
int crp_gatv2_attention_bwd_row_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                        const double *XT, long long ldXT,
                                        const double *XS0, long long ldXS0, const double *XS1, long long ldXS1, const double *a,
                                        const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                        double *dXT, long long lddXT, double *da_part, long long ldda,
                                        double *delta, double *ds_out, const int *out_pos, void *stream);
int crp_gatv2_attention_bwd_col_csr_f64(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
                                        const double *XS, long long ldXS, const double *XT, long long ldXT, const double *a,
                                        const double *dO, long long lddO, const double *lse, const double *delta,
                                        double *dXS, long long lddXS, void *stream);
int crp_gatv2_attention_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                const float *XT, long long ldXT,
                                const float *XS0, long long ldXS0, const float *XS1, long long ldXS1, const float *a,
                                float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream);
int crp_gatv2_attention_bwd_row_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
                                        const float *XT, long long ldXT,
                                        const float *XS0, long long ldXS0, const float *XS1, long long ldXS1, const float *a,
                                        const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
                                        float *dXT, long long lddXT, float *da_part, long long ldda,
                                        float *delta, float *ds_out, const int *out_pos, void *stream);
int crp_gatv2_attention_bwd_col_csr_f32(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
                                        const float *XS, long long ldXS, const float *XT, long long ldXT, const float *a,
                                        const float *dO, long long lddO, const float *lse, const float *delta,
                                        float *dXS, long long lddXS, void *stream);

/* ---- attention dropout in the fused GAT and GATv2 calls, both directions -----------------------------------------------
 * The crp_gat_attention_*_csr_* and crp_gatv2_attention_*_csr_* calls above with the attention coefficients dropped after the
 * edge softmax at rate `drop` and rescaled by 1 / (1 - drop): the same argument lists with (drop, seed) before the stream.  No
 * mask is stored: the keep bit of an edge is a pure function of (seed, r, c, h), so the forward, both sides of the backward and
 * crp_dropout_mask_csr re-form it, and nothing nnz-sized lies between forward and backward, as before.
 * The mask.  Philox4x32-10 (multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds, the key
 * bumped after each) with key = (seed's low word, seed's high word) and counter = (r, c, h, 0); x = output word 0; the edge is kept
 * iff x >= thr with thr = (uint32) floor(drop 2^32), formed once on the host in double.  r is the index of the row of O / el / XT /
 * lse the entry belongs to -- on a handle of A after the handle's row map, on a handle of A^T the entry's column index -- and c the
 * 32-bit column code as stored: on a handle of A the entry's code (a second-source code goes in as its bit pattern), on a handle of
 * A^T the index of the er / V / XS row after that handle's row map.  On a one-source pair both handles therefore draw the same
 * bit for the same edge.  Duplicate (r, c) entries share a bit.  For 0 < drop < 2^-32 every edge is kept and the scale still
 * applies.  rs = (T) (1.0 / (1.0 - drop)), formed in double and rounded once to the dtype.
 * Forward, with k_p the keep bit: scores, batches, m, f, e_u and l are exactly the plain call's -- the softmax runs over all
 * edges -- and only the accumulator changes: acc = fma(k_u ? e_u : +0, V[c_u][j], acc), and O = fl(fl(acc / l) rs).  lse and p_out
 * are untouched by dropout: bit for bit what the call without it writes.  A row whose edges are all dropped but not all masked
 * gives O = +0 with its finite lse.
 * Backward: p, s, g and D = < dO, O > as in the plain call (O is the dropped O, so D is the softmax Jacobian's term unchanged);
 * dP' = k ? fl(dP rs) : +0,  dS = p (dP' - D),  and the value-side weight is w = k ? fl(p rs) : +0, used in
 * dV[c] = fma(w_u, dO[i_u][j], acc) (GATv2: in accV).  Everything downstream -- dZ, d_el, d_er, dXT, da_part, accZ and
 * ds_out = dS -- is unchanged.  The two products with rs are roundings of their own, never contracted with the subtraction.
 * s, p, dP', dS and k have the same bits on the row side and on the column side.
 * Head h of a heads-head call is NOT the one-head call on head h's views: the key holds h.
 * drop == 0 takes the plain call's kernels: the same bits at the same cost.  Returns as the plain calls, and -1, before anything
 * is written, for a drop that is NaN or outside [0, 1).  Error bounds: DESIGN.md 5q. */
int crp_gat_attention_drop_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const double *el, long long ldel, const double *er0, long long lder0, const double *er1, long long lder1,
        const double *V0, long long ldV0, const double *V1, long long ldV1,
        double *O, long long ldO, double *lse, double *p_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gat_attention_drop_bwd_row_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const double *el, long long ldel, const double *er0, long long lder0, const double *er1, long long lder1,
        const double *V0, long long ldV0, const double *V1, long long ldV1,
        const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
        double *d_el, long long ldd_el, double *delta, double *ds_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gat_attention_drop_bwd_col_csr_f64(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
        const double *er, long long lder, const double *V, long long ldV,
        const double *el, long long ldel, const double *dO, long long lddO, const double *lse, const double *delta,
        double *d_er, long long ldd_er, double *dV, long long lddV,
        double drop, unsigned long long seed, void *stream);
int crp_gat_attention_drop_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const float *el, long long ldel, const float *er0, long long lder0, const float *er1, long long lder1,
        const float *V0, long long ldV0, const float *V1, long long ldV1,
        float *O, long long ldO, float *lse, float *p_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gat_attention_drop_bwd_row_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const float *el, long long ldel, const float *er0, long long lder0, const float *er1, long long lder1,
        const float *V0, long long ldV0, const float *V1, long long ldV1,
        const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
        float *d_el, long long ldd_el, float *delta, float *ds_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gat_attention_drop_bwd_col_csr_f32(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
        const float *er, long long lder, const float *V, long long ldV,
        const float *el, long long ldel, const float *dO, long long lddO, const float *lse, const float *delta,
        float *d_er, long long ldd_er, float *dV, long long lddV,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const double *XT, long long ldXT, const double *XS0, long long ldXS0, const double *XS1, long long ldXS1, const double *a,
        double *O, long long ldO, double *lse, double *p_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_bwd_row_csr_f64(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const double *XT, long long ldXT, const double *XS0, long long ldXS0, const double *XS1, long long ldXS1, const double *a,
        const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
        double *dXT, long long lddXT, double *da_part, long long ldda, double *delta, double *ds_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_bwd_col_csr_f64(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
        const double *XS, long long ldXS, const double *XT, long long ldXT, const double *a,
        const double *dO, long long lddO, const double *lse, const double *delta, double *dXS, long long lddXS,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const float *XT, long long ldXT, const float *XS0, long long ldXS0, const float *XS1, long long ldXS1, const float *a,
        float *O, long long ldO, float *lse, float *p_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_bwd_row_csr_f32(crp_csr_dev_p A, int heads, int dv, double slope, int bias,
        const float *XT, long long ldXT, const float *XS0, long long ldXS0, const float *XS1, long long ldXS1, const float *a,
        const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
        float *dXT, long long lddXT, float *da_part, long long ldda, float *delta, float *ds_out, const int *out_pos,
        double drop, unsigned long long seed, void *stream);
int crp_gatv2_attention_drop_bwd_col_csr_f32(crp_csr_dev_p At, int heads, int dv, double slope, int bias,
        const float *XS, long long ldXS, const float *XT, long long ldXT, const float *a,
        const float *dO, long long lddO, const float *lse, const float *delta, float *dXS, long long lddXS,
        double drop, unsigned long long seed, void *stream);

/* The mask on its own.  crp_dropout_keep_host: the keep bit (1 or 0) of edge (r, c) and head h, pure host code that needs no
 * device; -1 for a drop that is NaN or outside [0, 1).  crp_dropout_mask_csr: the (nnz, heads) keep flags of a handle as bytes 1 /
 * 0 in p_out's layout -- entry (pos, h) at pos heads + h with pos = out_pos[p], or p when out_pos is NULL -- with (r, c) of every
 * entry as stated above, over a handle of A or of A^T (crp_csr_dev_create_t): what the fused calls re-form, for callers who run
 * the chain of separate calls.  drop == 0 writes ones.  Asynchronous on `stream`.  Returns 0 (a handle without nonzeros: nothing
 * is launched), a HIP error (> 0), or -1 before anything is written: a NULL handle, heads < 1, a bad drop, a NULL mask. */
int crp_dropout_keep_host(unsigned long long seed, unsigned r, unsigned c, unsigned h, double drop);
int crp_dropout_mask_csr(crp_csr_dev_p A, int heads, double drop, unsigned long long seed, unsigned char *mask,
                         const int *out_pos, void *stream);

/* ---- row softmax over A's pattern (edge softmax) and its Jacobian product ------
 * For every row r with entries p in [rowptr[r], rowptr[r + 1]):
 *   forward :  m = max_p s[p],  e_p = exp(s[p] - m),  y[p] = e_p / sum_q e_q
 *   backward:  D = sum_q y[q] * dy[q] (accumulated with FMAs),  ds[p] = y[p] * (dy[p] - D)
 * -- the step between crp_sddmm_csr_* (which writes s) and a value update (which takes y), and its backward.  exp / expf are
 * the device library's functions, the division is IEEE.  No atomics, no LDS, no partial result in memory.
 * Raw forms: rowptr is a device int32 array of nrow + 1 non-decreasing entries that index s / y (dy, ds) directly;
 * rowptr[0] need not be 0, so `rowptr + r0` with fewer rows addresses a row subset of the same arrays.  Only the entries
 * rowptr[0] .. rowptr[nrow] - 1 are read or written.  Handle forms: the handle's own device row pointer; p counts in the
 * handle's CSR order, as for crp_sddmm_csr_* (a crp_csr_dev_create_t handle: the transposed order).  All pointers are
 * device pointers; the launch is asynchronous on `stream`.
 * Special cases: an empty row reads and writes nothing; a row of one finite entry gives exactly 1.0; an entry of -inf is a
 * masked edge, its y is exactly 0; a row whose entries are all -inf gives all zeros, not NaN; a row that holds NaN or +inf
 * has unspecified outputs for that row only -- other rows are unaffected and nothing faults.
 * Fixed order: both sums are formed from 64 strided partials -- partial k adds entries k, k + 64, k + 128, ... of the row in
 * ascending order, starting from +0 -- which meet in the balanced binary tree over k (k with k ^ 1, then k ^ 2, ... k ^ 32),
 * every node one IEEE addition.  The order is a function of the dtype ONLY: not of the row's position, the row pointer's
 * first value, pointer alignment, the kernel instance (a group of 8, 16, 32 or 64 lanes per row, which the kernel picks
 * from the launch's mean row length (rowptr[nrow] - rowptr[0]) / nrow) or the other rows of the call.  Repeated calls are
 * bit-identical, and a row subset reproduces the full call's entries bit for bit.
 * Aliasing: exact aliasing is allowed (y == s; ds == dy or ds == y), partial overlap is not.  Every element is read and
 * later written by the same lane; a row of up to 8 entries per lane of its group is read entirely before its first write,
 * in a longer row every element's last read precedes its own write.
 * Error bounds (u = 2^-53 / 2^-24; L = the row's length, T = max_p (m - s[p]) over its finite entries; against the exact
 * result of the dtype-rounded inputs, results away from the subnormal range):
 *   |y - ref|  <= 1.01 (L + 2 T + 8) u ref                      (exp within 2 ulp)
 *   |ds - ref| <= 1.01 u |y_p| ((L + 2) S + 2 |dy_p|),  S = sum_q |y_q dy_q|.
 * Return: 0 on success -- also for nrow == 0, for which nothing is launched; -1 for nrow < 0, a NULL handle, or a NULL
 * pointer when nrow > 0; a positive HIP error otherwise.  Nothing is written before the arguments have passed. */
int crp_row_softmax_f64(int nrow, const int *rowptr, const double *s, double *y, void *stream);
int crp_row_softmax_f32(int nrow, const int *rowptr, const float *s, float *y, void *stream);
int crp_row_softmax_bwd_f64(int nrow, const int *rowptr, const double *y, const double *dy, double *ds, void *stream);
int crp_row_softmax_bwd_f32(int nrow, const int *rowptr, const float *y, const float *dy, float *ds, void *stream);
int crp_csr_dev_row_softmax_f64(crp_csr_dev_p A, const double *s, double *y, void *stream);
int crp_csr_dev_row_softmax_f32(crp_csr_dev_p A, const float *s, float *y, void *stream);
int crp_csr_dev_row_softmax_bwd_f64(crp_csr_dev_p A, const double *y, const double *dy, double *ds, void *stream);
int crp_csr_dev_row_softmax_bwd_f32(crp_csr_dev_p A, const float *y, const float *dy, float *ds, void *stream);

/* ---- row gather / scatter (pack / unpack of the B exchange) ----------------
 * gather : dst[i][0:n] = src[ridx[i]][0:n]   (i < nidx)
 * scatter: dst[ridx[i]][0:n] = src[i][0:n]
 * layout 0: rows are contiguous (row-major, leading dimensions in elements);
 * layout 1: column-major operands (element (r, j) at r + j*ld).  ridx is a
 * device array of int32. */
int crp_gather_rows_f64(int layout, int nidx, int n, const int *ridx,
                        const double *src, long long lds,
                        double *dst, long long ldd, void *stream);
int crp_scatter_rows_f64(int layout, int nidx, int n, const int *ridx,
                         const double *src, long long lds,
                         double *dst, long long ldd, void *stream);
/* segmented accumulate (row-major): dst[seg_row[t]][0:n] += src[seg_pos[k]][0:n] for k = seg_ptr[t] .. seg_ptr[t + 1] - 1,
 * added one after the other in that order, for t < nseg.  seg_row holds distinct rows, so no two threads touch one
 * element: no atomics, and repeated calls are bit-identical (the reduce of C of the row-parallel engine's transposed
 * product, where one local row can come back from several peers).  seg_row / seg_ptr / seg_pos are device arrays. */
int crp_scatter_add_rows_f64(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos,
                             const double *src, long long lds, double *dst, long long ldd, void *stream);
/* the fp32 instance of the same kernel (the reduce of crp_rp_spmm_exec_t_f32_ex): plain IEEE fp32 additions in list order.
 * Pieces of 16 bytes (4 floats; the fp64 form: 2 doubles) when n, lds, ldd and both pointers keep them aligned, single
 * elements otherwise -- the same bits either way.  Arguments and return codes as the fp64 form: -1 for a negative count or,
 * with work to do, a NULL pointer; 0 when nseg or n is 0 (nothing is launched); a positive HIP error. */
int crp_scatter_add_rows_f32(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos,
                             const float *src, long long lds, float *dst, long long ldd, void *stream);
/* value gather: dst[i] = (double) src[map ? map[i] : i] for i < n; map (device int32, may repeat positions) == NULL is a
 * copy / a widening.  Widening fp32 to fp64 is exact, so the fp32 copies a handle derives from dst with (float) are the
 * caller's fp32 bits again: a device value update from fp32 values (crp_rp_spmm_update_values_dev) needs no fp32 value
 * store in the handle.  Asynchronous on `stream`; device pointers.  Returns 0 (n == 0: nothing is launched), -1 for n < 0
 * or, with n > 0, a NULL src or dst, or a positive HIP error. */
int crp_gather_vals_f64(long long n, const int *map, const double *src, double *dst, void *stream);
int crp_gather_vals_f32_f64(long long n, const int *map, const float *src, double *dst, void *stream);
/* sum of segments: out[p] = ((src[p] + src[seg_stride + p]) + src[2 * seg_stride + p]) + ... for 0 <= p < len, strictly left
 * to right over ascending segment number (the grid-row reduction of the 2D engine's SDDMM, crp_para2d_spmm_sddmm_ex).
 * Plain IEEE additions, no atomics and no LDS; every out[p] belongs to one thread; nseg == 1 is a copy.  Pieces of 16 bytes
 * when src, out and seg_stride keep them aligned, single elements otherwise and for the tail, in the same order: the result
 * does not depend on alignment, and repeated calls are bit-identical.  Asynchronous on `stream`; device pointers.  Returns 0
 * (also for len == 0: nothing is launched), -1 for a NULL pointer, nseg < 1 or len < 0, -4 for seg_stride < len with
 * nseg > 1, or a positive HIP error; nothing is written before the arguments have passed. */
int crp_sum_segments_f64(int nseg, long long len, const double *src, long long seg_stride, double *out, void *stream);
int crp_sum_segments_f32(int nseg, long long len, const float *src, long long seg_stride, float *out, void *stream);
/* column sums: out[j] = the sum over r < nrow of src[r * lds + j] for j < n (da of the GATv2 backward from da_part).  Rows are
 * taken in blocks of 256 consecutive rows; a block's sum per column runs from +0 in ascending row into work[b * n + j], and the
 * block sums are then added left to right in ascending block, which is crp_sum_segments_*'s order.  work holds
 * ceil(nrow / 256) * n elements.  Plain IEEE additions, no atomics and no LDS: the bits are a function of (dtype, nrow, n, data)
 * only, not of lds or alignment, and repeated calls are bit-identical.  nrow == 0 writes +0.  Asynchronous on `stream`; device
 * pointers.  Returns 0, -1 for a negative count, a NULL out or, with work to do, a NULL src or work, -4 for lds < n, or a
 * positive HIP error; nothing is written before the arguments have passed. */
int crp_col_sum_f64(int nrow, int n, const double *src, long long lds, double *work, double *out, void *stream);
int crp_col_sum_f32(int nrow, int n, const float *src, long long lds, float *work, float *out, void *stream);
/* out-of-place transpose: dst[c][r] = src[r][c] for an nrow x ncol row-major
 * src (equivalently col-major <-> row-major conversion). */
int crp_transpose_f64(int nrow, int ncol, const double *src, long long lds,
                      double *dst, long long ldd, void *stream);
/* fp32 forms of the three above, same contracts (the fp32 exec of the engines packs and transposes with them).
 * Row-major rows move in 16-byte accesses when n, lds, ldd are multiples of 4 and src, dst 16-byte aligned
 * (8-byte accesses for multiples of 2 and 8-byte alignment, single floats otherwise). */
int crp_gather_rows_f32(int layout, int nidx, int n, const int *ridx,
                        const float *src, long long lds,
                        float *dst, long long ldd, void *stream);
int crp_scatter_rows_f32(int layout, int nidx, int n, const int *ridx,
                         const float *src, long long lds,
                         float *dst, long long ldd, void *stream);
int crp_transpose_f32(int nrow, int ncol, const float *src, long long lds,
                      float *dst, long long ldd, void *stream);

/* Diagnostics for the exchange / compute overlap (tools/overlap_probe.py): a stand-in for a transport's copy kernel --
 * `blocks` workgroups of 256 threads copy `bytes` (a multiple of 16) between device buffers and record the 100 MHz device
 * wall clock: stamps_dev[0] = earliest workgroup start (initialise to ~0), stamps_dev[1] = latest end (initialise to 0);
 * crp_probe_stamp writes the clock to *out_dev from a one-thread kernel.  crp_stream_create_cu_mask creates a stream whose
 * kernels run only on the compute units whose bit is set in mask32 (words of 32 CUs; hipExtStreamCreateWithCUMask). */
int crp_probe_copy(long long bytes, const void *src_dev, void *dst_dev, int blocks, unsigned long long *stamps_dev, void *stream);
int crp_probe_stamp(unsigned long long *out_dev, void *stream);
int crp_stream_create_cu_mask(void **stream, int nwords, const unsigned *mask32);

/* Library identification: "crpspmm-hip <version> gfx950". */
const char *crp_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif
