/*
 * crp_engine.h -- communicator-agnostic C ABI of the two CRP-SpMM engines.
 *
 * Same operations, argument meaning and error behaviour as the reference's
 * public API, with the MPI_Comm replaced by a crp_comm_t* (crp_comm.h):
 *
 *   reference (/root/reference)                         this header
 *   --------------------------------------------------  -----------------------
 *   rp_spmm_init        src/rowpara_spmm.h:60-64         crp_rp_spmm_init
 *   rp_spmm_exec        src/rowpara_spmm.h:78-81         crp_rp_spmm_exec
 *   rp_spmm_free        src/rowpara_spmm.h:67            crp_rp_spmm_free
 *   rp_spmm_print_stat  src/rowpara_spmm.h:84            crp_rp_spmm_print_stat
 *   rp_spmm_clear_stat  src/rowpara_spmm.h:87            crp_rp_spmm_clear_stat
 *   para2d_spmm_*       src/para2d_spmm.h:42-75          crp_para2d_spmm_*
 *
 * include/rowpara_spmm.h and include/para2d_spmm.h are the MPI-typed facade
 * (exact reference signatures) over these functions.
 *
 * Differences that are deliberate ("reference defects"):
 *   - A is uploaded once at init and stays device-resident; exec does no
 *     malloc/free and creates no sparse handle (defect 6);
 *   - locally owned B rows are read in place: there is no self-to-self copy
 *     (defect 7), received rows land contiguously so there is no unpack pass;
 *   - all offsets are 64-bit internally (defect 3);
 *   - para2d at one rank does not self-send (defect 1).
 * B and C may be host pointers (staged through device buffers, as the
 * reference API implies) or device pointers (detected automatically; the
 * zero-copy path the benchmark uses).
 */
#ifndef CRP_ENGINE_H
#define CRP_ENGINE_H

#include <stddef.h>
#include <stdint.h>
#include "crp_comm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crp_rp_spmm     *crp_rp_spmm_p;
typedef struct crp_para2d_spmm *crp_para2d_spmm_p;

/* Host-side view of the exchange plan: the fields of struct rowpara_spmm
 * (src/rowpara_spmm.h:8-40), same names and meaning (counts / displs are in
 * ELEMENTS = rows * glb_n, as the reference stores them, but 64-bit). */
typedef struct crp_rp_plan_view
{
    int nproc, my_rank, glb_n, A_nrow, rB_nrow;
    int rB_self_src_offset, rB_self_dst_offset, rB_self_nrow;
    int rB_p2p, rB_reidx;
    const int       *A_rowptr;           /* A_nrow + 1, rebased to 0          */
    const int       *A_colidx;           /* compact (re-indexed) column ids   */
    const double    *A_val;
    const int       *rB_self_src_ridxs;  /* rB_self_nrow global row ids       */
    const long long *rB_scnts, *rB_sdispls;   /* nproc, nproc + 1             */
    const int       *rB_sridxs;          /* local B row ids to send           */
    const long long *rB_rcnts, *rB_rdispls;
    const int       *rB_rridxs;          /* compact rB row ids of received rows */
    size_t rB_recv_size;                 /* rows received from other ranks    */
    int    n_exec;
    double t_init, t_pack, t_a2a, t_unpack, t_spmm, t_exec;
} crp_rp_plan_view_t;

/* See rp_spmm_init (src/rowpara_spmm.h:49-64).  A_rowptr is a slice of the
 * global row pointer (global nnz offsets; rebased internally), A_srow is
 * accepted and ignored exactly like the reference.  comm is not duplicated
 * and must outlive the engine.  Honours RP_SPMM_P2P / RP_SPMM_REIDX
 * (src/rowpara_spmm.c:42-43).  On failure prints "[FATAL] ..." and aborts,
 * like ASSERT_PRINTF (src/utils.h:58-68). */
void crp_rp_spmm_init(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx,
                      const double *A_val, const int *B_row_displs, int glb_n,
                      crp_comm_t *comm, crp_rp_spmm_p *rp_spmm);
void crp_rp_spmm_free(crp_rp_spmm_p *rp_spmm);
/* C := A * B.  BC_layout 0 row-major / 1 column-major; NULL engine is a no-op
 * (src/rowpara_spmm.c:217). */
void crp_rp_spmm_exec(crp_rp_spmm_p rp_spmm, int BC_layout, const double *B, int ldB,
                      double *C, int ldC);
/* Same, 64-bit leading dimensions and an explicit HIP stream, taken literally
 * (NULL = the null stream; crp_rp_spmm_exec uses a stream the engine owns).
 * With device pointers and timing off nothing synchronises. */
void crp_rp_spmm_exec_ex(crp_rp_spmm_p rp_spmm, int BC_layout, const double *B, long long ldB,
                         double *C, long long ldC, void *stream);
/* The fp32 exec: B and C in fp32, fp32 FMAs (crp_spmm_csr_f32) on A's fp32 copies, which follow
 * crp_rp_spmm_update_values.  Same operands, staging, streams, overlap split, statistics and completion rules as
 * crp_rp_spmm_exec_ex; plan, init and A's fp64 values are shared with the fp64 exec, and both may be called on one
 * engine.  Exchange: rows of ld32 = round_up(glb_n, 4) floats (pad columns zero) carried through the communicator's
 * alltoallv_dev_f64 as opaque 8-byte words, counts rows * ld32 / 2. */
void crp_rp_spmm_exec_f32_ex(crp_rp_spmm_p rp_spmm, int BC_layout, const float *B, long long ldB,
                             float *C, long long ldC, void *stream);
/* C := A^T * B (fp64), A being the GLOBAL matrix whose row block this rank holds.  B is this rank's A_nrow x glb_n block
 * of the operand (partitioned like A's rows), C this rank's loc_B_nrow x glb_n block of the result (partitioned by
 * B_row_displs).  Layouts, host or device operands, staging, streams and completion rules as crp_rp_spmm_exec_ex.  The
 * first call builds the transposed device matrices from the engine's two-source local matrix (nothing before it does;
 * crp_rp_spmm_transposed_built: 0, then 1): its transpose cut by rows into the part that writes C and the part that
 * writes the rows owed to peers.  One call: the peers' part, the forward exchange plan run backwards (receive counts
 * as send counts), the local part beside it when timing is off, then the incoming rows added to C row by row in a fixed
 * order (crp_scatter_add_rows_f64) -- repeated calls are bit-identical.  Products bill to the SpMM time, the exchange to
 * the redistribution time, the accumulate to the unpack time of print_stat.  crp_rp_spmm_update_values refreshes the
 * transposed matrices once they exist.  A plan-only engine aborts as in exec. */
void crp_rp_spmm_exec_t_ex(crp_rp_spmm_p rp_spmm, int BC_layout, const double *B, long long ldB,
                           double *C, long long ldC, void *stream);
/* The fp32 form: B and C in fp32, fp32 FMAs (crp_spmm_csr_f32 with the fp32 variant) on the fp32 copies of the transposed
 * matrices, which follow the value updates.  The transposed matrices, the accumulate lists, streams and events are the ones
 * crp_rp_spmm_exec_t_ex builds -- whichever dtype is called first builds them, and both may be called on one engine.  The
 * exchange is the fp32 exchange of crp_rp_spmm_exec_f32_ex run backwards: rows of ld32 = round_up(glb_n, 4) floats from the
 * fp32 receive buffer into the fp32 send buffer, the word counts swapped; the peers' part writes glb_n columns at leading
 * dimension ld32, so the pad columns zeroed at allocation stay zero.  The accumulate is crp_scatter_add_rows_f32: one fp32
 * addition per returning row, in a fixed order -- repeated calls and both timing modes are bit-identical.  Entry (c, j) of C
 * passes through at most L_c roundings (L_c: nonzeros of column c of the global A) plus one for the fp64 -> fp32 value
 * conversion, whatever the rank count and kernel variant.  Operands, layouts, staging, statistics, completion rule, plan-only
 * abort and NULL no-op as the fp64 form. */
void crp_rp_spmm_exec_t_f32_ex(crp_rp_spmm_p rp_spmm, int BC_layout, const float *B, long long ldB,
                               float *C, long long ldC, void *stream);
int crp_rp_spmm_transposed_built(crp_rp_spmm_p rp_spmm);
/* Sampled dense-dense product over this rank's rows of A (crp_sddmm_csr_f64 / _f32 in crpspmm_hip.h): for every local nonzero
 * p = (i, c) of the GLOBAL matrix, out[p] = < X[i][0:glb_n], Y[c][0:glb_n] >, times the engine's current value of p in mode 1
 * (mode 0: the plain dot).  X is this rank's A_nrow x glb_n block (partitioned like A's rows and like C of exec), Y its
 * loc_B_nrow x glb_n block (partitioned by B_row_displs, like B of exec), out one value per local nonzero IN THE ORDER OF THE
 * A_val GIVEN TO INIT -- the order crp_rp_spmm_update_values takes.  X, Y and out may each be a host or a device pointer.
 * A row-parallel SDDMM needs exactly the rows of Y that exec needs of B: one call packs Y by the forward plan's send list,
 * runs the forward exchange as exec issues it, and forms the dots with the local rows of Y as the first and the receive
 * buffer as the second source -- with timing off and a split engine the interior rows' dots on the caller's stream beside the
 * exchange, the boundary rows' after the rows have landed.  The parts of a split engine write through device copies of their
 * nonzeros' positions in A_val, uploaded by the first SDDMM call and by nothing before it (crp_rp_spmm_sddmm_built: 0, then
 * 1).  Every entry is formed in the fixed order of crp_sddmm_csr_f64, so the result is bit-identical across rank counts,
 * timing modes and repeated calls.  Layouts (1: X and Y column-major, transposed on the device first), staging, streams,
 * statistics (pack, redistribution and SpMM time; n_exec counts these calls too) and completion rules as crp_rp_spmm_exec_ex:
 * with device pointers and timing off nothing synchronises, and a later crp_rp_spmm_update_values does not overtake the
 * call.  The fp32 form exchanges rows as crp_rp_spmm_exec_f32_ex does.  A plan-only engine aborts as in exec; a NULL engine
 * is a no-op. */
void crp_rp_spmm_sddmm_ex(crp_rp_spmm_p rp_spmm, int layout, const double *X, long long ldX,
                          const double *Y, long long ldY, double *out, int mode, void *stream);
void crp_rp_spmm_sddmm_f32_ex(crp_rp_spmm_p rp_spmm, int layout, const float *X, long long ldX,
                              const float *Y, long long ldY, float *out, int mode, void *stream);
int crp_rp_spmm_sddmm_built(crp_rp_spmm_p rp_spmm);
/* Fused sparse attention over this rank's rows of A (crp_attention_csr_f64 / _f32 in crpspmm_hip.h, with nk = nv = glb_n): for
 * every local row i with nonzeros p = (i, c_p) of the GLOBAL matrix, s_p = scale * < Q[i], K[c_p] > (+ the engine's current
 * value of p when bias = 1) and O[i] = sum_p softmax_p(s) * V[c_p].  Q and O are this rank's A_nrow x glb_n blocks (partitioned
 * like A's rows), K and V its loc_B_nrow x glb_n blocks (partitioned like B); lse (A_nrow entries) and p_out (one value per
 * local nonzero IN THE ORDER OF THE A_val GIVEN TO INIT, what crp_rp_spmm_update_values_dev and the row softmax's backward take)
 * are optional (NULL: skipped).  Every pointer may be a host or a device pointer.  The engine's values are not changed: an
 * exec before and after the call gives the same bits.
 * The call needs the rows of K and of V that exec needs of B: it runs the forward exchange twice, K into the forward
 * exchange's receive buffer and then V into a second one (per dtype, rows padded as the fp32 exchange pads them), which the
 * first call of a dtype allocates and nothing before it does (crp_rp_spmm_attention_built: 0, then 1; that call blocks); the
 * send buffer is reused in stream order.  With timing off and a split engine the interior rows' kernel is enqueued on the
 * caller's stream beside both packs and exchanges, which run on the engine's second stream, and the boundary rows' kernel
 * after both have landed; with timing on the phases run in sequence.  The parts of a split engine write O and lse through their
 * row maps and p_out through the positions crp_rp_spmm_sddmm_ex uses.  A row's entries keep A_val's order inside the parts,
 * and a row's bits depend on its entries in that order only (crpspmm_hip.h), so O, lse and p_out are bit-identical across
 * rank counts, timing modes and repeated calls, and equal crp_attention_csr_* on the whole matrix.  Layout 1, staging,
 * streams, statistics (pack, redistribution and SpMM time; n_exec counts these calls too) and the completion rule as
 * crp_rp_spmm_sddmm_ex: with device pointers and timing off nothing synchronises.  glb_n = 0 computes nothing.  A plan-only
 * engine aborts as in exec, as do a layout or a bias other than 0 or 1 and a non-finite scale; a NULL engine is a no-op. */
void crp_rp_spmm_attention_ex(crp_rp_spmm_p rp_spmm, int layout, double scale, int bias, const double *Q, long long ldQ,
                              const double *K, long long ldK, const double *V, long long ldV, double *O, long long ldO,
                              double *lse, double *p_out, void *stream);
void crp_rp_spmm_attention_f32_ex(crp_rp_spmm_p rp_spmm, int layout, double scale, int bias, const float *Q, long long ldQ,
                                  const float *K, long long ldK, const float *V, long long ldV, float *O, long long ldO,
                                  float *lse, float *p_out, void *stream);
int crp_rp_spmm_attention_built(crp_rp_spmm_p rp_spmm);
/* The fused backward of crp_rp_spmm_attention_ex over this rank's rows of A (crpspmm_hip.h, crp_attention_bwd_q_csr_* and
 * crp_attention_bwd_kv_csr_*; nk = nv = glb_n): with O and lse as the forward wrote them and the upstream gradient dO,
 *   dQ[i] = scale sum_p dS_p K[c_p],   dK[c] = scale sum_p dS_p Q[i_p],   dV[c] = sum_p p_p dO[i_p],   ds_out[p] = dS_p (optional: the
 * gradient of the bias, in A_val's order) -- without the stored probabilities, the value updates and the products of the chain of
 * existing calls; A's values are not touched.  Every operand is a DEVICE pointer to row-major data (anything else aborts, like the
 * engine's other argument errors; host operands and layout 1 are not offered): Q, O, dO, dQ and lse have this rank's A_nrow rows,
 * K, V, dK and dV its rows of B (B_row_displs).  glb_n is at most 512 (fp64) / 1024 (fp32): a wider engine aborts here and keeps
 * the chain.
 * Data flow: the forward exchange of K then V, exactly as crp_rp_spmm_attention_ex does it; the row side on the engine's parts
 * (dQ, an engine-owned delta, ds_out through the positions crp_rp_spmm_sddmm_ex uses); the transposed matrices of
 * crp_rp_spmm_exec_t_ex, built by the first call that needs them -- the rows owed to peers are computed in place over the received
 * K and V rows, this rank's own go to dK and dV; then the forward plan runs backwards twice, as exec_t runs it once, each followed
 * by the accumulate into dK, then dV, through the shared send buffer in stream order.  With timing off and nproc > 1 the first
 * reverse exchange runs on the engine's second stream beside the local column kernel; with timing on everything runs in sequence
 * and bills to the pack, redistribution, SpMM and unpack time; n_exec counts these calls too.  With bias = 1 the transposed
 * matrices hold the engine's current values whichever of crp_rp_spmm_update_values / _dev came before or after they were built.
 * The first call allocates delta (crp_rp_spmm_attention_bwd_built: 0, then 1) and whatever of the forward attention's and
 * exec_t's state does not exist yet; an engine that never calls it allocates nothing.
 * dQ and ds_out are bit-identical across rank counts, timing modes and repeated calls and equal the handle call on the whole
 * matrix; dK and dV are bit-identical across repeated calls and timing modes for one rank layout, equal the handle call at one
 * rank, and agree to rounding across rank counts (a column's sum is formed per rank and the ranks' sums are added, as in exec_t).
 * A plan-only engine aborts; a NULL engine is a no-op. */
void crp_rp_spmm_attention_bwd_ex(crp_rp_spmm_p rp_spmm, double scale, int bias, const double *Q, long long ldQ,
                                  const double *K, long long ldK, const double *V, long long ldV, const double *O, long long ldO,
                                  const double *dO, long long lddO, const double *lse,
                                  double *dQ, long long lddQ, double *dK, long long lddK, double *dV, long long lddV,
                                  double *ds_out, void *stream);
void crp_rp_spmm_attention_bwd_f32_ex(crp_rp_spmm_p rp_spmm, double scale, int bias, const float *Q, long long ldQ,
                                      const float *K, long long ldK, const float *V, long long ldV, const float *O, long long ldO,
                                      const float *dO, long long lddO, const float *lse,
                                      float *dQ, long long lddQ, float *dK, long long lddK, float *dV, long long lddV,
                                      float *ds_out, void *stream);
int crp_rp_spmm_attention_bwd_built(crp_rp_spmm_p rp_spmm);
/* Multi-head forms of the four calls above (crpspmm_hip.h, "Multi-head"): `heads` >= 1 must divide glb_n, and every head has
 * dk = dv = glb_n / heads columns; any other value aborts, as the other argument errors of these calls do.  Head h of every
 * output equals the single-head computation on columns [h d, (h + 1) d) bit for bit.  lse has A_nrow x heads entries (row-major)
 * and p_out / ds_out have heads values per local nonzero: entry (p, h) at p * heads + h with p in A_val's order; the gradient of
 * A's value of p is the caller's sum over h.  The K / V exchange, the reverse exchanges, the buffers, the staging, the
 * statistics and the completion rule are those of the single-head calls, unchanged: whole rows of K and V travel, and only the
 * part kernels receive `heads`.  The engine-owned delta grows to A_nrow x heads through its owner when a call needs more (that
 * call blocks while the old array is freed).  crp_rp_spmm_attention_built and _bwd_built keep their meaning.  The backward's
 * width cap (512 fp64, 1024 fp32) applies to glb_n / heads, so an engine wider than the cap has a fused backward once it has
 * enough heads.  O, lse, p_out, dQ and ds_out equal crp_attention_mh_csr_* / crp_attention_bwd_q_mh_csr_* on the whole matrix
 * bit for bit, across rank counts, timing modes and repeated calls; dK and dV as stated for the single-head backward. */
void crp_rp_spmm_attention_mh_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double scale, int bias, const double *Q,
                                 long long ldQ, const double *K, long long ldK, const double *V, long long ldV, double *O,
                                 long long ldO, double *lse, double *p_out, void *stream);
void crp_rp_spmm_attention_mh_f32_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double scale, int bias, const float *Q,
                                     long long ldQ, const float *K, long long ldK, const float *V, long long ldV, float *O,
                                     long long ldO, float *lse, float *p_out, void *stream);
void crp_rp_spmm_attention_bwd_mh_ex(crp_rp_spmm_p rp_spmm, int heads, double scale, int bias, const double *Q, long long ldQ,
                                     const double *K, long long ldK, const double *V, long long ldV, const double *O,
                                     long long ldO, const double *dO, long long lddO, const double *lse,
                                     double *dQ, long long lddQ, double *dK, long long lddK, double *dV, long long lddV,
                                     double *ds_out, void *stream);
void crp_rp_spmm_attention_bwd_mh_f32_ex(crp_rp_spmm_p rp_spmm, int heads, double scale, int bias, const float *Q, long long ldQ,
                                         const float *K, long long ldK, const float *V, long long ldV, const float *O,
                                         long long ldO, const float *dO, long long lddO, const float *lse,
                                         float *dQ, long long lddQ, float *dK, long long lddK, float *dV, long long lddV,
                                         float *ds_out, void *stream);
/* Fused GAT attention over this rank's rows of A, forward (crpspmm_hip.h, crp_gat_attention_csr_*): for every local row i, head h
 * and nonzero p = (i, c_p) of the GLOBAL matrix, s = leaky_relu(el[i][h] + er[c_p][h], slope) (+ the engine's current value of p
 * when bias = 1) and O[i]_h = sum_p softmax_p(s) * V[c_p]_h.  `heads` >= 1 must divide glb_n (anything else aborts), and every
 * head has dv = glb_n / heads columns.  V and O are this rank's loc_B_nrow x glb_n and A_nrow x glb_n blocks, in either layout,
 * on the host or the device, handled as crp_rp_spmm_attention_mh_ex handles them; el (A_nrow x heads, ldel >= heads) and er
 * (loc_B_nrow x heads, lder >= heads) are row-major DEVICE pointers (anything else aborts); lse (A_nrow x heads) and p_out
 * (heads values per local nonzero: entry (p, h) at p * heads + h, p in A_val's order) are optional, host or device.
 * Data flow: V travels as B does, into the forward exchange's receive buffer; er travels in a narrow exchange of its own --
 * rows of `heads` elements (fp32: padded to whole 8-byte words), gathered with the forward plan's row indices into a send
 * buffer of its own and received into a per-dtype buffer, with the per-peer counts and displacements of the forward plan
 * taken by rows.  The first call of a dtype allocates both and nothing before it does (crp_rp_spmm_gat_built: 0, then 1; that
 * call blocks, as does a call with another number of heads, which sets them up again).  With timing off and a split engine
 * the interior rows' kernel is enqueued first on the caller's stream, both packs and exchanges run on the engine's second
 * stream, and the boundary rows' kernel follows after they have landed; with timing on the phases run in sequence.  The parts
 * write O and lse through their row maps and p_out through the positions crp_rp_spmm_sddmm_ex uses.  The engine's values are
 * not changed.  O, lse and p_out equal crp_gat_attention_csr_* on the whole matrix bit for bit, whatever the rank count, the
 * timing mode and the number of calls.  Statistics and the completion rule as crp_rp_spmm_attention_ex.  glb_n = 0 computes
 * nothing.  A plan-only engine aborts, as do a layout or a bias other than 0 or 1 and a non-finite slope; a NULL engine is a
 * no-op.  The engine backward is not offered yet: the handle calls crp_gat_attention_bwd_*_csr_* serve one device. */
void crp_rp_spmm_gat_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const double *el, long long ldel,
                        const double *er, long long lder, const double *V, long long ldV, double *O, long long ldO,
                        double *lse, double *p_out, void *stream);
void crp_rp_spmm_gat_f32_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const float *el, long long ldel,
                            const float *er, long long lder, const float *V, long long ldV, float *O, long long ldO,
                            float *lse, float *p_out, void *stream);
int crp_rp_spmm_gat_built(crp_rp_spmm_p rp_spmm);
/* Fused GATv2 attention over this rank's rows of A, forward (crpspmm_hip.h, crp_gatv2_attention_csr_*): for every local row i, head
 * h and nonzero p = (i, c_p) of the GLOBAL matrix, s = sum_j a_h[j] leaky_relu(XT[i]_h[j] + XS[c_p]_h[j], slope) (+ the engine's
 * current value of p when bias = 1) and O[i]_h = sum_p softmax_p(s) * XS[c_p]_h.  `heads` >= 1 must divide glb_n and every head has
 * dv = glb_n / heads columns, at most the width cap of the handle call (anything else aborts).  XS and O are this rank's
 * loc_B_nrow x glb_n and A_nrow x glb_n blocks, in either layout, on the host or the device, handled as crp_rp_spmm_gat_ex
 * handles V and O: XS travels as B does, through the forward exchange only -- the same layouts, host operands and split-engine
 * overlap -- and there is no second exchange.  XT (A_nrow x glb_n, row-major, ldXT >= glb_n) and a (glb_n elements) are DEVICE
 * pointers local to the rank (anything else aborts); lse (A_nrow x heads) and p_out (heads values per local nonzero: entry
 * (p, h) at p * heads + h, p in A_val's order) are optional, host or device.  The parts write O and lse through their row maps
 * and p_out through the positions crp_rp_spmm_sddmm_ex uses; the first call uploads those and nothing before it does
 * (crp_rp_spmm_gatv2_built: 0, then 1; that call blocks).  The engine's values are not changed.  O, lse and p_out equal
 * crp_gatv2_attention_csr_* on the whole matrix bit for bit, whatever the rank count, the timing mode and the number of calls.
 * Statistics and the completion rule as crp_rp_spmm_attention_ex.  glb_n = 0 computes nothing.  A plan-only engine aborts, as
 * do a layout or a bias other than 0 or 1 and a non-finite slope; a NULL engine is a no-op.  The engine backward is not offered
 * yet: the handle calls crp_gatv2_attention_bwd_*_csr_* serve one device. */
void crp_rp_spmm_gatv2_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const double *XT, long long ldXT,
                          const double *a, const double *XS, long long ldXS, double *O, long long ldO,
                          double *lse, double *p_out, void *stream);
void crp_rp_spmm_gatv2_f32_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const float *XT, long long ldXT,
                              const float *a, const float *XS, long long ldXS, float *O, long long ldO,
                              float *lse, float *p_out, void *stream);
int crp_rp_spmm_gatv2_built(crp_rp_spmm_p rp_spmm);
void crp_rp_spmm_print_stat(crp_rp_spmm_p rp_spmm);
void crp_rp_spmm_clear_stat(crp_rp_spmm_p rp_spmm);
/* rp_spmm_init for a caller that ALSO holds the values in device memory, in the order of A_val (A_val_dev: the panel a
 * device all-gather produced, csrc/para2d_engine.cpp): the engine's device matrices take them from there and nothing is
 * uploaded a second time.  A_val (host) is still required: the plan and the derived formats are built on the host and
 * struct rowpara_spmm::A_val is a public host field (/root/reference/src/rowpara_spmm.h:8-40).  A_val_dev may be freed
 * when the call returns.  crp_rp_spmm_values_from_device(): 1 when an engine was built that way. */
void crp_rp_spmm_init_dv(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx, const double *A_val,
                         const double *A_val_dev, const int *B_row_displs, int glb_n, crp_comm_t *comm, crp_rp_spmm_p *rp_spmm);
int crp_rp_spmm_values_from_device(crp_rp_spmm_p rp_spmm);
void crp_rp_spmm_get_plan(crp_rp_spmm_p rp_spmm, crp_rp_plan_view_t *view);
/* Host seconds spent INSIDE the B exchange call (issuing the grouped sends / receives) since the last clear_stat, summed
 * over the execs -- accumulated in every timing mode; print_stat reports it per exec when there is more than one rank. */
double crp_rp_spmm_exchange_host_seconds(crp_rp_spmm_p rp_spmm);
/* timing = 1 (default): every phase is bracketed by stream synchronisation and
 * billed to t_pack / t_a2a / t_unpack / t_spmm like the reference; 0: fully
 * asynchronous exec, only t_exec (host enqueue time) is accumulated.  With timing on every call waits for its
 * stream. */
/* Exchange / compute overlap: with more than one rank the rows of A are split at init into
 * "interior" rows (no column owned by a peer) and "boundary" rows; with timing off, exec runs the
 * B exchange on a second stream beside the interior rows' product and the boundary rows' product
 * after the rows have landed (per-row summation order unchanged).  Both counts are 0 when the
 * engine runs one product (one rank, nothing to receive, a part too small to pay for a launch,
 * or CRPSPMM_OVERLAP=0). */
void crp_rp_spmm_overlap_rows(crp_rp_spmm_p rp_spmm, int *n_interior, int *n_boundary);
void crp_rp_spmm_set_timing(crp_rp_spmm_p rp_spmm, int timing);
/* the current setting (1 after init). */
int crp_rp_spmm_timing(crp_rp_spmm_p rp_spmm);
/* kernel variant for the local SpMM (crpspmm_hip.h: crp_spmm_variant_name). */
void crp_rp_spmm_set_variant(crp_rp_spmm_p rp_spmm, int variant);
/* kernel variant of the fp32 exec (crp_spmm_csr_f32): 0 auto (default), 1 row-group, 5 team kernel.  The fp32 exec
 * never reads the fp64 variant, nor the fp64 exec this one. */
void crp_rp_spmm_set_variant_f32(crp_rp_spmm_p rp_spmm, int variant);
/* bytes of HBM the local kernel must touch per exec (SURVEY 8d bytes_alg for
 * this rank): 12*nnz + 4*(A_nrow+1) + 8*n*(distinct B rows) + 8*n*A_nrow. */
long long crp_rp_spmm_alg_bytes(crp_rp_spmm_p rp_spmm);
/* the same for the fp32 exec (4-byte values): 8*nnz + 4*(A_nrow+1) + 4*n*(distinct B rows) + 4*n*A_nrow. */
long long crp_rp_spmm_alg_bytes_f32(crp_rp_spmm_p rp_spmm);
long long crp_rp_spmm_nnz(crp_rp_spmm_p rp_spmm);
/* What the local SpMM of this engine is (for reports): the kernel variant in use (crp_spmm_variant_name; the auto
 * choice resolved for the engine's glb_n), 1 if its formats hold the rows in the locality order of
 * csrc/locality.cpp, 1 if a stride lattice was found.  Any pointer may be NULL. */
void crp_rp_spmm_kernel_info(crp_rp_spmm_p rp_spmm, int *variant, int *reordered, int *lattice);
/* New values for the same sparsity pattern, in the order of the A_val given to init (the
 * deprecated crpspmm_engine passes A's values on every exec: deprecated/src/crpspmm.h:108-117). */
void crp_rp_spmm_update_values(crp_rp_spmm_p rp_spmm, const double *A_val);
/* The same from DEVICE memory: A_val_dev holds crp_rp_spmm_nnz values in the order of the A_val given to init -- the order
 * crp_rp_spmm_sddmm_ex writes -- as fp64 (f32 = 0) or fp32 (f32 = 1; widened exactly, so the fp32 products read the caller's
 * fp32 bits and the result equals a host update with the widened values bit for bit).  Asynchronous on `stream` (taken
 * literally), with no host synchronisation: it first waits for an exec that returned asynchronously; the values are widened
 * or copied (a split engine: gathered part by part through device copies of the parts' positions in A_val, the ones the
 * first SDDMM uploads) into an engine-owned scratch buffer, so A_val_dev is free again as soon as the stream has passed
 * the call, and handed to crp_csr_dev_update_values of every device matrix; once the transposed matrices exist they are
 * gathered into their order too.  The engine's own stream is made to wait for the update (an event recorded behind it), so
 * crp_rp_spmm_exec and a later host update cannot overtake it; calls on `stream` are ordered by the stream; work on any
 * other stream is the caller's to order.  Scratch, positions and the event are allocated by the first device update and by
 * nothing before it (that call allocates and uploads, hence blocks).  The host values behind crp_rp_spmm_get_plan are left
 * behind (crp_rp_spmm_host_values_stale: 1) and refreshed by one blocking download where they are read: get_plan, the
 * first exec_t; a host crp_rp_spmm_update_values overwrites them and clears the flag.  A plan-only engine aborts as in
 * exec; a NULL engine is a no-op (stale: 0). */
void crp_rp_spmm_update_values_dev(crp_rp_spmm_p rp_spmm, const void *A_val_dev, int f32, void *stream);
int crp_rp_spmm_host_values_stale(crp_rp_spmm_p rp_spmm);
/* Row softmax over this rank's rows of A and its Jacobian product (crp_row_softmax_* in crpspmm_hip.h: definition, special
 * cases, fixed order, aliasing rule and error bounds) -- the step between crp_rp_spmm_sddmm_ex and
 * crp_rp_spmm_update_values_dev, and its backward.  s / y (y / dy / ds) are DEVICE pointers to crp_rp_spmm_nnz entries IN THE
 * ORDER OF THE A_val GIVEN TO INIT, as fp64 (f32 = 0) or fp32 (f32 = 1); the rows are the rank's A_nrow rows with init's
 * A_rowptr.  Every row of A is whole on one rank, so the call needs no communication and is not collective; a split engine
 * needs no per-part work (the order is A_val's, not the parts').  Asynchronous on `stream` (taken literally), with no host
 * synchronisation; it reads nothing of the engine's values, so it needs no ordering against exec beyond the caller's stream.
 * The first call uploads the row pointer as a device array, and nothing before it does (crp_rp_spmm_row_softmax_built: 0, then
 * 1; that one call blocks).  A rank whose rows hold no nonzero uploads its (one-entry or all-equal) row pointer like any other
 * and then returns without a launch; its pointers may be NULL.  Because the summation order is fixed per row, a rank's result is bit-identical to
 * the same rows of a one-GPU call on the whole matrix, for any rank count.  A plan-only engine aborts as
 * crp_rp_spmm_update_values_dev does; a NULL engine is a no-op (_built: 0). */
void crp_rp_spmm_row_softmax_ex(crp_rp_spmm_p e, const void *s, void *y, int f32, void *stream);
void crp_rp_spmm_row_softmax_bwd_ex(crp_rp_spmm_p e, const void *y, const void *dy, void *ds, int f32, void *stream);
int  crp_rp_spmm_row_softmax_built(crp_rp_spmm_p e);

/* See para2d_spmm_init (src/para2d_spmm.h:22-47). Rank r sits at grid position
 * (r / pn, r % pn); A_rowptr/A_colidx/A_val is the rank's A0 slice. */
void crp_para2d_spmm_init(crp_comm_t *comm, int pm, int pn, const int *A0_rowptr,
                          const int *B_rowptr, const int *AC_rowptr, const int *BC_colptr,
                          const int *A_rowptr, const int *A_colidx, const double *A_val,
                          crp_para2d_spmm_p *para2d_spmm);
void crp_para2d_spmm_free(crp_para2d_spmm_p *para2d_spmm);
void crp_para2d_spmm_exec(crp_para2d_spmm_p para2d_spmm, int BC_layout, const double *B, int ldB,
                          double *C, int ldC);
void crp_para2d_spmm_exec_ex(crp_para2d_spmm_p para2d_spmm, int BC_layout, const double *B,
                             long long ldB, double *C, long long ldC, void *stream);
/* fp32 exec of the grid column's row engine (crp_rp_spmm_exec_f32_ex). */
void crp_para2d_spmm_exec_f32_ex(crp_para2d_spmm_p para2d_spmm, int BC_layout, const float *B,
                                 long long ldB, float *C, long long ldC, void *stream);
/* ---- the rest of the family on a pm x pn grid.  A NULL engine is a no-op everywhere.  The grid-row communicator, which init
 * frees, is split again from the GLOBAL communicator (which must still be alive) by the first crp_para2d_spmm_update_values
 * or crp_para2d_spmm_sddmm_* call of an engine with pn > 1 and kept from then on: that first call is collective over the
 * WHOLE grid, every later one over the grid row.  An engine that makes neither call splits and allocates nothing. */
/* New values for the same pattern: A_val is a HOST pointer to this rank's A0 slice values in the order given to init (NULL
 * when the slice is empty).  With pn > 1 the slices are all-gathered along the grid row (allgatherv_bytes, the byte counts of
 * init) into panel order and handed to crp_rp_spmm_update_values of the grid column's row engine, which refreshes the split
 * matrices, the fp32 copies and, once built, the transposed matrices; with pn == 1 a plain forward.  Works on a plan-only
 * engine (the plan's A_val is replaced). */
void crp_para2d_spmm_update_values(crp_para2d_spmm_p e, const double *A_val);
/* C := A^T * B (fp64) of the grid column's row engine (crp_rp_spmm_exec_t_ex): B is this rank's (panel rows) x n_loc block,
 * C its (B_rowptr block of grid row pi) x n_loc block. */
void crp_para2d_spmm_exec_t_ex(crp_para2d_spmm_p e, int BC_layout, const double *B, long long ldB,
                               double *C, long long ldC, void *stream);
/* SDDMM over all n columns: for every nonzero p = (i, c) of this rank's A0 SLICE, out[p] = < X[i][0:n], Y[c][0:n] >, times the
 * engine's current value of p in mode 1.  X is this rank's (panel rows) x n_loc block (partitioned like C of exec), Y its
 * (B_rowptr block) x n_loc block (like B of exec), out crp_para2d_spmm_slice_nnz entries IN THE ORDER OF THE A_val GIVEN TO
 * INIT -- the order crp_para2d_spmm_update_values takes.  X, Y and out may each be a host or a device pointer; layout 1 as in
 * crp_rp_spmm_sddmm_ex.  One call: (1) the row engine's SDDMM (mode passed through) gives the partial dots of the whole panel
 * over this rank's n_loc columns -- with pn == 1 straight into out, and the call ends there, bit-identical to the row engine;
 * (2) a reduce-scatter along the grid row through the communicator's alltoallv_dev_f64: the panel is the concatenation of
 * the row's slices in rank order, so peer j is sent the run [off_j, off_j + nnz_j) and this rank receives pn runs of its own
 * slice, the run of grid column j at segment j (fp32 runs travel inside 8-byte words from slots of round_up(nnz_j, 2)
 * floats whose pad float is zero); (3) crp_sum_segments_* adds the runs in ascending grid column into out (a host out is
 * staged).  Exchange and sum are ordered after the row engine's call on the caller's stream; completion as
 * crp_rp_spmm_sddmm_ex (device pointers and timing off: nothing synchronises).  print_stat's lines are unchanged: exchange
 * and sum are billed to no line, n_exec rises through the row engine's call only.  The buffers are allocated by the first
 * SDDMM of a dtype (crp_para2d_spmm_sddmm_built: 0, then 1; always 0 with pn == 1).  For a given grid the result is
 * bit-identical across repeated calls and timing modes; different pn cut the n columns differently, so across grids it
 * agrees to rounding only (entrywise |out - exact| <= (max_j n_j + pn) u sum|x y|).  A plan-only engine aborts as in exec. */
void crp_para2d_spmm_sddmm_ex(crp_para2d_spmm_p e, int layout, const double *X, long long ldX,
                              const double *Y, long long ldY, double *out, int mode, void *stream);
void crp_para2d_spmm_sddmm_f32_ex(crp_para2d_spmm_p e, int layout, const float *X, long long ldX,
                                  const float *Y, long long ldY, float *out, int mode, void *stream);
int crp_para2d_spmm_sddmm_built(crp_para2d_spmm_p e);
/* fp32 C := A^T * B of the grid column's row engine (crp_rp_spmm_exec_t_f32_ex). */
void crp_para2d_spmm_exec_t_f32_ex(crp_para2d_spmm_p e, int BC_layout, const float *B, long long ldB,
                                   float *C, long long ldC, void *stream);
/* New values from DEVICE memory: this rank's A0 slice values in the order given to init, crp_para2d_spmm_slice_nnz entries of
 * fp64 (f32 = 0) or fp32 (f32 = 1) -- what crp_para2d_spmm_sddmm_* writes (NULL when the slice is empty).  With pn == 1 a
 * forward to crp_rp_spmm_update_values_dev.  With pn > 1 the slices are all-gathered along the grid-row communicator between
 * device buffers (allgatherv_dev on `stream`, init's nonzero counts times the item size as byte counts) into an engine-owned
 * panel buffer -- the panel is the concatenation of the slices in rank order -- which is handed to
 * crp_rp_spmm_update_values_dev; a communicator without allgatherv_dev is served through allgatherv_bytes on host copies
 * (a download, the gather, an upload: that path blocks).  Collective like crp_para2d_spmm_update_values: the first call
 * of the three over the whole grid.  The panel buffer is allocated by the first device update.  A plan-only engine aborts. */
void crp_para2d_spmm_update_values_dev(crp_para2d_spmm_p e, const void *A_val_dev, int f32, void *stream);
/* Row softmax over this rank's A0 SLICE and its Jacobian product (crp_rp_spmm_row_softmax_ex): crp_para2d_spmm_slice_nnz
 * entries in the order given to init, device pointers, with the slice's own row pointer (a host copy kept by init, uploaded by
 * the first call on a slice with nonzeros: crp_para2d_spmm_row_softmax_built 0, then 1; that call blocks).  The slice is a run of
 * whole rows of the panel, so with pn > 1 the call neither splits the grid-row communicator nor touches the panel, and it is
 * not collective; with pn == 1 it forwards to the row engine (_built is then the row engine's).  An empty slice takes NULL
 * pointers and returns without an upload or a launch: _built stays 0.  Bit-identical to the same rows of a one-GPU call on
 * the whole matrix, on any grid.  A plan-only engine aborts; a NULL engine is a no-op (_built: 0). */
void crp_para2d_spmm_row_softmax_ex(crp_para2d_spmm_p e, const void *s, void *y, int f32, void *stream);
void crp_para2d_spmm_row_softmax_bwd_ex(crp_para2d_spmm_p e, const void *y, const void *dy, void *ds, int f32, void *stream);
int  crp_para2d_spmm_row_softmax_built(crp_para2d_spmm_p e);
/* nonzeros of this rank's A0 slice; of every slice of its grid row (pn entries written when nnz_of_pj != NULL; returns pn). */
long long crp_para2d_spmm_slice_nnz(crp_para2d_spmm_p e);
int crp_para2d_spmm_row_slice_nnz(crp_para2d_spmm_p e, long long *nnz_of_pj);
void crp_para2d_spmm_print_stat(crp_para2d_spmm_p para2d_spmm);
void crp_para2d_spmm_clear_stat(crp_para2d_spmm_p para2d_spmm);
crp_rp_spmm_p crp_para2d_spmm_rp(crp_para2d_spmm_p para2d_spmm);
/* 1 when init replicated the panel's column indices and values between device buffers (the communicator's
 * allgatherv_dev: RCCL; CRPSPMM_REPLICATE=host forces the host path), 0 when it went through allgatherv_bytes. */
int crp_para2d_spmm_replicated_on_device(crp_para2d_spmm_p para2d_spmm);
/* How often the values of the replicated panel crossed PCIe towards the device: 0 = never (they were all-gathered between
 * device buffers and the engine's matrices were filled from that copy), 1 = once (host replication, or one grid column). */
int crp_para2d_spmm_value_uploads(crp_para2d_spmm_p para2d_spmm);
size_t crp_para2d_spmm_rA_cost(crp_para2d_spmm_p para2d_spmm);
double crp_para2d_spmm_t_ag_A(crp_para2d_spmm_p para2d_spmm);

/* ---- generic dense 2D-block redistribution (src/mat_redist.h:7-100) over a crp_comm_t --------
 * Every rank owns the rectangle (src_srow, src_scol, src_nrow, src_ncol) of a global row-major
 * matrix (owners must not overlap) and asks for (req_srow, req_scol, req_nrow, req_ncol).  init
 * gathers all rectangles, intersects them (src/mat_redist.c:9-41, 81-153) and records, in rank
 * order, which rectangles go to / come from whom; exec packs the send rectangles contiguously
 * (row-major, ld = ncol), exchanges them, and unpacks into dst.  dev_type (include/dev_type.h):
 * 0 host buffers; 1 device buffers, exchange staged through pinned host memory; 2 device buffers,
 * exchanged device to device (dt_size 8 only; otherwise staged).  Pure byte movement: bit-exact. */
typedef struct crp_mat_redist *crp_mat_redist_p;
typedef struct crp_mat_redist_view
{
    int nproc, rank, src_srow, src_scol, src_nrow, src_ncol, req_srow, req_scol, req_nrow, req_ncol;
    int n_proc_send, n_proc_recv, send_cnt, recv_cnt;      /* counts in elements                      */
    const int *send_ranks, *send_sizes, *send_displs, *sblk_sizes;   /* as src/mat_redist.h:27-30     */
    const int *recv_ranks, *recv_sizes, *recv_displs, *rblk_sizes;   /* as src/mat_redist.h:31-34     */
    size_t dt_size;
    int    dev_type;
    double hd_trans_ms;
} crp_mat_redist_view_t;
/* *engine is left untouched (NULL) on an invalid dev_type, after the reference's "[ERROR] ...
 * Invalid device type" message (src/mat_redist.c:51-55).  workbuf_bytes != NULL: the size of the
 * work buffer is returned and the caller attaches one; NULL: the engine allocates it. */
void crp_mat_redist_init(int src_srow, int src_scol, int src_nrow, int src_ncol, int req_srow, int req_scol,
                         int req_nrow, int req_ncol, crp_comm_t *comm, size_t dt_size, int dev_type,
                         crp_mat_redist_p *engine, size_t *workbuf_bytes);
void crp_mat_redist_attach_workbuf(crp_mat_redist_p engine, void *workbuf_h, void *workbuf_d);
void crp_mat_redist_exec(crp_mat_redist_p engine, const void *src_blk, int src_ld, void *dst_blk, int dst_ld);
void crp_mat_redist_free(crp_mat_redist_p *engine);
void crp_mat_redist_get_view(crp_mat_redist_p engine, crp_mat_redist_view_t *view);

/* ---- compatibility engine: the older all-in-one API (deprecated/src/crpspmm.h:89-130) ----------
 * A arrives in any 1D row distribution, B and C in arbitrary 2D blocks, all on the HOST, and A's
 * values are passed on every exec.  init plans the np_row x np_col grid with the deprecated
 * engine's own rule (per prime factor of P, largest first, split M or N by comparing
 * 1.5*nnz*n_split(*p) + k*n-style upper bounds built from per-row column RANGES,
 * deprecated/src/crpspmm.c:136-195), redistributes A's pattern to row panels, B to an even
 * (k / np_row) x (n / np_col) layout and C back to the caller's layout with crp_mat_redist, and
 * runs the 1D row-parallel device engine inside every grid column.  Same statistics lines as
 * crpspmm_engine_print_stat (deprecated/src/crpspmm.c:715-772). */
typedef struct crp_crpspmm *crp_crpspmm_p;
typedef struct crp_crpspmm_view
{
    int np_glb, rank_glb, np_row, np_col, rank_row, rank_col, glb_m, glb_n, glb_k;
    int loc_A_srow, loc_A_erow, loc_A_nrow, loc_A_nnz, loc_A_nnz_s;
    int rd_B_srow, rd_B_erow, loc_B_scol, loc_B_ecol, loc_B_ncol;
    int loc_B_srow, loc_B_erow, loc_B_nrow;   /* hull and count of the B rows the panel touches */
    int a2a_B_finegrain;                      /* value of the A2A_B_FINEGRAIN knob (reported only) */
    const int *loc_A_rowptr, *loc_A_colidx;   /* panel CSR on the host (rowptr rebased to 0) */
    const double *loc_A_val, *red_B, *loc_C;
    int n_exec;
    double t_init, t_exec, t_rd_A, t_agv_A, t_rd_B, t_a2a_B, t_spmm, t_rd_C, t_exec_nr;
    size_t nelem_A_rd, nelem_A_agv, nelem_B_rd, nelem_B_a2av, nelem_B_a2av_min;
} crp_crpspmm_view_t;
void crp_crpspmm_init(int m, int n, int k, int src_A_srow, int src_A_nrow, const int *src_A_rowptr,
                      const int *src_A_colidx, int src_B_srow, int src_B_nrow, int src_B_scol, int src_B_ncol,
                      int dst_C_srow, int dst_C_nrow, int dst_C_scol, int dst_C_ncol, crp_comm_t *comm,
                      crp_crpspmm_p *engine);
/* host planning and redistribution only (no device state): exec stops after A's values and B
 * have reached the internal layout (inspect them through the view); used by the CPU tests */
void crp_crpspmm_init_plan_only(int m, int n, int k, int src_A_srow, int src_A_nrow, const int *src_A_rowptr,
                                const int *src_A_colidx, int src_B_srow, int src_B_nrow, int src_B_scol,
                                int src_B_ncol, int dst_C_srow, int dst_C_nrow, int dst_C_scol, int dst_C_ncol,
                                crp_comm_t *comm, crp_crpspmm_p *engine);
void crp_crpspmm_exec(crp_crpspmm_p engine, const int *src_A_rowptr, const int *src_A_colidx,
                      const double *src_A_val, const double *src_B, int ldB, double *dst_C, int ldC);
void crp_crpspmm_free(crp_crpspmm_p *engine);
void crp_crpspmm_print_stat(crp_crpspmm_p engine);
void crp_crpspmm_clear_stat(crp_crpspmm_p engine);
void crp_crpspmm_get_view(crp_crpspmm_p engine, crp_crpspmm_view_t *view);
/* the deprecated engine's grid rule alone (host, no communication): A_rowptr_glb has m + 1
 * entries, cidx_se holds (first, last) column of every row (2*m ints; an empty row holds any
 * pair with first > last and is ignored).  m_split_idx receives np_row + 1 row offsets
 * (room for P + 1). */
void crp_crpspmm_plan_grid(int P, int m, int n, int k, const int *A_rowptr_glb, const int *cidx_se,
                           int *np_row, int *np_col, int *m_split_idx);

/* ---- planner extension: grid for an A that is reused rA times ------------------------------------
 * Same arguments and output arrays as calc_spmm_part2d_from_1d (spmat_part.h; src/spmat_part.h:55-76)
 * without dbg_print.  Prices EVERY pm x pn with pn | nproc as floor(1.5 nnz (pn-1)) [replicate A once]
 * + rA * n * (B rows exchanged per multiply) and returns the cheapest; the reference rule leaves rA
 * out of its 1D starting cost and searches greedily, so there rA > 1 favours 1D.  Host only. */
void crp_spmm_part2d_amortized(int nproc, int m, int n, int k, const int *rb_displs0, const int *rowptr,
                               const int *colidx, int rA, int *pm, int *pn, size_t *comm_cost, int **A0_rowptr,
                               int **B_rowptr, int **AC_rowptr, int **BC_colptr);

/* Extension: grid choice by a TIME model of one node of point-to-point links instead of a byte
 * count -- one-time replication of the A panels (fan-out: the pn - 1 pieces arrive over different links), per multiply
 * max(local product at the kernels' measured roofline fraction for n / pn columns, slowest PAIR of the B exchange), priced
 * as t_rep / rA + t_exec; grids that do not fit a GPU's HBM are skipped.  mm = NULL or {link GB/s one way (64), HBM GB/s
 * (8000), HBM bytes per GPU (288e9)}; times (optional) = {t_rep, t_exch, t_comp} of the winner, seconds.  Output arrays as
 * calc_spmm_part2d_from_1d.  Host only. */
void crp_spmm_part2d_timed(int nproc, int m, int n, int k, const int *rb_displs0, const int *rowptr, const int *colidx,
                           int rA, const double *mm, int *pm, int *pn, double *times, int **A0_rowptr, int **B_rowptr,
                           int **AC_rowptr, int **BC_colptr);

/* ---- binary CSR cache (ingest extension) ---------------------------------------------------------
 * A converted matrix kept beside its .mtx so that later runs skip the text parse
 * (examples/mmio_utils.c:11-190 takes 3 s for pwtk, minutes for nlpkkt240).  One little-endian file:
 * "CRPCSR01", int64 nrow / ncol / nnz, rowptr, colidx, val.  Return 0, or -1 (unreadable, wrong
 * magic, inconsistent sizes); read hands back malloc'd arrays (caller frees). */
int crp_csr_cache_write(const char *fname, int nrow, int ncol, const int *rowptr, const int *colidx,
                        const double *val);
int crp_csr_cache_read(const char *fname, int *nrow, int *ncol, int **rowptr, int **colidx, double **val);

/* ---- host-only pieces exposed for tests (no GPU needed) -------------------
 * Build only the exchange plan (everything rp_spmm_init computes on the host,
 * including the alltoall of needed row ids) without touching the device.
 * Release with crp_rp_spmm_free. exec on such an engine aborts. */
void crp_rp_spmm_init_plan_only(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx,
                                const double *A_val, const int *B_row_displs, int glb_n,
                                crp_comm_t *comm, crp_rp_spmm_p *rp_spmm);
void crp_para2d_spmm_init_plan_only(crp_comm_t *comm, int pm, int pn, const int *A0_rowptr,
                                    const int *B_rowptr, const int *AC_rowptr, const int *BC_colptr,
                                    const int *A_rowptr, const int *A_colidx, const double *A_val,
                                    crp_para2d_spmm_p *para2d_spmm);
/* The device-side (two-source) column index the kernel consumes, host copy:
 * c >= 0 local B row, c < 0 -> ~c = row of the receive buffer. */
const int *crp_rp_spmm_dev_colidx_host(crp_rp_spmm_p rp_spmm);

#ifdef __cplusplus
}
#endif
#endif
