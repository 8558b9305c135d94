// dtype_calls.h -- the fp64 / fp32 pairs of the device ABI and of the row engine under one overloaded name each, for the engines'
// templates over the dtype, and the row softmax both engines run over a row pointer they keep on the device.  Forwarders only:
// what closes over engine state (the row engine's spmm reads its variant) stays with the engine.
#ifndef CRP_DTYPE_CALLS_H
#define CRP_DTYPE_CALLS_H

#include <vector>
#include "crp_engine.h"
#include "dev_owned.h"

namespace crp
{

static inline int transpose(int nrow, int ncol, const double *src, long long lds, double *dst, long long ldd, void *s)
{
    return crp_transpose_f64(nrow, ncol, src, lds, dst, ldd, s);
}
static inline int transpose(int nrow, int ncol, const float *src, long long lds, float *dst, long long ldd, void *s)
{
    return crp_transpose_f32(nrow, ncol, src, lds, dst, ldd, s);
}
static inline int gather(int nidx, int n, const int *ridx, const double *src, long long lds, double *dst, long long ldd, void *s)
{
    return crp_gather_rows_f64(0, nidx, n, ridx, src, lds, dst, ldd, s);
}
static inline int gather(int nidx, int n, const int *ridx, const float *src, long long lds, float *dst, long long ldd, void *s)
{
    return crp_gather_rows_f32(0, nidx, n, ridx, src, lds, dst, ldd, s);
}
static inline int scatter_add(int nseg, int n, const int *row, const int *ptr, const int *pos, const double *src, long long lds, double *dst,
                              long long ldd, void *s)
{
    return crp_scatter_add_rows_f64(nseg, n, row, ptr, pos, src, lds, dst, ldd, s);
}
static inline int scatter_add(int nseg, int n, const int *row, const int *ptr, const int *pos, const float *src, long long lds, float *dst,
                              long long ldd, void *s)
{
    return crp_scatter_add_rows_f32(nseg, n, row, ptr, pos, src, lds, dst, ldd, s);
}
static inline int sddmm(crp_csr_dev_p A, int n, const double *X, long long ldX, const double *Y0, long long ldY0, const double *Y1,
                        long long ldY1, double *out, const int *out_pos, int mode, void *s)
{
    return crp_sddmm_csr_f64(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, out_pos, mode, s);
}
static inline int sddmm(crp_csr_dev_p A, int n, const float *X, long long ldX, const float *Y0, long long ldY0, const float *Y1,
                        long long ldY1, float *out, const int *out_pos, int mode, void *s)
{
    return crp_sddmm_csr_f32(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, out_pos, mode, s);
}
// the fused attention and its backward: heads == 0 is the single-head entry point (d: all the columns), heads >= 1 the multi-head
// one with its heads of d columns each -- the one place that chooses between them
static inline int attention(crp_csr_dev_p A, int heads, int d, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                            long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1,
                            long long ldV1, double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *s)
{
    if (heads >= 1)
        return crp_attention_mh_csr_f64(A, heads, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
    return crp_attention_csr_f64(A, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
}
static inline int attention(crp_csr_dev_p A, int heads, int d, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                            long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1,
                            long long ldV1, float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *s)
{
    if (heads >= 1)
        return crp_attention_mh_csr_f32(A, heads, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
    return crp_attention_csr_f32(A, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
}
static inline int attention_bwd_q(crp_csr_dev_p A, int heads, int d, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                                  long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1,
                                  long long ldV1, const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                  double *dQ, long long lddQ, double *delta, double *ds_out, const int *out_pos, void *s)
{
    if (heads >= 1)
        return crp_attention_bwd_q_mh_csr_f64(A, heads, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse,
                                              dQ, lddQ, delta, ds_out, out_pos, s);
    return crp_attention_bwd_q_csr_f64(A, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                       delta, ds_out, out_pos, s);
}
static inline int attention_bwd_q(crp_csr_dev_p A, int heads, int d, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                                  long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1,
                                  long long ldV1, const float *O, long long ldO, const float *dO, long long lddO, const float *lse, float *dQ,
                                  long long lddQ, float *delta, float *ds_out, const int *out_pos, void *s)
{
    if (heads >= 1)
        return crp_attention_bwd_q_mh_csr_f32(A, heads, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse,
                                              dQ, lddQ, delta, ds_out, out_pos, s);
    return crp_attention_bwd_q_csr_f32(A, d, d, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                       delta, ds_out, out_pos, s);
}
static inline int attention_bwd_kv(crp_csr_dev_p At, int heads, int d, double scale, int bias, const double *K, long long ldK, const double *V,
                                   long long ldV, const double *Q, long long ldQ, const double *dO, long long lddO, const double *lse,
                                   const double *delta, double *dK, long long lddK, double *dV, long long lddV, void *s)
{
    if (heads >= 1)
        return crp_attention_bwd_kv_mh_csr_f64(At, heads, d, d, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
    return crp_attention_bwd_kv_csr_f64(At, d, d, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
}
static inline int attention_bwd_kv(crp_csr_dev_p At, int heads, int d, double scale, int bias, const float *K, long long ldK, const float *V,
                                   long long ldV, const float *Q, long long ldQ, const float *dO, long long lddO, const float *lse,
                                   const float *delta, float *dK, long long lddK, float *dV, long long lddV, void *s)
{
    if (heads >= 1)
        return crp_attention_bwd_kv_mh_csr_f32(At, heads, d, d, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
    return crp_attention_bwd_kv_csr_f32(At, d, d, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
}
// the fused GAT attention (additive LeakyReLU scores), forward
static inline int gat_attention(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const double *el, long long ldel, const double *er0,
                                long long lder0, const double *er1, long long lder1, const double *V0, long long ldV0, const double *V1,
                                long long ldV1, double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *s)
{
    return crp_gat_attention_csr_f64(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
}
static inline int gat_attention(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const float *el, long long ldel, const float *er0,
                                long long lder0, const float *er1, long long lder1, const float *V0, long long ldV0, const float *V1,
                                long long ldV1, float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *s)
{
    return crp_gat_attention_csr_f32(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos, s);
}
// the fused GATv2 attention (a LeakyReLU inside the dot with a), forward
static inline int gatv2_attention(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const double *XT, long long ldXT, const double *XS0,
                                  long long ldXS0, const double *XS1, long long ldXS1, const double *a, double *O, long long ldO, double *lse,
                                  double *p_out, const int *out_pos, void *s)
{
    return crp_gatv2_attention_csr_f64(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, lse, p_out, out_pos, s);
}
static inline int gatv2_attention(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const float *XT, long long ldXT, const float *XS0,
                                  long long ldXS0, const float *XS1, long long ldXS1, const float *a, float *O, long long ldO, float *lse,
                                  float *p_out, const int *out_pos, void *s)
{
    return crp_gatv2_attention_csr_f32(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, lse, p_out, out_pos, s);
}
static inline int sum_segments(int nseg, long long len, const double *src, long long stride, double *out, void *s)
{
    return crp_sum_segments_f64(nseg, len, src, stride, out, s);
}
static inline int sum_segments(int nseg, long long len, const float *src, long long stride, float *out, void *s)
{
    return crp_sum_segments_f32(nseg, len, src, stride, out, s);
}
static inline void inner_sddmm(crp_rp_spmm_p rp, int layout, const double *X, long long ldX, const double *Y, long long ldY, double *out,
                               int mode, void *s)
{
    crp_rp_spmm_sddmm_ex(rp, layout, X, ldX, Y, ldY, out, mode, s);
}
static inline void inner_sddmm(crp_rp_spmm_p rp, int layout, const float *X, long long ldX, const float *Y, long long ldY, float *out,
                               int mode, void *s)
{
    crp_rp_spmm_sddmm_f32_ex(rp, layout, X, ldX, Y, ldY, out, mode, s);
}

// ---- row softmax over the rows of a row pointer (crp_row_softmax_*) ----------------------------------------------------------------
// What an engine's entry point checks first; with `upload`, the first call puts the row pointer on the device through `stream`
// and waits for it.  (The array holds at least one entry, so "rowptr_dev is set" is "built".)
static inline void row_softmax_ready(const char *what, bool plan_only, int f32, bool upload, DevArray<int> &rowptr_dev,
                                     const std::vector<int> &rowptr, void *stream)
{
    ASSERT_PRINTF(!plan_only, "%s on a plan-only engine (no device state)\n", what);
    ASSERT_PRINTF(f32 == 0 || f32 == 1, "%s: f32 must be 0 or 1\n", what);
    if (upload && rowptr_dev == nullptr) rowptr_dev.upload(rowptr.data(), rowptr.size(), stream);
}
static inline void row_softmax(int nrow, const int *rowptr_dev, int f32, const void *s, void *y, void *stream)
{
    if (f32) HIP_OK(crp_row_softmax_f32(nrow, rowptr_dev, (const float *) s, (float *) y, stream));
    else HIP_OK(crp_row_softmax_f64(nrow, rowptr_dev, (const double *) s, (double *) y, stream));
}
static inline void row_softmax_bwd(int nrow, const int *rowptr_dev, int f32, const void *y, const void *dy, void *ds, void *stream)
{
    if (f32) HIP_OK(crp_row_softmax_bwd_f32(nrow, rowptr_dev, (const float *) y, (const float *) dy, (float *) ds, stream));
    else HIP_OK(crp_row_softmax_bwd_f64(nrow, rowptr_dev, (const double *) y, (const double *) dy, (double *) ds, stream));
}

}  // namespace crp

#endif
