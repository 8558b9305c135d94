// rp_attention_mh.cpp -- the row engine's multi-head attention calls (crp_rp_spmm_attention_mh_ex / _f32_ex and
// crp_rp_spmm_attention_bwd_mh_ex / _f32_ex, include/crp_engine.h): the one translation unit of the engines that names the
// multi-head device entry points of attention_kernels.hip and attention_bwd_kernels.hip.  The calls are the single-head ones'
// implementations (rp_engine.cpp, rp_attention_bwd.cpp) -- the same exchanges, buffers, staging, statistics and completion rule --
// with `heads` handed to the part kernels; `heads` must be positive and divide glb_n.
#include "rp_engine_impl.h"

extern "C" {

void crp_rp_spmm_attention_mh_ex(crp_rp_spmm_p e, int layout, int heads, double scale, int bias, const double *Q, long long ldQ,
                                 const double *K, long long ldK, const double *V, long long ldV, double *O, long long ldO, double *lse,
                                 double *p_out, void *stream)
{
    rp_attention_mh(e, layout, heads, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream, crp_attention_mh_csr_f64);
}

void crp_rp_spmm_attention_mh_f32_ex(crp_rp_spmm_p e, int layout, int heads, double scale, int bias, const float *Q, long long ldQ,
                                     const float *K, long long ldK, const float *V, long long ldV, float *O, long long ldO, float *lse,
                                     float *p_out, void *stream)
{
    rp_attention_mh(e, layout, heads, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream, crp_attention_mh_csr_f32);
}

void crp_rp_spmm_attention_bwd_mh_ex(crp_rp_spmm_p e, int heads, double scale, int bias, const double *Q, long long ldQ, const double *K,
                                     long long ldK, const double *V, long long ldV, const double *O, long long ldO, const double *dO,
                                     long long lddO, const double *lse, double *dQ, long long lddQ, double *dK, long long lddK, double *dV,
                                     long long lddV, double *ds_out, void *stream)
{
    rp_attention_bwd_mh(e, heads, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream,
                        crp_attention_bwd_q_mh_csr_f64, crp_attention_bwd_kv_mh_csr_f64);
}

void crp_rp_spmm_attention_bwd_mh_f32_ex(crp_rp_spmm_p e, int heads, double scale, int bias, const float *Q, long long ldQ, const float *K,
                                         long long ldK, const float *V, long long ldV, const float *O, long long ldO, const float *dO,
                                         long long lddO, const float *lse, float *dQ, long long lddQ, float *dK, long long lddK, float *dV,
                                         long long lddV, float *ds_out, void *stream)
{
    rp_attention_bwd_mh(e, heads, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream,
                        crp_attention_bwd_q_mh_csr_f32, crp_attention_bwd_kv_mh_csr_f32);
}

}  // extern "C"
