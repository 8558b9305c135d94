// rp_attention_bwd.cpp -- the row engine's fused attention backward (crp_rp_spmm_attention_bwd_ex / _f32_ex, include/crp_engine.h):
// the one translation unit of the engines that names the single-head device entry points of attention_bwd_kernels.hip (the
// multi-head calls, rp_attention_mh.cpp, run attention_bwd_impl below with their own device calls).
//
// Data flow, every piece of which the engine has: the forward exchange of K then V, as the forward attention does it
// (pack_exchange_run2: K's rows land in the forward receive buffer, V's in the attention's second one); bwd_q on the parts, through
// their row maps and their positions in A_val; the transposed matrices of exec_t (build_transposed) -- bwd_kv on At_rem reads K[c],
// V[c] from the two receive buffers and writes dK, dV IN PLACE over them (crpspmm_hip.h: dK == K, dV == V is legal), bwd_kv on
// At_loc writes this rank's dK, dV; then the forward plan run backwards twice, as exec_t does once, each followed by the
// accumulate into dK, then dV, through the shared send buffer in stream order.
#include "rp_engine_impl.h"

namespace crp
{
static inline int attention_bwd_q(crp_csr_dev_p A, int n, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                                  long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1,
                                  long long ldV1, const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                                  double *dQ, long long lddQ, double *delta, double *ds_out, const int *out_pos, void *s)
{
    return crp_attention_bwd_q_csr_f64(A, n, n, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                       delta, ds_out, out_pos, s);
}
static inline int attention_bwd_q(crp_csr_dev_p A, int n, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                                  long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1,
                                  long long ldV1, const float *O, long long ldO, const float *dO, long long lddO, const float *lse, float *dQ,
                                  long long lddQ, float *delta, float *ds_out, const int *out_pos, void *s)
{
    return crp_attention_bwd_q_csr_f32(A, n, n, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                       delta, ds_out, out_pos, s);
}
static inline int attention_bwd_kv(crp_csr_dev_p At, int n, double scale, int bias, const double *K, long long ldK, const double *V,
                                   long long ldV, const double *Q, long long ldQ, const double *dO, long long lddO, const double *lse,
                                   const double *delta, double *dK, long long lddK, double *dV, long long lddV, void *s)
{
    return crp_attention_bwd_kv_csr_f64(At, n, n, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
}
static inline int attention_bwd_kv(crp_csr_dev_p At, int n, double scale, int bias, const float *K, long long ldK, const float *V,
                                   long long ldV, const float *Q, long long ldQ, const float *dO, long long lddO, const float *lse,
                                   const float *delta, float *dK, long long lddK, float *dV, long long lddV, void *s)
{
    return crp_attention_bwd_kv_csr_f32(At, n, n, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV, s);
}
}  // namespace crp

// delta, one entry per row and head: allocated by the first call of a dtype for one head, grown through its owner by a call that
// needs more (the free waits for the device, so no earlier call still reads the old array)
template <class T> static T *delta_grow(crp::DevArray<T> &a, size_t *cap, size_t need)
{
    if (a != nullptr && *cap >= need) return a.get();
    *cap = need;
    return a.alloc(need);
}
static double *delta_of(crp_rp_spmm *e, const double *, size_t nh) { return delta_grow(e->bw_delta_dev, &e->bw_delta_cap, (size_t) e->A_nrow * nh + 1); }
static float *delta_of(crp_rp_spmm *e, const float *, size_t nh) { return delta_grow(e->bw_delta32_dev, &e->bw_delta32_cap, (size_t) e->A_nrow * nh + 1); }

template <class T>
static void attention_bwd_impl(crp_rp_spmm *e, double scale, int bias, const T *Q, long long ldQ, const T *K, long long ldK, const T *V,
                               long long ldV, const T *O, long long ldO, const T *dO, long long lddO, const T *lse, T *dQ, long long lddQ,
                               T *dK, long long lddK, T *dV, long long lddV, T *ds_out, void *stream_, int heads = 0,
                               crp::attn_bwd_q_mh_fn<T> q_mh = nullptr, crp::attn_bwd_kv_mh_fn<T> kv_mh = nullptr)
{
    // q_mh == nullptr: the single-head calls.  Else (the _mh_ calls, rp_attention_mh.cpp) the multi-head device calls and their
    // heads of glb_n / heads columns each, to which the cap applies; only the part kernels and delta's size know
    if (e == NULL) return;
    const bool mh = q_mh != nullptr;
    ASSERT_PRINTF(!mh || (heads >= 1 && e->glb_n % heads == 0), "rp_spmm_attention_bwd_mh: heads (%d) must be positive and divide the %d columns\n",
                  heads, e->glb_n);
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_attention_bwd on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(bias == 0 || bias == 1, "bias must be 0 or 1\n");
    ASSERT_PRINTF(scale - scale == 0.0, "scale must be finite\n");
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const int d = mh ? n / heads : n;                   // one head's width
    ASSERT_PRINTF(d <= 64 * 64 / (int) sizeof(T), "rp_spmm_attention_bwd: %d columns pass the fused backward's cap (%d)\n", d,
                  64 * 64 / (int) sizeof(T));
    // device-resident row-major operands only
    const struct { const void *p; long long ld; int rows; const char *name; } ops[] = {
        {Q, ldQ, m, "Q"}, {O, ldO, m, "O"}, {dO, lddO, m, "dO"}, {dQ, lddQ, m, "dQ"}, {K, ldK, kb, "K"}, {V, ldV, kb, "V"}, {dK, lddK, kb, "dK"},
        {dV, lddV, kb, "dV"}};
    for (const auto &op : ops)
    {
        if (op.rows == 0 || n == 0) continue;
        ASSERT_PRINTF(op.p != NULL && on_device(op.p), "rp_spmm_attention_bwd: %s must be a device pointer\n", op.name);
        ASSERT_PRINTF(op.ld >= n, "rp_spmm_attention_bwd: the leading dimension of %s is below %d\n", op.name, n);
    }
    ASSERT_PRINTF(m == 0 || (lse != NULL && on_device(lse)), "rp_spmm_attention_bwd: lse must be a device pointer\n");
    ASSERT_PRINTF(ds_out == NULL || e->A_val.empty() || on_device(ds_out), "rp_spmm_attention_bwd: ds_out must be a device pointer\n");
    const double t_begin = get_wtime_sec();
    if (!e->t_built) build_transposed(e);
    void *s = stream_;
    const bool timing = e->timing != 0;
    double t0;

    const Xchg x = exchange_of(e, K);
    T *recv2 = attention_recv(e, x, K);
    T *delta = delta_of(e, K, mh ? (size_t) heads : 1);
    e->bw_built = true;
    if (n == 0)
    {
        e->n_exec++;
        return;
    }

    // ---- K then V travel as in the forward; the row side on the parts
    pack_exchange_run2(e, x, recv2, K, ldK, V, ldV, s, t0, [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        const int *pos = part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
        if (mh)
            HIP_OK(q_mh(A, heads, d, d, scale, bias, Q, ldQ, K, ldK, (const T *) x.recv, x.ld, V, ldV, (const T *) recv2, x.ld, O, ldO, dO, lddO,
                        lse, dQ, lddQ, delta, ds_out, pos, s));
        else
            HIP_OK(crp::attention_bwd_q(A, n, scale, bias, Q, ldQ, K, ldK, (const T *) x.recv, x.ld, V, ldV, (const T *) recv2, x.ld, O, ldO, dO,
                                        lddO, lse, dQ, lddQ, delta, ds_out, pos, s));
    });
    lap(e, s, t0, &e->t_spmm);

    // ---- the column side: the rows owed to peers in place over the received K and V rows, this rank's own directly
    auto kv = [&](crp_csr_dev_p At, const T *Kr, long long ldKr, const T *Vr, long long ldVr, T *dKr, long long lddKr, T *dVr, long long lddVr) {
        if (mh) HIP_OK(kv_mh(At, heads, d, d, scale, bias, Kr, ldKr, Vr, ldVr, Q, ldQ, dO, lddO, lse, delta, dKr, lddKr, dVr, lddVr, s));
        else HIP_OK(crp::attention_bwd_kv(At, n, scale, bias, Kr, ldKr, Vr, ldVr, Q, ldQ, dO, lddO, lse, delta, dKr, lddKr, dVr, lddVr, s));
    };
    auto reverse_exchange = [&](const void *from, void *xs) {
        const double tx0 = get_wtime_sec();
        e->comm->alltoallv_dev_f64(e->comm->ctx, (const double *) from, x.rc, x.rd, (double *) x.send, x.sc, x.sd, xs);
        e->t_a2a_host += get_wtime_sec() - tx0;
    };
    auto accumulate = [&](T *dst, long long ldd) {
        if (e->n_acc == 0) return;
        const int *acc_row = e->acc_dev, *acc_ptr = acc_row + e->n_acc, *acc_pos = acc_ptr + e->n_acc + 1;
        HIP_OK(crp::scatter_add(e->n_acc, n, acc_row, acc_ptr, acc_pos, (const T *) x.send, x.ld, dst, ldd, s));
    };
    if (e->At_rem != nullptr) kv(e->At_rem, (const T *) x.recv, x.ld, recv2, x.ld, (T *) x.recv, x.ld, recv2, x.ld);
    if (e->nproc > 1 && !timing)
    {
        // the first reverse exchange on its own stream beside the local kernel, which is enqueued first (see exec_t); the second
        // reuses the send buffer, so it waits on s for the first accumulate
        HIP_OK(crp_event_record(e->ev_packed, s));
        if (kb > 0) kv(e->At_loc, K, ldK, V, ldV, dK, lddK, dV, lddV);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        reverse_exchange(x.recv, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        accumulate(dK, lddK);
        reverse_exchange(recv2, s);
        accumulate(dV, lddV);
    }
    else
    {
        lap(e, s, t0, &e->t_spmm);
        if (kb > 0) kv(e->At_loc, K, ldK, V, ldV, dK, lddK, dV, lddV);
        lap(e, s, t0, &e->t_spmm);
        for (int op = 0; op < 2; op++)
        {
            if (e->nproc > 1) reverse_exchange(op == 0 ? x.recv : (void *) recv2, s);
            lap(e, s, t0, &e->t_a2a);
            accumulate(op == 0 ? dK : dV, op == 0 ? lddK : lddV);
            lap(e, s, t0, &e->t_unpack);
        }
    }
    complete(e, s, false, timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

void rp_attention_bwd_mh(crp_rp_spmm *e, int heads, double scale, int bias, const double *Q, long long ldQ, const double *K, long long ldK,
                         const double *V, long long ldV, const double *O, long long ldO, const double *dO, long long lddO, const double *lse,
                         double *dQ, long long lddQ, double *dK, long long lddK, double *dV, long long lddV, double *ds_out, void *stream,
                         crp::attn_bwd_q_mh_fn<double> q_call, crp::attn_bwd_kv_mh_fn<double> kv_call)
{
    attention_bwd_impl<double>(e, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream, heads,
                               q_call, kv_call);
}
void rp_attention_bwd_mh(crp_rp_spmm *e, int heads, double scale, int bias, const float *Q, long long ldQ, const float *K, long long ldK,
                         const float *V, long long ldV, const float *O, long long ldO, const float *dO, long long lddO, const float *lse,
                         float *dQ, long long lddQ, float *dK, long long lddK, float *dV, long long lddV, float *ds_out, void *stream,
                         crp::attn_bwd_q_mh_fn<float> q_call, crp::attn_bwd_kv_mh_fn<float> kv_call)
{
    attention_bwd_impl<float>(e, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream, heads,
                              q_call, kv_call);
}

extern "C" {

void crp_rp_spmm_attention_bwd_ex(crp_rp_spmm_p e, double scale, int bias, const double *Q, long long ldQ, const double *K, long long ldK,
                                  const double *V, long long ldV, const double *O, long long ldO, const double *dO, long long lddO,
                                  const double *lse, double *dQ, long long lddQ, double *dK, long long lddK, double *dV, long long lddV,
                                  double *ds_out, void *stream)
{
    attention_bwd_impl<double>(e, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

void crp_rp_spmm_attention_bwd_f32_ex(crp_rp_spmm_p e, double scale, int bias, const float *Q, long long ldQ, const float *K, long long ldK,
                                      const float *V, long long ldV, const float *O, long long ldO, const float *dO, long long lddO,
                                      const float *lse, float *dQ, long long lddQ, float *dK, long long lddK, float *dV, long long lddV,
                                      float *ds_out, void *stream)
{
    attention_bwd_impl<float>(e, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

int crp_rp_spmm_attention_bwd_built(crp_rp_spmm_p e) { return (e && e->bw_built) ? 1 : 0; }

}  // extern "C"
