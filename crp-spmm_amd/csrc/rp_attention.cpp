// rp_attention.cpp -- the row engine's fused sparse attention, forward and backward, single- and multi-head
// (crp_rp_spmm_attention{,_mh}{,_f32}_ex and crp_rp_spmm_attention_bwd{,_mh}{,_f32}_ex, include/crp_engine.h).  One implementation per
// direction, templated over the dtype, with `heads` as data: 0 is the single-head call (d = glb_n columns, one lse / delta entry per
// row, one p_out / ds_out entry per nonzero), heads >= 1 the multi-head call (d = glb_n / heads columns per head, heads entries per
// row and per nonzero).  Only the part kernels and those sizes know; the exchange moves whole rows of K and V either way.  Which
// device entry point that is, is dtype_calls.h's business (crp::attention, crp::attention_bwd_q, crp::attention_bwd_kv).
//
//
// Both directions hand two travellers to the schedule of rp_engine_impl.h (pack_exchange_run, packed on the exchange stream): K, whose
// rows land in the forward receive buffer, then V, whose rows land in the attention's second one, both through the forward send
// buffer, which is reused in stream order.
//
// Data flow of the backward, every piece of which the engine has: that exchange of K then V; bwd_q on the parts, through
// their row maps and their positions in A_val; the transposed matrices of exec_t (build_transposed) -- bwd_kv on At_rem reads K[c],
// V[c] from the two receive buffers and writes dK, dV IN PLACE over them (crpspmm_hip.h: dK == K, dV == V is legal), bwd_kv on
// At_loc writes this rank's dK, dV; then the forward plan run backwards twice, as exec_t does once (reverse_exchange_rows), each
// followed by the accumulate into dK, then dV (accumulate_rows), through the shared send buffer in stream order.
#include "rp_engine_impl.h"

// heads of a multi-head call as the implementations take it: positive and a divisor of glb_n (0, theirs for the single-head calls,
// is refused with the rest)
static int mh_heads(const crp_rp_spmm *e, int heads, const char *what)
{
    ASSERT_PRINTF(e == NULL || (heads >= 1 && e->glb_n % heads == 0), "%s: heads (%d) must be positive and divide the %d columns\n", what, heads,
                  e->glb_n);
    return heads;
}

// ---- what the forward and the backward share: the second receive buffer ------------------------------------------------------------------
// first attention call of a dtype: the second receive buffer (rows of x.ld elements, zeroed once: the fp32 rows' pad columns are
// never written again), and the parts' positions in A_val; blocks
template <class T>
static T *attention_recv(crp_rp_spmm *e, const Xchg &x, crp::DevArray<T> &buf, bool *ready)
{
    if (!*ready)
    {
        upload_part_positions(e);
        if (e->n_recv_rows > 0 && x.ld > 0) buf.zeroed((size_t) e->n_recv_rows * (size_t) x.ld);
        *ready = true;
        e->at_built = true;
    }
    return buf;
}
static double *attention_recv(crp_rp_spmm *e, const Xchg &x, const double *) { return attention_recv(e, x, e->at_recv_dev, &e->at_ready64); }
static float *attention_recv(crp_rp_spmm *e, const Xchg &x, const float *) { return attention_recv(e, x, e->at_recv32_dev, &e->at_ready32); }

// ---- O = softmax_row(scale (Q K^T)|pattern(A) (+ A's values)) V over this rank's rows of A -------------------------------------------
template <class T>
static void attention_impl(crp_rp_spmm *e, int layout, int heads, double scale, int bias, const T *Q, long long ldQ, const T *K, long long ldK,
                           const T *V, long long ldV, T *O, long long ldO, T *lse, T *p_out, void *stream_)
{
    if (e == NULL) return;
    const size_t nh = heads >= 1 ? (size_t) heads : 1;
    check_call(e, "rp_spmm_attention", "layout", layout);
    check_scores(bias, scale, "scale");
    const double t_begin = get_wtime_sec();
    void *s = stream_;
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const int d = n / (int) nh;                         // one head's width
    const size_t nnz = e->A_val.size();
    const bool timing = e->timing != 0;
    double t0;

    const bool Q_on_dev = on_device(Q), K_on_dev = on_device(K), V_on_dev = on_device(V), O_on_dev = on_device(O);

    // ---- operands as device-resident row-major views: K takes B's buffers and the forward exchange, O takes C's
    const Xchg x = exchange_of(e, K);
    T *recv2 = attention_recv(e, x, K);
    const crp::InView<T> Kv = crp::operand_in(layout, K, ldK, kb, n, K_on_dev, e->B_stage, e->B_rm, s);
    const crp::InView<T> Vv = crp::operand_in(layout, V, ldV, kb, n, V_on_dev, e->V_stage, e->V_rm, s);
    const crp::InView<T> Qv = crp::operand_in(layout, Q, ldQ, m, n, Q_on_dev, e->Q_stage, e->Q_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    const HostVec<T> lsev = host_vec(lse, lse != NULL ? (size_t) m * nh : 0, e->at_lse);
    const HostVec<T> pv = host_vec(p_out, p_out != NULL ? nnz * nh : 0, e->sd_out);

    // ---- pack and exchange K, then V; the kernels: the parts of a split engine write O and lse through their row maps and p_out
    // through their positions in A_val
    const Traveller<T> travellers[] = {{x, Kv.p, Kv.ld, x.recv}, {x, Vv.p, Vv.ld, recv2}};
    pack_exchange_run(e, s, t0, PACK_ON_EXCHANGE, travellers, [&](crp_csr_dev_p A, int part) {
        if (n == 0 || crp_csr_dev_nrow(A) == 0) return;
        HIP_OK(crp::attention(A, heads, d, scale, bias, Qv.p, Qv.ld, Kv.p, Kv.ld, (const T *) x.recv, x.ld, Vv.p, Vv.ld, (const T *) recv2, x.ld,
                              Ov.p, Ov.ld, lsev.dev, pv.dev, part_positions(e, part), s));
    });
    lsev.download(s);
    pv.download(s);
    finish_call(e, Ov, s, t0, lsev.staged || pv.staged || !Q_on_dev || !K_on_dev || !V_on_dev || timing, t_begin);
}

// ---- the backward ---------------------------------------------------------------------------------------------------------------------
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
static void attention_bwd_impl(crp_rp_spmm *e, int heads, double scale, int bias, const T *Q, long long ldQ, const T *K, long long ldK,
                               const T *V, long long ldV, const T *O, long long ldO, const T *dO, long long lddO, const T *lse, T *dQ,
                               long long lddQ, T *dK, long long lddK, T *dV, long long lddV, T *ds_out, void *stream_)
{
    if (e == NULL) return;
    const size_t nh = heads >= 1 ? (size_t) heads : 1;
    check_call(e, "rp_spmm_attention_bwd");
    check_scores(bias, scale, "scale");
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const int d = n / (int) nh;                         // one head's width, to which the cap applies
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
    T *delta = delta_of(e, K, nh);
    e->bw_built = true;
    if (n == 0)
    {
        e->n_exec++;
        return;
    }

    // ---- K then V travel as in the forward; the row side on the parts
    const Traveller<T> travellers[] = {{x, K, ldK, x.recv}, {x, V, ldV, recv2}};
    pack_exchange_run(e, s, t0, PACK_ON_EXCHANGE, travellers, [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        HIP_OK(crp::attention_bwd_q(A, heads, d, scale, bias, Q, ldQ, K, ldK, (const T *) x.recv, x.ld, V, ldV, (const T *) recv2, x.ld, O, ldO,
                                    dO, lddO, lse, dQ, lddQ, delta, ds_out, part_positions(e, part), s));
    });
    lap(e, s, t0, &e->t_spmm);

    // ---- the column side: the rows owed to peers in place over the received K and V rows, this rank's own directly
    auto kv = [&](crp_csr_dev_p At, const T *Kr, long long ldKr, const T *Vr, long long ldVr, T *dKr, long long lddKr, T *dVr, long long lddVr) {
        HIP_OK(crp::attention_bwd_kv(At, heads, d, scale, bias, Kr, ldKr, Vr, ldVr, Q, ldQ, dO, lddO, lse, delta, dKr, lddKr, dVr, lddVr, s));
    };
    if (e->At_rem != nullptr) kv(e->At_rem, (const T *) x.recv, x.ld, recv2, x.ld, (T *) x.recv, x.ld, recv2, x.ld);
    if (e->nproc > 1 && !timing)
    {
        // the first reverse exchange on its own stream beside the local kernel, which is enqueued first (see exec_t); the second
        // reuses the send buffer, so it waits on s for the first accumulate
        HIP_OK(crp_event_record(e->ev_packed, s));
        if (kb > 0) kv(e->At_loc, K, ldK, V, ldV, dK, lddK, dV, lddV);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        reverse_exchange_rows(e, x, x.recv, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        accumulate_rows(e, x, dK, lddK, s);
        reverse_exchange_rows(e, x, recv2, s);
        accumulate_rows(e, x, dV, lddV, s);
    }
    else
    {
        lap(e, s, t0, &e->t_spmm);
        if (kb > 0) kv(e->At_loc, K, ldK, V, ldV, dK, lddK, dV, lddV);
        lap(e, s, t0, &e->t_spmm);
        for (int op = 0; op < 2; op++)
        {
            if (e->nproc > 1) reverse_exchange_rows(e, x, op == 0 ? x.recv : (void *) recv2, s);
            lap(e, s, t0, &e->t_a2a);
            accumulate_rows(e, x, op == 0 ? dK : dV, op == 0 ? lddK : lddV, s);
            lap(e, s, t0, &e->t_unpack);
        }
    }
    close_call(e, s, false, timing, t_begin);
}

extern "C" {

void crp_rp_spmm_attention_ex(crp_rp_spmm_p e, int layout, double scale, int bias, const double *Q, long long ldQ, const double *K,
                              long long ldK, const double *V, long long ldV, double *O, long long ldO, double *lse, double *p_out,
                              void *stream)
{
    attention_impl<double>(e, layout, 0, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream);
}

void crp_rp_spmm_attention_f32_ex(crp_rp_spmm_p e, int layout, double scale, int bias, const float *Q, long long ldQ, const float *K,
                                  long long ldK, const float *V, long long ldV, float *O, long long ldO, float *lse, float *p_out,
                                  void *stream)
{
    attention_impl<float>(e, layout, 0, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream);
}

void crp_rp_spmm_attention_mh_ex(crp_rp_spmm_p e, int layout, int heads, double scale, int bias, const double *Q, long long ldQ,
                                 const double *K, long long ldK, const double *V, long long ldV, double *O, long long ldO, double *lse,
                                 double *p_out, void *stream)
{
    attention_impl<double>(e, layout, mh_heads(e, heads, "rp_spmm_attention_mh"), scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream);
}

void crp_rp_spmm_attention_mh_f32_ex(crp_rp_spmm_p e, int layout, int heads, double scale, int bias, const float *Q, long long ldQ,
                                     const float *K, long long ldK, const float *V, long long ldV, float *O, long long ldO, float *lse,
                                     float *p_out, void *stream)
{
    attention_impl<float>(e, layout, mh_heads(e, heads, "rp_spmm_attention_mh"), scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream);
}

int crp_rp_spmm_attention_built(crp_rp_spmm_p e) { return (e && e->at_built) ? 1 : 0; }

void crp_rp_spmm_attention_bwd_ex(crp_rp_spmm_p e, double scale, int bias, const double *Q, long long ldQ, const double *K, long long ldK,
                                  const double *V, long long ldV, const double *O, long long ldO, const double *dO, long long lddO,
                                  const double *lse, double *dQ, long long lddQ, double *dK, long long lddK, double *dV, long long lddV,
                                  double *ds_out, void *stream)
{
    attention_bwd_impl<double>(e, 0, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

void crp_rp_spmm_attention_bwd_f32_ex(crp_rp_spmm_p e, double scale, int bias, const float *Q, long long ldQ, const float *K, long long ldK,
                                      const float *V, long long ldV, const float *O, long long ldO, const float *dO, long long lddO,
                                      const float *lse, float *dQ, long long lddQ, float *dK, long long lddK, float *dV, long long lddV,
                                      float *ds_out, void *stream)
{
    attention_bwd_impl<float>(e, 0, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ, lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

void crp_rp_spmm_attention_bwd_mh_ex(crp_rp_spmm_p e, int heads, double scale, int bias, const double *Q, long long ldQ, const double *K,
                                     long long ldK, const double *V, long long ldV, const double *O, long long ldO, const double *dO,
                                     long long lddO, const double *lse, double *dQ, long long lddQ, double *dK, long long lddK, double *dV,
                                     long long lddV, double *ds_out, void *stream)
{
    attention_bwd_impl<double>(e, mh_heads(e, heads, "rp_spmm_attention_bwd_mh"), scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ,
                               lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

void crp_rp_spmm_attention_bwd_mh_f32_ex(crp_rp_spmm_p e, int heads, double scale, int bias, const float *Q, long long ldQ, const float *K,
                                         long long ldK, const float *V, long long ldV, const float *O, long long ldO, const float *dO,
                                         long long lddO, const float *lse, float *dQ, long long lddQ, float *dK, long long lddK, float *dV,
                                         long long lddV, float *ds_out, void *stream)
{
    attention_bwd_impl<float>(e, mh_heads(e, heads, "rp_spmm_attention_bwd_mh"), scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, dO, lddO, lse, dQ,
                              lddQ, dK, lddK, dV, lddV, ds_out, stream);
}

int crp_rp_spmm_attention_bwd_built(crp_rp_spmm_p e) { return (e && e->bw_built) ? 1 : 0; }

}  // extern "C"
