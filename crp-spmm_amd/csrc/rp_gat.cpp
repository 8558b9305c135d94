// rp_gat.cpp -- the row engine's fused GAT and GATv2 attention, forward (crp_rp_spmm_gat{,_f32}_ex, crp_rp_spmm_gatv2{,_f32}_ex,
// include/crp_engine.h): one implementation each, templated over the dtype.  Both hand their travellers to the schedule of
// rp_engine_impl.h (pack_exchange_run, packed on the exchange stream).  GAT has two: V travels as B does, through the forward
// exchange; er -- `heads` scalars per row of B -- travels in a narrow exchange of its own (GatXchg: the forward plan's row indices
// and peers, rows of `heads` elements), which the schedule sees as one more Xchg.  GATv2 has one, XS.  The part kernels are
// crp_gat_attention_csr_* / crp_gatv2_attention_csr_* on the engine's device matrices, whose two-source column codes name this
// rank's rows of er / V / XS and the received ones.
#include "rp_engine_impl.h"

static GatXchg<double> &gat_xchg_of(crp_rp_spmm *e, const double *) { return e->gt_x64; }
static GatXchg<float> &gat_xchg_of(crp_rp_spmm *e, const float *) { return e->gt_x32; }

// first call of a dtype, or a call with another number of heads: word counts by rows from the forward plan's, and the two narrow
// buffers, zeroed once (the fp32 rows' pad column is never written again: no uninitialised byte crosses a link); blocks
template <class T>
static GatXchg<T> &gat_exchange(crp_rp_spmm *e, int heads, const T *like)
{
    GatXchg<T> &g = gat_xchg_of(e, like);
    if (!e->gt_built)
    {
        upload_part_positions(e);
        e->gt_built = true;
    }
    if (g.heads == heads) return g;
    const long long words = ((long long) heads * (long long) sizeof(T) + 7) / 8;       // 8-byte words per row
    plan_words(e, words, g.sc, g.sd, g.rc, g.rd);
    g.ld = words * 8 / (long long) sizeof(T);
    g.send.reset();
    g.recv.reset();
    if (e->n_send_rows > 0) g.send.zeroed((size_t) e->n_send_rows * (size_t) g.ld);
    if (e->n_recv_rows > 0) g.recv.zeroed((size_t) e->n_recv_rows * (size_t) g.ld);
    g.heads = heads;
    return g;
}

template <class T>
static void gat_impl(crp_rp_spmm *e, int layout, int heads, double slope, int bias, const T *el, long long ldel, const T *er, long long lder,
                     const T *V, long long ldV, T *O, long long ldO, T *lse, T *p_out, void *stream_)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_gat", "layout", layout);
    check_scores(bias, slope, "slope");
    ASSERT_PRINTF(heads >= 1 && e->glb_n % heads == 0, "rp_spmm_gat: heads (%d) must be positive and divide the %d columns\n", heads, e->glb_n);
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const int d = n / heads;                            // one head's width
    const size_t nh = (size_t) heads, nnz = e->A_val.size();
    ASSERT_PRINTF(m == 0 || (el != NULL && on_device(el)), "rp_spmm_gat: el must be a device pointer\n");
    ASSERT_PRINTF(kb == 0 || (er != NULL && on_device(er)), "rp_spmm_gat: er must be a device pointer\n");
    ASSERT_PRINTF((m == 0 || ldel >= heads) && (kb == 0 || lder >= heads), "rp_spmm_gat: a leading dimension of el / er is below %d\n", heads);
    const double t_begin = get_wtime_sec();
    void *s = stream_;
    const bool timing = e->timing != 0;
    double t0;

    const Xchg x = exchange_of(e, V);
    const Xchg gx = gat_exchange(e, heads, V).view();
    if (n == 0)
    {
        e->n_exec++;
        return;
    }
    const bool V_on_dev = on_device(V), O_on_dev = on_device(O);

    // ---- V and O as device-resident row-major views: V takes B's buffers and the forward exchange, O takes C's
    const crp::InView<T> Vv = crp::operand_in(layout, V, ldV, kb, n, V_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    const HostVec<T> lsev = host_vec(lse, lse != NULL ? (size_t) m * nh : 0, e->at_lse);
    const HostVec<T> pv = host_vec(p_out, p_out != NULL ? nnz * nh : 0, e->sd_out);

    // ---- pack and exchange V, then er; the kernels: the parts of a split engine write O and lse through their row maps and p_out
    // through their positions in A_val
    const Traveller<T> travellers[] = {{x, Vv.p, Vv.ld, x.recv}, {gx, er, lder, gx.recv}};
    pack_exchange_run(e, s, t0, PACK_ON_EXCHANGE, travellers, [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        HIP_OK(crp::gat_attention(A, heads, d, slope, bias, el, ldel, er, lder, (const T *) gx.recv, gx.ld, Vv.p, Vv.ld, (const T *) x.recv, x.ld,
                                  Ov.p, Ov.ld, lsev.dev, pv.dev, part_positions(e, part), s));
    });
    lsev.download(s);
    pv.download(s);
    finish_call(e, Ov, s, t0, lsev.staged || pv.staged || !V_on_dev || timing, t_begin);
}

// ---- GATv2 (crp_rp_spmm_gatv2{,_f32}_ex): XS is the score operand and the value operand, so it is the one operand that travels, as
// B does, through the forward exchange only; XT and a are local.  The first call uploads the parts' positions and nothing else.
template <class T>
static void gatv2_impl(crp_rp_spmm *e, int layout, int heads, double slope, int bias, const T *XT, long long ldXT, const T *av, const T *XS,
                       long long ldXS, T *O, long long ldO, T *lse, T *p_out, void *stream_)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_gatv2", "layout", layout);
    check_scores(bias, slope, "slope");
    ASSERT_PRINTF(heads >= 1 && e->glb_n % heads == 0, "rp_spmm_gatv2: heads (%d) must be positive and divide the %d columns\n", heads, e->glb_n);
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const int d = n / heads;                            // one head's width
    const size_t nh = (size_t) heads, nnz = e->A_val.size();
    ASSERT_PRINTF(n == 0 || m == 0 || (XT != NULL && on_device(XT)), "rp_spmm_gatv2: XT must be a device pointer\n");
    ASSERT_PRINTF(n == 0 || m == 0 || (av != NULL && on_device(av)), "rp_spmm_gatv2: a must be a device pointer\n");
    ASSERT_PRINTF(m == 0 || ldXT >= n, "rp_spmm_gatv2: the leading dimension of XT is below %d\n", n);
    ASSERT_PRINTF(d <= 4 * 64 * (16 / (int) sizeof(T)), "rp_spmm_gatv2: a head of %d columns is over the width cap\n", d);
    const double t_begin = get_wtime_sec();
    void *s = stream_;
    const bool timing = e->timing != 0;
    double t0;

    const Xchg x = exchange_of(e, XS);
    if (!e->gv2_built)
    {
        upload_part_positions(e);
        e->gv2_built = true;
    }
    if (n == 0)
    {
        e->n_exec++;
        return;
    }
    const bool X_on_dev = on_device(XS), O_on_dev = on_device(O);

    // ---- XS and O as device-resident row-major views: XS takes B's buffers and the forward exchange, O takes C's
    const crp::InView<T> Xv = crp::operand_in(layout, XS, ldXS, kb, n, X_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    const HostVec<T> lsev = host_vec(lse, lse != NULL ? (size_t) m * nh : 0, e->at_lse);
    const HostVec<T> pv = host_vec(p_out, p_out != NULL ? nnz * nh : 0, e->sd_out);

    // ---- pack and exchange XS; the kernels: the parts of a split engine write O and lse through their row maps and p_out through
    // their positions in A_val
    const Traveller<T> travellers[] = {{x, Xv.p, Xv.ld, x.recv}};
    pack_exchange_run(e, s, t0, PACK_ON_EXCHANGE, travellers, [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        HIP_OK(crp::gatv2_attention(A, heads, d, slope, bias, XT, ldXT, Xv.p, Xv.ld, (const T *) x.recv, x.ld, av, Ov.p, Ov.ld, lsev.dev, pv.dev,
                                    part_positions(e, part), s));
    });
    lsev.download(s);
    pv.download(s);
    finish_call(e, Ov, s, t0, lsev.staged || pv.staged || !X_on_dev || timing, t_begin);
}

extern "C" {

void crp_rp_spmm_gat_ex(crp_rp_spmm_p e, int layout, int heads, double slope, int bias, const double *el, long long ldel, const double *er,
                        long long lder, const double *V, long long ldV, double *O, long long ldO, double *lse, double *p_out, void *stream)
{
    gat_impl<double>(e, layout, heads, slope, bias, el, ldel, er, lder, V, ldV, O, ldO, lse, p_out, stream);
}

void crp_rp_spmm_gat_f32_ex(crp_rp_spmm_p e, int layout, int heads, double slope, int bias, const float *el, long long ldel, const float *er,
                            long long lder, const float *V, long long ldV, float *O, long long ldO, float *lse, float *p_out, void *stream)
{
    gat_impl<float>(e, layout, heads, slope, bias, el, ldel, er, lder, V, ldV, O, ldO, lse, p_out, stream);
}

int crp_rp_spmm_gat_built(crp_rp_spmm_p e) { return (e && e->gt_built) ? 1 : 0; }

void crp_rp_spmm_gatv2_ex(crp_rp_spmm_p e, int layout, int heads, double slope, int bias, const double *XT, long long ldXT, const double *a,
                          const double *XS, long long ldXS, double *O, long long ldO, double *lse, double *p_out, void *stream)
{
    gatv2_impl<double>(e, layout, heads, slope, bias, XT, ldXT, a, XS, ldXS, O, ldO, lse, p_out, stream);
}

void crp_rp_spmm_gatv2_f32_ex(crp_rp_spmm_p e, int layout, int heads, double slope, int bias, const float *XT, long long ldXT, const float *a,
                              const float *XS, long long ldXS, float *O, long long ldO, float *lse, float *p_out, void *stream)
{
    gatv2_impl<float>(e, layout, heads, slope, bias, XT, ldXT, a, XS, ldXS, O, ldO, lse, p_out, stream);
}

int crp_rp_spmm_gatv2_built(crp_rp_spmm_p e) { return (e && e->gv2_built) ? 1 : 0; }

}  // extern "C"
