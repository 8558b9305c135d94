// rp_gat.cpp -- the row engine's fused GAT and GATv2 attention, forward (crp_rp_spmm_gat{,_f32}_ex, crp_rp_spmm_gatv2{,_f32}_ex,
// include/crp_engine.h): one implementation each, templated over the dtype.  GAT:  V travels as B does, through the forward exchange; er -- `heads` scalars per row of B -- travels in a
// narrow exchange of its own (GatXchg, rp_engine_impl.h): the forward plan's row indices and peers, rows of `heads` elements.
// The part kernels are crp_gat_attention_csr_* on the engine's device matrices, whose two-source column codes name this rank's
// rows of er / V and the received ones.
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
    const long long n = e->glb_n;                       // rB_* hold rows * glb_n elements
    auto by_rows = [&](const std::vector<long long> &v, std::vector<long long> &out) {
        out.resize(v.size());
        for (size_t q = 0; q < v.size(); q++) out[q] = n > 0 ? v[q] / n * words : 0;
    };
    by_rows(e->rB_scnts, g.sc);
    by_rows(e->rB_sdispls, g.sd);
    by_rows(e->rB_rcnts, g.rc);
    by_rows(e->rB_rdispls, g.rd);
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
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_gat on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(layout == 0 || layout == 1, "layout must be 0 or 1\n");
    ASSERT_PRINTF(bias == 0 || bias == 1, "bias must be 0 or 1\n");
    ASSERT_PRINTF(slope - slope == 0.0, "slope must be finite\n");
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
    GatXchg<T> &g = gat_exchange(e, heads, V);
    if (n == 0)
    {
        e->n_exec++;
        return;
    }
    const bool V_on_dev = on_device(V), O_on_dev = on_device(O);
    const bool lse_host = lse != NULL && m > 0 && !on_device(lse), p_host = p_out != NULL && nnz > 0 && !on_device(p_out);

    // ---- V and O as device-resident row-major views: V takes B's buffers and the forward exchange, O takes C's
    const crp::InView<T> Vv = crp::operand_in(layout, V, ldV, kb, n, V_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    T *lsed = lse_host ? e->at_lse.grow<T>((size_t) m * nh) : lse;
    T *pd = p_host ? e->sd_out.grow<T>(nnz * nh) : p_out;

    auto pack_er = [&](void *st) {
        if (e->n_send_rows > 0) HIP_OK(crp::gather((int) e->n_send_rows, heads, e->sridxs_dev, er, lder, g.send.get(), g.ld, st));
    };
    auto exchange_er = [&](void *st) {
        const double tx0 = get_wtime_sec();
        e->comm->alltoallv_dev_f64(e->comm->ctx, (const double *) g.send.get(), g.sc.data(), g.sd.data(), (double *) g.recv.get(), g.rc.data(),
                                   g.rd.data(), st);
        e->t_a2a_host += get_wtime_sec() - tx0;
    };
    // the parts of a split engine write O and lse through their row maps and p_out through their positions in A_val
    auto product = [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        const int *pos = part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
        HIP_OK(crp::gat_attention(A, heads, d, slope, bias, el, ldel, er, lder, (const T *) g.recv.get(), g.ld, Vv.p, Vv.ld, (const T *) x.recv,
                                  x.ld, Ov.p, Ov.ld, lsed, pd, pos, s));
    };

    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->A_int != nullptr && !timing)
    {
        // the interior part first on s; both packs and exchanges beside it on the engine's second stream, from the point of s
        // where the operands are ready; the boundary part after both have landed (pack_exchange_run2, rp_attention.cpp)
        HIP_OK(crp_event_record(e->ev_packed, s));
        product(e->A_int, 1);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        pack_rows(e, x, Vv.p, Vv.ld, e->xstream);
        exchange_rows(e, x, x.recv, e->xstream);
        pack_er(e->xstream);
        exchange_er(e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        product(e->A_bnd, 2);
    }
    else
    {
        pack_rows(e, x, Vv.p, Vv.ld, s);
        pack_er(s);
        lap(e, s, t0, &e->t_pack);
        if (e->nproc > 1)
        {
            exchange_rows(e, x, x.recv, s);
            exchange_er(s);
        }
        lap(e, s, t0, &e->t_a2a);
        run_parts(e, product);
    }
    if (lse_host) HIP_OK(crp_dev_memcpy(lse, lsed, (size_t) m * nh * sizeof(T), 1, s));
    if (p_host) HIP_OK(crp_dev_memcpy(p_out, pd, nnz * nh * sizeof(T), 1, s));
    const bool synced = crp::finish(Ov, s, [&] { lap(e, s, t0, &e->t_spmm); });
    complete(e, s, synced, lse_host || p_host || !V_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

// ---- GATv2 (crp_rp_spmm_gatv2{,_f32}_ex): XS is the score operand and the value operand, so it is the one operand that travels, as
// B does, through the forward exchange only; XT and a are local.  The first call uploads the parts' positions and nothing else.
template <class T>
static void gatv2_impl(crp_rp_spmm *e, int layout, int heads, double slope, int bias, const T *XT, long long ldXT, const T *av, const T *XS,
                       long long ldXS, T *O, long long ldO, T *lse, T *p_out, void *stream_)
{
    if (e == NULL) return;
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_gatv2 on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(layout == 0 || layout == 1, "layout must be 0 or 1\n");
    ASSERT_PRINTF(bias == 0 || bias == 1, "bias must be 0 or 1\n");
    ASSERT_PRINTF(slope - slope == 0.0, "slope must be finite\n");
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
    const bool lse_host = lse != NULL && m > 0 && !on_device(lse), p_host = p_out != NULL && nnz > 0 && !on_device(p_out);

    // ---- XS and O as device-resident row-major views: XS takes B's buffers and the forward exchange, O takes C's
    const crp::InView<T> Xv = crp::operand_in(layout, XS, ldXS, kb, n, X_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    T *lsed = lse_host ? e->at_lse.grow<T>((size_t) m * nh) : lse;
    T *pd = p_host ? e->sd_out.grow<T>(nnz * nh) : p_out;

    // the parts of a split engine write O and lse through their row maps and p_out through their positions in A_val
    auto product = [&](crp_csr_dev_p A, int part) {
        if (crp_csr_dev_nrow(A) == 0) return;
        const int *pos = part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
        HIP_OK(crp::gatv2_attention(A, heads, d, slope, bias, XT, ldXT, Xv.p, Xv.ld, (const T *) x.recv, x.ld, av, Ov.p, Ov.ld, lsed, pd, pos, s));
    };

    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->A_int != nullptr && !timing)
    {
        // the interior part first on s; the pack and the exchange beside it on the engine's second stream, from the point of s where
        // the operand is ready; the boundary part after it has landed
        HIP_OK(crp_event_record(e->ev_packed, s));
        product(e->A_int, 1);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        pack_rows(e, x, Xv.p, Xv.ld, e->xstream);
        exchange_rows(e, x, x.recv, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        product(e->A_bnd, 2);
    }
    else
    {
        pack_rows(e, x, Xv.p, Xv.ld, s);
        lap(e, s, t0, &e->t_pack);
        if (e->nproc > 1) exchange_rows(e, x, x.recv, s);
        lap(e, s, t0, &e->t_a2a);
        run_parts(e, product);
    }
    if (lse_host) HIP_OK(crp_dev_memcpy(lse, lsed, (size_t) m * nh * sizeof(T), 1, s));
    if (p_host) HIP_OK(crp_dev_memcpy(p_out, pd, nnz * nh * sizeof(T), 1, s));
    const bool synced = crp::finish(Ov, s, [&] { lap(e, s, t0, &e->t_spmm); });
    complete(e, s, synced, lse_host || p_host || !X_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
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
