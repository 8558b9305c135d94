// rp_engine.cpp -- the 1D row-parallel SpMM engine (include/crp_engine.h).
//
// Host side of /root/reference/src/rowpara_spmm.c re-thought for a device-
// resident data path:
//   init  (reference :20-190): one pass builds the needed-row flags, a prefix
//         rank array gives the compact ids, the needs are exchanged through the
//         communicator's alltoall(v); A is uploaded once with a two-source column
//         index (local B row | row of the receive buffer), so exec never copies
//         locally owned B rows and never unpacks.
//   exec  (reference :212-422): gather kernel -> device all-to-all -> SpMM kernel;
//         no allocation, no sparse-handle creation.  Exec and sddmm hand their one
//         travelling operand to the schedule all calls share (pack_exchange_run,
//         rp_engine_impl.h); exec_t runs the plan backwards with that file's helpers.
// Public plan fields keep the reference's meaning (crp_rp_plan_view_t).
#include "rp_engine_impl.h"

// ---------------------------------------------------------------------------
static void build_plan(crp_rp_spmm *e, int A_nrow, const int *A_rowptr, const int *A_colidx,
                       const double *A_val, const int *B_row_displs, int glb_n, crp_comm_t *comm)
{
    const int P = comm->nproc, me = comm->rank;
    e->nproc = P;
    e->my_rank = me;
    e->glb_n = glb_n;
    e->A_nrow = A_nrow;
    e->comm = comm;
    GET_ENV_INT_VAR(e->rB_p2p, "RP_SPMM_P2P", "rB_p2p", 1, 0, 1, me == 0);
    GET_ENV_INT_VAR(e->rB_reidx, "RP_SPMM_REIDX", "rB_reidx", 1, 0, 1, me == 0);

    const int    base = A_rowptr[0];
    const size_t nnz  = (size_t) ((long long) A_rowptr[A_nrow] - (long long) base);
    const int    glb_k = B_row_displs[P];
    const int    lo = B_row_displs[me], hi = B_row_displs[me + 1];
    e->loc_B_nrow = hi - lo;

    // needed-row flags and the span of touched columns
    std::vector<unsigned char> flag((size_t) glb_k + 1, 0);
    int cmin = INT_MAX, cmax = -1;
    for (size_t p = 0; p < nnz; p++)
    {
        const int c = A_colidx[p];
        ASSERT_PRINTF(c >= 0 && c < glb_k, "column index %d outside B (%d rows)\n", c, glb_k);
        flag[c] = 1;
        if (c < cmin) cmin = c;
        if (c > cmax) cmax = c;
    }
    if (nnz == 0) { cmin = 0; cmax = -1; }

    // rank_[g] = number of needed rows with global index < g
    std::vector<int> rank_((size_t) glb_k + 1);
    int run = 0;
    for (int g = 0; g < glb_k; g++)
    {
        rank_[g] = run;
        run += flag[g];
    }
    rank_[glb_k] = run;
    const int n_needed = run;
    e->n_needed_rows = n_needed;
    e->rB_nrow = e->rB_reidx ? n_needed : (cmax - cmin + 1);

    // rebased / re-indexed copy of A (public plan fields)
    e->A_rowptr.resize((size_t) A_nrow + 1);
    for (int i = 0; i <= A_nrow; i++) e->A_rowptr[i] = A_rowptr[i] - base;
    e->A_colidx.resize(nnz);
    e->A_val.assign(A_val, A_val + nnz);
    for (size_t p = 0; p < nnz; p++)
        e->A_colidx[p] = e->rB_reidx ? rank_[A_colidx[p]] : (A_colidx[p] - cmin);

    // rows served from this rank's own block of B
    const int self_n = rank_[hi] - rank_[lo];
    e->rB_self_nrow = self_n;
    e->rB_self_src_ridxs.clear();
    e->rB_self_src_ridxs.reserve((size_t) self_n);
    for (int g = lo; g < hi; g++)
        if (flag[g]) e->rB_self_src_ridxs.push_back(g);
    if (self_n > 0)
    {
        const int first = e->rB_self_src_ridxs[0];
        e->rB_self_src_offset = first - lo;
        e->rB_self_dst_offset = e->rB_reidx ? rank_[first] : (first - cmin);
    }

    // rows to fetch, grouped by owner (owners hold ascending contiguous ranges,
    // so ascending global order is already owner order)
    std::vector<int> rcnt(P, 0), rdsp(P + 1, 0), need_glb;
    need_glb.reserve((size_t) (n_needed - self_n));
    for (int q = 0; q < P; q++)
    {
        if (q != me)
            for (int g = B_row_displs[q]; g < B_row_displs[q + 1]; g++)
                if (flag[g]) need_glb.push_back(g);
        rdsp[q + 1] = (int) need_glb.size();
        rcnt[q] = rdsp[q + 1] - rdsp[q];
    }
    e->n_recv_rows = rdsp[P];
    e->rB_recv_size = (size_t) rdsp[P];

    // tell every owner which of its rows are wanted (reference :152-165)
    std::vector<int> scnt(P, 0), sdsp(P + 1, 0);
    comm->alltoall_i32(comm->ctx, rcnt.data(), scnt.data(), 1);
    for (int q = 0; q < P; q++) sdsp[q + 1] = sdsp[q] + scnt[q];
    e->n_send_rows = sdsp[P];
    e->rB_sridxs.assign((size_t) sdsp[P] + 1, 0);
    if (need_glb.empty()) need_glb.push_back(0);   // keep .data() valid for empty lists
    comm->alltoallv_i32(comm->ctx, need_glb.data(), rcnt.data(), rdsp.data(), e->rB_sridxs.data(), scnt.data(),
                        sdsp.data());
    e->rB_sridxs.resize((size_t) sdsp[P]);
    for (auto &r : e->rB_sridxs)
    {
        ASSERT_PRINTF(r >= lo && r < hi, "peer requested row %d outside my block [%d, %d)\n", r, lo, hi);
        r -= lo;
    }

    e->rB_rridxs.resize((size_t) rdsp[P]);
    for (int i = 0; i < rdsp[P]; i++)
        e->rB_rridxs[i] = e->rB_reidx ? rank_[need_glb[i]] : (need_glb[i] - cmin);

    e->rB_rcnts.resize(P);
    e->rB_rdispls.resize((size_t) P + 1);
    e->rB_scnts.resize(P);
    e->rB_sdispls.resize((size_t) P + 1);
    for (int q = 0; q < P; q++)
    {
        e->rB_rcnts[q] = (long long) rcnt[q] * glb_n;
        e->rB_scnts[q] = (long long) scnt[q] * glb_n;
    }
    for (int q = 0; q <= P; q++)
    {
        e->rB_rdispls[q] = (long long) rdsp[q] * glb_n;
        e->rB_sdispls[q] = (long long) sdsp[q] * glb_n;
    }

    // device column index: local B row, or ~(position in the receive buffer).
    // Position = rank among needed rows minus the self rows that precede it.
    e->dev_colidx_host.resize(nnz);
    for (size_t p = 0; p < nnz; p++)
    {
        const int g = A_colidx[p];
        if (g >= lo && g < hi) e->dev_colidx_host[p] = g - lo;
        else e->dev_colidx_host[p] = ~(rank_[g] - (g >= hi ? self_n : 0));
    }
}

// Upload A: whole, or split by rows into interior / boundary parts when an exchange exists and
// both parts are worth a launch (CRPSPMM_OVERLAP=0 keeps the single product).
// A_val_dev (optional): the values of the rank's panel, in the panel's order, already in device memory (para2d_engine.cpp: the
// device all-gather of the panel) -- the device matrices then take their values from there, not from a second upload.
static void build_device_matrices(crp_rp_spmm *e, const double *A_val_dev)
{
    const int m = e->A_nrow;
    const int overlap = crp::knobs().overlap;
    std::vector<int> rows_int, rows_bnd;
    if (overlap && e->nproc > 1 && e->n_recv_rows > 0)
    {
        for (int i = 0; i < m; i++)
        {
            bool remote = false;
            for (int p = e->A_rowptr[i]; p < e->A_rowptr[i + 1] && !remote; p++) remote = e->dev_colidx_host[p] < 0;
            (remote ? rows_bnd : rows_int).push_back(i);
        }
    }
    // a part smaller than 1/16 of the rows does not pay for a second launch
    if (rows_int.size() < (size_t) m / 16 || rows_bnd.empty())
    {
        if (A_val_dev != nullptr && !e->A_val.empty())
            HIP_OK(crp_csr_dev_create_dv(m, e->loc_B_nrow, e->A_rowptr.data(), e->dev_colidx_host.data(), e->A_val.data(), A_val_dev, nullptr, e->A_dev.out()));
        else
            HIP_OK(crp_csr_dev_create(m, e->loc_B_nrow, e->A_rowptr.data(), e->dev_colidx_host.data(), e->A_val.data(), e->A_dev.out()));
        return;
    }
    // (a row's entries keep A_val's order inside its part: the fused attention's online softmax adds them in CSR order, and its
    //  bit-identity across rank counts rests on that)
    auto make = [&](const std::vector<int> &rows, std::vector<long long> &src, crp_csr_dev_p *out) {
        std::vector<int> rp(rows.size() + 1, 0), ci, start(rows.size(), 0);
        std::vector<double> va;
        src.clear();
        for (size_t t = 0; t < rows.size(); t++)
        {
            const int i = rows[t];
            start[t] = e->A_rowptr[i];
            for (int p = e->A_rowptr[i]; p < e->A_rowptr[i + 1]; p++)
            {
                ci.push_back(e->dev_colidx_host[p]);
                va.push_back(e->A_val[p]);
                src.push_back(p);
            }
            rp[t + 1] = (int) ci.size();
        }
        const bool have = !ci.empty();
        if (ci.empty()) { ci.push_back(0); va.push_back(0.0); }
        if (A_val_dev != nullptr && have)
            HIP_OK(crp_csr_dev_create_dv((int) rows.size(), e->loc_B_nrow, rp.data(), ci.data(), va.data(), A_val_dev, start.data(), out));
        else
            HIP_OK(crp_csr_dev_create((int) rows.size(), e->loc_B_nrow, rp.data(), ci.data(), va.data(), out));
        HIP_OK(crp_csr_dev_set_rowmap(*out, rows.data(), m));
    };
    make(rows_int, e->int_src, e->A_int.out());
    make(rows_bnd, e->bnd_src, e->A_bnd.out());
    e->xstream.ensure();
    e->ev_packed.ensure();
    e->ev_landed.ensure();
}

static void rp_init_common(int A_nrow, const int *A_rowptr, const int *A_colidx, const double *A_val,
                           const int *B_row_displs, int glb_n, crp_comm_t *comm, crp_rp_spmm_p *out,
                           bool plan_only, const double *A_val_dev = nullptr)
{
    ASSERT_PRINTF(out != NULL && comm != NULL && A_rowptr != NULL && B_row_displs != NULL && A_nrow >= 0 && glb_n >= 0,
                  "invalid arguments to rp_spmm_init\n");
    const double t0 = get_wtime_sec();
    crp_rp_spmm *e = new crp_rp_spmm;
    e->plan_only = plan_only;
    build_plan(e, A_nrow, A_rowptr, A_colidx, A_val, B_row_displs, glb_n, comm);
    if (!plan_only)
    {
        build_device_matrices(e, A_val_dev);
        e->vals_from_device = (A_val_dev != nullptr);
        e->stream.ensure();
        if (e->n_send_rows > 0)
        {
            e->sridxs_dev.upload(e->rB_sridxs.data(), (size_t) e->n_send_rows, NULL);
            e->sendbuf_dev.alloc((size_t) e->n_send_rows * (size_t) glb_n);
        }
        if (e->n_recv_rows > 0) e->recvbuf_dev.alloc((size_t) e->n_recv_rows * (size_t) glb_n);
        HIP_OK(crp_stream_sync(NULL));
    }
    e->t_init = get_wtime_sec() - t0;
    *out = e;
}

extern "C" {

void crp_rp_spmm_init(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx, const double *A_val,
                      const int *B_row_displs, int glb_n, crp_comm_t *comm, crp_rp_spmm_p *rp_spmm)
{
    (void) A_srow;   // never read by the reference either (src/rowpara_spmm.c:20-24)
    rp_init_common(A_nrow, A_rowptr, A_colidx, A_val, B_row_displs, glb_n, comm, rp_spmm, false);
}

void crp_rp_spmm_init_dv(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx, const double *A_val,
                         const double *A_val_dev, const int *B_row_displs, int glb_n, crp_comm_t *comm, crp_rp_spmm_p *rp_spmm)
{
    (void) A_srow;
    rp_init_common(A_nrow, A_rowptr, A_colidx, A_val, B_row_displs, glb_n, comm, rp_spmm, false, A_val_dev);
}

int crp_rp_spmm_values_from_device(crp_rp_spmm_p e) { return (e && e->vals_from_device) ? 1 : 0; }

void crp_rp_spmm_init_plan_only(int A_srow, int A_nrow, const int *A_rowptr, const int *A_colidx,
                                const double *A_val, const int *B_row_displs, int glb_n, crp_comm_t *comm,
                                crp_rp_spmm_p *rp_spmm)
{
    (void) A_srow;
    rp_init_common(A_nrow, A_rowptr, A_colidx, A_val, B_row_displs, glb_n, comm, rp_spmm, true);
}

void crp_rp_spmm_free(crp_rp_spmm_p *rp_spmm)
{
    if (rp_spmm == NULL || *rp_spmm == NULL) return;
    delete *rp_spmm;       // every device resource is a member that releases itself
    *rp_spmm = NULL;
}

}  // extern "C"

static int spmm(crp_rp_spmm *e, crp_csr_dev_p A, int n, const double *B0, long long ldB0, const double *B1, long long ldB1,
                double *C, long long ldC, void *s)
{
    return crp_spmm_csr_f64(A, 0, n, B0, ldB0, B1, ldB1, C, ldC, e->variant, s);
}
static int spmm(crp_rp_spmm *e, crp_csr_dev_p A, int n, const float *B0, long long ldB0, const float *B1, long long ldB1,
                float *C, long long ldC, void *s)
{
    return crp_spmm_csr_f32(A, n, B0, ldB0, B1, ldB1, C, ldC, e->variant_f32, s);
}

// C := A * B on this rank, one dtype (crp_rp_spmm_exec_ex / crp_rp_spmm_exec_f32_ex): B travels, packed on the caller's stream
template <class T>
static void exec_impl(crp_rp_spmm *e, int BC_layout, const T *B, long long ldB, T *C, long long ldC, void *stream_)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_exec", "BC_layout", BC_layout);
    const double t_begin = get_wtime_sec();
    void *s = stream_;   // taken literally: NULL is the HIP null stream (torch's default stream)
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const bool timing = e->timing != 0;
    double t0;

    const bool B_on_dev = on_device(B, &e->last_B, &e->last_B_dev), C_on_dev = on_device(C, &e->last_C, &e->last_C_dev);

    // ---- B as a device-resident row-major view, and where to compute C
    const Xchg x = exchange_of(e, B);
    const crp::InView<T> Bv = crp::operand_in(BC_layout, B, ldB, kb, n, B_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Cv = crp::operand_out(BC_layout, C, ldC, m, n, C_on_dev, e->C_stage, e->C_rm);

    // ---- 1 - 3. pack, exchange, local SpMM
    const Traveller<T> travellers[] = {{x, Bv.p, Bv.ld, x.recv}};
    pack_exchange_run(e, s, t0, PACK_ON_CALLER, travellers,
                      [&](crp_csr_dev_p A, int) { HIP_OK(spmm(e, A, n, Bv.p, Bv.ld, (const T *) x.recv, x.ld, Cv.p, Cv.ld, s)); });
    finish_call(e, Cv, s, t0, !B_on_dev || timing, t_begin);
}

// ---- out[p] = < X[row(p)], Y[col(p)] > over this rank's rows of A (crp_rp_spmm_sddmm_ex / _f32_ex); the helpers: rp_engine_impl.h
template <class T>
static void sddmm_impl(crp_rp_spmm *e, int layout, const T *X, long long ldX, const T *Y, long long ldY, T *out, int mode, void *stream_)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_sddmm", "layout", layout);
    ASSERT_PRINTF(mode == 0 || mode == 1, "mode must be 0 or 1\n");
    const double t_begin = get_wtime_sec();
    if (!e->sd_built)
    {
        upload_part_positions(e);
        e->sd_built = true;
    }
    void *s = stream_;
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const size_t nnz = e->A_val.size();
    const bool timing = e->timing != 0;
    double t0;

    const bool X_on_dev = on_device(X), Y_on_dev = on_device(Y);

    // ---- operands as device-resident row-major views: Y takes B's buffers, X takes C's
    const Xchg x = exchange_of(e, Y);
    const crp::InView<T> Yv = crp::operand_in(layout, Y, ldY, kb, n, Y_on_dev, e->B_stage, e->B_rm, s);
    const crp::InView<T> Xv = crp::operand_in(layout, X, ldX, m, n, X_on_dev, e->C_stage, e->C_rm, s);
    const HostVec<T> outv = host_vec(out, nnz, e->sd_out);

    if (n == 0 && nnz > 0) HIP_OK(crp_dev_memset(outv.dev, 0, nnz * sizeof(T), s));      // empty dots

    // ---- pack Y on the caller's stream, exchange, the kernels: the parts of a split engine write through their positions in A_val
    const Traveller<T> travellers[] = {{x, Yv.p, Yv.ld, x.recv}};
    pack_exchange_run(e, s, t0, PACK_ON_CALLER, travellers, [&](crp_csr_dev_p A, int part) {
        if (n == 0 || crp_csr_dev_nnz(A) == 0) return;
        HIP_OK(crp::sddmm(A, n, Xv.p, Xv.ld, Yv.p, Yv.ld, (const T *) x.recv, x.ld, outv.dev, part_positions(e, part), mode, s));
    });
    lap(e, s, t0, &e->t_spmm);
    outv.download(s);
    close_call(e, s, false, outv.staged || !X_on_dev || !Y_on_dev || timing, t_begin);
}

// ---- C := A^T * B (crp_rp_spmm_exec_t_ex); build_transposed: rp_engine_impl.h
// new values (A_val, already copied into e->A_val) for the transposed matrices
static void update_transposed_values(crp_rp_spmm *e)
{
    refresh_host_values(e);
    const size_t nnz = e->A_val.size();
    e->split_vals.resize(nnz);
    for (size_t q = 0; q < nnz; q++) e->split_vals[q] = e->A_val[(size_t) e->t_src[q]];
    if (e->t_loc_nnz > 0) HIP_OK(crp_csr_dev_update_values(e->At_loc, e->split_vals.data(), e->stream));
    if (e->At_rem != nullptr && nnz > e->t_loc_nnz)
        HIP_OK(crp_csr_dev_update_values(e->At_rem, e->split_vals.data() + e->t_loc_nnz, e->stream));
    HIP_OK(crp_stream_sync(e->stream));
}

// one dtype (crp_rp_spmm_exec_t_ex / crp_rp_spmm_exec_t_f32_ex): the transposed matrices, the accumulate lists, streams and events are
// shared, the products, the exchange buffers (exchange_of: the forward plan's, run backwards) and the accumulate are the dtype's own
template <class T>
static void exec_t_impl(crp_rp_spmm *e, int BC_layout, const T *B, long long ldB, T *C, long long ldC, void *stream_)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_exec_t", "BC_layout", BC_layout);
    const double t_begin = get_wtime_sec();
    if (!e->t_built) build_transposed(e);
    void *s = stream_;
    // B has A's rows, C the rows of this rank's block of the forward operand
    const int n = e->glb_n, mb = e->A_nrow, mc = e->loc_B_nrow;
    const bool timing = e->timing != 0;
    double t0;

    const bool B_on_dev = on_device(B), C_on_dev = on_device(C);

    // ---- B as a device-resident row-major view, and where to compute C
    const Xchg x = exchange_of(e, B);
    const crp::InView<T> Bv = crp::operand_in(BC_layout, B, ldB, mb, n, B_on_dev, e->B_stage, e->B_rm, s);
    const crp::OutView<T> Cv = crp::operand_out(BC_layout, C, ldC, mc, n, C_on_dev, e->C_stage, e->C_rm);

    auto product = [&](crp_csr_dev_p A, T *out, long long ldo) { HIP_OK(spmm(e, A, n, Bv.p, Bv.ld, (const T *) NULL, 0, out, ldo, s)); };

    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->nproc > 1 && !timing)
    {
        // the exchange on its own stream beside the local product, which is enqueued first (see exec_impl)
        if (e->At_rem != nullptr) product(e->At_rem, (T *) x.recv, x.ld);
        HIP_OK(crp_event_record(e->ev_packed, s));
        product(e->At_loc, Cv.p, Cv.ld);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        reverse_exchange_rows(e, x, x.recv, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        accumulate_rows(e, x, Cv.p, Cv.ld, s);
    }
    else
    {
        if (e->At_rem != nullptr) product(e->At_rem, (T *) x.recv, x.ld);
        lap(e, s, t0, &e->t_spmm);
        if (e->nproc > 1) reverse_exchange_rows(e, x, x.recv, s);
        lap(e, s, t0, &e->t_a2a);
        product(e->At_loc, Cv.p, Cv.ld);
        lap(e, s, t0, &e->t_spmm);
        accumulate_rows(e, x, Cv.p, Cv.ld, s);
        lap(e, s, t0, &e->t_unpack);
    }
    finish_call(e, Cv, s, t0, !B_on_dev || timing, t_begin);
}

extern "C" {

void crp_rp_spmm_exec_t_ex(crp_rp_spmm_p e, int BC_layout, const double *B, long long ldB, double *C, long long ldC, void *stream_)
{
    exec_t_impl<double>(e, BC_layout, B, ldB, C, ldC, stream_);
}

void crp_rp_spmm_exec_t_f32_ex(crp_rp_spmm_p e, int BC_layout, const float *B, long long ldB, float *C, long long ldC, void *stream_)
{
    exec_t_impl<float>(e, BC_layout, B, ldB, C, ldC, stream_);
}

int crp_rp_spmm_transposed_built(crp_rp_spmm_p e) { return (e && e->t_built) ? 1 : 0; }

void crp_rp_spmm_sddmm_ex(crp_rp_spmm_p e, int layout, const double *X, long long ldX, const double *Y, long long ldY, double *out,
                          int mode, void *stream_)
{
    sddmm_impl<double>(e, layout, X, ldX, Y, ldY, out, mode, stream_);
}

void crp_rp_spmm_sddmm_f32_ex(crp_rp_spmm_p e, int layout, const float *X, long long ldX, const float *Y, long long ldY, float *out,
                              int mode, void *stream_)
{
    sddmm_impl<float>(e, layout, X, ldX, Y, ldY, out, mode, stream_);
}

int crp_rp_spmm_sddmm_built(crp_rp_spmm_p e) { return (e && e->sd_built) ? 1 : 0; }

void crp_rp_spmm_exec_ex(crp_rp_spmm_p e, int BC_layout, const double *B, long long ldB, double *C,
                         long long ldC, void *stream_)
{
    exec_impl<double>(e, BC_layout, B, ldB, C, ldC, stream_);
}

void crp_rp_spmm_exec_f32_ex(crp_rp_spmm_p e, int BC_layout, const float *B, long long ldB, float *C, long long ldC,
                             void *stream_)
{
    exec_impl<float>(e, BC_layout, B, ldB, C, ldC, stream_);
}

void crp_rp_spmm_exec(crp_rp_spmm_p e, int BC_layout, const double *B, int ldB, double *C, int ldC)
{
    // The reference's entry point has no stream argument.  Host operands run on the engine's own (non-blocking)
    // stream.  Device operands were produced, and will be consumed, by work the caller enqueued somewhere the engine
    // cannot know -- by HIP's rules the null stream orders against that (every blocking stream, and the null stream
    // itself), the engine's non-blocking stream would not: device operands run on the null stream.
    void *s = e ? e->stream.h : NULL;
    if (e != NULL && !e->plan_only)
    {
        // (this fills the cache the exec below reads)
        const bool bd = on_device(B, &e->last_B, &e->last_B_dev), cd = on_device(C, &e->last_C, &e->last_C_dev);
        if (bd || cd) s = NULL;
    }
    crp_rp_spmm_exec_ex(e, BC_layout, B, (long long) ldB, C, (long long) ldC, s);
}

void crp_rp_spmm_print_stat(crp_rp_spmm_p e)
{
    if (e == NULL) return;
    const int n_exec = e->n_exec;
    if (n_exec == 0) return;
    uint64_t recv = (uint64_t) e->rB_recv_size, recv_max = 0, recv_sum = 0;
    double raw[7] = {e->t_init, e->t_pack, e->t_a2a, e->t_unpack, e->t_spmm, e->t_exec, e->t_a2a_host}, tmax[7], tavg[7];
    crp_comm_t *c = e->comm;
    c->reduce_u64(c->ctx, &recv, &recv_max, 1, CRP_OP_MAX);
    c->reduce_u64(c->ctx, &recv, &recv_sum, 1, CRP_OP_SUM);
    c->reduce_f64(c->ctx, raw, tmax, 7, CRP_OP_MAX);
    c->reduce_f64(c->ctx, raw, tavg, 7, CRP_OP_SUM);
    if (e->my_rank != 0) return;
    for (int i = 1; i <= 6; i++)
    {
        tmax[i] /= n_exec;
        tavg[i] /= ((double) n_exec * e->nproc);
    }
    recv_sum *= (uint64_t) e->glb_n;
    recv_max *= (uint64_t) e->glb_n;
    // same lines as src/rowpara_spmm.c:450-461 (harness scripts grep them)
    printf("rp_spmm_init() time = %.2f s\n", tmax[0]);
    printf("Total / rank-max SpMM comm size = %zu, %zu\n", (size_t) recv_sum, (size_t) recv_max);
    printf("-------------------- Runtime (s) --------------------\n");
    printf("                                     avg         max\n");
    printf("Pack B matrix for redistribution  %6.3f      %6.3f\n", tavg[1], tmax[1]);
    printf("Redistribute B matrix             %6.3f      %6.3f\n", tavg[2], tmax[2]);
    printf("Unpack received B matrix data     %6.3f      %6.3f\n", tavg[3], tmax[3]);
    printf("Local SpMM                        %6.3f      %6.3f\n", tavg[4], tmax[4]);
    printf("Total rp_spmm_exec()              %6.3f      %6.3f\n", tavg[5], tmax[5]);
    // additive to the reference's block: the device kernels finish in well under a millisecond
    printf("Local SpMM (us)                %9.1f   %9.1f\n", tavg[4] * 1e6, tmax[4] * 1e6);
    printf("Total rp_spmm_exec() (us)      %9.1f   %9.1f\n", tavg[5] * 1e6, tmax[5] * 1e6);
    if (e->nproc > 1) printf("Exchange call, host side (us)  %9.1f   %9.1f\n", tavg[6] * 1e6, tmax[6] * 1e6);
    printf("\n");
    fflush(stdout);
}

void crp_rp_spmm_clear_stat(crp_rp_spmm_p e)
{
    if (e == NULL) return;
    e->n_exec = 0;
    e->t_pack = e->t_a2a = e->t_unpack = e->t_spmm = e->t_exec = e->t_a2a_host = 0.0;
}

void crp_rp_spmm_get_plan(crp_rp_spmm_p e, crp_rp_plan_view_t *v)
{
    if (e == NULL || v == NULL) return;
    refresh_host_values(e);      // A_val is a public host field: device value updates left it behind
    v->nproc = e->nproc; v->my_rank = e->my_rank; v->glb_n = e->glb_n; v->A_nrow = e->A_nrow;
    v->rB_nrow = e->rB_nrow;
    v->rB_self_src_offset = e->rB_self_src_offset;
    v->rB_self_dst_offset = e->rB_self_dst_offset;
    v->rB_self_nrow = e->rB_self_nrow;
    v->rB_p2p = e->rB_p2p; v->rB_reidx = e->rB_reidx;
    v->A_rowptr = e->A_rowptr.data(); v->A_colidx = e->A_colidx.data(); v->A_val = e->A_val.data();
    v->rB_self_src_ridxs = e->rB_self_src_ridxs.data();
    v->rB_scnts = e->rB_scnts.data(); v->rB_sdispls = e->rB_sdispls.data(); v->rB_sridxs = e->rB_sridxs.data();
    v->rB_rcnts = e->rB_rcnts.data(); v->rB_rdispls = e->rB_rdispls.data(); v->rB_rridxs = e->rB_rridxs.data();
    v->rB_recv_size = e->rB_recv_size;
    v->n_exec = e->n_exec;
    v->t_init = e->t_init; v->t_pack = e->t_pack; v->t_a2a = e->t_a2a; v->t_unpack = e->t_unpack;
    v->t_spmm = e->t_spmm; v->t_exec = e->t_exec;
}

double crp_rp_spmm_exchange_host_seconds(crp_rp_spmm_p e) { return e ? e->t_a2a_host : -1.0; }

void crp_rp_spmm_update_values(crp_rp_spmm_p e, const double *A_val)
{
    if (e == NULL) return;
    const size_t nnz = e->A_val.size();
    if (nnz == 0) return;
    ASSERT_PRINTF(A_val != NULL, "rp_spmm_update_values: NULL values\n");
    memcpy(e->A_val.data(), A_val, sizeof(double) * nnz);
    e->host_vals_stale = false;  // (the engine's stream is already ordered after any device update)
    if (!e->plan_only)
    {
        if (e->exec_pending)        // kernels of an exec that returned asynchronously may still read the old values
        {
            HIP_OK(crp_stream_wait_event(e->stream, e->ev_exec));
            e->exec_pending = false;
        }
        if (e->A_int != nullptr)
        {
            for (int part = 0; part < 2; part++)
            {
                const std::vector<long long> &src = part == 0 ? e->int_src : e->bnd_src;
                if (src.empty()) continue;
                e->split_vals.resize(src.size());
                for (size_t t = 0; t < src.size(); t++) e->split_vals[t] = A_val[src[t]];
                HIP_OK(crp_csr_dev_update_values(part == 0 ? e->A_int : e->A_bnd, e->split_vals.data(), e->stream));
                HIP_OK(crp_stream_sync(e->stream));     // split_vals is reused by the next part
            }
        }
        else HIP_OK(crp_csr_dev_update_values(e->A_dev, A_val, e->stream));
        HIP_OK(crp_stream_sync(e->stream));
        if (e->t_built) update_transposed_values(e);
    }
}

// first device value update: the scratch regions and the event; the parts' positions when the engine is split
static void build_dev_update(crp_rp_spmm *e)
{
    e->dv_vals.alloc(e->A_val.size());
    e->ev_vals.ensure();
    upload_part_positions(e);
    e->dv_built = true;
}

void crp_rp_spmm_update_values_dev(crp_rp_spmm_p e, const void *A_val_dev, int f32, void *stream)
{
    if (e == NULL) return;
    check_call(e, "rp_spmm_update_values_dev");
    ASSERT_PRINTF(f32 == 0 || f32 == 1, "rp_spmm_update_values_dev: f32 must be 0 or 1\n");
    const size_t nnz = e->A_val.size();
    if (nnz == 0) return;
    ASSERT_PRINTF(A_val_dev != NULL, "rp_spmm_update_values_dev: NULL values\n");
    if (!e->dv_built) build_dev_update(e);
    if (e->t_built && e->dv_t_pos == nullptr)      // the first one after the transposed matrices were built: the second scratch region,
    {                                               // t_src on the device (nnz > 0 here: the pointer says "built")
        e->dv_tvals.alloc(nnz);
        e->dv_t_pos.upload(e->t_src.data(), nnz, e->stream);
    }
    void *s = stream;
    if (e->exec_pending)        // kernels of an exec that returned asynchronously may still read the old values
    {
        HIP_OK(crp_stream_wait_event(s, e->ev_exec));
        e->exec_pending = false;
    }
    if (e->dv_used) HIP_OK(crp_stream_wait_event(s, e->ev_vals));      // the scratch of an update on another stream
    auto gather = [&](size_t n, const int *map, double *dst) {
        if (f32) HIP_OK(crp_gather_vals_f32_f64((long long) n, map, (const float *) A_val_dev, dst, s));
        else HIP_OK(crp_gather_vals_f64((long long) n, map, (const double *) A_val_dev, dst, s));
    };
    if (e->A_int != nullptr)
    {
        const size_t n_int = e->int_src.size(), n_bnd = e->bnd_src.size();
        if (n_int > 0)
        {
            gather(n_int, e->sd_int_pos, e->dv_vals);
            HIP_OK(crp_csr_dev_update_values(e->A_int, e->dv_vals, s));
        }
        if (n_bnd > 0)
        {
            gather(n_bnd, e->sd_bnd_pos, e->dv_vals + n_int);
            HIP_OK(crp_csr_dev_update_values(e->A_bnd, e->dv_vals + n_int, s));
        }
    }
    else
    {
        gather(nnz, nullptr, e->dv_vals);       // widen or copy: the caller's buffer is free again when this has run
        HIP_OK(crp_csr_dev_update_values(e->A_dev, e->dv_vals, s));
    }
    if (e->t_built)
    {
        gather(nnz, e->dv_t_pos, e->dv_tvals);
        if (e->t_loc_nnz > 0) HIP_OK(crp_csr_dev_update_values(e->At_loc, e->dv_tvals, s));
        if (e->At_rem != nullptr && nnz > e->t_loc_nnz) HIP_OK(crp_csr_dev_update_values(e->At_rem, e->dv_tvals + e->t_loc_nnz, s));
    }
    HIP_OK(crp_event_record(e->ev_vals, s));
    if (s != e->stream) HIP_OK(crp_stream_wait_event(e->stream, e->ev_vals));
    e->dv_used = true;
    e->host_vals_stale = true;
}

// ---- row softmax over this rank's rows (crp_row_softmax_*): the values are the caller's, in A_val's order, so init's row pointer
// addresses them as it is, split engine or not
static bool row_softmax_ready(crp_rp_spmm *e, const char *what, int f32)
{
    crp::row_softmax_ready(what, e->plan_only, f32, true, e->sm_rowptr, e->A_rowptr, e->stream);
    return !e->A_val.empty();       // rows without a nonzero: nothing to launch, the pointers may be NULL
}

void crp_rp_spmm_row_softmax_ex(crp_rp_spmm_p e, const void *s, void *y, int f32, void *stream)
{
    if (e == NULL) return;
    if (!row_softmax_ready(e, "rp_spmm_row_softmax", f32)) return;
    ASSERT_PRINTF(s != NULL && y != NULL, "rp_spmm_row_softmax: NULL values\n");
    crp::row_softmax(e->A_nrow, e->sm_rowptr, f32, s, y, stream);
}

void crp_rp_spmm_row_softmax_bwd_ex(crp_rp_spmm_p e, const void *y, const void *dy, void *ds, int f32, void *stream)
{
    if (e == NULL) return;
    if (!row_softmax_ready(e, "rp_spmm_row_softmax_bwd", f32)) return;
    ASSERT_PRINTF(y != NULL && dy != NULL && ds != NULL, "rp_spmm_row_softmax_bwd: NULL values\n");
    crp::row_softmax_bwd(e->A_nrow, e->sm_rowptr, f32, y, dy, ds, stream);
}

int crp_rp_spmm_row_softmax_built(crp_rp_spmm_p e) { return (e && e->sm_rowptr) ? 1 : 0; }

int crp_rp_spmm_host_values_stale(crp_rp_spmm_p e) { return (e && e->host_vals_stale) ? 1 : 0; }

void crp_rp_spmm_overlap_rows(crp_rp_spmm_p e, int *n_interior, int *n_boundary)
{
    if (n_interior) *n_interior = (e && e->A_int) ? crp_csr_dev_nrow(e->A_int) : 0;
    if (n_boundary) *n_boundary = (e && e->A_bnd) ? crp_csr_dev_nrow(e->A_bnd) : 0;
}

void crp_rp_spmm_set_timing(crp_rp_spmm_p e, int timing) { if (e) e->timing = timing ? 1 : 0; }
int crp_rp_spmm_timing(crp_rp_spmm_p e) { return (e && e->timing) ? 1 : 0; }
void crp_rp_spmm_set_variant(crp_rp_spmm_p e, int variant) { if (e) e->variant = variant; }
void crp_rp_spmm_set_variant_f32(crp_rp_spmm_p e, int variant) { if (e) e->variant_f32 = variant; }

long long crp_rp_spmm_nnz(crp_rp_spmm_p e) { return e ? (long long) e->A_val.size() : -1; }

long long crp_rp_spmm_alg_bytes(crp_rp_spmm_p e)
{
    if (e == NULL) return -1;
    const long long nnz = (long long) e->A_val.size();
    return 12LL * nnz + 4LL * ((long long) e->A_nrow + 1) + 8LL * e->glb_n * e->n_needed_rows +
           8LL * e->glb_n * (long long) e->A_nrow;
}

long long crp_rp_spmm_alg_bytes_f32(crp_rp_spmm_p e)
{
    if (e == NULL) return -1;
    const long long nnz = (long long) e->A_val.size();
    return 8LL * nnz + 4LL * ((long long) e->A_nrow + 1) + 4LL * e->glb_n * e->n_needed_rows +
           4LL * e->glb_n * (long long) e->A_nrow;
}

// what the local kernel is for this engine's width: variant the auto choice resolves to (of the main device
// matrix, or of the interior part when the rows are split), whether its formats hold the rows in locality
// order, whether a stride lattice was found
void crp_rp_spmm_kernel_info(crp_rp_spmm_p e, int *variant, int *reordered, int *lattice)
{
    if (variant) *variant = -1;
    if (reordered) *reordered = 0;
    if (lattice) *lattice = 0;
    if (e == NULL) return;
    crp_csr_dev_p A = e->A_dev ? e->A_dev : e->A_int;
    if (A == NULL) return;
    // what the last exec launched (after alignment fallbacks); before the first exec, what auto would pick
    if (variant)
    {
        const int last = crp_csr_dev_last_variant(A);
        *variant = last > 0 ? last : (e->variant != 0 ? e->variant : crp_csr_dev_resolved_variant(A, e->glb_n));
    }
    if (reordered) *reordered = crp_csr_dev_reordered(A);
    if (lattice) *lattice = crp_csr_dev_lattice(A);
}

const int *crp_rp_spmm_dev_colidx_host(crp_rp_spmm_p e) { return e ? e->dev_colidx_host.data() : NULL; }

// ---------------------------------------------------------------------------
// single-rank communicator
static void self_a2a(void *, const int *s, int *r, int count) { memcpy(r, s, sizeof(int) * (size_t) count); }
static void self_a2av(void *, const int *s, const int *sc, const int *sd, int *r, const int *, const int *rd)
{
    memcpy(r + rd[0], s + sd[0], sizeof(int) * (size_t) sc[0]);
}
static void self_agv(void *, const void *s, size_t sb, void *r, const size_t *, const size_t *rd)
{
    memcpy((char *) r + rd[0], s, sb);
}
static void self_barrier(void *) {}
static void self_red_f64(void *, const double *in, double *out, int n, int) { memcpy(out, in, sizeof(double) * (size_t) n); }
static void self_red_u64(void *, const uint64_t *in, uint64_t *out, int n, int) { memcpy(out, in, sizeof(uint64_t) * (size_t) n); }
static void self_a2av_dev(void *, const double *, const long long *, const long long *, double *, const long long *,
                          const long long *, void *) {}
static void self_a2av_bytes(void *, const void *s, const size_t *sc, const size_t *sd, void *r, const size_t *,
                            const size_t *rd)
{
    memcpy((char *) r + rd[0], (const char *) s + sd[0], sc[0]);
}
static void self_free(crp_comm_t *c) { free(c); }
static crp_comm_t *self_split(void *, int, int) { return crp_comm_self(); }

crp_comm_t *crp_comm_self(void)
{
    crp_comm_t *c = (crp_comm_t *) calloc(1, sizeof(crp_comm_t));
    c->nproc = 1;
    c->rank = 0;
    c->alltoall_i32 = self_a2a;
    c->alltoallv_i32 = self_a2av;
    c->allgatherv_bytes = self_agv;
    c->barrier = self_barrier;
    c->reduce_f64 = self_red_f64;
    c->reduce_u64 = self_red_u64;
    c->alltoallv_dev_f64 = self_a2av_dev;
    c->alltoallv_bytes = self_a2av_bytes;
    c->split = self_split;
    c->free = self_free;
    return c;
}

}  // extern "C"
