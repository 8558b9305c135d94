// rp_engine.cpp -- the 1D row-parallel SpMM engine (include/crp_engine.h).
//
// Host side of /root/reference/src/rowpara_spmm.c re-thought for a device-
// resident data path:
//   init  (reference :20-190): one pass builds the needed-row flags, a prefix
//         rank array gives the compact ids, the needs are exchanged through the
//         communicator's alltoall(v); A is uploaded once with a two-source column
//         index (local B row | row of the receive buffer), so exec never copies
//         locally owned B rows and never unpacks.
//   exec  (reference :212-422): gather kernel -> device all-to-all -> SpMM kernel
//         on one stream; no allocation, no sparse-handle creation.
// Public plan fields keep the reference's meaning (crp_rp_plan_view_t).
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "crp_engine.h"
#include "crpspmm_hip.h"
#include "utils.h"
#include "operand_view.h"
#include "par.h"
#include <algorithm>

struct crp_rp_spmm
{
    // ---- plan, reference field names (src/rowpara_spmm.h:8-40)
    int nproc = 1, my_rank = 0, glb_n = 0, A_nrow = 0, rB_nrow = 0;
    int rB_self_src_offset = 0, rB_self_dst_offset = 0, rB_self_nrow = 0;
    int rB_p2p = 1, rB_reidx = 1;
    std::vector<int>       A_rowptr, A_colidx;
    std::vector<double>    A_val;
    std::vector<int>       rB_self_src_ridxs, rB_sridxs, rB_rridxs;
    std::vector<long long> rB_scnts, rB_sdispls, rB_rcnts, rB_rdispls;
    size_t rB_recv_size = 0;
    int    n_exec = 0;
    double t_init = 0, t_pack = 0, t_a2a = 0, t_unpack = 0, t_spmm = 0, t_exec = 0;
    bool vals_from_device = false;   // the device matrices took their values from a device copy (no second upload)
    double t_a2a_host = 0;           // host time inside the exchange CALL (issuing the sends / receives), whatever the timing mode
    crp_comm_t *comm = nullptr;

    // ---- device side.  Every device resource is a member that releases itself (dev_owned.h) and crp_rp_spmm_free is `delete`:
    // members go in REVERSE order of declaration, so the streams come first here, then the events, then the matrices and buffers
    // -- those are released before the events, and the events before the streams, as the hand-written free did.  A plan-only
    // engine holds empty owners only: its delete calls nothing on the device.
    bool plan_only = false;
    int  timing = 1, variant = 0;
    int  variant_f32 = 0;                        // the fp32 exec's kernel variant (crp_spmm_csr_f32: 0, 1, 5)
    int  loc_B_nrow = 0;
    long long n_send_rows = 0, n_recv_rows = 0, n_needed_rows = 0;
    std::vector<int> dev_colidx_host;
    crp::DevStream stream;                       // the engine's own stream
    crp::DevStream xstream;                      // the exchange's (nproc > 1: a split engine, or the first exec_t)
    // ev_exec: the end of the last exec that returned asynchronously -- a value update on the engine's own stream must not overtake
    // kernels of an exec that is still in flight on the caller's stream; ev_packed / ev_landed: with xstream; ev_vals: recorded at
    // the end of every device value update
    crp::DevEvent ev_exec, ev_landed, ev_packed, ev_vals;
    bool exec_pending = false;
    // staging (host-pointer API) and column-major temporaries, grown on demand
    crp::DevScratch C_rm, B_rm, C_stage, B_stage;
    // the forward exchange; the fp32 one is set up by the first fp32 exec: rows of round_up(glb_n, 4) floats, counts in 8-byte words
    crp::DevArray<float>  recvbuf32_dev, sendbuf32_dev;
    crp::DevArray<double> recvbuf_dev, sendbuf_dev;
    crp::DevArray<int>    sridxs_dev;
    bool x32_ready = false;
    std::vector<long long> x32_scnts, x32_sdispls, x32_rcnts, x32_rdispls;
    // fused attention (crp_rp_spmm_attention_ex), allocated by its first call of a dtype: the receive buffer of V's rows -- K's land
    // in the forward exchange's -- and the scratch of host operands (Q, V, lse; a host p_out takes sd_out)
    bool at_built = false, at_ready64 = false, at_ready32 = false;
    crp::DevScratch at_lse, V_rm, V_stage, Q_rm, Q_stage;
    crp::DevArray<float>  at_recv32_dev;
    crp::DevArray<double> at_recv_dev;
    // row softmax (crp_rp_spmm_row_softmax_ex), uploaded by its first call: A_rowptr as a device array
    crp::DevArray<int> sm_rowptr;
    // device value updates (crp_rp_spmm_update_values_dev), allocated by its first call: the new values as fp64 in the order the
    // device matrices take them (A_dev: A_val's order; a split engine: A_int's nonzeros, then A_bnd's) and, once the transposed
    // matrices exist, in theirs (through dv_t_pos, a device copy of t_src)
    bool dv_built = false, dv_used = false;
    crp::DevArray<int>    dv_t_pos;
    crp::DevArray<double> dv_tvals, dv_vals;
    bool host_vals_stale = false;                // A_val (host) is behind the device matrices: refreshed where it is read
    // SDDMM (crp_rp_spmm_sddmm_ex), uploaded by its first call: where the nonzeros of A_int / A_bnd sit in A_val (int_src / bnd_src
    // as int32 device arrays; none for the unsplit engine), and the staging buffer of a host `out`
    bool sd_built = false;
    crp::DevScratch sd_out;
    crp::DevArray<int> sd_bnd_pos, sd_int_pos;
    // transposed product (crp_rp_spmm_exec_t_ex), built by its first call: the transpose of the two-source local matrix cut by
    // rows -- At_loc writes this rank's C block, At_rem the rows owed to peers (into recvbuf_dev, in the forward plan's peer order)
    bool t_built = false;
    std::vector<int> t_src;                      // position in A_val of every nonzero of At_loc, then of At_rem
    size_t t_loc_nnz = 0;
    // the rows that come back (one per row this rank sends in the forward exchange), grouped by the C row they add to:
    // acc_dev = rows[n_acc] | ptr[n_acc + 1] | positions in sendbuf_dev[n_send_rows], ascending inside a group
    int  n_acc = 0;
    crp::DevArray<int> acc_dev;
    crp::DevCsr At_rem, At_loc;
    // exchange / compute overlap (nproc > 1): rows with no remote column ("interior") run while the
    // B rows travel, the rest ("boundary") after they have landed; A_dev then stays unset
    std::vector<long long> int_src, bnd_src;     // position in A_val of every nonzero of the two parts
    std::vector<double>    split_vals;
    crp::DevCsr A_bnd, A_int, A_dev;
    // last operands seen and where they live (the pointer-attribute query is not free); not owned
    const void *last_B = nullptr, *last_C = nullptr;
    int last_B_dev = 0, last_C_dev = 0;
};

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

// ---- what the fp64 and the fp32 exec do differently: kernels, variant, exchange buffers -----------------------------
// The fp32 exec packs rows of ld32 = round_up(n, 4) floats (16-byte rows for the packing kernel and for the team kernel's
// second B source) and carries them through the communicator's fp64 all-to-all as opaque 8-byte words: no back end does
// arithmetic on the payload, so crp_comm_t stays as it is.
static long long ld32_of(int n) { return ((long long) n + 3) / 4 * 4; }

struct Xchg
{
    void *send, *recv;                            // packed rows of ld elements
    long long ld;
    const long long *sc, *sd, *rc, *rd;           // counts / displacements in 8-byte words, as alltoallv_dev_f64 takes them
};

static Xchg exchange_of(crp_rp_spmm *e, const double *)
{
    return Xchg{e->sendbuf_dev, e->recvbuf_dev, (long long) e->glb_n, e->rB_scnts.data(), e->rB_sdispls.data(),
                e->rB_rcnts.data(), e->rB_rdispls.data()};
}

// first fp32 exec: word counts (rows * ld32 / 2) and the fp32 exchange buffers
static Xchg exchange_of(crp_rp_spmm *e, const float *)
{
    const long long ld = ld32_of(e->glb_n);
    if (!e->x32_ready)
    {
        const long long n = e->glb_n;     // rB_* hold rows * glb_n elements
        auto words = [&](const std::vector<long long> &v, std::vector<long long> &out) {
            out.resize(v.size());
            for (size_t q = 0; q < v.size(); q++) out[q] = n > 0 ? v[q] / n * ld / 2 : 0;
        };
        words(e->rB_scnts, e->x32_scnts);
        words(e->rB_sdispls, e->x32_sdispls);
        words(e->rB_rcnts, e->x32_rcnts);
        words(e->rB_rdispls, e->x32_rdispls);
        // the pad columns are zeroed here and never written again: no uninitialised byte crosses a link
        if (e->n_send_rows > 0 && ld > 0) e->sendbuf32_dev.zeroed((size_t) e->n_send_rows * (size_t) ld);
        if (e->n_recv_rows > 0 && ld > 0) e->recvbuf32_dev.zeroed((size_t) e->n_recv_rows * (size_t) ld);
        e->x32_ready = true;
    }
    return Xchg{e->sendbuf32_dev, e->recvbuf32_dev, ld, e->x32_scnts.data(), e->x32_sdispls.data(), e->x32_rcnts.data(),
                e->x32_rdispls.data()};
}

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

// Is this pointer on the device?  The pointer-attribute query is not free: the forward exec passes the engine's cache of the last
// operand seen in that place (last, last_dev), the other calls ask every time (last == nullptr).
static bool on_device(const void *p, const void **last = nullptr, int *last_dev = nullptr)
{
    if (last != nullptr && p == *last && p != NULL) return *last_dev != 0;
    int dev = 0;
    HIP_OK(crp_dev_ptr_is_device(p, &dev));
    if (last != nullptr)
    {
        *last = p;
        *last_dev = dev;
    }
    return dev != 0;
}

// The end of an exec, exec_t or sddmm that has not synchronised yet: wait for the stream when an operand lives on the host or the
// phases are timed, otherwise return asynchronously and remember where the call ends (crp_rp_spmm_update_values waits for it).
static void complete(crp_rp_spmm *e, void *s, bool synced, bool must_sync)
{
    if (synced) return;
    if (must_sync)
    {
        HIP_OK(crp_stream_sync(s));
        return;
    }
    HIP_OK(crp_event_record(e->ev_exec.ensure(), s));
    e->exec_pending = true;
}

// ---- the pieces pack_exchange_run and pack_exchange_run2 share ---------------------------------------------------------------------
// pack the rows of the row-major device operand Bd that other ranks asked for into x.send, on st (reference :232-262)
template <class T>
static void pack_rows(crp_rp_spmm *e, const Xchg &x, const T *Bd, long long ldBd, void *st)
{
    if (e->n_send_rows > 0 && e->glb_n > 0) HIP_OK(crp::gather((int) e->n_send_rows, e->glb_n, e->sridxs_dev, Bd, ldBd, (T *) x.send, x.ld, st));
}

// the exchange call on st (reference :275-309), its host time billed to t_a2a_host; the received rows land in recv in final order
static void exchange_rows(crp_rp_spmm *e, const Xchg &x, void *recv, void *st)
{
    const double tx0 = get_wtime_sec();
    e->comm->alltoallv_dev_f64(e->comm->ctx, (const double *) x.send, x.sc, x.sd, (double *) recv, x.rc, x.rd, st);
    e->t_a2a_host += get_wtime_sec() - tx0;
}

// with timing on: wait for s and bill the time since t0 to *bucket
static void lap(crp_rp_spmm *e, void *s, double &t0, double *bucket)
{
    if (!e->timing) return;
    HIP_OK(crp_stream_sync(s));
    const double t1 = get_wtime_sec();
    *bucket += t1 - t0;
    t0 = t1;
}

// the local kernels after the exchange (reference :388-408): product(A, part) once for A_dev (part 0), or for A_int (1) and A_bnd (2)
template <class F>
static void run_parts(crp_rp_spmm *e, F &&product)
{
    if (e->A_int != nullptr)
    {
        product(e->A_int, 1);
        product(e->A_bnd, 2);
    }
    else product(e->A_dev, 0);
}

// The half that exec and sddmm share: pack the rows of the row-major device operand Bd that other ranks asked for, exchange them
// (the received rows land in x.recv in final order), and run the local kernels.  With timing off and a split engine the interior
// part is enqueued on s beside the exchange, which runs on the engine's second stream, and the boundary part after the rows have
// landed; with timing on the phases run in sequence and bill to t_pack and t_a2a (t0 is left at the start of the kernels, which
// the caller bills).
template <class T, class F>
static void pack_exchange_run(crp_rp_spmm *e, const Xchg &x, const T *Bd, long long ldBd, void *s, double &t0, F &&product)
{
    const bool timing = e->timing != 0;
    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    pack_rows(e, x, Bd, ldBd, s);
    lap(e, s, t0, &e->t_pack);
    if (e->A_int != nullptr && !timing)
    {
        // The exchange runs on its own stream beside the interior rows' product.  The product is ENQUEUED FIRST: it does not
        // depend on the exchange, and issuing a group of sends / receives can hold the host for a while (a non-blocking RCCL
        // communicator is polled until the group is on the stream) -- with the exchange first, the whole interior product
        // (0.06 - 0.2 ms per GPU at pwtk size) could have passed before its launch was even issued.
        HIP_OK(crp_event_record(e->ev_packed, s));
        product(e->A_int, 1);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        exchange_rows(e, x, x.recv, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        product(e->A_bnd, 2);
        return;
    }
    if (e->nproc > 1) exchange_rows(e, x, x.recv, s);
    lap(e, s, t0, &e->t_a2a);
    run_parts(e, product);
}

// C := A * B on this rank, one dtype (crp_rp_spmm_exec_ex / crp_rp_spmm_exec_f32_ex)
template <class T>
static void exec_impl(crp_rp_spmm *e, int BC_layout, const T *B, long long ldB, T *C, long long ldC, void *stream_)
{
    if (e == NULL) return;
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_exec on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(BC_layout == 0 || BC_layout == 1, "BC_layout must be 0 or 1\n");
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
    pack_exchange_run(e, x, Bv.p, Bv.ld, s, t0, [&](crp_csr_dev_p A, int) { HIP_OK(spmm(e, A, n, Bv.p, Bv.ld, (const T *) x.recv, x.ld, Cv.p, Cv.ld, s)); });
    const bool synced = crp::finish(Cv, s, [&] { lap(e, s, t0, &e->t_spmm); });
    complete(e, s, synced, !B_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

// ---- out[p] = < X[row(p)], Y[col(p)] > over this rank's rows of A (crp_rp_spmm_sddmm_ex / _f32_ex) --------------------------------
// int_src / bnd_src of a split engine as int32 device arrays: the SDDMM's parts write through them into the order of A_val, a
// device value update gathers the parts' values through them; whichever call comes first uploads
static void upload_part_positions(crp_rp_spmm *e)
{
    auto up = [&](const std::vector<long long> &src, crp::DevArray<int> &dst) {
        if (src.empty() || dst != nullptr) return;
        std::vector<int> pos(src.begin(), src.end());          // (positions in A_val: below 2^31, as A_rowptr is int)
        dst.upload(pos.data(), pos.size(), e->stream);
    };
    if (e->A_int != nullptr)
    {
        up(e->int_src, e->sd_int_pos);
        up(e->bnd_src, e->sd_bnd_pos);
    }
}

// A_val (host) after device value updates: one blocking download of the values as the device matrices took them.  The engine's
// stream is ordered after every device update (crp_rp_spmm_update_values_dev), so the copy runs there.
static void refresh_host_values(crp_rp_spmm *e)
{
    if (!e->host_vals_stale) return;
    const size_t nnz = e->A_val.size();
    if (e->A_int != nullptr)
    {
        e->split_vals.resize(nnz);
        HIP_OK(crp_dev_memcpy(e->split_vals.data(), e->dv_vals, sizeof(double) * nnz, 1, e->stream));
        HIP_OK(crp_stream_sync(e->stream));
        const size_t n_int = e->int_src.size();
        for (size_t t = 0; t < n_int; t++) e->A_val[(size_t) e->int_src[t]] = e->split_vals[t];
        for (size_t t = 0; t < e->bnd_src.size(); t++) e->A_val[(size_t) e->bnd_src[t]] = e->split_vals[n_int + t];
    }
    else
    {
        HIP_OK(crp_dev_memcpy(e->A_val.data(), e->dv_vals, sizeof(double) * nnz, 1, e->stream));
        HIP_OK(crp_stream_sync(e->stream));
    }
    e->host_vals_stale = false;
}

template <class T>
static void sddmm_impl(crp_rp_spmm *e, int layout, const T *X, long long ldX, const T *Y, long long ldY, T *out, int mode, void *stream_)
{
    if (e == NULL) return;
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_sddmm on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(layout == 0 || layout == 1, "layout must be 0 or 1\n");
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

    const bool X_on_dev = on_device(X), Y_on_dev = on_device(Y), out_on_dev = on_device(out);

    // ---- operands as device-resident row-major views: Y takes B's buffers, X takes C's
    const Xchg x = exchange_of(e, Y);
    const crp::InView<T> Yv = crp::operand_in(layout, Y, ldY, kb, n, Y_on_dev, e->B_stage, e->B_rm, s);
    const crp::InView<T> Xv = crp::operand_in(layout, X, ldX, m, n, X_on_dev, e->C_stage, e->C_rm, s);
    T *outd = out;
    if (!out_on_dev && nnz > 0) outd = e->sd_out.grow<T>(nnz);

    if (n == 0 && nnz > 0) HIP_OK(crp_dev_memset(outd, 0, nnz * sizeof(T), s));      // empty dots

    // ---- pack Y, exchange, the kernels: the parts of a split engine write through their positions in A_val
    pack_exchange_run(e, x, Yv.p, Yv.ld, s, t0, [&](crp_csr_dev_p A, int part) {
        if (n == 0 || crp_csr_dev_nnz(A) == 0) return;
        const int *pos = part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
        HIP_OK(crp::sddmm(A, n, Xv.p, Xv.ld, Yv.p, Yv.ld, (const T *) x.recv, x.ld, outd, pos, mode, s));
    });
    lap(e, s, t0, &e->t_spmm);

    const bool download = !out_on_dev && nnz > 0;
    if (download) HIP_OK(crp_dev_memcpy(out, outd, nnz * sizeof(T), 1, s));
    complete(e, s, false, download || !X_on_dev || !Y_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

// ---- O = softmax_row(scale (Q K^T)|pattern(A) (+ A's values)) V over this rank's rows of A (crp_rp_spmm_attention_ex / _f32_ex) ----
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

// pack_exchange_run for two operands partitioned like B: the rows of Kd travel into x.recv, then those of Vd into recv2, both
// through x.send, which is reused in stream order.  With timing off and a split engine the interior part is enqueued on s first and
// both packs and both exchanges run beside it on the engine's second stream, from the point of s where the operands are ready; the
// boundary part follows on s after the second exchange has landed.  Otherwise everything runs on s in sequence and, with timing
// on, bills to t_pack and t_a2a (t0 is left at the start of the kernels).
template <class T, class F>
static void pack_exchange_run2(crp_rp_spmm *e, const Xchg &x, void *recv2, const T *Kd, long long ldKd, const T *Vd, long long ldVd, void *s,
                               double &t0, F &&product)
{
    const bool timing = e->timing != 0;
    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->A_int != nullptr && !timing)
    {
        HIP_OK(crp_event_record(e->ev_packed, s));          // (here: the operands are ready)
        product(e->A_int, 1);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        pack_rows(e, x, Kd, ldKd, e->xstream);
        exchange_rows(e, x, x.recv, e->xstream);
        pack_rows(e, x, Vd, ldVd, e->xstream);
        exchange_rows(e, x, recv2, e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        product(e->A_bnd, 2);
        return;
    }
    for (int op = 0; op < 2; op++)
    {
        pack_rows(e, x, op == 0 ? Kd : Vd, op == 0 ? ldKd : ldVd, s);
        lap(e, s, t0, &e->t_pack);
        if (e->nproc > 1) exchange_rows(e, x, op == 0 ? x.recv : recv2, s);
        lap(e, s, t0, &e->t_a2a);
    }
    run_parts(e, product);
}

template <class T>
static void attention_impl(crp_rp_spmm *e, int layout, double scale, int bias, const T *Q, long long ldQ, const T *K, long long ldK,
                           const T *V, long long ldV, T *O, long long ldO, T *lse, T *p_out, void *stream_)
{
    if (e == NULL) return;
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_attention on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(layout == 0 || layout == 1, "layout must be 0 or 1\n");
    ASSERT_PRINTF(bias == 0 || bias == 1, "bias must be 0 or 1\n");
    ASSERT_PRINTF(scale - scale == 0.0, "scale must be finite\n");
    const double t_begin = get_wtime_sec();
    void *s = stream_;
    const int n = e->glb_n, kb = e->loc_B_nrow, m = e->A_nrow;
    const size_t nnz = e->A_val.size();
    const bool timing = e->timing != 0;
    double t0;

    const bool Q_on_dev = on_device(Q), K_on_dev = on_device(K), V_on_dev = on_device(V), O_on_dev = on_device(O);
    const bool lse_host = lse != NULL && m > 0 && !on_device(lse), p_host = p_out != NULL && nnz > 0 && !on_device(p_out);

    // ---- operands as device-resident row-major views: K takes B's buffers and the forward exchange, O takes C's
    const Xchg x = exchange_of(e, K);
    T *recv2 = attention_recv(e, x, K);
    const crp::InView<T> Kv = crp::operand_in(layout, K, ldK, kb, n, K_on_dev, e->B_stage, e->B_rm, s);
    const crp::InView<T> Vv = crp::operand_in(layout, V, ldV, kb, n, V_on_dev, e->V_stage, e->V_rm, s);
    const crp::InView<T> Qv = crp::operand_in(layout, Q, ldQ, m, n, Q_on_dev, e->Q_stage, e->Q_rm, s);
    const crp::OutView<T> Ov = crp::operand_out(layout, O, ldO, m, n, O_on_dev, e->C_stage, e->C_rm);
    T *lsed = lse_host ? e->at_lse.grow<T>((size_t) m) : lse;
    T *pd = p_host ? e->sd_out.grow<T>(nnz) : p_out;

    // ---- pack and exchange K, then V; the kernels: the parts of a split engine write O and lse through their row maps and p_out
    // through their positions in A_val
    pack_exchange_run2(e, x, recv2, Kv.p, Kv.ld, Vv.p, Vv.ld, s, t0, [&](crp_csr_dev_p A, int part) {
        if (n == 0 || crp_csr_dev_nrow(A) == 0) return;
        const int *pos = part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
        HIP_OK(crp::attention(A, n, scale, bias, Qv.p, Qv.ld, Kv.p, Kv.ld, (const T *) x.recv, x.ld, Vv.p, Vv.ld, (const T *) recv2, x.ld, Ov.p,
                         Ov.ld, lsed, pd, pos, s));
    });
    if (lse_host) HIP_OK(crp_dev_memcpy(lse, lsed, (size_t) m * sizeof(T), 1, s));
    if (p_host) HIP_OK(crp_dev_memcpy(p_out, pd, nnz * sizeof(T), 1, s));
    const bool synced = crp::finish(Ov, s, [&] { lap(e, s, t0, &e->t_spmm); });
    complete(e, s, synced, lse_host || p_host || !Q_on_dev || !K_on_dev || !V_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

// ---- C := A^T * B (crp_rp_spmm_exec_t_ex) --------------------------------------------------------------------------------------
// First call: the two-source local matrix, its remote columns renumbered behind the local ones, is transposed on the device
// (crp_csr_transpose) and cut by rows into At_loc and At_rem; the rows that come back are grouped by the C row they add to.
static void build_transposed(crp_rp_spmm *e)
{
    refresh_host_values(e);
    const int m = e->A_nrow, kb = e->loc_B_nrow, nr = (int) e->n_recv_rows;
    const long long ncol_ll = (long long) kb + nr;
    ASSERT_PRINTF(ncol_ll < INT_MAX, "rp_spmm_exec_t: %lld local + received rows pass the 32-bit row index\n", ncol_ll);
    const int ncol = (int) ncol_ll;
    const size_t nnz = e->A_val.size(), n1 = nnz > 0 ? nnz : 1;
    std::vector<int> col(n1, 0), rp_t((size_t) ncol + 1, 0), ci_t(n1, 0);
    std::vector<double> va_t(n1, 0.0);
    e->t_src.assign(n1, 0);
    for (size_t p = 0; p < nnz; p++)
    {
        const int c = e->dev_colidx_host[p];
        col[p] = c >= 0 ? c : kb + ~c;
    }
    {
        // device temporaries: val | val_t | rowptr | rowptr_t | col | col_t | tmap
        const size_t vb = sizeof(double) * n1, ib = sizeof(int) * n1, rb = sizeof(int) * ((size_t) m + 1), tb = sizeof(int) * ((size_t) ncol + 1);
        crp::DevArray<char> tmp;
        char *b = tmp.alloc(2 * vb + rb + tb + 3 * ib);
        double *d_val = (double *) b, *d_val_t = (double *) (b + vb);
        int *d_rp = (int *) (b + 2 * vb), *d_rp_t = (int *) (b + 2 * vb + rb), *d_col = (int *) (b + 2 * vb + rb + tb), *d_col_t = d_col + n1,
            *d_tmap = d_col_t + n1;
        HIP_OK(crp_dev_memcpy(d_rp, e->A_rowptr.data(), rb, 0, e->stream));
        HIP_OK(crp_dev_memcpy(d_col, col.data(), ib, 0, e->stream));
        HIP_OK(crp_dev_memcpy(d_val, nnz > 0 ? e->A_val.data() : va_t.data(), vb, 0, e->stream));
        HIP_OK(crp_csr_transpose(m, ncol, d_rp, d_col, d_val, d_rp_t, d_col_t, d_val_t, d_tmap, e->stream));
        HIP_OK(crp_dev_memcpy(rp_t.data(), d_rp_t, tb, 1, e->stream));
        HIP_OK(crp_dev_memcpy(ci_t.data(), d_col_t, ib, 1, e->stream));
        HIP_OK(crp_dev_memcpy(va_t.data(), d_val_t, vb, 1, e->stream));
        HIP_OK(crp_dev_memcpy(e->t_src.data(), d_tmap, ib, 1, e->stream));
        HIP_OK(crp_stream_sync(e->stream));
    }
    e->t_loc_nnz = (size_t) rp_t[(size_t) kb];
    HIP_OK(crp_csr_dev_create(kb, m, rp_t.data(), ci_t.data(), va_t.data(), e->At_loc.out()));
    if (nr > 0)
    {
        std::vector<int> rp_r((size_t) nr + 1);
        for (int i = 0; i <= nr; i++) rp_r[(size_t) i] = rp_t[(size_t) kb + (size_t) i] - (int) e->t_loc_nnz;
        // (an empty part still gets valid pointers: the arrays hold at least one element)
        const size_t off = e->t_loc_nnz < n1 ? e->t_loc_nnz : 0;
        HIP_OK(crp_csr_dev_create(nr, m, rp_r.data(), ci_t.data() + off, va_t.data() + off, e->At_rem.out()));
    }
    if (e->n_send_rows > 0)
    {
        // incoming position q adds to C row rB_sridxs[q]: a row several peers asked for comes back several times
        const size_t ns = (size_t) e->n_send_rows;
        std::vector<int> cnt((size_t) kb + 1, 0);
        for (size_t q = 0; q < ns; q++) cnt[(size_t) e->rB_sridxs[q] + 1]++;
        std::vector<int> rows, ptr(1, 0), start((size_t) kb, 0);
        for (int r = 0; r < kb; r++)
            if (cnt[(size_t) r + 1] > 0)
            {
                start[(size_t) r] = ptr.back();
                rows.push_back(r);
                ptr.push_back(ptr.back() + cnt[(size_t) r + 1]);
            }
        std::vector<int> pos(ns);
        for (size_t q = 0; q < ns; q++) pos[(size_t) start[(size_t) e->rB_sridxs[q]]++] = (int) q;       // (ascending q inside a group)
        e->n_acc = (int) rows.size();
        std::vector<int> all(rows);
        all.insert(all.end(), ptr.begin(), ptr.end());
        all.insert(all.end(), pos.begin(), pos.end());
        e->acc_dev.upload(all.data(), all.size(), e->stream);
    }
    if (e->nproc > 1)
    {
        e->xstream.ensure();
        e->ev_packed.ensure();
        e->ev_landed.ensure();
    }
    e->t_built = true;
}

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
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_exec_t on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(BC_layout == 0 || BC_layout == 1, "BC_layout must be 0 or 1\n");
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

    auto reverse_exchange = [&](void *xs) {
        // the forward plan backwards: what this rank receives there it sends here, from the receive into the send buffer
        const double tx0 = get_wtime_sec();
        e->comm->alltoallv_dev_f64(e->comm->ctx, (const double *) x.recv, x.rc, x.rd, (double *) x.send, x.sc, x.sd, xs);
        e->t_a2a_host += get_wtime_sec() - tx0;
    };
    auto product = [&](crp_csr_dev_p A, T *out, long long ldo) { HIP_OK(spmm(e, A, n, Bv.p, Bv.ld, (const T *) NULL, 0, out, ldo, s)); };
    auto accumulate = [&]() {
        if (e->n_acc == 0 || n == 0) return;
        const int *acc_row = e->acc_dev, *acc_ptr = acc_row + e->n_acc, *acc_pos = acc_ptr + e->n_acc + 1;
        HIP_OK(crp::scatter_add(e->n_acc, n, acc_row, acc_ptr, acc_pos, (const T *) x.send, x.ld, Cv.p, Cv.ld, s));
    };

    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->nproc > 1 && !timing)
    {
        // the exchange on its own stream beside the local product, which is enqueued first (see exec_impl)
        if (e->At_rem != nullptr) product(e->At_rem, (T *) x.recv, x.ld);
        HIP_OK(crp_event_record(e->ev_packed, s));
        product(e->At_loc, Cv.p, Cv.ld);
        HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
        reverse_exchange(e->xstream);
        HIP_OK(crp_event_record(e->ev_landed, e->xstream));
        HIP_OK(crp_stream_wait_event(s, e->ev_landed));
        accumulate();
    }
    else
    {
        if (e->At_rem != nullptr) product(e->At_rem, (T *) x.recv, x.ld);
        lap(e, s, t0, &e->t_spmm);
        if (e->nproc > 1) reverse_exchange(s);
        lap(e, s, t0, &e->t_a2a);
        product(e->At_loc, Cv.p, Cv.ld);
        lap(e, s, t0, &e->t_spmm);
        accumulate();
        lap(e, s, t0, &e->t_unpack);
    }
    const bool synced = crp::finish(Cv, s, [&] { lap(e, s, t0, &e->t_spmm); });
    complete(e, s, synced, !B_on_dev || timing);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
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

void crp_rp_spmm_attention_ex(crp_rp_spmm_p e, int layout, double scale, int bias, const double *Q, long long ldQ, const double *K,
                              long long ldK, const double *V, long long ldV, double *O, long long ldO, double *lse, double *p_out,
                              void *stream_)
{
    attention_impl<double>(e, layout, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream_);
}

void crp_rp_spmm_attention_f32_ex(crp_rp_spmm_p e, int layout, double scale, int bias, const float *Q, long long ldQ, const float *K,
                                  long long ldK, const float *V, long long ldV, float *O, long long ldO, float *lse, float *p_out,
                                  void *stream_)
{
    attention_impl<float>(e, layout, scale, bias, Q, ldQ, K, ldK, V, ldV, O, ldO, lse, p_out, stream_);
}

int crp_rp_spmm_attention_built(crp_rp_spmm_p e) { return (e && e->at_built) ? 1 : 0; }

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
    ASSERT_PRINTF(!e->plan_only, "rp_spmm_update_values_dev on a plan-only engine (no device state)\n");
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
