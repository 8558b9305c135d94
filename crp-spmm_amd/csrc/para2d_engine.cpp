// para2d_engine.cpp -- the 2D (pm x pn) engine (include/crp_engine.h).
//
// Follows /root/reference/src/para2d_spmm.c:20-205: rank r sits at
// (pi, pj) = (r / pn, r % pn); the pn ranks of a grid row pool their A0 slices
// into the row panel AC_rowptr[pi] .. AC_rowptr[pi+1] (one-time replication,
// reference :56-98), then a 1D row-parallel engine runs inside each grid
// column on the BC_colptr[pj] .. BC_colptr[pj+1] columns of B and C.
// The panel's column indices and values are all-gathered between DEVICE buffers when the communicator
// offers allgatherv_dev (RCCL), on the host through allgatherv_bytes otherwise; the replication-cost statistic is
// computed without the reference's rank (P-1) -> rank 0 message, which
// deadlocks at one rank (reference :102-109).
//
// Beyond A*B the engine offers what the row engine offers on the panel: new values (update_values: the slices' values
// all-gathered along the grid row into panel order), C := A^T*B (a forward) and SDDMM, whose dots over all n columns are the
// sum of the grid row's partial dots over their column slices: a reduce-scatter along the grid row (the panel being the
// concatenation of the row's slices in rank order, every rank's share is one contiguous run) and crp_sum_segments_*.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "crp_engine.h"
#include "crpspmm_hip.h"
#include "utils.h"
#include "dtype_calls.h"       // HIP_OK, the owners (dev_owned.h), sum_segments, inner_sddmm, the row softmax
#include "knobs.h"

// the inner row engine, released with crp_rp_spmm_free
struct RpEngine
{
    crp_rp_spmm_p p = nullptr;
    RpEngine() = default;
    RpEngine(const RpEngine &) = delete;
    RpEngine &operator=(const RpEngine &) = delete;
    ~RpEngine() { if (p) crp_rp_spmm_free(&p); }
    operator crp_rp_spmm_p() const { return p; }
};

// crp_para2d_spmm_free is `delete`: members are released in REVERSE order of declaration -- the inner row engine first, then the
// two communicators it and the grid row use, then this engine's own device buffers, which is why those come first here.
struct crp_para2d_spmm
{
    crp_comm_t *comm_glb = nullptr;        // not owned
    size_t rA_cost = 0;
    double t_init = 0.0, t_ag_A = 0.0;
    int    value_uploads = 1;              // times the panel's values went host -> device (0: filled from the device all-gather)
    bool   replicated_on_device = false;   // the panel's colidx / val were all-gathered between device buffers
    bool   plan_only = false;
    int    pn = 1, pi = 0, pj = 0;
    std::vector<long long> row_nnz;        // pn: nonzeros of the grid row's A0 slices
    std::vector<long long> row_off;        // pn + 1: their prefix sums = where every slice starts in the panel
    // ---- row softmax over the slice (pn > 1): the slice's own row pointer from 0, kept by init; on the device from the first call
    std::vector<int> slice_rowptr;
    crp::DevArray<int> sm_rowptr;
    // ---- state of update_values / sddmm on a grid with pn > 1: nothing below exists before the first such call
    std::vector<double> panel_val;         // update_values: the panel's values as gathered
    crp::DevArray<double> dv_panel;        // update_values_dev: the panel's values as gathered (sized for fp64)
    std::vector<char> dv_host;             // ... staged on the host when the communicator has no allgatherv_dev
    crp::DevArray<float>  sd_send32;       // fp32: every peer's run in a slot of round_up(nnz_j, 2) floats
    crp::DevArray<double> sd_out;          // staging of a host `out` (these three are sized for fp64, used by both dtypes)
    crp::DevArray<double> sd_recv;         // the pn runs received: fp64 stride slice nnz, fp32 stride round_up(slice nnz, 2)
    crp::DevArray<double> sd_part;         // partial dots of the panel: row_off[pn] entries
    bool sd_built64 = false, sd_built32 = false;
    crp::OwnedComm comm_row;               // split again from comm_glb by the first update_values / sddmm
    crp::OwnedComm comm_col;               // the grid column's, the inner engine's communicator
    RpEngine rp;
};


static long long up2(long long v) { return (v + 1) / 2 * 2; }

// The grid-row communicator init freed: split again from the global one by the first call that needs it -- that call is
// therefore collective over the WHOLE grid (every rank makes these calls anyway) -- and kept from then on.
static crp_comm_t *row_comm(crp_para2d_spmm *e)
{
    if (e->comm_row == nullptr) e->comm_row = crp::OwnedComm(e->comm_glb->split(e->comm_glb->ctx, e->pi, e->pj));
    return e->comm_row;
}

// first SDDMM of a dtype on a grid with pn > 1: the partial buffer, the receive segments, the staging of a host `out`
// (sized for fp64, so the fp32 call reuses them) and, for fp32, the send slots with their pad floats zeroed once
static void build_sddmm(crp_para2d_spmm *e, bool f32)
{
    const long long p_nnz = e->row_off[e->pn], s_nnz = e->row_nnz[e->pj];
    if (!e->sd_built64 && !e->sd_built32)
    {
        e->sd_part.alloc((size_t) (p_nnz > 0 ? p_nnz : 1));
        e->sd_recv.alloc((size_t) (s_nnz > 0 ? s_nnz * e->pn : 1));
        e->sd_out.alloc((size_t) (s_nnz > 0 ? s_nnz : 1));
    }
    if (f32 && e->sd_send32 == nullptr)
    {
        size_t slots = 0;
        for (int j = 0; j < e->pn; j++) slots += (size_t) up2(e->row_nnz[j]);
        e->sd_send32.zeroed(slots > 0 ? slots : 2);
    }
    (f32 ? e->sd_built32 : e->sd_built64) = true;
}

template <class T>
static void sddmm_impl(crp_para2d_spmm *e, int layout, const T *X, long long ldX, const T *Y, long long ldY, T *out, int mode, void *s)
{
    if (e == NULL) return;
    if (e->pn == 1)
    {
        crp::inner_sddmm(e->rp, layout, X, ldX, Y, ldY, out, mode, s);     // one grid column: the row engine's result as it is
        return;
    }
    ASSERT_PRINTF(!e->plan_only, "para2d_spmm_sddmm on a plan-only engine (no device state)\n");
    constexpr bool f32 = sizeof(T) == sizeof(float);
    crp_comm_t *cr = row_comm(e);
    if (!(f32 ? e->sd_built32 : e->sd_built64)) build_sddmm(e, f32);
    const int pn = e->pn, pj = e->pj;
    const long long s_nnz = e->row_nnz[pj];
    int X_on_dev = 0, Y_on_dev = 0, out_on_dev = 1;
    HIP_OK(crp_dev_ptr_is_device(X, &X_on_dev));
    HIP_OK(crp_dev_ptr_is_device(Y, &Y_on_dev));
    if (out != NULL) HIP_OK(crp_dev_ptr_is_device(out, &out_on_dev));
    ASSERT_PRINTF(out != NULL || s_nnz == 0, "para2d_spmm_sddmm: NULL out\n");

    // 1. partial dots over this rank's n_loc columns, in panel order
    T *part = (T *) e->sd_part.get();
    crp::inner_sddmm(e->rp, layout, X, ldX, Y, ldY, part, mode, s);

    // 2. reduce-scatter along the grid row: peer j is owed the run of its slice, this rank receives pn runs of its own
    std::vector<long long> sc(pn), sd(pn), rc(pn), rd(pn);
    const double *send = (const double *) part;
    long long stride = s_nnz;                                         // of the receive segments, in elements of T
    if (!f32)
    {
        for (int j = 0; j < pn; j++) { sc[j] = e->row_nnz[j]; sd[j] = e->row_off[j]; rc[j] = s_nnz; rd[j] = (long long) j * s_nnz; }
    }
    else
    {
        // fp32 runs travel inside 8-byte words: every run is first copied to a slot that starts on a word
        stride = up2(s_nnz);
        long long slot = 0;
        for (int j = 0; j < pn; j++)
        {
            if (e->row_nnz[j] > 0)
                HIP_OK(crp_dev_memcpy(e->sd_send32 + slot, (const float *) part + e->row_off[j], sizeof(float) * (size_t) e->row_nnz[j], 2, s));
            sc[j] = up2(e->row_nnz[j]) / 2; sd[j] = slot / 2; rc[j] = stride / 2; rd[j] = (long long) j * (stride / 2);
            slot += up2(e->row_nnz[j]);
        }
        send = (const double *) e->sd_send32.get();
    }
    cr->alltoallv_dev_f64(cr->ctx, send, sc.data(), sd.data(), e->sd_recv, rc.data(), rd.data(), s);

    // 3. the pn runs added in ascending grid column
    if (s_nnz > 0)
    {
        T *outd = out_on_dev ? out : (T *) e->sd_out.get();
        HIP_OK(crp::sum_segments(pn, s_nnz, (const T *) e->sd_recv.get(), stride, outd, s));
        if (!out_on_dev) HIP_OK(crp_dev_memcpy(out, outd, sizeof(T) * (size_t) s_nnz, 1, s));
    }
    // completion as crp_rp_spmm_sddmm_ex: asynchronous only with device pointers and timing off
    if (!out_on_dev || !X_on_dev || !Y_on_dev || crp_rp_spmm_timing(e->rp)) HIP_OK(crp_stream_sync(s));
}

extern "C" {

static void para2d_init_common(crp_comm_t *comm, int pm, int pn, const int *A0_rowptr, const int *B_rowptr,
                               const int *AC_rowptr, const int *BC_colptr, const int *A_rowptr, const int *A_colidx,
                               const double *A_val, crp_para2d_spmm_p *out, bool plan_only)
{
    ASSERT_PRINTF(out != NULL && comm != NULL && pm > 0 && pn > 0 && comm->nproc == pm * pn,
                  "para2d_spmm_init: grid %d x %d does not match %d ranks\n", pm, pn, comm ? comm->nproc : -1);
    (void) AC_rowptr;   // implied by A0_rowptr, exactly as in the reference (:49-52)
    crp_para2d_spmm *e = new crp_para2d_spmm;
    e->comm_glb = comm;
    e->plan_only = plan_only;
    double t0 = get_wtime_sec();
    const int r = comm->rank, pi = r / pn, pj = r % pn;
    crp::OwnedComm comm_row(comm->split(comm->ctx, pi, pj));       // for the replication only: released on return
    e->comm_col = crp::OwnedComm(comm->split(comm->ctx, pj, pi));
    e->t_init += get_wtime_sec() - t0;

    // ---- replicate the row panel inside the grid row (reference :49-99)
    t0 = get_wtime_sec();
    const int my_nrow = A0_rowptr[r + 1] - A0_rowptr[r];
    const int my_nnz  = A_rowptr[my_nrow] - A_rowptr[0];
    const int p_srow  = A0_rowptr[pi * pn];
    const int p_nrow  = A0_rowptr[(pi + 1) * pn] - p_srow;
    std::vector<int>    p_rowptr((size_t) p_nrow + 1, 0), p_colidx;
    std::vector<double> p_val;
    crp::DevArray<double> panel_val_dev;           // the panel's values in HBM, when the replication left them there
    if (pn > 1)
    {
        std::vector<size_t> cnt(pn), dsp(pn);
        std::vector<int> nnzs(pn);
        for (int j = 0; j < pn; j++) { cnt[j] = sizeof(int); dsp[j] = sizeof(int) * (size_t) j; }
        comm_row->allgatherv_bytes(comm_row->ctx, &my_nnz, sizeof(int), nnzs.data(), cnt.data(), dsp.data());
        // row pointers carry global nnz offsets, so the slices concatenate into one monotone array
        size_t off = 0;
        for (int j = 0; j < pn; j++)
        {
            const int rk = pi * pn + j;
            cnt[j] = sizeof(int) * (size_t) (A0_rowptr[rk + 1] - A0_rowptr[rk]);
            dsp[j] = off;
            off += cnt[j];
        }
        comm_row->allgatherv_bytes(comm_row->ctx, A_rowptr, cnt[pj], p_rowptr.data(), cnt.data(), dsp.data());
        long long p_nnz = 0;
        for (int j = 0; j < pn; j++) p_nnz += nnzs[j];
        e->row_nnz.assign(nnzs.begin(), nnzs.end());
        // the gathered entries are the first row pointer of every row; an empty leading slice
        // starts where the next one does, so entry 0 is already the panel's first offset
        if (p_nrow == 0) p_rowptr[0] = 0;
        p_rowptr[p_nrow] = p_rowptr[0] + (int) p_nnz;
        p_colidx.resize((size_t) (p_nnz > 0 ? p_nnz : 1));
        p_val.resize((size_t) (p_nnz > 0 ? p_nnz : 1));
        std::vector<size_t> cnt_i(pn), dsp_i(pn), cnt_v(pn), dsp_v(pn);
        off = 0;
        for (int j = 0; j < pn; j++) { cnt_i[j] = sizeof(int) * (size_t) nnzs[j]; dsp_i[j] = off; off += cnt_i[j]; }
        off = 0;
        for (int j = 0; j < pn; j++) { cnt_v[j] = sizeof(double) * (size_t) nnzs[j]; dsp_v[j] = off; off += cnt_v[j]; }
        const bool host_only = crp::knobs().replicate_host;
        if (comm_row->allgatherv_dev != NULL && !plan_only && !host_only && p_nnz > 0)
        {
            // Device replication (reference :81-83: two MPI_Iallgatherv on duplicate communicators): the own slices go
            // up once, column indices and values are all-gathered between device buffers -- over xGMI every source feeds
            // its pn - 1 peers on distinct links; the two gathers use ONE RCCL communicator, which runs them one after the
            // other whatever streams they are given, so no overlap between them is claimed --, and the panel comes back
            // through pinned memory: the plan is built on the host from the column indices, and the values are a public
            // host field of the engine (struct rowpara_spmm::A_val, /root/reference/src/rowpara_spmm.h:8-40), so the copy
            // down is owed to the API.  The gathered VALUES stay in HBM until the 1D engine has been built: its device
            // matrices are filled from them (crp_rp_spmm_init_dv), not uploaded a second time.
            crp::DevStream s_i, s_v;
            crp::DevArray<int> ci_all;
            crp::HostPinned h_ci, h_va;
            s_i.ensure();
            s_v.ensure();
            void *d_ci_all = ci_all.alloc((size_t) p_nnz), *d_va_all = panel_val_dev.alloc((size_t) p_nnz);
            h_ci.alloc(sizeof(int) * (size_t) p_nnz);
            h_va.alloc(sizeof(double) * (size_t) p_nnz);
            // own slice straight into its place of the gathered arrays (send == recv + displacement: no extra copy)
            void *d_ci = (char *) d_ci_all + dsp_i[pj], *d_va = (char *) d_va_all + dsp_v[pj];
            int rc = 0;
            if (my_nnz > 0)
            {
                rc = crp_dev_memcpy(d_ci, A_colidx, cnt_i[pj], 0, s_i);
                if (rc == 0) rc = crp_dev_memcpy(d_va, A_val, cnt_v[pj], 0, s_v);
                ASSERT_PRINTF(rc == 0, "para2d_spmm_init: upload of the A0 slice (%d)\n", rc);
            }
            comm_row->allgatherv_dev(comm_row->ctx, d_ci, cnt_i[pj], d_ci_all, cnt_i.data(), dsp_i.data(), s_i);
            comm_row->allgatherv_dev(comm_row->ctx, d_va, cnt_v[pj], d_va_all, cnt_v.data(), dsp_v.data(), s_v);
            rc = crp_dev_memcpy(h_ci.p, d_ci_all, sizeof(int) * (size_t) p_nnz, 1, s_i);
            if (rc == 0) rc = crp_dev_memcpy(h_va.p, d_va_all, sizeof(double) * (size_t) p_nnz, 1, s_v);
            if (rc == 0) rc = crp_stream_sync(s_i);
            if (rc == 0) rc = crp_stream_sync(s_v);
            ASSERT_PRINTF(rc == 0, "para2d_spmm_init: panel replication on the device (%d)\n", rc);
            memcpy(p_colidx.data(), h_ci.p, sizeof(int) * (size_t) p_nnz);
            memcpy(p_val.data(), h_va.p, sizeof(double) * (size_t) p_nnz);
            e->replicated_on_device = true;
        }
        else
        {
            comm_row->allgatherv_bytes(comm_row->ctx, A_colidx, cnt_i[pj], p_colidx.data(), cnt_i.data(), dsp_i.data());
            comm_row->allgatherv_bytes(comm_row->ctx, A_val, cnt_v[pj], p_val.data(), cnt_v.data(), dsp_v.data());
        }
    }
    else
    {
        memcpy(p_rowptr.data(), A_rowptr, sizeof(int) * ((size_t) p_nrow + 1));
        p_colidx.assign(A_colidx, A_colidx + my_nnz);
        p_val.assign(A_val, A_val + my_nnz);
        if (my_nnz == 0) { p_colidx.resize(1); p_val.resize(1); }
        e->row_nnz.assign(1, my_nnz);
    }
    e->pn = pn; e->pi = pi; e->pj = pj;
    if (pn > 1)
    {
        e->slice_rowptr.resize((size_t) my_nrow + 1);
        for (int i = 0; i <= my_nrow; i++) e->slice_rowptr[i] = A_rowptr[i] - A_rowptr[0];
    }
    e->row_off.assign((size_t) pn + 1, 0);
    for (int j = 0; j < pn; j++) e->row_off[j + 1] = e->row_off[j] + e->row_nnz[j];
    e->t_ag_A += get_wtime_sec() - t0;

    // ---- replication cost statistic: floor(1.5 * nnz(A) * (pn - 1)), nnz(A) = end of the last
    //      rank's global row pointer (reference :100-106), shared without a point-to-point message
    {
        const int P = comm->nproc;
        std::vector<int> ends(P);
        std::vector<size_t> cnt(P, sizeof(int)), dsp(P);
        for (int q = 0; q < P; q++) dsp[q] = sizeof(int) * (size_t) q;
        const int my_end = A_rowptr[my_nrow];
        comm->allgatherv_bytes(comm->ctx, &my_end, sizeof(int), ends.data(), cnt.data(), dsp.data());
        e->rA_cost = (size_t) ((double) ends[P - 1] * (double) (pn - 1) * 1.5);
    }

    // ---- 1D engine on the grid column (reference :111-118)
    t0 = get_wtime_sec();
    const int n_loc = BC_colptr[pj + 1] - BC_colptr[pj];
    if (plan_only)
        crp_rp_spmm_init_plan_only(p_srow, p_nrow, p_rowptr.data(), p_colidx.data(), p_val.data(), B_rowptr, n_loc,
                                   e->comm_col, &e->rp.p);
    else if (panel_val_dev != nullptr)
    {
        crp_rp_spmm_init_dv(p_srow, p_nrow, p_rowptr.data(), p_colidx.data(), p_val.data(), panel_val_dev, B_rowptr, n_loc, e->comm_col,
                            &e->rp.p);
        e->value_uploads = 0;
    }
    else
        crp_rp_spmm_init(p_srow, p_nrow, p_rowptr.data(), p_colidx.data(), p_val.data(), B_rowptr, n_loc,
                         e->comm_col, &e->rp.p);
    panel_val_dev.reset();
    e->t_init += get_wtime_sec() - t0;
    *out = e;
}

void crp_para2d_spmm_init(crp_comm_t *comm, int pm, int pn, const int *A0_rowptr, const int *B_rowptr,
                          const int *AC_rowptr, const int *BC_colptr, const int *A_rowptr, const int *A_colidx,
                          const double *A_val, crp_para2d_spmm_p *out)
{
    para2d_init_common(comm, pm, pn, A0_rowptr, B_rowptr, AC_rowptr, BC_colptr, A_rowptr, A_colidx, A_val, out, false);
}

void crp_para2d_spmm_init_plan_only(crp_comm_t *comm, int pm, int pn, const int *A0_rowptr, const int *B_rowptr,
                                    const int *AC_rowptr, const int *BC_colptr, const int *A_rowptr,
                                    const int *A_colidx, const double *A_val, crp_para2d_spmm_p *out)
{
    para2d_init_common(comm, pm, pn, A0_rowptr, B_rowptr, AC_rowptr, BC_colptr, A_rowptr, A_colidx, A_val, out, true);
}

void crp_para2d_spmm_free(crp_para2d_spmm_p *p)
{
    if (p == NULL || *p == NULL) return;
    delete *p;       // every device resource, the communicators and the inner engine are members that release themselves
    *p = NULL;
}

void crp_para2d_spmm_exec(crp_para2d_spmm_p e, int BC_layout, const double *B, int ldB, double *C, int ldC)
{
    if (e == NULL) return;
    crp_rp_spmm_exec(e->rp, BC_layout, B, ldB, C, ldC);
}

void crp_para2d_spmm_exec_ex(crp_para2d_spmm_p e, int BC_layout, const double *B, long long ldB, double *C,
                             long long ldC, void *stream)
{
    if (e == NULL) return;
    crp_rp_spmm_exec_ex(e->rp, BC_layout, B, ldB, C, ldC, stream);
}

void crp_para2d_spmm_exec_f32_ex(crp_para2d_spmm_p e, int BC_layout, const float *B, long long ldB, float *C,
                                 long long ldC, void *stream)
{
    if (e == NULL) return;
    crp_rp_spmm_exec_f32_ex(e->rp, BC_layout, B, ldB, C, ldC, stream);
}

void crp_para2d_spmm_exec_t_ex(crp_para2d_spmm_p e, int BC_layout, const double *B, long long ldB, double *C, long long ldC,
                               void *stream)
{
    if (e == NULL) return;
    crp_rp_spmm_exec_t_ex(e->rp, BC_layout, B, ldB, C, ldC, stream);
}

void crp_para2d_spmm_update_values(crp_para2d_spmm_p e, const double *A_val)
{
    if (e == NULL) return;
    if (e->pn == 1)
    {
        crp_rp_spmm_update_values(e->rp, A_val);
        return;
    }
    crp_comm_t *cr = row_comm(e);
    const int pn = e->pn;
    ASSERT_PRINTF(A_val != NULL || e->row_nnz[e->pj] == 0, "para2d_spmm_update_values: NULL values\n");
    std::vector<size_t> cnt(pn), dsp(pn);
    for (int j = 0; j < pn; j++) { cnt[j] = sizeof(double) * (size_t) e->row_nnz[j]; dsp[j] = sizeof(double) * (size_t) e->row_off[j]; }
    e->panel_val.resize((size_t) (e->row_off[pn] > 0 ? e->row_off[pn] : 1));
    cr->allgatherv_bytes(cr->ctx, A_val, cnt[e->pj], e->panel_val.data(), cnt.data(), dsp.data());
    crp_rp_spmm_update_values(e->rp, e->panel_val.data());
}

void crp_para2d_spmm_exec_t_f32_ex(crp_para2d_spmm_p e, int BC_layout, const float *B, long long ldB, float *C, long long ldC,
                                   void *stream)
{
    if (e == NULL) return;
    crp_rp_spmm_exec_t_f32_ex(e->rp, BC_layout, B, ldB, C, ldC, stream);
}

void crp_para2d_spmm_update_values_dev(crp_para2d_spmm_p e, const void *A_val_dev, int f32, void *stream)
{
    if (e == NULL) return;
    if (e->pn == 1)
    {
        crp_rp_spmm_update_values_dev(e->rp, A_val_dev, f32, stream);
        return;
    }
    ASSERT_PRINTF(!e->plan_only, "para2d_spmm_update_values_dev on a plan-only engine (no device state)\n");
    ASSERT_PRINTF(f32 == 0 || f32 == 1, "para2d_spmm_update_values_dev: f32 must be 0 or 1\n");
    crp_comm_t *cr = row_comm(e);
    const int pn = e->pn, pj = e->pj;
    const size_t isz = f32 ? sizeof(float) : sizeof(double);
    ASSERT_PRINTF(A_val_dev != NULL || e->row_nnz[pj] == 0, "para2d_spmm_update_values_dev: NULL values\n");
    const size_t p_nnz = (size_t) e->row_off[pn];
    if (e->dv_panel == nullptr) e->dv_panel.alloc(p_nnz > 0 ? p_nnz : 1);
    std::vector<size_t> cnt(pn), dsp(pn);
    for (int j = 0; j < pn; j++) { cnt[j] = isz * (size_t) e->row_nnz[j]; dsp[j] = isz * (size_t) e->row_off[j]; }
    if (cr->allgatherv_dev != NULL && !crp::knobs().replicate_host)
        cr->allgatherv_dev(cr->ctx, A_val_dev, cnt[pj], e->dv_panel, cnt.data(), dsp.data(), stream);
    else
    {
        // no device all-gather (or CRPSPMM_REPLICATE=host, as in init): the slice comes down, the panel goes up
        e->dv_host.resize(isz * (p_nnz > 0 ? p_nnz : 1) + cnt[pj] + 1);
        char *panel = e->dv_host.data(), *mine = panel + isz * (p_nnz > 0 ? p_nnz : 1);
        if (cnt[pj] > 0)
        {
            HIP_OK(crp_dev_memcpy(mine, A_val_dev, cnt[pj], 1, stream));
            HIP_OK(crp_stream_sync(stream));
        }
        cr->allgatherv_bytes(cr->ctx, mine, cnt[pj], panel, cnt.data(), dsp.data());
        if (p_nnz > 0)
        {
            HIP_OK(crp_dev_memcpy(e->dv_panel, panel, isz * p_nnz, 0, stream));
            HIP_OK(crp_stream_sync(stream));       // dv_host is reused by the next call
        }
    }
    crp_rp_spmm_update_values_dev(e->rp, e->dv_panel, f32, stream);
}

void crp_para2d_spmm_sddmm_ex(crp_para2d_spmm_p e, int layout, const double *X, long long ldX, const double *Y, long long ldY,
                              double *out, int mode, void *stream)
{
    sddmm_impl<double>(e, layout, X, ldX, Y, ldY, out, mode, stream);
}

void crp_para2d_spmm_sddmm_f32_ex(crp_para2d_spmm_p e, int layout, const float *X, long long ldX, const float *Y, long long ldY,
                                  float *out, int mode, void *stream)
{
    sddmm_impl<float>(e, layout, X, ldX, Y, ldY, out, mode, stream);
}

// row softmax over the slice on a grid with pn > 1: the slice is a run of whole rows, so neither the panel nor a communicator
// is involved; false when the slice holds no nonzero (nothing to upload or launch)
static bool row_softmax_ready(crp_para2d_spmm *e, const char *what, int f32)
{
    const bool any = e->row_nnz[e->pj] != 0;
    crp::row_softmax_ready(what, e->plan_only, f32, any, e->sm_rowptr, e->slice_rowptr, NULL);
    return any;
}

void crp_para2d_spmm_row_softmax_ex(crp_para2d_spmm_p e, const void *s, void *y, int f32, void *stream)
{
    if (e == NULL) return;
    if (e->pn == 1)
    {
        crp_rp_spmm_row_softmax_ex(e->rp, s, y, f32, stream);
        return;
    }
    if (!row_softmax_ready(e, "para2d_spmm_row_softmax", f32)) return;
    ASSERT_PRINTF(s != NULL && y != NULL, "para2d_spmm_row_softmax: NULL values\n");
    crp::row_softmax((int) e->slice_rowptr.size() - 1, e->sm_rowptr, f32, s, y, stream);
}

void crp_para2d_spmm_row_softmax_bwd_ex(crp_para2d_spmm_p e, const void *y, const void *dy, void *ds, int f32, void *stream)
{
    if (e == NULL) return;
    if (e->pn == 1)
    {
        crp_rp_spmm_row_softmax_bwd_ex(e->rp, y, dy, ds, f32, stream);
        return;
    }
    if (!row_softmax_ready(e, "para2d_spmm_row_softmax_bwd", f32)) return;
    ASSERT_PRINTF(y != NULL && dy != NULL && ds != NULL, "para2d_spmm_row_softmax_bwd: NULL values\n");
    crp::row_softmax_bwd((int) e->slice_rowptr.size() - 1, e->sm_rowptr, f32, y, dy, ds, stream);
}

int crp_para2d_spmm_row_softmax_built(crp_para2d_spmm_p e)
{
    if (e == NULL) return 0;
    return e->pn == 1 ? crp_rp_spmm_row_softmax_built(e->rp) : (e->sm_rowptr ? 1 : 0);
}

int crp_para2d_spmm_sddmm_built(crp_para2d_spmm_p e) { return (e && (e->sd_built64 || e->sd_built32)) ? 1 : 0; }
long long crp_para2d_spmm_slice_nnz(crp_para2d_spmm_p e) { return e ? e->row_nnz[e->pj] : -1; }
int crp_para2d_spmm_row_slice_nnz(crp_para2d_spmm_p e, long long *nnz_of_pj)
{
    if (e == NULL) return 0;
    if (nnz_of_pj != NULL)
        for (int j = 0; j < e->pn; j++) nnz_of_pj[j] = e->row_nnz[j];
    return e->pn;
}

int crp_para2d_spmm_replicated_on_device(crp_para2d_spmm_p e) { return (e && e->replicated_on_device) ? 1 : 0; }
int crp_para2d_spmm_value_uploads(crp_para2d_spmm_p e) { return e ? e->value_uploads : -1; }

void crp_para2d_spmm_print_stat(crp_para2d_spmm_p e)
{
    if (e == NULL) return;
    crp_rp_plan_view_t v;
    crp_rp_spmm_get_plan(e->rp, &v);
    if (v.n_exec == 0) return;
    crp_comm_t *c = e->comm_glb;
    const int P = c->nproc;
    uint64_t recv = (uint64_t) v.rB_recv_size * (uint64_t) v.glb_n, recv_max = 0, recv_sum = 0;
    double raw[7] = {e->t_init, e->t_ag_A, v.t_pack, v.t_a2a, v.t_unpack, v.t_spmm, v.t_exec}, tmax[7], tavg[7];
    c->reduce_u64(c->ctx, &recv, &recv_max, 1, CRP_OP_MAX);
    c->reduce_u64(c->ctx, &recv, &recv_sum, 1, CRP_OP_SUM);
    c->reduce_f64(c->ctx, raw, tmax, 7, CRP_OP_MAX);
    c->reduce_f64(c->ctx, raw, tavg, 7, CRP_OP_SUM);
    if (c->rank != 0) return;
    for (int i = 2; i <= 6; i++)
    {
        tmax[i] /= v.n_exec;
        tavg[i] /= ((double) v.n_exec * P);
    }
    tavg[1] /= P;
    // same lines as src/para2d_spmm.c:183-196
    printf("para2d_spmm_init() time = %.2f s\n", tmax[0]);
    printf("Total comm size for replicating A = %zu\n", e->rA_cost);
    printf("Total comm size for replicating B = %zu\n", (size_t) recv_sum);
    printf("Total comm size for SpMM          = %zu\n", e->rA_cost + (size_t) recv_sum);
    printf("-------------------- Runtime (s) --------------------\n");
    printf("                                     avg         max\n");
    printf("Replicate A matrix (once)         %6.3f      %6.3f\n", tavg[1], tmax[1]);
    printf("Pack B matrix for redistribution  %6.3f      %6.3f\n", tavg[2], tmax[2]);
    printf("Redistribute B matrix             %6.3f      %6.3f\n", tavg[3], tmax[3]);
    printf("Unpack received B matrix data     %6.3f      %6.3f\n", tavg[4], tmax[4]);
    printf("Local SpMM                        %6.3f      %6.3f\n", tavg[5], tmax[5]);
    printf("Total para2d_spmm_exec()          %6.3f      %6.3f\n", tavg[6], tmax[6]);
    printf("Replicate A + para2d_spmm_exec()  %6.3f      %6.3f\n", tavg[1] + tavg[6], tmax[1] + tmax[6]);
    printf("\n");
    fflush(stdout);
}

void crp_para2d_spmm_clear_stat(crp_para2d_spmm_p e)
{
    if (e == NULL) return;
    crp_rp_spmm_clear_stat(e->rp);
}

crp_rp_spmm_p crp_para2d_spmm_rp(crp_para2d_spmm_p e) { return e ? e->rp.p : NULL; }
size_t crp_para2d_spmm_rA_cost(crp_para2d_spmm_p e) { return e ? e->rA_cost : 0; }
double crp_para2d_spmm_t_ag_A(crp_para2d_spmm_p e) { return e ? e->t_ag_A : 0.0; }

}  // extern "C"
