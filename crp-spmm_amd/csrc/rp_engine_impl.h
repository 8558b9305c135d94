// rp_engine_impl.h -- the row engine's state (struct crp_rp_spmm) and what its translation units share: rp_engine.cpp (init, exec,
// exec_t, sddmm, value updates), rp_attention.cpp (the fused attention, forward and backward, single- and multi-head) and
// rp_gat.cpp (the fused GAT and GATv2 attention, forward).  Internal: nothing outside csrc/ includes it.
//
// Every call that moves rows of a dense operand to the ranks that asked for them runs ONE schedule, pack_exchange_run below: the
// call names its travelling operands (Traveller: an Xchg, the source, the receive buffer), says where they are packed (PackOn) and
// gives the part kernel as product(A, part).  Around it, one definition each: the opening checks (check_call, check_scores), a
// part's positions array (part_positions), a host result vector staged on the device (HostVec), the way back of exec_t and the
// attention backward (reverse_exchange_rows, accumulate_rows) and the end of a call (finish_call, close_call).
#ifndef CRP_RP_ENGINE_IMPL_H
#define CRP_RP_ENGINE_IMPL_H

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

// One exchange of packed rows over the forward plan's peers: `cols` elements of every row travel, in rows of ld elements (a
// whole number of 8-byte words) from send to recv.  A view: the engine owns the buffers and the count vectors.
struct Xchg
{
    void *send, *recv;
    int cols;
    long long ld;
    const long long *sc, *sd, *rc, *rd;           // counts / displacements in 8-byte words, as alltoallv_dev_f64 takes them
};

// The storage of the GAT attention's narrow exchange of er (rp_gat.cpp): rows of `heads` elements, fp32 rows padded to whole 8-byte
// words, through buffers of their own
template <class T> struct GatXchg
{
    int heads = 0;                               // 0: not set up
    long long ld = 0;
    std::vector<long long> sc, sd, rc, rd;
    crp::DevArray<T> recv, send;
    Xchg view() { return Xchg{send.get(), recv.get(), heads, ld, sc.data(), sd.data(), rc.data(), rd.data()}; }
};

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
    // fused attention backward (crp_rp_spmm_attention_bwd_ex, rp_attention.cpp), allocated by its first call of a dtype: delta, one
    // entry per row of A, written by the row side and read by the column side
    bool bw_built = false;
    crp::DevArray<float>  bw_delta32_dev;
    crp::DevArray<double> bw_delta_dev;
    size_t bw_delta32_cap = 0, bw_delta_cap = 0;        // entries; a multi-head call that needs A_nrow * heads grows its array
    // fused GAT attention (crp_rp_spmm_gat_ex, rp_gat.cpp): the narrow exchange of er, one per dtype, set up by the first call of
    // that dtype and again by a call with another number of heads
    bool gt_built = false;
    GatXchg<float>  gt_x32;
    GatXchg<double> gt_x64;
    // fused GATv2 attention (crp_rp_spmm_gatv2_ex, rp_gat.cpp): XS travels as B does, so the first call uploads the parts' positions only
    bool gv2_built = false;
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

// ---- what the fp64 and the fp32 exec do differently: kernels, variant, exchange buffers -----------------------------
// The fp32 exec packs rows of ld32 = round_up(n, 4) floats (16-byte rows for the packing kernel and for the team kernel's
// second B source) and carries them through the communicator's fp64 all-to-all as opaque 8-byte words: no back end does
// arithmetic on the payload, so crp_comm_t stays as it is.
static inline long long ld32_of(int n) { return ((long long) n + 3) / 4 * 4; }

static inline Xchg exchange_of(crp_rp_spmm *e, const double *)
{
    return Xchg{e->sendbuf_dev, e->recvbuf_dev, e->glb_n, (long long) e->glb_n, e->rB_scnts.data(), e->rB_sdispls.data(),
                e->rB_rcnts.data(), e->rB_rdispls.data()};
}

// the forward plan's per-peer counts and displacements (rB_*: rows * glb_n elements) for rows of `words` 8-byte words
static inline void plan_words(const crp_rp_spmm *e, long long words, std::vector<long long> &sc, std::vector<long long> &sd,
                              std::vector<long long> &rc, std::vector<long long> &rd)
{
    const long long n = e->glb_n;
    auto by_rows = [&](const std::vector<long long> &v, std::vector<long long> &out) {
        out.resize(v.size());
        for (size_t q = 0; q < v.size(); q++) out[q] = n > 0 ? v[q] / n * words : 0;
    };
    by_rows(e->rB_scnts, sc);
    by_rows(e->rB_sdispls, sd);
    by_rows(e->rB_rcnts, rc);
    by_rows(e->rB_rdispls, rd);
}

// first fp32 exec: word counts (rows of ld32 / 2 words) and the fp32 exchange buffers
static inline Xchg exchange_of(crp_rp_spmm *e, const float *)
{
    const long long ld = ld32_of(e->glb_n);
    if (!e->x32_ready)
    {
        plan_words(e, ld / 2, e->x32_scnts, e->x32_sdispls, e->x32_rcnts, e->x32_rdispls);
        // the pad columns are zeroed here and never written again: no uninitialised byte crosses a link
        if (e->n_send_rows > 0 && ld > 0) e->sendbuf32_dev.zeroed((size_t) e->n_send_rows * (size_t) ld);
        if (e->n_recv_rows > 0 && ld > 0) e->recvbuf32_dev.zeroed((size_t) e->n_recv_rows * (size_t) ld);
        e->x32_ready = true;
    }
    return Xchg{e->sendbuf32_dev, e->recvbuf32_dev, e->glb_n, ld, e->x32_scnts.data(), e->x32_sdispls.data(), e->x32_rcnts.data(),
                e->x32_rdispls.data()};
}

// Is this pointer on the device?  The pointer-attribute query is not free: the forward exec passes the engine's cache of the last
// operand seen in that place (last, last_dev), the other calls ask every time (last == nullptr).
static inline bool on_device(const void *p, const void **last = nullptr, int *last_dev = nullptr)
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
static inline void complete(crp_rp_spmm *e, void *s, bool synced, bool must_sync)
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

// with timing on: wait for s and bill the time since t0 to *bucket
static inline void lap(crp_rp_spmm *e, void *s, double &t0, double *bucket)
{
    if (!e->timing) return;
    HIP_OK(crp_stream_sync(s));
    const double t1 = get_wtime_sec();
    *bucket += t1 - t0;
    t0 = t1;
}

// ---- the opening and the end of a call ----------------------------------------------------------------------------------------------
// what every call refuses first; layout_name: what the call's ABI names its layout argument (nullptr: it takes none)
static inline void check_call(const crp_rp_spmm *e, const char *what, const char *layout_name = nullptr, int layout = 0)
{
    ASSERT_PRINTF(!e->plan_only, "%s on a plan-only engine (no device state)\n", what);
    ASSERT_PRINTF(layout_name == nullptr || layout == 0 || layout == 1, "%s must be 0 or 1\n", layout_name);
}
// ... and the attention family after it: bias, and the scalar of its scores (scale, slope)
static inline void check_scores(int bias, double scalar, const char *scalar_name)
{
    ASSERT_PRINTF(bias == 0 || bias == 1, "bias must be 0 or 1\n");
    ASSERT_PRINTF(scalar - scalar == 0.0, "%s must be finite\n", scalar_name);
}

// The end of a call: complete() unless the stream was synchronised already, then the call's host time and count.
static inline void close_call(crp_rp_spmm *e, void *s, bool synced, bool must_sync, double t_begin)
{
    complete(e, s, synced, must_sync);
    e->t_exec += get_wtime_sec() - t_begin;
    e->n_exec++;
}

// ... of a call with a dense result: the result back in the caller's layout and memory first, the kernels billed to t_spmm between
// the transpose and the copy to the host
template <class T>
static inline void finish_call(crp_rp_spmm *e, const crp::OutView<T> &v, void *s, double &t0, bool must_sync, double t_begin)
{
    const bool synced = crp::finish(v, s, [&] { lap(e, s, t0, &e->t_spmm); });
    close_call(e, s, synced, must_sync, t_begin);
}

// ---- a result vector of the call's (lse, p_out, sddmm's out): n entries at p, on the host or on the device ------------------------------
// A host vector is computed in `scratch` on the device and downloaded after the kernels; the call then has to wait for its stream.
template <class T> struct HostVec
{
    T *host, *dev;        // dev: where the kernels write
    size_t n;
    bool staged;
    void download(void *s) const { if (staged) HIP_OK(crp_dev_memcpy(host, dev, n * sizeof(T), 1, s)); }
};
// (n == 0: the caller did not ask for it, or it has no entries -- the pointer passes through, nothing is staged)
template <class T>
static inline HostVec<T> host_vec(T *p, size_t n, crp::DevScratch &scratch)
{
    const bool staged = n > 0 && !on_device(p);
    return HostVec<T>{p, staged ? scratch.grow<T>(n) : p, n, staged};
}

// ---- the schedule: pack, exchange, and the part kernels beside or after them ---------------------------------------------------------------
// One operand on its way to the ranks that asked for its rows: x.cols columns of the row-major device operand src (leading dimension
// ld) are packed into x.send and land in recv in final order (x.recv, or a buffer of the same shape: several operands may share x)
template <class T> struct Traveller
{
    Xchg x;
    const T *src;
    long long ld;
    void *recv;
};

// Where the overlapped path packs.  ON_CALLER: on the caller's stream, ahead of ev_packed, so the exchange stream starts with
// packed rows (exec, sddmm; one traveller only: the send buffer is not reused).  ON_EXCHANGE: on the exchange stream behind the
// ev_packed wait, every traveller's pack in front of its exchange, so travellers may share a send buffer in stream order (the
// attention family).  The two are as measured and not interchangeable without measuring again.
enum PackOn { PACK_ON_CALLER, PACK_ON_EXCHANGE };

// pack the rows of t.src that other ranks asked for into t.x.send, on st (reference :232-262)
template <class T>
static inline void pack_rows(crp_rp_spmm *e, const Traveller<T> &t, void *st)
{
    if (e->n_send_rows > 0 && t.x.cols > 0)
        HIP_OK(crp::gather((int) e->n_send_rows, t.x.cols, e->sridxs_dev, t.src, t.ld, (T *) t.x.send, t.x.ld, st));
}

// the exchange call on st (reference :275-309), its host time billed to t_a2a_host: x's counts, from -> to
static inline void exchange(crp_rp_spmm *e, const void *from, const long long *fc, const long long *fd, void *to, const long long *tc,
                            const long long *td, void *st)
{
    const double tx0 = get_wtime_sec();
    e->comm->alltoallv_dev_f64(e->comm->ctx, (const double *) from, fc, fd, (double *) to, tc, td, st);
    e->t_a2a_host += get_wtime_sec() - tx0;
}
template <class T>
static inline void exchange_rows(crp_rp_spmm *e, const Traveller<T> &t, void *st)
{
    exchange(e, t.x.send, t.x.sc, t.x.sd, t.recv, t.x.rc, t.x.rd, st);
}

// the local kernels after the exchange (reference :388-408): product(A, part) once for A_dev (part 0), or for A_int (1) and A_bnd (2)
template <class F>
static inline void run_parts(crp_rp_spmm *e, F &&product)
{
    if (e->A_int != nullptr)
    {
        product(e->A_int, 1);
        product(e->A_bnd, 2);
    }
    else product(e->A_dev, 0);
}

// the positions in A_val through which that part writes per-nonzero results (sddmm's out, p_out, ds_out); part 0: in place
static inline const int *part_positions(const crp_rp_spmm *e, int part)
{
    return part == 1 ? e->sd_int_pos.get() : (part == 2 ? e->sd_bnd_pos.get() : nullptr);
}

// The schedule.  With timing off and a split engine the interior part is enqueued on s while the packs (PACK_ON_EXCHANGE) and the
// exchanges run on the engine's second stream, from the point of s where the operands are ready (ev_packed); the boundary part
// follows on s after the last exchange has landed (ev_landed).  Otherwise everything runs on s in sequence, traveller by traveller,
// and with timing on bills to t_pack and t_a2a.  t0 is left at the start of the kernels, which the caller bills.
template <class T, size_t N, class F>
static inline void pack_exchange_run(crp_rp_spmm *e, void *s, double &t0, PackOn where, const Traveller<T> (&travellers)[N], F &&product)
{
    const bool timing = e->timing != 0;
    if (timing) { HIP_OK(crp_stream_sync(s)); }
    t0 = get_wtime_sec();
    if (e->A_int == nullptr || timing)
    {
        for (const Traveller<T> &t : travellers)
        {
            pack_rows(e, t, s);
            lap(e, s, t0, &e->t_pack);
            if (e->nproc > 1) exchange_rows(e, t, s);
            lap(e, s, t0, &e->t_a2a);
        }
        run_parts(e, product);
        return;
    }
    if (where == PACK_ON_CALLER)
        for (const Traveller<T> &t : travellers) pack_rows(e, t, s);
    // The exchange runs on its own stream beside the interior rows' product.  The product is ENQUEUED FIRST: it does not
    // depend on the exchange, and issuing a group of sends / receives can hold the host for a while (a non-blocking RCCL
    // communicator is polled until the group is on the stream) -- with the exchange first, the whole interior product
    // (0.06 - 0.2 ms per GPU at pwtk size) could have passed before its launch was even issued.
    HIP_OK(crp_event_record(e->ev_packed, s));
    product(e->A_int, 1);
    HIP_OK(crp_stream_wait_event(e->xstream, e->ev_packed));
    for (const Traveller<T> &t : travellers)
    {
        if (where == PACK_ON_EXCHANGE) pack_rows(e, t, e->xstream);
        exchange_rows(e, t, e->xstream);
    }
    HIP_OK(crp_event_record(e->ev_landed, e->xstream));
    HIP_OK(crp_stream_wait_event(s, e->ev_landed));
    product(e->A_bnd, 2);
}

// ---- the way back (exec_t, the attention backward): the forward plan run backwards -------------------------------------------------------
// what this rank receives in the forward exchange it sends here, from `from` (a receive buffer of x's shape) into x.send, on st
static inline void reverse_exchange_rows(crp_rp_spmm *e, const Xchg &x, const void *from, void *st)
{
    exchange(e, from, x.rc, x.rd, x.send, x.sc, x.sd, st);
}

// ... and the rows that came back (x.send) added to the rows of dst they belong to (acc_dev: build_transposed), on s
template <class T>
static inline void accumulate_rows(crp_rp_spmm *e, const Xchg &x, T *dst, long long ldd, void *s)
{
    if (e->n_acc == 0 || x.cols == 0) return;
    const int *acc_row = e->acc_dev, *acc_ptr = acc_row + e->n_acc, *acc_pos = acc_ptr + e->n_acc + 1;
    HIP_OK(crp::scatter_add(e->n_acc, x.cols, acc_row, acc_ptr, acc_pos, (const T *) x.send, x.ld, dst, ldd, s));
}

// ---- the parts' positions in A_val and the host copy of the values --------------------------------------------------------------
// int_src / bnd_src of a split engine as int32 device arrays: the SDDMM's parts write through them into the order of A_val, a
// device value update gathers the parts' values through them; whichever call comes first uploads
static inline void upload_part_positions(crp_rp_spmm *e)
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
static inline void refresh_host_values(crp_rp_spmm *e)
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

// ---- the transposed matrices (crp_rp_spmm_exec_t_ex, crp_rp_spmm_attention_bwd_ex) -----------------------------------------------
// First call: the two-source local matrix, its remote columns renumbered behind the local ones, is transposed on the device
// (crp_csr_transpose) and cut by rows into At_loc and At_rem; the rows that come back are grouped by the C row they add to.
static inline void build_transposed(crp_rp_spmm *e)
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

#endif
