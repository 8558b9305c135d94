// The ORDER of the row-parallel engine's device work across streams (csrc/rp_engine.cpp, csrc/rp_attention.cpp, csrc/rp_gat.cpp), checked on the
// CPU under AddressSanitizer / UBSan; built and run by tests/test_host_sanitizers.py.  The device ABI is the set of host stand-ins of
// tests/host_device_standins.h, which log every call as (call, stream, buffers read, buffers written) and every event record and wait.
// A single-threaded fake communicator plays rank 0 of 2: it answers the plan's alltoall_i32 / alltoallv_i32 with fabricated but
// valid requests from the peer and logs alltoallv_dev_f64 as "read send, write recv" on its stream -- so the engine is SPLIT into
// interior and boundary rows and takes the xstream / ev_packed / ev_landed paths that one rank never reaches.  The caller's stream is
// a token of its own, distinct from the engine's streams and from the null stream.
//
// The log is replayed with vector clocks.  Ordering edges: the order of a stream's own work, event record -> wait, and a stream
// synchronisation (the host has seen everything on that stream; what it enqueues afterwards comes later).  Asserted: every read of
// a buffer is ordered after its last write, every write after all earlier reads and writes.  A buffer is a whole live block or a
// matrix handle (its values), so the check is conservative.  Negative control: the same checker on the same log with one
// stream_wait_event removed must report a race.  This is the only place the overlap path's order can be checked without several
// devices; it says nothing about what a real transport does inside alltoallv_dev_f64.
//
// The call list runs twice, each time on a fresh engine: with timing off (the overlap path; every check above) and with the phases
// timed (everything in sequence on the caller's stream; the race checker again).  `--dump` prints both logs as text, one op per line
// with streams, events and buffers numbered in order of first appearance: the dumps of two builds of csrc/ compare with diff.
#include "host_device_standins.h"

// ---- rank 0 of 2 -------------------------------------------------------------------------------------------------------------
struct FakeCtx { int lo, hi, wanted; };      // my block of B rows, and how many of them the peer asks for

static void f_alltoall(void *ctx, const int *send, int *recv, int count)
{
    CHECK(count == 1, "alltoall_i32 with count %d", count);
    recv[0] = send[0];
    recv[1] = ((FakeCtx *) ctx)->wanted;
}
static void f_alltoallv(void *ctx, const int *send, const int *scnts, const int *sdispls, int *recv, const int *rcnts, const int *rdispls)
{
    const FakeCtx *c = (const FakeCtx *) ctx;
    for (int i = 0; i < rcnts[0]; i++) recv[rdispls[0] + i] = send[sdispls[0] + i];
    CHECK(scnts[0] == rcnts[0] && rcnts[1] == c->wanted && rcnts[1] <= c->hi - c->lo, "the plan's counts");
    for (int i = 0; i < rcnts[1]; i++) recv[rdispls[1] + i] = c->hi - 1 - i;      // the peer wants my last rows
}
static void f_allgatherv(void *, const void *send, size_t sbytes, void *recv, const size_t *, const size_t *rdispls)
{
    if (sbytes) memcpy((char *) recv + rdispls[0], send, sbytes);
}
static void f_barrier(void *) {}
static void f_reduce_f64(void *, const double *in, double *out, int count, int) { memcpy(out, in, sizeof(double) * (size_t) count); }
static void f_reduce_u64(void *, const uint64_t *in, uint64_t *out, int count, int) { memcpy(out, in, sizeof(uint64_t) * (size_t) count); }
static void f_exchange(void *, const double *send_dev, const long long *scnts, const long long *, double *recv_dev, const long long *rcnts,
                       const long long *, void *stream)
{
    live_stream(stream);
    log_op(OP_WORK, "alltoallv_dev_f64", stream, NULL, {R{scnts[1] > 0 ? send_dev : NULL}}, {W{rcnts[1] > 0 ? recv_dev : NULL}});
    hit("alltoallv_dev_f64");
}
static void f_free(crp_comm_t *) {}

// ---- the replay ----------------------------------------------------------------------------------------------------------------
typedef std::map<void *, long> Clock;      // stream -> count of its operations that have happened
static void join(Clock &a, const Clock &b)
{
    for (auto &kv : b)
        if (a[kv.first] < kv.second) a[kv.first] = kv.second;
}
struct Access { void *stream; long tick; const char *call; size_t index; };
static bool before(const Access &a, const Clock &now)
{
    auto it = now.find(a.stream);
    return it != now.end() && a.tick <= it->second;
}
struct Race { size_t first, second; const void *buffer; };

// every pair of conflicting accesses that the log does not order; skip_wait: the index of a wait to leave out (the negative control)
static std::vector<Race> races(const std::vector<Op> &log, size_t skip_wait = (size_t) -1)
{
    std::map<void *, Clock> at;                  // the clock of every stream (key NULL: the null stream)
    std::map<void *, Clock> recorded;            // the clock an event was last recorded at
    Clock host;                                  // what the host has waited for
    std::map<const void *, Access> last_write;
    std::map<const void *, std::vector<Access>> reads_since;
    std::vector<Race> out;
    for (size_t i = 0; i < log.size(); i++)
    {
        const Op &op = log[i];
        if (op.kind == OP_FORGET)
        {
            for (const void *b : op.writes) { last_write.erase(b); reads_since.erase(b); }
            continue;
        }
        Clock &c = at[op.stream];
        join(c, host);                           // enqueued now: after everything the host has waited for
        if (op.kind == OP_SYNC) { join(host, c); continue; }
        if (op.kind == OP_WAIT)
        {
            if (i != skip_wait && recorded.count(op.event)) join(c, recorded[op.event]);
            continue;
        }
        const long tick = ++c[op.stream];
        if (op.kind == OP_RECORD) { recorded[op.event] = c; continue; }
        const Access me{op.stream, tick, op.call, i};
        for (const void *b : op.reads)
            if (last_write.count(b) && !before(last_write[b], c)) out.push_back(Race{last_write[b].index, i, b});
        for (const void *b : op.writes)
        {
            if (last_write.count(b) && !before(last_write[b], c)) out.push_back(Race{last_write[b].index, i, b});
            for (const Access &r : reads_since[b])
                if (r.index != i && !before(r, c)) out.push_back(Race{r.index, i, b});
        }
        for (const void *b : op.reads) reads_since[b].push_back(me);
        for (const void *b : op.writes) { last_write[b] = me; reads_since[b].clear(); }
    }
    return out;
}

// ---- the engine's calls ----------------------------------------------------------------------------------------------------------
template <class T> struct Dev      // a caller's device array
{
    T *p = nullptr;
    explicit Dev(size_t n) { void *d; crp_dev_malloc(&d, sizeof(T) * (n ? n : 1)); p = (T *) d; }
    ~Dev() { crp_dev_free(p); }
};

// ---- one pass over the call list ---------------------------------------------------------------------------------------------------
struct Pass
{
    void *caller = NULL, *caller2 = NULL;                  // the caller's streams (tokens: destroyed by the end of the pass)
    std::vector<std::pair<size_t, size_t>> gat_calls;      // the log's [first, end) of every GAT / GATv2 call
    size_t probe = 0;                                      // ... and which of them the GAT negative control takes apart
};

// a fresh split engine, every call of the list with this timing mode, the engine freed; g_log holds the log of it all, from empty
static Pass run_calls(int timing)
{
    // 4 of 8 rows on rank 0, B rows 0 .. 3 here and 4 .. 7 on the peer; rows 0 and 1 name local columns only (interior), rows 2 and 3
    // name columns of the peer (boundary)
    const int m = 4, N = 3, displs[3] = {0, 4, 8};
    const std::vector<int> rp{0, 2, 4, 7, 9}, ci{0, 1, 1, 3, 2, 4, 6, 0, 7};
    const std::vector<double> va{1, 2, 3, 4, 5, 6, 7, 8, 9};
    const size_t nnz = va.size();
    FakeCtx fc{0, 4, 2};
    crp_comm_t comm;
    memset(&comm, 0, sizeof(comm));
    comm.ctx = &fc; comm.nproc = 2; comm.rank = 0;
    comm.alltoall_i32 = f_alltoall; comm.alltoallv_i32 = f_alltoallv; comm.allgatherv_bytes = f_allgatherv; comm.barrier = f_barrier;
    comm.reduce_f64 = f_reduce_f64; comm.reduce_u64 = f_reduce_u64; comm.alltoallv_dev_f64 = f_exchange; comm.free = f_free;

    g_log.clear();
    g_logging = true;
    crp_rp_spmm_p e = NULL;
    crp_rp_spmm_init(0, m, rp.data(), ci.data(), va.data(), displs, N, &comm, &e);
    int n_int = 0, n_bnd = 0;
    crp_rp_spmm_overlap_rows(e, &n_int, &n_bnd);
    CHECK(n_int == 2 && n_bnd == 2, "the engine is not split: %d interior, %d boundary rows", n_int, n_bnd);
    crp_rp_spmm_set_timing(e, timing);
    Pass pass;
    void *&caller = pass.caller, *&caller2 = pass.caller2;
    std::vector<std::pair<size_t, size_t>> &gat_calls = pass.gat_calls;
    size_t &probe = pass.probe;
    crp_stream_create(&caller);
    crp_stream_create(&caller2);
    {
        Dev<double> B((size_t) m * N), C((size_t) m * N), X((size_t) m * N), Ct((size_t) m * N), out(nnz), Q((size_t) m * N), K((size_t) m * N),
            V((size_t) m * N), O((size_t) m * N), lse(m), p(nnz), dO((size_t) m * N), dQ((size_t) m * N), dK((size_t) m * N), dV((size_t) m * N),
            ds(nnz), vals(nnz), vals2(nnz), lse_mh((size_t) m * N), p_mh(nnz * N), ds_mh(nnz * N);      // (_mh: N heads of one column)
        Dev<float> Bf((size_t) m * N), Cf((size_t) m * N), Xf((size_t) m * N), outf(nnz), valsf(nnz);
        // the GAT and GATv2 calls' own operands: el, er (N heads, one scalar each), XT and a; fp32 lse and p_out for N heads
        Dev<double> el((size_t) m * N), er((size_t) m * N), XT((size_t) m * N), av(N);
        Dev<float> elf((size_t) m * N), erf((size_t) m * N), XTf((size_t) m * N), avf(N), lsef((size_t) m * N), pf(nnz * N);
        // what the caller wrote before: on the caller's stream (the engine must order its other streams after it)
        for (double *b : {B.p, X.p, Q.p, K.p, V.p, dO.p, vals.p, el.p, er.p, XT.p, av.p}) crp_dev_memset(b, 0, 8, caller);
        for (float *b : {Bf.p, Xf.p, valsf.p, elf.p, erf.p, XTf.p, avf.p}) crp_dev_memset(b, 0, 4, caller);
        // (heads == N in the rounds; the heads sequence below also passes 1: the buffers hold N entries per row either way)
        auto gat = [&](int heads, void *s) {
            const size_t lo = g_log.size();
            crp_rp_spmm_gat_ex(e, 0, heads, 0.2, 1, el.p, N, er.p, N, V.p, N, O.p, N, lse_mh.p, p_mh.p, s);
            gat_calls.push_back({lo, g_log.size()});
        };
        auto gat_f32 = [&](int heads, void *s) {
            const size_t lo = g_log.size();
            crp_rp_spmm_gat_f32_ex(e, 0, heads, 0.2, 1, elf.p, N, erf.p, N, Bf.p, N, Cf.p, N, lsef.p, pf.p, s);
            gat_calls.push_back({lo, g_log.size()});
        };
        auto round_of_calls = [&](void *s) {
            crp_rp_spmm_exec_ex(e, 0, B.p, N, C.p, N, s);
            crp_rp_spmm_exec_f32_ex(e, 0, Bf.p, N, Cf.p, N, s);
            crp_rp_spmm_exec_t_ex(e, 0, X.p, N, Ct.p, N, s);
            crp_rp_spmm_exec_t_f32_ex(e, 0, Xf.p, N, Cf.p, N, s);
            crp_rp_spmm_sddmm_ex(e, 0, X.p, N, B.p, N, out.p, 1, s);
            crp_rp_spmm_sddmm_f32_ex(e, 0, Xf.p, N, Bf.p, N, outf.p, 1, s);
            crp_rp_spmm_attention_ex(e, 0, 0.5, 1, Q.p, N, K.p, N, V.p, N, O.p, N, lse.p, p.p, s);
            crp_rp_spmm_attention_bwd_ex(e, 0.5, 1, Q.p, N, K.p, N, V.p, N, O.p, N, dO.p, N, lse.p, dQ.p, N, dK.p, N, dV.p, N, ds.p, s);
            crp_rp_spmm_attention_mh_ex(e, 0, N, 0.5, 1, Q.p, N, K.p, N, V.p, N, O.p, N, lse_mh.p, p_mh.p, s);
            crp_rp_spmm_attention_bwd_mh_ex(e, N, 0.5, 1, Q.p, N, K.p, N, V.p, N, O.p, N, dO.p, N, lse_mh.p, dQ.p, N, dK.p, N, dV.p, N, ds_mh.p, s);
            gat(N, s);
            gat_f32(N, s);
            const size_t lo = g_log.size();
            crp_rp_spmm_gatv2_ex(e, 0, N, 0.2, 1, XT.p, N, av.p, V.p, N, O.p, N, lse_mh.p, p_mh.p, s);
            crp_rp_spmm_gatv2_f32_ex(e, 0, N, 0.2, 1, XTf.p, N, avf.p, Bf.p, N, Cf.p, N, lsef.p, pf.p, s);
            gat_calls.push_back({lo, g_log.size()});
        };
        round_of_calls(caller);                                  // the first calls build what they need
        round_of_calls(caller);                                  // steady state
        crp_rp_spmm_update_values(e, va.data());                 // a host update behind execs in flight on the caller's stream
        round_of_calls(caller);
        crp_rp_spmm_update_values_dev(e, vals.p, 0, caller);     // a device update on the caller's stream, then more work there
        crp_rp_spmm_update_values_dev(e, valsf.p, 1, caller);
        round_of_calls(caller);
        crp_rp_spmm_update_values(e, va.data());                 // ... and a host update behind the device update
        round_of_calls(caller);
        // a second caller stream: the caller orders its own buffers (it waits for the first), the engine orders its values
        crp_stream_sync(caller);
        crp_dev_memset(vals2.p, 0, 8, caller2);
        crp_rp_spmm_update_values_dev(e, vals2.p, 0, caller2);
        round_of_calls(caller2);
        crp_stream_sync(caller2);
        crp_rp_spmm_update_values_dev(e, vals.p, 0, caller);     // ... and back: after an update on another stream
        round_of_calls(caller);
        // other numbers of heads behind work in flight on the caller's stream: every call frees the narrow send and receive
        // buffers, allocates them again and zero-fills them on the null stream; then one steady-state call (the negative control's)
        for (int heads : {1, N})
        {
            gat(heads, caller);
            gat_f32(heads, caller);
        }
        round_of_calls(caller);
        probe = gat_calls.size();
        gat(N, caller);
        crp_stream_sync(caller);
        crp_stream_sync(caller2);
    }
    crp_rp_spmm_free(&e);
    crp_stream_destroy(caller);
    crp_stream_destroy(caller2);
    g_logging = false;
    check_balanced("split row engine");
    return pass;
}

// the log as text, one op per line: kind, call, stream, event, buffers read, buffers written.  Streams, events and buffers are named
// by their index in order of first appearance (a freed buffer's address gets a new index when it appears again), so the dumps of
// two builds compare as text
static void dump(const char *title, const std::vector<Op> &log)
{
    static const char *const kinds[] = {"work", "record", "wait", "sync", "forget"};
    std::map<const void *, size_t> streams, events, buffers;
    size_t n_buffers = 0;
    auto name = [](std::map<const void *, size_t> &ids, const void *p) { return ids.emplace(p, ids.size()).first->second; };
    printf("# %s: %zu ops\n", title, log.size());
    for (const Op &op : log)
    {
        printf("%s %s", kinds[op.kind], op.call);
        if (op.kind == OP_FORGET)
        {
            for (const void *b : op.writes)
            {
                if (buffers.count(b)) printf(" b%zu", buffers[b]);
                buffers.erase(b);
            }
            printf("\n");
            continue;
        }
        if (op.stream == NULL) printf(" s-null");
        else printf(" s%zu", name(streams, op.stream));
        if (op.event != NULL) printf(" e%zu", name(events, op.event));
        for (int w = 0; w < 2; w++)
        {
            printf(w == 0 ? " r:" : " w:");
            for (const void *b : w == 0 ? op.reads : op.writes)
            {
                if (!buffers.count(b)) buffers[b] = n_buffers++;
                printf(" b%zu", buffers[b]);
            }
        }
        printf("\n");
    }
}

static void report(const char *pass, const std::vector<Op> &log, const std::vector<Race> &found)
{
    for (size_t i = 0; i < found.size() && i < 10; i++)
        fprintf(stderr, "%s: race: #%zu %s (stream %p) and #%zu %s (stream %p) on buffer %p\n", pass, found[i].first, log[found[i].first].call,
                log[found[i].first].stream, found[i].second, log[found[i].second].call, log[found[i].second].stream, found[i].buffer);
}

// `--dump`: the two passes' logs on stdout, ahead of the checks
int main(int argc, char **argv)
{
    // the timed pass first, its log set aside: g_log then holds the pass with timing off, which the checks below were written for
    const Pass timed = run_calls(1);
    std::vector<Op> timed_log;
    timed_log.swap(g_log);
    const Pass off = run_calls(0);
    void *const caller = off.caller, *const caller2 = off.caller2;
    const std::vector<std::pair<size_t, size_t>> &gat_calls = off.gat_calls;
    const size_t probe = off.probe;
    if (argc > 1 && strcmp(argv[1], "--dump") == 0)
    {
        dump("timing off", g_log);
        dump("timing on", timed_log);
    }

    // ---- the log reached the overlap path, and it is ordered
    std::set<void *> work_streams;
    long exchanges = 0, waits = 0;
    for (const Op &op : g_log)
    {
        if (op.kind == OP_WORK) work_streams.insert(op.stream);
        if (op.kind == OP_WORK && strcmp(op.call, "alltoallv_dev_f64") == 0 && op.stream != caller && op.stream != caller2) exchanges++;
        if (op.kind == OP_WAIT) waits++;
    }
    CHECK(work_streams.count(caller) && work_streams.count(caller2) && work_streams.size() >= 4, "work on %zu streams only", work_streams.size());
    CHECK(exchanges > 0 && waits > 0, "no exchange on the engine's second stream (%ld) or no wait (%ld)", exchanges, waits);
    const std::vector<Race> found = races(g_log);
    report("timing off", g_log, found);
    CHECK(found.empty(), "%zu unordered pairs of conflicting accesses", found.size());

    // ---- the same calls with the phases timed: everything in sequence on the caller's stream, so no exchange leaves it, and what
    // the engine's own streams do beside it (first-call uploads, value updates) is ordered all the same
    long timed_exchanges = 0;
    for (const Op &op : timed_log)
    {
        if (op.kind != OP_WORK || strcmp(op.call, "alltoallv_dev_f64") != 0) continue;
        CHECK(op.stream == timed.caller || op.stream == timed.caller2, "a timed exchange off the caller's stream");
        timed_exchanges++;
    }
    CHECK(timed_exchanges > 0, "the timed pass made no exchange");
    const std::vector<Race> timed_found = races(timed_log);
    report("timing on", timed_log, timed_found);
    CHECK(timed_found.empty(), "timing on: %zu unordered pairs of conflicting accesses", timed_found.size());

    // ---- negative control: without its first wait for the exchange stream, the caller's stream races with the exchange
    std::map<void *, void *> recorded_on;
    size_t victim = (size_t) -1;
    long needed = 0, cross = 0;
    for (size_t i = 0; i < g_log.size(); i++)
    {
        const Op &op = g_log[i];
        if (op.kind == OP_RECORD) recorded_on[op.event] = op.stream;
        if (op.kind != OP_WAIT || !recorded_on.count(op.event) || recorded_on[op.event] == op.stream) continue;
        cross++;
        if (!races(g_log, i).empty()) needed++;
        if (victim == (size_t) -1 && op.stream == caller && recorded_on[op.event] != caller2) victim = i;
    }
    CHECK(victim != (size_t) -1, "the caller's stream never waits for an engine stream");
    const std::vector<Race> broken = races(g_log, victim);
    CHECK(!broken.empty(), "the checker does not see the race of a log without wait #%zu", victim);

    // ---- the GAT and GATv2 calls (csrc/rp_gat.cpp) reached the overlap path: exchanges on the engine's second stream and
    // cross-stream waits inside their stretches of the log; the heads sequence set the narrow buffers up again
    long gat_exchanges = 0, gat_waits = 0, gat_zero_fills = 0;
    for (const std::pair<size_t, size_t> &call : gat_calls)
        for (size_t i = call.first; i < call.second; i++)
        {
            const Op &op = g_log[i];
            if (op.kind == OP_WORK && strcmp(op.call, "alltoallv_dev_f64") == 0 && op.stream != caller && op.stream != caller2) gat_exchanges++;
            if (op.kind == OP_WORK && strcmp(op.call, "dev_memset") == 0 && op.stream == NULL) gat_zero_fills++;
            if (op.kind == OP_WAIT && recorded_on.count(op.event) && recorded_on[op.event] != op.stream) gat_waits++;
        }
    CHECK(gat_exchanges > 0 && gat_waits > 0, "the GAT calls made no exchange on the engine's second stream (%ld) or no wait (%ld)", gat_exchanges,
          gat_waits);
    // both dtypes, both buffers: the first call and the two calls with another number of heads
    CHECK(gat_zero_fills == 2 * 2 * 3, "the narrow buffers were zero-filled %ld times", gat_zero_fills);

    // ---- negative control of the GAT call: one steady-state call packs and exchanges V, then er, on the engine's second stream; the
    // caller's stream then waits for both.  Without that wait the boundary kernel races with the exchanges, and one of the buffers
    // is the narrow receive buffer, which the call's SECOND alltoallv_dev_f64 wrote: the stand-in reads it
    CHECK(probe < gat_calls.size(), "no GAT call for the control");
    const void *narrow_recv = NULL;
    size_t gat_victim = (size_t) -1;
    int seen = 0;
    for (size_t i = gat_calls[probe].first; i < gat_calls[probe].second; i++)
    {
        const Op &op = g_log[i];
        if (op.kind == OP_WORK && strcmp(op.call, "alltoallv_dev_f64") == 0 && ++seen == 2)
        {
            CHECK(op.stream != caller && op.writes.size() == 1, "the GAT call's second exchange");
            narrow_recv = op.writes[0];
        }
        if (op.kind == OP_WAIT && seen == 2 && op.stream == caller && gat_victim == (size_t) -1) gat_victim = i;
    }
    CHECK(seen == 2 && narrow_recv != NULL && gat_victim != (size_t) -1, "the GAT call made %d exchanges, or the caller's stream does not wait", seen);
    const std::vector<Race> gat_broken = races(g_log, gat_victim);
    bool on_narrow = false;
    for (const Race &r : gat_broken)
        if (r.buffer == narrow_recv && strncmp(g_log[r.second].call, "gat_attention_csr", 17) == 0) on_narrow = true;
    CHECK(!gat_broken.empty(), "the checker does not see the race of a GAT call without wait #%zu", gat_victim);
    CHECK(on_narrow, "none of the %zu races without wait #%zu is the boundary kernel's read of the narrow receive buffer", gat_broken.size(), gat_victim);
    printf("HOST_ENGINE_STREAMS_OK ops=%zu streams=%zu exchanges=%ld cross_stream_waits=%ld needed=%ld control_races=%zu gat_calls=%zu "
           "gat_exchanges=%ld gat_cross_stream_waits=%ld gat_zero_fills=%ld gat_control_races=%zu timed_ops=%zu timed_exchanges=%ld\n", g_log.size(),
           work_streams.size(), exchanges, cross, needed, broken.size(), gat_calls.size(), gat_exchanges, gat_waits, gat_zero_fills, gat_broken.size(),
           timed_log.size(), timed_exchanges);
    return 0;
}
