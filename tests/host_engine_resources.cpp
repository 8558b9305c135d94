// Who releases what in the two engines (csrc/rp_engine.cpp, csrc/rp_attention.cpp, csrc/rp_gat.cpp, csrc/para2d_engine.cpp, csrc/dev_owned.h), under AddressSanitizer /
// UBSan on the CPU; built and run by tests/test_host_sanitizers.py.  The device ABI is a set of host stand-ins: "device" memory is
// calloc, kernels and matrix handles do no arithmetic, every call is counted, and a free, destroy, copy or stream / event call on
// something that is not live ends the program.  The engines run over crp_comm_self() on a tiny matrix and on one without
// nonzeros; afterwards every create has its destroy and nothing is live.  `--trace` prints the names of the ABI calls in order.
// NOT reached here (only a communicator of several ranks builds them): the interior / boundary split, xstream with ev_packed and
// ev_landed, the parts' position arrays, the second receive buffer, and the 2D engine's state for pn > 1 (the split engine and its
// streams: tests/host_engine_streams.cpp, over the same stand-ins, tests/host_device_standins.h).
#include "host_device_standins.h"

// ---- the owners by themselves ------------------------------------------------------------------------------------------------------
#ifdef HAVE_OWNERS
static int g_comm_freed = 0;
static void counting_free(crp_comm_t *c) { g_comm_freed++; free(c); }
static crp_comm_t *counted_comm()
{
    crp_comm_t *c = (crp_comm_t *) calloc(1, sizeof(crp_comm_t));
    c->free = counting_free;
    return c;
}

template <class O> static void empty_owner(const char *name)
{
    const long c0 = total_calls();
    {
        O a, b(std::move(a)), c;
        c = std::move(b);
        c.reset();
        c.reset();
    }
    CHECK(total_calls() == c0, "an empty %s made %ld ABI calls", name, total_calls() - c0);
}

static void owners()
{
    empty_owner<crp::DevArray<int>>("DevArray");
    empty_owner<crp::DevStream>("DevStream");
    empty_owner<crp::DevEvent>("DevEvent");
    empty_owner<crp::DevCsr>("DevCsr");
    empty_owner<crp::OwnedComm>("OwnedComm");
    empty_owner<crp::HostPinned>("HostPinned");
    {
        const long c0 = total_calls();
        crp::DevScratch a, b(std::move(a)), c;
        c = std::move(b);
        c.release();
        CHECK(total_calls() == c0, "an empty DevScratch made ABI calls");
    }
    // moving hands the resource over, the source releases nothing; reset() twice frees once
    {
        const int host[3] = {1, 2, 3};
        crp::DevArray<int> a;
        a.upload(host, 3, NULL);
        CHECK(a[2] == 3 && calls("dev_malloc") == 1 && calls("dev_memcpy") == 1 && calls("stream_sync") == 1, "upload: allocate, copy, sync");
        int *p = a;
        crp::DevArray<int> b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == p && calls("dev_free") == 0, "move construction");
        crp::DevArray<int> c;
        c.zeroed(2);
        CHECK(c[1] == 0 && calls("dev_memset") == 1 && calls("stream_sync") == 2, "zeroed: allocate, memset, sync");
        c = std::move(b);      // releases c's own block, takes b's
        CHECK(b.get() == nullptr && c.get() == p && calls("dev_free") == 1, "move assignment");
        c.reset();
        c.reset();
        CHECK(calls("dev_free") == 2 && calls("dev_free(null)") == 0 && g_dev.empty(), "reset() twice frees once");
    }
    CHECK(calls("dev_malloc") == 2 && calls("dev_free") == 2, "DevArray: %ld allocations, %ld frees", calls("dev_malloc"), calls("dev_free"));
    {
        crp::DevStream s, s2;
        crp::DevEvent ev;
        void *h = s.ensure();
        CHECK(s.ensure() == h && calls("stream_create") == 1, "ensure() creates once");
        ev.ensure();
        ev.ensure();
        s2 = std::move(s);
        CHECK((void *) s == nullptr && (void *) s2 == h && calls("stream_destroy") == 0, "a moved stream");
        crp::DevCsr A, B;
        const int rp[2] = {0, 0};
        crp_csr_dev_create(1, 1, rp, rp, NULL, A.out());
        B = std::move(A);
        CHECK((crp_csr_dev_p) A == nullptr && (crp_csr_dev_p) B != nullptr, "a moved matrix");
        crp::HostPinned hp, hp2;
        hp.alloc(8);
        hp2 = std::move(hp);
        crp::OwnedComm c1(counted_comm()), c2(std::move(c1));
        c1.reset();
        CHECK(g_comm_freed == 0, "a moved-from communicator owner freed something");
    }
    CHECK(g_comm_freed == 1 && calls("event_create") == 1, "communicator freed %d times, %ld events", g_comm_freed, calls("event_create"));
    check_balanced("owners");
    // DevScratch: grow-only, one allocation per growth, the old block freed first; release() frees once
    {
        g_calls.clear();
        crp::DevScratch sc;
        sc.grow<double>(10);
        CHECK(calls("dev_malloc") == 1 && total_calls() == 1, "first growth");
        sc.grow<float>(20);      // 80 bytes: fits
        sc.grow<double>(5);
        CHECK(total_calls() == 1, "no growth needed");
        sc.grow<double>(11);
        CHECK(calls("dev_malloc") == 2 && calls("dev_free") == 1 && total_calls() == 3, "second growth");
        sc.release();
        sc.release();
        CHECK(calls("dev_free") == 2 && total_calls() == 4, "release() twice frees once");
        sc.grow<double>(1);      // ... and the destructor releases what is left
    }
    check_balanced("DevScratch");
    g_calls.clear();
}
#endif

// ---- the engines ------------------------------------------------------------------------------------------------------------------
struct Matrix { int m; std::vector<int> rp, ci; std::vector<double> va; };
static const int N = 3;      // width of the dense operands

template <class T> struct DevBuf      // a caller's device array
{
    T *p = nullptr;
    explicit DevBuf(size_t n) { void *d; crp_dev_malloc(&d, sizeof(T) * (n ? n : 1)); p = (T *) d; }
    ~DevBuf() { crp_dev_free(p); }
};

template <class T> static void dense_ops(crp_rp_spmm_p e, const Matrix &A, int layout, void (*exec)(crp_rp_spmm_p, int, const T *, long long, T *, long long, void *),
                                         void (*sddmm)(crp_rp_spmm_p, int, const T *, long long, const T *, long long, T *, int, void *),
                                         void (*attention)(crp_rp_spmm_p, int, double, int, const T *, long long, const T *, long long, const T *,
                                                           long long, T *, long long, T *, T *, void *),
                                         int which)
{
    const int m = A.m, ld = layout == 0 ? N : m;
    const size_t nnz = A.va.size();
    std::vector<T> B((size_t) m * N, (T) 1), C((size_t) m * N), Q(B), V(B), lse((size_t) m + 1), out(nnz + 1);
    if (which == 0) exec(e, layout, B.data(), ld, C.data(), ld, NULL);
    if (which == 1) sddmm(e, layout, C.data(), ld, B.data(), ld, out.data(), 0, NULL);
    if (which == 2) attention(e, layout, 0.5, 1, Q.data(), ld, B.data(), ld, V.data(), ld, C.data(), ld, lse.data(), out.data(), NULL);
}

// the multi-head attention with host operands: N heads of one column each, lse and p_out with an entry per head
template <class T> static void attention_mh(crp_rp_spmm_p e, const Matrix &A, int layout,
                                            void (*call)(crp_rp_spmm_p, int, int, double, int, const T *, long long, const T *, long long, const T *,
                                                         long long, T *, long long, T *, T *, void *))
{
    const int m = A.m, ld = layout == 0 ? N : m, heads = N;
    std::vector<T> K((size_t) m * N, (T) 1), O((size_t) m * N), Q(K), V(K), lse((size_t) m * heads + 1), out(A.va.size() * heads + 1);
    call(e, layout, heads, 0.5, 1, Q.data(), ld, K.data(), ld, V.data(), ld, O.data(), ld, lse.data(), out.data(), NULL);
}

// every operation once per dtype (the dense ones with host operands in both layouts); dev_update_first: the first device value
// update comes before the first exec_t (its scratch for the transposed matrices is then built by the second one) or after it
static void full_engine(const Matrix &A, bool dev_update_first)
{
    const int displs[2] = {0, A.m};
    crp_comm_t *comm = crp_comm_self();
    crp_rp_spmm_p e = NULL;
    const size_t nnz = A.va.size();
    crp_rp_spmm_init(0, A.m, A.rp.data(), A.ci.data(), A.va.data(), displs, N, comm, &e);
    DevBuf<double> v64(nnz), w64(nnz), u64(nnz);
    DevBuf<float> v32(nnz), w32(nnz), u32(nnz);
    auto exec_t = [&] {
        for (int layout = 0; layout < 2; layout++)
        {
            dense_ops<double>(e, A, layout, crp_rp_spmm_exec_t_ex, nullptr, nullptr, 0);
            dense_ops<float>(e, A, layout, crp_rp_spmm_exec_t_f32_ex, nullptr, nullptr, 0);
        }
    };
    for (int layout = 0; layout < 2; layout++)
    {
        dense_ops<double>(e, A, layout, crp_rp_spmm_exec_ex, nullptr, nullptr, 0);
        dense_ops<float>(e, A, layout, crp_rp_spmm_exec_f32_ex, nullptr, nullptr, 0);
    }
    if (dev_update_first) crp_rp_spmm_update_values_dev(e, v64.p, 0, NULL);
    exec_t();
    for (int layout = 0; layout < 2; layout++)
    {
        dense_ops<double>(e, A, layout, nullptr, crp_rp_spmm_sddmm_ex, nullptr, 1);
        dense_ops<float>(e, A, layout, nullptr, crp_rp_spmm_sddmm_f32_ex, nullptr, 1);
    }
    crp_rp_spmm_update_values(e, A.va.data());
    if (!dev_update_first) crp_rp_spmm_update_values_dev(e, v64.p, 0, NULL);
    crp_rp_spmm_update_values_dev(e, v32.p, 1, NULL);
    exec_t();      // (the host values are stale by now: refreshed from the device first)
    crp_rp_spmm_row_softmax_ex(e, v64.p, w64.p, 0, NULL);
    crp_rp_spmm_row_softmax_ex(e, v32.p, w32.p, 1, NULL);
    crp_rp_spmm_row_softmax_bwd_ex(e, w64.p, v64.p, u64.p, 0, NULL);
    crp_rp_spmm_row_softmax_bwd_ex(e, w32.p, v32.p, u32.p, 1, NULL);
    for (int layout = 0; layout < 2; layout++)
    {
        dense_ops<double>(e, A, layout, nullptr, nullptr, crp_rp_spmm_attention_ex, 2);
        dense_ops<float>(e, A, layout, nullptr, nullptr, crp_rp_spmm_attention_f32_ex, 2);
    }
    for (int layout = 0; layout < 2; layout++)
    {
        attention_mh<double>(e, A, layout, crp_rp_spmm_attention_mh_ex);
        attention_mh<float>(e, A, layout, crp_rp_spmm_attention_mh_f32_ex);
    }
    // the GAT and GATv2 forward (csrc/rp_gat.cpp): el, er, XT and a on the device, V, O, lse and p_out on the host; one GAT call per
    // dtype, one with another number of heads (the narrow exchange is set up again), one GATv2 call
    {
        const size_t mN = (size_t) A.m * N;
        DevBuf<double> el(mN), er(mN), XT(mN), av(N);
        DevBuf<float> elf(mN), erf(mN);
        std::vector<double> V(mN, 1.0), O(mN), lse(mN + 1), p(nnz * N + 1);
        std::vector<float> Vf(mN, 1.0f), Of(mN), lsef(mN + 1), pf(nnz * N + 1);
        crp_rp_spmm_gat_ex(e, 0, N, 0.2, 1, el.p, N, er.p, N, V.data(), N, O.data(), N, lse.data(), p.data(), NULL);
        crp_rp_spmm_gat_f32_ex(e, 1, N, 0.2, 1, elf.p, N, erf.p, N, Vf.data(), A.m, Of.data(), A.m, lsef.data(), pf.data(), NULL);
        crp_rp_spmm_gat_ex(e, 1, 1, 0.2, 0, el.p, N, er.p, N, V.data(), A.m, O.data(), A.m, lse.data(), p.data(), NULL);
        crp_rp_spmm_gat_ex(e, 0, N, 0.2, 1, el.p, N, er.p, N, V.data(), N, O.data(), N, lse.data(), p.data(), NULL);
        crp_rp_spmm_gatv2_ex(e, 0, N, 0.2, 1, XT.p, N, av.p, V.data(), N, O.data(), N, lse.data(), p.data(), NULL);
        CHECK(crp_rp_spmm_gat_built(e) == 1 && crp_rp_spmm_gatv2_built(e) == 1, "the GAT calls built nothing");
    }
    // device operands with timing off: the exec returns asynchronously and leaves its event behind
    {
        DevBuf<double> B((size_t) A.m * N), C((size_t) A.m * N);
        crp_rp_spmm_set_timing(e, 0);
        crp_rp_spmm_exec_ex(e, 0, B.p, N, C.p, N, NULL);
        crp_rp_spmm_update_values(e, A.va.data());
    }
    crp_rp_spmm_free(&e);
    CHECK(e == NULL, "free leaves the handle NULL");
    crp_rp_spmm_free(&e);
    comm->free(comm);
}

static void para2d_engine(const Matrix &A)
{
    const int A0_rowptr[2] = {0, A.m}, ptr[2] = {0, A.m}, colptr[2] = {0, N};
    crp_comm_t *comm = crp_comm_self();
    crp_para2d_spmm_p e = NULL;
    const size_t nnz = A.va.size();
    crp_para2d_spmm_init(comm, 1, 1, A0_rowptr, ptr, ptr, colptr, A.rp.data(), A.ci.data(), A.va.data(), &e);
    std::vector<double> B((size_t) A.m * N, 1.0), C((size_t) A.m * N), out(nnz + 1);
    DevBuf<double> v(nnz), w(nnz);
    crp_para2d_spmm_exec_ex(e, 0, B.data(), N, C.data(), N, NULL);
    crp_para2d_spmm_exec_t_ex(e, 1, B.data(), A.m, C.data(), A.m, NULL);
    crp_para2d_spmm_sddmm_ex(e, 0, C.data(), N, B.data(), N, out.data(), 0, NULL);
    crp_para2d_spmm_update_values(e, A.va.data());
    crp_para2d_spmm_update_values_dev(e, v.p, 0, NULL);
    crp_para2d_spmm_row_softmax_ex(e, v.p, w.p, 0, NULL);
    crp_para2d_spmm_free(&e);
    CHECK(e == NULL, "free leaves the handle NULL");
    comm->free(comm);
}

static void plan_only(const Matrix &A)
{
    const int displs[2] = {0, A.m}, colptr[2] = {0, N};
    crp_comm_t *comm = crp_comm_self();
    const long c0 = total_calls();
    crp_rp_spmm_p e = NULL;
    crp_rp_spmm_init_plan_only(0, A.m, A.rp.data(), A.ci.data(), A.va.data(), displs, N, comm, &e);
    crp_rp_spmm_update_values(e, A.va.data());
    crp_rp_spmm_free(&e);
    crp_para2d_spmm_p e2 = NULL;
    crp_para2d_spmm_init_plan_only(comm, 1, 1, displs, displs, displs, colptr, A.rp.data(), A.ci.data(), A.va.data(), &e2);
    crp_para2d_spmm_free(&e2);
    CHECK(total_calls() == c0, "plan-only engines made %ld device ABI calls", total_calls() - c0);
    comm->free(comm);
}

int main(int argc, char **argv)
{
#ifdef HAVE_OWNERS
    owners();
#endif
    g_trace = argc > 1 && strcmp(argv[1], "--trace") == 0;
    // 4 x 4, rows of 2, 0, 3 and 1 entries; and 3 rows without a nonzero (the arrays still valid pointers)
    const Matrix tiny{4, {0, 2, 2, 5, 6}, {0, 3, 1, 2, 3, 0}, {1, 2, 3, 4, 5, 6}};
    Matrix empty_{3, {0, 0, 0, 0}, {}, {}};
    empty_.ci.reserve(1);
    empty_.va.reserve(1);
    const Matrix &empty = empty_;
    int runs = 0;
    for (const Matrix *A : {&tiny, &empty})
    {
        plan_only(*A);
        for (int first = 0; first < 2; first++, runs++)
        {
            full_engine(*A, first != 0);
            check_balanced("row engine");
        }
        para2d_engine(*A);
        check_balanced("2D engine");
    }
    CHECK(calls("dev_malloc") > 0 && calls("stream_create") >= runs && calls("event_create") > 0 && calls("csr_dev_create") >= 2 * runs,
          "the engines did not run: %ld allocations", calls("dev_malloc"));
    printf("HOST_ENGINE_RESOURCES_OK runs=%d allocations=%ld streams=%ld events=%ld matrices=%ld\n", runs, calls("dev_malloc"),
           calls("stream_create"), calls("event_create"), calls("csr_dev_create"));
    return 0;
}
