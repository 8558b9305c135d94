// Who releases what in the two engines (csrc/rp_engine.cpp, csrc/para2d_engine.cpp, csrc/dev_owned.h), under AddressSanitizer /
// UBSan on the CPU; built and run by tests/test_host_sanitizers.py.  The device ABI is a set of host stand-ins: "device" memory is
// calloc, kernels and matrix handles do no arithmetic, every call is counted, and a free, destroy, copy or stream / event call on
// something that is not live ends the program.  The engines run over crp_comm_self() on a tiny matrix and on one without
// nonzeros; afterwards every create has its destroy and nothing is live.  `--trace` prints the names of the ABI calls in order.
// NOT reached here (only a communicator of several ranks builds them): the interior / boundary split, xstream with ev_packed and
// ev_landed, the parts' position arrays, the second receive buffer, and the 2D engine's state for pn > 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "crp_engine.h"
#include "crpspmm_hip.h"
#if __has_include("dev_owned.h")
#include "dev_owned.h"
#define HAVE_OWNERS 1
#endif

#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                        \
            fprintf(stderr, "\n");                                               \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

// ---- stand-ins ------------------------------------------------------------------------------------------------------------------
struct crp_csr_dev { int nrow; long long nnz; };

static std::map<const char *, size_t> g_dev;          // live "device" blocks: start -> bytes
static std::set<void *> g_pinned, g_streams, g_events, g_csr;
static std::map<std::string, long> g_calls;
static bool g_trace = false;

static int hit(const char *name)
{
    g_calls[name]++;
    if (g_trace) printf("%s\n", name);
    return 0;
}
static long calls(const char *name) { return g_calls.count(name) ? g_calls[name] : 0; }
static long total_calls()
{
    long t = 0;
    for (auto &kv : g_calls) t += kv.second;
    return t;
}
static bool in_device(const void *p, size_t bytes)
{
    auto it = g_dev.upper_bound((const char *) p);
    if (it == g_dev.begin()) return false;
    --it;
    return (const char *) p + bytes <= it->first + it->second;
}
static void live_stream(void *s) { CHECK(s == NULL || g_streams.count(s), "a stream that is not live"); }
static void live_csr(crp_csr_dev_p A) { CHECK(A != NULL && g_csr.count(A), "a matrix handle that is not live"); }
static int kernel(const char *name, void *stream)
{
    live_stream(stream);
    return hit(name);
}
static int csr_create(const char *name, int nrow, const int *rowptr, crp_csr_dev_p *out)
{
    crp_csr_dev *A = new crp_csr_dev{nrow, rowptr[nrow]};
    g_csr.insert(A);
    *out = A;
    return hit(name);
}

extern "C" {
int crp_dev_malloc(void **p, size_t bytes)
{
    *p = NULL;
    if (bytes == 0) return hit("dev_malloc(0)");      // NULL, as the device ABI gives it: nothing to free
    *p = calloc(bytes, 1);
    g_dev[(const char *) *p] = bytes;
    return hit("dev_malloc");
}
int crp_dev_free(void *p)
{
    if (p == NULL) return hit("dev_free(null)");
    CHECK(g_dev.erase((const char *) p) == 1, "crp_dev_free of a block that is not live");
    free(p);
    return hit("dev_free");
}
int crp_dev_memset(void *p, int v, size_t bytes, void *stream)
{
    live_stream(stream);
    CHECK(bytes == 0 || in_device(p, bytes), "memset outside a live block");
    if (bytes) memset(p, v, bytes);
    return hit("dev_memset");
}
int crp_dev_memcpy(void *dst, const void *src, size_t bytes, int kind, void *stream)
{
    live_stream(stream);
    if (bytes)
    {
        CHECK(kind == 1 || in_device(dst, bytes), "copy into something that is no live block");
        CHECK(kind == 0 || in_device(src, bytes), "copy out of something that is no live block");
        memcpy(dst, src, bytes);
    }
    return hit("dev_memcpy");
}
int crp_dev_memcpy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, int kind, void *stream)
{
    live_stream(stream);
    for (size_t r = 0; r < height && width_bytes > 0; r++)
    {
        CHECK(kind == 1 || in_device((char *) dst + r * dpitch, width_bytes), "2D copy into something that is no live block");
        CHECK(kind == 0 || in_device((const char *) src + r * spitch, width_bytes), "2D copy out of something that is no live block");
        memcpy((char *) dst + r * dpitch, (const char *) src + r * spitch, width_bytes);
    }
    return hit("dev_memcpy2d");
}
int crp_host_malloc(void **p, size_t bytes)
{
    *p = calloc(bytes ? bytes : 1, 1);
    g_pinned.insert(*p);
    return hit("host_malloc");
}
int crp_host_free(void *p)
{
    CHECK(g_pinned.erase(p) == 1, "crp_host_free of a block that is not live");
    free(p);
    return hit("host_free");
}
int crp_dev_ptr_is_device(const void *p, int *is_dev)
{
    *is_dev = (p != NULL && in_device(p, 1)) ? 1 : 0;
    return 0;      // (a query: neither counted nor traced)
}
int crp_stream_create(void **s)
{
    *s = malloc(1);
    g_streams.insert(*s);
    return hit("stream_create");
}
int crp_stream_destroy(void *s)
{
    CHECK(g_streams.erase(s) == 1, "crp_stream_destroy of a stream that is not live");
    free(s);
    return hit("stream_destroy");
}
int crp_stream_sync(void *s) { return kernel("stream_sync", s); }
int crp_event_create(void **ev)
{
    *ev = malloc(1);
    g_events.insert(*ev);
    return hit("event_create");
}
int crp_event_destroy(void *ev)
{
    CHECK(g_events.erase(ev) == 1, "crp_event_destroy of an event that is not live");
    free(ev);
    return hit("event_destroy");
}
int crp_event_record(void *ev, void *s)
{
    CHECK(g_events.count(ev), "record of an event that is not live");
    return kernel("event_record", s);
}
int crp_stream_wait_event(void *s, void *ev)
{
    CHECK(g_events.count(ev), "wait for an event that is not live");
    return kernel("stream_wait_event", s);
}
int crp_csr_dev_create(int nrow, int, const int *rowptr, const int *, const double *, crp_csr_dev_p *out)
{
    return csr_create("csr_dev_create", nrow, rowptr, out);
}
int crp_csr_dev_create_dv(int nrow, int, const int *rowptr, const int *, const double *, const double *, const int *, crp_csr_dev_p *out)
{
    return csr_create("csr_dev_create_dv", nrow, rowptr, out);
}
int crp_csr_dev_destroy(crp_csr_dev_p *A)
{
    if (A == NULL || *A == NULL) return hit("csr_dev_destroy(null)");
    CHECK(g_csr.erase(*A) == 1, "crp_csr_dev_destroy of a handle that is not live");
    delete *A;
    *A = NULL;
    return hit("csr_dev_destroy");
}
int crp_csr_dev_update_values(crp_csr_dev_p A, const double *, void *s) { live_csr(A); return kernel("csr_dev_update_values", s); }
int crp_csr_dev_set_rowmap(crp_csr_dev_p A, const int *, int) { live_csr(A); return hit("csr_dev_set_rowmap"); }
int crp_csr_dev_nrow(crp_csr_dev_p A) { live_csr(A); return A->nrow; }
long long crp_csr_dev_nnz(crp_csr_dev_p A) { live_csr(A); return A->nnz; }
int crp_csr_dev_last_variant(crp_csr_dev_p) { return 0; }
int crp_csr_dev_resolved_variant(crp_csr_dev_p, int) { return 1; }
int crp_csr_dev_reordered(crp_csr_dev_p) { return 0; }
int crp_csr_dev_lattice(crp_csr_dev_p) { return 0; }
int crp_csr_transpose(int nrow, int ncol, const int *rowptr, const int *, const double *, int *rowptr_t, int *colidx_t, double *val_t,
                      int *tmap, void *s)
{
    // zeros: every entry in row 0 of the transpose's first ncol rows is a legal, if wrong, answer for code that only moves it about
    CHECK(in_device(rowptr, sizeof(int) * ((size_t) nrow + 1)) && in_device(rowptr_t, sizeof(int) * ((size_t) ncol + 1)), "transpose outside live blocks");
    const size_t nnz = (size_t) rowptr[nrow];
    memset(rowptr_t, 0, sizeof(int) * ((size_t) ncol + 1));
    CHECK(nnz == 0 || (in_device(colidx_t, sizeof(int) * nnz) && in_device(val_t, sizeof(double) * nnz) && in_device(tmap, sizeof(int) * nnz)),
          "transpose outside live blocks");
    if (nnz) { memset(colidx_t, 0, sizeof(int) * nnz); memset(val_t, 0, sizeof(double) * nnz); memset(tmap, 0, sizeof(int) * nnz); }
    return kernel("csr_transpose", s);
}
int crp_spmm_csr_f64(crp_csr_dev_p A, int, int, const double *, long long, const double *, long long, double *, long long, int, void *s)
{
    live_csr(A);
    return kernel("spmm_csr_f64", s);
}
int crp_spmm_csr_f32(crp_csr_dev_p A, int, const float *, long long, const float *, long long, float *, long long, int, void *s)
{
    live_csr(A);
    return kernel("spmm_csr_f32", s);
}
int crp_sddmm_csr_f64(crp_csr_dev_p A, int, const double *, long long, const double *, long long, const double *, long long, double *,
                      const int *, int, void *s)
{
    live_csr(A);
    return kernel("sddmm_csr_f64", s);
}
int crp_sddmm_csr_f32(crp_csr_dev_p A, int, const float *, long long, const float *, long long, const float *, long long, float *, const int *,
                      int, void *s)
{
    live_csr(A);
    return kernel("sddmm_csr_f32", s);
}
int crp_attention_csr_f64(crp_csr_dev_p A, int, int, double, int, const double *, long long, const double *, long long, const double *,
                          long long, const double *, long long, const double *, long long, double *, long long, double *, double *,
                          const int *, void *s)
{
    live_csr(A);
    return kernel("attention_csr_f64", s);
}
int crp_attention_csr_f32(crp_csr_dev_p A, int, int, double, int, const float *, long long, const float *, long long, const float *, long long,
                          const float *, long long, const float *, long long, float *, long long, float *, float *, const int *, void *s)
{
    live_csr(A);
    return kernel("attention_csr_f32", s);
}
int crp_row_softmax_f64(int, const int *rp, const double *, double *, void *s) { CHECK(in_device(rp, 4), "row pointer"); return kernel("row_softmax_f64", s); }
int crp_row_softmax_f32(int, const int *rp, const float *, float *, void *s) { CHECK(in_device(rp, 4), "row pointer"); return kernel("row_softmax_f32", s); }
int crp_row_softmax_bwd_f64(int, const int *rp, const double *, const double *, double *, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_bwd_f64", s);
}
int crp_row_softmax_bwd_f32(int, const int *rp, const float *, const float *, float *, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_bwd_f32", s);
}
int crp_gather_rows_f64(int, int, int, const int *, const double *, long long, double *, long long, void *s) { return kernel("gather_rows_f64", s); }
int crp_gather_rows_f32(int, int, int, const int *, const float *, long long, float *, long long, void *s) { return kernel("gather_rows_f32", s); }
int crp_scatter_add_rows_f64(int, int, const int *, const int *, const int *, const double *, long long, double *, long long, void *s)
{
    return kernel("scatter_add_rows_f64", s);
}
int crp_scatter_add_rows_f32(int, int, const int *, const int *, const int *, const float *, long long, float *, long long, void *s)
{
    return kernel("scatter_add_rows_f32", s);
}
int crp_gather_vals_f64(long long n, const int *, const double *, double *dst, void *s)
{
    CHECK(in_device(dst, sizeof(double) * (size_t) n), "value gather outside a live block");
    return kernel("gather_vals_f64", s);
}
int crp_gather_vals_f32_f64(long long n, const int *, const float *, double *dst, void *s)
{
    CHECK(in_device(dst, sizeof(double) * (size_t) n), "value gather outside a live block");
    return kernel("gather_vals_f32_f64", s);
}
int crp_sum_segments_f64(int, long long, const double *, long long, double *, void *s) { return kernel("sum_segments_f64", s); }
int crp_sum_segments_f32(int, long long, const float *, long long, float *, void *s) { return kernel("sum_segments_f32", s); }
int crp_transpose_f64(int, int, const double *, long long, double *, long long, void *s) { return kernel("transpose_f64", s); }
int crp_transpose_f32(int, int, const float *, long long, float *, long long, void *s) { return kernel("transpose_f32", s); }
}

static void check_balanced(const char *what)
{
    CHECK(calls("dev_malloc") == calls("dev_free"), "%s: %ld allocations, %ld frees", what, calls("dev_malloc"), calls("dev_free"));
    CHECK(g_dev.empty(), "%s: %zu device blocks are still live", what, g_dev.size());
    CHECK(g_pinned.empty() && calls("host_malloc") == calls("host_free"), "%s: pinned blocks are still live", what);
    CHECK(g_streams.empty() && calls("stream_create") == calls("stream_destroy"), "%s: %zu streams are still live", what, g_streams.size());
    CHECK(g_events.empty() && calls("event_create") == calls("event_destroy"), "%s: %zu events are still live", what, g_events.size());
    CHECK(g_csr.empty() && calls("csr_dev_create") + calls("csr_dev_create_dv") == calls("csr_dev_destroy"), "%s: %zu matrices are still live", what,
          g_csr.size());
}

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
