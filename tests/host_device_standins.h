// Host stand-ins for the device ABI (include/crpspmm_hip.h), shared by tests/host_engine_resources.cpp and
// tests/host_engine_streams.cpp: "device" memory is calloc, kernels and matrix handles do no arithmetic, every call is counted, and a
// free, destroy, copy or stream / event call on something that is not live ends the program.  With g_logging on, every call is also
// logged as (call, stream, buffers read, buffers written), and events log their records and waits.  Include once per program.
#ifndef HOST_DEVICE_STANDINS_H
#define HOST_DEVICE_STANDINS_H
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
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
// (b0 / b1: whether a column code names the first / the second source: a kernel reads only the sources its handle names)
struct crp_csr_dev { int nrow; long long nnz; bool b0, b1; };

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
// ---- the log: every call that works on a stream with the live blocks (by their start) and matrix handles it reads and writes, every
// event record and wait, every stream synchronisation, and what is freed (tests/host_engine_streams.cpp replays it)
enum OpKind { OP_WORK, OP_RECORD, OP_WAIT, OP_SYNC, OP_FORGET };
struct Op { OpKind kind; const char *call; void *stream; void *event; std::vector<const void *> reads, writes; };
static std::vector<Op> g_log;
static bool g_logging = false;
struct R { const void *p; };      // a pointer the call reads
struct W { const void *p; };      // a pointer the call writes
// the buffer a pointer belongs to: the start of its live block, a live matrix handle, or NULL (host memory, nothing)
static const void *buffer_of(const void *p)
{
    if (p == NULL) return NULL;
    if (g_csr.count((void *) p)) return p;
    auto it = g_dev.upper_bound((const char *) p);
    if (it == g_dev.begin()) return NULL;
    --it;
    return (const char *) p < it->first + it->second ? it->first : NULL;
}
static void log_op(OpKind kind, const char *call, void *stream, void *event, std::initializer_list<R> rd = {}, std::initializer_list<W> wr = {})
{
    if (!g_logging) return;
    Op op{kind, call, stream, event, {}, {}};
    for (const R &r : rd) if (const void *b = buffer_of(r.p)) op.reads.push_back(b);
    for (const W &w : wr) if (const void *b = buffer_of(w.p)) op.writes.push_back(b);
    g_log.push_back(op);
}
static int kernel(const char *name, void *stream, std::initializer_list<R> rd = {}, std::initializer_list<W> wr = {})
{
    live_stream(stream);
    log_op(OP_WORK, name, stream, NULL, rd, wr);
    return hit(name);
}
static int csr_create(const char *name, int nrow, const int *rowptr, const int *colidx, crp_csr_dev_p *out)
{
    crp_csr_dev *A = new crp_csr_dev{nrow, rowptr[nrow], false, false};
    for (int p = 0; p < rowptr[nrow]; p++) (colidx[p] >= 0 ? A->b0 : A->b1) = true;
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
    log_op(OP_FORGET, "dev_free", NULL, NULL, {}, {W{p}});
    CHECK(g_dev.erase((const char *) p) == 1, "crp_dev_free of a block that is not live");
    free(p);
    return hit("dev_free");
}
int crp_dev_memset(void *p, int v, size_t bytes, void *stream)
{
    live_stream(stream);
    CHECK(bytes == 0 || in_device(p, bytes), "memset outside a live block");
    if (bytes) memset(p, v, bytes);
    log_op(OP_WORK, "dev_memset", stream, NULL, {}, {W{bytes ? p : NULL}});
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
    log_op(OP_WORK, "dev_memcpy", stream, NULL, {R{bytes ? src : NULL}}, {W{bytes ? dst : NULL}});
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
    log_op(OP_WORK, "dev_memcpy2d", stream, NULL, {R{width_bytes && height ? src : NULL}}, {W{width_bytes && height ? dst : NULL}});
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
int crp_stream_sync(void *s)
{
    live_stream(s);
    log_op(OP_SYNC, "stream_sync", s, NULL);
    return hit("stream_sync");
}
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
    live_stream(s);
    log_op(OP_RECORD, "event_record", s, ev);
    return hit("event_record");
}
int crp_stream_wait_event(void *s, void *ev)
{
    CHECK(g_events.count(ev), "wait for an event that is not live");
    live_stream(s);
    log_op(OP_WAIT, "stream_wait_event", s, ev);
    return hit("stream_wait_event");
}
int crp_csr_dev_create(int nrow, int, const int *rowptr, const int *colidx, const double *, crp_csr_dev_p *out)
{
    return csr_create("csr_dev_create", nrow, rowptr, colidx, out);
}
int crp_csr_dev_create_dv(int nrow, int, const int *rowptr, const int *colidx, const double *, const double *, const int *, crp_csr_dev_p *out)
{
    return csr_create("csr_dev_create_dv", nrow, rowptr, colidx, out);
}
int crp_csr_dev_destroy(crp_csr_dev_p *A)
{
    if (A == NULL || *A == NULL) return hit("csr_dev_destroy(null)");
    log_op(OP_FORGET, "csr_dev_destroy", NULL, NULL, {}, {W{*A}});
    CHECK(g_csr.erase(*A) == 1, "crp_csr_dev_destroy of a handle that is not live");
    delete *A;
    *A = NULL;
    return hit("csr_dev_destroy");
}
int crp_csr_dev_update_values(crp_csr_dev_p A, const double *val, void *s) { live_csr(A); return kernel("csr_dev_update_values", s, {R{val}}, {W{A}}); }
int crp_csr_dev_set_rowmap(crp_csr_dev_p A, const int *, int) { live_csr(A); return hit("csr_dev_set_rowmap"); }
int crp_csr_dev_nrow(crp_csr_dev_p A) { live_csr(A); return A->nrow; }
long long crp_csr_dev_nnz(crp_csr_dev_p A) { live_csr(A); return A->nnz; }
int crp_csr_dev_last_variant(crp_csr_dev_p) { return 0; }
int crp_csr_dev_resolved_variant(crp_csr_dev_p, int) { return 1; }
int crp_csr_dev_reordered(crp_csr_dev_p) { return 0; }
int crp_csr_dev_lattice(crp_csr_dev_p) { return 0; }
int crp_csr_transpose(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, int *rowptr_t, int *colidx_t, double *val_t,
                      int *tmap, void *s)
{
    // zeros: every entry in row 0 of the transpose's first ncol rows is a legal, if wrong, answer for code that only moves it about
    CHECK(in_device(rowptr, sizeof(int) * ((size_t) nrow + 1)) && in_device(rowptr_t, sizeof(int) * ((size_t) ncol + 1)), "transpose outside live blocks");
    const size_t nnz = (size_t) rowptr[nrow];
    memset(rowptr_t, 0, sizeof(int) * ((size_t) ncol + 1));
    CHECK(nnz == 0 || (in_device(colidx_t, sizeof(int) * nnz) && in_device(val_t, sizeof(double) * nnz) && in_device(tmap, sizeof(int) * nnz)),
          "transpose outside live blocks");
    if (nnz) { memset(colidx_t, 0, sizeof(int) * nnz); memset(val_t, 0, sizeof(double) * nnz); memset(tmap, 0, sizeof(int) * nnz); }
    return kernel("csr_transpose", s, {R{rowptr}, R{colidx}, R{val}}, {W{rowptr_t}, W{colidx_t}, W{val_t}, W{tmap}});
}
int crp_spmm_csr_f64(crp_csr_dev_p A, int, int, const double *B0, long long, const double *B1, long long, double *C, long long, int, void *s)
{
    live_csr(A);
    return kernel("spmm_csr_f64", s, {R{A}, R{A->b0 ? B0 : NULL}, R{A->b1 ? B1 : NULL}}, {W{C}});
}
int crp_spmm_csr_f32(crp_csr_dev_p A, int, const float *B0, long long, const float *B1, long long, float *C, long long, int, void *s)
{
    live_csr(A);
    return kernel("spmm_csr_f32", s, {R{A}, R{A->b0 ? B0 : NULL}, R{A->b1 ? B1 : NULL}}, {W{C}});
}
int crp_sddmm_csr_f64(crp_csr_dev_p A, int, const double *X, long long, const double *Y0, long long, const double *Y1, long long, double *out,
                      const int *pos, int, void *s)
{
    live_csr(A);
    return kernel("sddmm_csr_f64", s, {R{A}, R{X}, R{A->b0 ? Y0 : NULL}, R{A->b1 ? Y1 : NULL}, R{pos}}, {W{out}});
}
int crp_sddmm_csr_f32(crp_csr_dev_p A, int, const float *X, long long, const float *Y0, long long, const float *Y1, long long, float *out,
                      const int *pos, int, void *s)
{
    live_csr(A);
    return kernel("sddmm_csr_f32", s, {R{A}, R{X}, R{A->b0 ? Y0 : NULL}, R{A->b1 ? Y1 : NULL}, R{pos}}, {W{out}});
}
int crp_row_softmax_f64(int, const int *rp, const double *x, double *y, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_f64", s, {R{rp}, R{x}}, {W{y}});
}
int crp_row_softmax_f32(int, const int *rp, const float *x, float *y, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_f32", s, {R{rp}, R{x}}, {W{y}});
}
int crp_row_softmax_bwd_f64(int, const int *rp, const double *y, const double *dy, double *ds, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_bwd_f64", s, {R{rp}, R{y}, R{dy}}, {W{ds}});
}
int crp_row_softmax_bwd_f32(int, const int *rp, const float *y, const float *dy, float *ds, void *s)
{
    CHECK(in_device(rp, 4), "row pointer");
    return kernel("row_softmax_bwd_f32", s, {R{rp}, R{y}, R{dy}}, {W{ds}});
}
int crp_gather_rows_f64(int, int, int, const int *ridx, const double *src, long long, double *dst, long long, void *s)
{
    return kernel("gather_rows_f64", s, {R{ridx}, R{src}}, {W{dst}});
}
int crp_gather_rows_f32(int, int, int, const int *ridx, const float *src, long long, float *dst, long long, void *s)
{
    return kernel("gather_rows_f32", s, {R{ridx}, R{src}}, {W{dst}});
}
int crp_scatter_add_rows_f64(int, int, const int *row, const int *ptr, const int *pos, const double *src, long long, double *dst, long long, void *s)
{
    return kernel("scatter_add_rows_f64", s, {R{row}, R{ptr}, R{pos}, R{src}, R{dst}}, {W{dst}});
}
int crp_scatter_add_rows_f32(int, int, const int *row, const int *ptr, const int *pos, const float *src, long long, float *dst, long long, void *s)
{
    return kernel("scatter_add_rows_f32", s, {R{row}, R{ptr}, R{pos}, R{src}, R{dst}}, {W{dst}});
}
int crp_gather_vals_f64(long long n, const int *map, const double *src, double *dst, void *s)
{
    CHECK(in_device(dst, sizeof(double) * (size_t) n), "value gather outside a live block");
    return kernel("gather_vals_f64", s, {R{map}, R{src}}, {W{dst}});
}
int crp_gather_vals_f32_f64(long long n, const int *map, const float *src, double *dst, void *s)
{
    CHECK(in_device(dst, sizeof(double) * (size_t) n), "value gather outside a live block");
    return kernel("gather_vals_f32_f64", s, {R{map}, R{src}}, {W{dst}});
}
int crp_sum_segments_f64(int, long long, const double *src, long long, double *out, void *s) { return kernel("sum_segments_f64", s, {R{src}}, {W{out}}); }
int crp_sum_segments_f32(int, long long, const float *src, long long, float *out, void *s) { return kernel("sum_segments_f32", s, {R{src}}, {W{out}}); }
int crp_transpose_f64(int, int, const double *src, long long, double *dst, long long, void *s) { return kernel("transpose_f64", s, {R{src}}, {W{dst}}); }
int crp_transpose_f32(int, int, const float *src, long long, float *dst, long long, void *s) { return kernel("transpose_f32", s, {R{src}}, {W{dst}}); }
// the fused attention and its backward (csrc/rp_attention.cpp); the variadic part is the multi-head calls' `int heads,` after the handle
#define FWD_STANDIN(NAME, T, ...)                                                                                                           \
    int NAME(crp_csr_dev_p A, __VA_ARGS__ int, int, double, int, const T *Q, long long, const T *K0, long long, const T *K1, long long,     \
             const T *V0, long long, const T *V1, long long, T *O, long long, T *lse, T *p_out, const int *pos, void *s)                    \
    {                                                                                                                                       \
        live_csr(A);                                                                                                                        \
        return kernel(#NAME + 4, s, {R{A}, R{Q}, R{A->b0 ? K0 : NULL}, R{A->b1 ? K1 : NULL}, R{A->b0 ? V0 : NULL}, R{A->b1 ? V1 : NULL}, R{pos}}, {W{O}, W{lse}, W{p_out}});   \
    }
#define BWD_Q_STANDIN(NAME, T, ...)                                                                                                         \
    int NAME(crp_csr_dev_p A, __VA_ARGS__ int, int, double, int, const T *Q, long long, const T *K0, long long, const T *K1, long long,     \
             const T *V0, long long, const T *V1, long long, const T *O, long long, const T *dO, long long, const T *lse, T *dQ, long long, \
             T *delta, T *ds_out, const int *pos, void *s)                                                                                  \
    {                                                                                                                                       \
        live_csr(A);                                                                                                                        \
        return kernel(#NAME + 4, s, {R{A}, R{Q}, R{A->b0 ? K0 : NULL}, R{A->b1 ? K1 : NULL}, R{A->b0 ? V0 : NULL}, R{A->b1 ? V1 : NULL}, R{O}, R{dO}, R{lse}, R{pos}}, {W{dQ}, W{delta}, W{ds_out}});   \
    }
#define BWD_KV_STANDIN(NAME, T, ...)                                                                                                        \
    int NAME(crp_csr_dev_p At, __VA_ARGS__ int, int, double, int, const T *K, long long, const T *V, long long, const T *Q, long long,      \
             const T *dO, long long, const T *lse, const T *delta, T *dK, long long, T *dV, long long, void *s)                             \
    {                                                                                                                                       \
        live_csr(At);                                                                                                                       \
        return kernel(#NAME + 4, s, {R{At}, R{K}, R{V}, R{Q}, R{dO}, R{lse}, R{delta}}, {W{dK}, W{dV}});                                    \
    }
// the fused GAT and GATv2 attention, forward (csrc/rp_gat.cpp): el / XT and a are local, er, V and XS have the two sources of the column code
#define GAT_STANDIN(NAME, T)                                                                                                                \
    int NAME(crp_csr_dev_p A, int, int, double, int, const T *el, long long, const T *er0, long long, const T *er1, long long,              \
             const T *V0, long long, const T *V1, long long, T *O, long long, T *lse, T *p_out, const int *pos, void *s)                    \
    {                                                                                                                                       \
        live_csr(A);                                                                                                                        \
        return kernel(#NAME + 4, s, {R{A}, R{el}, R{A->b0 ? er0 : NULL}, R{A->b1 ? er1 : NULL}, R{A->b0 ? V0 : NULL}, R{A->b1 ? V1 : NULL}, R{pos}}, {W{O}, W{lse}, W{p_out}});   \
    }
#define GATV2_STANDIN(NAME, T)                                                                                                              \
    int NAME(crp_csr_dev_p A, int, int, double, int, const T *XT, long long, const T *XS0, long long, const T *XS1, long long, const T *a,  \
             T *O, long long, T *lse, T *p_out, const int *pos, void *s)                                                                    \
    {                                                                                                                                       \
        live_csr(A);                                                                                                                        \
        return kernel(#NAME + 4, s, {R{A}, R{XT}, R{a}, R{A->b0 ? XS0 : NULL}, R{A->b1 ? XS1 : NULL}, R{pos}}, {W{O}, W{lse}, W{p_out}});   \
    }
GAT_STANDIN(crp_gat_attention_csr_f64, double)
GAT_STANDIN(crp_gat_attention_csr_f32, float)
GATV2_STANDIN(crp_gatv2_attention_csr_f64, double)
GATV2_STANDIN(crp_gatv2_attention_csr_f32, float)
FWD_STANDIN(crp_attention_csr_f64, double)
FWD_STANDIN(crp_attention_csr_f32, float)
FWD_STANDIN(crp_attention_mh_csr_f64, double, int,)
FWD_STANDIN(crp_attention_mh_csr_f32, float, int,)
BWD_Q_STANDIN(crp_attention_bwd_q_csr_f64, double)
BWD_Q_STANDIN(crp_attention_bwd_q_csr_f32, float)
BWD_Q_STANDIN(crp_attention_bwd_q_mh_csr_f64, double, int,)
BWD_Q_STANDIN(crp_attention_bwd_q_mh_csr_f32, float, int,)
BWD_KV_STANDIN(crp_attention_bwd_kv_csr_f64, double)
BWD_KV_STANDIN(crp_attention_bwd_kv_csr_f32, float)
BWD_KV_STANDIN(crp_attention_bwd_kv_mh_csr_f64, double, int,)
BWD_KV_STANDIN(crp_attention_bwd_kv_mh_csr_f32, float, int,)
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

#endif
