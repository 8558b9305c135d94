// csrc/operand_view.h under AddressSanitizer / UBSan (CPU only; built and run by tests/test_host_sanitizers.py).  The eight device
// ABI functions the layer may call are host stand-ins that count their calls and know which blocks are "device" memory; every
// caller buffer is allocated at exactly the span a legal caller owns, so an access one element past it is an ASan error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "operand_view.h"

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
static std::map<const char *, size_t> g_dev;         // "device" blocks: start -> bytes
struct Calls { int malloc_, free_, memcpy_, memcpy2d, transpose, sync; int total() const { return malloc_ + free_ + memcpy_ + memcpy2d + transpose + sync; } };
static Calls g_calls;

static bool in_device(const void *p, size_t bytes)
{
    auto it = g_dev.upper_bound((const char *) p);
    if (it == g_dev.begin()) return false;
    --it;
    return (const char *) p + bytes <= it->first + it->second;
}
static bool touches_device(const void *p)
{
    auto it = g_dev.upper_bound((const char *) p);
    if (it == g_dev.begin()) return false;
    --it;
    return (const char *) p < it->first + it->second;
}

template <class T>
static int transpose_host(int nrow, int ncol, const T *src, long long lds, T *dst, long long ldd)
{
    // dst[c][r] = src[r][c] (row_kernels.hip: transpose_f64_kernel); both sides are device memory
    g_calls.transpose++;
    if (nrow < 0 || ncol < 0) return -1;
    for (int r = 0; r < nrow; r++)
        for (int c = 0; c < ncol; c++)
        {
            CHECK(in_device(src + r * lds + c, sizeof(T)) && in_device(dst + c * ldd + r, sizeof(T)), "transpose outside device memory");
            dst[c * ldd + r] = src[r * lds + c];
        }
    return 0;
}

extern "C" {
int crp_dev_malloc(void **p, size_t bytes)
{
    g_calls.malloc_++;
    *p = NULL;
    if (bytes == 0) return 0;
    *p = malloc(bytes);
    memset(*p, 0x5a, bytes);
    g_dev[(const char *) *p] = bytes;
    return 0;
}
int crp_dev_free(void *p)
{
    g_calls.free_++;
    if (p == NULL) return 0;
    CHECK(g_dev.erase((const char *) p) == 1, "free of a pointer that is no device block");
    free(p);
    return 0;
}
int crp_dev_memcpy(void *dst, const void *src, size_t bytes, int kind, void *)
{
    g_calls.memcpy_++;
    if (bytes == 0) return 0;
    CHECK(kind == 0, "the layer only uploads with the 1D copy");
    CHECK(in_device(dst, bytes) && !touches_device(src), "1D copy: wrong side");
    memcpy(dst, src, bytes);
    return 0;
}
int crp_dev_memcpy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, int kind, void *)
{
    g_calls.memcpy2d++;
    if (width_bytes == 0 || height == 0) return 0;
    CHECK(kind == 1, "the layer only downloads with the 2D copy");
    for (size_t r = 0; r < height; r++)
    {
        CHECK(in_device((const char *) src + r * spitch, width_bytes) && !touches_device((char *) dst + r * dpitch), "2D copy: wrong side");
        memcpy((char *) dst + r * dpitch, (const char *) src + r * spitch, width_bytes);
    }
    return 0;
}
int crp_transpose_f64(int nrow, int ncol, const double *src, long long lds, double *dst, long long ldd, void *)
{
    return transpose_host(nrow, ncol, src, lds, dst, ldd);
}
int crp_transpose_f32(int nrow, int ncol, const float *src, long long lds, float *dst, long long ldd, void *)
{
    return transpose_host(nrow, ncol, src, lds, dst, ldd);
}
int crp_stream_sync(void *)
{
    g_calls.sync++;
    return 0;
}
}

// ---- a caller's operand: `off` sentinels, then exactly the span of the rows x n view ---------------------------------------------------
static const double SENT = -7.0;

template <class T> struct Caller
{
    int layout, rows, n;
    long long ld;
    size_t off, span;
    bool on_dev;
    T *buf = nullptr;

    Caller(int layout_, int rows_, int n_, int pad, int off_, bool on_dev_) : layout(layout_), rows(rows_), n(n_), off((size_t) off_), on_dev(on_dev_)
    {
        ld = (layout == 0 ? n : rows) + pad;
        span = (rows > 0 && n > 0) ? crp::used_span(layout, rows, n, ld) : 0;
        const size_t bytes = (off + span) * sizeof(T);
        if (bytes == 0) return;
        if (on_dev)
        {
            void *p = NULL;
            crp_dev_malloc(&p, bytes);
            buf = (T *) p;
        }
        else buf = (T *) malloc(bytes);
        for (size_t i = 0; i < off + span; i++) buf[i] = (T) SENT;
    }
    ~Caller()
    {
        if (on_dev) crp_dev_free(buf);
        else free(buf);
    }
    T *view() const { return buf ? buf + off : nullptr; }
    T &at(int i, int j) const { return layout == 0 ? view()[(size_t) i * ld + j] : view()[(size_t) j * ld + i]; }
    bool inside(size_t pos) const      // is element pos of the view's span one of the rows x n entries?
    {
        const size_t major = pos / (size_t) ld, minor = pos % (size_t) ld;
        return layout == 0 ? (major < (size_t) rows && minor < (size_t) n) : (major < (size_t) n && minor < (size_t) rows);
    }
};

template <class T> static T value(int i, int j, int salt) { return (T) (1 + i * 131 + j * 7 + salt); }

struct Scratch { crp::DevScratch B_stage, B_rm, C_stage, C_rm; void release() { B_stage.release(); B_rm.release(); C_stage.release(); C_rm.release(); } };

template <class T>
static void one_case(int layout, bool on_dev, int rows, int n, int pad, int off, Scratch &sc, const char *name)
{
    int dummy_stream;
    void *s = &dummy_stream;
    // ---- the input view
    {
        Caller<T> c(layout, rows, n, pad, off, on_dev);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < n; j++) c.at(i, j) = value<T>(i, j, 1);
        std::vector<T> before(c.buf, c.buf + (c.buf ? c.off + c.span : 0));
        const Calls c0 = g_calls;
        const crp::InView<T> v = rows == 0 ? crp::operand_in<T>(layout, nullptr, 0, 0, n, on_dev, sc.B_stage, sc.B_rm, s)
                                           : crp::operand_in<T>(layout, c.view(), c.ld, rows, n, on_dev, sc.B_stage, sc.B_rm, s);
        const Calls c1 = g_calls;
        const int copies = c1.memcpy_ - c0.memcpy_, transposes = c1.transpose - c0.transpose;
        CHECK(c1.sync == c0.sync && c1.memcpy2d == c0.memcpy2d, "%s: operand_in synchronised or used the 2D copy", name);
        if (rows == 0)
        {
            CHECK(v.p == nullptr && v.ld == n, "%s: an operand without rows is {nullptr, n}", name);
            CHECK(c1.total() == c0.total(), "%s: an operand without rows made a call", name);
        }
        else if (n == 0) CHECK(c1.total() == c0.total(), "%s: a width of zero made a call", name);
        else if (on_dev && layout == 0)
        {
            CHECK(v.p == c.view() && v.ld == c.ld, "%s: a device row-major operand passes through", name);
            CHECK(c1.total() == c0.total(), "%s: a device row-major operand made %d calls", name, c1.total() - c0.total());
        }
        else
        {
            CHECK(copies == (on_dev ? 0 : 1) && transposes == (layout == 1 ? 1 : 0), "%s: %d copies, %d transposes", name, copies, transposes);
            CHECK(in_device(v.p, sizeof(T) * ((size_t) (rows - 1) * (size_t) v.ld + (size_t) n)), "%s: the view is not device memory", name);
        }
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < n; j++)
                CHECK(v.p[(size_t) i * v.ld + j] == value<T>(i, j, 1), "%s: view[%d][%d] = %g", name, i, j, (double) v.p[(size_t) i * v.ld + j]);
        CHECK(before.empty() || memcmp(before.data(), c.buf, before.size() * sizeof(T)) == 0, "%s: the source was written", name);
    }
    // ---- the result view
    {
        Caller<T> c(layout, rows, n, pad, off, on_dev);
        const Calls c0 = g_calls;
        const crp::OutView<T> v = crp::operand_out<T>(layout, c.view(), c.ld, rows, n, on_dev, sc.C_stage, sc.C_rm);
        CHECK(g_calls.memcpy_ == c0.memcpy_ && g_calls.memcpy2d == c0.memcpy2d && g_calls.transpose == c0.transpose && g_calls.sync == c0.sync,
              "%s: operand_out enqueued something", name);
        if (on_dev && layout == 0) CHECK(g_calls.total() == c0.total() && (rows == 0 || (v.p == c.view() && v.ld == c.ld)), "%s: a device row-major result is computed in place", name);
        CHECK(v.ld >= n, "%s: the result view's leading dimension %lld is below n", name, v.ld);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < n; j++) v.p[(size_t) i * v.ld + j] = value<T>(i, j, 2);
        const Calls c1 = g_calls;
        int computed = 0;
        const bool synced = crp::finish(v, s, [&] { computed++; });
        const Calls c2 = g_calls;
        const bool any = rows > 0 && n > 0;
        CHECK(computed == 1, "%s: the callback ran %d times", name, computed);
        CHECK(synced == (!on_dev && any) && c2.sync - c1.sync == (synced ? 1 : 0), "%s: synchronised %d, %d syncs", name, (int) synced, c2.sync - c1.sync);
        CHECK(c2.memcpy2d - c1.memcpy2d == (synced ? 1 : 0) && c2.memcpy_ == c1.memcpy_, "%s: %d 2D copies", name, c2.memcpy2d - c1.memcpy2d);
        CHECK(c2.transpose - c1.transpose == ((layout == 1 && any) ? 1 : 0), "%s: %d transposes in finish", name, c2.transpose - c1.transpose);
        if (on_dev && layout == 0) CHECK(c2.total() == c1.total(), "%s: finish of a device row-major result made a call", name);
        for (size_t p = 0; p < c.off; p++) CHECK(c.buf[p] == (T) SENT, "%s: element %zu in front of C was written", name, p);
        for (size_t p = 0; p < c.span; p++)
            if (!c.inside(p)) CHECK(c.view()[p] == (T) SENT, "%s: pad element %zu of C was written", name, p);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < n; j++) CHECK(c.at(i, j) == value<T>(i, j, 2), "%s: C[%d][%d] = %g", name, i, j, (double) c.at(i, j));
    }
}

template <class T> static int sweep(const char *dtype, Scratch &shared)
{
    int cases = 0;
    char name[128];
    for (int layout = 0; layout < 2; layout++)
        for (int on_dev = 0; on_dev < 2; on_dev++)
            for (int rows : {0, 1, 5})
                for (int n : {0, 1, 7})
                    for (int pad : {0, 3})
                        for (int off : {0, 1})
                        {
                            snprintf(name, sizeof(name), "%s layout %d %s rows %d n %d pad %d off %d", dtype, layout, on_dev ? "dev" : "host", rows, n, pad, off);
                            Scratch fresh;                       // every buffer at exactly the size the layer asked for ...
                            one_case<T>(layout, on_dev != 0, rows, n, pad, off, fresh, name);
                            fresh.release();
                            one_case<T>(layout, on_dev != 0, rows, n, pad, off, shared, name);      // ... and the grow-only set both dtypes share
                            cases++;
                        }
    return cases;
}

int main()
{
    Scratch shared;
    int cases = sweep<double>("f64", shared);
    cases += sweep<float>("f32", shared);
    cases += sweep<double>("f64 again", shared);
    shared.release();
    CHECK(g_dev.empty(), "%zu device blocks were never freed", g_dev.size());
    printf("HOST_OPERAND_VIEW_OK cases=%d\n", cases);
    return 0;
}
