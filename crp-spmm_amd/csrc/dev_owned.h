// dev_owned.h -- what the engines hold on the device, each in a type that releases it.
//
// The engines sit on the C ABI (crpspmm_hip.h) and are plain host C++: these are their owners of device arrays, scratch, streams,
// events, matrix handles, pinned host blocks and owned communicators.  Every type is move-only, and an EMPTY one makes no ABI call at
// all -- not when it is constructed, moved, reset or destroyed -- so a plan-only engine never touches the device.  An engine's
// `free` is `delete`: members are released in reverse order of declaration.
#ifndef CRP_DEV_OWNED_H
#define CRP_DEV_OWNED_H

#include "crp_comm.h"
#include "crpspmm_hip.h"
#include "utils.h"

#define HIP_OK(call)                                                              \
    do {                                                                          \
        int rc__ = (call);                                                        \
        ASSERT_PRINTF(rc__ == 0, "%s failed with code %d\n", #call, rc__);        \
    } while (0)

namespace crp
{

// a device array of T.  A zero-byte allocation is NULL (crp_dev_malloc), so "p is null" does not say "not built yet" for an empty
// matrix: the engines keep their own flags for that.
template <class T> struct DevArray
{
    T *p = nullptr;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevArray &operator=(DevArray &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevArray() { reset(); }
    T *alloc(size_t count)
    {
        reset();
        void *d = NULL;
        HIP_OK(crp_dev_malloc(&d, sizeof(T) * count));
        return p = (T *) d;
    }
    // allocate, copy from the host on `stream`, wait for that stream
    T *upload(const T *host, size_t count, void *stream)
    {
        alloc(count);
        HIP_OK(crp_dev_memcpy(p, host, sizeof(T) * count, 0, stream));
        HIP_OK(crp_stream_sync(stream));
        return p;
    }
    // allocate and zero-fill on the null stream, wait for it (a caller's stream may not order against the null stream)
    T *zeroed(size_t count)
    {
        alloc(count);
        HIP_OK(crp_dev_memset(p, 0, sizeof(T) * count, NULL));
        HIP_OK(crp_stream_sync(NULL));
        return p;
    }
    T *get() const { return p; }
    operator T *() const { return p; }
    void reset() { if (p) crp_dev_free(p); p = nullptr; }
};

// grow-only device scratch: raw bytes shared by both dtypes, its size kept in doubles
struct DevScratch
{
    double *p = nullptr;
    size_t  sz = 0;
    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    DevScratch(DevScratch &&o) noexcept : p(o.p), sz(o.sz) { o.p = nullptr; o.sz = 0; }
    DevScratch &operator=(DevScratch &&o) noexcept { if (this != &o) { release(); p = o.p; sz = o.sz; o.p = nullptr; o.sz = 0; } return *this; }
    ~DevScratch() { release(); }
    template <class T> T *grow(size_t need_elems)
    {
        const size_t need = (need_elems * sizeof(T) + sizeof(double) - 1) / sizeof(double);
        if (need > sz)
        {
            if (p) HIP_OK(crp_dev_free(p));
            void *q = NULL;
            HIP_OK(crp_dev_malloc(&q, need * sizeof(double)));
            p = (double *) q;
            sz = need;
        }
        return (T *) p;
    }
    void release() { if (p) crp_dev_free(p); p = nullptr; sz = 0; }
};

// a stream / an event, created by the first ensure()
struct DevStream
{
    void *h = nullptr;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    DevStream(DevStream &&o) noexcept : h(o.h) { o.h = nullptr; }
    DevStream &operator=(DevStream &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~DevStream() { reset(); }
    void *ensure() { if (h == nullptr) HIP_OK(crp_stream_create(&h)); return h; }
    operator void *() const { return h; }
    void reset() { if (h) crp_stream_destroy(h); h = nullptr; }
};

struct DevEvent
{
    void *h = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    DevEvent(DevEvent &&o) noexcept : h(o.h) { o.h = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~DevEvent() { reset(); }
    void *ensure() { if (h == nullptr) HIP_OK(crp_event_create(&h)); return h; }
    operator void *() const { return h; }
    void reset() { if (h) crp_event_destroy(h); h = nullptr; }
};

// a device matrix: out() is where crp_csr_dev_create* puts the handle
struct DevCsr
{
    crp_csr_dev_p A = nullptr;
    DevCsr() = default;
    DevCsr(const DevCsr &) = delete;
    DevCsr &operator=(const DevCsr &) = delete;
    DevCsr(DevCsr &&o) noexcept : A(o.A) { o.A = nullptr; }
    DevCsr &operator=(DevCsr &&o) noexcept { if (this != &o) { reset(); A = o.A; o.A = nullptr; } return *this; }
    ~DevCsr() { reset(); }
    crp_csr_dev_p *out() { reset(); return &A; }
    operator crp_csr_dev_p() const { return A; }
    void reset() { if (A) crp_csr_dev_destroy(&A); A = nullptr; }
};

// a communicator this side owns (the result of a split), released through its own ->free
struct OwnedComm
{
    crp_comm_t *c = nullptr;
    OwnedComm() = default;
    explicit OwnedComm(crp_comm_t *c_) : c(c_) {}
    OwnedComm(const OwnedComm &) = delete;
    OwnedComm &operator=(const OwnedComm &) = delete;
    OwnedComm(OwnedComm &&o) noexcept : c(o.c) { o.c = nullptr; }
    OwnedComm &operator=(OwnedComm &&o) noexcept { if (this != &o) { reset(); c = o.c; o.c = nullptr; } return *this; }
    ~OwnedComm() { reset(); }
    crp_comm_t *operator->() const { return c; }
    operator crp_comm_t *() const { return c; }
    void reset() { if (c) c->free(c); c = nullptr; }
};

// a block of pinned host memory
struct HostPinned
{
    void *p = nullptr;
    HostPinned() = default;
    HostPinned(const HostPinned &) = delete;
    HostPinned &operator=(const HostPinned &) = delete;
    HostPinned(HostPinned &&o) noexcept : p(o.p) { o.p = nullptr; }
    HostPinned &operator=(HostPinned &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~HostPinned() { reset(); }
    void *alloc(size_t bytes) { reset(); HIP_OK(crp_host_malloc(&p, bytes)); return p; }
    void reset() { if (p) crp_host_free(p); p = nullptr; }
};

}  // namespace crp

#endif
