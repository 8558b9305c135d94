// operand_view.h -- a caller's dense operand as a device-resident row-major view, and the way back.
//
// The engines' entry points take B, C, X and Y on the host or on the device, row-major (layout 0: rows x n, ld >= n) or
// column-major (layout 1: n x rows as stored, ld >= rows), while the kernels read and write row-major device memory.  This
// layer is the one copy of that conversion.  It holds no engine state: the scratch buffers (crp::DevScratch, dev_owned.h) and the stream
// are the caller's, and the buffers release themselves with the engine that holds them.
//   operand_in    a source operand:  stage the used span with ONE copy if it is on the host, transpose if it is column-major
//   operand_out   a result operand:  where to compute (the caller's memory, a row-major temporary or a host image)
//   finish        transpose the temporary back and, for a host result, ONE 2D copy that never writes the caller's padding
// Three rules:
//   1. an operand without rows is {nullptr, n}: neither its pointer nor its leading dimension is read (a column-major ld only has
//      to cover zero rows and says nothing about n), nothing is enqueued;
//   2. a width of zero enqueues nothing;
//   3. a row-major device operand passes through as it is, without a call into the device ABI.
#ifndef CRP_OPERAND_VIEW_H
#define CRP_OPERAND_VIEW_H

#include "dtype_calls.h"      // HIP_OK, DevScratch, transpose

namespace crp
{

// elements a rows x n operand spans from its first to its last element
static inline size_t used_span(int layout, int rows, int n, long long ld)
{
    return layout == 0 ? (size_t) (rows - 1) * (size_t) ld + (size_t) n : (size_t) (n - 1) * (size_t) ld + (size_t) rows;
}

template <class T> struct InView
{
    const T  *p;
    long long ld;
};

// The rows x n operand P (ld, on the device or not) as a row-major device view.  A host operand is staged with one copy straight
// from the caller's pageable memory: the runtime stages it through its own pinned buffers at PCIe rate (measured: 16 ms per exec
// for B in + C out of the pwtk-size operands; an engine-owned pinned mirror with a memcpy in front of the DMA took 46 ms,
// pipelined through two pinned chunks with threaded memcpy 35 ms).
template <class T>
static InView<T> operand_in(int layout, const T *P, long long ld, int rows, int n, bool on_dev, DevScratch &stage, DevScratch &rm, void *s)
{
    if (rows <= 0) return InView<T>{nullptr, (long long) n};
    if (n <= 0 || (on_dev && layout == 0)) return InView<T>{P, ld};
    const T *Pd = P;
    if (!on_dev)
    {
        T *st = stage.grow<T>((size_t) (layout == 0 ? rows : n) * (size_t) ld);      // the whole block, ld preserved
        HIP_OK(crp_dev_memcpy(st, P, used_span(layout, rows, n, ld) * sizeof(T), 0, s));
        Pd = st;
    }
    if (layout == 0) return InView<T>{Pd, ld};
    T *r = rm.grow<T>((size_t) rows * (size_t) n);
    HIP_OK(transpose(n, rows, Pd, ld, r, n, s));      // column-major rows x n (ld) == row-major n x rows
    return InView<T>{r, (long long) n};
}

template <class T> struct OutView
{
    T        *p;         // compute into this, row-major with leading dimension ld
    long long ld;
    // the caller's operand, and the host image finish() fills
    T          *C;
    long long   ldC;
    int         layout, rows, n;
    bool        on_dev;
    DevScratch *stage;
};

// Where to compute the rows x n result C (ldC): the row-major temporary `rm` for a column-major result, the host image `stage`
// for a row-major host result, the caller's memory otherwise.
template <class T>
static OutView<T> operand_out(int layout, T *C, long long ldC, int rows, int n, bool on_dev, DevScratch &stage, DevScratch &rm)
{
    OutView<T> v{C, ldC, C, ldC, layout, rows, n, on_dev, &stage};
    if (layout == 1)
    {
        v.p = rm.grow<T>((size_t) rows * (size_t) n);
        v.ld = n;
    }
    else if (!on_dev && rows > 0 && n > 0) v.p = stage.grow<T>((size_t) rows * (size_t) ldC);
    return v;
}

// The result back in the caller's layout and memory.  `computed()` runs between the transpose and the copy to the host: the
// caller closes its timing of the device work there.  Returns whether the stream was synchronised.
template <class T, class F>
static bool finish(const OutView<T> &v, void *s, F &&computed)
{
    const bool any = v.rows > 0 && v.n > 0;
    const T *img = v.p;
    if (v.layout == 1 && any)
    {
        // a host column-major result is transposed into the host image and copied from there
        T *Ccm = v.on_dev ? v.C : v.stage->template grow<T>((size_t) v.n * (size_t) v.ldC);
        HIP_OK(transpose(v.rows, v.n, v.p, v.n, Ccm, v.ldC, s));   // row-major n x rows (ld ldC) == column-major rows x n
        img = Ccm;
    }
    computed();
    if (v.on_dev || !any) return false;
    // ONE 2D copy straight into the caller's C; the caller's padding between rows (columns) is never written
    const size_t w = v.layout == 0 ? (size_t) v.n : (size_t) v.rows, h = v.layout == 0 ? (size_t) v.rows : (size_t) v.n;
    HIP_OK(crp_dev_memcpy2d(v.C, (size_t) v.ldC * sizeof(T), img, (size_t) v.ldC * sizeof(T), w * sizeof(T), h, 1, s));
    HIP_OK(crp_stream_sync(s));
    return true;
}
template <class T> static bool finish(const OutView<T> &v, void *s) { return finish(v, s, [] {}); }

}  // namespace crp

#endif
