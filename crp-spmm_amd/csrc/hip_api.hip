// hip_api.hip -- implementation of include/crpspmm_hip.h (device-level C ABI).
// Replaces the host/CUDA shims of /root/reference/deprecated/src/cuda_proxy.cu:53-182
// with HIP-only code for gfx950; there is no CPU fallback in this file.  Which kernel a product runs is decided in dispatch.cpp.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <new>
#include <memory>
#include <algorithm>
#include <array>
#include <vector>
#include "crpspmm_hip.h"
#include "kernels.h"
#include "panel_format.h"
#include "dispatch.h"
#include "locality.h"
#include "knobs.h"
#include "csr_transpose.h"

// a device allocation that frees itself (move-only)
template <typename T> struct DevBuf
{
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); return *this; }     // (o frees what this held)
    ~DevBuf() { reset(); }
    void reset() { if (p) (void) hipFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { reset(); return hipMalloc((void **) &p, bytes); }
    operator T *() const { return p; }
};

// bytes + pad of device memory: the bytes from the host, the pad zeroed (the kernels read past the ends of their arrays)
template <typename T> static hipError_t upload(DevBuf<T> &dst, const void *src, size_t bytes, size_t pad)
{
    hipError_t e = dst.alloc(bytes + pad);
    if (e == hipSuccess && pad) e = hipMemset((char *) dst.p + bytes, 0, pad);
    if (e == hipSuccess && bytes) e = hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice);
    return e;
}

// a format's value array and the slot map that puts every CSR nonzero's value into it (nullptr: none)
struct SlotMap { const uint32_t *map; double *val; };

// device copy of one row-panel format (panel_format.h)
struct PanelDev
{
    bool      built = false;
    int       R = 0, npanel = 0;
    DevBuf<int> pptr, pcol, porder;
    int       norder = 0;
    DevBuf<int> psync;
    DevBuf<uint32_t> pmask4, pmap;
    DevBuf<double> pval;
    double    fill = 0.0;
    long long entries = 0;
    // compact values for the narrow-operand kernel (R = 8 panels that are mostly holes; PanelHost::cmo / cbase / cval / cmap)
    DevBuf<uint32_t> cmo, cmap;
    DevBuf<long long> cbase;
    DevBuf<double> cval;
    long long cvalues = 0;
    std::array<SlotMap, 2> slot_maps() const { return {{{pmap, pval}, {cmap, cval}}}; }
};

struct Team2Dev
{
    bool built = false;
    int  nteam = 0;
    int ngrid = 0;                 // entries of torder (= the launch grid, 8 equal runs, -1 = no team)
    bool compact = true;           // Team2Host::compact
    DevBuf<int> torder, tpanel, tinfo, tpro;
    DevBuf<uint32_t> trec;
    DevBuf<long long> tvoff;
    DevBuf<double> tval;
    DevBuf<uint32_t> tmap;         // per CSR nonzero: its slot in tval (value updates)
    DevBuf<float> tval32;          // fp32 copy of the value groups (fp32 path), built on first use
    long long entries = 0, value_entries = 0;
    bool lattice = false;
    std::array<SlotMap, 1> slot_maps() const { return {{{tmap, tval}}}; }
};

struct Team2RDev              // panel_format.h, Team2RHost: the row-owner team kernel's streams (variant 7)
{
    bool built = false;
    int G = 4, nteam = 0, ngrid = 0;
    DevBuf<int> tgrid, tpanel, tinfo;
    DevBuf<uint32_t> trec;
    DevBuf<long long> tvoff;
    DevBuf<double> tval;
    DevBuf<uint32_t> tmap;
    DevBuf<uint32_t> tent;         // the entry table (Team2RHost::tent); its C rows are filled for rows_epoch
    long long rows_epoch = -1;
    const int *rows_map = nullptr;
    bool refused = false;          // the streams of this matrix would pass their 32-bit offsets: remembered, not rebuilt per product
    long long value_entries = 0;
    bool lattice = false;
    std::array<SlotMap, 1> slot_maps() const { return {{{tmap, tval}}}; }
};

struct crp_csr_dev
{
    int       nrow = 0;
    int       ncol = 0;
    long long nnz = 0;
    DevBuf<int> rowptr, colidx;
    DevBuf<double> val;
    // host copy kept for building further formats on demand
    std::vector<int>    h_rowptr, h_colidx;
    std::vector<double> h_val;
    PanelDev pan[2];          // [0]: R = 4, [1]: R = 8
    Team2Dev team2;           // teams of eight R = 8 panels, LDS-shared B rows (variant 5)
    Team2RDev team2r[2];      // the row-owner team kernel's streams (variant 7): [0] n <= 32 (G = 4), [1] n <= 64 (G = 2); tvoff in units of 16 bytes
    crp::MatrixTraits traits;      // what variant 0 resolves to (dispatch.h), decided at create
    bool     team2r_refused = false;   // a variant-0 product found the row-owner streams too large: variant 0 no longer takes them
    long long rowmap_epoch = 0;    // bumped by crp_csr_dev_set_rowmap: the team2r entry tables hold C rows
    int      last_variant = 0;     // what the last product launched (crp_csr_dev_last_variant)
    const char *last_kernel = "";  // ... and the kernel instance, as its launcher named it (crp_csr_dev_last_kernel)
    long long b0_rows = 0, b1_rows = 0;   // 1 + largest local / receive-buffer row a column index addresses
    DevBuf<float> val32;                  // fp32 copy of val (fp32 path), built on first use
    DevBuf<int> rowmap;                   // row-subset matrices: C row of every row (device), else nullptr
    // locality order (dispatch.h, FormatOrder): the derived formats (panels, teams) are built on the rows in processing order;
    // f_val = the values in that order, rowmap_fmt = C row of every position (the caller's row map composed with perm)
    crp::FormatOrder ord;
    std::vector<double>   f_val;
    std::vector<int>      h_rowmap;       // host copy of the caller's row map (empty: none)
    DevBuf<int> rowmap_fmt;
    int       c_nrow = 0;                 // rows of C the product writes into (nrow without a rowmap)
    // crp_csr_dev_update_values() with a DEVICE pointer leaves the host copies (h_val / f_val) behind: formats built
    // afterwards take their values from the device CSR through their fresh slot maps (refresh_values_after_build)
    bool      host_vals_stale = false;
    // crp_csr_dev_create_t: this handle holds A^T; tmap[q] = position in A's arrays of nonzero q (device and host copies), so
    // that value updates, which come in A's order, can be gathered into this handle's order.  Empty for every other handle.
    DevBuf<int> tmap;
    std::vector<int> h_tmap;
    // The R = 8 panels in column order WITHOUT values (pcol, masks, slot map: 7 bytes per nonzero at fill 0.23) and the teams built on
    // them: shared by the team formats of this matrix (team2, team2r for <= 32 and <= 64 columns) -- a further operand width costs the
    // streams of its format, not the panels and the clustering again.  Dropped once the two that variant 0 uses exist.
    std::unique_ptr<crp::PanelHost> skel8;
    crp::TeamSeed seed8;
};

static const int *fmt_rowptr(const crp_csr_dev *A) { return A->ord.perm.empty() ? A->h_rowptr.data() : A->ord.f_rowptr.data(); }
static const int *fmt_colidx(const crp_csr_dev *A) { return A->ord.perm.empty() ? A->h_colidx.data() : A->ord.f_colidx.data(); }
static const double *fmt_val(const crp_csr_dev *A) { return A->ord.perm.empty() ? A->h_val.data() : A->f_val.data(); }
// slot map of a derived format, built on the processing order, re-indexed by the caller's nonzero positions
static void fmt_slotmap_to_caller(const crp_csr_dev *A, crp::big_vector<uint32_t> *pmap)
{
    if (A->ord.perm.empty()) return;
    crp::big_vector<uint32_t> out(pmap->size());
    for (size_t pz = 0; pz < pmap->size(); pz++) out[(size_t) A->ord.f_nz[pz]] = (*pmap)[pz];
    pmap->swap(out);
}
// position of every row in the processing order (square, re-ordered matrices), or empty
static std::vector<int> fmt_colpos(const crp_csr_dev *A)
{
    std::vector<int> colpos(A->ord.perm.size());
    for (size_t i = 0; i < A->ord.perm.size(); i++) colpos[(size_t) A->ord.perm[i]] = (int) i;
    return colpos;
}
// a format's values from the device CSR, through its slot maps
template <class D> static hipError_t scatter_values(const crp_csr_dev *A, const D &d, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    for (const SlotMap &m : d.slot_maps())
        if (m.map && e == hipSuccess) e = crp::scatter_vals_f64(A->nnz, m.map, A->val, m.val, stream);
    return e;
}

// the shared structure-only panels (see crp_csr_dev::skel8)
static const crp::PanelHost &panel_skeleton(crp_csr_dev *A)
{
    if (!A->skel8)
    {
        A->skel8.reset(new crp::PanelHost);
        crp::build_panels(A->nrow, fmt_rowptr(A), fmt_colidx(A), nullptr, 8, A->skel8.get(), false, false);
        fmt_slotmap_to_caller(A, &A->skel8->pmap);
    }
    return *A->skel8;
}
static void drop_skeleton_when_done(crp_csr_dev *A)
{
    // (the formats variant 0 can ask for: the team format and the row-owner format of n <= 32; an explicit variant 7 at 33 .. 64 columns
    //  afterwards builds its panels and teams again)
    const bool r0 = A->team2r[0].built || A->team2r[0].refused;
    if (A->team2.built && r0)
    {
        A->skel8.reset();
        A->seed8 = crp::TeamSeed();
    }
}

#define CRP_TRY(expr)                                 \
    do                                                \
    {                                                 \
        hipError_t e__ = (expr);                      \
        if (e__ != hipSuccess) return (int) e__;      \
    } while (0)

// State that a call builds on a handle is COMPLETE ON RETURN (include/crpspmm_hip.h, "Streams"): whatever the building call
// enqueued on its stream is waited for once, so that a later call on any other stream finds it ready.
// The fp32 copy of the values (the fp32 products, the fp32 SDDMM in mode 1, the fp32 attention calls with bias), built by the
// first call that needs it and kept current by crp_csr_dev_update_values.
static int ensure_val32(crp_csr_dev *A, hipStream_t s)
{
    if (A->val32 != nullptr) return 0;
    DevBuf<float> v;
    CRP_TRY(v.alloc(sizeof(float) * (size_t) (A->nnz > 0 ? A->nnz : 1)));
    CRP_TRY(crp::convert_f64_f32(A->nnz, A->val, v, s));
    CRP_TRY(hipStreamSynchronize(s));
    A->val32 = std::move(v);
    return 0;
}

// Build (once) and upload the row-panel format with R = 4 (idx 0) or 8 (idx 1). Blocking.  (A failed upload leaves the format unbuilt.)
static int ensure_panel(crp_csr_dev *A, int idx, hipStream_t stream)
{
    if (A->pan[idx].built) return 0;
    PanelDev d;
    crp::PanelHost h;
    crp::build_panels(A->nrow, fmt_rowptr(A), fmt_colidx(A), fmt_val(A), idx == 0 ? 4 : 8, &h);
    fmt_slotmap_to_caller(A, &h.pmap);
    d.R = h.R;
    d.npanel = h.npanel;
    d.norder = (int) h.porder.size();
    d.fill = h.fill();
    d.entries = (long long) h.pcol.size();
    hipError_t e = upload(d.pmap, h.pmap.data(), sizeof(uint32_t) * h.pmap.size(), sizeof(uint32_t));
    // processing order as 16-byte records {panel (-1: none), first entry, rounds, 0}, one per position
    {
        std::vector<int> rec(4 * (h.porder.size() + 4), 0);
        for (size_t i = 0; i < h.porder.size(); i++)
        {
            const int pnl = h.porder[i];
            rec[4 * i] = pnl;
            if (pnl >= 0)
            {
                rec[4 * i + 1] = h.pptr[(size_t) pnl];
                rec[4 * i + 2] = (h.pptr[(size_t) pnl + 1] - h.pptr[(size_t) pnl]) / crp::PANEL_PAD;
            }
        }
        for (size_t i = h.porder.size(); i < h.porder.size() + 4; i++) rec[4 * i] = -1;
        if (e == hipSuccess) e = upload(d.porder, rec.data(), sizeof(int) * rec.size(), 0);
    }
    // team schedule: the waves of a workgroup start their rounds together
    if (e == hipSuccess && !h.psync.empty()) e = upload(d.psync, h.psync.data(), sizeof(int) * h.psync.size(), sizeof(int) * 8);
    if (e == hipSuccess) e = upload(d.pptr, h.pptr.data(), sizeof(int) * h.pptr.size(), 0);
    {
        // the kernels read column indices up to three rounds past a panel: the tail of the array
        // repeats the last real column (an addressable row), never an arbitrary value
        std::vector<int> padded(h.pcol.begin(), h.pcol.end());
        if (!h.pcol.empty()) padded.resize(h.pcol.size() + 64, h.pcol.back());
        if (e == hipSuccess) e = upload(d.pcol, padded.data(), sizeof(int) * padded.size(), sizeof(int) * (h.pcol.size() + 64 - padded.size()));
    }
    if (e == hipSuccess) e = upload(d.pmask4, h.pmask4.data(), sizeof(uint32_t) * h.pmask4.size(), sizeof(uint32_t) * 16);
    if (e == hipSuccess) e = upload(d.pval, h.pval.data(), sizeof(double) * h.pval.size(), sizeof(double) * 512);
    // Compact values for the narrow-operand kernel when under 60 % of the panels' (row, entry) pairs exist (n = 32, compact
    // against full values: nlpkkt stand-in, fill 0.23: 0.527 against 0.599 ms; Queen stand-in, 0.57: 0.243 against 0.260; pwtk
    // stand-in, 0.61: 0.068 against 0.067)
    {
        const bool want = idx == 1 && d.fill < 0.6;
        if (e == hipSuccess && want && A->nnz > 0 && crp::build_compact_values(&h))
        {
            d.cvalues = h.cbase.back();          // (cmap is derived from pmap, which is indexed by the caller's nonzeros already)
            e = upload(d.cmo, h.cmo.data(), sizeof(uint32_t) * h.cmo.size(), sizeof(uint32_t) * 64);
            if (e == hipSuccess) e = upload(d.cbase, h.cbase.data(), sizeof(long long) * h.cbase.size(), 0);
            if (e == hipSuccess) e = upload(d.cval, h.cval.data(), sizeof(double) * h.cval.size(), 0);
            if (e == hipSuccess) e = upload(d.cmap, h.cmap.data(), sizeof(uint32_t) * h.cmap.size(), sizeof(uint32_t));
        }
    }
    if (e != hipSuccess) return (int) e;
    if (A->host_vals_stale && A->nnz > 0)
    {
        CRP_TRY(scatter_values(A, d, stream));
        CRP_TRY(hipStreamSynchronize(stream));      // complete on return, for callers on other streams
    }
    d.built = true;
    A->pan[idx] = std::move(d);
    return 0;
}

// Build (once) and upload the team2 streams on top of the R = 8 panels (column-ordered entries). Blocking.
static int ensure_team2(crp_csr_dev *A, hipStream_t stream, bool for_f32 = false)
{
    if (A->team2.built) return 0;
    Team2Dev t;
    crp::PhaseClock clk;
    const crp::PanelHost &h = panel_skeleton(A);
    clk.lap("ensure_team2: build_panels (R = 8, structure only)");
    crp::released_async<crp::Team2Host> th_owner;
    crp::Team2Host &th = *th_owner;
    th.compact = crp::team2_compact(h.fill(), for_f32);
    const std::vector<int> colpos = fmt_colpos(A);
    crp::build_team2(h, A->nrow, fmt_rowptr(A), fmt_colidx(A), &th, colpos.empty() ? nullptr : colpos.data(), &A->seed8);
    clk.lap("ensure_team2: build_team2");
    t.nteam = th.nteam;
    t.entries = th.real_entries;
    t.lattice = th.lattice;
    t.ngrid = (int) th.tgrid.size();
    hipError_t e = upload(t.torder, th.tgrid.data(), sizeof(int) * th.tgrid.size(), 4);      // the launch grid (panel_format.h)
    if (e == hipSuccess) e = upload(t.tpanel, th.tpanel.data(), sizeof(int) * th.tpanel.size(), 4);
    if (e == hipSuccess) e = upload(t.tinfo, th.tinfo.data(), sizeof(int) * th.tinfo.size(), 16);
    if (e == hipSuccess) e = upload(t.tpro, th.tpro.data(), sizeof(int) * th.tpro.size(), 8);
    if (e == hipSuccess) e = upload(t.trec, th.trec.data(), sizeof(uint32_t) * th.trec.size(), 1024);
    t.value_entries = th.nvalues;          // values of the streams
    t.compact = th.compact;
    if (e == hipSuccess) e = upload(t.tvoff, th.tvoff.data(), sizeof(long long) * th.tvoff.size(), 8);
    // the kernel requests 256 bytes per wave and round: up to four groups past a wave's last part.  The streams start as zeros in
    // HBM and take their values from the device CSR through the slot map: no copy of them is ever made on the host.
    if (e == hipSuccess) e = t.tval.alloc(sizeof(double) * (size_t) th.nvalues + 4096);
    if (e == hipSuccess) e = hipMemsetAsync(t.tval, 0, sizeof(double) * (size_t) th.nvalues + 4096, stream);
    if (e == hipSuccess) e = upload(t.tmap, th.vmap.data(), sizeof(uint32_t) * th.vmap.size(), 4);
    if (e != hipSuccess) return (int) e;
    if (A->nnz > 0) CRP_TRY(scatter_values(A, t, stream));
    CRP_TRY(hipStreamSynchronize(stream));
    clk.lap("ensure_team2: upload");
    t.built = true;
    A->team2 = std::move(t);
    drop_skeleton_when_done(A);
    return 0;
}

static void team2_args(const Team2Dev &d, crp::Team2Args *t)
{
    t->nteam = d.nteam; t->ngrid = d.ngrid; t->compact = d.compact; t->torder = d.torder; t->tpanel = d.tpanel;
    t->tinfo = d.tinfo; t->tpro = d.tpro; t->trec = d.trec; t->tvoff = d.tvoff; t->tval = d.tval; t->tval32 = d.tval32;
}

static int ensure_team2r(crp_csr_dev *A, hipStream_t stream, int G)
{
    Team2RDev &slot = A->team2r[G == 2 ? 1 : 0];
    if (slot.built) return 0;
    if (slot.refused) return -6;
    // a cheap bound first: a wave's block takes at least 10 bytes per nonzero (value + offset), and the streams address 34 GB
    if ((double) A->nnz * 10.0 > 34.0e9) { slot.refused = true; return -6; }
    Team2RDev t;
    crp::PhaseClock clk;
    const crp::PanelHost &h = panel_skeleton(A);
    clk.lap("ensure_team2r: build_panels (R = 8, structure only)");
    crp::released_async<crp::Team2RHost> th_owner;
    crp::Team2RHost &th = *th_owner;
    th.G = G == 2 ? 2 : 4;
    const std::vector<int> colpos = fmt_colpos(A);
    if (!crp::build_team2r(h, A->nrow, fmt_rowptr(A), fmt_colidx(A), &th, colpos.empty() ? nullptr : colpos.data(), &A->seed8))
    {
        slot.refused = true;                // too large for this format
        drop_skeleton_when_done(A);
        return -6;
    }
    clk.lap("ensure_team2r: build_team2r");
    t.G = th.G;
    t.nteam = th.nteam;
    t.lattice = th.lattice;
    t.ngrid = (int) th.tgrid.size();
    t.value_entries = th.nwords;
    hipError_t e = upload(t.tgrid, th.tgrid.data(), sizeof(int) * th.tgrid.size(), 4);
    if (e == hipSuccess) e = upload(t.tpanel, th.tpanel.data(), sizeof(int) * th.tpanel.size(), 4);
    if (e == hipSuccess) e = upload(t.tinfo, th.tinfo.data(), sizeof(int) * th.tinfo.size(), 16);
    if (e == hipSuccess) e = upload(t.trec, th.trec.data(), sizeof(uint32_t) * th.trec.size(), 1024);
    if (e == hipSuccess) e = upload(t.tvoff, th.tvoff.data(), sizeof(long long) * th.tvoff.size(), 8);
    // (the streams: values and uint16 offsets; a wave's DMAs take whole 16-byte lanes of its block)
    if (e == hipSuccess) e = upload(t.tval, th.tval.data(), sizeof(double) * th.tval.size(), 4096);
    if (e == hipSuccess) e = upload(t.tmap, th.vmap.data(), sizeof(uint32_t) * th.vmap.size(), 4);
    if (e == hipSuccess) e = upload(t.tent, th.tent.data(), sizeof(uint32_t) * th.tent.size(), 1024);
    if (e != hipSuccess) return (int) e;
    // (the streams were uploaded with their offsets and headers and 0.0 for every value: the values come from the device CSR)
    if (A->nnz > 0) CRP_TRY(scatter_values(A, t, stream));
    CRP_TRY(hipStreamSynchronize(stream));
    clk.lap("ensure_team2r: upload");
    t.built = true;
    slot = std::move(t);
    drop_skeleton_when_done(A);
    return 0;
}

// a row-major operand as the dispatch rules see it
static crp::Operand operand_of(int n, const void *B0, long long ldB0, const void *B1, long long ldB1, const void *C, long long ldC)
{
    crp::Operand op;
    op.n = n; op.ldB0 = ldB0; op.ldB1 = ldB1; op.ldC = ldC; op.has_b1 = B1 != nullptr;
    op.aligned16 = (((uintptr_t) B0 | (uintptr_t) B1 | (uintptr_t) C) % 16) == 0;
    return op;
}

// a malloc'd copy of v with one spare element (the host-only format helpers: the caller frees)
template <class V> static typename V::value_type *dup(const V &v)
{
    typedef typename V::value_type T;
    T *p = (T *) malloc(sizeof(T) * (v.size() + 1));
    if (!v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

static hipError_t sddmm_launch(const crp::SddmmArgs<double> &a, hipStream_t s) { return crp::sddmm_rm_f64(a, s); }
static hipError_t sddmm_launch(const crp::SddmmArgs<float> &a, hipStream_t s) { return crp::sddmm_rm_f32(a, s); }
// out[p] = < X[row(p)], Y[col(p)] > over A's pattern (sddmm_kernels.hip), one dtype.  Every argument is checked before anything is
// launched or allocated: a negative return has written nothing.
template <class T>
static int sddmm_csr(crp_csr_dev *A, int n, const T *X, long long ldX, const T *Y0, long long ldY0, const T *Y1, long long ldY1, T *out,
                     const int *out_pos, int mode, const T *val, hipStream_t s)
{
    crp::SddmmArgs<T> a;
    a.nrow = A->nrow; a.n = n; a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = val;
    a.X = X; a.ldX = ldX; a.Y0 = Y0; a.ldY0 = ldY0; a.Y1 = Y1; a.ldY1 = ldY1;
    a.out = out; a.rowmap = A->rowmap; a.out_pos = out_pos; a.mode = mode;
    return (int) sddmm_launch(a, s);
}
static int sddmm_check(const crp_csr_dev *A, int n, const void *X, long long ldX, const void *Y0, long long ldY0, const void *Y1,
                       long long ldY1, const void *out, int mode)
{
    if (A == NULL || X == NULL || out == NULL) return -1;
    if (n < 1 || (mode != 0 && mode != 1)) return -1;
    if (Y0 == NULL && A->b0_rows > 0) return -1;        // a column code names the first source
    if (Y1 == NULL && A->b1_rows > 0) return -1;        // a column code names the second source
    if (ldX < n || (Y0 != NULL && ldY0 < n) || (Y1 != NULL && ldY1 < n)) return -4;
    return 0;
}

// every argument is checked before anything is launched or allocated: a negative return has written nothing
static int attention_check(const crp_csr_dev *A, int nk, int nv, double scale, int bias, const void *Q, long long ldQ, const void *K0,
                           long long ldK0, const void *K1, long long ldK1, const void *V0, long long ldV0, const void *V1, long long ldV1,
                           const void *O, long long ldO, int heads = 1)
{
    if (A == NULL || Q == NULL || O == NULL) return -1;
    if (nk < 1 || nv < 1 || heads < 1 || (bias != 0 && bias != 1) || !std::isfinite(scale)) return -1;
    if ((K0 == NULL || V0 == NULL) && A->b0_rows > 0) return -1;        // a column code names the first source
    if ((K1 == NULL || V1 == NULL) && A->b1_rows > 0) return -1;        // a column code names the second source
    const long long wk = (long long) heads * nk, wv = (long long) heads * nv;      // (nk, nv: the widths of one head)
    if (ldQ < wk || ldO < wv) return -4;
    if ((K0 != NULL && ldK0 < wk) || (K1 != NULL && ldK1 < wk) || (V0 != NULL && ldV0 < wv) || (V1 != NULL && ldV1 < wv)) return -4;
    return 0;
}

// the fp32 copy of the values, as crp_sddmm_csr_f32 mode 1 derives it; the values in T for the bias, or nullptr
template <class T> static int attention_bias_values(crp_csr_dev *A, int bias, hipStream_t s, const T **val);
template <> int attention_bias_values<double>(crp_csr_dev *A, int bias, hipStream_t, const double **val)
{
    *val = bias ? (const double *) A->val : nullptr;
    return 0;
}
template <> int attention_bias_values<float>(crp_csr_dev *A, int bias, hipStream_t s, const float **val)
{
    *val = nullptr;
    if (bias != 1 || A->nnz == 0) return 0;
    const int rc = ensure_val32(A, s);
    if (rc != 0) return rc;
    *val = (const float *) A->val32;
    return 0;
}
// O = softmax_row(scale (Q K^T)|pattern(A) (+ A's values)) V (attention_kernels.hip), one dtype.  nk, nv: the widths of one head;
// mh: the (row, head) instances (the crp_attention_*_mh_* entry points, whatever their heads), else the single-head ones.
template <class T>
static int attention_fwd_csr(crp_csr_dev *A, int heads, bool mh, int nk, int nv, double scale, int bias, const T *Q, long long ldQ, const T *K0,
                             long long ldK0, const T *K1, long long ldK1, const T *V0, long long ldV0, const T *V1, long long ldV1, T *O,
                             long long ldO, T *lse, T *p_out, const int *out_pos, hipStream_t s)
{
    int rc = attention_check(A, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, heads);
    if (rc != 0 || A->nrow == 0) return rc;
    crp::AttnArgs<T> a;
    a.heads = heads;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nk = nk; a.nv = nv; a.rowptr = A->rowptr; a.colidx = A->colidx; a.scale = (T) scale;
    a.Q = Q; a.ldQ = ldQ; a.K0 = K0; a.ldK0 = ldK0; a.K1 = K1; a.ldK1 = ldK1; a.V0 = V0; a.ldV0 = ldV0; a.V1 = V1; a.ldV1 = ldV1;
    a.O = O; a.ldO = ldO; a.lse = lse; a.p_out = p_out; a.rowmap = A->rowmap; a.out_pos = out_pos;
    return (int) crp::attention_rm(a, mh, s);
}
// the fused backward (attention_bwd_kernels.hip), one dtype.  Every argument is checked before anything is launched or
// allocated: a negative return has written nothing.  nk, nv: the widths of one head (the cap is theirs); mh: the (row, head)
// instances.
template <class T>
static int attention_bwd_q_csr(crp_csr_dev *A, int nk, int nv, double scale, int bias, const T *Q, long long ldQ, const T *K0, long long ldK0,
                               const T *K1, long long ldK1, const T *V0, long long ldV0, const T *V1, long long ldV1, const T *O,
                               long long ldO, const T *dO, long long lddO, const T *lse, T *dQ, long long lddQ, T *delta, T *ds_out,
                               const int *out_pos, hipStream_t s, bool mh = false, int heads = 1)
{
    int rc = attention_check(A, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, heads);
    if (rc == 0 && (dO == NULL || lse == NULL || dQ == NULL || delta == NULL)) rc = -1;
    if (rc == 0 && (lddO < (long long) heads * nv || lddQ < (long long) heads * nk)) rc = -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (rc == 0 && (nk > cap || nv > cap)) rc = CRP_ATTN_BWD_EWIDTH;
    if (rc != 0 || A->nrow == 0) return rc;
    crp::AttnBwdQArgs<T> a;
    a.heads = heads;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nk = nk; a.nv = nv; a.rowptr = A->rowptr; a.colidx = A->colidx; a.scale = (T) scale;
    a.Q = Q; a.ldQ = ldQ; a.K0 = K0; a.ldK0 = ldK0; a.K1 = K1; a.ldK1 = ldK1; a.V0 = V0; a.ldV0 = ldV0; a.V1 = V1; a.ldV1 = ldV1;
    a.O = O; a.ldO = ldO; a.dO = dO; a.lddO = lddO; a.lse = lse; a.dQ = dQ; a.lddQ = lddQ; a.delta = delta; a.ds_out = ds_out;
    a.rowmap = A->rowmap; a.out_pos = out_pos;
    return (int) crp::attention_bwd_q(a, mh, s);
}
template <class T>
static int attention_bwd_kv_csr(crp_csr_dev *At, int nk, int nv, double scale, int bias, const T *K, long long ldK, const T *V, long long ldV,
                                const T *Q, long long ldQ, const T *dO, long long lddO, const T *lse, const T *delta, T *dK,
                                long long lddK, T *dV, long long lddV, hipStream_t s, bool mh = false, int heads = 1)
{
    if (At == NULL || K == NULL || V == NULL || dK == NULL || dV == NULL) return -1;
    if (nk < 1 || nv < 1 || heads < 1 || (bias != 0 && bias != 1) || !std::isfinite(scale)) return -1;
    if (At->b1_rows > 0) return -1;                      // a code names a second source: this call takes one
    if ((Q == NULL || dO == NULL || lse == NULL || delta == NULL) && At->nnz > 0) return -1;
    const long long wk = (long long) heads * nk, wv = (long long) heads * nv;
    if (ldK < wk || lddK < wk || ldV < wv || lddV < wv) return -4;
    if (At->nnz > 0 && (ldQ < wk || lddO < wv)) return -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (nk > cap || nv > cap) return CRP_ATTN_BWD_EWIDTH;
    if (At->nrow == 0) return 0;
    crp::AttnBwdKVArgs<T> a;
    a.heads = heads;
    const int rc = attention_bias_values<T>(At, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = At->nrow; a.nk = nk; a.nv = nv; a.rowptr = At->rowptr; a.colidx = At->colidx; a.scale = (T) scale;
    a.K = K; a.ldK = ldK; a.V = V; a.ldV = ldV; a.Q = Q; a.ldQ = ldQ; a.dO = dO; a.lddO = lddO; a.lse = lse; a.delta = delta;
    a.dK = dK; a.lddK = lddK; a.dV = dV; a.lddV = lddV; a.rowmap = At->rowmap;
    return (int) crp::attention_bwd_kv(a, mh, s);
}

// ---- the fused GAT attention (gat_kernels.hip), one dtype.  Every argument is checked before anything is launched or allocated: a
// negative return has written nothing.  dv: the width of one head.  drop, seed: the attention dropout of the _drop_ entry points
// (dropout.h); the plain entry points pass 0, which takes the instances without it.
static bool drop_rate_ok(double drop) { return drop >= 0.0 && drop < 1.0; }         // (NaN fails both)
static int gat_check(const crp_csr_dev *A, int heads, int dv, double slope, int bias, const void *el, long long ldel, const void *er0,
                     long long lder0, const void *er1, long long lder1, const void *V0, long long ldV0, const void *V1, long long ldV1,
                     const void *O, long long ldO, double drop)
{
    if (A == NULL || el == NULL || O == NULL) return -1;
    if (heads < 1 || dv < 1 || (bias != 0 && bias != 1) || !std::isfinite(slope) || !drop_rate_ok(drop)) return -1;
    if ((er0 == NULL || V0 == NULL) && A->b0_rows > 0) return -1;       // a column code names the first source
    if ((er1 == NULL || V1 == NULL) && A->b1_rows > 0) return -1;       // a column code names the second source
    const long long wv = (long long) heads * dv;
    if (ldel < heads || ldO < wv) return -4;
    if ((er0 != NULL && lder0 < heads) || (er1 != NULL && lder1 < heads) || (V0 != NULL && ldV0 < wv) || (V1 != NULL && ldV1 < wv)) return -4;
    return 0;
}
template <class T>
static int gat_fwd_csr(crp_csr_dev *A, int heads, int dv, double slope, int bias, const T *el, long long ldel, const T *er0, long long lder0,
                       const T *er1, long long lder1, const T *V0, long long ldV0, const T *V1, long long ldV1, T *O, long long ldO, T *lse,
                       T *p_out, const int *out_pos, hipStream_t s, double drop = 0.0, unsigned long long seed = 0)
{
    int rc = gat_check(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, drop);
    if (rc != 0 || A->nrow == 0) return rc;
    crp::GatArgs<T> a;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nv = dv; a.heads = heads; a.rowptr = A->rowptr; a.colidx = A->colidx; a.slope = (T) slope;
    a.el = el; a.ldel = ldel; a.er0 = er0; a.lder0 = lder0; a.er1 = er1; a.lder1 = lder1;
    a.V0 = V0; a.ldV0 = ldV0; a.V1 = V1; a.ldV1 = ldV1;
    a.O = O; a.ldO = ldO; a.lse = lse; a.p_out = p_out; a.rowmap = A->rowmap; a.out_pos = out_pos;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gat_attention_rm(a, s);
}
template <class T>
static int gat_bwd_row_csr(crp_csr_dev *A, int heads, int dv, double slope, int bias, const T *el, long long ldel, const T *er0, long long lder0,
                           const T *er1, long long lder1, const T *V0, long long ldV0, const T *V1, long long ldV1, const T *O, long long ldO,
                           const T *dO, long long lddO, const T *lse, T *d_el, long long ldd_el, T *delta, T *ds_out, const int *out_pos,
                           hipStream_t s, double drop = 0.0, unsigned long long seed = 0)
{
    int rc = gat_check(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, drop);
    if (rc == 0 && (dO == NULL || lse == NULL || d_el == NULL || delta == NULL)) rc = -1;
    if (rc == 0 && (lddO < (long long) heads * dv || ldd_el < heads)) rc = -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (rc == 0 && dv > cap) rc = CRP_ATTN_BWD_EWIDTH;
    if (rc != 0 || A->nrow == 0) return rc;
    crp::GatBwdRowArgs<T> a;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nv = dv; a.heads = heads; a.rowptr = A->rowptr; a.colidx = A->colidx; a.slope = (T) slope;
    a.el = el; a.ldel = ldel; a.er0 = er0; a.lder0 = lder0; a.er1 = er1; a.lder1 = lder1;
    a.V0 = V0; a.ldV0 = ldV0; a.V1 = V1; a.ldV1 = ldV1;
    a.O = O; a.ldO = ldO; a.dO = dO; a.lddO = lddO; a.lse = lse; a.d_el = d_el; a.ldd_el = ldd_el; a.delta = delta; a.ds_out = ds_out;
    a.rowmap = A->rowmap; a.out_pos = out_pos;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gat_attention_bwd_row(a, s);
}
template <class T>
static int gat_bwd_col_csr(crp_csr_dev *At, int heads, int dv, double slope, int bias, const T *er, long long lder, const T *V, long long ldV,
                           const T *el, long long ldel, const T *dO, long long lddO, const T *lse, const T *delta, T *d_er, long long ldd_er,
                           T *dV, long long lddV, hipStream_t s, double drop = 0.0, unsigned long long seed = 0)
{
    if (At == NULL || er == NULL || V == NULL || d_er == NULL || dV == NULL) return -1;
    if (heads < 1 || dv < 1 || (bias != 0 && bias != 1) || !std::isfinite(slope) || !drop_rate_ok(drop)) return -1;
    if (At->b1_rows > 0) return -1;                      // a code names a second source: this call takes one
    if ((el == NULL || dO == NULL || lse == NULL || delta == NULL) && At->nnz > 0) return -1;
    const long long wv = (long long) heads * dv;
    if (lder < heads || ldd_er < heads || ldV < wv || lddV < wv) return -4;
    if (At->nnz > 0 && (ldel < heads || lddO < wv)) return -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (dv > cap) return CRP_ATTN_BWD_EWIDTH;
    if (At->nrow == 0) return 0;
    crp::GatBwdColArgs<T> a;
    const int rc = attention_bias_values<T>(At, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = At->nrow; a.nv = dv; a.heads = heads; a.rowptr = At->rowptr; a.colidx = At->colidx; a.slope = (T) slope;
    a.er = er; a.lder = lder; a.V = V; a.ldV = ldV; a.el = el; a.ldel = ldel; a.dO = dO; a.lddO = lddO; a.lse = lse; a.delta = delta;
    a.d_er = d_er; a.ldd_er = ldd_er; a.dV = dV; a.lddV = lddV; a.rowmap = At->rowmap;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gat_attention_bwd_col(a, s);
}

// ---- the fused GATv2 attention (gatv2_kernels.hip), one dtype.  Every argument is checked before anything is launched or allocated:
// a negative return has written nothing.  dv: the width of one head, capped in both directions.
template <class T>
static int gatv2_check(const crp_csr_dev *A, int heads, int dv, double slope, int bias, const void *XT, long long ldXT, const void *XS0,
                       long long ldXS0, const void *XS1, long long ldXS1, const void *av, const void *O, long long ldO, double drop)
{
    if (A == NULL || XT == NULL || av == NULL || O == NULL) return -1;
    if (heads < 1 || dv < 1 || (bias != 0 && bias != 1) || !std::isfinite(slope) || !drop_rate_ok(drop)) return -1;
    if (XS0 == NULL && A->b0_rows > 0) return -1;        // a column code names the first source
    if (XS1 == NULL && A->b1_rows > 0) return -1;        // a column code names the second source
    const long long wv = (long long) heads * dv;
    if (ldXT < wv || ldO < wv || (XS0 != NULL && ldXS0 < wv) || (XS1 != NULL && ldXS1 < wv)) return -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (dv > cap) return CRP_GATV2_EWIDTH;
    return 0;
}
template <class T>
static int gatv2_fwd_csr(crp_csr_dev *A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT, const T *XS0, long long ldXS0,
                         const T *XS1, long long ldXS1, const T *av, T *O, long long ldO, T *lse, T *p_out, const int *out_pos, hipStream_t s,
                         double drop = 0.0, unsigned long long seed = 0)
{
    int rc = gatv2_check<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, av, O, ldO, drop);
    if (rc != 0 || A->nrow == 0) return rc;
    crp::Gatv2Args<T> a;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nv = dv; a.heads = heads; a.rowptr = A->rowptr; a.colidx = A->colidx; a.slope = (T) slope;
    a.XT = XT; a.ldXT = ldXT; a.XS0 = XS0; a.ldXS0 = ldXS0; a.XS1 = XS1; a.ldXS1 = ldXS1; a.av = av;
    a.O = O; a.ldO = ldO; a.lse = lse; a.p_out = p_out; a.rowmap = A->rowmap; a.out_pos = out_pos;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gatv2_attention_rm(a, s);
}
template <class T>
static int gatv2_bwd_row_csr(crp_csr_dev *A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT, const T *XS0,
                             long long ldXS0, const T *XS1, long long ldXS1, const T *av, const T *O, long long ldO, const T *dO, long long lddO,
                             const T *lse, T *dXT, long long lddXT, T *da_part, long long ldda, T *delta, T *ds_out, const int *out_pos,
                             hipStream_t s, double drop = 0.0, unsigned long long seed = 0)
{
    int rc = 0;
    if (A == NULL || dO == NULL || lse == NULL || dXT == NULL || da_part == NULL || delta == NULL) rc = -1;
    if (rc == 0) rc = gatv2_check<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, av, O, ldO, drop);
    if (rc == 0 || rc == CRP_GATV2_EWIDTH)
    {
        const long long wv = (long long) heads * dv;
        if (lddO < wv || lddXT < wv || ldda < wv) rc = -4;
    }
    if (rc != 0 || A->nrow == 0) return rc;
    crp::Gatv2BwdRowArgs<T> a;
    rc = attention_bias_values<T>(A, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = A->nrow; a.nv = dv; a.heads = heads; a.rowptr = A->rowptr; a.colidx = A->colidx; a.slope = (T) slope;
    a.XT = XT; a.ldXT = ldXT; a.XS0 = XS0; a.ldXS0 = ldXS0; a.XS1 = XS1; a.ldXS1 = ldXS1; a.av = av;
    a.O = O; a.ldO = ldO; a.dO = dO; a.lddO = lddO; a.lse = lse; a.dXT = dXT; a.lddXT = lddXT; a.da_part = da_part; a.ldda = ldda;
    a.delta = delta; a.ds_out = ds_out; a.rowmap = A->rowmap; a.out_pos = out_pos;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gatv2_attention_bwd_row(a, s);
}
template <class T>
static int gatv2_bwd_col_csr(crp_csr_dev *At, int heads, int dv, double slope, int bias, const T *XS, long long ldXS, const T *XT,
                             long long ldXT, const T *av, const T *dO, long long lddO, const T *lse, const T *delta, T *dXS, long long lddXS,
                             hipStream_t s, double drop = 0.0, unsigned long long seed = 0)
{
    if (At == NULL || XS == NULL || av == NULL || dXS == NULL) return -1;
    if (heads < 1 || dv < 1 || (bias != 0 && bias != 1) || !std::isfinite(slope) || !drop_rate_ok(drop)) return -1;
    if (At->b1_rows > 0) return -1;                      // a code names a second source: this call takes one
    if ((XT == NULL || dO == NULL || lse == NULL || delta == NULL) && At->nnz > 0) return -1;
    const long long wv = (long long) heads * dv;
    if (ldXS < wv || lddXS < wv) return -4;
    if (At->nnz > 0 && (ldXT < wv || lddO < wv)) return -4;
    constexpr int cap = crp::ATTN_BWD_MAX_PIECES * 64 * (16 / (int) sizeof(T));
    if (dv > cap) return CRP_GATV2_EWIDTH;
    if (At->nrow == 0) return 0;
    crp::Gatv2BwdColArgs<T> a;
    const int rc = attention_bias_values<T>(At, bias, s, &a.val);
    if (rc != 0) return rc;
    a.nrow = At->nrow; a.nv = dv; a.heads = heads; a.rowptr = At->rowptr; a.colidx = At->colidx; a.slope = (T) slope;
    a.XS = XS; a.ldXS = ldXS; a.XT = XT; a.ldXT = ldXT; a.av = av; a.dO = dO; a.lddO = lddO; a.lse = lse; a.delta = delta;
    a.dXS = dXS; a.lddXS = lddXS; a.rowmap = At->rowmap;
    a.drop = crp::dropout_args<T>(drop, seed);
    return (int) crp::gatv2_attention_bwd_col(a, s);
}

extern "C" {

const char *crp_hip_version(void) { return "crpspmm-hip 0.1 gfx950"; }

int crp_hip_device_count(int *count)
{
    if (count == NULL) return -1;
    *count = 0;
    CRP_TRY(hipGetDeviceCount(count));
    return 0;
}

int crp_hip_set_device(int dev) { CRP_TRY(hipSetDevice(dev)); return 0; }
int crp_hip_get_device(int *dev) { if (!dev) return -1; CRP_TRY(hipGetDevice(dev)); return 0; }

int crp_hip_device_info(int dev, char *name, int *cu_count, size_t *hbm_bytes)
{
    hipDeviceProp_t prop;
    CRP_TRY(hipGetDeviceProperties(&prop, dev));
    if (name) snprintf(name, 256, "%s (%s)", prop.name, prop.gcnArchName);
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return 0;
}

int crp_hip_device_bus_id(char *out, size_t len)
{
    if (out == NULL || len < 16) return -1;
    int dev = 0;
    CRP_TRY(hipGetDevice(&dev));
    CRP_TRY(hipDeviceGetPCIBusId(out, (int) len, dev));
    return 0;
}

int crp_dev_malloc(void **ptr, size_t bytes)
{
    if (ptr == NULL) return -1;
    *ptr = NULL;
    if (bytes == 0) return 0;
    CRP_TRY(hipMalloc(ptr, bytes));
    return 0;
}

int crp_dev_free(void *ptr)
{
    if (ptr == NULL) return 0;
    CRP_TRY(hipFree(ptr));
    return 0;
}

int crp_dev_memset(void *ptr, int value, size_t bytes, void *stream)
{
    if (bytes == 0) return 0;
    CRP_TRY(hipMemsetAsync(ptr, value, bytes, (hipStream_t) stream));
    return 0;
}

static const hipMemcpyKind k_copy_kinds[] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice};   // kind 0, 1, 2
int crp_dev_memcpy(void *dst, const void *src, size_t bytes, int kind, void *stream)
{
    if (bytes == 0) return 0;
    if (kind < 0 || kind > 2) return -1;
    CRP_TRY(hipMemcpyAsync(dst, src, bytes, k_copy_kinds[kind], (hipStream_t) stream));
    return 0;
}

int crp_dev_memcpy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height,
                     int kind, void *stream)
{
    if (width_bytes == 0 || height == 0) return 0;
    if (kind < 0 || kind > 2) return -1;
    CRP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, k_copy_kinds[kind], (hipStream_t) stream));
    return 0;
}

int crp_host_malloc(void **ptr, size_t bytes)
{
    if (ptr == NULL) return -1;
    *ptr = NULL;
    if (bytes == 0) return 0;
    CRP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return 0;
}

int crp_host_free(void *ptr)
{
    if (ptr == NULL) return 0;
    CRP_TRY(hipHostFree(ptr));
    return 0;
}

int crp_dev_ptr_is_device(const void *ptr, int *is_dev)
{
    if (is_dev == NULL) return -1;
    *is_dev = 0;
    if (ptr == NULL) return 0;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, ptr);
    if (e != hipSuccess)
    {
        (void) hipGetLastError();   // plain malloc'd host memory is "invalid value": not an error for us
        return 0;
    }
    *is_dev = (attr.type == hipMemoryTypeDevice) ? 1 : 0;
    return 0;
}

int crp_stream_create(void **stream)
{
    if (stream == NULL) return -1;
    hipStream_t s;
    CRP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *) s;
    return 0;
}
int crp_stream_create_cu_mask(void **stream, int nwords, const unsigned *mask32)
{
    if (stream == NULL || nwords <= 0 || mask32 == NULL) return -1;
    hipStream_t s;
    CRP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t) nwords, mask32));
    *stream = (void *) s;
    return 0;
}
int crp_probe_copy(long long bytes, const void *src, void *dst, int blocks, unsigned long long *stamps, void *stream)
{
    if (bytes <= 0 || (bytes & 15) || src == NULL || dst == NULL || stamps == NULL) return -1;
    CRP_TRY(crp::probe_copy(bytes, src, dst, blocks, stamps, (hipStream_t) stream));
    return 0;
}
int crp_probe_stamp(unsigned long long *out, void *stream)
{
    if (out == NULL) return -1;
    CRP_TRY(crp::probe_stamp(out, (hipStream_t) stream));
    return 0;
}
int crp_stream_destroy(void *stream) { if (stream) CRP_TRY(hipStreamDestroy((hipStream_t) stream)); return 0; }
int crp_stream_sync(void *stream) { CRP_TRY(hipStreamSynchronize((hipStream_t) stream)); return 0; }

int crp_event_create(void **event)
{
    if (event == NULL) return -1;
    hipEvent_t e;
    CRP_TRY(hipEventCreate(&e));
    *event = (void *) e;
    return 0;
}
int crp_event_destroy(void *event) { if (event) CRP_TRY(hipEventDestroy((hipEvent_t) event)); return 0; }
int crp_event_record(void *event, void *stream) { CRP_TRY(hipEventRecord((hipEvent_t) event, (hipStream_t) stream)); return 0; }
int crp_event_sync(void *event) { CRP_TRY(hipEventSynchronize((hipEvent_t) event)); return 0; }
int crp_stream_wait_event(void *stream, void *event)
{
    CRP_TRY(hipStreamWaitEvent((hipStream_t) stream, (hipEvent_t) event, 0));
    return 0;
}
int crp_event_elapsed_ms(void *start, void *stop, float *ms)
{
    if (ms == NULL) return -1;
    CRP_TRY(hipEventElapsedTime(ms, (hipEvent_t) start, (hipEvent_t) stop));
    return 0;
}

// ---------------------------------------------------------------------------
// dst_val[dst_rowptr[t] + k] = src_val[src_start[t] + k]: the values of selected rows of a matrix whose values already sit in
// HBM (crp_csr_dev_create_dv); one wave per row
__global__ void gather_row_vals_kernel(const int nrow, const int *__restrict__ dst_rowptr, const int *__restrict__ src_start,
                                       const double *__restrict__ src_val, double *__restrict__ dst_val)
{
    const int lane = threadIdx.x & 63;
    const long long wave0 = ((long long) blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = ((long long) gridDim.x * blockDim.x) >> 6;
    for (long long t = wave0; t < nrow; t += nwave)
    {
        const int d0 = dst_rowptr[t], len = dst_rowptr[t + 1] - d0;
        const long long s0 = src_start[t];
        for (int k = lane; k < len; k += 64) dst_val[(long long) d0 + k] = src_val[s0 + k];
    }
}

// the host side of a handle whose device CSR is in place: the host copies, the locality order, the traits
static int csr_dev_host_side(crp_csr_dev *A, const int *rowptr, const int *colidx, const double *val)
{
    const int nrow = A->nrow, ncol = A->ncol;
    const long long nnz = A->nnz;
    for (long long p = 0; p < nnz; p++)
    {
        const int c = colidx[p];
        if (c >= 0) { if (c + 1LL > A->b0_rows) A->b0_rows = c + 1LL; }
        else if ((long long) (~c) + 1 > A->b1_rows) A->b1_rows = (long long) (~c) + 1;
    }
    if (A->b0_rows > ncol && ncol > 0) return -2;      // a column index addresses a row past B0
    A->h_rowptr.assign(rowptr, rowptr + nrow + 1);
    if (nnz > 0)
    {
        A->h_colidx.assign(colidx, colidx + nnz);
        A->h_val.assign(val, val + nnz);
    }
    A->ord = crp::format_order(nrow, ncol, rowptr, colidx, A->b1_rows > 0);
    if (!A->ord.perm.empty())
    {
        A->f_val.resize((size_t) nnz);
        for (long long q = 0; q < nnz; q++) A->f_val[(size_t) q] = val[A->ord.f_nz[(size_t) q]];
        CRP_TRY(upload(A->rowmap_fmt, A->ord.perm.data(), sizeof(int) * (size_t) nrow, 0));
    }
    A->traits = crp::matrix_traits(nrow, fmt_rowptr(A), fmt_colidx(A));
    // (the derived formats are built by the first product that uses them: a matrix multiplied by wide operands only never
    //  needs its row-panel format -- 20 GB for the nlpkkt240-size stand-in)
    return 0;
}

static int csr_dev_create_impl(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, const double *val_dev,
                               const int *src_start, crp_csr_dev_p *out)
{
    if (out == NULL) return -1;
    *out = NULL;
    if (nrow < 0 || ncol < 0 || rowptr == NULL) return -1;
    if (rowptr[0] != 0) return -2;
    const long long nnz = rowptr[nrow];
    if (nnz < 0) return -2;
    if (nnz > 0 && (colidx == NULL || val == NULL)) return -1;
    std::unique_ptr<crp_csr_dev> A(new (std::nothrow) crp_csr_dev);
    if (A == NULL) return -3;
    A->nrow = nrow;
    A->ncol = ncol;
    A->nnz  = nnz;
    hipError_t e = A->rowptr.alloc(sizeof(int) * ((size_t) nrow + 1));
    if (e == hipSuccess) e = A->colidx.alloc(sizeof(int) * (size_t) (nnz > 0 ? nnz : 1));
    if (e == hipSuccess) e = A->val.alloc(sizeof(double) * (size_t) (nnz > 0 ? nnz : 1));
    if (e == hipSuccess) e = hipMemcpy(A->rowptr, rowptr, sizeof(int) * ((size_t) nrow + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(A->colidx, colidx, sizeof(int) * (size_t) nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0 && val_dev == nullptr) e = hipMemcpy(A->val, val, sizeof(double) * (size_t) nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0 && val_dev != nullptr)
    {
        // the values are in HBM already (a panel replicated between devices): no second trip over PCIe
        if (src_start == nullptr) e = hipMemcpy(A->val, val_dev, sizeof(double) * (size_t) nnz, hipMemcpyDeviceToDevice);
        else
        {
            DevBuf<int> d_start;
            e = d_start.alloc(sizeof(int) * (size_t) (nrow > 0 ? nrow : 1));
            if (e == hipSuccess && nrow > 0) e = hipMemcpy(d_start, src_start, sizeof(int) * (size_t) nrow, hipMemcpyHostToDevice);
            if (e == hipSuccess && nrow > 0)
            {
                const int blocks = (int) std::min<long long>(((long long) nrow + 3) / 4, 65536);
                hipLaunchKernelGGL(gather_row_vals_kernel, dim3(blocks), dim3(256), 0, 0, nrow, A->rowptr, d_start, val_dev, A->val);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipDeviceSynchronize();
            }
        }
    }
    if (e != hipSuccess) return (int) e;
    const int rc = csr_dev_host_side(A.get(), rowptr, colidx, val);
    if (rc != 0) return rc;
    *out = A.release();
    return 0;
}

int crp_csr_dev_create(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val,
                       crp_csr_dev_p *out)
{
    return csr_dev_create_impl(nrow, ncol, rowptr, colidx, val, nullptr, nullptr, out);
}

int crp_csr_dev_create_dv(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val_host, const double *val_dev,
                          const int *src_start, crp_csr_dev_p *out)
{
    if (val_dev == NULL) return -1;
    return csr_dev_create_impl(nrow, ncol, rowptr, colidx, val_host, val_dev, src_start, out);
}

int crp_csr_dev_create_t(int nrow, int ncol, const int *rowptr, const int *colidx, const double *val, crp_csr_dev_p *out)
{
    if (out == NULL) return CRP_CSR_T_EARG;
    *out = NULL;
    if (nrow < 0 || ncol < 0 || rowptr == NULL) return CRP_CSR_T_EARG;
    if (rowptr[0] != 0) return CRP_CSR_T_EPTR;
    const long long nnz = rowptr[nrow];
    if (nnz < 0) return CRP_CSR_T_EPTR;
    if (nnz > 0 && (colidx == NULL || val == NULL)) return CRP_CSR_T_EARG;
    std::unique_ptr<crp_csr_dev> A(new (std::nothrow) crp_csr_dev);
    if (A == NULL) return -3;
    A->nrow = ncol;                                  // the handle is A^T
    A->ncol = nrow;
    A->nnz  = nnz;
    const size_t n1 = (size_t) (nnz > 0 ? nnz : 1);
    // A's arrays go up once, into temporaries that live until the transpose is done
    DevBuf<int> a_rowptr, a_colidx;
    DevBuf<double> a_val;
    hipError_t e = a_rowptr.alloc(sizeof(int) * ((size_t) nrow + 1));
    if (e == hipSuccess) e = a_colidx.alloc(sizeof(int) * n1);
    if (e == hipSuccess) e = a_val.alloc(sizeof(double) * n1);
    if (e == hipSuccess) e = A->rowptr.alloc(sizeof(int) * ((size_t) ncol + 1));
    if (e == hipSuccess) e = A->colidx.alloc(sizeof(int) * n1);
    if (e == hipSuccess) e = A->val.alloc(sizeof(double) * n1);
    if (e == hipSuccess) e = A->tmap.alloc(sizeof(int) * n1);
    if (e == hipSuccess) e = hipMemcpy(a_rowptr, rowptr, sizeof(int) * ((size_t) nrow + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(a_colidx, colidx, sizeof(int) * (size_t) nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(a_val, val, sizeof(double) * (size_t) nnz, hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int) e;
    int rc = crp::csr_transpose_dev(nrow, ncol, a_rowptr, a_colidx, a_val, A->rowptr, A->colidx, A->val, A->tmap, nullptr);
    if (rc != 0) return rc;
    // the transposed arrays come back for the host-side format builders; tmap stays in device memory as well
    std::vector<int> t_rowptr((size_t) ncol + 1), t_colidx(n1);
    std::vector<double> t_val(n1);
    A->h_tmap.resize((size_t) nnz);
    e = hipMemcpy(t_rowptr.data(), A->rowptr, sizeof(int) * ((size_t) ncol + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(t_colidx.data(), A->colidx, sizeof(int) * (size_t) nnz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(t_val.data(), A->val, sizeof(double) * (size_t) nnz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(A->h_tmap.data(), A->tmap, sizeof(int) * (size_t) nnz, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int) e;
    rc = csr_dev_host_side(A.get(), t_rowptr.data(), t_colidx.data(), t_val.data());
    if (rc != 0) return rc;
    *out = A.release();
    return 0;
}

int crp_csr_dev_is_transposed(crp_csr_dev_p A) { return A ? (A->tmap ? 1 : 0) : -1; }

int crp_csr_dev_destroy(crp_csr_dev_p *A_)
{
    if (A_ == NULL || *A_ == NULL) return 0;
    delete *A_;
    *A_ = NULL;
    return 0;
}

int crp_csr_dev_update_values(crp_csr_dev_p A, const double *val, void *stream)
{
    if (A == NULL || (val == NULL && A->nnz > 0)) return -1;
    if (A->nnz == 0) return 0;
    // the slot maps of the derived formats are 32-bit
    for (int i = 0; i < 2; i++)
        if (A->pan[i].built && A->pan[i].entries * (long long) A->pan[i].R >= (1LL << 32)) return -5;
    if (A->team2.built && A->team2.value_entries >= (1LL << 32)) return -5;
    for (const Team2RDev &t : A->team2r)
        if (t.built && t.value_entries >= (1LL << 32)) return -5;
    int is_dev = 0;
    crp_dev_ptr_is_device(val, &is_dev);
    const hipStream_t s = (hipStream_t) stream;
    // a handle for A^T (crp_csr_dev_create_t) takes val in A's order: from device memory the device CSR gathers it through tmap,
    // from host memory the host copy does the same gather and goes up as it is
    if (A->tmap && is_dev) CRP_TRY(crp::gather_vals_f64(A->nnz, A->tmap, val, A->val, s));
    else
    {
        if (A->tmap)
            for (long long q = 0; q < A->nnz; q++) A->h_val[(size_t) q] = val[A->h_tmap[(size_t) q]];
        CRP_TRY(hipMemcpyAsync(A->val, A->tmap ? A->h_val.data() : val, sizeof(double) * (size_t) A->nnz,
                               is_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
    if (!is_dev)
    {
        if (!A->tmap) memcpy(A->h_val.data(), val, sizeof(double) * (size_t) A->nnz);   // formats built later see the new values
        for (size_t q = 0; q < A->f_val.size(); q++) A->f_val[q] = A->h_val[(size_t) A->ord.f_nz[q]];
        A->host_vals_stale = false;
    }
    else A->host_vals_stale = true;      // formats built later are refreshed from the device CSR (ensure_*)
    for (const PanelDev &d : A->pan)
        if (d.built) CRP_TRY(scatter_values(A, d, s));
    if (A->team2.built) CRP_TRY(scatter_values(A, A->team2, s));
    for (const Team2RDev &d : A->team2r)
        if (d.built) CRP_TRY(scatter_values(A, d, s));
    // fp32 copies follow
    if (A->val32) CRP_TRY(crp::convert_f64_f32(A->nnz, A->val, A->val32, s));
    if (A->team2.tval32) CRP_TRY(crp::convert_f64_f32(A->team2.value_entries, A->team2.tval, A->team2.tval32, s));
    return 0;
}

int crp_csr_dev_set_rowmap(crp_csr_dev_p A, const int *rowmap, int c_nrow)
{
    if (A != NULL) A->rowmap_epoch++;
    if (A == NULL || (rowmap != NULL && c_nrow < 0)) return -1;
    A->rowmap.reset();
    A->c_nrow = A->nrow;
    A->h_rowmap.clear();
    if (!A->ord.perm.empty())        // formats in processing order: C row of position i = map[perm[i]]
    {
        std::vector<int> comp(A->ord.perm);
        if (rowmap != NULL)
            for (int i = 0; i < A->nrow; i++)
            {
                const int r = rowmap[A->ord.perm[(size_t) i]];
                if (r < 0 || r >= c_nrow) return -2;
                comp[(size_t) i] = r;
            }
        CRP_TRY(hipMemcpy(A->rowmap_fmt, comp.data(), sizeof(int) * (size_t) A->nrow, hipMemcpyHostToDevice));
    }
    if (rowmap == NULL || A->nrow == 0) return 0;
    for (int i = 0; i < A->nrow; i++)
        if (rowmap[i] < 0 || rowmap[i] >= c_nrow) return -2;
    CRP_TRY(upload(A->rowmap, rowmap, sizeof(int) * (size_t) A->nrow, 0));
    A->h_rowmap.assign(rowmap, rowmap + A->nrow);
    A->c_nrow = c_nrow;
    return 0;
}


int crp_csr_dev_nrow(crp_csr_dev_p A) { return A ? A->nrow : -1; }
long long crp_csr_dev_nnz(crp_csr_dev_p A) { return A ? A->nnz : -1; }
long long crp_csr_dev_bytes(crp_csr_dev_p A) { return A ? 12LL * A->nnz + 4LL * ((long long) A->nrow + 1) : -1; }

// csr_mat_row_part_comm_size (/root/reference/src/spmat_part.c:38-64) on the device-resident CSR of A: the re-plan case -- the
// matrix is in HBM already, so nothing but the two partition arrays goes up and nblk + 1 ints come down.
int crp_csr_dev_row_part_comm_size(crp_csr_dev_p A, int nblk, const int *rblk_ptr, const int *x_displs, int *comm_sizes, int *total_size)
{
    if (A == NULL || nblk < 1 || rblk_ptr == NULL || x_displs == NULL || comm_sizes == NULL || total_size == NULL) return -1;
    if (rblk_ptr[0] != 0 || rblk_ptr[nblk] != A->nrow) return -2;
    for (int b = 0; b < nblk; b++)
        if (rblk_ptr[b + 1] < rblk_ptr[b] || x_displs[b + 1] < x_displs[b] || x_displs[b] < 0 || x_displs[b + 1] > A->ncol) return -2;
    const long long words = ((long long) A->ncol + 31) / 32;
    DevBuf<unsigned> bits;
    DevBuf<int> dv;                         // rblk (nblk + 1), xd (nblk + 1), comm (nblk), bad (1)
    const size_t nint = (size_t) 3 * (size_t) nblk + 3;
    hipError_t e = bits.alloc(sizeof(unsigned) * (size_t) std::max<long long>(words * nblk, 1));
    if (e == hipSuccess) e = dv.alloc(sizeof(int) * nint);
    if (e == hipSuccess) e = hipMemset(bits, 0, sizeof(unsigned) * (size_t) std::max<long long>(words * nblk, 1));
    if (e == hipSuccess) e = hipMemset(dv, 0, sizeof(int) * nint);
    if (e == hipSuccess) e = hipMemcpy(dv, rblk_ptr, sizeof(int) * ((size_t) nblk + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dv + nblk + 1, x_displs, sizeof(int) * ((size_t) nblk + 1), hipMemcpyHostToDevice);
    int *comm_dev = dv + 2 * (nblk + 1), *bad_dev = comm_dev + nblk;
    if (e == hipSuccess) e = crp::row_part_comm_size(A->nrow, A->ncol, A->rowptr, A->colidx, nblk, dv, dv + nblk + 1, bits, comm_dev, bad_dev, 0);
    std::vector<int> out((size_t) nblk + 1, 0);
    if (e == hipSuccess) e = hipMemcpy(out.data(), comm_dev, sizeof(int) * ((size_t) nblk + 1), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int) e;
    if (out[(size_t) nblk] != 0) return -2;              // two-source column indices: not a matrix the planner partitions
    *total_size = 0;
    for (int b = 0; b < nblk; b++) { comm_sizes[b] = out[(size_t) b]; *total_size += out[(size_t) b]; }
    return 0;
}

// (4 and 6 were the round-1 LDS team kernel and the narrow team kernel of round 3: measured slower than what variant 0 picks,
//  removed in round 4; the numbers stay so that 5 and 7 keep their meaning)
static const char *k_variant_names[] = {"auto", "csr-rowgroup", "rowpanel-R4", "rowpanel-R8", "(removed)", "team2-R8", "(removed)", "team2r-R8"};
int crp_spmm_variant_count(void) { return (int) (sizeof(k_variant_names) / sizeof(k_variant_names[0])); }
// the variants a caller may name: fp64 all but the removed ones, fp32 the ones with an fp32 instance
static bool variant_valid(int variant, bool f32)
{
    if (f32) return variant == 0 || variant == 1 || variant == 5;
    return variant >= 0 && variant < crp_spmm_variant_count() && variant != 4 && variant != 6;
}
const char *crp_spmm_variant_name(int variant)
{
    if (variant < 0 || variant >= crp_spmm_variant_count()) return NULL;
    return k_variant_names[variant];
}

static int spmm_csr_f64(crp_csr_dev_p A, int layout, int n, const double *B0, long long ldB0, const double *B1,
                        long long ldB1, double *C, long long ldC, int variant, void *stream)
{
    if (A == NULL || n < 0) return -1;
    if (layout != CRP_LAYOUT_ROW_MAJOR && layout != CRP_LAYOUT_COL_MAJOR) return -1;
    if (!variant_valid(variant, false)) return -1;
    if (A->nrow == 0 || n == 0) return 0;
    if (C == NULL || (B0 == NULL && B1 == NULL && A->nnz > 0)) return -1;
    if (layout == CRP_LAYOUT_ROW_MAJOR && (ldC < n || (B0 && ldB0 < n) || (B1 && ldB1 < n))) return -4;
    if (layout == CRP_LAYOUT_COL_MAJOR && ldC < (A->rowmap ? A->c_nrow : A->nrow)) return -4;
    const hipStream_t s = (hipStream_t) stream;
    crp::SpmmArgs a;
    a.nrow = A->nrow; a.n = n;
    a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = A->val;
    a.B0 = B0; a.ldB0 = ldB0; a.B1 = B1; a.ldB1 = ldB1; a.C = C; a.ldC = ldC;
    a.rowmap = A->rowmap;
    if (layout == CRP_LAYOUT_COL_MAJOR) return (int) crp::spmm_cm_f64(a, s);
    const crp::Operand op = operand_of(n, B0, ldB0, B1, ldB1, C, ldC);
    int v = crp::resolve_f64(A->traits, op, variant, A->team2r_refused, crp::knobs());
    // the derived formats hold the rows in processing order: their C row map is chosen per launch, AFTER every fallback has
    // resolved (a re-ordered matrix that falls back to the CSR kernel writes through the caller's map)
    int *const fmt_map = A->rowmap_fmt ? A->rowmap_fmt.p : A->rowmap.p;
    if (v == 5)
    {
        a.rowmap = fmt_map;
        A->last_variant = 5;
        const int rc = ensure_team2(A, s);
        if (rc != 0) return rc;
        crp::Team2Args t;
        team2_args(A->team2, &t);
        return (int) crp::spmm_rm_f64_team2(t, a, s);
    }
    if (v == 7)
    {
        A->last_variant = 7;
        const int G = n <= 32 ? 4 : 2;
        const int rc = ensure_team2r(A, s, G);
        if (rc == -6 && variant == 0)
        {
            // the streams of this matrix would pass their 32-bit offsets: variant 0 goes on with the row-panel kernels, for good
            A->team2r_refused = true;
            v = crp::resolve_f64(A->traits, op, variant, true, crp::knobs());
        }
        else
        {
            if (rc != 0) return rc;
            a.rowmap = fmt_map;
            Team2RDev &d = A->team2r[G == 2 ? 1 : 0];
            crp::Team2NArgs t;
            t.G = d.G; t.nteam = d.nteam; t.ngrid = d.ngrid; t.tgrid = d.tgrid; t.tpanel = d.tpanel; t.tinfo = d.tinfo; t.trec = d.trec; t.tvoff = d.tvoff; t.tval = d.tval; t.tent = d.tent;
            if (d.rows_epoch != A->rowmap_epoch || d.rows_map != a.rowmap)      // the C rows of the panels, once per row map
            {
                CRP_TRY(crp::team2r_fill_rows(t, a, s));
                CRP_TRY(hipStreamSynchronize(s));       // complete on return: a product on another stream reads these rows
                d.rows_epoch = A->rowmap_epoch;
                d.rows_map = a.rowmap;
            }
            return (int) crp::spmm_rm_f64_team2r(t, a, s);
        }
    }
    A->last_variant = v;
    if (v == 1) return (int) crp::spmm_rm_f64_rowgroup(a, s);
    a.rowmap = fmt_map;
    const int rc = ensure_panel(A, v - 2, s);       // no-op unless an explicit variant asks for a new format
    if (rc != 0) return rc;
    const PanelDev &d = A->pan[v - 2];
    crp::PanelArgs p;
    memset(&p, 0, sizeof(p));
    p.R = d.R; p.npanel = d.npanel; p.pptr = d.pptr; p.porder = d.porder; p.norder = d.norder; p.psync = d.psync; p.pcol = d.pcol; p.pmask4 = d.pmask4; p.pval = d.pval;
    p.b0_rows = A->b0_rows; p.b1_rows = A->b1_rows;
    p.cmo = d.cmo; p.cbase = d.cbase; p.cval = d.cval;
    return (int) crp::spmm_rm_f64_panel(p, a, s);
}

// (the launcher that runs names its kernel instance in crp::t_last_kernel: kept on the handle, "" when nothing was launched)
int crp_spmm_csr_f64(crp_csr_dev_p A, int layout, int n, const double *B0, long long ldB0, const double *B1,
                     long long ldB1, double *C, long long ldC, int variant, void *stream)
{
    crp::t_last_kernel = "";
    const int rc = spmm_csr_f64(A, layout, n, B0, ldB0, B1, ldB1, C, ldC, variant, stream);
    if (A != NULL) A->last_kernel = crp::t_last_kernel;
    return rc;
}

// C[nrow x n] := A * B with values, B and C in fp32 (row-major only): the fp32 instance of the team kernel where it
// applies and pays (variant 0 / 5), the fp32 CSR row-group kernel otherwise (variant 1, any width and alignment)
static int spmm_csr_f32(crp_csr_dev_p A, int n, const float *B0, long long ldB0, const float *B1, long long ldB1, float *C,
                        long long ldC, int variant, void *stream)
{
    if (A == NULL || n < 0) return -1;
    if (!variant_valid(variant, true)) return -1;
    if (A->nrow == 0 || n == 0) return 0;
    if (C == NULL || (B0 == NULL && B1 == NULL && A->nnz > 0)) return -1;
    if (ldC < n || (B0 && ldB0 < n) || (B1 && ldB1 < n)) return -4;
    const hipStream_t s = (hipStream_t) stream;
    {
        const int rc = ensure_val32(A, s);
        if (rc != 0) return rc;
    }
    crp::SpmmArgsF32 a;
    a.nrow = A->nrow; a.n = n; a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = A->val32;
    a.B0 = B0; a.ldB0 = ldB0; a.B1 = B1; a.ldB1 = ldB1; a.C = C; a.ldC = ldC; a.rowmap = A->rowmap;
    A->last_variant = crp::resolve_f32(A->traits, operand_of(n, B0, ldB0, B1, ldB1, C, ldC), variant);
    if (A->last_variant == 1) return (int) crp::spmm_rm_f32_rowgroup(a, s);
    const int rc = ensure_team2(A, s, true);
    if (rc != 0) return rc;
    Team2Dev &d = A->team2;
    if (d.tval32 == nullptr)
    {
        DevBuf<float> v;
        CRP_TRY(v.alloc(sizeof(float) * ((size_t) d.value_entries + 1024)));
        CRP_TRY(hipMemsetAsync(v, 0, sizeof(float) * ((size_t) d.value_entries + 1024), s));
        CRP_TRY(crp::convert_f64_f32(d.value_entries, d.tval, v, s));
        CRP_TRY(hipStreamSynchronize(s));           // complete on return, for callers on other streams
        d.tval32 = std::move(v);
    }
    if (A->rowmap_fmt != nullptr) a.rowmap = A->rowmap_fmt;
    crp::Team2Args t;
    team2_args(d, &t);
    return (int) crp::spmm_rm_f32_team2(t, a, s);
}

int crp_spmm_csr_f32(crp_csr_dev_p A, int n, const float *B0, long long ldB0, const float *B1, long long ldB1, float *C,
                     long long ldC, int variant, void *stream)
{
    crp::t_last_kernel = "";
    const int rc = spmm_csr_f32(A, n, B0, ldB0, B1, ldB1, C, ldC, variant, stream);
    if (A != NULL) A->last_kernel = crp::t_last_kernel;
    return rc;
}

int crp_sddmm_csr_f64(crp_csr_dev_p A, int n, const double *X, long long ldX, const double *Y0, long long ldY0, const double *Y1,
                      long long ldY1, double *out, const int *out_pos, int mode, void *stream)
{
    const int rc = sddmm_check(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, mode);
    if (rc != 0 || A->nnz == 0) return rc;
    return sddmm_csr<double>(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, out_pos, mode, A->val, (hipStream_t) stream);
}

int crp_sddmm_csr_f32(crp_csr_dev_p A, int n, const float *X, long long ldX, const float *Y0, long long ldY0, const float *Y1,
                      long long ldY1, float *out, const int *out_pos, int mode, void *stream)
{
    const int rc = sddmm_check(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, mode);
    if (rc != 0 || A->nnz == 0) return rc;
    const hipStream_t s = (hipStream_t) stream;
    if (mode == 1)                                      // the fp32 copy of the values, as crp_spmm_csr_f32 derives it
    {
        const int rc1 = ensure_val32(A, s);
        if (rc1 != 0) return rc1;
    }
    return sddmm_csr<float>(A, n, X, ldX, Y0, ldY0, Y1, ldY1, out, out_pos, mode, A->val32, s);
}

// ---- fused sparse attention over A's pattern (attention_kernels.hip)
int crp_attention_csr_f64(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                          long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1,
                          long long ldV1, double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream)
{
    return attention_fwd_csr<double>(A, 1, false, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,
                                     (hipStream_t) stream);
}

int crp_attention_csr_f32(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                          long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1,
                          long long ldV1, float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream)
{
    return attention_fwd_csr<float>(A, 1, false, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,
                                    (hipStream_t) stream);
}

// ---- the fused backward of the sparse attention (attention_bwd_kernels.hip)
int crp_attention_bwd_q_csr_f64(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                                long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1,
                                long long ldV1, const double *O, long long ldO, const double *dO, long long lddO, const double *lse, double *dQ,
                                long long lddQ, double *delta, double *ds_out, const int *out_pos, void *stream)
{
    return attention_bwd_q_csr<double>(A, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                    delta, ds_out, out_pos, (hipStream_t) stream);
}

int crp_attention_bwd_kv_csr_f64(crp_csr_dev_p At, int nk, int nv, double scale, int bias, const double *K, long long ldK, const double *V,
                                 long long ldV, const double *Q, long long ldQ, const double *dO, long long lddO, const double *lse,
                                 const double *delta, double *dK, long long lddK, double *dV, long long lddV, void *stream)
{
    return attention_bwd_kv_csr<double>(At, nk, nv, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV,
                                     (hipStream_t) stream);
}

int crp_attention_bwd_q_csr_f32(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                                long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1,
                                long long ldV1, const float *O, long long ldO, const float *dO, long long lddO, const float *lse, float *dQ,
                                long long lddQ, float *delta, float *ds_out, const int *out_pos, void *stream)
{
    return attention_bwd_q_csr<float>(A, nk, nv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                    delta, ds_out, out_pos, (hipStream_t) stream);
}

int crp_attention_bwd_kv_csr_f32(crp_csr_dev_p At, int nk, int nv, double scale, int bias, const float *K, long long ldK, const float *V,
                                 long long ldV, const float *Q, long long ldQ, const float *dO, long long lddO, const float *lse,
                                 const float *delta, float *dK, long long lddK, float *dV, long long lddV, void *stream)
{
    return attention_bwd_kv_csr<float>(At, nk, nv, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV,
                                     (hipStream_t) stream);
}

// ---- ... with heads heads of dk / dv columns side by side in every operand (include/crpspmm_hip.h, "Multi-head"): head h's
// bits are the single-head call's on the column views of head h

int crp_attention_mh_csr_f64(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const double *Q, long long ldQ, const double *K0,
                             long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0, const double *V1, long long ldV1,
                             double *O, long long ldO, double *lse, double *p_out, const int *out_pos, void *stream)
{
    return attention_fwd_csr<double>(A, heads, true, dk, dv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,
                                     (hipStream_t) stream);
}

int crp_attention_mh_csr_f32(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                             long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1, long long ldV1,
                             float *O, long long ldO, float *lse, float *p_out, const int *out_pos, void *stream)
{
    return attention_fwd_csr<float>(A, heads, true, dk, dv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,
                                    (hipStream_t) stream);
}

int crp_attention_bwd_q_mh_csr_f64(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const double *Q, long long ldQ,
                                   const double *K0, long long ldK0, const double *K1, long long ldK1, const double *V0, long long ldV0,
                                   const double *V1, long long ldV1, const double *O, long long ldO, const double *dO, long long lddO,
                                   const double *lse, double *dQ, long long lddQ, double *delta, double *ds_out, const int *out_pos, void *stream)
{
    return attention_bwd_q_csr<double>(A, dk, dv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                    delta, ds_out, out_pos, (hipStream_t) stream, true, heads);
}

int crp_attention_bwd_kv_mh_csr_f64(crp_csr_dev_p At, int heads, int dk, int dv, double scale, int bias, const double *K, long long ldK,
                                    const double *V, long long ldV, const double *Q, long long ldQ, const double *dO, long long lddO,
                                    const double *lse, const double *delta, double *dK, long long lddK, double *dV, long long lddV, void *stream)
{
    return attention_bwd_kv_csr<double>(At, dk, dv, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV,
                                     (hipStream_t) stream, true, heads);
}

int crp_attention_bwd_q_mh_csr_f32(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const float *Q, long long ldQ, const float *K0,
                                   long long ldK0, const float *K1, long long ldK1, const float *V0, long long ldV0, const float *V1, long long ldV1,
                                   const float *O, long long ldO, const float *dO, long long lddO, const float *lse, float *dQ, long long lddQ,
                                   float *delta, float *ds_out, const int *out_pos, void *stream)
{
    return attention_bwd_q_csr<float>(A, dk, dv, scale, bias, Q, ldQ, K0, ldK0, K1, ldK1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, dQ, lddQ,
                                    delta, ds_out, out_pos, (hipStream_t) stream, true, heads);
}

int crp_attention_bwd_kv_mh_csr_f32(crp_csr_dev_p At, int heads, int dk, int dv, double scale, int bias, const float *K, long long ldK,
                                    const float *V, long long ldV, const float *Q, long long ldQ, const float *dO, long long lddO, const float *lse,
                                    const float *delta, float *dK, long long lddK, float *dV, long long lddV, void *stream)
{
    return attention_bwd_kv_csr<float>(At, dk, dv, scale, bias, K, ldK, V, ldV, Q, ldQ, dO, lddO, lse, delta, dK, lddK, dV, lddV,
                                     (hipStream_t) stream, true, heads);
}

// ---- the fused GAT attention: additive LeakyReLU scores, forward and the two-handle backward (gat_kernels.hip)
#define CRP_GAT_ENTRY_POINTS(SFX, T)                                                                                                              \
    int crp_gat_attention_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *el, long long ldel, const T *er0,        \
                                    long long lder0, const T *er1, long long lder1, const T *V0, long long ldV0, const T *V1, long long ldV1,     \
                                    T *O, long long ldO, T *lse, T *p_out, const int *out_pos, void *stream)                                      \
    {                                                                                                                                             \
        return gat_fwd_csr<T>(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,      \
                              (hipStream_t) stream);                                                                                              \
    }                                                                                                                                             \
    int crp_gat_attention_bwd_row_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *el, long long ldel,              \
                                            const T *er0, long long lder0, const T *er1, long long lder1, const T *V0, long long ldV0,            \
                                            const T *V1, long long ldV1, const T *O, long long ldO, const T *dO, long long lddO, const T *lse,    \
                                            T *d_el, long long ldd_el, T *delta, T *ds_out, const int *out_pos, void *stream)                     \
    {                                                                                                                                             \
        return gat_bwd_row_csr<T>(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, d_el,  \
                                  ldd_el, delta, ds_out, out_pos, (hipStream_t) stream);                                                          \
    }                                                                                                                                             \
    int crp_gat_attention_bwd_col_csr_##SFX(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const T *er, long long lder, const T *V, \
                                            long long ldV, const T *el, long long ldel, const T *dO, long long lddO, const T *lse,                \
                                            const T *delta, T *d_er, long long ldd_er, T *dV, long long lddV, void *stream)                       \
    {                                                                                                                                             \
        return gat_bwd_col_csr<T>(At, heads, dv, slope, bias, er, lder, V, ldV, el, ldel, dO, lddO, lse, delta, d_er, ldd_er, dV, lddV,           \
                                  (hipStream_t) stream);                                                                                          \
    }
CRP_GAT_ENTRY_POINTS(f64, double)
CRP_GAT_ENTRY_POINTS(f32, float)
#undef CRP_GAT_ENTRY_POINTS

// ---- the fused GATv2 attention: a LeakyReLU inside the dot with a, forward and the two-handle backward (gatv2_kernels.hip)
#define CRP_GATV2_ENTRY_POINTS(SFX, T)                                                                                                            \
    int crp_gatv2_attention_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT, const T *XS0,      \
                                      long long ldXS0, const T *XS1, long long ldXS1, const T *a, T *O, long long ldO, T *lse, T *p_out,          \
                                      const int *out_pos, void *stream)                                                                           \
    {                                                                                                                                             \
        return gatv2_fwd_csr<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, lse, p_out, out_pos,                      \
                                (hipStream_t) stream);                                                                                            \
    }                                                                                                                                             \
    int crp_gatv2_attention_bwd_row_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT,            \
                                              const T *XS0, long long ldXS0, const T *XS1, long long ldXS1, const T *a, const T *O,               \
                                              long long ldO, const T *dO, long long lddO, const T *lse, T *dXT, long long lddXT, T *da_part,      \
                                              long long ldda, T *delta, T *ds_out, const int *out_pos, void *stream)                              \
    {                                                                                                                                             \
        return gatv2_bwd_row_csr<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, dO, lddO, lse, dXT, lddXT, da_part,  \
                                    ldda, delta, ds_out, out_pos, (hipStream_t) stream);                                                          \
    }                                                                                                                                             \
    int crp_gatv2_attention_bwd_col_csr_##SFX(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const T *XS, long long ldXS,           \
                                              const T *XT, long long ldXT, const T *a, const T *dO, long long lddO, const T *lse,                 \
                                              const T *delta, T *dXS, long long lddXS, void *stream)                                              \
    {                                                                                                                                             \
        return gatv2_bwd_col_csr<T>(At, heads, dv, slope, bias, XS, ldXS, XT, ldXT, a, dO, lddO, lse, delta, dXS, lddXS, (hipStream_t) stream);  \
    }
CRP_GATV2_ENTRY_POINTS(f64, double)
CRP_GATV2_ENTRY_POINTS(f32, float)
#undef CRP_GATV2_ENTRY_POINTS

// ---- ... and both with attention dropout (dropout.h): the same argument lists with (drop, seed) before the stream;
// drop == 0 takes the instances of the calls above
#define CRP_GAT_DROP_ENTRY_POINTS(SFX, T)                                                                                                                                 \
    int crp_gat_attention_drop_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *el, long long ldel, const T *er0,                           \
                                    long long lder0, const T *er1, long long lder1, const T *V0, long long ldV0, const T *V1, long long ldV1,                             \
                                    T *O, long long ldO, T *lse, T *p_out, const int *out_pos, double drop, unsigned long long seed, void *stream)                        \
    {                                                                                                                                                                     \
        return gat_fwd_csr<T>(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, lse, p_out, out_pos,                               \
                              (hipStream_t) stream, drop, seed);                                                                                                          \
    }                                                                                                                                                                     \
    int crp_gat_attention_drop_bwd_row_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *el, long long ldel,                                 \
                                            const T *er0, long long lder0, const T *er1, long long lder1, const T *V0, long long ldV0,                                    \
                                            const T *V1, long long ldV1, const T *O, long long ldO, const T *dO, long long lddO, const T *lse,                            \
                                            T *d_el, long long ldd_el, T *delta, T *ds_out, const int *out_pos, double drop, unsigned long long seed, void *stream)       \
    {                                                                                                                                                                     \
        return gat_bwd_row_csr<T>(A, heads, dv, slope, bias, el, ldel, er0, lder0, er1, lder1, V0, ldV0, V1, ldV1, O, ldO, dO, lddO, lse, d_el,                           \
                                  ldd_el, delta, ds_out, out_pos, (hipStream_t) stream, drop, seed);                                                                      \
    }                                                                                                                                                                     \
    int crp_gat_attention_drop_bwd_col_csr_##SFX(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const T *er, long long lder, const T *V,                    \
                                            long long ldV, const T *el, long long ldel, const T *dO, long long lddO, const T *lse,                                        \
                                            const T *delta, T *d_er, long long ldd_er, T *dV, long long lddV, double drop, unsigned long long seed, void *stream)         \
    {                                                                                                                                                                     \
        return gat_bwd_col_csr<T>(At, heads, dv, slope, bias, er, lder, V, ldV, el, ldel, dO, lddO, lse, delta, d_er, ldd_er, dV, lddV,                                   \
                                  (hipStream_t) stream, drop, seed);                                                                                                      \
    }
CRP_GAT_DROP_ENTRY_POINTS(f64, double)
CRP_GAT_DROP_ENTRY_POINTS(f32, float)
#undef CRP_GAT_DROP_ENTRY_POINTS

#define CRP_GATV2_DROP_ENTRY_POINTS(SFX, T)                                                                                                                               \
    int crp_gatv2_attention_drop_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT, const T *XS0,                         \
                                      long long ldXS0, const T *XS1, long long ldXS1, const T *a, T *O, long long ldO, T *lse, T *p_out,                                  \
                                      const int *out_pos, double drop, unsigned long long seed, void *stream)                                                             \
    {                                                                                                                                                                     \
        return gatv2_fwd_csr<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, lse, p_out, out_pos,                                              \
                                (hipStream_t) stream, drop, seed);                                                                                                        \
    }                                                                                                                                                                     \
    int crp_gatv2_attention_drop_bwd_row_csr_##SFX(crp_csr_dev_p A, int heads, int dv, double slope, int bias, const T *XT, long long ldXT,                               \
                                              const T *XS0, long long ldXS0, const T *XS1, long long ldXS1, const T *a, const T *O,                                       \
                                              long long ldO, const T *dO, long long lddO, const T *lse, T *dXT, long long lddXT, T *da_part,                              \
                                              long long ldda, T *delta, T *ds_out, const int *out_pos, double drop, unsigned long long seed, void *stream)                \
    {                                                                                                                                                                     \
        return gatv2_bwd_row_csr<T>(A, heads, dv, slope, bias, XT, ldXT, XS0, ldXS0, XS1, ldXS1, a, O, ldO, dO, lddO, lse, dXT, lddXT, da_part,                           \
                                    ldda, delta, ds_out, out_pos, (hipStream_t) stream, drop, seed);                                                                      \
    }                                                                                                                                                                     \
    int crp_gatv2_attention_drop_bwd_col_csr_##SFX(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const T *XS, long long ldXS,                              \
                                              const T *XT, long long ldXT, const T *a, const T *dO, long long lddO, const T *lse,                                         \
                                              const T *delta, T *dXS, long long lddXS, double drop, unsigned long long seed, void *stream)                                \
    {                                                                                                                                                                     \
        return gatv2_bwd_col_csr<T>(At, heads, dv, slope, bias, XS, ldXS, XT, ldXT, a, dO, lddO, lse, delta, dXS, lddXS, (hipStream_t) stream, drop, seed);               \
    }
CRP_GATV2_DROP_ENTRY_POINTS(f64, double)
CRP_GATV2_DROP_ENTRY_POINTS(f32, float)
#undef CRP_GATV2_DROP_ENTRY_POINTS

// ---- the dropout mask on its own (dropout.h): one draw on the host, and the (nnz, heads) keep flags of a handle
int crp_dropout_keep_host(unsigned long long seed, unsigned r, unsigned c, unsigned h, double drop)
{
    if (!drop_rate_ok(drop)) return -1;
    return crp::dropout_keep((uint32_t) seed, (uint32_t) (seed >> 32), r, c, h, crp::dropout_threshold(drop)) ? 1 : 0;
}

int crp_dropout_mask_csr(crp_csr_dev_p A, int heads, double drop, unsigned long long seed, unsigned char *mask, const int *out_pos,
                         void *stream)
{
    if (A == NULL || heads < 1 || !drop_rate_ok(drop)) return -1;
    if (A->nnz == 0 || A->nrow == 0) return 0;
    if (mask == NULL) return -1;
    return (int) crp::dropout_mask_csr(A->nrow, heads, A->rowptr, A->colidx, A->rowmap, (bool) A->tmap, drop, seed, mask, out_pos,
                                       (hipStream_t) stream);
}

// ---- row softmax over a CSR pattern (softmax_kernels.hip).  Every argument is checked before anything is launched.
int crp_row_softmax_f64(int nrow, const int *rowptr, const double *s, double *y, void *stream)
{
    if (nrow < 0) return -1;
    if (nrow == 0) return 0;
    if (rowptr == NULL || s == NULL || y == NULL) return -1;
    return (int) crp::row_softmax_f64(nrow, rowptr, s, y, (hipStream_t) stream);
}

int crp_row_softmax_f32(int nrow, const int *rowptr, const float *s, float *y, void *stream)
{
    if (nrow < 0) return -1;
    if (nrow == 0) return 0;
    if (rowptr == NULL || s == NULL || y == NULL) return -1;
    return (int) crp::row_softmax_f32(nrow, rowptr, s, y, (hipStream_t) stream);
}

int crp_row_softmax_bwd_f64(int nrow, const int *rowptr, const double *y, const double *dy, double *ds, void *stream)
{
    if (nrow < 0) return -1;
    if (nrow == 0) return 0;
    if (rowptr == NULL || y == NULL || dy == NULL || ds == NULL) return -1;
    return (int) crp::row_softmax_bwd_f64(nrow, rowptr, y, dy, ds, (hipStream_t) stream);
}

int crp_row_softmax_bwd_f32(int nrow, const int *rowptr, const float *y, const float *dy, float *ds, void *stream)
{
    if (nrow < 0) return -1;
    if (nrow == 0) return 0;
    if (rowptr == NULL || y == NULL || dy == NULL || ds == NULL) return -1;
    return (int) crp::row_softmax_bwd_f32(nrow, rowptr, y, dy, ds, (hipStream_t) stream);
}

// the handle forms: the handle's own device row pointer (its CSR order, as crp_sddmm_csr_*)
int crp_csr_dev_row_softmax_f64(crp_csr_dev_p A, const double *s, double *y, void *stream)
{
    if (A == NULL) return -1;
    return crp_row_softmax_f64(A->nrow, A->rowptr, s, y, stream);
}

int crp_csr_dev_row_softmax_f32(crp_csr_dev_p A, const float *s, float *y, void *stream)
{
    if (A == NULL) return -1;
    return crp_row_softmax_f32(A->nrow, A->rowptr, s, y, stream);
}

int crp_csr_dev_row_softmax_bwd_f64(crp_csr_dev_p A, const double *y, const double *dy, double *ds, void *stream)
{
    if (A == NULL) return -1;
    return crp_row_softmax_bwd_f64(A->nrow, A->rowptr, y, dy, ds, stream);
}

int crp_csr_dev_row_softmax_bwd_f32(crp_csr_dev_p A, const float *y, const float *dy, float *ds, void *stream)
{
    if (A == NULL) return -1;
    return crp_row_softmax_bwd_f32(A->nrow, A->rowptr, y, dy, ds, stream);
}

int crp_csr_dev_auto_variant(crp_csr_dev_p A) { return A ? A->traits.auto_variant : -1; }
int crp_csr_dev_reordered(crp_csr_dev_p A) { return A ? (A->ord.perm.empty() ? 0 : 1) : -1; }
int crp_csr_dev_resolved_variant(crp_csr_dev_p A, int n)      // (an aligned operand of ld = n without B1)
{
    return A ? crp::resolve_f64(A->traits, operand_of(n, nullptr, n, nullptr, 0, nullptr, n), 0, A->team2r_refused, crp::knobs()) : -1;
}
int crp_csr_dev_last_variant(crp_csr_dev_p A) { return A ? A->last_variant : -1; }
const char *crp_csr_dev_last_kernel(crp_csr_dev_p A) { return A ? A->last_kernel : NULL; }
int crp_csr_dev_lattice(crp_csr_dev_p A) { return A ? ((A->team2.built && A->team2.lattice) ? 1 : 0) : -1; }
int crp_csr_dev_team2_compact(crp_csr_dev_p A) { return (A && A->team2.built) ? (A->team2.compact ? 1 : 0) : -1; }

int crp_panel_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int R, int *npanel,
                          int **pptr, int **pcol, unsigned **pmask4, double **pval, long long *real_entries,
                          int **porder, int *norder)
{
    if (nrow < 0 || rowptr == NULL || (R != 4 && R != 8) || !npanel || !pptr || !pcol || !pmask4 || !pval) return -1;
    crp::PanelHost h;
    crp::build_panels(nrow, rowptr, colidx, val, R, &h);
    *npanel = h.npanel;
    *pptr = dup(h.pptr);
    *pcol = dup(h.pcol);
    *pmask4 = dup(h.pmask4);
    *pval = dup(h.pval);
    if (real_entries) *real_entries = h.real_entries;
    if (norder) *norder = (int) h.porder.size();
    if (porder) *porder = dup(h.porder);
    return 0;
}

int crp_team_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int *nteam, int *lattice,
                         int **tpanel, int **tptr, int **tcol, unsigned **tmask, int **torder)
{
    if (nrow < 0 || rowptr == NULL || !nteam || !tpanel || !tptr || !tcol || !tmask || !torder) return -1;
    crp::PanelHost h;
    crp::build_panels(nrow, rowptr, colidx, val, 8, &h, false);
    crp::TeamHost th;
    crp::build_teams(h, nrow, rowptr, colidx, &th);
    *nteam = th.nteam;
    if (lattice) *lattice = th.lattice ? 1 : 0;
    *tpanel = dup(th.tpanel);
    *tptr = dup(th.tptr);
    *tcol = dup(th.tcol);
    *torder = dup(th.torder);
    *tmask = dup(th.tmask);
    return 0;
}

static std::vector<int> g_last_tgrid;       // launch grid of the last crp_team2_format_host() (planning / test helper)
static int g_last_compact = 1;              // ... and whether its value blocks are compact
int crp_team2_format_host_compact(void) { return g_last_compact; }
int crp_team2_format_host_grid(int **tgrid, int *ngrid)
{
    if (tgrid == NULL || ngrid == NULL) return -1;
    *ngrid = (int) g_last_tgrid.size();
    *tgrid = dup(g_last_tgrid);
    return 0;
}

int crp_team2r_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int G, int *nteam, int *lattice, int **tpanel,
                           int **tinfo, unsigned **trec, long long *nrecwords, long long **tvoff, double **tval, long long *nwords,
                           int **tgrid, int *ngrid, unsigned **vmap, long long *stats, unsigned **tent)
{
    if (nrow < 0 || rowptr == NULL || (G != 2 && G != 4) || !nteam || !tpanel || !tinfo || !trec || !nrecwords || !tvoff || !tval || !nwords || !tgrid || !ngrid)
        return -1;
    crp::PanelHost h;
    crp::build_panels(nrow, rowptr, colidx, val, 8, &h, false, false);
    crp::Team2RHost th;
    th.G = G;
    if (!crp::build_team2r(h, nrow, rowptr, colidx, &th)) return -6;
    *nteam = th.nteam;
    if (lattice) *lattice = th.lattice ? 1 : 0;
    *tpanel = dup(th.tpanel);
    *tinfo = dup(th.tinfo);
    *tgrid = dup(th.tgrid);
    *ngrid = (int) th.tgrid.size();
    *trec = dup(th.trec);
    *nrecwords = (long long) th.trec.size();
    *tvoff = dup(th.tvoff);
    *tval = dup(th.tval);
    *nwords = th.nwords;
    if (vmap) *vmap = dup(th.vmap);
    if (stats) { stats[0] = th.rounds; stats[1] = th.steps; stats[2] = th.slots_filled; stats[3] = th.nnz; }
    if (tent) *tent = dup(th.tent);
    return 0;
}

int crp_team2_format_host(int nrow, const int *rowptr, const int *colidx, const double *val, int *nteam, int *lattice,
                          int **tpanel, int **tinfo, int **tpro, unsigned **trec, long long *nrecwords,
                          long long **tvoff, double **tval, long long *nvalent, int **torder, unsigned **vmap)
{
    if (nrow < 0 || rowptr == NULL || !nteam || !tpanel || !tinfo || !tpro || !trec || !nrecwords || !tvoff || !tval ||
        !nvalent || !torder)
        return -1;
    crp::PhaseClock clk;
    crp::PanelHost h;
    crp::build_panels(nrow, rowptr, colidx, val, 8, &h, false, false);
    clk.lap("crp_team2_format_host: build_panels (R = 8)");
    crp::Team2Host th;
    th.compact = crp::team2_compact(h.fill(), false);      // (the product's fp64 default)
    crp::build_team2(h, nrow, rowptr, colidx, &th);
    g_last_compact = th.compact ? 1 : 0;
    clk.lap("crp_team2_format_host: build_team2");
    g_last_tgrid = th.tgrid;
    *nteam = th.nteam;
    if (lattice) *lattice = th.lattice ? 1 : 0;
    *tpanel = dup(th.tpanel);
    *tinfo = dup(th.tinfo);
    *tpro = dup(th.tpro);
    *torder = dup(th.torder);
    *trec = dup(th.trec);
    *nrecwords = (long long) th.trec.size();
    *tvoff = dup(th.tvoff);
    *nvalent = th.nvalues;
    *tval = (double *) calloc(th.tval.size() + 1, sizeof(double));
    if (!th.tval.empty()) memcpy(*tval, th.tval.data(), sizeof(double) * th.tval.size());
    if (vmap) *vmap = dup(th.vmap);
    return 0;
}

int crp_locality_order_host(int nrow, int ncol, const int *rowptr, const int *colidx, int nparts, int *perm, double *info)
{
    if (nrow < 0 || rowptr == NULL || perm == NULL || nparts < 1) return -1;
    std::vector<int> pv;
    crp::LocalityInfo li;
    const bool ok = crp::locality_reorder(nrow, ncol, rowptr, colidx, nparts, &pv, &li);
    if (!ok)
    {
        for (int i = 0; i < nrow; i++) perm[i] = i;
        return 1;
    }
    memcpy(perm, pv.data(), sizeof(int) * (size_t) nrow);
    if (info) { info[0] = li.groups; info[1] = li.parts; info[2] = li.mean_dist_before; info[3] = li.mean_dist_after; }
    return 0;
}

int crp_spmm_plan_host(int nrow, int ncol, const int *rowptr, const int *colidx, int nwidth, const int *widths, int variant, int f32,
                       int shape, int *resolved, int *info)
{
    if (nrow < 0 || rowptr == NULL || (rowptr[nrow] > 0 && colidx == NULL) || nwidth < 0 || (nwidth > 0 && (widths == NULL || resolved == NULL)))
        return -1;
    if (shape < 0 || shape > 3) return -1;
    if (!variant_valid(variant, f32 != 0)) return -1;
    // the same order and traits as crp_csr_dev_create, the same rules as crp_spmm_csr_f64 / _f32 (no refused row-owner streams)
    const bool two_source = std::any_of(colidx, colidx + rowptr[nrow], [](int c) { return c < 0; });
    const crp::FormatOrder ord = crp::format_order(nrow, ncol, rowptr, colidx, two_source);
    const bool re = !ord.perm.empty();
    const crp::MatrixTraits t = crp::matrix_traits(nrow, re ? ord.f_rowptr.data() : rowptr, re ? ord.f_colidx.data() : colidx);
    if (info)
    {
        info[0] = t.auto_variant; info[1] = re ? 1 : 0; info[2] = t.team2_min_n; info[3] = t.team2_pays ? 1 : 0; info[4] = t.panels_sparse ? 1 : 0;
    }
    for (int i = 0; i < nwidth; i++)
    {
        // operand shapes: 0 aligned (ld = n), 1 ld = n + 1, 2 with B1, 3 B0 8-byte aligned
        const int n = widths[i];
        const long long ld = shape == 1 ? n + 1 : n;
        const uintptr_t b0 = shape == 3 ? 8 : 16;
        const crp::Operand op = operand_of(n, (const void *) b0, ld, shape == 2 ? (const void *) 16 : nullptr, ld, (const void *) 16, ld);
        resolved[i] = f32 ? crp::resolve_f32(t, op, variant) : crp::resolve_f64(t, op, variant, false, crp::knobs());
    }
    return 0;
}

int crp_gather_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, long long lds,
                        double *dst, long long ldd, void *stream)
{
    if (nidx < 0 || n < 0 || (layout != 0 && layout != 1)) return -1;
    return (int) crp::gather_rows_f64(layout, nidx, n, ridx, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_scatter_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, long long lds,
                         double *dst, long long ldd, void *stream)
{
    if (nidx < 0 || n < 0 || (layout != 0 && layout != 1)) return -1;
    return (int) crp::scatter_rows_f64(layout, nidx, n, ridx, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_scatter_add_rows_f64(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const double *src,
                             long long lds, double *dst, long long ldd, void *stream)
{
    if (nseg < 0 || n < 0) return -1;
    if (nseg > 0 && n > 0 && (seg_row == NULL || seg_ptr == NULL || seg_pos == NULL || src == NULL || dst == NULL)) return -1;
    return (int) crp::scatter_add_rows_f64(nseg, n, seg_row, seg_ptr, seg_pos, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_scatter_add_rows_f32(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const float *src,
                             long long lds, float *dst, long long ldd, void *stream)
{
    if (nseg < 0 || n < 0) return -1;
    if (nseg > 0 && n > 0 && (seg_row == NULL || seg_ptr == NULL || seg_pos == NULL || src == NULL || dst == NULL)) return -1;
    return (int) crp::scatter_add_rows_f32(nseg, n, seg_row, seg_ptr, seg_pos, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_gather_vals_f64(long long n, const int *map, const double *src, double *dst, void *stream)
{
    if (n < 0 || (n > 0 && (src == NULL || dst == NULL))) return -1;
    return (int) crp::gather_vals_f64(n, map, src, dst, (hipStream_t) stream);
}

int crp_gather_vals_f32_f64(long long n, const int *map, const float *src, double *dst, void *stream)
{
    if (n < 0 || (n > 0 && (src == NULL || dst == NULL))) return -1;
    return (int) crp::gather_vals_f32_f64(n, map, src, dst, (hipStream_t) stream);
}

int crp_sum_segments_f64(int nseg, long long len, const double *src, long long seg_stride, double *out, void *stream)
{
    if (src == NULL || out == NULL || nseg < 1 || len < 0) return -1;
    if (nseg > 1 && seg_stride < len) return -4;
    if (len == 0) return 0;
    return (int) crp::sum_segments_f64(nseg, len, src, seg_stride, out, (hipStream_t) stream);
}

int crp_sum_segments_f32(int nseg, long long len, const float *src, long long seg_stride, float *out, void *stream)
{
    if (src == NULL || out == NULL || nseg < 1 || len < 0) return -1;
    if (nseg > 1 && seg_stride < len) return -4;
    if (len == 0) return 0;
    return (int) crp::sum_segments_f32(nseg, len, src, seg_stride, out, (hipStream_t) stream);
}

int crp_col_sum_f64(int nrow, int n, const double *src, long long lds, double *work, double *out, void *stream)
{
    if (nrow < 0 || n < 0 || out == NULL || (nrow > 0 && n > 0 && (src == NULL || work == NULL))) return -1;
    if (nrow > 0 && lds < n) return -4;
    return (int) crp::col_sum_f64(nrow, n, src, lds, work, out, (hipStream_t) stream);
}

int crp_col_sum_f32(int nrow, int n, const float *src, long long lds, float *work, float *out, void *stream)
{
    if (nrow < 0 || n < 0 || out == NULL || (nrow > 0 && n > 0 && (src == NULL || work == NULL))) return -1;
    if (nrow > 0 && lds < n) return -4;
    return (int) crp::col_sum_f32(nrow, n, src, lds, work, out, (hipStream_t) stream);
}

int crp_transpose_f64(int nrow, int ncol, const double *src, long long lds, double *dst, long long ldd,
                      void *stream)
{
    if (nrow < 0 || ncol < 0) return -1;
    return (int) crp::transpose_f64(nrow, ncol, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_gather_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, long long lds,
                        float *dst, long long ldd, void *stream)
{
    if (nidx < 0 || n < 0 || (layout != 0 && layout != 1)) return -1;
    return (int) crp::gather_rows_f32(layout, nidx, n, ridx, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_scatter_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, long long lds,
                         float *dst, long long ldd, void *stream)
{
    if (nidx < 0 || n < 0 || (layout != 0 && layout != 1)) return -1;
    return (int) crp::scatter_rows_f32(layout, nidx, n, ridx, src, lds, dst, ldd, (hipStream_t) stream);
}

int crp_transpose_f32(int nrow, int ncol, const float *src, long long lds, float *dst, long long ldd,
                      void *stream)
{
    if (nrow < 0 || ncol < 0) return -1;
    return (int) crp::transpose_f32(nrow, ncol, src, lds, dst, ldd, (hipStream_t) stream);
}

}  // extern "C"

