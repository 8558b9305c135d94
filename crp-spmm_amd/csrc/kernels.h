// kernels.h -- internal launch interfaces between the C ABI (hip_api.hip) and
// the gfx950 kernels.  Not installed; the public surface is include/*.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "dropout.h"

namespace crp {

struct SpmmArgs
{
    int nrow;
    int n;
    const int    *rowptr;
    const int    *colidx;
    const double *val;
    const double *B0;
    int64_t       ldB0;
    const double *B1;
    int64_t       ldB1;
    double       *C;
    int64_t       ldC;
    const int    *rowmap;   // nullptr, or the C row of every row (row-subset matrices)
};

struct SpmmArgsF32          // the fp32 path (values, B and C in fp32; BASELINE configs[3])
{
    int nrow;
    int n;
    const int   *rowptr;
    const int   *colidx;
    const float *val;
    const float *B0;
    int64_t      ldB0;
    const float *B1;
    int64_t      ldB1;
    float       *C;
    int64_t      ldC;
    const int   *rowmap;
};

struct PanelArgs
{
    int R;
    int npanel;
    const int      *pptr;
    const int      *porder;    // processing order: norder records {panel or -1, first entry, rounds, 0}
    int             norder;
    const int      *psync;     // per workgroup (4 positions): rounds that start at a barrier, or nullptr
    const int      *pcol;
    const uint32_t *pmask4;
    const double   *pval;
    long long       b0_rows;   // rows of B0 / B1 the column indices can address (for the 4 GiB check)
    long long       b1_rows;
    // compact values (PanelHost::cmo / cbase / cval), or nullptr: the narrow-operand kernel reads them instead of pmask4 / pval
    const uint32_t *cmo;
    const long long *cbase;
    const double   *cval;
};

struct Team2Args          // panel_format.h, Team2Host
{
    int nteam;
    int ngrid;                 // entries of torder: the launch grid (Team2Host::tgrid), a multiple of 8
    bool compact;              // value blocks hold only the values that exist (Team2Host::compact); false: 8 per part
    const int      *torder;
    const int      *tpanel;    // 8 * nteam
    const int      *tinfo;     // 4 * nteam: rounds, first record block, union entries, 0
    const int      *tpro;      // nteam * TEAM2_D * 8 * 2: {column, value offset}
    const uint32_t *trec;      // record blocks (1 KiB each)
    const long long *tvoff;    // 8 * nteam
    const double   *tval;
    const float    *tval32;    // the same value groups in fp32 (fp32 path), or nullptr
};

struct Team2NArgs         // panel_format.h, Team2RHost (the row-owner team kernel, variant 7)
{
    int G;                     // entries per instruction: 4 (n <= 32) or 2 (n <= 64)
    int nteam;
    int ngrid;                 // entries of tgrid, a multiple of 8
    const int      *tgrid;
    const int      *tpanel;    // 8 * nteam
    const int      *tinfo;     // 2 * nteam: rounds, first record (in rounds)
    const uint32_t *trec;      // 128 words per round
    const long long *tvoff;    // 8 * nteam
    const double   *tval;
    uint32_t       *tent;      // the entry table (Team2RHost::tent)
};

template <typename T> struct SddmmArgs     // sddmm_kernels.hip: out[p] = < X[row(p)], Y[col(p)] > over the CSR pattern
{
    int nrow;
    int n;
    const int *rowptr;
    const int *colidx;
    const T   *val;         // the values in T (mode 1), else unused
    const T   *X;
    int64_t    ldX;
    const T   *Y0;
    int64_t    ldY0;
    const T   *Y1;
    int64_t    ldY1;
    T         *out;
    const int *rowmap;      // nullptr, or the X row of every row (row-subset matrices)
    const int *out_pos;     // nullptr, or where nonzero p writes: out[out_pos[p]]
    int        mode;        // 0: the dot, 1: the dot times val[p]
};

template <typename T> struct AttnArgs      // attention_kernels.hip: O[i] = sum_p softmax_p(scale <Q[i], K[c_p]> (+ val[p])) V[c_p]
{
    int nrow;
    int nk;                 // columns of Q and K
    int nv;                 // columns of V and O
    const int *rowptr;
    const int *colidx;
    const T   *val;         // the values in T (bias), or nullptr
    T          scale;
    const T   *Q;
    int64_t    ldQ;
    const T   *K0;
    int64_t    ldK0;
    const T   *K1;
    int64_t    ldK1;
    const T   *V0;
    int64_t    ldV0;
    const T   *V1;
    int64_t    ldV1;
    T         *O;
    int64_t    ldO;
    T         *lse;         // nullptr, or one entry per row (indexed like the rows of O)
    T         *p_out;       // nullptr, or the probabilities per nonzero
    const int *rowmap;      // nullptr, or the Q / O row of every row (row-subset matrices)
    const int *out_pos;     // nullptr, or where nonzero p writes: p_out[out_pos[p]]
    int heads = 1;          // read by the multi-head instances only (attention_rm, mh): nk and nv are then one head's widths
};

// attention_bwd_kernels.hip, row side: dQ[i] = scale sum_p dS_p K[c_p], delta[i] = <dO[i], O[i]>, ds_out[p] = dS_p over A's rows
template <typename T> struct AttnBwdQArgs
{
    int nrow;
    int nk;                 // columns of Q, K and dQ
    int nv;                 // columns of V, O and dO
    const int *rowptr;
    const int *colidx;
    const T   *val;         // the values in T (bias), or nullptr
    T          scale;
    const T   *Q;
    int64_t    ldQ;
    const T   *K0;
    int64_t    ldK0;
    const T   *K1;
    int64_t    ldK1;
    const T   *V0;
    int64_t    ldV0;
    const T   *V1;
    int64_t    ldV1;
    const T   *O;
    int64_t    ldO;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;         // one entry per row, as the forward wrote it (indexed like the rows of O)
    T         *dQ;
    int64_t    lddQ;
    T         *delta;       // one entry per row, indexed like lse
    T         *ds_out;      // nullptr, or dS per nonzero
    const int *rowmap;      // nullptr, or the Q / O / dO / dQ / lse / delta row of every row (row-subset matrices)
    const int *out_pos;     // nullptr, or where nonzero p writes: ds_out[out_pos[p]]
    int heads = 1;          // read by the multi-head instances only (attention_bwd_q, mh)
};

// attention_bwd_kernels.hip, column side, over a handle of A^T (row c = column c of A, entries = the rows i of A that hold c):
// dK[c] = scale sum_p dS_p Q[i_p], dV[c] = sum_p p_p dO[i_p]
template <typename T> struct AttnBwdKVArgs
{
    int nrow;               // rows of the transposed handle
    int nk;
    int nv;
    const int *rowptr;
    const int *colidx;      // rows of Q / dO / lse / delta (one source: no negative code)
    const T   *val;         // the transposed handle's values in T (bias), or nullptr
    T          scale;
    const T   *K;
    int64_t    ldK;
    const T   *V;
    int64_t    ldV;
    const T   *Q;
    int64_t    ldQ;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;
    const T   *delta;
    T         *dK;          // may be K exactly (a group reads its row whole before it writes it)
    int64_t    lddK;
    T         *dV;          // may be V exactly
    int64_t    lddV;
    const int *rowmap;      // nullptr, or the K / V / dK / dV row of every row (row-subset matrices)
    int heads = 1;          // read by the multi-head instances only (attention_bwd_kv, mh)
};

// gat_kernels.hip: O[i]_h = sum_p softmax_p(lrelu(el[i][h] + er[c_p][h]) (+ val[p])) V[c_p]_h over (row, head) units
template <typename T> struct GatArgs
{
    int nrow;
    int nv;                 // columns of one head of V and O
    int heads;
    const int *rowptr;
    const int *colidx;
    const T   *val;         // the values in T (bias), or nullptr
    T          slope;
    const T   *el;          // (rows of O, heads)
    int64_t    ldel;
    const T   *er0;         // the two sources of the column code, (rows of V0 / V1, heads)
    int64_t    lder0;
    const T   *er1;
    int64_t    lder1;
    const T   *V0;
    int64_t    ldV0;
    const T   *V1;
    int64_t    ldV1;
    T         *O;
    int64_t    ldO;
    T         *lse;         // nullptr, or (rows, heads), indexed like the rows of O
    T         *p_out;       // nullptr, or the probabilities, (nnz, heads)
    const int *rowmap;      // nullptr, or the el / O row of every row (row-subset matrices)
    const int *out_pos;     // nullptr, or where nonzero p writes: row out_pos[p] of p_out
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// gat_kernels.hip, row side of the backward over a handle of A: delta = <dO[i]_h, O[i]_h>, d_el = sum_p dZ_p, ds_out = dS_p
template <typename T> struct GatBwdRowArgs
{
    int nrow;
    int nv;
    int heads;
    const int *rowptr;
    const int *colidx;
    const T   *val;
    T          slope;
    const T   *el;
    int64_t    ldel;
    const T   *er0;
    int64_t    lder0;
    const T   *er1;
    int64_t    lder1;
    const T   *V0;
    int64_t    ldV0;
    const T   *V1;
    int64_t    ldV1;
    const T   *O;
    int64_t    ldO;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;         // (rows, heads), as the forward wrote it
    T         *d_el;        // (rows, heads), indexed like el
    int64_t    ldd_el;
    T         *delta;       // (rows, heads), indexed like lse
    T         *ds_out;      // nullptr, or dS, (nnz, heads)
    const int *rowmap;      // nullptr, or the el / O / dO / d_el / lse / delta row of every row
    const int *out_pos;     // nullptr, or where nonzero p writes: row out_pos[p] of ds_out
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// gat_kernels.hip, column side over a handle of A^T (row c = column c of A): d_er[c][h] = sum_p dZ_p, dV[c]_h = sum_p p_p dO[i_p]_h
template <typename T> struct GatBwdColArgs
{
    int nrow;               // rows of the transposed handle
    int nv;
    int heads;
    const int *rowptr;
    const int *colidx;      // rows of el / dO / lse / delta (one source: no negative code)
    const T   *val;         // the transposed handle's values in T (bias), or nullptr
    T          slope;
    const T   *er;
    int64_t    lder;
    const T   *V;
    int64_t    ldV;
    const T   *el;
    int64_t    ldel;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;
    const T   *delta;
    T         *d_er;
    int64_t    ldd_er;
    T         *dV;          // may be V exactly (a group reads its slice whole before it writes it)
    int64_t    lddV;
    const int *rowmap;      // nullptr, or the er / V / d_er / dV row of every row (row-subset matrices)
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// gatv2_kernels.hip: O[i]_h = sum_p softmax_p(sum_j a[h][j] lrelu(XT[i]_h[j] + XS[c_p]_h[j]) (+ val[p])) XS[c_p]_h over (row, head) units
template <typename T> struct Gatv2Args
{
    int nrow;
    int nv;                 // columns of one head of XT, XS, a and O
    int heads;
    const int *rowptr;
    const int *colidx;
    const T   *val;         // the values in T (bias), or nullptr
    T          slope;
    const T   *XT;          // (rows of O, heads * nv)
    int64_t    ldXT;
    const T   *XS0;         // the two sources of the column code
    int64_t    ldXS0;
    const T   *XS1;
    int64_t    ldXS1;
    const T   *av;          // heads * nv contiguous elements
    T         *O;
    int64_t    ldO;
    T         *lse;         // nullptr, or (rows, heads), indexed like the rows of O
    T         *p_out;       // nullptr, or the probabilities, (nnz, heads)
    const int *rowmap;      // nullptr, or the XT / O row of every row (row-subset matrices)
    const int *out_pos;     // nullptr, or where nonzero p writes: row out_pos[p] of p_out
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// gatv2_kernels.hip, row side of the backward over a handle of A: delta, dXT, da_part (the row's share of d/da), ds_out
template <typename T> struct Gatv2BwdRowArgs
{
    int nrow;
    int nv;
    int heads;
    const int *rowptr;
    const int *colidx;
    const T   *val;
    T          slope;
    const T   *XT;
    int64_t    ldXT;
    const T   *XS0;
    int64_t    ldXS0;
    const T   *XS1;
    int64_t    ldXS1;
    const T   *av;
    const T   *O;
    int64_t    ldO;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;         // (rows, heads), as the forward wrote it
    T         *dXT;         // (rows, heads * nv), indexed like XT
    int64_t    lddXT;
    T         *da_part;     // (rows, heads * nv), indexed like XT
    int64_t    ldda;
    T         *delta;       // (rows, heads), indexed like lse
    T         *ds_out;      // nullptr, or dS, (nnz, heads)
    const int *rowmap;      // nullptr, or the XT / O / dO / dXT / da_part / lse / delta row of every row
    const int *out_pos;     // nullptr, or where nonzero p writes: row out_pos[p] of ds_out
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// gatv2_kernels.hip, column side over a handle of A^T (row c = column c of A): dXS[c]_h = sum_p dS_p ag_p + sum_p p_p dO[i_p]_h
template <typename T> struct Gatv2BwdColArgs
{
    int nrow;               // rows of the transposed handle
    int nv;
    int heads;
    const int *rowptr;
    const int *colidx;      // rows of XT / dO / lse / delta (one source: no negative code)
    const T   *val;         // the transposed handle's values in T (bias), or nullptr
    T          slope;
    const T   *XS;
    int64_t    ldXS;
    const T   *XT;
    int64_t    ldXT;
    const T   *av;
    const T   *dO;
    int64_t    lddO;
    const T   *lse;
    const T   *delta;
    T         *dXS;         // may be XS exactly (a group reads its slice whole before it writes it)
    int64_t    lddXS;
    const int *rowmap;      // nullptr, or the XS / dXS row of every row (row-subset matrices)
    DropArgs<T> drop;       // attention dropout (dropout.h); off by default
};

// The instance every SpMM launcher names at its hipLaunchKernelGGL, from its own template arguments ("rowgroup<16,2,1>",
// "panel<8,2,2,a32,b1>", "team2<f64,NV1,b0,compact>", ...): a string with static storage, per host thread.  hip_api.hip copies
// it into the handle after the product (crp_csr_dev_last_kernel); nothing else reads it.
extern thread_local const char *t_last_kernel;
// "<family><a,b,c>" once per instantiation (the function-local buffer is the instance's name for the life of the library)
#define CRP_KERNEL_NAME(...)                                                         \
    do                                                                               \
    {                                                                                \
        static char name_[48];                                                       \
        static const int once_ = snprintf(name_, sizeof(name_), __VA_ARGS__);        \
        (void) once_;                                                                \
        ::crp::t_last_kernel = name_;                                                \
    } while (0)

// narrow_kernel.hip: row-panel format, n <= 64 (several entries of a panel per instruction)
bool spmm_narrow_applicable(const PanelArgs &p, const SpmmArgs &a);
hipError_t spmm_rm_f64_narrow(const PanelArgs &p, const SpmmArgs &a, hipStream_t s);

// spmm_kernels.hip
hipError_t spmm_rm_f64_rowgroup(const SpmmArgs &a, hipStream_t s);
hipError_t spmm_cm_f64(const SpmmArgs &a, hipStream_t s);
hipError_t spmm_rm_f64_panel(const PanelArgs &p, const SpmmArgs &a, hipStream_t s);

// team2r_kernel.hip (Team2RHost streams; the argument block is Team2NArgs: same arrays, tvoff in units of 16 bytes)
hipError_t spmm_rm_f64_team2r(const Team2NArgs &t, const SpmmArgs &a, hipStream_t s);
hipError_t team2r_fill_rows(const Team2NArgs &t, const SpmmArgs &a, hipStream_t s);      // the C rows into the entry table: once per row map

// team2_kernel.hip
hipError_t spmm_rm_f64_team2(const Team2Args &t, const SpmmArgs &a, hipStream_t s);
hipError_t spmm_rm_f32_team2(const Team2Args &t, const SpmmArgsF32 &a, hipStream_t s);

// spmm_f32.hip: CSR row-group kernel of the fp32 path (any width, both sources)
hipError_t spmm_rm_f32_rowgroup(const SpmmArgsF32 &a, hipStream_t s);

// sddmm_kernels.hip: row-major operands, any width and alignment, both sources
hipError_t sddmm_rm_f64(const SddmmArgs<double> &a, hipStream_t s);
hipError_t sddmm_rm_f32(const SddmmArgs<float> &a, hipStream_t s);

// attention_kernels.hip: fused scores, online row softmax and product with V; row-major operands, any widths and alignment.
// mh: over (row, head) units -- a.heads heads of a.nk / a.nv columns each, side by side in every operand; lse is (rows, heads) and
// p_out (nnz, heads).  Head h's bits are the single-head instances' on the column views of head h.  (mh is the entry point's, not
// a.heads > 1: a multi-head call of one head runs the multi-head instances, a single-head call never does.)
hipError_t attention_rm(const AttnArgs<double> &a, bool mh, hipStream_t s);
hipError_t attention_rm(const AttnArgs<float> &a, bool mh, hipStream_t s);

// attention_bwd_kernels.hip: the fused backward of attention_rm; nk and nv at most ATTN_BWD_MAX_PIECES * 64 * (16 / sizeof(T)).
// mh: over (row, head) and (column, head) units; the cap applies to one head's widths
constexpr int ATTN_BWD_MAX_PIECES = 4;
hipError_t attention_bwd_q(const AttnBwdQArgs<double> &a, bool mh, hipStream_t s);
hipError_t attention_bwd_q(const AttnBwdQArgs<float> &a, bool mh, hipStream_t s);
hipError_t attention_bwd_kv(const AttnBwdKVArgs<double> &a, bool mh, hipStream_t s);
hipError_t attention_bwd_kv(const AttnBwdKVArgs<float> &a, bool mh, hipStream_t s);

// gat_kernels.hip: the fused GAT attention (additive LeakyReLU scores) over (row, head) units and its two-handle backward; the
// backward's per-head width is capped as attention_bwd's.  a.drop.on takes the DROP instances (attention dropout, dropout.h)
hipError_t gat_attention_rm(const GatArgs<double> &a, hipStream_t s);
hipError_t gat_attention_rm(const GatArgs<float> &a, hipStream_t s);
hipError_t gat_attention_bwd_row(const GatBwdRowArgs<double> &a, hipStream_t s);
hipError_t gat_attention_bwd_row(const GatBwdRowArgs<float> &a, hipStream_t s);
hipError_t gat_attention_bwd_col(const GatBwdColArgs<double> &a, hipStream_t s);
hipError_t gat_attention_bwd_col(const GatBwdColArgs<float> &a, hipStream_t s);

// gatv2_kernels.hip: the fused GATv2 attention (a LeakyReLU inside the dot with a) over (row, head) units and its two-handle
// backward; the per-head width is capped as attention_bwd's, in both directions.  a.drop.on takes the DROP instances
hipError_t gatv2_attention_rm(const Gatv2Args<double> &a, hipStream_t s);
hipError_t gatv2_attention_rm(const Gatv2Args<float> &a, hipStream_t s);
hipError_t gatv2_attention_bwd_row(const Gatv2BwdRowArgs<double> &a, hipStream_t s);
hipError_t gatv2_attention_bwd_row(const Gatv2BwdRowArgs<float> &a, hipStream_t s);
hipError_t gatv2_attention_bwd_col(const Gatv2BwdColArgs<double> &a, hipStream_t s);
hipError_t gatv2_attention_bwd_col(const Gatv2BwdColArgs<float> &a, hipStream_t s);

// dropout_kernels.hip: the keep flags of dropout.h over a CSR, (nnz, heads) bytes at (out_pos ? out_pos[p] : p) * heads + h
hipError_t dropout_mask_csr(int nrow, int heads, const int *rowptr, const int *colidx, const int *rowmap, bool transposed, double drop,
                            unsigned long long seed, uint8_t *mask, const int *out_pos, hipStream_t s);

// softmax_kernels.hip: row softmax over a CSR pattern and its Jacobian product; rowptr entries index the value arrays directly
hipError_t row_softmax_f64(int nrow, const int *rowptr, const double *s, double *y, hipStream_t st);
hipError_t row_softmax_f32(int nrow, const int *rowptr, const float *s, float *y, hipStream_t st);
hipError_t row_softmax_bwd_f64(int nrow, const int *rowptr, const double *y, const double *dy, double *ds, hipStream_t st);
hipError_t row_softmax_bwd_f32(int nrow, const int *rowptr, const float *y, const float *dy, float *ds, hipStream_t st);

// row_kernels.hip
hipError_t gather_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, int64_t lds,
                           double *dst, int64_t ldd, hipStream_t s);
hipError_t scatter_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, int64_t lds,
                            double *dst, int64_t ldd, hipStream_t s);
hipError_t scatter_vals_f64(int64_t n, const uint32_t *map, const double *src, double *dst, hipStream_t s);
// dst[i] = (double) src[map ? map[i] : i]
hipError_t gather_vals_f64(int64_t n, const int *map, const double *src, double *dst, hipStream_t s);
hipError_t gather_vals_f32_f64(int64_t n, const int *map, const float *src, double *dst, hipStream_t s);
hipError_t scatter_add_rows_f64(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const double *src,
                                int64_t lds, double *dst, int64_t ldd, hipStream_t s);
hipError_t scatter_add_rows_f32(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const float *src,
                                int64_t lds, float *dst, int64_t ldd, hipStream_t s);
// out[p] = the sum over j < nseg of src[j * seg_stride + p], added left to right (p < len)
hipError_t sum_segments_f64(int nseg, int64_t len, const double *src, int64_t seg_stride, double *out, hipStream_t s);
hipError_t sum_segments_f32(int nseg, int64_t len, const float *src, int64_t seg_stride, float *out, hipStream_t s);
// out[j] = the sum of column j of src (nrow x n): blocks of 256 rows from +0 in ascending row into work, then sum_segments over the blocks
hipError_t col_sum_f64(int nrow, int n, const double *src, int64_t lds, double *work, double *out, hipStream_t s);
hipError_t col_sum_f32(int nrow, int n, const float *src, int64_t lds, float *work, float *out, hipStream_t s);
hipError_t convert_f64_f32(int64_t n, const double *src, float *dst, hipStream_t s);
hipError_t transpose_f64(int nrow, int ncol, const double *src, int64_t lds, double *dst, int64_t ldd,
                         hipStream_t s);
hipError_t gather_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, int64_t lds,
                           float *dst, int64_t ldd, hipStream_t s);
hipError_t scatter_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, int64_t lds,
                            float *dst, int64_t ldd, hipStream_t s);
hipError_t transpose_f32(int nrow, int ncol, const float *src, int64_t lds, float *dst, int64_t ldd, hipStream_t s);
// csr_mat_row_part_comm_size on a device-resident CSR (bits: nblk * ceil(ncol / 32) words, zeroed; comm_dev: nblk ints, zeroed)
hipError_t row_part_comm_size(int nrow, int ncol, const int *rowptr, const int *colidx, int nblk, const int *rblk_dev, const int *xd_dev,
                              unsigned *bits, int *comm_dev, int *bad_dev, hipStream_t s);
hipError_t probe_copy(int64_t bytes, const void *src, void *dst, int blocks, unsigned long long *stamps, hipStream_t s);
hipError_t probe_stamp(unsigned long long *out, hipStream_t s);

}  // namespace crp
