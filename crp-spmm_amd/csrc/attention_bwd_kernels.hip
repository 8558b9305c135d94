// attention_bwd_kernels.hip -- the fused backward of the sparse attention (attention_kernels.hip) for gfx950 (MI355X, wave64),
// fp64 and fp32.  With O and lse as the forward wrote them and the upstream gradient dO, for every nonzero p = (i, c):
//     s_p  = scale * < Q[i][0:nk], K[c][0:nk] >      (bias: + the handle's current value of p, exactly as the forward forms it)
//     p_p  = exp(s_p - lse[i])          dP_p = < dO[i][0:nv], V[c][0:nv] >          D_i = < dO[i][0:nv], O[i][0:nv] >
//     dS_p = p_p * (dP_p - D_i)
//     dQ[i] = scale * sum_{p in row i} dS_p K[c_p]     dK[c] = scale * sum_{p in column c} dS_p Q[i_p]     dV[c] = sum_{p in column c} p_p dO[i_p]
// in two kernels, neither of which writes anything nnz-sized unless ds_out is asked for:
//     bwd_q   over a handle of A:    a group of lanes owns row i and writes dQ[i], delta[i] = D_i and optionally ds_out[p] = dS_p;
//     bwd_kv  over a handle of A^T:  a group owns column c, keeps K[c], V[c] and both accumulators in registers, re-forms s, p, dP
//             and dS of every entry of the column with the same routines (the same bits as the row side) and writes dK[c], dV[c].
// No atomics, no LDS, no partial result in memory.
//
// INSTANCE.  W = elements per 16 bytes, G(n) = 8, 16, 32, 64 for n <= 8 W, 16 W, 32 W, else (the SDDMM's group for a width n),
// LPR = max(G(nk), G(nv)); column j of every operand belongs to lane (j / W) % LPR, piece (j / W) / LPR of that lane: the
// forward's assignment.  A lane keeps PK = 1, 2 or 4 pieces of the nk-wide rows and PV = 1, 2 or 4 of the nv-wide ones, the
// smallest that covers the width; wider operands (nk or nv > 4 * 64 * W) are refused by the launchers.  All of it is a function
// of (dtype, nk, nv) alone.  Operands that cannot be accessed in 16-byte pieces (odd widths or leading dimensions, unaligned
// pointers) are accessed element by element in the SAME assignment.
//
// FIXED ORDER.  Both dots of an entry are the SDDMM's for (dtype, nk) and (dtype, nv): a lane adds its products in ascending j
// with FMAs from +0 and the lanes' sums meet in the balanced binary tree over the lane number (lanes past G(n) hold +0, which the
// tree adds exactly).  D_i is the same dot of dO[i] and O[i].  s = dot * scale (bias: then + val), p = exp(s - lse),
// dS = p * (dP - D): one subtraction, one multiplication; p == 0 gives dS = +0.  Entries go in batches of 8 in ascending p, and
// per batch acc[j] = fma(dS_u, K[c_u][j], acc[j]) for u = 0 .. 7 (kv: accK with Q[i_u], accV = fma(p_u, dO[i_u][j], accV)), from
// +0; slots of a last partial batch count as p = dS = +0 with the row's last entry's operand rows.  After the row
// dQ = acc * scale (dK = accK * scale, dV = accV).  A row's (column's) bits depend on (dtype, nk, nv, scale, bias) and its entries
// in the handle's CSR order ONLY: not on alignment, leading dimensions, the source a row comes from, the handle (full or row
// subset), the optional output or the other rows.
//
// SPECIAL CASES.  lse[i] == -inf (an empty or all-masked row): every p and dS of the row is +0 and dQ[i] = +0.  s_p = -inf: p =
// dS = +0.  An empty row of either handle writes +0 to its outputs; delta is still written.  NaN or +inf among a row's scores:
// that row's outputs (kv: those of the columns it touches) are unspecified.
//
// ALIASING.  bwd_kv: dK == K and dV == V (exactly) are legal: a group reads its K and V row whole before it writes them, and no
// other group reads them.  bwd_q: no output may alias an input.
//
// MULTI-HEAD (the MH instances: attention_bwd_q / attention_bwd_kv with mh).  a.heads = H heads of nk / nv columns each, side by
// side in every operand, as in the forward: a group owns the unit (row, head) = (u / H, u % H) -- bwd_kv: (column c, head h) -- and
// works on the column views of its head, so head h's bits are the single-head instance's.  lse and delta are (rows of A, H)
// row-major, ds_out (nnz, H); val[p] is shared by the heads.  dK == K and dV == V stay legal: a group reads its own slice of the row
// whole before it writes it, and no other group reads that slice.  The cap applies to one head's widths.  The single-head
// instances (MH = false) compile none of this.
//
// LOADS IN FLIGHT.  Per batch, the gathers of a step (per lane two 16-byte pieces, or one piece by elements, of each of the 8 K
// rows and of the 8 V rows; kv: Q and dO rows) are all issued before the step's FMAs.  The second read of a batch's rows, for the
// accumulators, goes through rg_again's opaque zero (row_group.h, which says what would fold it and how the build notices).
//
// The pieces, the row loads and stores, rg_load8 and the batch's butterfly (rg_reduce8) are row_group.h's (rg_), one definition
// for this file, gat_kernels.hip and gatv2_kernels.hip; ab_ marks what is this file's own: the two-operand dots and the entry.
#include "row_group.h"

namespace crp {

// part[u] += < this lane's pieces piece0 .. of x, of row u >: FMAs in column order (the SDDMM's chunk)
template <typename T, int LPR, int CH, int NP>
__device__ __forceinline__ void ab_fma_dot(T (&part)[RG_UNR], const T (&x)[NP][Piece<T>::VW], const T (&yv)[RG_UNR][CH][Piece<T>::VW],
                                           const int piece0, const int n, const int lir)
{
    constexpr int VW = Piece<T>::VW;
#pragma unroll
    for (int u = 0; u < RG_UNR; u++)
#pragma unroll
        for (int v = 0; v < CH; v++)
#pragma unroll
            for (int w = 0; w < VW; w++)
            {
                const int c = ((piece0 + v) * LPR + lir) * VW + w;
                if (c < n) part[u] = fma(x[piece0 + v][w], yv[u][v][w], part[u]);
            }
}

// acc[piece] = fma(coef[u], row u's piece, acc[piece]) for u = 0 .. 7 (slots past the width gather garbage that is never stored)
template <typename T, int CH, int NP>
__device__ __forceinline__ void ab_fma_acc(T (&acc)[NP][Piece<T>::VW], const T (&coef)[RG_UNR], const T (&yv)[RG_UNR][CH][Piece<T>::VW],
                                           const int piece0)
{
    constexpr int VW = Piece<T>::VW;
#pragma unroll
    for (int u = 0; u < RG_UNR; u++)
#pragma unroll
        for (int v = 0; v < CH; v++)
#pragma unroll
            for (int w = 0; w < VW; w++) acc[piece0 + v][w] = fma(coef[u], yv[u][v][w], acc[piece0 + v][w]);
}

// partA[u] = the lane's part of < xa, rows ya[u] > (width na, PA pieces), partB likewise: per step the gathers of both operands
// (two pieces per lane and row at most) go out before the step's FMAs
template <typename T, int LPR, int PA, int PB, bool VEC>
__device__ __forceinline__ void ab_dots2(T (&partA)[RG_UNR], const T (&xa)[PA][Piece<T>::VW], const T *const (&ya)[RG_UNR], const int na,
                                         T (&partB)[RG_UNR], const T (&xb)[PB][Piece<T>::VW], const T *const (&yb)[RG_UNR], const int nb,
                                         const int lir)
{
    constexpr int VW = Piece<T>::VW;
    constexpr int CA = rg_ch<PA, VEC>, CB = rg_ch<PB, VEC>, PM = PA > PB ? PA : PB;
#pragma unroll
    for (int u = 0; u < RG_UNR; u++) partA[u] = partB[u] = (T) 0;
    rg_static_for<0, PM, (VEC ? 2 : 1)>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        T va[RG_UNR][CA][VW], vb[RG_UNR][CB][VW];
        if constexpr (K < PA) rg_load8<T, LPR, CA, VEC>(va, ya, K, na, lir);
        if constexpr (K < PB) rg_load8<T, LPR, CB, VEC>(vb, yb, K, nb, lir);
        __builtin_amdgcn_sched_barrier(0);              // every load of the step is in flight before the first FMA waits for one
        if constexpr (K < PA) ab_fma_dot<T, LPR, CA, PA>(partA, xa, va, K, na, lir);
        if constexpr (K < PB) ab_fma_dot<T, LPR, CB, PB>(partB, xb, vb, K, nb, lir);
        if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);      // (by elements: the next step's loads wait, for the registers)
    });
}

// p and dS of one entry from its two dots (see FIXED ORDER); dead: lse == -inf
template <typename T>
__device__ __forceinline__ void ab_entry(const T dot, const T dp, const T scale, const T *val, const int p, const T lse, const T delta,
                                         const bool dead, T *pp, T *ds)
{
    T s = dot * scale;
    if (val != nullptr) s = s + val[p];
    const T e = dead ? (T) 0 : rg_exp(s - lse);
    *pp = e;
    *ds = (e == (T) 0) ? (T) 0 : e * (dp - delta);
}

// LPR lanes per row; PK / PV pieces per lane of the nk- / nv-wide rows.  VEC: 16-byte accesses; else single elements.
// MH: a group owns the unit (row, head) = (u / heads, u % heads), nk and nv are the widths of one head, and head h's slices start
// at column h * nk and h * nv; lse and delta are (rows, heads), ds_out is (nnz, heads).  Without MH none of it is compiled.
template <typename T, int LPR, int PK, int PV, bool VEC, bool MH = false>
__global__ __launch_bounds__(256) void attention_bwd_q_kernel(const AttnBwdQArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr int CK  = rg_ch<PK, VEC>;
    const int lir = threadIdx.x % LPR;                  // lane in row group
    int row = blockIdx.x * RPB + threadIdx.x / LPR;
    int64_t nh = 1, h = 0;                              // heads, and this group's
    if constexpr (MH)
    {
        const int64_t u = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR;
        nh = a.heads;
        if (u >= (int64_t) a.nrow * nh) return;
        row = (int) (u / nh);
        h = u % nh;
    }
    else if (row >= a.nrow) return;
    int pb = a.rowptr[row];
    const int pe = a.rowptr[row + 1];
    if constexpr (LPR == 64) pb = __builtin_amdgcn_readfirstlane(pb);
    const int nk = a.nk, nv = a.nv;
    const int64_t orow = a.rowmap ? a.rowmap[row] : row;
    const int64_t hk = h * nk, hv = h * nv;             // the head's first column (MH; else 0)
    const int64_t srow = MH ? orow * nh + h : orow;     // the unit's entry of lse and delta
    auto ppos = [&](const int pos) {                    // where nonzero position pos of this unit lies in ds_out
        if constexpr (MH) return pos * nh + h;
        else return pos;
    };
    const T ninf = rg_ninf<T>();

    // D = < dO[i], O[i] >, the SDDMM's dot for (dtype, nv); every lane of the group ends with the same bits
    T xd[PV][VW];
    rg_load_row<T, LPR, PV, VEC>(xd, a.dO + orow * a.lddO + hv, nv, lir);
    T delta = (T) 0;
    {
        T xo[PV][VW];
        rg_load_row<T, LPR, PV, VEC>(xo, a.O + orow * a.ldO + hv, nv, lir);
#pragma unroll
        for (int v = 0; v < PV; v++)
#pragma unroll
            for (int w = 0; w < VW; w++)
                if ((v * LPR + lir) * VW + w < nv) delta = fma(xd[v][w], xo[v][w], delta);
#pragma unroll
        for (int mask = 1; mask < LPR; mask <<= 1) delta = delta + __shfl_xor(delta, mask, LPR);
    }
    if (lir == 0) a.delta[srow] = delta;

    T acc[PK][VW];
#pragma unroll
    for (int v = 0; v < PK; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) acc[v][w] = (T) 0;
    T *const dqrow = a.dQ + orow * a.lddQ + hk;
    const T lse = a.lse[srow];
    if (pb >= pe || lse == ninf)                        // an empty or all-masked row: +0 everywhere; no Q row is read
    {
        rg_store_row<T, LPR, PK, VEC>(acc, dqrow, nk, lir);
        if (a.ds_out != nullptr)
            for (int p = pb + lir; p < pe; p += LPR) a.ds_out[ppos(a.out_pos ? a.out_pos[p] : p)] = (T) 0;
        return;
    }
    T xq[PK][VW];
    rg_load_row<T, LPR, PK, VEC>(xq, a.Q + orow * a.ldQ + hk, nk, lir);
    const T scale = a.scale;
    const int again = rg_again<VW>(a.nk);

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose dS counts as +0
            const T *krow[UNR], *vrow[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++)
            {
                const int cj = rg_bcast_i<LPR>(c, min(j + u, cnt - 1));
                krow[u] = ((cj >= 0) ? (a.K0 + (int64_t) cj * a.ldK0) : (a.K1 + (int64_t) (~cj) * a.ldK1)) + hk;
                vrow[u] = ((cj >= 0) ? (a.V0 + (int64_t) cj * a.ldV0) : (a.V1 + (int64_t) (~cj) * a.ldV1)) + hv;
            }
            T ps[UNR], pp[UNR];
            ab_dots2<T, LPR, PK, PV, VEC>(ps, xq, krow, nk, pp, xd, vrow, nv, lir);
            const T rs = rg_reduce8<T, LPR>(ps, lir), rp = rg_reduce8<T, LPR>(pp, lir);
            // every lane holds both dots of entry (lir & 7) of the batch
            const int mine = j + (lir & 7);
            T prob = (T) 0, ds = (T) 0;
            if (mine < cnt)
            {
                const int p = p0 + mine;
                ab_entry<T>(rs, rp, scale, a.val, p, lse, delta, false, &prob, &ds);
                if (a.ds_out != nullptr && lir < UNR) a.ds_out[ppos(a.out_pos ? a.out_pos[p] : p)] = ds;
            }
            T coef[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) coef[u] = __shfl(ds, u, LPR);
#pragma unroll
            for (int k = 0; k < PK; k += CK)
            {
                T kv[UNR][CK][VW];
                rg_load8<T, LPR, CK, VEC>(kv, krow, k, nk, lir, again);      // (cache hits: the dots read these rows)
                __builtin_amdgcn_sched_barrier(0);
                ab_fma_acc<T, CK, PK>(acc, coef, kv, k);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < PK; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) acc[v][w] = acc[v][w] * scale;
    rg_store_row<T, LPR, PK, VEC>(acc, dqrow, nk, lir);
}

// MH: the unit is (column c, head h); lse and delta of row i of A are read at i * heads + h
template <typename T, int LPR, int PK, int PV, bool VEC, bool MH = false>
__global__ __launch_bounds__(256) void attention_bwd_kv_kernel(const AttnBwdKVArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr int CK  = rg_ch<PK, VEC>, CV = rg_ch<PV, VEC>, PM = PK > PV ? PK : PV;
    const int lir = threadIdx.x % LPR;
    int row = blockIdx.x * RPB + threadIdx.x / LPR;
    int64_t nh = 1, h = 0;                              // heads, and this group's
    if constexpr (MH)
    {
        const int64_t u = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR;
        nh = a.heads;
        if (u >= (int64_t) a.nrow * nh) return;
        row = (int) (u / nh);
        h = u % nh;
    }
    else if (row >= a.nrow) return;
    int pb = a.rowptr[row];
    const int pe = a.rowptr[row + 1];
    if constexpr (LPR == 64) pb = __builtin_amdgcn_readfirstlane(pb);
    const int nk = a.nk, nv = a.nv;
    const int64_t crow = a.rowmap ? a.rowmap[row] : row;
    const T ninf = rg_ninf<T>();
    const int64_t hk = h * nk, hv = h * nv;             // the head's first column (MH; else 0)
    T *const dkrow = a.dK + crow * a.lddK + hk;
    T *const dvrow = a.dV + crow * a.lddV + hv;

    T accK[PK][VW], accV[PV][VW];
#pragma unroll
    for (int v = 0; v < PK; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accK[v][w] = (T) 0;
#pragma unroll
    for (int v = 0; v < PV; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accV[v][w] = (T) 0;
    if (pb >= pe)                                       // a column no row names: +0; its K and V rows are not read
    {
        rg_store_row<T, LPR, PK, VEC>(accK, dkrow, nk, lir);
        rg_store_row<T, LPR, PV, VEC>(accV, dvrow, nv, lir);
        return;
    }
    // K[c] and V[c] whole, before anything of this row is written (dK == K, dV == V)
    T xk[PK][VW], xv[PV][VW];
    rg_load_row<T, LPR, PK, VEC>(xk, a.K + crow * a.ldK + hk, nk, lir);
    rg_load_row<T, LPR, PV, VEC>(xv, a.V + crow * a.ldV + hv, nv, lir);
    const T scale = a.scale;
    const int again = rg_again<VW>(a.nk);

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        for (int j = 0; j < cnt; j += UNR)
        {
            const T *qrow[UNR], *drow[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++)
            {
                const int ij = rg_bcast_i<LPR>(c, min(j + u, cnt - 1));
                qrow[u] = a.Q + (int64_t) ij * a.ldQ + hk;
                drow[u] = a.dO + (int64_t) ij * a.lddO + hv;
            }
            T ps[UNR], pp[UNR];
            ab_dots2<T, LPR, PK, PV, VEC>(ps, xk, qrow, nk, pp, xv, drow, nv, lir);
            const T rs = rg_reduce8<T, LPR>(ps, lir), rp = rg_reduce8<T, LPR>(pp, lir);
            const int mine = j + (lir & 7);
            const int im = __shfl(c, min(mine, cnt - 1), LPR);          // the row of A of this lane's entry
            T prob = (T) 0, ds = (T) 0;
            if (mine < cnt)
            {
                auto sidx = [&](const int i) {                                  // row i's entry of lse and delta
                    if constexpr (MH) return i * nh + h;
                    else return i;
                };
                const T lse = a.lse[sidx(im)];
                ab_entry<T>(rs, rp, scale, a.val, p0 + mine, lse, a.delta[sidx(im)], lse == ninf, &prob, &ds);
            }
            T cs[UNR], cp[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++)
            {
                cs[u] = __shfl(ds, u, LPR);
                cp[u] = __shfl(prob, u, LPR);
            }
            rg_static_for<0, PM, (VEC ? 2 : 1)>([&](auto kc) {
                constexpr int K = decltype(kc)::value;
                T qv[UNR][CK][VW], dv[UNR][CV][VW];
                if constexpr (K < PK) rg_load8<T, LPR, CK, VEC>(qv, qrow, K, nk, lir, again);      // (cache hits: the dots read these rows)
                if constexpr (K < PV) rg_load8<T, LPR, CV, VEC>(dv, drow, K, nv, lir, again);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (K < PK) ab_fma_acc<T, CK, PK>(accK, cs, qv, K);
                if constexpr (K < PV) ab_fma_acc<T, CV, PV>(accV, cp, dv, K);
                if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
            });
        }
    }
#pragma unroll
    for (int v = 0; v < PK; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accK[v][w] = accK[v][w] * scale;
    rg_store_row<T, LPR, PK, VEC>(accK, dkrow, nk, lir);
    rg_store_row<T, LPR, PV, VEC>(accV, dvrow, nv, lir);
}

// (nk % VW == 0 and nv % VW == 0 keep every head's slice on a 16-byte boundary; the leading dimension of a source that is NULL is
// not read: it counts as 0.  The single-head instances take a.heads as 1, whatever it holds)
template <typename T, int LPR, int PK, int PV, bool MH>
static hipError_t launch_bwd(const AttnBwdQArgs<T> &a, hipStream_t s)
{
    const bool vec = rg_aligned({a.Q, a.K0, a.K1, a.V0, a.V1, a.O, a.dO, a.dQ},
                                {a.nk, a.nv, a.ldQ, a.ldO, a.lddO, a.lddQ, a.K0 ? a.ldK0 : 0, a.K0 ? a.ldV0 : 0, a.K1 ? a.ldK1 : 0,
                                 a.K1 ? a.ldV1 : 0}, Piece<T>::VW);
    dim3 grid;
    if (!rg_grid(a.nrow, MH ? a.heads : 1, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL((attention_bwd_q_kernel<T, LPR, PK, PV, true, MH>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attention_bwd_q_kernel<T, LPR, PK, PV, false, MH>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <typename T, int LPR, int PK, int PV, bool MH>
static hipError_t launch_bwd(const AttnBwdKVArgs<T> &a, hipStream_t s)
{
    const bool vec = rg_aligned({a.K, a.V, a.Q, a.dO, a.dK, a.dV}, {a.nk, a.nv, a.ldK, a.ldV, a.ldQ, a.lddO, a.lddK, a.lddV}, Piece<T>::VW);
    dim3 grid;
    if (!rg_grid(a.nrow, MH ? a.heads : 1, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL((attention_bwd_kv_kernel<T, LPR, PK, PV, true, MH>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attention_bwd_kv_kernel<T, LPR, PK, PV, false, MH>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <typename T, int PK, bool MH, class Args>
static hipError_t bwd_wave(const Args &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T);
    if (a.nv <= 64 * W)  return launch_bwd<T, 64, PK, 1, MH>(a, s);
    if (a.nv <= 128 * W) return launch_bwd<T, 64, PK, 2, MH>(a, s);
    return launch_bwd<T, 64, PK, 4, MH>(a, s);
}

// The instance, from (dtype, nk, nv) alone (the rule is stated at the top of this file); MH: from the widths of one head
template <typename T, bool MH, class Args>
static hipError_t attention_bwd(const Args &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T), CAP = ATTN_BWD_MAX_PIECES * 64 * W;
    if (a.nk > CAP || a.nv > CAP) return hipErrorInvalidValue;         // (the entry points refuse these before they come here)
    if (a.nrow <= 0) return hipSuccess;
    const int wide = a.nk > a.nv ? a.nk : a.nv;
    if (wide <= 8 * W)  return launch_bwd<T, 8, 1, 1, MH>(a, s);
    if (wide <= 16 * W) return launch_bwd<T, 16, 1, 1, MH>(a, s);
    if (wide <= 32 * W) return launch_bwd<T, 32, 1, 1, MH>(a, s);
    if (a.nk <= 64 * W)  return bwd_wave<T, 1, MH>(a, s);
    if (a.nk <= 128 * W) return bwd_wave<T, 2, MH>(a, s);
    return bwd_wave<T, 4, MH>(a, s);
}

// mh: the (row, head) / (column, head) instances, whatever a.heads; else the single-head ones
template <typename T, class Args>
static hipError_t attention_bwd_of(const Args &a, bool mh, hipStream_t s)
{
    if (!mh) return attention_bwd<T, false>(a, s);
    return attention_bwd<T, true>(a, s);
}
hipError_t attention_bwd_q(const AttnBwdQArgs<double> &a, bool mh, hipStream_t s) { return attention_bwd_of<double>(a, mh, s); }
hipError_t attention_bwd_q(const AttnBwdQArgs<float> &a, bool mh, hipStream_t s) { return attention_bwd_of<float>(a, mh, s); }
hipError_t attention_bwd_kv(const AttnBwdKVArgs<double> &a, bool mh, hipStream_t s) { return attention_bwd_of<double>(a, mh, s); }
hipError_t attention_bwd_kv(const AttnBwdKVArgs<float> &a, bool mh, hipStream_t s) { return attention_bwd_of<float>(a, mh, s); }

}  // namespace crp
