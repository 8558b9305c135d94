// gat_kernels.hip -- fused GAT attention over A's pattern for gfx950 (MI355X, wave64), fp64 and fp32, forward and backward.
// For every row i, head h and entry p = (i, c_p), p in the handle's CSR order:
//     z_p = el[i][h] + er[c_p][h]          a_p = z_p > 0 ? z_p : slope * z_p          s_p = a_p (bias: + A's current value of p)
//     O[i]_h = sum_p softmax_p(s) * V[c_p]_h
// -- the additive LeakyReLU score of a graph attention layer in place of the scaled dot product of attention_kernels.hip: two
// scalars per node and head and no K.  From the scores on everything is attention_kernels.hip's: the batches of 8, the online
// softmax, lse / p_out, the (row, head) units and the column-to-lane assignment.  No atomics, no LDS, no partial result in memory.
// The pieces, the row loads and stores, the walk over a batch's 8 rows, the batch's butterfly, the keep bits and the launcher are
// row_group.h's (rg_), one definition for this file, gatv2_kernels.hip and the attention's two; gt_ marks what is this score's own.
//
// OPERANDS.  heads = H >= 1 heads of nv columns each lie side by side in V / O / dO / dV: head h owns columns [h nv, (h + 1) nv).
// el is (rows of O, H) with leading dimension ldel, read through the row map like Q; er0 / er1 are the two sources of the column
// code exactly as V0 / V1 (c >= 0 -> row c of er0 / V0, c < 0 -> row ~c of er1 / V1).  lse, delta are (rows, H) row-major;
// p_out, ds_out are (nnz, H): entry (pos, h) at pos * H + h with pos = out_pos[p], or p.  val[p] (bias) is shared by the heads.
//
// INSTANCE.  W = elements per 16 bytes, G(n) = 8, 16, 32, 64 for n <= 8 W, 16 W, 32 W, else (the SDDMM's group for a width n):
// LPR = G(nv) lanes own the unit u = row * H + h (consecutive groups hold consecutive heads of a row).  Column j of the head's
// slice belongs to lane (j / W) % LPR, piece (j / W) / LPR of that lane.  Forward: PV = the smallest of 1, 2, 4, 8 pieces that
// covers nv; a wider head is processed in column blocks of 8 LPR W columns with the scores formed again for every block (same
// bits).  Backward: PV = 1, 2 or 4, wider heads are refused by the launchers.  Operands that cannot be accessed in 16-byte pieces
// are accessed element by element in the SAME assignment.
//
// SCORES.  Every lane forms the score of entry (lir & 7) of the batch itself, from one scalar load of er and the unit's el, which
// it keeps for the row: no K walk and no butterfly.  The gather of that scalar (and of the bias value) is issued ahead of the
// batch's V loads, and those before the exponentials.  z, a and s are rounded one by one -- gt_score compiles with contraction
// off, so slope * z + val never becomes an FMA -- and so is dZ = dS * g ahead of its sum (gt_dz).
//
// FIXED ORDER.  Forward: attention_kernels.hip's, verbatim, from s on; O, lse and p_out are bit for bit what that file's order
// gives for these scores and (dtype, nv).  Backward: p = exp(s - lse), dP = < dO[i]_h, V[c]_h > and D = < dO[i]_h, O[i]_h > as the
// SDDMM forms a dot for (dtype, nv) (per lane FMAs in ascending j from +0, then the balanced tree over the lane number),
// dS = p * (dP - D) (p == 0: +0), dZ = dS * g with g = z > 0 ? 1 : slope.  Row side (a handle of A): delta = D, d_el = the sum of
// the row's dZ, one IEEE addition per entry from +0 in ascending p, ds_out = dS.  Column side (a handle of A^T): d_er = the same
// sum in that handle's CSR order, dV[c][j] = fma(p_u, dO[i_u][j], acc) from +0 in that order.  s, p, dP, dS and dZ have the same
// bits on both sides.  Slots of a last partial batch count as s = -inf (forward) and p = dS = dZ = +0 (backward) with the row's
// last entry's operand rows.
//
// SPECIAL CASES.  attention_kernels.hip's and attention_bwd_kernels.hip's: an empty row writes +0 and lse = -inf for every head; a
// one-entry row gives O = V[c]; s = -inf (a bias value, or z = -inf with slope > 0) is a masked edge; an all-masked row gives
// zeros; NaN or +inf among a row's scores (slope = 0 with an infinite z is this case) leaves that row's outputs unspecified.
// Rows with lse = -inf give +0 everywhere in the backward; delta is still written.
//
// ALIASING.  Column side: dV == V (exactly) is legal, a group reads its slice of V[c] whole before it writes it.  Nothing else.
//
// DROPOUT (the DROP instances; a.drop, dropout.h).  k_p = the keep bit of (row of O, column code, head).  Forward:
// scores, batches, m, f, e_u and l are the plain call's -- the softmax runs over all edges -- and only the accumulator changes:
// acc = fma(k_u ? e_u : +0, V[c_u][j], acc), O = fl(fl(acc / l) rs); lse and p_out keep the plain call's bits.  Backward: p, s, g
// and D = < dO, O > (O is the dropped O) as above, dP' = k ? fl(dP rs) : +0, dS = p (dP' - D), and the value-side weight of dV is
// w = k ? fl(p rs) : +0.  The two products with rs are roundings of their own (rg_mul).  The lane that loads the column code of
// its own entry of a chunk draws that entry's bit -- one draw per entry and (unit, V block) -- and one ballot hands the chunk's
// bits to the group; a batch takes its 8 bits from that word.  DROP = false compiles to the code without any of this.
#include "row_group.h"

namespace crp {

// s = lrelu(el + er) (+ val): three statements, three roundings.  hipcc contracts across statements by default; here it may not.
// *g = the derivative of the LeakyReLU at z.
template <typename T>
__device__ __forceinline__ T gt_score(const T el, const T er, const T slope, const bool bias, const T val, T *g)
{
#pragma clang fp contract(off)
    const T z = el + er;
    const bool pos = z > (T) 0;
    T s = slope * z;
    s = pos ? z : s;
    if (bias) s = s + val;
    *g = pos ? (T) 1 : slope;
    return s;
}
// dZ = dS * g, rounded before it is added to anything
template <typename T>
__device__ __forceinline__ T gt_dz(const T ds, const T g)
{
#pragma clang fp contract(off)
    const T dz = ds * g;
    return dz;
}

// where the er scalar of column code c and head h lies
template <typename T>
__device__ __forceinline__ const T *gt_er(const int c, const int64_t h, const T *er0, const int64_t lder0, const T *er1, const int64_t lder1)
{
    return ((c >= 0) ? (er0 + (int64_t) c * lder0) : (er1 + (int64_t) (~c) * lder1)) + h;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// LPR lanes per unit (row, head); PV pieces of the accumulator per lane and V block.  VEC: 16-byte accesses; else elements.
template <typename T, int LPR, int PV, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gat_fwd_kernel(const GatArgs<T> a)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr int VC  = PV < 4 ? PV : 4;                // pieces of V per load chunk (8 VC pieces in flight)
    constexpr int VBW = LPR * VW * PV;                  // columns of a V block
    const int lir = threadIdx.x % LPR;                  // lane in the unit's group
    const int64_t u = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR;
    const int64_t nh = a.heads;
    if (u >= (int64_t) a.nrow * nh) return;
    const int row = (int) (u / nh);
    const int64_t h = u % nh;
    int pb = a.rowptr[row];
    const int pe = a.rowptr[row + 1];
    if constexpr (LPR == 64) pb = __builtin_amdgcn_readfirstlane(pb);
    const int nv = a.nv;
    const int64_t orow = a.rowmap ? a.rowmap[row] : row;        // rowmap: the el and O row of every row of a row-subset matrix
    const T ninf = rg_ninf<T>();
    const int64_t hv = h * nv;                          // the head's first column
    const int64_t srow = orow * nh + h;                 // the unit's entry of lse
    T *const orp = a.O + orow * a.ldO + hv;

    // this lane's piece v of block vb of O[orow]
    auto store_o = [&](const T (*acc)[VW], const int vb) {
#pragma unroll
        for (int v = 0; v < PV; v++)
        {
            const int c = vb + (v * LPR + lir) * VW;
            if constexpr (VEC)
            {
                PT t;
#pragma unroll
                for (int w = 0; w < VW; w++) t[w] = acc[v][w];
                if (c < nv) *reinterpret_cast<PT *>(orp + c) = t;
            }
            else
            {
#pragma unroll
                for (int w = 0; w < VW; w++)
                    if (c + w < nv) orp[c + w] = acc[v][w];
            }
        }
    };

    if (pb >= pe)                                       // an empty row: zeros; el is not read
    {
        T z[PV][VW];
#pragma unroll
        for (int v = 0; v < PV; v++)
#pragma unroll
            for (int w = 0; w < VW; w++) z[v][w] = (T) 0;
        for (int vb = 0; vb < nv; vb += VBW) store_o(z, vb);
        if (a.lse != nullptr && lir == 0) a.lse[srow] = ninf;
        return;
    }
    const T elv = a.el[orow * a.ldel + h];              // kept for the row
    const T slope = a.slope;
    const bool bias = a.val != nullptr;

    // this lane's pieces v0 .. v0 + VC - 1 of block vb of the 8 V rows (slots past nv: column 0, not used)
    auto load_v = [&](T (&vv)[UNR][VC][VW], const int vb, const int v0, const T *(&vrow)[UNR]) {
#pragma unroll
        for (int q = 0; q < UNR; q++)
#pragma unroll
            for (int v = 0; v < VC; v++)
            {
                const int c = vb + ((v0 + v) * LPR + lir) * VW;
                if constexpr (VEC)
                {
                    const PT t = *reinterpret_cast<const PT *>(vrow[q] + ((c < nv) ? c : 0));
#pragma unroll
                    for (int w = 0; w < VW; w++) vv[q][v][w] = t[w];
                }
                else
                {
#pragma unroll
                    for (int w = 0; w < VW; w++) vv[q][v][w] = vrow[q][(c + w < nv) ? c + w : 0];
                }
            }
    };

    for (int vb = 0; vb < nv; vb += VBW)
    {
        const bool first = vb == 0;                     // the block that writes lse and p_out
        T m = ninf, l = (T) 0;
        T acc[PV][VW];
#pragma unroll
        for (int v = 0; v < PV; v++)
#pragma unroll
            for (int w = 0; w < VW; w++) acc[v][w] = (T) 0;

        for (int p0 = pb; p0 < pe; p0 += LPR)
        {
            const int my = p0 + lir;
            const int c = (my < pe) ? a.colidx[my] : 0;
            const int cnt = min(LPR, pe - p0);
            unsigned long long km = 0;                  // (DROP: the chunk's keep bits)
            if constexpr (DROP) km = rg_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) orow, (uint32_t) c, (uint32_t) h, lir);
            for (int j = 0; j < cnt; j += UNR)
            {
                // the scalar of this lane's entry (lir & 7) of the batch goes out first: a tiny gather under the V loads.
                // Indices past the row end are clamped to the row's last entry: a valid row whose score counts as -inf
                const int mine = j + (lir & 7);
                const int mcl = min(mine, cnt - 1);
                const int cm = __shfl(c, mcl, LPR);
                const T erv = *gt_er<T>(cm, h, a.er0, a.lder0, a.er1, a.lder1);
                const T bv = bias ? a.val[p0 + mcl] : (T) 0;
                const T *vrow[UNR];
#pragma unroll
                for (int q = 0; q < UNR; q++)
                {
                    const int cj = rg_bcast_i<LPR>(c, min(j + q, cnt - 1));
                    vrow[q] = ((cj >= 0) ? (a.V0 + (int64_t) cj * a.ldV0) : (a.V1 + (int64_t) (~cj) * a.ldV1)) + hv;
                }
                // the first V pieces of the batch go out before the exponentials
                T vv[UNR][VC][VW];
                load_v(vv, vb, 0, vrow);
                __builtin_amdgcn_sched_barrier(0);

                T s = ninf;
                if (mine < cnt)
                {
                    T g;
                    s = gt_score<T>(elv, erv, slope, bias, bv, &g);
                    if (first && a.p_out != nullptr && lir < UNR)
                    {
                        const int p = p0 + mine;
                        a.p_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = s;
                    }
                }
                T bm = fmax(s, __shfl_xor(s, 1, LPR));
                bm = fmax(bm, __shfl_xor(bm, 2, LPR));
                bm = fmax(bm, __shfl_xor(bm, 4, LPR));
                const T mn = fmax(m, bm);
                T f = (T) 1, e = (T) 0;
                if (mn != ninf)                         // (else every entry so far is masked: l and acc stay 0)
                {
                    f = rg_exp(m - mn);
                    e = rg_exp(s - mn);
                }
                m = mn;
                T eu[UNR];
#pragma unroll
                for (int q = 0; q < UNR; q++) eu[q] = __shfl(e, q, LPR);
                l = l * f;
#pragma unroll
                for (int q = 0; q < UNR; q++) l = l + eu[q];
                if constexpr (DROP)                     // l has every edge; the accumulator takes the kept ones
                {
                    const unsigned kb = (unsigned) (km >> j);
#pragma unroll
                    for (int q = 0; q < UNR; q++) eu[q] = ((kb >> q) & 1u) ? eu[q] : (T) 0;
                }
#pragma unroll
                for (int v = 0; v < PV; v++)
#pragma unroll
                    for (int w = 0; w < VW; w++) acc[v][w] = acc[v][w] * f;
#pragma unroll
                for (int v0 = 0; v0 < PV; v0 += VC)
                {
                    if (v0 > 0)
                    {
                        load_v(vv, vb, v0, vrow);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int q = 0; q < UNR; q++)
#pragma unroll
                        for (int v = 0; v < VC; v++)
#pragma unroll
                            for (int w = 0; w < VW; w++) acc[v0 + v][w] = fma(eu[q], vv[q][v][w], acc[v0 + v][w]);
                }
            }
        }

        const bool masked = m == ninf;                  // every entry masked: zeros, not 0 / 0
#pragma unroll
        for (int v = 0; v < PV; v++)
#pragma unroll
            for (int w = 0; w < VW; w++)
            {
                acc[v][w] = masked ? (T) 0 : acc[v][w] / l;
                if constexpr (DROP) acc[v][w] = rg_mul<T>(acc[v][w], a.drop.rs);
            }
        store_o(acc, vb);
        if (first)
        {
            if (a.lse != nullptr && lir == 0) a.lse[srow] = masked ? ninf : m + rg_log(l);
            if (a.p_out != nullptr && lir < UNR)
                for (int p = pb + lir; p < pe; p += UNR)        // this lane's own stores
                {
                    const int64_t pos = (int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h;
                    const T sv = a.p_out[pos];
                    a.p_out[pos] = masked ? (T) 0 : rg_exp(sv - m) / l;
                }
        }
    }
}

// ---- backward: the pieces (row_group.h's, and the score's own) ----------------------------------------------------------------
// part[q] = the lane's part of < x, row y[q] > (width n, NP pieces): rg_walk8's trip, FMAs in column order from +0
template <typename T, int LPR, int NP, bool VEC>
__device__ __forceinline__ void gt_dots(T (&part)[RG_UNR], const T (&x)[NP][Piece<T>::VW], const T *const (&y)[RG_UNR], const int n,
                                        const int lir)
{
#pragma unroll
    for (int q = 0; q < RG_UNR; q++) part[q] = (T) 0;
    rg_walk8<T, LPR, NP, VEC>(y, n, lir, 0, [&](const int q, const int v, const int w, const bool in, const T yv) {
        if (in) part[q] = fma(x[v][w], yv, part[q]);
    });
}

// p, dS and dZ of one entry from its score, the LeakyReLU's derivative and dP (see FIXED ORDER); dead: lse == -inf.  DROP: dP
// counts as dP' = keep ? fl(dP rs) : +0, and *pp is the value-side weight w = keep ? fl(p rs) : +0 (see DROPOUT)
template <typename T, bool DROP>
__device__ __forceinline__ void gt_entry(const T s, const T g, T dp, const T lse, const T delta, const bool dead, const bool keep, const T rs,
                                         T *pp, T *ds, T *dz)
{
    const T e = dead ? (T) 0 : rg_exp(s - lse);
    if constexpr (DROP)
    {
        dp = keep ? rg_mul<T>(dp, rs) : (T) 0;
        *pp = keep ? rg_mul<T>(e, rs) : (T) 0;
    }
    else *pp = e;
    *ds = (e == (T) 0) ? (T) 0 : e * (dp - delta);
    *dz = (e == (T) 0) ? (T) 0 : gt_dz<T>(*ds, g);
}

// ---- backward, row side: delta, d_el and ds_out over a handle of A ----------------------------------------------------------------
template <typename T, int LPR, int PV, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gat_bwd_row_kernel(const GatBwdRowArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    const int lir = threadIdx.x % LPR;
    const int64_t u = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR;
    const int64_t nh = a.heads;
    if (u >= (int64_t) a.nrow * nh) return;
    const int row = (int) (u / nh);
    const int64_t h = u % nh;
    int pb = a.rowptr[row];
    const int pe = a.rowptr[row + 1];
    if constexpr (LPR == 64) pb = __builtin_amdgcn_readfirstlane(pb);
    const int nv = a.nv;
    const int64_t orow = a.rowmap ? a.rowmap[row] : row;
    const int64_t hv = h * nv;
    const int64_t srow = orow * nh + h;                 // the unit's entry of lse and delta
    const T ninf = rg_ninf<T>();

    // D = < dO[i]_h, O[i]_h >, the SDDMM's dot for (dtype, nv); every lane of the group ends with the same bits
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

    T *const delp = a.d_el + orow * a.ldd_el + h;
    const T lse = a.lse[srow];
    if (pb >= pe || lse == ninf)                        // an empty or all-masked row: +0 everywhere; el is not read
    {
        if (lir == 0) *delp = (T) 0;
        if (a.ds_out != nullptr)
            for (int p = pb + lir; p < pe; p += LPR) a.ds_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = (T) 0;
        return;
    }
    const T elv = a.el[orow * a.ldel + h];
    const T slope = a.slope;
    const bool bias = a.val != nullptr;
    T sum = (T) 0;                                      // d_el: the same bits in every lane

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits)
        if constexpr (DROP) km = rg_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) orow, (uint32_t) c, (uint32_t) h, lir);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose dS counts as +0
            const int mine = j + (lir & 7);
            const int mcl = min(mine, cnt - 1);
            const int cm = __shfl(c, mcl, LPR);
            const T erv = *gt_er<T>(cm, h, a.er0, a.lder0, a.er1, a.lder1);
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *vrow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++)
            {
                const int cj = rg_bcast_i<LPR>(c, min(j + q, cnt - 1));
                vrow[q] = ((cj >= 0) ? (a.V0 + (int64_t) cj * a.ldV0) : (a.V1 + (int64_t) (~cj) * a.ldV1)) + hv;
            }
            T pp[UNR];
            gt_dots<T, LPR, PV, VEC>(pp, xd, vrow, nv, lir);
            const T rp = rg_reduce8<T, LPR>(pp, lir);
            // every lane holds the score and dP of entry (lir & 7) of the batch
            T prob = (T) 0, ds = (T) 0, dz = (T) 0;
            if (mine < cnt)
            {
                T g;
                const T s = gt_score<T>(elv, erv, slope, bias, bv, &g);
                gt_entry<T, DROP>(s, g, rp, lse, delta, false, ((km >> mine) & 1u) != 0, a.drop.rs, &prob, &ds, &dz);
                if (a.ds_out != nullptr && lir < UNR)
                {
                    const int p = p0 + mine;
                    a.ds_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = ds;
                }
            }
#pragma unroll
            for (int q = 0; q < UNR; q++) sum = sum + __shfl(dz, q, LPR);
        }
    }
    if (lir == 0) *delp = sum;
}

// ---- backward, column side: d_er and dV over a handle of A^T (the unit is (column c, head h)) ----------------------------------
template <typename T, int LPR, int PV, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gat_bwd_col_kernel(const GatBwdColArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr int CV  = rg_ch<PV, VEC>;
    const int lir = threadIdx.x % LPR;
    const int64_t u = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR;
    const int64_t nh = a.heads;
    if (u >= (int64_t) a.nrow * nh) return;
    const int row = (int) (u / nh);
    const int64_t h = u % nh;
    int pb = a.rowptr[row];
    const int pe = a.rowptr[row + 1];
    if constexpr (LPR == 64) pb = __builtin_amdgcn_readfirstlane(pb);
    const int nv = a.nv;
    const int64_t crow = a.rowmap ? a.rowmap[row] : row;
    const T ninf = rg_ninf<T>();
    const int64_t hv = h * nv;
    T *const dvrow = a.dV + crow * a.lddV + hv;
    T *const derp = a.d_er + crow * a.ldd_er + h;

    T accV[PV][VW];
#pragma unroll
    for (int v = 0; v < PV; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accV[v][w] = (T) 0;
    if (pb >= pe)                                       // a column no row names: +0; its er and V row are not read
    {
        rg_store_row<T, LPR, PV, VEC>(accV, dvrow, nv, lir);
        if (lir == 0) *derp = (T) 0;
        return;
    }
    // er[c][h] and V[c]_h whole, before anything of this unit is written (dV == V)
    T xv[PV][VW];
    rg_load_row<T, LPR, PV, VEC>(xv, a.V + crow * a.ldV + hv, nv, lir);
    const T erv = a.er[crow * a.lder + h];
    const T slope = a.slope;
    const bool bias = a.val != nullptr;
    const int again = rg_again<VW>(a.nv);
    T sum = (T) 0;                                      // d_er: the same bits in every lane

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits; the entry's row of A is r, this unit's row c)
        if constexpr (DROP) km = rg_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) c, (uint32_t) crow, (uint32_t) h, lir);
        for (int j = 0; j < cnt; j += UNR)
        {
            const int mine = j + (lir & 7);
            const int mcl = min(mine, cnt - 1);
            const int64_t im = __shfl(c, mcl, LPR);     // the row of A of this lane's entry
            const T elv = a.el[im * a.ldel + h];
            const T lse = a.lse[im * nh + h];
            const T dl = a.delta[im * nh + h];
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *drow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++)
            {
                const int ij = rg_bcast_i<LPR>(c, min(j + q, cnt - 1));
                drow[q] = a.dO + (int64_t) ij * a.lddO + hv;
            }
            T pp[UNR];
            gt_dots<T, LPR, PV, VEC>(pp, xv, drow, nv, lir);
            const T rp = rg_reduce8<T, LPR>(pp, lir);
            T prob = (T) 0, ds = (T) 0, dz = (T) 0;
            if (mine < cnt)
            {
                T g;
                const T s = gt_score<T>(elv, erv, slope, bias, bv, &g);
                gt_entry<T, DROP>(s, g, rp, lse, dl, lse == ninf, ((km >> mine) & 1u) != 0, a.drop.rs, &prob, &ds, &dz);
            }
            T cp[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++)
            {
                sum = sum + __shfl(dz, q, LPR);
                cp[q] = __shfl(prob, q, LPR);
            }
            rg_static_for<0, PV, (VEC ? 2 : 1)>([&](auto kc) {
                constexpr int K = decltype(kc)::value;
                T dv[UNR][CV][VW];
                rg_load8<T, LPR, CV, VEC>(dv, drow, K, nv, lir, again);        // (cache hits: the dots read these rows)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int v = 0; v < CV; v++)
#pragma unroll
                        for (int w = 0; w < VW; w++) accV[K + v][w] = fma(cp[q], dv[q][v][w], accV[K + v][w]);
                if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);
            });
        }
    }
    rg_store_row<T, LPR, PV, VEC>(accV, dvrow, nv, lir);
    if (lir == 0) *derp = sum;
}


// ---- launchers ----------------------------------------------------------------------------------------------------------------
// Per argument list: which pointers and which leading dimensions decide VEC (nv % VW == 0 keeps every head's slice on a 16-byte
// boundary; the leading dimension of a source that is NULL is not read), and the kernel family; rg_launch does the rest.
template <typename T, int LPR, int PV>
static hipError_t launch_gat(const GatArgs<T> &a, hipStream_t s)
{
    return rg_launch<T, LPR>(a, s, {a.V0, a.V1, a.O}, {a.nv, a.ldO, a.V0 ? a.ldV0 : 0, a.V1 ? a.ldV1 : 0},
                             [](auto v, auto d) { return gat_fwd_kernel<T, LPR, PV, decltype(v)::value, decltype(d)::value>; });
}
template <typename T, int LPR, int PV>
static hipError_t launch_gat(const GatBwdRowArgs<T> &a, hipStream_t s)
{
    return rg_launch<T, LPR>(a, s, {a.V0, a.V1, a.O, a.dO}, {a.nv, a.ldO, a.lddO, a.V0 ? a.ldV0 : 0, a.V1 ? a.ldV1 : 0},
                             [](auto v, auto d) { return gat_bwd_row_kernel<T, LPR, PV, decltype(v)::value, decltype(d)::value>; });
}
template <typename T, int LPR, int PV>
static hipError_t launch_gat(const GatBwdColArgs<T> &a, hipStream_t s)
{
    return rg_launch<T, LPR>(a, s, {a.V, a.dO, a.dV}, {a.nv, a.ldV, a.lddO, a.lddV},
                             [](auto v, auto d) { return gat_bwd_col_kernel<T, LPR, PV, decltype(v)::value, decltype(d)::value>; });
}

// The instance, from (dtype, nv) alone (the rule is stated at the top of this file)
template <typename T>
static hipError_t gat_fwd(const GatArgs<T> &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T);
    if (a.nrow <= 0) return hipSuccess;
    if (a.nv <= 8 * W)   return launch_gat<T, 8, 1>(a, s);
    if (a.nv <= 16 * W)  return launch_gat<T, 16, 1>(a, s);
    if (a.nv <= 32 * W)  return launch_gat<T, 32, 1>(a, s);
    if (a.nv <= 64 * W)  return launch_gat<T, 64, 1>(a, s);
    if (a.nv <= 128 * W) return launch_gat<T, 64, 2>(a, s);
    if (a.nv <= 256 * W) return launch_gat<T, 64, 4>(a, s);
    return launch_gat<T, 64, 8>(a, s);
}
template <typename T, class Args>
static hipError_t gat_bwd(const Args &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T), CAP = ATTN_BWD_MAX_PIECES * 64 * W;
    if (a.nv > CAP) return hipErrorInvalidValue;         // (the entry points refuse these before they come here)
    if (a.nrow <= 0) return hipSuccess;
    if (a.nv <= 8 * W)   return launch_gat<T, 8, 1>(a, s);
    if (a.nv <= 16 * W)  return launch_gat<T, 16, 1>(a, s);
    if (a.nv <= 32 * W)  return launch_gat<T, 32, 1>(a, s);
    if (a.nv <= 64 * W)  return launch_gat<T, 64, 1>(a, s);
    if (a.nv <= 128 * W) return launch_gat<T, 64, 2>(a, s);
    return launch_gat<T, 64, 4>(a, s);
}

hipError_t gat_attention_rm(const GatArgs<double> &a, hipStream_t s) { return gat_fwd<double>(a, s); }
hipError_t gat_attention_rm(const GatArgs<float> &a, hipStream_t s) { return gat_fwd<float>(a, s); }
hipError_t gat_attention_bwd_row(const GatBwdRowArgs<double> &a, hipStream_t s) { return gat_bwd<double>(a, s); }
hipError_t gat_attention_bwd_row(const GatBwdRowArgs<float> &a, hipStream_t s) { return gat_bwd<float>(a, s); }
hipError_t gat_attention_bwd_col(const GatBwdColArgs<double> &a, hipStream_t s) { return gat_bwd<double>(a, s); }
hipError_t gat_attention_bwd_col(const GatBwdColArgs<float> &a, hipStream_t s) { return gat_bwd<float>(a, s); }

}  // namespace crp
