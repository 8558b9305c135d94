// gatv2_kernels.hip -- fused GATv2 attention over A's pattern for gfx950 (MI355X, wave64), fp64 and fp32, forward and backward.
// For every row i, head h and entry p = (i, c_p), p in the handle's CSR order:
//     z_pj = XT[i]_h[j] + XS[c_p]_h[j]     r_pj = z_pj > 0 ? z_pj : slope * z_pj     s_p = sum_j a_h[j] r_pj (bias: + A's value of p)
//     O[i]_h = sum_p softmax_p(s) * XS[c_p]_h
// -- the LeakyReLU INSIDE the dot with a, where gat_kernels.hip has it outside a sum of two scalars.  The gathered row XS[c] is the
// score operand and the value operand: one gather per entry.  From the scores on everything is attention_kernels.hip's: the batches
// of 8, the online softmax, lse / p_out, the (row, head) units and the column-to-lane assignment.  No atomics, no LDS, no partial
// result in memory.  The pieces, the row loads and stores, the walk over a batch's 8 rows (rg_walk8), the batch's butterfly
// (rg_reduce8), the keep bits and the launcher are row_group.h's (rg_), one definition for this file, gat_kernels.hip and the
// attention's two; g2_ marks what is this score's own.
//
// OPERANDS.  heads = H >= 1 heads of nv columns each lie side by side in XT / XS / a / O / dO / dXT / da_part / dXS: head h owns
// columns [h nv, (h + 1) nv).  XT is (rows of O, H nv), read through the row map like Q; XS0 / XS1 are the two sources of the column
// code (c >= 0 -> row c of XS0, c < 0 -> row ~c of XS1); a is H nv contiguous elements.  lse, delta are (rows, H) row-major; p_out,
// ds_out are (nnz, H): entry (pos, h) at pos * H + h with pos = out_pos[p], or p.  val[p] (bias) is shared by the heads.
//
// INSTANCE.  W = elements per 16 bytes, G(n) = 8, 16, 32, 64 for n <= 8 W, 16 W, 32 W, else (the SDDMM's group for a width n):
// LPR = G(nv) lanes own the unit u = row * H + h (consecutive groups hold consecutive heads of a row).  Column j of the head's
// slice belongs to lane (j / W) % LPR, piece (j / W) / LPR of that lane; a lane keeps P = 1, 2 or 4 pieces of XT[i]_h (column side:
// XS[c]_h), a_h and as_h = fl(a_h slope) for the unit, so nv <= 4 * 64 * W in both directions; wider heads are refused by the
// launchers.  Operands that cannot be accessed in 16-byte pieces are accessed element by element in the SAME assignment.
//
// SCORES.  Per batch of 8 entries a lane forms its part of the 8 dots from its pieces of the 8 gathered rows -- z and r rounded one
// by one (g2_lrelu compiles with contraction off, so slope * z never meets the product with a in one instruction), then
// part = fma(a_j, r_j, part) in ascending j from +0 -- and the SDDMM's reduce-scatter butterfly (rg_reduce8) leaves the dot of
// entry u in lane u of every block of 8 lanes: the bits of crp_sddmm_csr_* for (dtype, nv) on the rows a and r.  s = dot (bias:
// + val, one rounding).
//
// LOADS.  Forward, P = 1: the 8 row pieces loaded for the dots stay in registers and serve the accumulator FMAs.  Backward, P = 1
// in fp64: what the second trip over a batch needs stays in registers -- row side r and the branch bits, column side the dO
// pieces and the branch bits -- and nothing is formed or fetched twice.  In fp32 the same 32 + 32 registers take the row side
// from 4 waves per SIMD to 2, and the backward measured 10 - 17 % slower with them than without, so fp32 does
// as P = 2 and 4 do in both directions: holding 8 rows x P pieces across the exponentials would spill, so the rows are read again
// through rg_again's opaque zero -- cache hits, the dots read these lines a moment ago -- and z, the branch and r are formed
// again, with the same bits.  Per step at most 8 x 2 pieces by 16-byte accesses (8 x 1 by elements) are in flight, issued ahead
// of the step's FMAs.
//
// FIXED ORDER.  Forward: attention_kernels.hip's, verbatim, from s on; O, lse and p_out are bit for bit what that file's order
// gives for these scores and (dtype, nv), with XS in the place of V.  Backward: p = exp(s - lse), dP = < dO[i]_h, XS[c]_h > and
// D = < dO[i]_h, O[i]_h > as the SDDMM forms a dot for (dtype, nv), dS = p * (dP - D) (p == 0: +0), ag_pj = z_pj > 0 ? a_j : as_j.
// Row side (a handle of A): delta = D, dXT[i]_h[j] = fma(dS_p, ag_pj, acc) and da_part[i]_h[j] = fma(dS_p, r_pj, acc), both from +0
// in ascending p, ds_out = dS.  Column side (a handle of A^T): accZ = fma(dS, ag, accZ) and accV = fma(p, dO[i][j], accV) from +0
// in that handle's CSR order, dXS[c]_h = accZ + accV, one addition.  s, p, dP and dS have the same bits on both sides.  Slots of a
// last partial batch count as s = -inf (forward) and p = dS = +0 (backward) with the row's last entry's operand rows.
//
// SPECIAL CASES.  attention_kernels.hip's and attention_bwd_kernels.hip's: an empty row writes +0 and lse = -inf for every head; a
// one-entry row gives O = XS[c]; s = -inf (a bias value) is a masked edge; an all-masked row gives zeros; NaN or +inf among a
// row's scores leaves that row's outputs unspecified.  XS is taken to be finite.  Rows with lse = -inf give +0 everywhere in the
// backward; delta is still written.
//
// ALIASING.  Column side: dXS == XS (exactly) is legal, a group reads its slice of XS[c] whole before it writes it and no other
// unit reads it.  Nothing else.
//
// DROPOUT (the DROP instances; a.drop, dropout.h).  k_p = the keep bit of (row of O, column code, head).  Forward:
// scores, batches, m, f, e_u and l are the plain call's -- the softmax runs over all edges -- and only the accumulator changes:
// acc = fma(k_u ? e_u : +0, XS[c_u][j], acc), O = fl(fl(acc / l) rs); lse and p_out keep the plain call's bits.  Backward: p, s
// and D = < dO, O > (O is the dropped O) as above, dP' = k ? fl(dP rs) : +0, dS = p (dP' - D), and accV takes the weight
// w = k ? fl(p rs) : +0 in the place of p.  The two products with rs are roundings of their own (rg_mul).  The lane that loads the
// column code of its own entry of a chunk draws that entry's bit, one ballot hands the chunk's bits to the group, and a batch takes
// its 8 bits from that word.  DROP = false compiles to the code without any of this.
#include "row_group.h"

namespace crp {

// r = lrelu(xt + xs): two statements, two roundings; the caller's fma(a, r, .) is a third.  hipcc contracts across statements by
// default; here it may not.  *pos: z > 0, which chooses a or as in the backward.
template <typename T>
__device__ __forceinline__ T g2_lrelu(const T xt, const T xs, const T slope, bool *pos)
{
#pragma clang fp contract(off)
    const T z = xt + xs;
    const T sz = slope * z;
    *pos = z > (T) 0;
    return *pos ? z : sz;
}
// s = dot (+ val), and accZ + accV: additions of their own
template <typename T>
__device__ __forceinline__ T g2_add(const T x, const T y)
{
#pragma clang fp contract(off)
    const T r = x + y;
    return r;
}

// where the row of column code c lies, advanced to the head's slice
template <typename T>
__device__ __forceinline__ const T *g2_xs(const int c, const int64_t hv, const T *XS0, const int64_t ld0, const T *XS1, const int64_t ld1)
{
    return ((c >= 0) ? (XS0 + (int64_t) c * ld0) : (XS1 + (int64_t) (~c) * ld1)) + hv;
}

// p and dS of one entry from its score and dP (see FIXED ORDER); dead: lse == -inf.  DROP: dP counts as dP' = keep ? fl(dP rs) : +0,
// and *pp is the value-side weight w = keep ? fl(p rs) : +0 (see DROPOUT)
template <typename T, bool DROP>
__device__ __forceinline__ void g2_entry(const T s, T dp, const T lse, const T delta, const bool dead, const bool keep, const T rs, T *pp,
                                         T *ds)
{
    const T e = dead ? (T) 0 : rg_exp(s - lse);
    if constexpr (DROP)
    {
        dp = keep ? rg_mul<T>(dp, rs) : (T) 0;
        *pp = keep ? rg_mul<T>(e, rs) : (T) 0;
    }
    else *pp = e;
    *ds = (e == (T) 0) ? (T) 0 : e * (dp - delta);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// LPR lanes per unit (row, head); P pieces of XT, a and the accumulator per lane.  VEC: 16-byte accesses; else elements.
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_fwd_kernel(const Gatv2Args<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr bool HOLD = P == 1;                       // the rows of a batch stay in registers from the dots to the accumulator
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
    const int64_t orow = a.rowmap ? a.rowmap[row] : row;        // rowmap: the XT and O row of every row of a row-subset matrix
    const T ninf = rg_ninf<T>();
    const int64_t hv = h * nv;                          // the head's first column
    const int64_t srow = orow * nh + h;                 // the unit's entry of lse
    T *const orp = a.O + orow * a.ldO + hv;

    T acc[P][VW];
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) acc[v][w] = (T) 0;
    if (pb >= pe)                                       // an empty row: zeros; XT is not read
    {
        rg_store_row<T, LPR, P, VEC>(acc, orp, nv, lir);
        if (a.lse != nullptr && lir == 0) a.lse[srow] = ninf;
        return;
    }
    T xt[P][VW], av[P][VW];                             // kept for the row
    rg_load_row<T, LPR, P, VEC>(xt, a.XT + orow * a.ldXT + hv, nv, lir);
    rg_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
    const T slope = a.slope;
    const bool bias = a.val != nullptr;
    const int again = rg_again<VW>(a.nv);
    T m = ninf, l = (T) 0;

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits)
        if constexpr (DROP) km = rg_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) orow, (uint32_t) c, (uint32_t) h, lir);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose score counts as -inf
            const int mine = j + (lir & 7);
            const int mcl = min(mine, cnt - 1);
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *xrow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) xrow[q] = g2_xs<T>(rg_bcast_i<LPR>(c, min(j + q, cnt - 1)), hv, a.XS0, a.ldXS0, a.XS1, a.ldXS1);

            T part[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) part[q] = (T) 0;
            T hold[UNR][1][VW];                         // (P == 1: the batch's pieces; else not used)
            if constexpr (HOLD)
            {
                rg_load8<T, LPR, 1, VEC>(hold, xrow, 0, nv, lir);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++)
                        if (lir * VW + w < nv)
                        {
                            bool pos;
                            const T r = g2_lrelu<T>(xt[0][w], hold[q][0][w], slope, &pos);
                            part[q] = fma(av[0][w], r, part[q]);
                        }
            }
            else
            {
                rg_walk8<T, LPR, P, VEC>(xrow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                        part[q] = fma(av[v][w], r, part[q]);
                    }
                });
            }
            const T dot = rg_reduce8<T, LPR>(part, lir);

            // every lane holds the score of entry (lir & 7) of the batch
            T s = ninf;
            if (mine < cnt)
            {
                s = bias ? g2_add<T>(dot, bv) : dot;
                if (a.p_out != nullptr && lir < UNR)
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
            if (mn != ninf)                             // (else every entry so far is masked: l and acc stay 0)
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
            if constexpr (DROP)                         // l has every edge; the accumulator takes the kept ones
            {
                const unsigned kb = (unsigned) (km >> j);
#pragma unroll
                for (int q = 0; q < UNR; q++) eu[q] = ((kb >> q) & 1u) ? eu[q] : (T) 0;
            }
#pragma unroll
            for (int v = 0; v < P; v++)
#pragma unroll
                for (int w = 0; w < VW; w++) acc[v][w] = acc[v][w] * f;
            if constexpr (HOLD)
            {
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++) acc[0][w] = fma(eu[q], hold[q][0][w], acc[0][w]);
            }
            else
            {
                // (cache hits: the dots read these rows)
                rg_walk8<T, LPR, P, VEC>(xrow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    acc[v][w] = fma(eu[q], y, acc[v][w]);
                });
            }
        }
    }

    const bool masked = m == ninf;                      // every entry masked: zeros, not 0 / 0
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++)
        {
            acc[v][w] = masked ? (T) 0 : acc[v][w] / l;
            if constexpr (DROP) acc[v][w] = rg_mul<T>(acc[v][w], a.drop.rs);
        }
    rg_store_row<T, LPR, P, VEC>(acc, orp, nv, lir);
    if (a.lse != nullptr && lir == 0) a.lse[srow] = masked ? ninf : m + rg_log(l);
    if (a.p_out != nullptr && lir < UNR)
        for (int p = pb + lir; p < pe; p += UNR)        // this lane's own stores
        {
            const int64_t pos = (int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h;
            const T sv = a.p_out[pos];
            a.p_out[pos] = masked ? (T) 0 : rg_exp(sv - m) / l;
        }
}

// ---- backward, row side: delta, dXT, da_part and ds_out over a handle of A ----------------------------------------------------------
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_bwd_row_kernel(const Gatv2BwdRowArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr bool HOLD = P == 1 && sizeof(T) == 8;     // what the second trip over a batch needs stays in registers (see LOADS)
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
    T xd[P][VW];
    rg_load_row<T, LPR, P, VEC>(xd, a.dO + orow * a.lddO + hv, nv, lir);
    T delta = (T) 0;
    {
        T xo[P][VW];
        rg_load_row<T, LPR, P, VEC>(xo, a.O + orow * a.ldO + hv, nv, lir);
#pragma unroll
        for (int v = 0; v < P; v++)
#pragma unroll
            for (int w = 0; w < VW; w++)
                if ((v * LPR + lir) * VW + w < nv) delta = fma(xd[v][w], xo[v][w], delta);
#pragma unroll
        for (int mask = 1; mask < LPR; mask <<= 1) delta = delta + __shfl_xor(delta, mask, LPR);
    }
    if (lir == 0) a.delta[srow] = delta;

    T *const dxrow = a.dXT + orow * a.lddXT + hv;
    T *const darow = a.da_part + orow * a.ldda + hv;
    T dxt[P][VW], dap[P][VW];
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) dxt[v][w] = dap[v][w] = (T) 0;
    const T lse = a.lse[srow];
    if (pb >= pe || lse == ninf)                        // an empty or all-masked row: +0 everywhere; XT is not read
    {
        rg_store_row<T, LPR, P, VEC>(dxt, dxrow, nv, lir);
        rg_store_row<T, LPR, P, VEC>(dap, darow, nv, lir);
        if (a.ds_out != nullptr)
            for (int p = pb + lir; p < pe; p += LPR) a.ds_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = (T) 0;
        return;
    }
    const T slope = a.slope;
    T xt[P][VW], av[P][VW], as[P][VW];
    rg_load_row<T, LPR, P, VEC>(xt, a.XT + orow * a.ldXT + hv, nv, lir);
    rg_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) as[v][w] = rg_mul<T>(av[v][w], slope);
    const bool bias = a.val != nullptr;
    const int again = rg_again<VW>(a.nv);

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
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *xrow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) xrow[q] = g2_xs<T>(rg_bcast_i<LPR>(c, min(j + q, cnt - 1)), hv, a.XS0, a.ldXS0, a.XS1, a.ldXS1);

            // one trip serves both dots: the score's and dP's
            T sp[UNR], dp[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) sp[q] = dp[q] = (T) 0;
            T rr[UNR][VW];                              // (P == 1: the batch's r and its branches, bit q VW + w of posm; else not used)
            unsigned posm = 0;
            if constexpr (HOLD)
            {
                T y[UNR][1][VW];
                rg_load8<T, LPR, 1, VEC>(y, xrow, 0, nv, lir);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(xt[0][w], y[q][0][w], slope, &pos);
                        rr[q][w] = r;
                        posm |= (unsigned) pos << (q * VW + w);
                        if (lir * VW + w < nv)
                        {
                            sp[q] = fma(av[0][w], r, sp[q]);
                            dp[q] = fma(xd[0][w], y[q][0][w], dp[q]);
                        }
                    }
            }
            else
            {
                rg_walk8<T, LPR, P, VEC>(xrow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                        sp[q] = fma(av[v][w], r, sp[q]);
                        dp[q] = fma(xd[v][w], y, dp[q]);
                    }
                });
            }
            const T dot = rg_reduce8<T, LPR>(sp, lir);
            const T rp = rg_reduce8<T, LPR>(dp, lir);
            // every lane holds the score and dP of entry (lir & 7) of the batch
            T prob = (T) 0, ds = (T) 0;
            if (mine < cnt)
            {
                const T s = bias ? g2_add<T>(dot, bv) : dot;
                g2_entry<T, DROP>(s, rp, lse, delta, false, ((km >> mine) & 1u) != 0, a.drop.rs, &prob, &ds);
                if (a.ds_out != nullptr && lir < UNR)
                {
                    const int p = p0 + mine;
                    a.ds_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = ds;
                }
            }
            T dsu[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) dsu[q] = __shfl(ds, q, LPR);
            if constexpr (HOLD)
            {
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++)
                    {
                        const T ag = ((posm >> (q * VW + w)) & 1u) ? av[0][w] : as[0][w];
                        dxt[0][w] = fma(dsu[q], ag, dxt[0][w]);
                        dap[0][w] = fma(dsu[q], rr[q][w], dap[0][w]);
                    }
            }
            else
            {
                // (cache hits: the dots read these rows)
                rg_walk8<T, LPR, P, VEC>(xrow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    bool pos;
                    const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                    const T ag = pos ? av[v][w] : as[v][w];
                    dxt[v][w] = fma(dsu[q], ag, dxt[v][w]);
                    dap[v][w] = fma(dsu[q], r, dap[v][w]);
                });
            }
        }
    }
    rg_store_row<T, LPR, P, VEC>(dxt, dxrow, nv, lir);
    rg_store_row<T, LPR, P, VEC>(dap, darow, nv, lir);
}

// ---- backward, column side: dXS over a handle of A^T (the unit is (column c, head h)) ------------------------------------------
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_bwd_col_kernel(const Gatv2BwdColArgs<T> a)
{
    constexpr int VW  = Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = RG_UNR;
    constexpr bool HOLD = P == 1 && sizeof(T) == 8;     // what the second trip over a batch needs stays in registers (see LOADS)
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
    T *const dxrow = a.dXS + crow * a.lddXS + hv;

    T accZ[P][VW], accV[P][VW];
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accZ[v][w] = accV[v][w] = (T) 0;
    if (pb >= pe)                                       // a column no row names: +0; its XS row is not read
    {
        rg_store_row<T, LPR, P, VEC>(accZ, dxrow, nv, lir);
        return;
    }
    // XS[c]_h whole, before anything of this unit is written (dXS == XS)
    const T slope = a.slope;
    T xs[P][VW], av[P][VW], as[P][VW];
    rg_load_row<T, LPR, P, VEC>(xs, a.XS + crow * a.ldXS + hv, nv, lir);
    rg_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) as[v][w] = rg_mul<T>(av[v][w], slope);
    const bool bias = a.val != nullptr;
    const int again = rg_again<VW>(a.nv);

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
            const T lse = a.lse[im * nh + h];
            const T dl = a.delta[im * nh + h];
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *trow[UNR], *drow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++)
            {
                const int ij = rg_bcast_i<LPR>(c, min(j + q, cnt - 1));
                trow[q] = a.XT + (int64_t) ij * a.ldXT + hv;
                drow[q] = a.dO + (int64_t) ij * a.lddO + hv;
            }
            T sp[UNR], dp[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) sp[q] = dp[q] = (T) 0;
            T dy[UNR][1][VW];                           // (P == 1: the batch's dO pieces and its branches; else not used)
            unsigned posm = 0;
            if constexpr (HOLD)
            {
                T ty[UNR][1][VW];
                rg_load8<T, LPR, 1, VEC>(ty, trow, 0, nv, lir);
                rg_load8<T, LPR, 1, VEC>(dy, drow, 0, nv, lir);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(ty[q][0][w], xs[0][w], slope, &pos);
                        posm |= (unsigned) pos << (q * VW + w);
                        if (lir * VW + w < nv)
                        {
                            sp[q] = fma(av[0][w], r, sp[q]);
                            dp[q] = fma(dy[q][0][w], xs[0][w], dp[q]);
                        }
                    }
            }
            else
            {
                rg_walk8<T, LPR, P, VEC>(trow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(y, xs[v][w], slope, &pos);
                        sp[q] = fma(av[v][w], r, sp[q]);
                    }
                });
                rg_walk8<T, LPR, P, VEC>(drow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in) dp[q] = fma(y, xs[v][w], dp[q]);
                });
            }
            const T dot = rg_reduce8<T, LPR>(sp, lir);
            const T rp = rg_reduce8<T, LPR>(dp, lir);
            T prob = (T) 0, ds = (T) 0;
            if (mine < cnt)
            {
                const T s = bias ? g2_add<T>(dot, bv) : dot;
                g2_entry<T, DROP>(s, rp, lse, dl, lse == ninf, ((km >> mine) & 1u) != 0, a.drop.rs, &prob, &ds);
            }
            T dsu[UNR], pu[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++)
            {
                dsu[q] = __shfl(ds, q, LPR);
                pu[q] = __shfl(prob, q, LPR);
            }
            if constexpr (HOLD)
            {
#pragma unroll
                for (int q = 0; q < UNR; q++)
#pragma unroll
                    for (int w = 0; w < VW; w++)
                    {
                        const T ag = ((posm >> (q * VW + w)) & 1u) ? av[0][w] : as[0][w];
                        accZ[0][w] = fma(dsu[q], ag, accZ[0][w]);
                        accV[0][w] = fma(pu[q], dy[q][0][w], accV[0][w]);
                    }
            }
            else
            {
                // (cache hits: the dots read these rows)
                rg_walk8<T, LPR, P, VEC>(trow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    bool pos;
                    (void) g2_lrelu<T>(y, xs[v][w], slope, &pos);
                    const T ag = pos ? av[v][w] : as[v][w];
                    accZ[v][w] = fma(dsu[q], ag, accZ[v][w]);
                });
                rg_walk8<T, LPR, P, VEC>(drow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    accV[v][w] = fma(pu[q], y, accV[v][w]);
                });
            }
        }
    }
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accZ[v][w] = g2_add<T>(accZ[v][w], accV[v][w]);
    rg_store_row<T, LPR, P, VEC>(accZ, dxrow, nv, lir);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
// Per argument list: which pointers and which leading dimensions decide VEC (nv % VW == 0 keeps every head's slice on a 16-byte
// boundary; the leading dimension of a source that is NULL is not read), and the kernel family; rg_launch does the rest.
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2Args<T> &a, hipStream_t s)
{
    return rg_launch<T, LPR>(a, s, {a.XT, a.XS0, a.XS1, a.av, a.O}, {a.nv, a.ldXT, a.ldO, a.XS0 ? a.ldXS0 : 0, a.XS1 ? a.ldXS1 : 0},
                             [](auto v, auto d) { return gatv2_fwd_kernel<T, LPR, P, decltype(v)::value, decltype(d)::value>; });
}
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2BwdRowArgs<T> &a, hipStream_t s)
{
    return rg_launch<T, LPR>(a, s, {a.XT, a.XS0, a.XS1, a.av, a.O, a.dO, a.dXT, a.da_part},
                             {a.nv, a.ldXT, a.ldO, a.lddO, a.lddXT, a.ldda, a.XS0 ? a.ldXS0 : 0, a.XS1 ? a.ldXS1 : 0},
                             [](auto v, auto d) { return gatv2_bwd_row_kernel<T, LPR, P, decltype(v)::value, decltype(d)::value>; });
}
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2BwdColArgs<T> &a, hipStream_t s)
{
    // (XT and dO are not read when the handle has no nonzero, and may then be NULL)
    return rg_launch<T, LPR>(a, s, {a.XS, a.XT, a.av, a.dO, a.dXS}, {a.nv, a.ldXS, a.XT ? a.ldXT : 0, a.dO ? a.lddO : 0, a.lddXS},
                             [](auto v, auto d) { return gatv2_bwd_col_kernel<T, LPR, P, decltype(v)::value, decltype(d)::value>; });
}

// The instance, from (dtype, nv) alone (the rule is stated at the top of this file)
template <typename T, class Args>
static hipError_t gatv2_any(const Args &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T), CAP = ATTN_BWD_MAX_PIECES * 64 * W;
    if (a.nv > CAP) return hipErrorInvalidValue;         // (the entry points refuse these before they come here)
    if (a.nrow <= 0) return hipSuccess;
    if (a.nv <= 8 * W)   return launch_gatv2<T, 8, 1>(a, s);
    if (a.nv <= 16 * W)  return launch_gatv2<T, 16, 1>(a, s);
    if (a.nv <= 32 * W)  return launch_gatv2<T, 32, 1>(a, s);
    if (a.nv <= 64 * W)  return launch_gatv2<T, 64, 1>(a, s);
    if (a.nv <= 128 * W) return launch_gatv2<T, 64, 2>(a, s);
    return launch_gatv2<T, 64, 4>(a, s);
}

hipError_t gatv2_attention_rm(const Gatv2Args<double> &a, hipStream_t s) { return gatv2_any<double>(a, s); }
hipError_t gatv2_attention_rm(const Gatv2Args<float> &a, hipStream_t s) { return gatv2_any<float>(a, s); }
hipError_t gatv2_attention_bwd_row(const Gatv2BwdRowArgs<double> &a, hipStream_t s) { return gatv2_any<double>(a, s); }
hipError_t gatv2_attention_bwd_row(const Gatv2BwdRowArgs<float> &a, hipStream_t s) { return gatv2_any<float>(a, s); }
hipError_t gatv2_attention_bwd_col(const Gatv2BwdColArgs<double> &a, hipStream_t s) { return gatv2_any<double>(a, s); }
hipError_t gatv2_attention_bwd_col(const Gatv2BwdColArgs<float> &a, hipStream_t s) { return gatv2_any<float>(a, s); }

}  // namespace crp
