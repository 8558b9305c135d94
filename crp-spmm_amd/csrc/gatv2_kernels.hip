// gatv2_kernels.hip -- fused GATv2 attention over A's pattern for gfx950 (MI355X, wave64), fp64 and fp32, forward and backward.
// For every row i, head h and entry p = (i, c_p), p in the handle's CSR order:
//     z_pj = XT[i]_h[j] + XS[c_p]_h[j]     r_pj = z_pj > 0 ? z_pj : slope * z_pj     s_p = sum_j a_h[j] r_pj (bias: + A's value of p)
//     O[i]_h = sum_p softmax_p(s) * XS[c_p]_h
// -- the LeakyReLU INSIDE the dot with a, where gat_kernels.hip has it outside a sum of two scalars.  The gathered row XS[c] is the
// score operand and the value operand: one gather per entry.  From the scores on everything is attention_kernels.hip's: the batches
// of 8, the online softmax, lse / p_out, the (row, head) units and the column-to-lane assignment.  No atomics, no LDS, no partial
// result in memory.
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
// part = fma(a_j, r_j, part) in ascending j from +0 -- and the SDDMM's reduce-scatter butterfly leaves the dot of entry u in lane u
// of every block of 8 lanes: the bits of crp_sddmm_csr_* for (dtype, nv) on the rows a and r.  s = dot (bias: + val, one rounding).
//
// LOADS.  Forward, P = 1: the 8 row pieces loaded for the dots stay in registers and serve the accumulator FMAs.  Backward, P = 1
// in fp64: what the second trip over a batch needs stays in registers -- row side r and the branch bits, column side the dO
// pieces and the branch bits -- and nothing is formed or fetched twice.  In fp32 the same 32 + 32 registers take the row side
// from 4 waves per SIMD to 2, and the backward measured 10 - 17 % slower with them than without, so fp32 does
// as P = 2 and 4 do in both directions: holding 8 rows x P pieces across the exponentials would spill, so the rows are read again
// through g2_again's opaque zero -- cache hits, the dots read these lines a moment ago -- and z, the branch and r are formed
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
// w = k ? fl(p rs) : +0 in the place of p.  The two products with rs are roundings of their own (g2_mul).  The lane that loads the
// column code of its own entry of a chunk draws that entry's bit, one ballot hands the chunk's bits to the group, and a batch takes
// its 8 bits from that word.  DROP = false compiles to the code without any of this.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <type_traits>
#include "kernels.h"

namespace crp {

constexpr int G2_UNR = 8;

template <typename T> struct G2Piece;
template <> struct G2Piece<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int VW = 2; };
template <> struct G2Piece<float>  { typedef float type __attribute__((ext_vector_type(4))); static constexpr int VW = 4; };

__device__ __forceinline__ double g2_exp(double x) { return exp(x); }
__device__ __forceinline__ float  g2_exp(float x) { return expf(x); }
__device__ __forceinline__ double g2_log(double x) { return log(x); }
__device__ __forceinline__ float  g2_log(float x) { return logf(x); }
template <typename T> __device__ __forceinline__ T g2_ninf() { return -__builtin_huge_val(); }
template <> __device__ __forceinline__ float g2_ninf<float>() { return -__builtin_huge_valf(); }

template <int LPR>
__device__ __forceinline__ int g2_bcast_i(int v, int j)
{
    if constexpr (LPR == 64) return __builtin_amdgcn_readlane(v, j);
    else return __shfl(v, j, LPR);
}

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
// as = a * slope, rounded before it is used in anything; the products with rs of the DROP instances likewise
template <typename T>
__device__ __forceinline__ T g2_mul(const T x, const T y)
{
#pragma clang fp contract(off)
    const T r = x * y;
    return r;
}
// s = dot (+ val), and accZ + accV: additions of their own
template <typename T>
__device__ __forceinline__ T g2_add(const T x, const T y)
{
#pragma clang fp contract(off)
    const T r = x + y;
    return r;
}

// The keep bits of a chunk of LPR entries: the lane that holds entry `lir` of the chunk (live: it has one) draws the bit of
// (r, c, h); bit e of the result is entry e's, the same word in every lane of the group.  Every lane of a group is active here
// together (the chunk loop's bounds are the group's); lanes of other groups that are not contribute 0 to bits this group drops.
template <typename T, int LPR>
__device__ __forceinline__ unsigned long long g2_keep_bits(const DropArgs<T> &d, const bool live, const uint32_t r, const uint32_t c,
                                                           const uint32_t h, const int lir)
{
    const bool k = live && dropout_keep(d.seed_lo, d.seed_hi, r, c, h, d.thr);
    const unsigned long long all = __ballot(k);
    if constexpr (LPR == 64) return all;
    else return all >> ((threadIdx.x & 63u) - (unsigned) lir);
}

// pieces per lane and row of one load step: two by 16-byte accesses, one by elements, so that no instance spills
template <int P, bool VEC> constexpr int g2_ch = VEC ? (P < 2 ? P : 2) : 1;

template <int K0, int END, int STEP, class F>
__device__ __forceinline__ void g2_static_for(F &&f)
{
    if constexpr (K0 < END)
    {
        f(std::integral_constant<int, K0>{});
        g2_static_for<K0 + STEP, END, STEP>(f);
    }
}

// The zero of g2_load8's `again`: opaque as long as nothing lets the compiler prove nv >= 0, so that the second read of a batch's
// rows stays a load of its own (a cache hit) instead of 8 rows held in registers across the batch.
template <int VW> __device__ __forceinline__ int g2_again(const int nv) { return VW * (int) (nv < 0); }

// this lane's NP pieces of a row of n columns: piece q starts at column (q * LPR + lir) * VW; slots past n hold 0
template <typename T, int LPR, int NP, bool VEC>
__device__ __forceinline__ void g2_load_row(T (&x)[NP][G2Piece<T>::VW], const T *row, const int n, const int lir)
{
    typedef typename G2Piece<T>::type PT;
    constexpr int VW = G2Piece<T>::VW;
#pragma unroll
    for (int v = 0; v < NP; v++)
    {
        const int c = (v * LPR + lir) * VW;
        if constexpr (VEC)
        {
            PT t = {};
            if (c < n) t = *reinterpret_cast<const PT *>(row + c);
#pragma unroll
            for (int w = 0; w < VW; w++) x[v][w] = t[w];
        }
        else
        {
#pragma unroll
            for (int w = 0; w < VW; w++) x[v][w] = (c + w < n) ? row[c + w] : (T) 0;
        }
    }
}

// ... and the store of them (slots past n are not written)
template <typename T, int LPR, int NP, bool VEC>
__device__ __forceinline__ void g2_store_row(const T (&x)[NP][G2Piece<T>::VW], T *row, const int n, const int lir)
{
    typedef typename G2Piece<T>::type PT;
    constexpr int VW = G2Piece<T>::VW;
#pragma unroll
    for (int v = 0; v < NP; v++)
    {
        const int c = (v * LPR + lir) * VW;
        if constexpr (VEC)
        {
            PT t;
#pragma unroll
            for (int w = 0; w < VW; w++) t[w] = x[v][w];
            if (c < n) *reinterpret_cast<PT *>(row + c) = t;
        }
        else
        {
#pragma unroll
            for (int w = 0; w < VW; w++)
                if (c + w < n) row[c + w] = x[v][w];
        }
    }
}

// this lane's pieces piece0 .. piece0 + CH - 1 of the 8 rows y[q] (slots past n: column 0, a valid address, not used)
template <typename T, int LPR, int CH, bool VEC>
__device__ __forceinline__ void g2_load8(T (&yv)[G2_UNR][CH][G2Piece<T>::VW], const T *const (&y)[G2_UNR], const int piece0, const int n,
                                         const int lir, const int again = 0)
{
    typedef typename G2Piece<T>::type PT;
    constexpr int VW = G2Piece<T>::VW;
#pragma unroll
    for (int q = 0; q < G2_UNR; q++)
#pragma unroll
        for (int v = 0; v < CH; v++)
        {
            const int c = ((piece0 + v) * LPR + lir) * VW;
            if constexpr (VEC)
            {
                const PT t = *reinterpret_cast<const PT *>(y[q] + again + (unsigned) ((c < n) ? c : 0));
#pragma unroll
                for (int w = 0; w < VW; w++) yv[q][v][w] = t[w];
            }
            else
            {
#pragma unroll
                for (int w = 0; w < VW; w++) yv[q][v][w] = (y[q] + again)[(unsigned) ((c + w < n) ? c + w : 0)];
            }
        }
}

// One trip over this lane's NP pieces of the 8 rows y[q]: per step the gathers go out before the step's arithmetic, which runs in
// the order (q, piece, element) -- per q in column order, the SDDMM's chunk.  f(q, piece, element, in-range, value).
template <typename T, int LPR, int NP, bool VEC, class F>
__device__ __forceinline__ void g2_walk8(const T *const (&y)[G2_UNR], const int n, const int lir, const int again, F &&f)
{
    constexpr int VW = G2Piece<T>::VW;
    constexpr int CH = g2_ch<NP, VEC>;
    g2_static_for<0, NP, (VEC ? 2 : 1)>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        T yv[G2_UNR][CH][VW];
        g2_load8<T, LPR, CH, VEC>(yv, y, K, n, lir, again);
        __builtin_amdgcn_sched_barrier(0);              // every load of the step is in flight before the first FMA waits for one
#pragma unroll
        for (int q = 0; q < G2_UNR; q++)
#pragma unroll
            for (int v = 0; v < CH; v++)
#pragma unroll
                for (int w = 0; w < VW; w++) f(q, K + v, w, ((K + v) * LPR + lir) * VW + w < n, yv[q][v][w]);
        if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);      // (by elements: the next step's loads wait, for the registers)
    });
}

// reduce-scatter butterfly of the SDDMM: after it lane l holds entry (l & 7) of the batch summed over the group
template <typename T, int LPR>
__device__ __forceinline__ T g2_reduce8(const T (&part)[G2_UNR], const int lir)
{
    const bool b0 = (lir & 1) != 0, b1 = (lir & 2) != 0, b2 = (lir & 4) != 0;
    T q4[4], q2[2];
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const T keep = b0 ? part[2 * i + 1] : part[2 * i], send = b0 ? part[2 * i] : part[2 * i + 1];
        q4[i] = keep + __shfl_xor(send, 1, LPR);
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        const T keep = b1 ? q4[2 * i + 1] : q4[2 * i], send = b1 ? q4[2 * i] : q4[2 * i + 1];
        q2[i] = keep + __shfl_xor(send, 2, LPR);
    }
    T r = (b2 ? q2[1] : q2[0]) + __shfl_xor(b2 ? q2[0] : q2[1], 4, LPR);
#pragma unroll
    for (int mask = 8; mask < LPR; mask <<= 1) r = r + __shfl_xor(r, mask, LPR);
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
    const T e = dead ? (T) 0 : g2_exp(s - lse);
    if constexpr (DROP)
    {
        dp = keep ? g2_mul<T>(dp, rs) : (T) 0;
        *pp = keep ? g2_mul<T>(e, rs) : (T) 0;
    }
    else *pp = e;
    *ds = (e == (T) 0) ? (T) 0 : e * (dp - delta);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// LPR lanes per unit (row, head); P pieces of XT, a and the accumulator per lane.  VEC: 16-byte accesses; else elements.
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_fwd_kernel(const Gatv2Args<T> a)
{
    constexpr int VW  = G2Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = G2_UNR;
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
    const T ninf = g2_ninf<T>();
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
        g2_store_row<T, LPR, P, VEC>(acc, orp, nv, lir);
        if (a.lse != nullptr && lir == 0) a.lse[srow] = ninf;
        return;
    }
    T xt[P][VW], av[P][VW];                             // kept for the row
    g2_load_row<T, LPR, P, VEC>(xt, a.XT + orow * a.ldXT + hv, nv, lir);
    g2_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
    const T slope = a.slope;
    const bool bias = a.val != nullptr;
    const int again = g2_again<VW>(a.nv);
    T m = ninf, l = (T) 0;

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits)
        if constexpr (DROP) km = g2_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) orow, (uint32_t) c, (uint32_t) h, lir);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose score counts as -inf
            const int mine = j + (lir & 7);
            const int mcl = min(mine, cnt - 1);
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *xrow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) xrow[q] = g2_xs<T>(g2_bcast_i<LPR>(c, min(j + q, cnt - 1)), hv, a.XS0, a.ldXS0, a.XS1, a.ldXS1);

            T part[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) part[q] = (T) 0;
            T hold[UNR][1][VW];                         // (P == 1: the batch's pieces; else not used)
            if constexpr (HOLD)
            {
                g2_load8<T, LPR, 1, VEC>(hold, xrow, 0, nv, lir);
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
                g2_walk8<T, LPR, P, VEC>(xrow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                        part[q] = fma(av[v][w], r, part[q]);
                    }
                });
            }
            const T dot = g2_reduce8<T, LPR>(part, lir);

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
                f = g2_exp(m - mn);
                e = g2_exp(s - mn);
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
                g2_walk8<T, LPR, P, VEC>(xrow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
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
            if constexpr (DROP) acc[v][w] = g2_mul<T>(acc[v][w], a.drop.rs);
        }
    g2_store_row<T, LPR, P, VEC>(acc, orp, nv, lir);
    if (a.lse != nullptr && lir == 0) a.lse[srow] = masked ? ninf : m + g2_log(l);
    if (a.p_out != nullptr && lir < UNR)
        for (int p = pb + lir; p < pe; p += UNR)        // this lane's own stores
        {
            const int64_t pos = (int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h;
            const T sv = a.p_out[pos];
            a.p_out[pos] = masked ? (T) 0 : g2_exp(sv - m) / l;
        }
}

// ---- backward, row side: delta, dXT, da_part and ds_out over a handle of A ----------------------------------------------------------
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_bwd_row_kernel(const Gatv2BwdRowArgs<T> a)
{
    constexpr int VW  = G2Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = G2_UNR;
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
    const T ninf = g2_ninf<T>();

    // D = < dO[i]_h, O[i]_h >, the SDDMM's dot for (dtype, nv); every lane of the group ends with the same bits
    T xd[P][VW];
    g2_load_row<T, LPR, P, VEC>(xd, a.dO + orow * a.lddO + hv, nv, lir);
    T delta = (T) 0;
    {
        T xo[P][VW];
        g2_load_row<T, LPR, P, VEC>(xo, a.O + orow * a.ldO + hv, nv, lir);
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
        g2_store_row<T, LPR, P, VEC>(dxt, dxrow, nv, lir);
        g2_store_row<T, LPR, P, VEC>(dap, darow, nv, lir);
        if (a.ds_out != nullptr)
            for (int p = pb + lir; p < pe; p += LPR) a.ds_out[(int64_t) (a.out_pos ? a.out_pos[p] : p) * nh + h] = (T) 0;
        return;
    }
    const T slope = a.slope;
    T xt[P][VW], av[P][VW], as[P][VW];
    g2_load_row<T, LPR, P, VEC>(xt, a.XT + orow * a.ldXT + hv, nv, lir);
    g2_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) as[v][w] = g2_mul<T>(av[v][w], slope);
    const bool bias = a.val != nullptr;
    const int again = g2_again<VW>(a.nv);

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits)
        if constexpr (DROP) km = g2_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) orow, (uint32_t) c, (uint32_t) h, lir);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose dS counts as +0
            const int mine = j + (lir & 7);
            const int mcl = min(mine, cnt - 1);
            const T bv = bias ? a.val[p0 + mcl] : (T) 0;
            const T *xrow[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) xrow[q] = g2_xs<T>(g2_bcast_i<LPR>(c, min(j + q, cnt - 1)), hv, a.XS0, a.ldXS0, a.XS1, a.ldXS1);

            // one trip serves both dots: the score's and dP's
            T sp[UNR], dp[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) sp[q] = dp[q] = (T) 0;
            T rr[UNR][VW];                              // (P == 1: the batch's r and its branches, bit q VW + w of posm; else not used)
            unsigned posm = 0;
            if constexpr (HOLD)
            {
                T y[UNR][1][VW];
                g2_load8<T, LPR, 1, VEC>(y, xrow, 0, nv, lir);
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
                g2_walk8<T, LPR, P, VEC>(xrow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                        sp[q] = fma(av[v][w], r, sp[q]);
                        dp[q] = fma(xd[v][w], y, dp[q]);
                    }
                });
            }
            const T dot = g2_reduce8<T, LPR>(sp, lir);
            const T rp = g2_reduce8<T, LPR>(dp, lir);
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
                g2_walk8<T, LPR, P, VEC>(xrow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    bool pos;
                    const T r = g2_lrelu<T>(xt[v][w], y, slope, &pos);
                    const T ag = pos ? av[v][w] : as[v][w];
                    dxt[v][w] = fma(dsu[q], ag, dxt[v][w]);
                    dap[v][w] = fma(dsu[q], r, dap[v][w]);
                });
            }
        }
    }
    g2_store_row<T, LPR, P, VEC>(dxt, dxrow, nv, lir);
    g2_store_row<T, LPR, P, VEC>(dap, darow, nv, lir);
}

// ---- backward, column side: dXS over a handle of A^T (the unit is (column c, head h)) ------------------------------------------
template <typename T, int LPR, int P, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gatv2_bwd_col_kernel(const Gatv2BwdColArgs<T> a)
{
    constexpr int VW  = G2Piece<T>::VW;
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = G2_UNR;
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
    const T ninf = g2_ninf<T>();
    const int64_t hv = h * nv;
    T *const dxrow = a.dXS + crow * a.lddXS + hv;

    T accZ[P][VW], accV[P][VW];
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accZ[v][w] = accV[v][w] = (T) 0;
    if (pb >= pe)                                       // a column no row names: +0; its XS row is not read
    {
        g2_store_row<T, LPR, P, VEC>(accZ, dxrow, nv, lir);
        return;
    }
    // XS[c]_h whole, before anything of this unit is written (dXS == XS)
    const T slope = a.slope;
    T xs[P][VW], av[P][VW], as[P][VW];
    g2_load_row<T, LPR, P, VEC>(xs, a.XS + crow * a.ldXS + hv, nv, lir);
    g2_load_row<T, LPR, P, VEC>(av, a.av + hv, nv, lir);
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) as[v][w] = g2_mul<T>(av[v][w], slope);
    const bool bias = a.val != nullptr;
    const int again = g2_again<VW>(a.nv);

    for (int p0 = pb; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? a.colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        unsigned long long km = 0;                      // (DROP: the chunk's keep bits; the entry's row of A is r, this unit's row c)
        if constexpr (DROP) km = g2_keep_bits<T, LPR>(a.drop, my < pe, (uint32_t) c, (uint32_t) crow, (uint32_t) h, lir);
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
                const int ij = g2_bcast_i<LPR>(c, min(j + q, cnt - 1));
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
                g2_load8<T, LPR, 1, VEC>(ty, trow, 0, nv, lir);
                g2_load8<T, LPR, 1, VEC>(dy, drow, 0, nv, lir);
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
                g2_walk8<T, LPR, P, VEC>(trow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in)
                    {
                        bool pos;
                        const T r = g2_lrelu<T>(y, xs[v][w], slope, &pos);
                        sp[q] = fma(av[v][w], r, sp[q]);
                    }
                });
                g2_walk8<T, LPR, P, VEC>(drow, nv, lir, 0, [&](const int q, const int v, const int w, const bool in, const T y) {
                    if (in) dp[q] = fma(y, xs[v][w], dp[q]);
                });
            }
            const T dot = g2_reduce8<T, LPR>(sp, lir);
            const T rp = g2_reduce8<T, LPR>(dp, lir);
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
                g2_walk8<T, LPR, P, VEC>(trow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    bool pos;
                    (void) g2_lrelu<T>(y, xs[v][w], slope, &pos);
                    const T ag = pos ? av[v][w] : as[v][w];
                    accZ[v][w] = fma(dsu[q], ag, accZ[v][w]);
                });
                g2_walk8<T, LPR, P, VEC>(drow, nv, lir, again, [&](const int q, const int v, const int w, const bool, const T y) {
                    accV[v][w] = fma(pu[q], y, accV[v][w]);
                });
            }
        }
    }
#pragma unroll
    for (int v = 0; v < P; v++)
#pragma unroll
        for (int w = 0; w < VW; w++) accZ[v][w] = g2_add<T>(accZ[v][w], accV[v][w]);
    g2_store_row<T, LPR, P, VEC>(accZ, dxrow, nv, lir);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
static inline bool g2_aligned(std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> lds, int vw)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t) p;
    bool ok = bits % 16 == 0;
    for (int64_t ld : lds) ok = ok && ld % vw == 0;
    return ok;
}

// the grid of nrow * heads units, RPB per block; false when it does not fit one launch (before anything is written)
static inline bool g2_grid(int nrow, int heads, int rpb, dim3 *grid)
{
    const int64_t blocks = ((int64_t) nrow * heads + rpb - 1) / rpb;
    if (blocks > INT32_MAX) return false;
    *grid = dim3((unsigned) blocks);
    return true;
}

// (nv % VW == 0 keeps every head's slice on a 16-byte boundary; the leading dimension of a source that is NULL is not read)
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2Args<T> &a, hipStream_t s)
{
    constexpr int VW = G2Piece<T>::VW;
    const bool vec = g2_aligned({a.XT, a.XS0, a.XS1, a.av, a.O}, {a.nv, a.ldXT, a.ldO, a.XS0 ? a.ldXS0 : 0, a.XS1 ? a.ldXS1 : 0}, VW);
    dim3 grid;
    if (!g2_grid(a.nrow, a.heads, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (a.drop.on)
    {
        if (vec) hipLaunchKernelGGL((gatv2_fwd_kernel<T, LPR, P, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gatv2_fwd_kernel<T, LPR, P, false, true>), grid, dim3(256), 0, s, a);
    }
    else if (vec) hipLaunchKernelGGL((gatv2_fwd_kernel<T, LPR, P, true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gatv2_fwd_kernel<T, LPR, P, false, false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2BwdRowArgs<T> &a, hipStream_t s)
{
    constexpr int VW = G2Piece<T>::VW;
    const bool vec = g2_aligned({a.XT, a.XS0, a.XS1, a.av, a.O, a.dO, a.dXT, a.da_part},
                                {a.nv, a.ldXT, a.ldO, a.lddO, a.lddXT, a.ldda, a.XS0 ? a.ldXS0 : 0, a.XS1 ? a.ldXS1 : 0}, VW);
    dim3 grid;
    if (!g2_grid(a.nrow, a.heads, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (a.drop.on)
    {
        if (vec) hipLaunchKernelGGL((gatv2_bwd_row_kernel<T, LPR, P, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gatv2_bwd_row_kernel<T, LPR, P, false, true>), grid, dim3(256), 0, s, a);
    }
    else if (vec) hipLaunchKernelGGL((gatv2_bwd_row_kernel<T, LPR, P, true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gatv2_bwd_row_kernel<T, LPR, P, false, false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename T, int LPR, int P>
static hipError_t launch_gatv2(const Gatv2BwdColArgs<T> &a, hipStream_t s)
{
    constexpr int VW = G2Piece<T>::VW;
    // (XT and dO are not read when the handle has no nonzero, and may then be NULL)
    const bool vec = g2_aligned({a.XS, a.XT, a.av, a.dO, a.dXS}, {a.nv, a.ldXS, a.XT ? a.ldXT : 0, a.dO ? a.lddO : 0, a.lddXS}, VW);
    dim3 grid;
    if (!g2_grid(a.nrow, a.heads, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (a.drop.on)
    {
        if (vec) hipLaunchKernelGGL((gatv2_bwd_col_kernel<T, LPR, P, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((gatv2_bwd_col_kernel<T, LPR, P, false, true>), grid, dim3(256), 0, s, a);
    }
    else if (vec) hipLaunchKernelGGL((gatv2_bwd_col_kernel<T, LPR, P, true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gatv2_bwd_col_kernel<T, LPR, P, false, false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
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
