// attention_kernels.hip -- fused sparse attention over A's pattern for gfx950 (MI355X, wave64), fp64 and fp32.  For every row i
// with entries p = (i, c_p), p in CSR order:
//     s_p = scale * < Q[i][0:nk], K[c_p][0:nk] >     (bias: + A's current value of p)
//     O[i][0:nv] = sum_p softmax_p(s) * V[c_p][0:nv]
// in ONE trip over the row: the SDDMM's dots (sddmm_kernels.hip), an online softmax and the product with V, without the nnz-sized
// scores, probabilities or a value update in between.  A group of LPR lanes owns a row, keeps its slice of Q[i] and of the
// accumulator of O[i] in registers and walks the row in batches of 8 nonzeros.  No atomics, no LDS, no partial result in memory.
//
// Two-source column code (include/crpspmm_hip.h), for K and V alike: c >= 0 -> row c of K0 / V0, c < 0 -> row ~c of K1 / V1.
//
// INSTANCE.  With W = elements per 16 bytes and G(n) = 8, 16, 32, 64 for n <= 8 W, 16 W, 32 W, else (the SDDMM's group for a
// width n), LPR = max(G(nk), G(nv)).  Column j of Q / K and of V / O belongs to lane (j / W) % LPR, piece (j / W) / LPR of that
// lane.  PK = pieces of Q a lane keeps for the row: the smallest of 1, 2, 4 that covers nk, else 0 (any nk: the group walks K in
// chunks of two pieces and re-reads its pieces of Q per batch, which are cache hits).  PV = pieces of the accumulator a lane
// keeps: the smallest of 1, 2, 4, 8 that covers nv; a wider V is processed in column blocks of 8 LPR W columns, and the row's
// scores are formed again for every block (same bits), so that nothing partial ever goes to memory.  All of it is a function of
// (dtype, nk, nv) alone.  Operands that cannot be read in 16-byte pieces (odd widths or leading dimensions, unaligned pointers)
// are read and written element by element in the SAME assignment.
//
// FIXED ORDER.  The dot of an entry is the SDDMM's for (dtype, nk): a lane adds its products in ascending j with FMAs from +0
// and the lanes' sums meet in the balanced binary tree over the lane number; lanes of a group larger than G(nk) hold +0, which
// the tree adds exactly, so the bits before `* scale` equal crp_sddmm_csr_*'s (a dot of -0, which needs underflow in every lane,
// may come out as +0; no later step tells the two apart).  s = dot * scale, one rounding (bias: then s + val, one more).  Then per
// batch of 8 entries in ascending p, with m = -inf, l = 0, acc = 0 before the first:
//     m' = max(m, the batch's scores);   f = exp(m - m');   e_u = exp(s_u - m')          (m' == -inf: f = 1, e_u = 0)
//     l = l * f;  l = l + e_u for u = 0 .. 7;   acc[j] = acc[j] * f;  acc[j] = fma(e_u, V[c_u][j], acc[j]) for u = 0 .. 7
// (slots of a last partial batch past the row's end count as s = -inf, and their FMAs use the row's last entry's V row with
// e = 0), and after the row O[i][j] = acc[j] / l (IEEE), lse[i] = m + log(l), p_out[p] = exp(s_p - m) / l with the final m, l.
// The maximum is taken at every batch and never deferred: every quantity at the old maximum is multiplied by f exactly once, and
// a batch's e_u are formed only after the m' that covers them.  A row's bits are a function of (dtype, nk, nv, scale, bias) and
// the row's entries in CSR order ONLY: not of alignment, leading dimensions, the source a K / V row comes from, the handle (full
// or row subset), the optional outputs, or the other rows.
//
// SPECIAL CASES.  An empty row writes +0 to O[i][0:nv] and lse = -inf.  A one-entry row with a finite score gives f = 0, e = 1,
// l = 1 and O[i] = V[c].  s_p = -inf (a bias value, or a product) is a masked edge: e = +0 exactly, its V row is still read (V is
// taken to be finite: 0 * V must be 0).  An all-masked row keeps m == -inf and writes zeros, lse = -inf, p_out = 0.  A row with
// NaN or +inf among its scores has unspecified outputs in that row only.
//
// MULTI-HEAD (the MH instances: attention_rm with mh).  a.heads = H heads of nk / nv columns each lie side by side in every operand:
// head h owns columns [h nk, (h + 1) nk) of Q / K and [h nv, (h + 1) nv) of V / O.  A group owns the unit u = row * H + h
// (row = u / H, h = u % H in 64 bits), so consecutive groups of a wave hold consecutive heads of one row, share its column
// indices and gather adjacent slices of the same K / V row.  Everything above holds per unit with the operand bases advanced by
// h nk / h nv: head h's bits are the single-head instance's on the column views of head h.  lse is (rows, H) row-major, p_out
// (nnz, H): entry (pos, h) at pos * H + h; val[p] (bias) is shared by the heads.  The 16-byte path needs nk % W == 0 and
// nv % W == 0 as before, which now keeps every head's slice aligned.  The grid is ceil(nrow * H / RPB) in 64 bits.  The
// single-head instances (MH = false) compile none of this.
//
// p_out: the lanes 0 .. 7 of the group that hold a batch's scores store them raw (through out_pos); after the row the same lanes
// -- entry p of a row that starts at pb belongs to lane (p - pb) % 8 -- read their own stores back and overwrite them with the
// probabilities.  No lane ever reads what another lane wrote.
//
// The piece type, exp / log / -inf, the broadcast of a column code and the launcher's alignment and grid checks are row_group.h's
// (rg_).  The kernel's own lambdas, its inlined butterfly and the online-softmax step stay here: as functions of that header they
// compile to other instructions (measured), and this file's instructions are not to change.
#include "row_group.h"

namespace crp {

// LPR lanes per row; PK pieces of Q per lane in registers (0: any nk); PV pieces of the accumulator per lane and V block.
// VEC: 16-byte accesses; else single elements.  Every column slot is checked against its width.
// MH: a group owns the unit (row, head) = (u / heads, u % heads), nk and nv are the widths of one head, and head h's slices start
// at column h * nk of Q / K and h * nv of V / O; lse is (rows, heads), p_out is (nnz, heads).  Without MH none of it is compiled.
template <typename T, int LPR, int PK, int PV, bool VEC, bool MH = false>
__global__ __launch_bounds__(256) void attention_rm_kernel(const AttnArgs<T> a)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW  = 16 / (int) sizeof(T);
    constexpr int RPB = 256 / LPR;
    constexpr int UNR = 8;
    constexpr int KC  = PK == 1 ? 1 : 2;                // pieces of K per load chunk (8 KC pieces in flight)
    constexpr int QP  = PK > 0 ? PK : KC;
    constexpr int VC  = PV < 4 ? PV : 4;                // pieces of V per load chunk (8 VC pieces in flight)
    constexpr int VBW = LPR * VW * PV;                  // columns of a V block
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
    const int64_t orow = a.rowmap ? a.rowmap[row] : row;        // rowmap: the Q and O row of every row of a row-subset matrix
    const T ninf = rg_ninf<T>();
    const int64_t hk = h * nk, hv = h * nv;             // the head's first column (MH; else 0)
    const int64_t srow = MH ? orow * nh + h : orow;     // the unit's entry of lse
    T *const orp = a.O + orow * a.ldO + hv;
    auto ppos = [&](const int pos) {                    // where nonzero position pos of this unit lies in p_out
        if constexpr (MH) return pos * nh + h;
        else return pos;
    };

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

    if (pb >= pe)                                       // an empty row: zeros (C of a product is defined on every row); no Q row is read
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
    const T *qrow = a.Q + orow * a.ldQ + hk;

    // this lane's pieces piece0 .. piece0 + np - 1 of Q[orow]: piece q starts at column (q * LPR + lir) * VW
    auto load_q = [&](T (*x)[VW], const int piece0, const int np) {
#pragma unroll
        for (int v = 0; v < QP; v++)
        {
            if (v >= np) break;
            const int c = ((piece0 + v) * LPR + lir) * VW;
            if constexpr (VEC)
            {
                PT t = {};
                if (c < nk) t = *reinterpret_cast<const PT *>(qrow + c);
#pragma unroll
                for (int w = 0; w < VW; w++) x[v][w] = t[w];
            }
            else
            {
#pragma unroll
                for (int w = 0; w < VW; w++) x[v][w] = (c + w < nk) ? qrow[c + w] : (T) 0;
            }
        }
    };
    // part[u] += < x, this lane's pieces piece0 .. piece0 + KC - 1 of K row krow[u] >, u < 8: all loads first, then the FMAs in
    // column order (the SDDMM's chunk)
    auto kchunk = [&](const T (*x)[VW], const int piece0, const T *(&krow)[UNR], T (&part)[UNR]) {
        T yv[UNR][KC][VW];
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int v = 0; v < KC; v++)
            {
                const int c = ((piece0 + v) * LPR + lir) * VW;
                if constexpr (VEC)
                {
                    // slots past nk load column 0 of the row (a valid address) and are not used
                    const PT t = *reinterpret_cast<const PT *>(krow[u] + ((c < nk) ? c : 0));
#pragma unroll
                    for (int w = 0; w < VW; w++) yv[u][v][w] = t[w];
                }
                else
                {
#pragma unroll
                    for (int w = 0; w < VW; w++) yv[u][v][w] = krow[u][(c + w < nk) ? c + w : 0];
                }
            }
        __builtin_amdgcn_sched_barrier(0);              // every K load of the chunk is in flight before the first FMA waits for one
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int v = 0; v < KC; v++)
#pragma unroll
                for (int w = 0; w < VW; w++)
                {
                    const int c = ((piece0 + v) * LPR + lir) * VW + w;
                    if (c < nk) part[u] = fma(x[v][w], yv[u][v][w], part[u]);
                }
    };
    // this lane's pieces v0 .. v0 + VC - 1 of block vb of the 8 V rows (slots past nv: column 0, not used)
    auto load_v = [&](T (&vv)[UNR][VC][VW], const int vb, const int v0, const T *(&vrow)[UNR]) {
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int v = 0; v < VC; v++)
            {
                const int c = vb + ((v0 + v) * LPR + lir) * VW;
                if constexpr (VEC)
                {
                    const PT t = *reinterpret_cast<const PT *>(vrow[u] + ((c < nv) ? c : 0));
#pragma unroll
                    for (int w = 0; w < VW; w++) vv[u][v][w] = t[w];
                }
                else
                {
#pragma unroll
                    for (int w = 0; w < VW; w++) vv[u][v][w] = vrow[u][(c + w < nv) ? c + w : 0];
                }
            }
    };

    T xr[QP][VW];
    if constexpr (PK > 0) load_q(xr, 0, PK);
    const int npk = (nk + LPR * VW - 1) / (LPR * VW);   // pieces of K per lane (PK == 0)
    const bool b0 = (lir & 1) != 0, b1 = (lir & 2) != 0, b2 = (lir & 4) != 0;
    const T scale = a.scale;

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
            for (int j = 0; j < cnt; j += UNR)
            {
                // indices past the row end are clamped to the row's last entry: a valid row whose score counts as -inf
                const T *krow[UNR], *vrow[UNR];
#pragma unroll
                for (int u = 0; u < UNR; u++)
                {
                    const int cj = rg_bcast_i<LPR>(c, min(j + u, cnt - 1));
                    krow[u] = ((cj >= 0) ? (a.K0 + (int64_t) cj * a.ldK0) : (a.K1 + (int64_t) (~cj) * a.ldK1)) + hk;
                    vrow[u] = ((cj >= 0) ? (a.V0 + (int64_t) cj * a.ldV0) : (a.V1 + (int64_t) (~cj) * a.ldV1)) + hv;
                }
                T part[UNR];
#pragma unroll
                for (int u = 0; u < UNR; u++) part[u] = (T) 0;
                if constexpr (PK > 0)
                {
#pragma unroll
                    for (int k = 0; k < PK; k += KC) kchunk(xr + k, k, krow, part);
                }
                else
                {
                    for (int k = 0; k < npk; k += KC)
                    {
                        load_q(xr, k, KC);
                        kchunk(xr, k, krow, part);
                    }
                }
                // reduce-scatter butterfly: after the xor-1, -2, -4 steps lane l holds entry (l & 7) summed over its 8 lanes
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

                // the first V pieces of the batch go out before the exponentials
                T vv[UNR][VC][VW];
                load_v(vv, vb, 0, vrow);
                __builtin_amdgcn_sched_barrier(0);

                // every lane holds the score of entry (lir & 7) of the batch
                const int mine = j + (lir & 7);
                T s = ninf;
                if (mine < cnt)
                {
                    s = r * scale;
                    if (a.val != nullptr) s = s + a.val[p0 + mine];
                    if (first && a.p_out != nullptr && lir < UNR)
                    {
                        const int p = p0 + mine;
                        a.p_out[ppos(a.out_pos ? a.out_pos[p] : p)] = s;
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
                for (int u = 0; u < UNR; u++) eu[u] = __shfl(e, u, LPR);
                l = l * f;
#pragma unroll
                for (int u = 0; u < UNR; u++) l = l + eu[u];
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
                    for (int u = 0; u < UNR; u++)
#pragma unroll
                        for (int v = 0; v < VC; v++)
#pragma unroll
                            for (int w = 0; w < VW; w++) acc[v0 + v][w] = fma(eu[u], vv[u][v][w], acc[v0 + v][w]);
                }
            }
        }

        const bool masked = m == ninf;                  // every entry masked: zeros, not 0 / 0
#pragma unroll
        for (int v = 0; v < PV; v++)
#pragma unroll
            for (int w = 0; w < VW; w++) acc[v][w] = masked ? (T) 0 : acc[v][w] / l;
        store_o(acc, vb);
        if (first)
        {
            if (a.lse != nullptr && lir == 0) a.lse[srow] = masked ? ninf : m + rg_log(l);
            if (a.p_out != nullptr && lir < UNR)
                for (int p = pb + lir; p < pe; p += UNR)        // this lane's own stores
                {
                    const auto pos = ppos(a.out_pos ? a.out_pos[p] : p);
                    const T sv = a.p_out[pos];
                    a.p_out[pos] = masked ? (T) 0 : rg_exp(sv - m) / l;
                }
        }
    }
}

// (nk % VW == 0 and nv % VW == 0 keep every head's slice on a 16-byte boundary; the leading dimension of a source that is NULL is
// not read: it counts as 0.  The single-head instances take a.heads as 1, whatever it holds)
template <typename T, int LPR, int PK, int PV, bool MH>
static hipError_t launch_attention(const AttnArgs<T> &a, hipStream_t s)
{
    const bool vec = rg_aligned({a.Q, a.O, a.K0, a.K1, a.V0, a.V1},
                                {a.nk, a.nv, a.ldQ, a.ldO, a.K0 ? a.ldK0 : 0, a.K0 ? a.ldV0 : 0, a.K1 ? a.ldK1 : 0, a.K1 ? a.ldV1 : 0},
                                Piece<T>::VW);
    dim3 grid;
    if (!rg_grid(a.nrow, MH ? a.heads : 1, 256 / LPR, &grid)) return hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL((attention_rm_kernel<T, LPR, PK, PV, true, MH>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attention_rm_kernel<T, LPR, PK, PV, false, MH>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <typename T, int PK, bool MH>
static hipError_t attention_wave(const AttnArgs<T> &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T);
    if (a.nv <= 64 * W)  return launch_attention<T, 64, PK, 1, MH>(a, s);
    if (a.nv <= 128 * W) return launch_attention<T, 64, PK, 2, MH>(a, s);
    if (a.nv <= 256 * W) return launch_attention<T, 64, PK, 4, MH>(a, s);
    return launch_attention<T, 64, PK, 8, MH>(a, s);
}

// The instance, from (dtype, nk, nv) alone (the rule is stated at the top of this file); MH: from the widths of one head
template <typename T, bool MH>
static hipError_t attention_rm(const AttnArgs<T> &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T);
    if (a.nrow <= 0) return hipSuccess;
    const int wide = a.nk > a.nv ? a.nk : a.nv;
    if (wide <= 8 * W)  return launch_attention<T, 8, 1, 1, MH>(a, s);
    if (wide <= 16 * W) return launch_attention<T, 16, 1, 1, MH>(a, s);
    if (wide <= 32 * W) return launch_attention<T, 32, 1, 1, MH>(a, s);
    if (a.nk <= 64 * W)  return attention_wave<T, 1, MH>(a, s);
    if (a.nk <= 128 * W) return attention_wave<T, 2, MH>(a, s);
    if (a.nk <= 256 * W) return attention_wave<T, 4, MH>(a, s);
    return attention_wave<T, 0, MH>(a, s);
}

// (instantiated here, in this order, so that the kernels keep their places in the code object: both single-head families first)
template hipError_t attention_rm<double, false>(const AttnArgs<double> &, hipStream_t);
template hipError_t attention_rm<float, false>(const AttnArgs<float> &, hipStream_t);
template hipError_t attention_rm<double, true>(const AttnArgs<double> &, hipStream_t);
template hipError_t attention_rm<float, true>(const AttnArgs<float> &, hipStream_t);

// mh: the (row, head) instances, whatever a.heads; else the single-head ones
hipError_t attention_rm(const AttnArgs<double> &a, bool mh, hipStream_t s)
{
    return mh ? attention_rm<double, true>(a, s) : attention_rm<double, false>(a, s);
}
hipError_t attention_rm(const AttnArgs<float> &a, bool mh, hipStream_t s)
{
    return mh ? attention_rm<float, true>(a, s) : attention_rm<float, false>(a, s);
}

}  // namespace crp
