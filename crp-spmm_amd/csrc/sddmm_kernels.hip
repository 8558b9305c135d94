// sddmm_kernels.hip -- sampled dense-dense product over A's pattern for gfx950 (MI355X, wave64), fp64 and fp32:
//     out[p] = < X[i][0:n], Y[c][0:n] >   (mode 1: times val[p])      for every nonzero p = (i, c) of A.
// Gather work with the byte profile of the CSR row-group SpMM (spmm_rm_f64_kernel, spmm_kernels.hip): one Y row slice
// per nonzero; X is read once per row and one scalar is written per nonzero.  A group of LPR lanes owns one row of A
// and keeps its slice of X[i] in registers, in 16-byte pieces per lane.  The row's column codes are loaded coalesced
// LPR at a time and broadcast inside the group; nonzeros go in batches of 8: every Y-row load of the batch is issued,
// 8 per-lane partial dots are formed with FMAs, and the batch is reduced with a reduce-scatter butterfly (xor-1
// exchanges 4 partials, xor-2 two, xor-4 one, then log2(LPR) - 3 single-value steps), after which lanes 0 .. 7 of the
// group hold the 8 results and store them as one contiguous run.  No atomics, no LDS, no partial sum in memory.
//
// Two-source column code (include/crpspmm_hip.h): c >= 0 -> row c of Y0, c < 0 -> row ~c of Y1.
//
// FIXED ORDER.  Column j of the operands belongs to lane ((j / VW) % LPR) of the group, piece (j / VW) / LPR of that
// lane (VW = elements per 16 bytes); a lane adds its products in ascending j with FMAs, starting from 0; the lanes'
// partial sums meet in the balanced binary tree over the lane number (l with l ^ 1, then with l ^ 2, ...), every node
// one IEEE addition, which is commutative -- so which lane of a pair forms a node does not matter.  LPR and the piece
// count are picked from (dtype, n) alone.  Operands that cannot be read in 16-byte pieces (odd n or ld, unaligned
// pointers) are read element by element into the SAME assignment.  Hence an entry's bits depend on (dtype, n) and the
// two rows only: not on alignment, leading dimensions, the source of the Y row, the handle, or the entry's position.
#include "row_group.h"

namespace crp {

// LPR lanes per row, NV 16-byte pieces per lane and column chunk => chunks of TW = LPR * VW * NV columns.
// NCH > 0: the operands are NCH chunks wide at most and the whole slice of X[i] stays in registers for the row;
// NCH = 0: any width, the group walks the chunks inside each batch and re-reads its piece of X[i] per chunk (cache hits).
// VEC: 16-byte accesses; else single elements.  TAIL: some column slot of the chunks lies past n (checked per element).
template <typename T, int LPR, int NV, int NCH, bool VEC, bool TAIL>
__global__ __launch_bounds__(256) void sddmm_rm_kernel(
    const int nrow, const int n, const int *__restrict__ rowptr, const int *__restrict__ colidx, const T *__restrict__ val,
    const T *__restrict__ X, const int64_t ldX, const T *__restrict__ Y0, const int64_t ldY0,
    const T *__restrict__ Y1, const int64_t ldY1, T *__restrict__ out, const int *__restrict__ rowmap,
    const int *__restrict__ out_pos, const int mode)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW  = 16 / (int) sizeof(T);
    constexpr int RPB = 256 / LPR;
    constexpr int TW  = LPR * VW * NV;
    constexpr int UNR = 8;
    constexpr int XCH = NCH > 0 ? NCH : 1;
    const int lir = threadIdx.x % LPR;                  // lane in row group
    const int row = blockIdx.x * RPB + threadIdx.x / LPR;
    if (row >= nrow) return;
    int p0 = rowptr[row];
    const int pe = rowptr[row + 1];
    if (p0 >= pe) return;                               // an empty row reads no X row
    if constexpr (LPR == 64) p0 = __builtin_amdgcn_readfirstlane(p0);
    const T *xrow = X + (int64_t) (rowmap ? rowmap[row] : row) * ldX;      // rowmap: X row of every row of a row-subset matrix

    // this lane's piece v of chunk k starts at column k * TW + (v * LPR + lir) * VW
    auto load_x = [&](T (&x)[NV][VW], const int k) {
#pragma unroll
        for (int v = 0; v < NV; v++)
        {
            const int c = k * TW + (v * LPR + lir) * VW;
            if constexpr (VEC)
            {
                PT t = {};
                if (!TAIL || c < n) t = *reinterpret_cast<const PT *>(xrow + c);
#pragma unroll
                for (int w = 0; w < VW; w++) x[v][w] = t[w];
            }
            else
            {
#pragma unroll
                for (int w = 0; w < VW; w++) x[v][w] = (c + w < n) ? xrow[c + w] : (T) 0;
            }
        }
    };
    // part[u] += < x, this lane's pieces of chunk k of Y row yrow[u] >, u < 8: all loads first, then the FMAs in column order
    auto chunk = [&](const T (&x)[NV][VW], const int k, const T *(&yrow)[UNR], T (&part)[UNR]) {
        T yv[UNR][NV][VW];
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int v = 0; v < NV; v++)
            {
                const int c = k * TW + (v * LPR + lir) * VW;
                if constexpr (VEC)
                {
                    // slots past n load column 0 of the row (a valid address) and are not used
                    const PT t = *reinterpret_cast<const PT *>(yrow[u] + ((!TAIL || c < n) ? c : 0));
#pragma unroll
                    for (int w = 0; w < VW; w++) yv[u][v][w] = t[w];
                }
                else
                {
#pragma unroll
                    for (int w = 0; w < VW; w++) yv[u][v][w] = yrow[u][(c + w < n) ? c + w : 0];
                }
            }
        // every load of the batch is in flight before the first FMA waits for one: without the fence the scheduler trades the
        // loads in flight for registers (4 to 6 at a time instead of 8 NV)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int v = 0; v < NV; v++)
#pragma unroll
                for (int w = 0; w < VW; w++)
                {
                    const int c = k * TW + (v * LPR + lir) * VW + w;
                    if (!TAIL || c < n) part[u] = fma(x[v][w], yv[u][v][w], part[u]);
                }
    };

    T xr[XCH][NV][VW];
    if constexpr (NCH > 0)
    {
#pragma unroll
        for (int k = 0; k < NCH; k++) load_x(xr[k], k);
    }
    const int nch = (n + TW - 1) / TW;
    const bool b0 = (lir & 1) != 0, b1 = (lir & 2) != 0, b2 = (lir & 4) != 0;

    for (; p0 < pe; p0 += LPR)
    {
        const int my = p0 + lir;
        const int c = (my < pe) ? colidx[my] : 0;
        const int cnt = min(LPR, pe - p0);
        for (int j = 0; j < cnt; j += UNR)
        {
            // indices past the row end are clamped to the row's last entry: a valid row whose dot is not stored
            const T *yrow[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++)
            {
                const int cj = rg_bcast_i<LPR>(c, min(j + u, cnt - 1));
                yrow[u] = (cj >= 0) ? (Y0 + (int64_t) cj * ldY0) : (Y1 + (int64_t) (~cj) * ldY1);
            }
            T part[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) part[u] = (T) 0;
            if constexpr (NCH > 0)
            {
#pragma unroll
                for (int k = 0; k < NCH; k++) chunk(xr[k], k, yrow, part);
            }
            else
            {
                for (int k = 0; k < nch; k++)
                {
                    load_x(xr[0], k);
                    chunk(xr[0], k, yrow, part);
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
            if (lir < UNR && j + lir < cnt)
            {
                const int p = p0 + j + lir;
                if (mode != 0) r = r * val[p];
                out[out_pos ? out_pos[p] : p] = r;
            }
        }
    }
}

template <typename T, int LPR, int NV, int NCH>
static hipError_t launch_sddmm(const SddmmArgs<T> &a, hipStream_t s)
{
    constexpr int VW = 16 / (int) sizeof(T), RPB = 256 / LPR, TW = LPR * VW * NV;
    const bool vec = (a.n % VW == 0) && (a.ldX % VW == 0) && (a.ldY0 % VW == 0) && (a.Y1 == nullptr || a.ldY1 % VW == 0) &&
                     (((uintptr_t) a.X | (uintptr_t) a.Y0 | (uintptr_t) a.Y1) % 16 == 0);
    const bool tail = NCH > 0 ? (a.n != NCH * TW) : (a.n % TW != 0);
    const dim3 grid((a.nrow + RPB - 1) / RPB), block(256);
#define CRP_SDDMM_LAUNCH(VEC, TAIL)                                                                                                   \
    hipLaunchKernelGGL((sddmm_rm_kernel<T, LPR, NV, NCH, VEC, TAIL>), grid, block, 0, s, a.nrow, a.n, a.rowptr, a.colidx, a.val, a.X, \
                       a.ldX, a.Y0, a.ldY0, a.Y1, a.ldY1, a.out, a.rowmap, a.out_pos, a.mode)
    if (!vec) CRP_SDDMM_LAUNCH(false, true);            // (the checks of TAIL hold for every n)
    else if (tail) CRP_SDDMM_LAUNCH(true, true);
    else CRP_SDDMM_LAUNCH(true, false);
#undef CRP_SDDMM_LAUNCH
    return hipGetLastError();
}

// The lane group and the chunk shape, from n alone (W = columns per 16 bytes: 2 fp64, 4 fp32): narrow operands take
// small groups so that most of a wave does not idle; from 64 W columns on a whole wave owns the row, two pieces per lane
// and chunk; X[i] stays in registers up to 8 pieces per lane (512 W columns).
template <typename T>
static hipError_t sddmm_rm(const SddmmArgs<T> &a, hipStream_t s)
{
    constexpr int W = 16 / (int) sizeof(T);
    if (a.nrow <= 0) return hipSuccess;
    if (a.n <= 8 * W)   return launch_sddmm<T, 8, 1, 1>(a, s);
    if (a.n <= 16 * W)  return launch_sddmm<T, 16, 1, 1>(a, s);
    if (a.n <= 32 * W)  return launch_sddmm<T, 32, 1, 1>(a, s);
    if (a.n <= 64 * W)  return launch_sddmm<T, 64, 1, 1>(a, s);
    if (a.n <= 128 * W) return launch_sddmm<T, 64, 2, 1>(a, s);
    if (a.n <= 256 * W) return launch_sddmm<T, 64, 2, 2>(a, s);
    if (a.n <= 384 * W) return launch_sddmm<T, 64, 2, 3>(a, s);
    if (a.n <= 512 * W) return launch_sddmm<T, 64, 2, 4>(a, s);
    return launch_sddmm<T, 64, 2, 0>(a, s);
}

hipError_t sddmm_rm_f64(const SddmmArgs<double> &a, hipStream_t s) { return sddmm_rm<double>(a, s); }
hipError_t sddmm_rm_f32(const SddmmArgs<float> &a, hipStream_t s) { return sddmm_rm<float>(a, s); }

}  // namespace crp
