// row_group.h -- what the row-group kernels over A's pattern share (sddmm_kernels.hip, softmax_kernels.hip, attention_kernels.hip,
// attention_bwd_kernels.hip, gat_kernels.hip, gatv2_kernels.hip): a group of LPR lanes owns a row (or a (row, head) unit), column j
// of an operand belongs to lane (j / VW) % LPR, piece (j / VW) / LPR of that lane (VW = elements per 16 bytes), and entries go in
// batches of RG_UNR = 8.  Included from .hip files only.  These files promise one another the same bits -- a dot "as the SDDMM
// forms it", the forward's scores formed again in the backward -- and one definition of each helper is what keeps that promise.
// Every device helper is force-inlined.  A change here changes every kernel that uses it: compare the files' device assembly
// (the Makefile's flags plus --cuda-device-only -S) before and after, and read the resource-usage remarks the Makefile keeps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <type_traits>
#include "kernels.h"

namespace crp {

constexpr int RG_UNR = 8;                               // entries of a batch

// the 16-byte piece of a row
template <typename T> struct Piece;
template <> struct Piece<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int VW = 2; };
template <> struct Piece<float>  { typedef float type __attribute__((ext_vector_type(4))); static constexpr int VW = 4; };

__device__ __forceinline__ double rg_exp(double x) { return exp(x); }
__device__ __forceinline__ float  rg_exp(float x) { return expf(x); }
__device__ __forceinline__ double rg_log(double x) { return log(x); }
__device__ __forceinline__ float  rg_log(float x) { return logf(x); }
template <typename T> __device__ __forceinline__ T rg_ninf() { return -__builtin_huge_val(); }
template <> __device__ __forceinline__ float rg_ninf<float>() { return -__builtin_huge_valf(); }

// lane j's v for every lane of the group (a whole wave: j is uniform, one readlane)
template <int LPR>
__device__ __forceinline__ int rg_bcast_i(int v, int j)
{
    if constexpr (LPR == 64) return __builtin_amdgcn_readlane(v, j);
    else return __shfl(v, j, LPR);
}

// A product that is a rounding of its own (as = a * slope, the products with rs of the DROP instances): contraction off.  hipcc
// contracts across statements by default, and dP rs - D may never become one FMA.
template <typename T>
__device__ __forceinline__ T rg_mul(const T x, const T y)
{
#pragma clang fp contract(off)
    const T r = x * y;
    return r;
}

// The keep bits of a chunk of LPR entries: the lane that holds entry `lir` of the chunk (live: it has one) draws the bit of
// (r, c, h); bit e of the result is entry e's, the same word in every lane of the group.  Every lane of a group is active here
// together (the chunk loop's bounds are the group's); lanes of other groups that are not contribute 0 to bits this group drops.
template <typename T, int LPR>
__device__ __forceinline__ unsigned long long rg_keep_bits(const DropArgs<T> &d, const bool live, const uint32_t r, const uint32_t c,
                                                           const uint32_t h, const int lir)
{
    const bool k = live && dropout_keep(d.seed_lo, d.seed_hi, r, c, h, d.thr);
    const unsigned long long all = __ballot(k);
    if constexpr (LPR == 64) return all;
    else return all >> ((threadIdx.x & 63u) - (unsigned) lir);
}

// pieces per lane and row of one load step: two by 16-byte accesses, one by elements (which cost a register per element AND
// an address each), so that no instance spills
template <int P, bool VEC> constexpr int rg_ch = VEC ? (P < 2 ? P : 2) : 1;

// f(integral_constant K) for K = K0, K0 + STEP, ... < END
template <int K0, int END, int STEP, class F>
__device__ __forceinline__ void rg_static_for(F &&f)
{
    if constexpr (K0 < END)
    {
        f(std::integral_constant<int, K0>{});
        rg_static_for<K0 + STEP, END, STEP>(f);
    }
}

// The zero of rg_load8's `again`.  It stays opaque only as long as nothing lets the compiler prove n >= 0 for the width n it is
// formed from: an assumption or a check on n ahead of the loops (__builtin_assume, an early return on n < 1) folds it to 0, the
// two reads of a batch's rows merge again and the wide instances spill without a warning.  csrc/Makefile compiles the files that
// use it with the resource-usage remarks and fails the build when any instance reports scratch or LDS.
template <int VW> __device__ __forceinline__ int rg_again(const int n) { return VW * (int) (n < 0); }

// this lane's NP pieces of a row of n columns: piece q starts at column (q * LPR + lir) * VW; slots past n hold 0
template <typename T, int LPR, int NP, bool VEC>
__device__ __forceinline__ void rg_load_row(T (&x)[NP][Piece<T>::VW], const T *row, const int n, const int lir)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW = Piece<T>::VW;
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
__device__ __forceinline__ void rg_store_row(const T (&x)[NP][Piece<T>::VW], T *row, const int n, const int lir)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW = Piece<T>::VW;
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

// this lane's pieces piece0 .. piece0 + CH - 1 of the 8 rows y[q] (slots past n: column 0, a valid address, not used).  again:
// 0 at run time in a form the compiler cannot see through (rg_again), added to the row's address -- the second read of a batch's
// rows (for the accumulators, after the dots) stays a load of its own, a cache hit, instead of 8 rows held in registers across
// the batch
template <typename T, int LPR, int CH, bool VEC>
__device__ __forceinline__ void rg_load8(T (&yv)[RG_UNR][CH][Piece<T>::VW], const T *const (&y)[RG_UNR], const int piece0, const int n,
                                         const int lir, const int again = 0)
{
    typedef typename Piece<T>::type PT;
    constexpr int VW = Piece<T>::VW;
#pragma unroll
    for (int q = 0; q < RG_UNR; q++)
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
__device__ __forceinline__ void rg_walk8(const T *const (&y)[RG_UNR], const int n, const int lir, const int again, F &&f)
{
    constexpr int VW = Piece<T>::VW;
    constexpr int CH = rg_ch<NP, VEC>;
    rg_static_for<0, NP, (VEC ? 2 : 1)>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        T yv[RG_UNR][CH][VW];
        rg_load8<T, LPR, CH, VEC>(yv, y, K, n, lir, again);
        __builtin_amdgcn_sched_barrier(0);              // every load of the step is in flight before the first FMA waits for one
#pragma unroll
        for (int q = 0; q < RG_UNR; q++)
#pragma unroll
            for (int v = 0; v < CH; v++)
#pragma unroll
                for (int w = 0; w < VW; w++) f(q, K + v, w, ((K + v) * LPR + lir) * VW + w < n, yv[q][v][w]);
        if constexpr (!VEC) __builtin_amdgcn_sched_barrier(0);      // (by elements: the next step's loads wait, for the registers)
    });
}

// reduce-scatter butterfly of the SDDMM: after it lane l holds entry (l & 7) of the batch summed over the group
template <typename T, int LPR>
__device__ __forceinline__ T rg_reduce8(const T (&part)[RG_UNR], const int lir)
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

// ---- host side: what a launcher decides ---------------------------------------------------------------------------------------
// 16-byte accesses are possible: every pointer on a 16-byte boundary (NULL is) and every width and leading dimension a multiple
// of vw.  A caller passes 0 for the leading dimension of a source that is NULL: it is not read.
static inline bool rg_aligned(std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> lds, int vw)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t) p;
    bool ok = bits % 16 == 0;
    for (int64_t ld : lds) ok = ok && ld % vw == 0;
    return ok;
}

// the grid of nrow * heads units, rpb per block; false when it does not fit one launch (before anything is written)
static inline bool rg_grid(int nrow, int heads, int rpb, dim3 *grid)
{
    const int64_t blocks = ((int64_t) nrow * heads + rpb - 1) / rpb;
    if (blocks > INT32_MAX) return false;
    *grid = dim3((unsigned) blocks);
    return true;
}

// One launch of a kernel family with <VEC, DROP> instances over the (row, head) units of a: VEC from the alignment of ptrs and
// lds, DROP from a.drop.on.  kernel(vec, drop) names the instance for two std::bool_constant arguments.
template <typename T, int LPR, class Args, class Family>
static inline hipError_t rg_launch(const Args &a, hipStream_t s, std::initializer_list<const void *> ptrs,
                                   std::initializer_list<int64_t> lds, Family kernel)
{
    const bool vec = rg_aligned(ptrs, lds, Piece<T>::VW);
    dim3 grid;
    if (!rg_grid(a.nrow, a.heads, 256 / LPR, &grid)) return hipErrorInvalidValue;
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    void (*const k)(Args) = a.drop.on ? (vec ? kernel(yes, yes) : kernel(no, yes)) : (vec ? kernel(yes, no) : kernel(no, no));
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace crp
