// softmax_kernels.hip -- row softmax over a CSR pattern (edge softmax) and its Jacobian product for gfx950 (MI355X, wave64),
// fp64 and fp32.  For every row r with entries p in [rowptr[r], rowptr[r + 1]):
//     forward :  m = max_p s[p],  e_p = exp(s[p] - m),  y[p] = e_p / sum_q e_q
//     backward:  D = sum_q y[q] * dy[q] (FMAs),  ds[p] = y[p] * (dy[p] - D)
// Streaming work: 2 nnz sizeof(T) + 4 (nrow + 1) bytes forward (3 nnz sizeof(T) backward), no atomics, no LDS, no partial
// result in memory.  A group of LPR lanes (8, 16, 32 or 64) owns a row and reads it coalesced, LPR consecutive entries per
// load.  A row of up to 8 LPR entries is read once and kept in registers (8 values per lane); a longer row makes its passes
// over memory (forward: max, sum, write; backward: sum, write), which the L2 serves.  Any row length works on any group: a
// 70 000-entry row on 8 lanes is 8750 steps per pass.
//
// ONE KERNEL PER (dtype, direction).  The raw entry points (include/crpspmm_hip.h) receive the row pointer as a device array
// and are asynchronous, so the host cannot know the mean row length without a synchronising copy.  The kernel therefore
// picks LPR itself, from (rowptr[nrow] - rowptr[0]) / nrow -- two scalar loads, uniform over the launch -- and branches to
// the instance; the grid is a fixed number of workgroups that stride over the row groups.
//
// SPECIAL CASES.  An empty row reads and writes nothing.  s[p] = -inf is a masked edge: exp(-inf - m) is exactly 0.  A row
// whose entries are all -inf (m == -inf) writes zeros.  A row of one finite entry gives exp(0) / exp(0) = 1 exactly.  A row
// that holds NaN or +inf has unspecified outputs, in that row only.
//
// FIXED ORDER.  The sums (of e, of y dy) are formed in an order that is a function of the dtype only: 64 strided partials,
// partial k adding entries k, k + 64, k + 128, ... of the row in ascending order from +0 (the backward with FMAs), which
// then meet in the balanced binary tree over k (k with k ^ 1, then k ^ 2, ... k ^ 32), every node one IEEE addition.  An
// instance with LPR < 64 keeps A = 64 / LPR partials per lane (partial k in lane k % LPR, slot k / LPR), runs the tree's
// low log2(LPR) levels across lanes for every slot and its high levels inside the lane.  Entries past the row's end add
// +0 (forward) or fma(0, 0, acc) (backward), which is exact, so every instance and both row paths form the same tree: a
// row's bits do not depend on its position, the row pointer's first value, pointer alignment, the instance that ran or the
// other rows of the call.  The maximum is order-free.  exp / expf are the device library's; the division is IEEE.
//
// ALIASING.  Exact aliasing is allowed (y == s; ds == dy or ds == y), partial overlap is not.  Every element is read and
// later written by the same lane.  A row kept in registers is read entirely before its first write; in a longer row every
// element's last read precedes its own write.  Hence no __restrict__ on the value arrays.
#include <algorithm>
#include "row_group.h"

namespace crp {

constexpr int SM_KEEP = 8;                  // values a lane keeps of a register row

template <typename T, int LPR>
__device__ __forceinline__ T sm_group_max(T m)
{
#pragma unroll
    for (int mask = 1; mask < LPR; mask <<= 1) m = fmax(m, __shfl_xor(m, mask, LPR));
    return m;
}

// the tree over the 64 partials: low levels across the group's lanes (slot by slot), high levels inside the lane
template <typename T, int LPR>
__device__ __forceinline__ T sm_group_sum(T (&acc)[64 / LPR])
{
    constexpr int A = 64 / LPR;
#pragma unroll
    for (int j = 0; j < A; j++)
#pragma unroll
        for (int mask = 1; mask < LPR; mask <<= 1) acc[j] = acc[j] + __shfl_xor(acc[j], mask, LPR);
#pragma unroll
    for (int step = 1; step < A; step <<= 1)
#pragma unroll
        for (int j = 0; j < A; j += 2 * step) acc[j] = acc[j] + acc[j + step];
    return acc[0];
}

template <typename T, int LPR>
__device__ __forceinline__ void softmax_fwd_rows(const int nrow, const int *__restrict__ rowptr, const T *s, T *y)
{
    constexpr int A = 64 / LPR, RPB = 256 / LPR;
    const int l = threadIdx.x % LPR;
    const T ninf = rg_ninf<T>();
    for (int64_t row = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR; row < nrow; row += (int64_t) gridDim.x * RPB)
    {
        const int p0 = rowptr[row];
        const int64_t L = (int64_t) rowptr[row + 1] - p0;
        if (L <= 0) continue;
        const T *sr = s + p0;
        T *yr = y + p0;
        T acc[A];
#pragma unroll
        for (int j = 0; j < A; j++) acc[j] = (T) 0;
        if (L <= SM_KEEP * LPR)
        {
            T v[SM_KEEP];
            T m = ninf;
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++)
            {
                const int i = r * LPR + l;
                v[r] = (i < L) ? sr[i] : ninf;
                m = fmax(m, v[r]);
            }
            m = sm_group_max<T, LPR>(m);
            if (m == ninf)                                  // every entry masked: zeros, not exp(-inf + inf)
            {
#pragma unroll
                for (int r = 0; r < SM_KEEP; r++)
                    if (r * LPR + l < L) yr[r * LPR + l] = (T) 0;
                continue;
            }
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++)
            {
                if (r * LPR < L)                            // (group-uniform; a skipped step would add +0)
                {
                    v[r] = rg_exp(v[r] - m);                // past the end: exp(-inf) = +0
                    acc[r % A] = acc[r % A] + v[r];
                }
            }
            const T sum = sm_group_sum<T, LPR>(acc);
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++)
                if (r * LPR + l < L) yr[r * LPR + l] = v[r] / sum;
        }
        else
        {
            T m = ninf;
            for (int64_t base = 0; base < L; base += 64)
#pragma unroll
                for (int j = 0; j < A; j++)
                {
                    const int64_t i = base + j * LPR + l;
                    m = fmax(m, (i < L) ? sr[i] : ninf);
                }
            m = sm_group_max<T, LPR>(m);
            if (m == ninf)
            {
                for (int64_t i = l; i < L; i += LPR) yr[i] = (T) 0;
                continue;
            }
            for (int64_t base = 0; base < L; base += 64)
#pragma unroll
                for (int j = 0; j < A; j++)
                {
                    const int64_t i = base + j * LPR + l;
                    acc[j] = acc[j] + rg_exp(((i < L) ? sr[i] : ninf) - m);
                }
            const T sum = sm_group_sum<T, LPR>(acc);
            for (int64_t i = l; i < L; i += LPR) yr[i] = rg_exp(sr[i] - m) / sum;
        }
    }
}

template <typename T, int LPR>
__device__ __forceinline__ void softmax_bwd_rows(const int nrow, const int *__restrict__ rowptr, const T *y, const T *dy, T *ds)
{
    constexpr int A = 64 / LPR, RPB = 256 / LPR;
    const int l = threadIdx.x % LPR;
    for (int64_t row = (int64_t) blockIdx.x * RPB + threadIdx.x / LPR; row < nrow; row += (int64_t) gridDim.x * RPB)
    {
        const int p0 = rowptr[row];
        const int64_t L = (int64_t) rowptr[row + 1] - p0;
        if (L <= 0) continue;
        const T *yr = y + p0, *gr = dy + p0;
        T *dr = ds + p0;
        T acc[A];
#pragma unroll
        for (int j = 0; j < A; j++) acc[j] = (T) 0;
        if (L <= SM_KEEP * LPR)
        {
            T v[SM_KEEP], g[SM_KEEP];
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++)
            {
                const int i = r * LPR + l;
                v[r] = (i < L) ? yr[i] : (T) 0;
                g[r] = (i < L) ? gr[i] : (T) 0;
            }
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++) acc[r % A] = fma(v[r], g[r], acc[r % A]);     // past the end: fma(0, 0, acc) = acc
            const T D = sm_group_sum<T, LPR>(acc);
#pragma unroll
            for (int r = 0; r < SM_KEEP; r++)
                if (r * LPR + l < L) dr[r * LPR + l] = v[r] * (g[r] - D);
        }
        else
        {
            for (int64_t base = 0; base < L; base += 64)
#pragma unroll
                for (int j = 0; j < A; j++)
                {
                    const int64_t i = base + j * LPR + l;
                    const bool in = i < L;
                    acc[j] = fma(in ? yr[i] : (T) 0, in ? gr[i] : (T) 0, acc[j]);
                }
            const T D = sm_group_sum<T, LPR>(acc);
            for (int64_t i = l; i < L; i += LPR)
            {
                const T yv = yr[i], gv = gr[i];
                dr[i] = yv * (gv - D);
            }
        }
    }
}

// The group size, from the mean row length of the launch (uniform: two scalar loads): short rows take small groups so that
// most of a wave does not idle.  The boundaries sit at 1.5 x the group below.
__device__ __forceinline__ int sm_pick_lpr(const int nrow, const int *__restrict__ rowptr)
{
    const int64_t nnz = (int64_t) rowptr[nrow] - rowptr[0];
    if (nnz <= 12 * (int64_t) nrow) return 8;
    if (nnz <= 24 * (int64_t) nrow) return 16;
    if (nnz <= 48 * (int64_t) nrow) return 32;
    return 64;
}

template <typename T>
__global__ __launch_bounds__(256) void row_softmax_kernel(const int nrow, const int *__restrict__ rowptr, const T *s, T *y)
{
    switch (sm_pick_lpr(nrow, rowptr))
    {
    case 8:  softmax_fwd_rows<T, 8>(nrow, rowptr, s, y); break;
    case 16: softmax_fwd_rows<T, 16>(nrow, rowptr, s, y); break;
    case 32: softmax_fwd_rows<T, 32>(nrow, rowptr, s, y); break;
    default: softmax_fwd_rows<T, 64>(nrow, rowptr, s, y); break;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void row_softmax_bwd_kernel(const int nrow, const int *__restrict__ rowptr, const T *y, const T *dy,
                                                              T *ds)
{
    switch (sm_pick_lpr(nrow, rowptr))
    {
    case 8:  softmax_bwd_rows<T, 8>(nrow, rowptr, y, dy, ds); break;
    case 16: softmax_bwd_rows<T, 16>(nrow, rowptr, y, dy, ds); break;
    case 32: softmax_bwd_rows<T, 32>(nrow, rowptr, y, dy, ds); break;
    default: softmax_bwd_rows<T, 64>(nrow, rowptr, y, dy, ds); break;
    }
}

// enough workgroups for one row per wave (the 64-lane instance), at most 8 resident workgroups on each of 256 CUs: the
// workgroups stride over the row groups, so a smaller instance leaves the surplus ones without a row
static dim3 sm_grid(int nrow) { return dim3((unsigned) std::min<int64_t>(((int64_t) nrow + 3) / 4, 2048)); }

template <typename T>
static hipError_t row_softmax(int nrow, const int *rowptr, const T *s, T *y, hipStream_t st)
{
    if (nrow <= 0) return hipSuccess;
    hipLaunchKernelGGL((row_softmax_kernel<T>), sm_grid(nrow), dim3(256), 0, st, nrow, rowptr, s, y);
    return hipGetLastError();
}

template <typename T>
static hipError_t row_softmax_bwd(int nrow, const int *rowptr, const T *y, const T *dy, T *ds, hipStream_t st)
{
    if (nrow <= 0) return hipSuccess;
    hipLaunchKernelGGL((row_softmax_bwd_kernel<T>), sm_grid(nrow), dim3(256), 0, st, nrow, rowptr, y, dy, ds);
    return hipGetLastError();
}

hipError_t row_softmax_f64(int nrow, const int *rowptr, const double *s, double *y, hipStream_t st) { return row_softmax<double>(nrow, rowptr, s, y, st); }
hipError_t row_softmax_f32(int nrow, const int *rowptr, const float *s, float *y, hipStream_t st) { return row_softmax<float>(nrow, rowptr, s, y, st); }
hipError_t row_softmax_bwd_f64(int nrow, const int *rowptr, const double *y, const double *dy, double *ds, hipStream_t st)
{
    return row_softmax_bwd<double>(nrow, rowptr, y, dy, ds, st);
}
hipError_t row_softmax_bwd_f32(int nrow, const int *rowptr, const float *y, const float *dy, float *ds, hipStream_t st)
{
    return row_softmax_bwd<float>(nrow, rowptr, y, dy, ds, st);
}

}  // namespace crp
