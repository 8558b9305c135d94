// row_kernels.hip -- index-list row gather / scatter and transpose for gfx950.
//
// These replace the OpenMP pack / unpack loops of the reference's B exchange
// (/root/reference/src/rowpara_spmm.c:232-262 pack, :313-344 unpack) and the
// strided rectangle copy of /root/reference/src/utils.c:92-119.  Pure byte
// movement: 16-byte accesses per lane, consecutive lanes on consecutive
// addresses, grid-stride so that a launch is capped at ~8 blocks per CU.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include "kernels.h"

namespace crp {

typedef double d2 __attribute__((ext_vector_type(2)));

static inline int grid_for(int64_t work)
{
    int64_t blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (int) blocks;
}

// Row-major: rows are contiguous runs of n doubles.  VW = 2 uses 16-byte accesses.
// GATHER: dst[i] = src[ridx[i]];  !GATHER: dst[ridx[i]] = src[i].
template <int VW, bool GATHER>
__global__ __launch_bounds__(256) void move_rows_rm_kernel(
    const int64_t nidx, const int cpr /* chunks per row */, const int *__restrict__ ridx,
    const double *__restrict__ src, const int64_t lds, double *__restrict__ dst, const int64_t ldd)
{
    const int64_t total = nidx * (int64_t) cpr;
    for (int64_t t = (int64_t) blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t) gridDim.x * 256)
    {
        const int64_t i = t / cpr;
        const int     c = (int) (t - i * cpr) * VW;
        const int64_t r = ridx[i];
        const int64_t srow = GATHER ? r : i;
        const int64_t drow = GATHER ? i : r;
        if constexpr (VW == 2)
        {
            const d2 v = *reinterpret_cast<const d2 *>(src + srow * lds + c);
            *reinterpret_cast<d2 *>(dst + drow * ldd + c) = v;
        }
        else
        {
            dst[drow * ldd + c] = src[srow * lds + c];
        }
    }
}

// Column-major: element (r, j) at r + j*ld; consecutive lanes walk the index list.
template <bool GATHER>
__global__ __launch_bounds__(256) void move_rows_cm_kernel(
    const int64_t nidx, const int n, const int *__restrict__ ridx,
    const double *__restrict__ src, const int64_t lds, double *__restrict__ dst, const int64_t ldd)
{
    const int64_t total = nidx * (int64_t) n;
    for (int64_t t = (int64_t) blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t) gridDim.x * 256)
    {
        const int64_t j = t / nidx;
        const int64_t i = t - j * nidx;
        const int64_t r = ridx[i];
        if (GATHER) dst[i + j * ldd] = src[r + j * lds];
        else        dst[r + j * ldd] = src[i + j * lds];
    }
}

template <bool GATHER>
static hipError_t move_rows(int layout, int nidx, int n, const int *ridx, const double *src, int64_t lds,
                            double *dst, int64_t ldd, hipStream_t s)
{
    if (nidx <= 0 || n <= 0) return hipSuccess;
    if (layout == 0)
    {
        const bool vec2 = (n % 2 == 0) && (lds % 2 == 0) && (ldd % 2 == 0) &&
                          (((uintptr_t) src | (uintptr_t) dst) % 16 == 0);
        if (vec2)
        {
            const int cpr = n / 2;
            hipLaunchKernelGGL((move_rows_rm_kernel<2, GATHER>), dim3(grid_for((int64_t) nidx * cpr)), dim3(256), 0, s,
                               (int64_t) nidx, cpr, ridx, src, lds, dst, ldd);
        }
        else
        {
            hipLaunchKernelGGL((move_rows_rm_kernel<1, GATHER>), dim3(grid_for((int64_t) nidx * n)), dim3(256), 0, s,
                               (int64_t) nidx, n, ridx, src, lds, dst, ldd);
        }
    }
    else
    {
        hipLaunchKernelGGL((move_rows_cm_kernel<GATHER>), dim3(grid_for((int64_t) nidx * n)), dim3(256), 0, s,
                           (int64_t) nidx, n, ridx, src, lds, dst, ldd);
    }
    return hipGetLastError();
}

hipError_t gather_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, int64_t lds,
                           double *dst, int64_t ldd, hipStream_t s)
{
    return move_rows<true>(layout, nidx, n, ridx, src, lds, dst, ldd, s);
}

hipError_t scatter_rows_f64(int layout, int nidx, int n, const int *ridx, const double *src, int64_t lds,
                            double *dst, int64_t ldd, hipStream_t s)
{
    return move_rows<false>(layout, nidx, n, ridx, src, lds, dst, ldd, s);
}

// 32x32 tile transpose through LDS; 33-double row pitch keeps the column reads
// off a single bank.  dst[c][r] = src[r][c].
__global__ __launch_bounds__(256) void transpose_f64_kernel(
    const int nrow, const int ncol, const double *__restrict__ src, const int64_t lds,
    double *__restrict__ dst, const int64_t ldd)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;   // 32 x 8
    const int64_t r0 = (int64_t) blockIdx.x * 32, c0 = (int64_t) blockIdx.y * 32;   // rows on grid.x (2^31 limit)
#pragma unroll
    for (int k = 0; k < 32; k += 8)
    {
        const int64_t r = r0 + ty + k, c = c0 + tx;
        if (r < nrow && c < ncol) tile[ty + k][tx] = src[r * lds + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8)
    {
        const int64_t c = c0 + ty + k, r = r0 + tx;
        if (r < nrow && c < ncol) dst[c * ldd + r] = tile[tx][ty + k];
    }
}

hipError_t transpose_f64(int nrow, int ncol, const double *src, int64_t lds, double *dst, int64_t ldd,
                         hipStream_t s)
{
    if (nrow <= 0 || ncol <= 0) return hipSuccess;
    dim3 grid((nrow + 31) / 32, (ncol + 31) / 32);
    hipLaunchKernelGGL(transpose_f64_kernel, grid, dim3(256), 0, s, nrow, ncol, src, lds, dst, ldd);
    return hipGetLastError();
}

// ---- fp32 row movement and transpose (the fp32 exec of the engines; the fp64 kernels above are left as they are)
//
// Row-major: a workgroup of 256 lanes takes 256 / TPR rows at a time, TPR lanes per row walk the row's chunks of VW
// floats (VW = 4: 16-byte accesses).  TPR is the smallest power of two >= the chunks of a row (at most 256), so a row of
// 1024 floats is one workgroup of 16-byte accesses, and a row of 24 floats is 8 lanes of a 32-row group: every lane
// moves whole chunks, the row index is read once per row, and no lane divides.
template <int VW, int TPR, bool GATHER>
__global__ __launch_bounds__(256) void move_rows_rm_f32_kernel(
    const int nidx, const int cpr /* chunks per row */, const int *__restrict__ ridx,
    const float *__restrict__ src, const int64_t lds, float *__restrict__ dst, const int64_t ldd)
{
    typedef float fv __attribute__((ext_vector_type(VW)));
    constexpr int RPB = 256 / TPR;   // rows per workgroup and step
    const int lane = threadIdx.x % TPR;
    for (int64_t i = (int64_t) blockIdx.x * RPB + threadIdx.x / TPR; i < nidx; i += (int64_t) gridDim.x * RPB)
    {
        const int64_t r = ridx[i];
        const int64_t srow = GATHER ? r : i;
        const int64_t drow = GATHER ? i : r;
        const float *s = src + srow * lds;
        float *d = dst + drow * ldd;
        for (int c = lane; c < cpr; c += TPR)
        {
            if constexpr (VW == 1) d[c] = s[c];
            else *reinterpret_cast<fv *>(d + (int64_t) c * VW) = *reinterpret_cast<const fv *>(s + (int64_t) c * VW);
        }
    }
}

// Column-major: element (r, j) at r + j*ld; consecutive lanes walk the index list.
template <bool GATHER>
__global__ __launch_bounds__(256) void move_rows_cm_f32_kernel(
    const int64_t nidx, const int n, const int *__restrict__ ridx,
    const float *__restrict__ src, const int64_t lds, float *__restrict__ dst, const int64_t ldd)
{
    const int64_t total = nidx * (int64_t) n;
    for (int64_t t = (int64_t) blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t) gridDim.x * 256)
    {
        const int64_t j = t / nidx;
        const int64_t i = t - j * nidx;
        const int64_t r = ridx[i];
        if (GATHER) dst[i + j * ldd] = src[r + j * lds];
        else        dst[r + j * ldd] = src[i + j * lds];
    }
}

template <int VW, int TPR, bool GATHER>
static void launch_rm_f32(int nidx, int cpr, const int *ridx, const float *src, int64_t lds, float *dst, int64_t ldd,
                          hipStream_t s)
{
    const int blocks = grid_for((int64_t) nidx * TPR);   // 256 / TPR rows per workgroup, capped like every launch here
    hipLaunchKernelGGL((move_rows_rm_f32_kernel<VW, TPR, GATHER>), dim3(blocks), dim3(256), 0, s, nidx, cpr, ridx, src,
                       lds, dst, ldd);
}

template <int VW, bool GATHER>
static void move_rows_rm_f32(int nidx, int cpr, const int *ridx, const float *src, int64_t lds, float *dst, int64_t ldd,
                             hipStream_t s)
{
    if (cpr <= 4)        launch_rm_f32<VW, 4, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else if (cpr <= 8)   launch_rm_f32<VW, 8, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else if (cpr <= 16)  launch_rm_f32<VW, 16, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else if (cpr <= 32)  launch_rm_f32<VW, 32, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else if (cpr <= 64)  launch_rm_f32<VW, 64, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else if (cpr <= 128) launch_rm_f32<VW, 128, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
    else                 launch_rm_f32<VW, 256, GATHER>(nidx, cpr, ridx, src, lds, dst, ldd, s);
}

template <bool GATHER>
static hipError_t move_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, int64_t lds,
                                float *dst, int64_t ldd, hipStream_t s)
{
    if (nidx <= 0 || n <= 0) return hipSuccess;
    if (layout == 0)
    {
        const uintptr_t a = (uintptr_t) src | (uintptr_t) dst;
        if (n % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && a % 16 == 0)
            move_rows_rm_f32<4, GATHER>(nidx, n / 4, ridx, src, lds, dst, ldd, s);
        else if (n % 2 == 0 && lds % 2 == 0 && ldd % 2 == 0 && a % 8 == 0)
            move_rows_rm_f32<2, GATHER>(nidx, n / 2, ridx, src, lds, dst, ldd, s);
        else
            move_rows_rm_f32<1, GATHER>(nidx, n, ridx, src, lds, dst, ldd, s);
    }
    else
    {
        hipLaunchKernelGGL((move_rows_cm_f32_kernel<GATHER>), dim3(grid_for((int64_t) nidx * n)), dim3(256), 0, s,
                           (int64_t) nidx, n, ridx, src, lds, dst, ldd);
    }
    return hipGetLastError();
}

hipError_t gather_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, int64_t lds,
                           float *dst, int64_t ldd, hipStream_t s)
{
    return move_rows_f32<true>(layout, nidx, n, ridx, src, lds, dst, ldd, s);
}

hipError_t scatter_rows_f32(int layout, int nidx, int n, const int *ridx, const float *src, int64_t lds,
                            float *dst, int64_t ldd, hipStream_t s)
{
    return move_rows_f32<false>(layout, nidx, n, ridx, src, lds, dst, ldd, s);
}

// 32x32 tile transpose through LDS; the 33-float row pitch puts the 32 elements of a tile column on 32 different banks.
// dst[c][r] = src[r][c].
__global__ __launch_bounds__(256) void transpose_f32_kernel(
    const int nrow, const int ncol, const float *__restrict__ src, const int64_t lds,
    float *__restrict__ dst, const int64_t ldd)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;   // 32 x 8
    const int64_t r0 = (int64_t) blockIdx.x * 32, c0 = (int64_t) blockIdx.y * 32;   // rows on grid.x (2^31 limit)
#pragma unroll
    for (int k = 0; k < 32; k += 8)
    {
        const int64_t r = r0 + ty + k, c = c0 + tx;
        if (r < nrow && c < ncol) tile[ty + k][tx] = src[r * lds + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8)
    {
        const int64_t c = c0 + ty + k, r = r0 + tx;
        if (r < nrow && c < ncol) dst[c * ldd + r] = tile[tx][ty + k];
    }
}

hipError_t transpose_f32(int nrow, int ncol, const float *src, int64_t lds, float *dst, int64_t ldd, hipStream_t s)
{
    if (nrow <= 0 || ncol <= 0) return hipSuccess;
    dim3 grid((nrow + 31) / 32, (ncol + 31) / 32);
    hipLaunchKernelGGL(transpose_f32_kernel, grid, dim3(256), 0, s, nrow, ncol, src, lds, dst, ldd);
    return hipGetLastError();
}

// dst[map[i]] = src[i]: refresh the values of a derived sparse format from new CSR values
__global__ __launch_bounds__(256) void scatter_vals_kernel(const int64_t n, const uint32_t *__restrict__ map,
                                                           const double *__restrict__ src, double *__restrict__ dst)
{
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) dst[map[i]] = src[i];
}

hipError_t scatter_vals_f64(int64_t n, const uint32_t *map, const double *src, double *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_vals_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, map, src, dst);
    return hipGetLastError();
}

// dst[i] = (double) src[map ? map[i] : i]: the values of a transposed handle from values in the original order
// (crp_csr_dev_update_values), and the parts / the transposed order of an engine's device value update (crp_gather_vals_*).
// Widening fp32 to fp64 is exact, so the fp32 copies a handle derives from dst are the caller's fp32 bits again.
template <class S>
__global__ __launch_bounds__(256) void gather_vals_kernel(const int64_t n, const int *__restrict__ map, const S *__restrict__ src,
                                                          double *__restrict__ dst)
{
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256)
        dst[i] = (double) src[map ? (int64_t) map[i] : i];
}

template <class S> static hipError_t gather_vals(int64_t n, const int *map, const S *src, double *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((gather_vals_kernel<S>), dim3(grid_for(n)), dim3(256), 0, s, n, map, src, dst);
    return hipGetLastError();
}

hipError_t gather_vals_f64(int64_t n, const int *map, const double *src, double *dst, hipStream_t s)
{
    return gather_vals<double>(n, map, src, dst, s);
}

hipError_t gather_vals_f32_f64(int64_t n, const int *map, const float *src, double *dst, hipStream_t s)
{
    return gather_vals<float>(n, map, src, dst, s);
}

// Segmented accumulate: dst[seg_row[t]] += src[seg_pos[k]] for k = seg_ptr[t] .. seg_ptr[t + 1] - 1, in that order.  One
// thread owns a piece of VW elements of one destination row -- VW * sizeof(T) = 16 bytes, or one element -- and adds the
// segment's source rows one after the other: plain IEEE additions, element by element in the vector form too, so both
// instances give the same bits; the destination rows are distinct, so nothing races and the sum has one order.
template <class T, int VW>
__global__ __launch_bounds__(256) void scatter_add_rows_kernel(const int64_t nseg, const int cpr /* pieces per row */,
                                                               const int *__restrict__ seg_row, const int *__restrict__ seg_ptr,
                                                               const int *__restrict__ seg_pos, const T *__restrict__ src,
                                                               const int64_t lds, T *__restrict__ dst, const int64_t ldd)
{
    typedef T tv __attribute__((ext_vector_type(VW)));
    const int64_t total = nseg * (int64_t) cpr;
    for (int64_t x = (int64_t) blockIdx.x * 256 + threadIdx.x; x < total; x += (int64_t) gridDim.x * 256)
    {
        const int64_t t = x / cpr;
        const int     c = (int) (x - t * cpr) * VW;
        const int     k0 = seg_ptr[t], k1 = seg_ptr[t + 1];
        T *out = dst + (int64_t) seg_row[t] * ldd + c;
        if constexpr (VW > 1)
        {
            tv acc = *reinterpret_cast<const tv *>(out);
            for (int k = k0; k < k1; k++) acc += *reinterpret_cast<const tv *>(src + (int64_t) seg_pos[k] * lds + c);
            *reinterpret_cast<tv *>(out) = acc;
        }
        else
        {
            T acc = *out;
            for (int k = k0; k < k1; k++) acc += src[(int64_t) seg_pos[k] * lds + c];
            *out = acc;
        }
    }
}

// 16-byte pieces when n, both leading dimensions and both pointers keep every piece 16-byte aligned, single elements otherwise
template <class T>
static hipError_t scatter_add_rows(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const T *src,
                                   int64_t lds, T *dst, int64_t ldd, hipStream_t s)
{
    if (nseg <= 0 || n <= 0) return hipSuccess;
    constexpr int VW = 16 / (int) sizeof(T);
    const bool vec = (n % VW == 0) && (lds % VW == 0) && (ldd % VW == 0) && (((uintptr_t) src | (uintptr_t) dst) % 16 == 0);
    if (vec)
        hipLaunchKernelGGL((scatter_add_rows_kernel<T, VW>), dim3(grid_for((int64_t) nseg * (n / VW))), dim3(256), 0, s, (int64_t) nseg,
                           n / VW, seg_row, seg_ptr, seg_pos, src, lds, dst, ldd);
    else
        hipLaunchKernelGGL((scatter_add_rows_kernel<T, 1>), dim3(grid_for((int64_t) nseg * n)), dim3(256), 0, s, (int64_t) nseg, n, seg_row,
                           seg_ptr, seg_pos, src, lds, dst, ldd);
    return hipGetLastError();
}

hipError_t scatter_add_rows_f64(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const double *src,
                                int64_t lds, double *dst, int64_t ldd, hipStream_t s)
{
    return scatter_add_rows<double>(nseg, n, seg_row, seg_ptr, seg_pos, src, lds, dst, ldd, s);
}

hipError_t scatter_add_rows_f32(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, const float *src,
                                int64_t lds, float *dst, int64_t ldd, hipStream_t s)
{
    return scatter_add_rows<float>(nseg, n, seg_row, seg_ptr, seg_pos, src, lds, dst, ldd, s);
}

// Sum of segments: out[p] = ((src[p] + src[stride + p]) + src[2 * stride + p]) + ..., segment after segment in ascending
// order (the grid-row reduction of the 2D engine's SDDMM: segment j holds the partial dots grid column j formed).  One
// thread owns a piece of VW elements of out -- VW * sizeof(T) = 16 bytes, or one element -- reads that piece of every
// segment and adds them left to right: plain IEEE additions, element by element in the vector form too, so both instances
// give the same bits.  No atomics, no LDS; nseg = 1 is a copy.
template <class T, int VW>
__global__ __launch_bounds__(256) void sum_segments_kernel(const int nseg, const int64_t npiece, const T *__restrict__ src,
                                                           const int64_t seg_stride, T *__restrict__ out)
{
    typedef T tv __attribute__((ext_vector_type(VW)));
    for (int64_t x = (int64_t) blockIdx.x * 256 + threadIdx.x; x < npiece; x += (int64_t) gridDim.x * 256)
    {
        const T *p = src + x * VW;
        if constexpr (VW > 1)
        {
            tv acc = *reinterpret_cast<const tv *>(p);
            for (int j = 1; j < nseg; j++) acc += *reinterpret_cast<const tv *>(p + (int64_t) j * seg_stride);
            *reinterpret_cast<tv *>(out + x * VW) = acc;
        }
        else
        {
            T acc = *p;
            for (int j = 1; j < nseg; j++) acc += p[(int64_t) j * seg_stride];
            out[x] = acc;
        }
    }
}

// 16-byte pieces when src, out and the segment stride keep every piece 16-byte aligned; the elements that do not fill a
// piece (and everything, when the alignment does not allow pieces) go to the element-wise instance.
template <class T>
static hipError_t sum_segments(int nseg, int64_t len, const T *src, int64_t seg_stride, T *out, hipStream_t s)
{
    if (nseg <= 0 || len <= 0) return hipSuccess;
    constexpr int VW = 16 / (int) sizeof(T);
    const bool vec = (((uintptr_t) src | (uintptr_t) out) % 16 == 0) && (nseg == 1 || seg_stride % VW == 0);
    const int64_t npiece = vec ? len / VW : 0, body = npiece * VW;
    if (npiece > 0)
        hipLaunchKernelGGL((sum_segments_kernel<T, VW>), dim3(grid_for(npiece)), dim3(256), 0, s, nseg, npiece, src, seg_stride, out);
    if (len > body)
        hipLaunchKernelGGL((sum_segments_kernel<T, 1>), dim3(grid_for(len - body)), dim3(256), 0, s, nseg, len - body, src + body,
                           seg_stride, out + body);
    return hipGetLastError();
}

hipError_t sum_segments_f64(int nseg, int64_t len, const double *src, int64_t seg_stride, double *out, hipStream_t s)
{
    return sum_segments<double>(nseg, len, src, seg_stride, out, s);
}

hipError_t sum_segments_f32(int nseg, int64_t len, const float *src, int64_t seg_stride, float *out, hipStream_t s)
{
    return sum_segments<float>(nseg, len, src, seg_stride, out, s);
}

// Column sums of a row-major nrow x n array (the reduction of the GATv2 backward's da_part over the rows): block b of 256
// consecutive rows is summed per column from +0 in ascending row by one thread -- work[b * n + j], coalesced across the columns --
// and sum_segments adds the blocks left to right in ascending b.  Plain IEEE additions of single elements: the bits are a function
// of (dtype, nrow, n, data) only.  No atomics, no LDS.  sum_segments alone would be one serial chain of nrow additions on n threads.
constexpr int COL_SUM_ROWS = 256;
template <class T>
__global__ __launch_bounds__(256) void col_block_sum_kernel(const int nrow, const int n, const int ncb, const T *__restrict__ src,
                                                            const int64_t lds, T *__restrict__ work)
{
    const int blk = (int) (blockIdx.x / (unsigned) ncb);
    const int col = (int) (blockIdx.x % (unsigned) ncb) * 256 + (int) threadIdx.x;
    if (col >= n) return;
    const int r0 = blk * COL_SUM_ROWS, r1 = min(nrow, r0 + COL_SUM_ROWS);
    T acc = (T) 0;
    for (int r = r0; r < r1; r++) acc = acc + src[(int64_t) r * lds + col];
    work[(int64_t) blk * n + col] = acc;
}

template <class T>
static hipError_t col_sum(int nrow, int n, const T *src, int64_t lds, T *work, T *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (nrow <= 0) return hipMemsetAsync(out, 0, (size_t) n * sizeof(T), s);        // an empty sum: +0
    const int64_t nblk = ((int64_t) nrow + COL_SUM_ROWS - 1) / COL_SUM_ROWS, ncb = ((int64_t) n + 255) / 256;
    if (nblk * ncb > INT32_MAX) return hipErrorInvalidValue;            // before anything is written
    hipLaunchKernelGGL((col_block_sum_kernel<T>), dim3((unsigned) (nblk * ncb)), dim3(256), 0, s, nrow, n, (int) ncb, src, lds, work);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    return sum_segments<T>((int) nblk, n, work, n, out, s);
}

hipError_t col_sum_f64(int nrow, int n, const double *src, int64_t lds, double *work, double *out, hipStream_t s)
{
    return col_sum<double>(nrow, n, src, lds, work, out, s);
}

hipError_t col_sum_f32(int nrow, int n, const float *src, int64_t lds, float *work, float *out, hipStream_t s)
{
    return col_sum<float>(nrow, n, src, lds, work, out, s);
}

// fp32 copy of fp64 values (the fp32 path keeps A's values in fp64 as the caller gave them and derives its own copy)
__global__ void convert_f64_f32_kernel(const int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) dst[i] = (float) src[i];
}

hipError_t convert_f64_f32(int64_t n, const double *src, float *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(convert_f64_f32_kernel, dim3(blocks), dim3(256), 0, s, n, src, dst);
    return hipGetLastError();
}

// ---- exchange-overlap probe (tools/overlap_probe.py; SURVEY 8(e): does a transfer kernel make progress beside the product?)
// A stand-in for the transport's copy kernels: `blocks` workgroups of 256 threads copy n16 16-byte words and stamp the
// 100 MHz wall clock: stamps[0] = the earliest start of a workgroup, stamps[1] = the latest end.
__global__ __launch_bounds__(256) void probe_copy_kernel(const int64_t n16, const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                          unsigned long long *__restrict__ stamps)
{
    if (threadIdx.x == 0) atomicMin(&stamps[0], (unsigned long long) wall_clock64());
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t) gridDim.x * 256) dst[i] = src[i];
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&stamps[1], (unsigned long long) wall_clock64());
}

__global__ void probe_stamp_kernel(unsigned long long *__restrict__ out) { *out = (unsigned long long) wall_clock64(); }

hipError_t probe_copy(int64_t bytes, const void *src, void *dst, int blocks, unsigned long long *stamps, hipStream_t s)
{
    if (bytes <= 0 || blocks <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_copy_kernel, dim3(blocks), dim3(256), 0, s, bytes / 16, (const uint4 *) src, (uint4 *) dst, stamps);
    return hipGetLastError();
}

hipError_t probe_stamp(unsigned long long *out, hipStream_t s)
{
    hipLaunchKernelGGL(probe_stamp_kernel, dim3(1), dim3(1), 0, s, out);
    return hipGetLastError();
}

// ---- csr_mat_row_part_comm_size on the device (planner, /root/reference/src/spmat_part.c:38-64) -------------------------
// For a row partition rblk (nblk + 1) and a partition xd of the columns (nblk + 1): comm[b] = distinct columns the rows of
// block b name that lie outside [xd[b], xd[b + 1]).  One bitmap of ncol bits per block: pass 1 sets the bit of every nonzero
// (one wave per row; the row's block by binary search), pass 2 counts the set bits outside the block's own range.
// Integer work: bit-exact against the reference.
__global__ void comm_mark_kernel(const int nrow, const int *__restrict__ rowptr, const int *__restrict__ colidx, const int nblk,
                                 const int *__restrict__ rblk, const long long words, unsigned *__restrict__ bits, int *__restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const long long wave0 = ((long long) blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = ((long long) gridDim.x * blockDim.x) >> 6;
    for (long long r = wave0; r < nrow; r += nwave)
    {
        int lo = 0, hi = nblk;                       // rblk[lo] <= r < rblk[hi]: the last block that starts at or before r
        while (hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if (rblk[mid] <= (int) r) lo = mid; else hi = mid;
        }
        unsigned *my = bits + (long long) lo * words;
        for (int p = rowptr[r] + lane; p < rowptr[r + 1]; p += 64)
        {
            const int c = colidx[p];
            if (c < 0) { *bad = 1; continue; }       // (a two-source index: not a column of the global matrix)
            atomicOr(my + (c >> 5), 1u << (c & 31));
        }
    }
}

__global__ void comm_count_kernel(const int ncol, const int nblk, const int *__restrict__ xd, const long long words,
                                  const unsigned *__restrict__ bits, int *__restrict__ comm)
{
    const int b = blockIdx.y;
    const int own0 = xd[b], own1 = xd[b + 1];
    int cnt = 0;
    for (long long w = (long long) blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (long long) gridDim.x * blockDim.x)
    {
        unsigned v = bits[(long long) b * words + w];
        if (v == 0) continue;
        const long long c0 = w << 5;
        // clear the bits of the block's own columns [own0, own1)
        if (c0 + 32 > own0 && c0 < own1)
        {
            const int lo = (int) std::max<long long>(own0 - c0, 0), hi = (int) std::min<long long>(own1 - c0, 32);
            const unsigned m = (hi - lo >= 32) ? 0xFFFFFFFFu : (((1u << (hi - lo)) - 1u) << lo);
            v &= ~m;
        }
        cnt += __popc(v);
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(comm + b, cnt);
    (void) ncol;
}

hipError_t row_part_comm_size(int nrow, int ncol, const int *rowptr, const int *colidx, int nblk, const int *rblk_dev, const int *xd_dev,
                              unsigned *bits, int *comm_dev, int *bad_dev, hipStream_t s)
{
    const long long words = ((long long) ncol + 31) / 32;
    if (nrow > 0)
    {
        const int blocks = (int) std::min<long long>(((long long) nrow + 3) / 4, 65536);
        hipLaunchKernelGGL(comm_mark_kernel, dim3(blocks), dim3(256), 0, s, nrow, rowptr, colidx, nblk, rblk_dev, words, bits, bad_dev);
    }
    if (words > 0)
    {
        const int bx = (int) std::min<long long>((words + 255) / 256, 1024);
        hipLaunchKernelGGL(comm_count_kernel, dim3(bx, nblk), dim3(256), 0, s, ncol, nblk, xd_dev, words, bits, comm_dev);
    }
    return hipGetLastError();
}

}  // namespace crp
