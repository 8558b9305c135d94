// scan_sort.h -- device helpers shared by permute_kernels.hip (P A P^T) and transpose_kernels.hip (A^T): the in-place
// exclusive scan of an int array and the pieces of the three-tier per-row sort of 64-bit keys (one wave in registers, one
// workgroup in LDS, one workgroup in a scratch buffer).  Everything is internal to the translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {
namespace devsort {

constexpr int WAVE = 64;
constexpr int LDS_PAIRS = 4096;         // largest row sorted in LDS (partition.py: PERMUTE_LDS_PAIRS)
constexpr int MID_THREADS = 256;
constexpr int LONG_THREADS = 1024;
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr uint64_t PAD = ~(uint64_t) 0;

__device__ inline int pow2_at_least(int x)
{
    int n = 1;
    while (n < x) n <<= 1;
    return n;
}

// ---- exclusive scan of x[0 .. n) in place
template <int NT>
__device__ inline int block_exclusive_scan(int v, int *s, int *total = nullptr)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1)
    {
        const int add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const int incl = s[tid];
    if (total) *total = s[NT - 1];
    __syncthreads();
    return incl - v;
}

static __global__ void __launch_bounds__(SCAN_THREADS) k_scan_tile_sums(int n, const int *__restrict__ x, int *bsum)
{
    __shared__ int s[SCAN_THREADS];
    const long long base = (long long) blockIdx.x * SCAN_TILE + (long long) threadIdx.x * SCAN_ITEMS;
    int v = 0;
    for (int j = 0; j < SCAN_ITEMS; j++)
        if (base + j < n) v += x[base + j];
    const int ex = block_exclusive_scan<SCAN_THREADS>(v, s);
    if (threadIdx.x == SCAN_THREADS - 1) bsum[blockIdx.x] = ex + v;
}

static __global__ void __launch_bounds__(1024) k_scan_block_sums(int nb, int *bsum)
{
    __shared__ int s[1024];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 1024)
    {
        const int b = b0 + (int) threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        int chunk = 0;
        const int ex = block_exclusive_scan<1024>(v, s, &chunk);
        if (b < nb) bsum[b] = carry + ex;
        carry += chunk;
    }
}

static __global__ void __launch_bounds__(SCAN_THREADS) k_scan_tile_apply(int n, int *x, const int *__restrict__ bsum)
{
    __shared__ int s[SCAN_THREADS];
    const long long base = (long long) blockIdx.x * SCAN_TILE + (long long) threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS], sum = 0;
    for (int j = 0; j < SCAN_ITEMS; j++)
    {
        v[j] = base + j < n ? x[base + j] : 0;
        sum += v[j];
    }
    int run = bsum[blockIdx.x] + block_exclusive_scan<SCAN_THREADS>(sum, s);
    for (int j = 0; j < SCAN_ITEMS; j++)
        if (base + j < n)
        {
            x[base + j] = run;
            run += v[j];
        }
}

// tiles of an n-entry scan (the size of its bsum work array)
static inline int scan_tiles(int n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

// x[0 .. n) := its exclusive scan, on stream st (tile sums, one workgroup over the tile sums, tiles again)
static inline hipError_t exclusive_scan_inplace(int n, int *x, int *bsum, hipStream_t st)
{
    const int nb = scan_tiles(n);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(nb), dim3(SCAN_THREADS), 0, st, n, x, bsum);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, st, nb, bsum);
    hipLaunchKernelGGL(k_scan_tile_apply, dim3(nb), dim3(SCAN_THREADS), 0, st, n, x, bsum);
    return hipGetLastError();
}

// ---- sorting 64-bit keys
__device__ inline uint64_t shfl_xor_u64(uint64_t v, int mask)
{
    const int lo = __shfl_xor((int) (uint32_t) v, mask), hi = __shfl_xor((int) (uint32_t) (v >> 32), mask);
    return ((uint64_t) (uint32_t) hi << 32) | (uint32_t) lo;
}

// one key per lane (PAD past the row's end), np2 = the power of two that holds the row: ascending over the lanes of a wave
__device__ inline uint64_t wave_bitonic(uint64_t key, int lane, int np2)
{
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
        {
            const uint64_t other = shfl_xor_u64(key, j);
            const bool up = (lane & k) == 0, lower = (lane & j) == 0;
            key = (lower == up) ? (key < other ? key : other) : (key < other ? other : key);
        }
    return key;
}

// bitonic sort of s[0 .. np2) (np2 a power of two) by the threads of one workgroup
__device__ inline void block_bitonic(uint64_t *s, int np2)
{
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
        {
            for (int t = threadIdx.x; t < np2; t += blockDim.x)
            {
                const int p = t ^ j;
                if (p > t)
                {
                    const uint64_t a = s[t], b = s[p];
                    if ((a > b) == ((t & k) == 0))
                    {
                        s[t] = b;
                        s[p] = a;
                    }
                }
            }
            __syncthreads();
        }
}

}  // namespace devsort
}  // namespace crp
