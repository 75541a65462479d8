// pgx_block.h -- the lane-group and workgroup primitives that the stages share whatever they work on: the reductions over the
// lanes of a group and over a workgroup, the workgroup's exclusive scan and the scan of a whole array by one workgroup (the
// middle step of every compaction here: count, block_scan_array, rank), the LDS tally of roots per workgroup (k_tracks.hip,
// k_meshclean.hip), and the clamp of a count that the device reads.  Nothing here knows a track graph, a cloud or a mesh.
// Internal to libpgx.so; DESIGN.md section 14i.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __HIPCC__

__device__ __forceinline__ int pgx_clamp_count(int n, int max_n) { return n < 0 ? 0 : (n > max_n ? max_n : n); }

// ---- reductions over the G lanes of a group: xor butterflies, identical bits in every lane ----------------------------

__device__ __forceinline__ double nan_max(double a, double b)
{
    if (a != a || b != b) return __builtin_nan("");
    return a > b ? a : b;
}

template <int G> __device__ __forceinline__ double gsum(double x)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) x += __shfl_xor(x, m, G);
    return x;
}
template <int G> __device__ __forceinline__ int gsum_i(int x)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) x += __shfl_xor(x, m, G);
    return x;
}
template <int G> __device__ __forceinline__ double gmax(double x)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) x = nan_max(x, __shfl_xor(x, m, G));
    return x;
}

// Fixed-shape sum over a workgroup of 256 threads of NV values per thread: xor butterflies per wave, then the four waves in a
// fixed order; identical bits in every thread.  sh: NV rows of LDS.
template <int NV> __device__ __forceinline__ void block_sums(double (&v)[NV], double (*sh)[4])
{
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = gsum<64>(v[k]);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; k++) sh[k][w] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
    __syncthreads();
}

// block_sums' integer sibling: the sum of one count per thread over the workgroup of 256 threads, in every thread.  sh: 4 ints.
__device__ __forceinline__ int block_sum_i(int c, int *sh)
{
    c = gsum_i<64>(c);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    c = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return c;
}

// ... and the 64-bit one.  sh: 4 values.
__device__ __forceinline__ long long block_sum_ll(long long v, long long *sh)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return v;
}

// The exclusive prefix of one value per thread over a workgroup of NT threads, in thread order (shuffle-up scan per wave, then the
// waves in order), and the workgroup's total in every thread.  lds: NT / 64 values.  Two counts whose SUMS stay below 2^32 scan
// as one 64-bit value (hi << 32 | lo), as k_tracks.hip's (tracks, nodes) do: no carry crosses.
template <class T, int NT> __device__ __forceinline__ T block_excl_scan(T v, T *lds, T &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        const T s = lds[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// One workgroup of NT threads, every thread of it: the exclusive scan of n values, NT at a time with a running carry:
// store(j, load(0) + .. + load(j - 1)) for j < n, and the sum of all n in every thread.  lds: NT / 64 values.  A store may go
// where a load came from.  What follows the scan (a report, a status bit, the closing offset) is the caller's.
template <class T, int NT, class Load, class Store> __device__ __forceinline__ T block_scan_array(int n, T *lds, Load load, Store store)
{
    T carry = 0;
    for (int base = 0; base < n; base += NT) {
        const int j = base + (int)threadIdx.x;
        T tot;
        const T ex = block_excl_scan<T, NT>(j < n ? load(j) : (T)0, lds, tot);
        if (j < n) store(j, carry + ex);
        carry += tot;
    }
    return carry;
}

// ... of plain arrays: out[j] = in[0] + .. + in[j - 1] (out may be in); stride: the arrays' step in elements, for interleaved values
template <class T, int NT> __device__ __forceinline__ T block_scan_array(const T *in, T *out, int n, T *lds, size_t stride = 1)
{
    return block_scan_array<T, NT>(n, lds, [&](int j) { return in[j * stride]; }, [&](int j, T v) { out[j * stride] = v; });
}

// ---- the tally of a workgroup's roots in LDS --------------------------------------------------------------------------
// hkey / hcnt / hmin of `slots` entries (a power of two, more than the roots a workgroup adds between two flushes), cleared to
// BLOCK_TALLY_EMPTY / 0 / INT_MAX: root r counted once more, lo into the minimum kept for it.  True when r claimed a new entry.
// The owner flushes one global atomic per entry in use, not one per thread: same-address global atomics serialise.

constexpr uint32_t BLOCK_TALLY_EMPTY = 0xFFFFFFFFu;

__device__ __forceinline__ bool block_tally_add(uint32_t *hkey, int *hcnt, int *hmin, int slots, int r, int lo)
{
    uint32_t h = ((uint32_t)r * 2654435761u) >> 9;
    for (;;) {
        h &= (uint32_t)(slots - 1);
        const uint32_t old = atomicCAS(&hkey[h], BLOCK_TALLY_EMPTY, (uint32_t)r);
        if (old == BLOCK_TALLY_EMPTY || old == (uint32_t)r) {
            atomicAdd(&hcnt[h], 1);
            atomicMin(&hmin[h], lo);
            return old == BLOCK_TALLY_EMPTY;
        }
        h++;
    }
}

#endif // __HIPCC__
