// pgx_ransac.h -- what the RANSAC stages share (k_pose.hip's fundamental-matrix RANSAC, k_register.hip, k_verify.hip): the
// counter-based sampler (splitmix64, the per-sample stream seed, the draw of distinct positions), the "first best sample"
// key with its wave, workgroup and row maxima, and the chunk-size rule of the launchers.  Internal to libpgx.so; DESIGN.md
// section 14e.
#pragma once

#include "pgx_internal.h"

// Samples per chunk: `cells` (row x sample) cells shared by `rows` rows, in whole scoring workgroups of `granule` samples (a
// power of two), never below one workgroup and never above n_samples rounded up to whole workgroups.
inline int ransac_chunk(long long cells, int rows, int granule, int n_samples)
{
    const long long g = granule;
    long long ch = cells / (rows > 0 ? rows : 1);
    ch = ch < g ? g : ch & ~(g - 1);
    const long long all = ((long long)n_samples + g - 1) & ~(g - 1);
    return (int)(ch < all ? ch : all);
}

#ifdef __HIPCC__

// ---- sampling ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t splitmix64(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the state of the stream of sample s of row `hi` (an image pair, a frame) under the call's seed
__device__ __forceinline__ uint64_t ransac_stream(uint64_t seed, int hi, int s)
{
    return seed ^ ((uint64_t)(uint32_t)hi << 32) ^ (uint64_t)(uint32_t)s * 0xD1B54A32D192ED03ull;
}

// id[0 .. count): distinct positions of an n-entry list (n >= count), each the stream's next draw that is not yet taken
__device__ __forceinline__ void ransac_draw(uint64_t &st, int n, int count, int *id)
{
    for (int k = 0; k < count; k++) {
        while (true) {
            const int c = (int)(splitmix64(st) % (uint64_t)n);
            bool dup = false;
            for (int j = 0; j < k; j++) dup |= id[j] == c;
            if (!dup) {
                id[k] = c;
                break;
            }
        }
    }
}

// ---- the key: the largest wins ----------------------------------------------------------------------------------------
// Most inliers first, then the smallest index (the first best sample); 0 means none and loses to every valid key.
// (count + 1) << 32 | ~index, so that a valid sample without inliers still beats none.

__device__ __forceinline__ unsigned long long ransac_key(bool valid, int count, int index)
{
    return valid ? ((unsigned long long)(count + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)index) : 0ull;
}
__device__ __forceinline__ int ransac_key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }
__device__ __forceinline__ int ransac_key_count(unsigned long long key) { return (int)(key >> 32) - 1; }

// the largest key of the wave, in every lane
__device__ __forceinline__ unsigned long long ransac_wave_max(unsigned long long key)
{
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) {
        const unsigned long long o = __shfl_xor(key, mk, 64);
        key = o > key ? o : key;
    }
    return key;
}

// the largest key of a workgroup of NT threads, valid on thread 0; sh: NT / 64 keys of LDS.  One barrier: what a caller
// writes to LDS ahead of the call is visible behind it.
template <int NT> __device__ __forceinline__ unsigned long long ransac_block_max(unsigned long long key, unsigned long long *sh)
{
    key = ransac_wave_max(key);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = key;
    __syncthreads();
    key = sh[0];
    for (int w = 1; w < NT / 64; w++) key = sh[w] > key ? sh[w] : key;
    return key;
}

// this thread's largest of the keys best[row * nblk + b], b in [b0, b1) strided by the workgroup's NT threads
template <int NT>
__device__ __forceinline__ unsigned long long ransac_row_max(const unsigned long long *best, int row, int nblk, int b0, int b1)
{
    unsigned long long key = 0;
    for (int b = b0 + threadIdx.x; b < b1; b += NT) {
        const unsigned long long k = best[(size_t)row * nblk + b];
        key = k > key ? k : key;
    }
    return key;
}

#endif // __HIPCC__
