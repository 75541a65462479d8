// pgx_pixel.h -- source pixels and Grayscale.FromRgba64, shared by k_image.hip (dewarp + grey) and k_fast.hip (the fused
// dewarp + grey + FAST tile kernel): one definition of the grey value, so both paths round the same way.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

__device__ __forceinline__ float gray_of(uint2 px)
{
    // px.x = R | G<<16, px.y = B | A<<16.  Sum order R, B, G as the C# writes it; the sum is
    // exact (< 2^24) and the division is one correctly rounded float32 divide.
    float r = (float)(px.x & 0xFFFFu), g = (float)(px.x >> 16), b = (float)(px.y & 0xFFFFu);
    float s = __fadd_rn(__fadd_rn(r, b), g);
    return __fdiv_rn(s, 196605.0f);
}

// 8-bit sources (PGX_SRC_RGBA8): a channel c becomes c * 257 = c | c << 8, the scaling an 8-bit image gets when it is
// loaded as Rgba64 (LocalImageReader.cs:22 via ImageSharp; 255 -> 65535).  Bytes r,g,b,a -> words r,r,g,g | b,b,a,a.
__device__ __forceinline__ uint2 widen8(uint32_t v)
{
    return make_uint2(__builtin_amdgcn_perm(v, v, 0x01010000u), __builtin_amdgcn_perm(v, v, 0x03030202u));
}

template <bool SRC8> struct SrcPix { using type = uint2; };
template <> struct SrcPix<true> { using type = uint32_t; };
template <bool SRC8> __device__ __forceinline__ uint2 load_px(const typename SrcPix<SRC8>::type *p);
template <> __device__ __forceinline__ uint2 load_px<false>(const uint2 *p) { return *p; }
template <> __device__ __forceinline__ uint2 load_px<true>(const uint32_t *p) { return widen8(*p); }

// the dewarp gather plan (k_dewarp_plan): one word per output pixel, sv * W + su of the map entry after its (ushort) wrap;
// this value where the wrapped source lies outside the image (W, H <= 65535: no real offset reaches it)
#define PGX_GATHER_OOB 0xFFFFFFFFu
