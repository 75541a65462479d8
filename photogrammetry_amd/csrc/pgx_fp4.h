// pgx_fp4.h -- the Hamming distance of 256-bit descriptors (8 words) on the matrix pipe: the arithmetic that k_ham_fp4 and
// the residual-rows kernel (k_match_mfma.inc) and the nearest-column body of k_knn_fp4 and k_vocab_fp4 (pgx_fp4_nn.h) share.
// Internal to libpgx.so; device code only.
//
// hamming(a, b) = (K - a.b) / 2 for a, b in {-1,+1}^K (K = 256).  Every descriptor bit is expanded IN THE KERNEL
// (registers only, never in HBM) to the fp4 code of -+1 and fed to v_mfma_scale_f32_32x32x64_f8f6f4; the C input carries
// the argmin keys, so that BOTH argmins are plain integer maxima of accumulators -- no per-element masking:
//   * row side (best column of every row): a lane always holds the same rows and, in tile ct, column ct*32 + (lane & 31);
//     rbest[reg] = max(rbest[reg], acc[reg]) orders by (dot, smaller ct): ONE v_max per element, lanes are combined once,
//     after the last tile.
//   * column side (best row of every column): the 16 registers of a lane are 16 rows of one column; max over them
//     (v_max3 tree) orders by (dot, smaller row); the winner's tile field is swapped for the wave's row offset and posted
//     with an LDS atomic max.
// C/D lane map (cdna_hip_programming.md section 3): col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x8 = int __attribute__((ext_vector_type(8)));
using i32x16 = int __attribute__((ext_vector_type(16)));
using f32x16 = float __attribute__((ext_vector_type(16)));

// most columns one workgroup walks in one pass (LDS column-best array): 128 tiles = the 7-bit tile field of the key
constexpr int F4_CHUNK = 4096;

// ---- distance + argmin on the block-scaled FP4 matrix instruction ----------------------------------------------------
// v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 operands takes the cycles of the int8 32x32x32 form at twice the K: a
// descriptor bit becomes the fp4 code of -1 (set, 0xA) or +1 (clear, 0x2), four MFMAs cover the 256 bits, and the A
// operand's block scale (E8M0 byte 140 = 2^13) puts the dot product above the key field:
//     acc = 8192 * dot + C      exactly (|8192 * dot| <= 2^21, C < 2^14: all integers below 2^24 in f32)
// Products and sums of +-1 are exact in any order (tools/probe/fp4_probe.hip checks the instruction against popcounts
// over the whole distance range).  dot = 256 - 2 * hamming is even, so
// acc = 16384 * (dot / 2) + C: 14 key bits.  C[reg] of column tile ct = (127 - ct) << 7 | (127 - row position inside the
// wave's RT x 32 rows); both argmins are maxima of accumulators.
// Bit -> k-slot assignment: MFMA s takes word s (lanes 0..31) and word 4 + s (lanes 32..63) of the descriptor, so a lane
// loads ONE 16-byte quarter of its row / column; dword q of a fragment = ((word << q) & 0x88888888) | 0x22222222.
// No LDS operand staging and no barrier in the loop: every wavefront expands the columns it needs itself (the fp4
// expansion is 7 VALU per 32 bits; shared staging through LDS costs a workgroup barrier per 32-column tile: 35 % of the
// wave time of round 2's int8 kernel, which worked that way).  A wavefront keeps RT row tiles (RT x 16 fragment registers); LDS holds the column indices and the column
// bests of the workgroup.

// (x & m) | c in one instruction: the masks do not fit inline constants and a VOP3 takes no 32-bit literal on gfx9, so
// with literal masks the compiler emits v_and + v_or; with both constants in registers (made opaque once per kernel) it
// selects v_and_or_b32.  Plain C rather than inline asm: the hazard recogniser does not look inside an asm statement, and
// the result feeds an MFMA operand.
__device__ __forceinline__ int and_or(uint32_t x, int m, int c) { return (int)((x & (uint32_t)m) | (uint32_t)c); }

__device__ __forceinline__ void expand_fp4(uint32_t w, int km, int kc, int (&d)[4])
{
    d[0] = and_or(w, km, kc);
    d[1] = and_or(w << 1, km, kc);
    d[2] = and_or(w << 2, km, kc);
    d[3] = and_or(w << 3, km, kc);
}

// Accumulators carry a bias of 2^23 + 2^21, which puts every value into ONE binade, [2^23, 2^24): there f32 has unit spacing, the
// raw register is F4_RAW0 + (16384 * (dot / 2) + key) -- an affine image of the value -- so all maxima are INTEGER maxima of the
// raw registers (v_max_i32 / v_max3_i32; fmaxf would cost a canonicalising v_max x, x, x per operand on top: 204 instead of
// 64 max instructions per step, measured) and key fields are moved with integer adds on the raw bits, no conversions.
constexpr int F4_BIAS = (1 << 23) + (1 << 21);
constexpr int F4_RAW0 = 0x4B000000 + (1 << 21); // raw bits of (float)F4_BIAS
constexpr int F4_SCALE_A = 140; // E8M0: 2^(140 - 127) = 8192

__device__ __forceinline__ int max16i(const i32x16 &v)
{
    // 16 values in 8 instructions (7 v_max3 + 1 v_max; the tree of pairs that stood here before took 9)
    const int m0 = max(max(v[0], v[1]), v[2]), m1 = max(max(v[3], v[4]), v[5]), m2 = max(max(v[6], v[7]), v[8]);
    const int m3 = max(max(v[9], v[10]), v[11]), m4 = max(max(v[12], v[13]), v[14]);
    const int n0 = max(max(m0, m1), m2), n1 = max(max(m3, m4), v[15]);
    return max(n0, n1);
}

// signed maximum over each half (32 lanes) of a fully active wavefront by DPP row operations: quads, 8, 16 lanes, then
// row_bcast:15 carries rows 0 and 2 into rows 1 and 3.  Complete in lanes 16..31 and 48..63; no LDS crossbar traffic
// (the publishing step of k_ham_fp4 made 160 ds_bpermute round trips per wavefront before).
__device__ __forceinline__ int half_max_i32(int v)
{
    const int id = (int)0x80000000;
    v = max(v, __builtin_amdgcn_update_dpp(id, v, 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_update_dpp(id, v, 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_update_dpp(id, v, 0x141, 0xF, 0xF, false)); // row_half_mirror
    v = max(v, __builtin_amdgcn_update_dpp(id, v, 0x140, 0xF, 0xF, false)); // row_mirror
    v = max(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xA, 0xF, false)); // row_bcast:15 into rows 1, 3
    return v;
}
