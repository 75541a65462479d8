// pgx_fp4_nn.h -- the exact nearest columns of one block of rows on the FP4 matrix instruction: the body that k_knn_fp4
// (k_knn.hip: the rows and columns are two frames of an image pair) and k_vocab_fp4 (k_vocab.hip: the rows are one slot's
// descriptors, the columns the vocabulary) are both one call of.  The two kernels keep their block maps, counts and addresses;
// everything between the row loads and the write-out of (distance, column) is here, once.  256-bit descriptors (8 words);
// the arithmetic is pgx_fp4.h's: acc = F4_BIAS + 8192 * dot + C exactly, dot = 256 - 2 * hamming, and the C input carries a
// 14-bit key so that every selection is an INTEGER maximum of raw accumulator bits.  What differs from k_ham_fp4:
//   * a workgroup owns one row block and walks ALL columns, in chunks of at most 4096 (the key's 7-bit tile field): a row's
//     K <= 2 nearest columns are final inside the workgroup (merged over chunks as distance << 20 | column keys in LDS), so
//     there is no merge between workgroups on the row side and no distance matrix anywhere;
//   * row side: per accumulator element a lane keeps b1 >= b2; an element x makes b2 = max(b2, min(b1, x)) -- med3(b1, b2, x)
//     when b1 >= b2 -- and b1 = max(b1, x).  Keys of one lane differ in the tile field, so ties go to the smaller column;
//   * the 32 lanes that share a row are merged by the DPP pattern of half_max_i32 (pgx_fp4.h), with a top-2 merge at every step
//     for K == 2 (every step combines two disjoint lane sets, so no element is counted twice);
//   * column side (COL): k_ham_fp4's LDS column bests, published once per chunk with a global atomic min of
//     (distance << 20 | row) into the caller's column keys;
//   * padding: columns past the end of the ragged LAST tile of a chunk are masked on the row side (a duplicate of a real column
//     would come back as a second neighbour); row slots past the end repeat the last row as in k_ham_fp4 (a duplicate ties with
//     its original at a larger row position and never wins a column; its own row results are not written).
// Internal to libpgx.so; device code only.  DESIGN.md section 14b.
#pragma once

#include "pgx_fp4.h"
#include "pgx_pairlist.h"

#include <climits>

// one DPP step of the half-wave merge: (v1 > v2) with the partner lane's pair; lanes of masked-off rows see (INT_MIN, INT_MIN)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void top2_step(int &v1, int &v2)
{
    const int p1 = __builtin_amdgcn_update_dpp(INT_MIN, v1, CTRL, ROWMASK, 0xF, false);
    const int p2 = __builtin_amdgcn_update_dpp(INT_MIN, v2, CTRL, ROWMASK, 0xF, false);
    v2 = max(min(v1, p1), max(v2, p2));
    v1 = max(v1, p1);
}

// the K largest over each half (32 lanes) of a fully active wavefront, complete in lanes 16..31 and 48..63: half_max_i32, or
// its steps as top-2 merges
template <int K>
__device__ __forceinline__ void half_top(int &v1, int &v2)
{
    if (K == 1) {
        v1 = half_max_i32(v1);
    } else {
        top2_step<0xB1, 0xF>(v1, v2);  // quad_perm [1,0,3,2]
        top2_step<0x4E, 0xF>(v1, v2);  // quad_perm [2,3,0,1]
        top2_step<0x141, 0xF>(v1, v2); // row_half_mirror
        top2_step<0x140, 0xF>(v1, v2); // row_mirror
        top2_step<0x142, 0xA>(v1, v2); // row_bcast:15 into rows 1, 3
    }
}

// (d, index) keys in min order: merge the pair (n1 <= n2) into (k1 <= k2)
__device__ __forceinline__ void merge_min2(uint32_t &k1, uint32_t &k2, uint32_t n1, uint32_t n2)
{
    k2 = min(max(k1, n1), min(k2, n2));
    k1 = min(k1, n1);
}

// Rows rb .. rb + 4 * RT * 32 - 1 (those below n1) of the row set against the n2 >= 1 columns of the column set; one workgroup
// of 256 threads, RT row tiles per wavefront.  Row i's descriptor is rows + 8 i, column j's is cols + 8 (col0 + j): the column
// set is named by a descriptor index so that a caller's frame offset and the chunk's first column are added up before the scaling.
// oidx / odist: the row set's [row][K] outputs, entries past the K-th neighbour (-1, PGX_DIST_NONE); odist may be null.
// colkey (COL): the column set's keys, PGX_KEY_NONE on entry (k_knn_col_init).
template <int K, bool COL, int RT>
__device__ __forceinline__ void fp4_nn_block(const uint32_t *__restrict__ rows, int n1, const uint32_t *__restrict__ cols,
                                             size_t col0, int n2, int rb, int32_t *__restrict__ oidx, int32_t *__restrict__ odist,
                                             uint32_t *__restrict__ colkey)
{
    constexpr int WROWS = RT * 32, BM = 4 * WROWS;
    __shared__ int colbest[COL ? F4_CHUNK : 1];
    __shared__ uint32_t rowtop[K][BM]; // running (distance << 20 | column) keys of every row, min order; row owned by one lane
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    int km = (int)0x88888888, kc = 0x22222222;
    asm volatile("" : "+v"(km), "+v"(kc)); // pin the two expansion constants in vector registers

    // row operand: this lane's row of each 32-row tile, its 16-byte quarter-pair (words 4h .. 4h+3) expanded
    int afr[RT][4][4];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        const int row = rb + wv * WROWS + t * 32 + r;
        const uint4 w = *reinterpret_cast<const uint4 *>(rows + (size_t)(row < n1 ? row : n1 - 1) * 8 + 4 * h);
        expand_fp4(w.x, km, kc, afr[t][0]);
        expand_fp4(w.y, km, kc, afr[t][1]);
        expand_fp4(w.z, km, kc, afr[t][2]);
        expand_fp4(w.w, km, kc, afr[t][3]);
    }
    const int kwv = (127 - wv) << 7; // column side: the tile field is swapped for the wave's place in the workgroup

    for (int cb = 0; cb < n2; cb += F4_CHUNK) {
        const int ncol = n2 - cb < F4_CHUNK ? n2 - cb : F4_CHUNK, ntile = (ncol + 31) / 32;
        if (COL) {
            for (int c = tid; c < ntile * 32; c += 256) colbest[c] = 0; // below every real value
            __syncthreads();
        }
        const char *dB = reinterpret_cast<const char *>(cols + (col0 + cb) * 8);
        auto fetch = [&](int ct) -> uint4 { // this lane's quarter-pair of column ct * 32 + r, clamped into the chunk
            int c = (ct > 0 ? ct : 0) * 32 + r;
            c = c < ncol ? c : ncol - 1;
            return *reinterpret_cast<const uint4 *>(dB + (uint32_t)c * 32u + 16u * (uint32_t)h);
        };
        // C input of the LAST tile (the loop walks the tiles downwards; a tile step adds 128 on the matrix pipe, see k_ham_fp4):
        // (127 - ct) << 7 | (127 - row position inside the wave's tile)
        f32x16 cc;
        int b1[RT][16], b2[RT][16];
#pragma unroll
        for (int g = 0; g < 16; g++) {
            cc[g] = (float)(F4_BIAS + (((127 - (ntile - 1)) << 7) | (127 - ((g & 3) + 8 * (g >> 2) + 4 * h))));
#pragma unroll
            for (int t = 0; t < RT; t++) b1[t][g] = b2[t][g] = 0; // below every real value (raw bits of a float >= 2^23)
        }
        // one column tile; `slot` holds its raw words (loaded four tiles ago) and is refilled for tile ct - 4
        auto step = [&](int ct, uint4 &slot, bool ragged) {
            int b[4][4];
            expand_fp4(slot.x, km, kc, b[0]);
            expand_fp4(slot.y, km, kc, b[1]);
            expand_fp4(slot.z, km, kc, b[2]);
            expand_fp4(slot.w, km, kc, b[3]);
            slot = fetch(ct - 4);
            const i32x8 onesv = {kc, kc, kc, kc, 0, 0, 0, 0}; // the fp4 code of +1 in every nibble
            const f32x16 ccn = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(onesv, onesv, cc, 4, 4, 0, 128, 0, 127);
            const bool valid = !ragged || ct * 32 + r < ncol;
            int xm[RT];
#pragma unroll
            for (int t = 0; t < RT; t++) {
                f32x16 acc = cc;
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const i32x8 av = {afr[t][s4][0], afr[t][s4][1], afr[t][s4][2], afr[t][s4][3], 0, 0, 0, 0};
                    const i32x8 bv = {b[s4][0], b[s4][1], b[s4][2], b[s4][3], 0, 0, 0, 0};
                    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 4, 4, 0, F4_SCALE_A, 0, 127);
                }
                i32x16 ai;
#pragma unroll
                for (int g = 0; g < 16; g++) ai[g] = __float_as_int(acc[g]);
#pragma unroll
                for (int g = 0; g < 16; g++) {
                    const int x = valid ? ai[g] : 0;
                    if (K == 2) b2[t][g] = max(min(b1[t][g], x), min(max(b1[t][g], x), b2[t][g])); // v_med3_i32
                    b1[t][g] = max(b1[t][g], x);
                }
                if (COL) xm[t] = max16i(ai) - 32 * t; // best of the lane's 16 rows, moved to the tile's place in the wave
            }
            if (COL) {
                int cm = xm[0];
#pragma unroll
                for (int t = 1; t < RT; t++) cm = max(cm, xm[t]);
                atomicMax(&colbest[ct * 32 + r], cm + (kwv - ((127 - ct) << 7)));
            }
            cc = ccn;
        };
        uint4 w0 = fetch(ntile - 1), w1 = fetch(ntile - 2), w2 = fetch(ntile - 3), w3 = fetch(ntile - 4);
        int ct = ntile - 1;
        step(ct, w0, true); // the only tile that can be ragged
        ct--;
        for (; ct >= 3; ct -= 4) {
            step(ct, w1, false);
            step(ct - 1, w2, false);
            step(ct - 2, w3, false);
            step(ct - 3, w0, false);
        }
        if (ct >= 0) { step(ct, w1, false); ct--; }
        if (ct >= 0) { step(ct, w2, false); ct--; }
        if (ct >= 0) { step(ct, w3, false); ct--; }

        // row side: rebuild each value's column position (key = 8191 - position: the smaller column wins a tie), merge the
        // 32 lanes of a row set; value g of a tile ends in lane 16 + g (h = 0) / 48 + g (h = 1).  With raw = x - F4_RAW0 and
        // position = (127 - tile field) * 32 + r the new value is (raw & ~0x3FFF) | (8191 - position), three disjoint fields;
        // F4_RAW0 has no bit below 2^21, so they are read from x itself and the constants gather in kr
        int tid2 = threadIdx.x;
        asm volatile("" : "+v"(tid2));
        const int r2 = tid2 & 31, kr = 8191 - 127 * 32 - F4_RAW0 - r2;
        uint32_t n1k[RT], n2k[RT];
#pragma unroll
        for (int t = 0; t < RT; t++) {
            int mine1 = INT_MIN, mine2 = INT_MIN;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                auto rekey = [&](int x) { // the dot product's field + the tile field as 32 columns a tile + (constants - r)
                    return x == 0 ? INT_MIN : (x & ~0x3FFF) + ((x >> 2) & 0xFE0) + kr;
                };
                int v1 = rekey(b1[t][g]), v2 = K == 2 ? rekey(b2[t][g]) : INT_MIN;
                half_top<K>(v1, v2);
                if (r2 == 16 + g) { mine1 = v1; mine2 = v2; }
            }
            auto gkey = [&](int v) -> uint32_t { // (hamming << 20 | column) of a merged value
                return v == INT_MIN ? PGX_KEY_NONE
                                    : ((uint32_t)(128 - (v >> 14)) << PGX_IDX_BITS) | (uint32_t)(cb + 8191 - (v & 0x3FFF));
            };
            n1k[t] = gkey(mine1);
            n2k[t] = gkey(mine2);
        }
        if (r2 >= 16) { // the lane owns row value g = r2 - 16 of each of its tiles (in LDS: no registers held across the chunks)
            const int g = r2 - 16, h2 = (tid2 >> 5) & 1, wv2 = tid2 >> 6;
#pragma unroll
            for (int t = 0; t < RT; t++) {
                const int iloc = wv2 * WROWS + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h2;
                uint32_t k1 = cb ? rowtop[0][iloc] : PGX_KEY_NONE, k2 = K == 2 && cb ? rowtop[K - 1][iloc] : PGX_KEY_NONE;
                merge_min2(k1, k2, n1k[t], n2k[t]);
                // One key and no column side (k_knn_fp4<1, false, 2>, k_vocab_fp4): chunks after the first merge with a ds_min, which
                // leaves what the store leaves.  hipcc 7.2 fits the chunk loop of these forms into 223 registers with it; without, it
                // takes 230 and keeps a fifth column slot in flight, 1 % of the call (measured).
                if (K == 1 && !COL && cb) atomicMin(&rowtop[0][iloc], n1k[t]);
                else rowtop[0][iloc] = k1;
                if (K == 2) rowtop[K - 1][iloc] = k2;
            }
        }
        if (COL) {
            __syncthreads(); // colbest complete
            uint32_t *ck = colkey + cb;
            for (int c = tid; c < ncol; c += 256) {
                const int cbv = colbest[c];
                if (cbv == 0) continue;
                const int v = cbv - F4_RAW0;
                const int key = 16383 - (v & 0x3FFF); // wave << 7 | row position inside the wave
                const int iloc = (key >> 7) * WROWS + (key & 127);
                atomicMin(&ck[c], ((uint32_t)(128 - (v >> 14)) << PGX_IDX_BITS) | (uint32_t)(rb + iloc));
            }
            __syncthreads(); // before the next chunk clears colbest
        }
    }

    int tid3 = threadIdx.x;
    asm volatile("" : "+v"(tid3));
    const int r3 = tid3 & 31, h3 = (tid3 >> 5) & 1, wv3 = tid3 >> 6;
    if (r3 >= 16) {
        const int g = r3 - 16;
#pragma unroll
        for (int t = 0; t < RT; t++) {
            const int iloc = wv3 * WROWS + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h3, i = rb + iloc;
            if (i < n1)
                pgx_store_keys<K>(rowtop[0][iloc], K == 2 ? rowtop[K - 1][iloc] : PGX_KEY_NONE, oidx + (size_t)i * K,
                                  odist ? odist + (size_t)i * K : nullptr);
        }
    }
}
