// k_match_mfma.inc -- the Hamming distance on the matrix pipe (included by k_match.hip; 256-bit descriptors = 8 words).
// The arithmetic (fp4 expansion, biased accumulators, key fields) is derived in pgx_fp4.h, which k_knn.hip shares.
#include "pgx_fp4.h"

namespace {

constexpr int HAM_PAD = 4;      // pad tiles in front of k_ham_fp4's staged column offsets (its prefetch ring runs four tiles ahead, downwards)
constexpr int MF_CHUNK = F4_CHUNK; // most columns one workgroup walks (LDS column-best array)

// One row block of one image pair against its column chunk, RT row tiles per wavefront (4 * RT * 32 rows).  The kernel below
// owns the LDS and the block map and picks RT by the rows the block really has: the LAST row block of a pair is usually ragged
// (4096 rows = 10 blocks of 384 + 256), and 256 rows are exactly four waves x two tiles -- with three tiles per wave the
// block would spend a full block's time on two thirds of a block's rows (3 % of the launch at 4096 rows).
template <int RT>
__device__ __forceinline__ void ham_block(const PairWs &p, const uint32_t *__restrict__ dA, const uint32_t *__restrict__ dB,
                                          const uint32_t *rows, const uint32_t *cols, int n1, int rb, int cb, int ncol, int ntile,
                                          int *colbest, uint32_t *coloff, uint32_t *rowidx, unsigned long long *dbg)
{
    constexpr int WROWS = RT * 32, BM = 4 * WROWS; // rows per wavefront / in this block
#ifdef PGX_HAM_STAMP // developer builds only: phase times of thread 0 (10 ns units) summed over the workgroups, into the debug counters
    const long long hs0 = wall_clock64();
#define HAM_STAMP(x) const long long x = wall_clock64()
#else
#define HAM_STAMP(x)
#endif
    // opaque per instantiation: what depends on the thread id only is otherwise shared between the three inlined forms of this
    // function and stays live across all of their loops
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    int km = (int)0x88888888, kc = 0x22222222;
    asm volatile("" : "+v"(km), "+v"(kc)); // pin the two expansion constants in vector registers

    // column operand addresses staged once, as the BYTE OFFSET of every lane's quarter-pair from dB (entry tile * 64 + lane:
    // descriptor index * 32 + 16 h): the loop's loads are then `base in scalar registers + 32-bit lane offset` straight from
    // the LDS word, no address arithmetic on the vector ALU (it was a 64-bit shift and a 64-bit add per tile).  Entries past
    // the end (the rest of the last tile, the tiles the prefetch touches beyond it) point at a real descriptor: such a
    // duplicate ties with its original, which sits at a smaller column position and therefore wins every comparison
    // The loop walks the tiles from the LAST to the first (see the C vector below) and prefetches four tiles ahead, i.e. down to
    // tile -4: the staged array starts with HAM_PAD pad tiles (entry (tile + HAM_PAD) * 64 + lane), which are loaded but never used
    const int nstage = (ntile + HAM_PAD) * 64;
    for (int e = tid; e < nstage; e += 256) {
        const int c = ((e >> 6) - HAM_PAD) * 32 + (e & 31);
        coloff[e] = cols[cb + (c >= 0 && c < ncol ? c : 0)] * 32u + 16u * (uint32_t)((e >> 5) & 1);
    }
    for (int c = tid; c < ntile * 32; c += 256) colbest[c] = 0; // below every real value (raw bits of a float >= 2^23)
    for (int c = tid; c < BM; c += 256) rowidx[c] = rows[rb + c < n1 ? rb + c : n1 - 1];

    // row operand: this lane's row of each 32-row tile, its quarter-pair (words 4h .. 4h+3) expanded
    int afr[RT][4][4];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        // slots past the end reuse the LAST valid row: equal dot, larger row position, so they can never win a column
        // (their own row results are dropped at the end)
        const int row = rb + wv * WROWS + t * 32 + r;
        const uint32_t oi = rows[row < n1 ? row : n1 - 1];
        const uint4 w = *reinterpret_cast<const uint4 *>(dA + (size_t)oi * 8 + 4 * h);
        expand_fp4(w.x, km, kc, afr[t][0]);
        expand_fp4(w.y, km, kc, afr[t][1]);
        expand_fp4(w.z, km, kc, afr[t][2]);
        expand_fp4(w.w, km, kc, afr[t][3]);
    }
    // C input of the LAST tile for row tile 0 (row tile t sits 32 t rows further down).  The tile field of the key, 127 - ct, must
    // fall with ct (equal distances: the smaller column wins); walking the tiles from the last to the first makes its step
    // POSITIVE, +128 per tile, and that step is taken on the matrix pipe: one more MFMA per tile whose operands are both the
    // fp4 code of +1 (64 products of 1 at block scale 2 = 128 in every element, exact).  Round 5: as eight v_pk_add_f32 the step
    // cost vector-issue slots the loop is bound by (the compiler even unpacks them in the shadow of the MFMAs), the matrix pipe
    // is half idle; with it there, and the kernel held to 240 registers (below), 3.71 -> 3.63 ms per bench step alone and 7.12 -> 7.06 ms
    // per step in interleaved runs.  One operand tuple serves A and B (4 registers).
    f32x16 cc;
    // raw accumulator bits (positive floats order like integers).  Plain int arrays and __float_as_int: with an
    // ext_vector_type(16) array and __builtin_bit_cast on its elements, every element of a vector came out as element 0
    // (hipcc 7.2; every row of a lane then published the first row's result)
    int rbest[RT][16];
#pragma unroll
    for (int g = 0; g < 16; g++) {
        cc[g] = (float)(F4_BIAS + (((127 - (ntile - 1)) << 7) | (127 - ((g & 3) + 8 * (g >> 2) + 4 * h))));
#pragma unroll
        for (int t = 0; t < RT; t++) rbest[t][g] = 0; // below every real value
    }
    __syncthreads(); // coloff, colbest visible
    HAM_STAMP(hs1);

    const char *dBb = reinterpret_cast<const char *>(dB);
    auto fetch = [&](int ct) -> uint4 { // this lane's quarter-pair of column ct * 32 + r
        return *reinterpret_cast<const uint4 *>(dBb + coloff[(ct + HAM_PAD) * 64 + lane]);
    };
    const int kwv = (127 - wv) << 7; // column side: the ct field is swapped for the wave's position in the workgroup
    // one column tile; `slot` holds the tile's raw words (loaded four tiles ago) and is refilled for tile ct - 4, so three
    // loads stay in flight over a step (a two-deep rotation made the compiler wait for the newest load at every loop top)
    auto step = [&](int ct, uint4 &slot) {
        int b[4][4];
        expand_fp4(slot.x, km, kc, b[0]);
        expand_fp4(slot.y, km, kc, b[1]);
        expand_fp4(slot.z, km, kc, b[2]);
        expand_fp4(slot.w, km, kc, b[3]);
        slot = fetch(ct - 4);
        int xm[RT];
        // the next tile's C input, made OUT OF PLACE before this tile's chains start (they read cc): the last chain then runs in
        // place on the dying cc and nothing is copied
        const i32x8 onesv = {kc, kc, kc, kc, 0, 0, 0, 0}; // kc = 0x22222222: the fp4 code of +1 in every nibble
        const f32x16 ccn = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(onesv, onesv, cc, 4, 4, 0, 128, 0, 127);
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
            // row side: one max per element (orders by (dot, smaller ct)); column side: best of the lane's 16 rows, moved
            // to the row tile's place in the wave (-32 t on the key's row field: an integer subtraction on the raw bits)
#pragma unroll
            for (int g = 0; g < 16; g++) rbest[t][g] = max(rbest[t][g], ai[g]);
            xm[t] = max16i(ai) - 32 * t;
        }
        int cm = xm[0];
#pragma unroll
        for (int t = 1; t + 1 < RT; t += 2) cm = max(max(cm, xm[t]), xm[t + 1]); // v_max3
        if ((RT & 1) == 0) cm = max(cm, xm[RT - 1]);
        // every lane's winner carries this tile's ct field, (127 - ct) << 7: swapping it for the wave's field is ONE add of a
        // wave-uniform constant (made on the scalar unit)
        atomicMax(&colbest[ct * 32 + r], cm + (kwv - ((127 - ct) << 7)));
        cc = ccn;
    };
    uint4 w0 = fetch(ntile - 1), w1 = fetch(ntile - 2), w2 = fetch(ntile - 3), w3 = fetch(ntile - 4);
    int ct = ntile - 1;
    for (; ct >= 3; ct -= 4) {
        step(ct, w0);
        step(ct - 1, w1);
        step(ct - 2, w2);
        step(ct - 3, w3);
    }
    if (ct >= 0) { step(ct, w0); ct--; }
    if (ct >= 0) { step(ct, w1); ct--; }
    if (ct >= 0) { step(ct, w2); ct--; }
    __syncthreads();
    HAM_STAMP(hs2);

    // row results: a lane's best is (dot, ct) of column ct*32 + r; rebuild the column position, combine the 32 lanes
    // that share a row set (five DPP row operations, no LDS shuffles).  The finished value number g sits in all of the
    // lanes r = 16..31: lane 16 + g keeps it, so the 16 values of a row tile are published by 16 lanes at once (one
    // lane publishing all 32 made 32 dependent LDS look-ups in a row)
    // the lane's coordinates once more, from an opaque copy of the thread id: kept live across the tile loops they cost two of the
    // 240 registers the kernel is held to (see the kernel below) and, in the two-tile form, a spill
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int r2 = tid2 & 31, h2 = (tid2 >> 5) & 1, wv2 = tid2 >> 6;
    int mine[RT];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        mine[t] = 0;
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int raw = rbest[t][g] - F4_RAW0;
            const int cpos = (127 - ((raw >> 7) & 127)) * 32 + r2;
            int v = (raw & ~0x3FFF) | (8191 - cpos);
            v = half_max_i32(v); // complete in lanes 16..31 (h = 0) and 48..63 (h = 1)
            if (r2 == 16 + g) mine[t] = v;
        }
    }
    if (r2 >= 16) {
        const int g = r2 - 16;
#pragma unroll
        for (int t = 0; t < RT; t++) {
            const int iloc = wv2 * WROWS + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h2;
            if (rb + iloc < n1) {
                const int v = mine[t];
                const int mdot = v >> 14;                       // dot / 2
                const int jloc = 8191 - (v & 0x3FFF);
                const uint32_t ham = (uint32_t)(128 - mdot);
                atomicMin(&p.rowkey[rowidx[iloc]], (ham << PGX_IDX_BITS) | (coloff[((jloc >> 5) + HAM_PAD) * 64 + (jloc & 31)] >> 5));
            }
        }
    }
    HAM_STAMP(hs3);
    // column results: low 14 bits = (127 - wave) << 7 | (127 - row position inside the wave)
    for (int c = tid; c < ncol; c += 256) {
        if (colbest[c] == 0) continue; // no valid row in this workgroup's row block
        const int v = colbest[c] - F4_RAW0;
        const int mdot = v >> 14;
        const int key = 16383 - (v & 0x3FFF); // wave << 7 | row position
        const int iloc = (key >> 7) * WROWS + (key & 127);
        const uint32_t ham = (uint32_t)(128 - mdot);
        atomicMin(&p.colkey[coloff[((c >> 5) + HAM_PAD) * 64 + (c & 31)] >> 5], (ham << PGX_IDX_BITS) | rowidx[iloc]);
    }
#ifdef PGX_HAM_STAMP
    if (tid == 0) {
        const long long hs4 = wall_clock64();
        atomicAdd(&dbg[0], (unsigned long long)(hs1 - hs0)); atomicAdd(&dbg[1], (unsigned long long)(hs2 - hs1)); atomicAdd(&dbg[2], (unsigned long long)(hs3 - hs2));
        atomicAdd(&dbg[5], (unsigned long long)(hs4 - hs3)); atomicAdd(&dbg[7], 1ull);
    }
#endif
#undef HAM_STAMP
}

// Held to 240 vector registers (amdgpu_num_vgpr counts half on gfx90a and later: 120): two of its waves then leave 32 registers of a
// SIMD free, in which the small kernels of other jobs in flight (FAST at 32 registers, the track-graph kernels, scans) run WITHOUT
// displacing one of them.  At 252 registers -- the allocation granule above 240 is 256 -- the same code was 1.6 % faster alone and
// made the bench step 1.8 % slower (k_trk_union 1.10 instead of 0.57 ms beside it, k_match_select waiting 0.7 ms for a CU);
// tests/test_ham_codegen.py pins the budget on the code object.
template <int RT> // row tiles per wavefront of a FULL row block; the host sizes the grid with 4 * RT * 32 rows per block
__attribute__((amdgpu_num_vgpr(120))) __global__ __launch_bounds__(256, 2) void k_ham_fp4(uint32_t *ws, const uint32_t *__restrict__ desc,
                                                    const int32_t *__restrict__ pairlist, int S, int cols_per_wg,
                                                    int skip_below, int nbx, int nby, int npairs, unsigned long long *dbg)
{
    constexpr int BM = 4 * RT * 32;
    __shared__ int colbest[MF_CHUNK];
    __shared__ uint32_t coloff[(MF_CHUNK + 32 * 8) * 2]; // this workgroup's slice of the column list as byte offsets, per lane (+ prefetch overrun)
    __shared__ uint32_t rowidx[BM];                // the row block's keypoint indices: the publishing loops below would
                                                   // otherwise gather them from global memory one dependent load per atomic
    // XCD-aware workgroup -> (image pair, row block, column chunk) map: consecutive workgroup ids are dealt round-robin to
    // the 8 XCDs, so id % 8 picks the pair inside a group of 8 pairs and all workgroups of one image pair run on ONE XCD:
    // they stream the same 128 KiB of column descriptors, which then stay in that XCD's 4 MiB L2 (with the plain 3-D grid
    // every XCD touched every pair of a chunk: 8 MB of columns per XCD, L2 hit rate 46 %; with this map 70 % -- the kernel's time did not move, it is not bound there)
    int m, bx, by;
    {
        const int per_pair = nbx * nby, M8 = (npairs / 8) * 8;
        const int L = blockIdx.x;
        if (L < per_pair * M8) {
            const int slot = L >> 3;
            m = (slot / per_pair) * 8 + (L & 7);
            const int q = slot % per_pair;
            by = q / nbx; bx = q - by * nbx;
        } else {
            const int q0 = L - per_pair * M8;
            m = M8 + q0 / per_pair;
            const int q = q0 % per_pair;
            by = q / nbx; bx = q - by * nbx;
        }
    }
    PairWs p = pair_ws(ws, m, S);
    const int n1 = p.cnt[CNT_N1], n2 = p.cnt[CNT_N2], parity = p.cnt[CNT_PARITY];
    if (n1 <= 0 || n2 <= 0) return;
    if (n1 <= skip_below && n2 <= skip_below) return; // small enough: the per-pair tail takes it from here
#ifdef PGX_HAM_PRIO
    __builtin_amdgcn_s_setprio(PGX_HAM_PRIO);
#endif
    const int rb = bx * BM, cb = by * cols_per_wg;
    if (rb >= n1 || cb >= n2) return;
    const int ce = (cb + cols_per_wg < n2) ? cb + cols_per_wg : n2;
    const int ncol = ce - cb, ntile = (ncol + 31) / 32;
    const uint32_t *dA = desc + (size_t)pairlist[2 * m] * S * 8;
    const uint32_t *dB = desc + (size_t)pairlist[2 * m + 1] * S * 8;
    const uint32_t *rows = (parity ? p.rows1 : p.rows0), *cols = (parity ? p.cols1 : p.cols0);
    const int rem = n1 - rb; // rows this block really has (uniform)
    if (RT >= 3 && rem <= 4 * 64) {
        if (rem <= 4 * 32) ham_block<1>(p, dA, dB, rows, cols, n1, rb, cb, ncol, ntile, colbest, coloff, rowidx, dbg);
        else ham_block<2>(p, dA, dB, rows, cols, n1, rb, cb, ncol, ntile, colbest, coloff, rowidx, dbg);
    } else ham_block<RT>(p, dA, dB, rows, cols, n1, rb, cb, ncol, ntile, colbest, coloff, rowidx, dbg);
}

// ---- the same residual rows on the block-scaled FP4 instruction ----------------------------------------------------
// Roles are swapped against k_ham_fp4 so that a LANE owns a matrix row: the A operand (registers, 4 x 16 per lane) is 128 residual
// COLUMNS, the B operand (LDS) a tile of 32 residual ROWS; a lane's 4 x 16 accumulator registers are 64 columns of its row.
// Operands as in k_ham_fp4 (a lane holds one 16-byte quarter of a descriptor, MFMA s takes word 4h + s), the row side
// expanded from the COMPLEMENTED words, A block scale 2^7:
//     acc = C + 128 * dot(~a, b) = 2^23 + 256 * hamming + g           with C = 2^23 + 32768 + g   (g = the register's index)
// Every partial sum stays inside [2^23, 2^24), where f32 has unit spacing: exact, and the raw register is
// 0x4B000000 | (256 * hamming + g): the distance byte IS byte 1 of the register (four of them make a matrix dword with three
// v_perm_b32), bit 16 is the distance-256 flag, and the row minimum is the integer minimum of raw registers (g orders the
// lane's columns of one tile; the tile and the lane's place are added to the one value that survives).
// Four column tiles per wave: one read of the row fragments from LDS feeds 16 MFMAs, a wave's stores are whole 128-byte
// lines, and the byte-aligned distance field makes a matrix dword 3 instructions instead of 7 (1.08 -> 1.00 ms per bench
// step against the two-tile / 2^12 form).  Where the rest goes, from builds with parts removed (128 random pairs, us):
// whole kernel 103; without the LDS transposition and the stores 76; also without the minima, flags and packing 63 --
// fragment staging, dependent column loads and the MFMAs themselves (23 us of matrix pipe) are 60 % of it.
constexpr int F4_SCALE_ROWS = 134; // E8M0: 2^7
constexpr int TM_ROWS = 256;   // matrix rows per workgroup (128: the kernel alone 3 % faster, the pipelined step 1.5 % slower)
constexpr int TM_CT = 4;       // column tiles per wave: a wave owns 128 columns = one 128-byte line of every matrix row
constexpr int TM_PITCH = 36;   // dwords per staged tile row (128 bytes of data + 16 of padding)

__global__ __launch_bounds__(256, 2) void k_tail_rows_fp4(uint32_t *ws, const uint32_t *__restrict__ desc,
                                                          const int32_t *__restrict__ pairlist, int S)
{
    __shared__ i32x4 rfrag[TM_ROWS / 32][4][64];   // [row tile][MFMA step][half * 32 + row]   32 KiB
    __shared__ uint32_t rowmin[TM_ROWS];
    __shared__ __attribute__((aligned(16))) uint32_t stile[4][32 * TM_PITCH];
    const int m = blockIdx.y;
    PairWs p = pair_ws(ws, m, S);
    const int R = p.cnt[CNT_N1], C = p.cnt[CNT_N2], parity = p.cnt[CNT_PARITY];
    if (R <= 0 || C <= 0 || R > PGX_TAIL_MAX || C > PGX_TAIL_MAX) return;
    const int rb = blockIdx.x * TM_ROWS;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&p.cnt[CNT_FILLED], 1);
    if (rb >= R) return;
    const uint32_t *dA = desc + (size_t)pairlist[2 * m] * S * 8;
    const uint32_t *dB = desc + (size_t)pairlist[2 * m + 1] * S * 8;
    const uint32_t *rows = (parity ? p.rows1 : p.rows0), *cols = (parity ? p.cols1 : p.cols0);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const int Cs = tail_row_stride(C);
    uint8_t *D = tail_matrix(p);
    const int ntr = (R - rb + 31) / 32 < TM_ROWS / 32 ? (R - rb + 31) / 32 : TM_ROWS / 32;
    int km = (int)0x88888888u, kc = 0x22222222;
    asm volatile("" : "+v"(km), "+v"(kc)); // opaque: keeps the masks in registers so that (x & m) | c is one v_and_or_b32
    {   // word ss of a row goes to MFMA step ss & 3, half ss >> 2; complemented: the accumulator grows with the distance.
        // A thread takes one 16-byte half of a descriptor per pass (two passes cover 256 rows: two dependent load pairs per
        // thread instead of eight with one word per thread and pass)
        for (int q = tid; q < ntr * 64; q += 256) {
            const int rl = q >> 1, hh = q & 1, rt = rl >> 5, sc = rl & 31; // row inside the block, half, row tile, row in the tile
            const int row = rb + rl;
            const uint4 w4 = *reinterpret_cast<const uint4 *>(dA + (size_t)rows[row < R ? row : R - 1] * 8 + 4 * hh);
            const uint32_t ww[4] = {~w4.x, ~w4.y, ~w4.z, ~w4.w};
#pragma unroll
            for (int s = 0; s < 4; s++) {
                int f[4];
                expand_fp4(ww[s], km, kc, f);
                const i32x4 fv = {f[0], f[1], f[2], f[3]};
                rfrag[rt][s][hh * 32 + sc] = fv;
            }
        }
        if (tid < TM_ROWS) rowmin[tid] = 0xFFFFFFFFu;
    }
    __syncthreads();
    f32x16 cc; // shared by the four column tiles: only the distance byte and the order of a tile's 16 columns ride in it
#pragma unroll
    for (int g = 0; g < 16; g++) cc[g] = __int_as_float(0x4B000000 | (32768 + g));
    int orall = 0;
    for (int cb = wv * (32 * TM_CT); cb < Cs; cb += 4 * 32 * TM_CT) { // this wave's 128-column blocks (Cs is a multiple of 128)
        int afr[TM_CT][4][4];
#pragma unroll
        for (int t = 0; t < TM_CT; t++) {
            const int col = cb + t * 32 + r;
            const uint32_t oj = cols[col < C ? col : 0];
            const uint4 w = *reinterpret_cast<const uint4 *>(dB + (size_t)oj * 8 + 4 * h);
            expand_fp4(w.x, km, kc, afr[t][0]);
            expand_fp4(w.y, km, kc, afr[t][1]);
            expand_fp4(w.z, km, kc, afr[t][2]);
            expand_fp4(w.w, km, kc, afr[t][3]);
        }
        for (int rt = 0; rt < ntr; rt++) {
            i32x4 b[4];
#pragma unroll
            for (int s = 0; s < 4; s++) b[s] = rfrag[rt][s][lane];
            f32x16 acc[TM_CT];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const i32x8 bv = {b[s][0], b[s][1], b[s][2], b[s][3], 0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < TM_CT; t++) {
                    const i32x8 av = {afr[t][s][0], afr[t][s][1], afr[t][s][2], afr[t][s][3], 0, 0, 0, 0};
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, s == 0 ? cc : acc[t], 4, 4, 0, F4_SCALE_ROWS, 0, 127);
                }
            }
            const int i = rb + rt * 32 + r;
            uint32_t *tile = stile[wv];
            int mn = 0x7FFFFFFF;
#pragma unroll
            for (int t = 0; t < TM_CT; t++) {
                int a[16]; // raw bits: 0x4B000000 | (256 * distance + g)
#pragma unroll
                for (int g = 0; g < 16; g++) { a[g] = __float_as_int(acc[t][g]); orall |= a[g]; }
                int mt = a[0];
#pragma unroll
                for (int g = 1; g < 16; g++) mt = min(mt, a[g]);
                mn = min(mn, mt + 16 * t); // (distance, tile, g): the column order inside this lane
#pragma unroll
                for (int q = 0; q < 4; q++) { // registers 4q .. 4q+3 are four consecutive columns: byte 1 of each
                    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)a[4 * q + 1], (uint32_t)a[4 * q], 0x0c0c0501u);
                    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)a[4 * q + 3], (uint32_t)a[4 * q + 2], 0x05010c0cu);
                    tile[r * TM_PITCH + t * 8 + 2 * q + h] = lo | hi;
                }
            }
            if (i < R) { // the lane's best as (distance << 16 | column), the key format of k_match_gs (GS_KEY_SHIFT)
                const int tg = mn & 63, g = tg & 15;
                const uint32_t col = (uint32_t)(cb + (tg >> 4) * 32 + (g & 3) + 8 * (g >> 2) + 4 * h);
                atomicMin(&rowmin[rt * 32 + r], (((uint32_t)mn >> 8) & 0x1FFu) << 16 | col);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 4; k++) { // 8 rows x 128 bytes per store instruction: whole lines
                const int rr = k * 8 + (lane >> 3), seg = lane & 7;
                const uint4 v = *reinterpret_cast<const uint4 *>(tile + rr * TM_PITCH + seg * 4);
                const int ii = rb + rt * 32 + rr;
                if (ii < R) *reinterpret_cast<uint4 *>(D + (size_t)ii * Cs + cb + seg * 16) = v;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    if (tid < TM_ROWS && rb + tid < R) p.rowkey[rb + tid] = rowmin[tid];
    if (orall & (1 << 16)) atomicOr(&p.cnt[CNT_FILLED], 2); // a distance of 256 does not fit the byte matrix
}

} // namespace

static void pgx_launch_ham_mfma(hipStream_t s, uint32_t *ws, const uint32_t *desc, const int32_t *pairlist,
                                const MatchPlan &plan, hipEvent_t ev_begin, hipEvent_t ev_end, int *status)
{
    // three row tiles per wavefront: 240 VGPRs, two waves per SIMD (four spill; two: 184 VGPRs, 7 % slower alone)
#ifndef PGX_HAM_RT
#define PGX_HAM_RT 3
#endif
    constexpr int RT = PGX_HAM_RT;
    const int BM = RT * 128;
    const int rowtiles = (plan.max_n + BM - 1) / BM;
    // enough workgroups to fill 256 CUs a few times over, few enough that the row-operand prologue amortises
    int cols_per_wg = MF_CHUNK;
    const long target = 1024;
    while (cols_per_wg > 128 && (long)rowtiles * ((plan.max_n + cols_per_wg - 1) / cols_per_wg) * plan.M < target)
        cols_per_wg /= 2;
    dim3 grid(rowtiles, (plan.max_n + cols_per_wg - 1) / cols_per_wg, plan.M);
    const dim3 grid1(grid.x * grid.y * grid.z);
    if (ev_begin && ev_end) // profiling: the dispatch's own time stamps (ProfScope, attach)
        hipExtLaunchKernelGGL(k_ham_fp4<RT>, grid1, dim3(256), 0, s, ev_begin, ev_end, 0, ws, desc, pairlist, plan.stride, cols_per_wg,
                              plan.skip_below, (int)grid.x, (int)grid.y, plan.M, pgx_dbg(status));
    else
        hipLaunchKernelGGL(k_ham_fp4<RT>, grid1, dim3(256), 0, s, ws, desc, pairlist, plan.stride, cols_per_wg, plan.skip_below, (int)grid.x, (int)grid.y, plan.M, pgx_dbg(status));
}
