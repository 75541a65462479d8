// k_brief_core.inc -- the two per-keypoint BRIEF evaluators, shared by k_brief.hip (upright table) and k_steer.hip (the table
// of the keypoint's direction).  Included inside the including file's anonymous namespace, after pgx_internal.h and
// pgx_brief_plan.h.  Both work on any int32 offsets, so a turned table is just another table.

constexpr int MAX_WORDS = 128; // P <= 4096

// P == 256 fast path on the table's row-sorted sample plan (pgx_brief_plan.h).  The 512 end points are loaded in (dy, dx)
// order, sample 64g + l by lane l in gather g, so that a gather instruction covers a band of adjacent image rows instead of
// 64 scattered ones; all eight gathers are issued before any is used.  A sample outside the image is not loaded and counts
// as 0.  The values go to the wave's LDS strip at their sorted positions (slot 64g + l: no bank conflict), the eight
// inside-the-image ballots to the 16 mask words behind it; lane l of chunk c then reads the two values and the two mask
// bits of pair 64c + l.  Same f32 values, same comparison, same eight output words as the table-order form.
constexpr int STRIP_WORDS = PGX_PLAN_SAMPLES + 16;
static_assert(MAX_WORDS + 2 <= STRIP_WORDS && PGX_PLAN_PAIRS == 256, "the LDS strip also serves brief_one");

__device__ __forceinline__ void brief_256(const float *__restrict__ img, int W, int H, int x, int y,
                                          const int32_t *__restrict__ plan, uint32_t *strip /*LDS, STRIP_WORDS*/,
                                          uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int2 *smp = reinterpret_cast<const int2 *>(plan);
    const uint32_t *pos = reinterpret_cast<const uint32_t *>(plan) + 2 * PGX_PLAN_SAMPLES;
    float *val = reinterpret_cast<float *>(strip);
    uint32_t *mask = strip + PGX_PLAN_SAMPLES;
    int2 sm[8];
#pragma unroll
    for (int g = 0; g < 8; g++) sm[g] = smp[g * 64 + lane];
    uint32_t off[8];
    bool in[8];
#pragma unroll
    for (int g = 0; g < 8; g++) {
        const int xs = x + sm[g].x, ys = y + sm[g].y;
        in[g] = xs >= 0 && xs < W && ys >= 0 && ys < H; // Keypoint.cs:39-40, :44-45
        off[g] = (uint32_t)ys * (uint32_t)W + (uint32_t)xs; // exact inside the image: W, H <= 65535 (dims_ok)
        const unsigned long long m = __ballot(in[g]);
        if (lane == 0) { mask[2 * g] = (uint32_t)m; mask[2 * g + 1] = (uint32_t)(m >> 32); }
    }
    float v[8];
#pragma unroll
    for (int g = 0; g < 8; g++) v[g] = in[g] ? img[off[g]] : 0.f;
    uint32_t pp[4];
#pragma unroll
    for (int c = 0; c < 4; c++) pp[c] = pos[c * 64 + lane];
#pragma unroll
    for (int g = 0; g < 8; g++) val[g * 64 + lane] = v[g];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unsigned long long rev[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t p1 = pp[c] & 511u, p2 = (pp[c] >> 16) & 511u;
        const bool ok = ((mask[p1 >> 5] >> (p1 & 31)) & (mask[p2 >> 5] >> (p2 & 31)) & 1u) != 0; // both end points inside
        const float v1 = val[p1], v2 = val[p2];
        rev[c] = __brevll(__ballot(ok && v1 < v2)); // :50; bits [192-64c, 256-64c)
    }
    if (lane < 8) {
        const int q = lane >> 1; // 64-bit piece q of the descriptor comes from chunk 3 - q (selects, not a runtime index)
        const unsigned long long r = q == 0 ? rev[3] : (q == 1 ? rev[2] : (q == 2 ? rev[1] : rev[0]));
        out[lane] = (lane & 1) ? (uint32_t)(r >> 32) : (uint32_t)r;
    }
}

__device__ __forceinline__ void brief_one(const float *__restrict__ g, int W, int H, int x, int y,
                                          const int4 *__restrict__ pairs, int P, int words, uint32_t *wbuf /*LDS*/,
                                          uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    for (int w = lane; w < words + 2; w += 64) wbuf[w] = 0;
    __builtin_amdgcn_wave_barrier();
    const int nchunk = (P + 63) / 64;
    for (int c = 0; c < nchunk; c++) {
        const int p = c * 64 + lane;
        bool bit = false;
        if (p < P) {
            const int4 pr = pairs[p];
            const int x1 = x + pr.x, y1 = y + pr.y;
            if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H) {           // Keypoint.cs:39-40
                const int x2 = x + pr.z, y2 = y + pr.w;
                if (x2 >= 0 && x2 < W && y2 >= 0 && y2 < H)          // :44-45
                    bit = g[(size_t)y1 * W + x1] < g[(size_t)y2 * W + x2]; // :50
            }
        }
        const unsigned long long rev = __brevll(__ballot(bit));
        if (lane == 0) {
            const int off = P - 64 * (c + 1); // bit position of rev's bit 0 (may be negative on the last chunk)
            unsigned long long v = rev;
            int o = off;
            if (o < 0) { v >>= -o; o = 0; }
            const int wi = o >> 5, sh = o & 31;
            wbuf[wi] |= (uint32_t)(v << sh);
            wbuf[wi + 1] |= (uint32_t)(sh ? (v >> (32 - sh)) : (v >> 32));
            if (sh) wbuf[wi + 2] |= (uint32_t)(v >> (64 - sh));
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int w = lane; w < words; w += 64) out[w] = wbuf[w];
}
