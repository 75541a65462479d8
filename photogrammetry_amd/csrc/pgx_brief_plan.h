// pgx_brief_plan.h -- the sample plan of a 256-pair BRIEF table (plain host C++, no GPU; built once per pgx_set_brief_pairs).
//
// The table's 512 end points (pair p: end point 2p = (x1, y1), 2p + 1 = (x2, y2)) sorted by (dy, dx); ties keep table
// order.  Sorted sample 64g + l is loaded by lane l in gather g of brief_256 (k_brief.hip), so that one gather instruction
// covers a band of adjacent image rows, and it is written to slot 64g + l of the wave's LDS strip.  pos[p] tells the lane
// that evaluates pair p where its two values lie: slot of (x1, y1) in bits 0-8, slot of (x2, y2) in bits 16-24.
// Every end point keeps a slot of its own (equal offsets are not merged), so any int32 offsets are fine.
#pragma once
#include <algorithm>
#include <cstdint>

constexpr int PGX_PLAN_PAIRS = 256;
constexpr int PGX_PLAN_SAMPLES = 2 * PGX_PLAN_PAIRS;
// device layout: int32 samples[512][2] = (dx, dy), then uint32 pos[256]
constexpr int PGX_PLAN_WORDS = 2 * PGX_PLAN_SAMPLES + PGX_PLAN_PAIRS;

inline void pgx_build_brief_plan(const int32_t *pairs /* [256][4] */, int32_t *plan /* [PGX_PLAN_WORDS] */)
{
    uint16_t idx[PGX_PLAN_SAMPLES];
    for (int i = 0; i < PGX_PLAN_SAMPLES; i++) idx[i] = (uint16_t)i;
    std::stable_sort(idx, idx + PGX_PLAN_SAMPLES, [pairs](uint16_t a, uint16_t b) {
        const int32_t ax = pairs[2 * a], ay = pairs[2 * a + 1], bx = pairs[2 * b], by = pairs[2 * b + 1];
        return ay != by ? ay < by : ax < bx;
    });
    uint32_t *pos = reinterpret_cast<uint32_t *>(plan + 2 * PGX_PLAN_SAMPLES);
    for (int p = 0; p < PGX_PLAN_PAIRS; p++) pos[p] = 0;
    for (int s = 0; s < PGX_PLAN_SAMPLES; s++) {
        const int e = idx[s]; // end point e of the table: pair e / 2, second end point if e is odd
        plan[2 * s] = pairs[2 * e];
        plan[2 * s + 1] = pairs[2 * e + 1];
        pos[e >> 1] |= (uint32_t)s << ((e & 1) * 16);
    }
}
