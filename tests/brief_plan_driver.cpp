// Stand-alone driver of the BRIEF sample-plan builder (photogrammetry_amd/csrc/pgx_brief_plan.h) for tests/test_brief_plan.py:
// reads a 256-pair table (1024 int32, native endian) from the file argv[1] and writes the plan (PGX_PLAN_WORDS int32) to
// stdout.  Host code only; the test builds it with -fsanitize=address,undefined, so a sanitizer report fails the run.
#include <cstdio>
#include <vector>

#include "../photogrammetry_amd/csrc/pgx_brief_plan.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    // heap buffers of the exact sizes, so that an access past either end is a sanitizer report
    std::vector<int32_t> pairs(4 * PGX_PLAN_PAIRS), plan(PGX_PLAN_WORDS);
    const size_t got = std::fread(pairs.data(), sizeof(int32_t), pairs.size(), f);
    std::fclose(f);
    if (got != pairs.size()) return 2;
    pgx_build_brief_plan(pairs.data(), plan.data());
    return std::fwrite(plan.data(), sizeof(int32_t), plan.size(), stdout) == plan.size() ? 0 : 3;
}
