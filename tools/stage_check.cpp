// Exercises the host-only part of maxent_amd/csrc/mxe_stage.h stand-alone: the block layout and the three checks the
// single-launch entry points share (finite scan, group offsets, rows of the launch).  Exact-size heap arrays, so that a
// read past an end is seen by the sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stage_check.cpp -o stage_check && ./stage_check
// Prints "stage_check: ok" and returns 0, or names the first expectation that does not hold.
#define MXE_STAGE_PURE
#include "../maxent_amd/csrc/mxe_stage.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "stage_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // block layout: empty, zero-length arrays in between, offsets in the order of the calls
    Block b;
    EXPECT(b.total == 0);
    EXPECT(b.add(0) == 0 && b.total == 0);
    EXPECT(b.add(5) == 0 && b.add(0) == 5 && b.add(3) == 5 && b.add(1) == 8 && b.total == 9);

    // finite scan: nothing, every length around the stride of 8, the bad value in every position -- the tail included
    EXPECT(all_finite(nullptr, 0));
    for (size_t n = 1; n <= 27; ++n) {
        std::unique_ptr<double[]> x(new double[n]);
        for (size_t i = 0; i < n; ++i) x[i] = 1.0e300 * (i % 2 ? -1.0 : 1.0);
        EXPECT(all_finite(x.get(), n));
        for (size_t i = 0; i < n; ++i) {
            const double keep = x[i];
            x[i] = nan;  EXPECT(!all_finite(x.get(), n));
            x[i] = inf;  EXPECT(!all_finite(x.get(), n));
            x[i] = -inf; EXPECT(!all_finite(x.get(), n));
            x[i] = keep;
        }
        EXPECT(all_finite(x.get(), n));
    }
    {   // the case of the issue: 13 values (not a multiple of 8), NaN in the last one
        std::unique_ptr<double[]> x(new double[13]());
        x[12] = nan;
        EXPECT(!all_finite(x.get(), 13) && all_finite(x.get(), 12));
    }

    // group offsets: n_groups + 1 entries are read, no more
    {
        std::unique_ptr<int32_t[]> off(new int32_t[4]{0, 2, 2, 7});
        int longest = -1;
        EXPECT(group_offsets_ok(off.get(), 3, &longest) && longest == 5);
        EXPECT(group_offsets_ok(off.get(), 3));
        EXPECT(group_offsets_ok(off.get(), 0, &longest) && longest == 0);      // (only off[0] is read)
        off[0] = 1; EXPECT(!group_offsets_ok(off.get(), 3));
        off[0] = 0; off[2] = 1; EXPECT(!group_offsets_ok(off.get(), 3));
        off[2] = 2; off[3] = 1; EXPECT(!group_offsets_ok(off.get(), 3) && group_offsets_ok(off.get(), 2));
        std::unique_ptr<int32_t[]> one(new int32_t[2]{0, 0});
        EXPECT(group_offsets_ok(one.get(), 1, &longest) && longest == 0);
    }

    // rows of the launch: no rows, no index, an index in range, out of range at either end
    {
        EXPECT(launch_rows(nullptr, 0, 0, nullptr));
        std::unique_ptr<int[]> out(new int[5]);
        EXPECT(launch_rows(nullptr, 5, 5, out.get()));
        for (int r = 0; r < 5; ++r) EXPECT(out[r] == r);
        EXPECT(!launch_rows(nullptr, 5, 4, out.get()));
        std::unique_ptr<int32_t[]> idx(new int32_t[5]{19, 0, 7, 7, 3});
        EXPECT(launch_rows(idx.get(), 5, 20, out.get()));
        for (int r = 0; r < 5; ++r) EXPECT(out[r] == idx[r]);
        EXPECT(!launch_rows(idx.get(), 5, 19, out.get()));
        idx[4] = -1; EXPECT(!launch_rows(idx.get(), 5, 20, out.get()));
        idx[4] = 20; EXPECT(!launch_rows(idx.get(), 5, 20, out.get()));
        EXPECT(launch_rows(idx.get(), 4, 20, out.get()));                         // (the bad entry is beyond the rows asked for)
    }
    std::puts("stage_check: ok");
    return 0;
}
