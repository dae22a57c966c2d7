// filter_args_check.cpp — psgpu_weld_filter's argument rules (parsip_amd/csrc/psgpu_filter_check.h)
// as a stand-alone host program, for a run under the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/cpp/filter_args_check.cpp -o filter_args_check && ./filter_args_check
//
// Exit status 0: every rule holds (tests/test_filter.py builds and runs it so).
#include <cstdio>
#include <limits>
#include <vector>

#include "../../parsip_amd/csrc/psgpu_filter_check.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                \
        }                                                              \
    } while (0)

int main() {
    using psgpu::filter_criteria;
    using psgpu::filter_mask_fits;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    PsShellFilter out;
    EXPECT(filter_criteria(nullptr, &out));  // NULL: all zero
    EXPECT(out.flags == 0 && out.minVertices == 0 && out.minTriangles == 0 && out.reserved == 0);
    EXPECT(out.minArea == 0.0 && out.minAbsVolume == 0.0);
    PsShellFilter f{};
    f.flags = PSGPU_FILTER_CLOSED_ONLY | PSGPU_FILTER_DROP_CAVITIES;
    f.minVertices = 0xffffffffu;
    f.minTriangles = 7;
    f.minArea = 1e300;
    f.minAbsVolume = 4.9e-324;  // the smallest denormal
    EXPECT(filter_criteria(&f, &out));
    EXPECT(out.flags == 3 && out.minVertices == 0xffffffffu && out.minTriangles == 7);
    EXPECT(out.minArea == 1e300 && out.minAbsVolume == 4.9e-324);
    f = PsShellFilter{};
    f.minArea = -0.0;
    EXPECT(filter_criteria(&f, &out));
    for (uint32_t bit = 2; bit < 32; ++bit) {
        f = PsShellFilter{};
        f.flags = 1u << bit;
        EXPECT(!filter_criteria(&f, &out));
        f.flags |= PSGPU_FILTER_CLOSED_ONLY;
        EXPECT(!filter_criteria(&f, &out));
    }
    f = PsShellFilter{};
    f.reserved = 1;
    EXPECT(!filter_criteria(&f, &out));
    for (double bad : {nan, -nan, inf, -inf, -1.0, -4.9e-324}) {
        f = PsShellFilter{};
        f.minArea = bad;
        EXPECT(!filter_criteria(&f, &out));
        f = PsShellFilter{};
        f.minAbsVolume = bad;
        EXPECT(!filter_criteria(&f, &out));
    }
    std::vector<uint8_t> mask(3, 1);
    EXPECT(filter_mask_fits(nullptr, 0, 3) && filter_mask_fits(nullptr, 9, 3) && filter_mask_fits(nullptr, 0, 0));
    EXPECT(filter_mask_fits(mask.data(), 3, 3));
    EXPECT(!filter_mask_fits(mask.data(), 2, 3) && !filter_mask_fits(mask.data(), 4, 3));
    EXPECT(!filter_mask_fits(mask.data(), 0, 3) && !filter_mask_fits(mask.data(), 3, 0));
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
