// The escape-query predicate (pbrt-v3-rs_amd/csrc/mis_escape.h) on the CPU: prints, for each of the 24 combinations of scene features,
//     eligible area=<0|1> alpha=<0|1|2> quadric=<0|1> counting=<0|1> -> <0|1>
// for each of the 12 kinds of traversal row
//     row alpha=<0|1|2> quadric=<0|1> counting=<0|1> -> <0|1>
// and for a list of bin keys, marked and unmarked, the joint key the binning makes of a closest-hit key
//     joint key=<key> -> bin=<bin in the joint key space> mark=<0|1>
// tests/test_mis_escape_plan_cpu.py holds what the lines must say.
// Build and run:  bash scripts/mis_escape_check.sh
#include "../pbrt-v3-rs_amd/csrc/mis_escape.h"
#include <cstdio>

int main() {
    for (int k = 0; k < 24; k++) {
        const int area = k & 1, counting = (k >> 1) & 1, quadric = (k >> 2) & 1, alpha = k >> 3;
        std::printf("eligible area=%d alpha=%d quadric=%d counting=%d -> %d\n", area, alpha, quadric, counting, (int)ph::mis_escape_eligible(area != 0, alpha, quadric != 0, counting != 0));
    }
    for (int k = 0; k < 12; k++) {
        const int counting = k & 1, quadric = (k >> 1) & 1, alpha = k >> 2;
        std::printf("row alpha=%d quadric=%d counting=%d -> %d\n", alpha, quadric, counting, (int)ph::mis_escape_row(alpha, quadric != 0, counting != 0));
    }
    const uint32_t keys[] = {0u, 1u, 4095u, 4096u, 4097u, 8191u, 2048u, 2048u + 4096u};
    for (uint32_t key : keys) {
        const uint32_t j = ph::mis_escape_joint_key(key);
        std::printf("joint key=%u -> bin=%u mark=%d\n", key, j & (PH_SORT_KEYS - 1u), (int)((j & PH_ORDER_ESCAPE) != 0u));
    }
    return 0;
}
