// The slice plan of the ray binning (pbrt-v3-rs_amd/csrc/raysort_plan.h) on the CPU; needs neither the built library nor a device.  Answers every line of standard input:
//     <n_cl> <n_sh> <grid> <block> <floor> <mis_cl> <mis_sh>
// with one line: for every block up to and including the last one that has work  " <lo> <hi> <cl.head> <cl.body> <cl.tail> <cl.end> <sh.head> <sh.body> <sh.tail> <sh.end>",
// then " | <idle> <clean>": the number of blocks behind those, and whether every one of them got the empty slice [n, n) with empty runs.
// tests/test_raysort_plan_cpu.py holds the cases and checks the answers.  Build and run under the address and undefined-behaviour sanitizers:  bash scripts/raysort_plan_check.sh < cases
#include "../pbrt-v3-rs_amd/csrc/raysort_plan.h"
#include <cstdio>
#include <vector>

int main() {
    unsigned long long n_cl, n_sh, grid, block, floor, mis_cl, mis_sh;
    while (std::scanf("%llu %llu %llu %llu %llu %llu %llu", &n_cl, &n_sh, &grid, &block, &floor, &mis_cl, &mis_sh) == 7) {
        if (!grid || !block || n_cl + n_sh > 0xFFFFFFFFull) return 2;
        const uint32_t n = (uint32_t)(n_cl + n_sh);
        std::vector<ph::RaySortSlice> busy;
        uint32_t idle = 0; bool clean = true;
        for (uint32_t b = 0; b < (uint32_t)grid; b++) {
            const ph::RaySortSlice s = ph::raysort_plan((uint32_t)n_cl, (uint32_t)n_sh, (uint32_t)grid, (uint32_t)block, (uint32_t)floor, b, (uint32_t)mis_cl, (uint32_t)mis_sh);
            if (s.lo < s.hi) {
                if (idle) clean = false;   // work behind an idle block
                busy.push_back(s);
            } else {
                idle++;
                const ph::RaySortRun* runs[2] = {&s.cl, &s.sh};
                for (const ph::RaySortRun* r : runs) clean = clean && r->head == r->end && r->body == r->end && r->tail == r->end;
                clean = clean && s.lo == n && s.hi == n;
            }
        }
        for (const ph::RaySortSlice& s : busy)
            std::printf(" %u %u %u %u %u %u %u %u %u %u", s.lo, s.hi, s.cl.head, s.cl.body, s.cl.tail, s.cl.end, s.sh.head, s.sh.body, s.sh.tail, s.sh.end);
        std::printf(" | %u %d\n", idle, clean ? 1 : 0);
    }
    return 0;
}
