// Which part of a round's queue each block of the ray binning (raysort.h) owns, and how it reads it.  Both passes over the keys must give block b the same
// slice, since the first pass claims b's share of every bin and the second fills exactly that share: one function, one grid.  A slice [lo, hi) of the joint
// index space (closest-hit keys 0 .. n_cl, any-hit keys behind them) is a run of keys_cl followed by a run of keys_sh; each run is read with scalar loads up
// to the first 16-byte boundary of its own array, 16-byte loads from there, and a scalar tail.
// Plain integer arithmetic, no device code: scripts/raysort_plan_check.cpp runs it on the CPU (tests/test_raysort_plan_cpu.py holds the cases).
#pragma once
#include <cstdint>

namespace ph {

#define PH_SORT_BINS 4096u            // per ray kind
#define PH_SORT_KEYS (2u * PH_SORT_BINS)
#define PH_SORT_BLOCK 256
// A slice is never shorter than this (unless the round is): a block clears, flushes and claims PH_SORT_KEYS bins whatever it holds, so a late round of few rays is
// served by few blocks and the others leave before they touch LDS.  Swept on the configs[2] frame (sum of the three kernels per frame, one kernel trace each): floor 256 (no
// floor to speak of) 9.32 ms, 4 096: 9.21, 16 384: 9.18, 65 536: 9.40 — flat within 0.2 ms, no more than two traces of one build differ by, so the value is the one the sweep started from:
// about where a block's fixed work (three passes over 8 192 bins) and its keys weigh the same.
#define PH_SORT_FLOOR 16384u

#if defined(__HIPCC__)
#define PH_PLAN_HD __host__ __device__ inline
#else
#define PH_PLAN_HD inline
#endif

// One run, in indices of its own array: scalar [head, body), 16-byte loads over [body, tail) (a multiple of four keys, starting on a 16-byte boundary), scalar [tail, end)
struct RaySortRun { uint32_t head, body, tail, end; };
struct RaySortSlice { uint32_t lo, hi; RaySortRun cl, sh; };

// keys per block: ceil(n / grid) rounded up to the block size, at least `floor`.  n <= 0x7FFF0000 (ChunkPolicy::limit): the sums below stay under 2^32
PH_PLAN_HD uint32_t raysort_slice_keys(uint32_t n, uint32_t grid, uint32_t block, uint32_t floor) {
    const uint32_t each = (n + grid - 1u) / grid;
    const uint32_t per = (each + block - 1u) / block * block;
    return per > floor ? per : floor;
}

// [a, e) of an array whose first key lies `mis` keys behind a 16-byte boundary (mis = (address / 4) & 3; 0 for an allocation of its own)
PH_PLAN_HD RaySortRun raysort_run(uint32_t a, uint32_t e, uint32_t mis) {
    RaySortRun r;
    r.head = a; r.end = e;
    const uint32_t to_boundary = (4u - ((a + mis) & 3u)) & 3u;
    r.body = e - a < to_boundary ? e : a + to_boundary;
    r.tail = r.body + ((e - r.body) & ~3u);
    return r;
}

PH_PLAN_HD RaySortSlice raysort_plan(uint32_t n_cl, uint32_t n_sh, uint32_t grid, uint32_t block, uint32_t floor, uint32_t b, uint32_t mis_cl, uint32_t mis_sh) {
    const uint32_t n = n_cl + n_sh;
    const uint64_t per = raysort_slice_keys(n, grid, block, floor);
    const uint64_t lo64 = (uint64_t)b * per, hi64 = lo64 + per;     // (b * per passes 2^32 for the trailing blocks of a large grid)
    RaySortSlice s;
    s.lo = lo64 < n ? (uint32_t)lo64 : n;
    s.hi = hi64 < n ? (uint32_t)hi64 : n;
    const uint32_t cl_a = s.lo < n_cl ? s.lo : n_cl, cl_e = s.hi < n_cl ? s.hi : n_cl;
    s.cl = raysort_run(cl_a, cl_e, mis_cl);
    s.sh = raysort_run(s.lo - cl_a, s.hi - cl_e, mis_sh);
    return s;
}

}  // namespace ph
