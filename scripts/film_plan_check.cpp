// The film geometry (pbrt-v3-rs_amd/csrc/film_plan.h) brute-forced on the CPU against the reference's rules restated literally: Film::get_sample_bounds and get_film_tile
// (film/mod.rs:150-198) and the float32 pixel range of FilmTile::add_sample (film_tile.rs:62-108).  Needs neither the built library nor a device.  One axis: x and y share the rules.
// For every radius, pixel, tile size, crop and candidate film position of the sets below it checks
//     reach        the gather (reach_columns, the rounded-up mark, then sample_reaches) takes a sample if and only if add_sample adds it to the pixel
//     slot         every tile's pixel bounds fit slot_extent
//     tile range   tiles_holding contains every tile whose pixel bounds hold the pixel
// and prints one line per failure (at most 40 of each kind) and the totals; the exit status is 1 if anything failed.  tests/test_film_plan_cpu.py runs it.
// Build and run under the address and undefined-behaviour sanitizers:  bash scripts/film_plan_check.sh
#ifndef FILM_PLAN_HEADER   // (another statement of the same functions can be put to the same check)
#define FILM_PLAN_HEADER "../pbrt-v3-rs_amd/csrc/film_plan.h"
#endif
#include FILM_PLAN_HEADER
#include <cmath>
#include <cstdio>
#include <vector>

namespace ref {   // the reference, literally; nothing here comes from film_plan.h
static int as_i32(float f) { if (f != f) return 0; if (f >= 2147483648.0f) return 2147483647; if (f <= -2147483648.0f) return (int)0x80000000; return (int)f; }
struct Axis { int c0, c1; float r; int ts, s0, s1, nt; };
static Axis axis(int c0, int c1, float r, int ts) {
    Axis a{c0, c1, r, ts, 0, 0, 0};
    a.s0 = as_i32(std::floor((float)c0 + 0.5f - r)); a.s1 = as_i32(std::ceil((float)c1 - 0.5f + r));   // film/mod.rs:150-159
    a.nt = (a.s1 - a.s0 + ts - 1) / ts;                                                               // sampler_integrator.rs:252-259
    return a;
}
static void tile(const Axis& a, int t, int* tb0, int* tb1, int* pb0, int* pb1) {
    *tb0 = a.s0 + t * a.ts; *tb1 = std::min(*tb0 + a.ts, a.s1);                                       // sampler_integrator.rs:331-336
    const int p0 = as_i32(std::ceil((float)*tb0 - 0.5f - a.r)), p1 = as_i32(std::floor((float)*tb1 - 0.5f + a.r)) + 1;   // film/mod.rs:182-198
    *pb0 = std::max(p0, a.c0); *pb1 = std::min(p1, a.c1);
}
static bool adds(float p, float r, int x, int pb0, int pb1) {                                          // film_tile.rs:70-84
    const float pd = p - 0.5f;
    int p0 = as_i32(std::ceil(pd - r)), p1 = as_i32(std::floor(pd + r)) + 1;
    p0 = std::max(p0, pb0); p1 = std::min(p1, pb1);
    return x >= p0 && x < p1;
}
}  // namespace ref

static int fails[3] = {0, 0, 0};
static unsigned long long n_reach = 0, n_added = 0, n_added_rounded = 0, n_added_edge_column = 0, n_slot = 0, n_range = 0;
static float step(float f, int n) { for (; n > 0; n--) f = std::nextafterf(f, INFINITY); for (; n < 0; n++) f = std::nextafterf(f, -INFINITY); return f; }

static void check_axis(int c0, int c1, float r, int ts, int x) {
    const ref::Axis a = ref::axis(c0, c1, r, ts);
    if (a.nt <= 0) return;
    // the grid itself
    const int s0 = phfilm::sample_begin(c0, r), s1 = phfilm::sample_end(c1, r), nt = phfilm::tile_count(s0, s1, ts);
    if (s0 != a.s0 || s1 != a.s1 || nt != a.nt) { if (fails[1]++ < 40) std::printf("FAIL grid: crop [%d, %d) r %.9g tile %d\n", c0, c1, r, ts); return; }
    // slot: every tile's pixel bounds fit
    const int slot = phfilm::slot_extent(c0, c1, r, ts);
    for (int t = 0; t < a.nt; t++) {
        int tb0, tb1, pb0, pb1, qa, qb, q0, q1;
        ref::tile(a, t, &tb0, &tb1, &pb0, &pb1);
        phfilm::tile_samples(s0, s1, ts, t, &qa, &qb); phfilm::tile_pixels(qa, qb, r, c0, c1, &q0, &q1);
        n_slot++;
        if (qa != tb0 || qb != tb1 || q0 != pb0 || q1 != pb1 || pb1 - pb0 > slot)
            if (fails[1]++ < 40) std::printf("FAIL slot: crop [%d, %d) r %.9g tile size %d: tile %d has pixels [%d, %d), %d wide; the slot is %d\n", c0, c1, r, ts, t, pb0, pb1, pb1 - pb0, slot);
    }
    if (x < c0 || x >= c1) return;
    // tile range: every tile whose pixel bounds hold x
    int lo, hi;
    phfilm::tiles_holding(x, r, s0, ts, nt, &lo, &hi);
    for (int t = 0; t < a.nt; t++) {
        int tb0, tb1, pb0, pb1;
        ref::tile(a, t, &tb0, &tb1, &pb0, &pb1);
        if (x < pb0 || x >= pb1) continue;
        n_range++;
        if (t < lo || t > hi) if (fails[2]++ < 40) std::printf("FAIL tile range: crop [%d, %d) r %.9g tile size %d pixel %d: tile %d holds it, the range is [%d, %d]\n", c0, c1, r, ts, x, t, lo, hi);
    }
    // reach: every candidate position of every sample column within r + 3 of the pixel
    const int span = (int)std::ceil(r) + 3;
    const float fr = r - std::floor(r), fracs[4] = {0.5f, fr, (0.5f + r) - std::floor(0.5f + r), (0.5f - r) - std::floor(0.5f - r)};
    for (int sx = std::max(x - span, a.s0); sx <= std::min(x + span, a.s1 - 1); sx++) {
        const int t = (sx - a.s0) / ts;
        int tb0, tb1, pb0, pb1;
        ref::tile(a, t, &tb0, &tb1, &pb0, &pb1);
        if (x < pb0 || x >= pb1) continue;   // the tile keeps no sum for x: add_sample clips to its bounds, and the film pass has no thread there
        std::vector<float> cand;
        for (int k = 0; k <= 5; k++) { cand.push_back(step((float)sx, k)); cand.push_back(step((float)(sx + 1), -k)); }
        for (float f : fracs) for (int k = -3; k <= 3; k++) cand.push_back(step((float)sx + f, k));
        const phfilm::Reach c = phfilm::reach_columns(x, r, tb0, tb1);
        bool marked = false;   // raygen's mark of the sample's pixel: some sample of it lies ON the next coordinate.  Both states are tried for every other sample.
        for (int pass = 0; pass < 2; pass++, marked = true)
            for (float p : cand) {
                if (!(p >= (float)sx && p <= (float)(sx + 1))) continue;   // a sample of pixel sx
                const bool up = phfilm::rounded_up(p, sx);
                if (up && !marked) continue;   // (a pixel with such a sample is marked)
                const bool want = ref::adds(p, r, x, pb0, pb1);
                const bool scanned = sx >= c.lo && sx <= c.hi && (sx >= c.full || marked);
                const bool got = scanned && phfilm::sample_reaches(p, r, x, pb0, pb1);
                n_reach++;
                if (want) { n_added++; if (up) n_added_rounded++; if (sx < c.full) n_added_edge_column++; }
                if (want != got && fails[0]++ < 40)
                    std::printf("FAIL reach: crop [%d, %d) r %.9g tile size %d: pixel %d, sample %.9g of pixel %d (tile samples [%d, %d)): the reference %s, the gather scans [%d, %d] (from %d on unmarked) and %s\n",
                                c0, c1, r, ts, x, p, sx, tb0, tb1, want ? "adds it" : "does not add it", c.lo, c.hi, c.full, got ? "adds it" : "does not");
            }
    }
}

int main() {
    std::vector<float> radii = {0.3f, 0.5f, 0.7f, 1.25f, 1.3f, 1.5f, 2.0f, 2.5f, 4.0f, 17.0f, 1.4998f, 1.0f / 3.0f};
    for (float h : {0.5f, 1.5f, 2.0f, 2.5f}) { radii.push_back(std::nextafterf(h, 0.0f)); radii.push_back(std::nextafterf(h, INFINITY)); }
    std::vector<int> pixels;
    for (int x = -3; x <= 20; x++) pixels.push_back(x);
    for (int k : {512, 1024, 4096, 16384}) for (int d = -2; d <= 2; d++) pixels.push_back(k + d);
    pixels.push_back(1000); pixels.push_back(5000);
    for (float r : radii)
        for (int ts : {1, 2, 3, 16, 64})
            for (int x : pixels) {
                check_axis(x - 37, x + 41, r, ts, x);      // a crop around the pixel, not aligned to tiles
                check_axis(x, x + 1, r, ts, x);            // one pixel wide
                check_axis(x - 1, x + 2, r, ts, x);
                if (x >= 0 && x <= 20) check_axis(0, 24, r, ts, x);   // at the origin: negative sample bounds
                if (x >= 0 && x > 20) check_axis(0, x + 3, r, ts == 1 ? 2 : ts, x);   // a whole film up to the pixel (tile size 1 is covered above)
                if (x < 0) check_axis(-7, 5, r, ts, x);    // negative pixels: the arithmetic does not know a film starts at 0
            }
    std::printf("reach %llu added %llu added_rounded_up %llu added_from_edge_column %llu slot %llu tile_range %llu\n", n_reach, n_added, n_added_rounded, n_added_edge_column, n_slot, n_range);
    std::printf("failures reach %d slot %d tile_range %d\n", fails[0], fails[1], fails[2]);
    return fails[0] || fails[1] || fails[2] ? 1 : 0;
}
