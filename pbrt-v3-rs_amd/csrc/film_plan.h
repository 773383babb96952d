// The integer geometry of the film side, one axis at a time (x and y follow the same rules): Film::get_sample_bounds (film/mod.rs:150-159), the tile grid of
// SamplerIntegrator::render (sampler_integrator.rs:252-259, 331-336), a tile's FilmTile pixel bounds (film/mod.rs:182-198), the tile-buffer slot that holds any tile's
// pixels, which sample columns of a tile can reach a pixel under FilmTile::add_sample's float32 rule (film_tile.rs:62-108), and which tiles can hold a pixel.
// film_tiles_kernel, merge_kernel, the raygen kernels and the host code that sizes and lists tiles (wavefront.hip, whitted.h, probe.hip) all call these; none keeps a copy.
// Compiles for host and device; scripts/film_plan_check.cpp brute-forces it on the CPU against the reference's rule restated literally.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PH_FILM_FN __host__ __device__ inline
#else
#define PH_FILM_FN inline
#endif

namespace phfilm {

// `as i32` of the reference: saturating, NaN -> 0
PH_FILM_FN int f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (int)0x80000000;
    return (int)f;
}
PH_FILM_FN int imin(int a, int b) { return a < b ? a : b; }
PH_FILM_FN int imax(int a, int b) { return a > b ? a : b; }
// the float32 below a finite f
PH_FILM_FN float f32_below(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) == 0u) u = 0x80000001u;
    else if (u & 0x80000000u) u++;
    else u--;
    memcpy(&f, &u, 4);
    return f;
}

// ---- sample bounds and tiles of one axis -----------------------------------------------------------------------------------------------------------
// Film::get_sample_bounds: the samples [s0, s1) whose filter footprint can touch the crop [c0, c1)
PH_FILM_FN int sample_begin(int c0, float r) { return f2i(floorf((float)c0 + 0.5f - r)); }
PH_FILM_FN int sample_end(int c1, float r) { return f2i(ceilf((float)c1 - 0.5f + r)); }
PH_FILM_FN int tile_count(int s0, int s1, int tile_size) { return imax((s1 - s0 + tile_size - 1) / tile_size, 0); }
// tile t's samples [*a, *b)
PH_FILM_FN void tile_samples(int s0, int s1, int tile_size, int t, int* a, int* b) { *a = s0 + t * tile_size; *b = imin(*a + tile_size, s1); }
// Film::get_film_tile: the pixels [*p0, *p1) a tile with samples [a, b) keeps sums for
PH_FILM_FN void tile_pixels(int a, int b, float r, int c0, int c1, int* p0, int* p1) {
    *p0 = imax(f2i(ceilf((float)a - 0.5f - r)), c0);
    *p1 = imin(f2i(floorf((float)b - 0.5f + r)) + 1, c1);
}
// The tile-buffer slot along this axis.  In exact arithmetic a whole tile's pixels are tile_size + floor(.5 + r) + floor(r - .5) + 1 wide, and callers have sized their buffers
// by that; where r is a hair under a half-integer the float32 sums of tile_pixels land one pixel further out on either side, so the slot is that width or the widest pixel
// range any tile of the frame really has, whichever is larger, and at least 1.
PH_FILM_FN int slot_extent(int c0, int c1, float r, int tile_size) {
    const int s0 = sample_begin(c0, r), s1 = sample_end(c1, r), n = tile_count(s0, s1, tile_size);
    int w = imax(tile_size + f2i(floorf(0.5f + r)) + f2i(floorf(r - 0.5f)) + 1, 1);
    for (int t = 0; t < n; t++) {
        int a, b, p0, p1;
        tile_samples(s0, s1, tile_size, t, &a, &b);
        tile_pixels(a, b, r, c0, c1, &p0, &p1);
        w = imax(w, p1 - p0);
    }
    return w;
}

// ---- reach: FilmTile::add_sample's pixel range of a sample at film position p, before the clip to the tile's pixel bounds ---------------------------
PH_FILM_FN int reach_first(float p, float r) { return f2i(ceilf((p - 0.5f) - r)); }
PH_FILM_FN int reach_last(float p, float r) { return f2i(floorf((p - 0.5f) + r)); }
// ... clipped: does the sample add to pixel x of a tile whose pixels are [p0, p1)?  The only test that decides a contribution.
PH_FILM_FN bool sample_reaches(float p, float r, int x, int p0, int p1) {
    return x >= imax(reach_first(p, r), p0) && x < imin(reach_last(p, r) + 1, p1);
}
// a sample of pixel sx whose float32 position `sx + offset` rounded up ONTO the next pixel's coordinate (beyond x = 512 every offset above 1 - 2^-15 does)
PH_FILM_FN bool rounded_up(float p, int sx) { return p == (float)(sx + 1); }

// Which sample columns [lo, hi] of a tile with samples [t0, t1) can add to pixel x.  The samples of column sx lie in [sx, sx + 1], the upper end included (rounded_up), and
// reach_first / reach_last never decrease with p: column sx can reach x only if its upper end's reach_last is at least x and its lower end's reach_first at most x.  Both are
// evaluated in float32, as add_sample evaluates them, starting from the float64 estimate of x + .5 -+ r and stepping while the test moves; float64 alone is wrong wherever
// the float32 sums round across a whole number (r = 1.5 at x = 2^k + 1, or r a hair under a half-integer).  Columns [lo, full) are reached only by samples ON their upper
// end: the film pass skips their pixels unless raygen marked them (mark_rounded_up).  Empty: lo > hi.
struct Reach { int lo, full, hi; };
PH_FILM_FN Reach reach_columns(int x, float r, int t0, int t1) {
    Reach c;
    if (t1 <= t0) { c.lo = c.full = t0; c.hi = t0 - 1; return c; }
    const double mid = (double)x + 0.5, gl = floor(mid - (double)r), gh = floor(mid + (double)r);
    int lo = gl <= (double)t0 ? t0 : (gl >= (double)t1 ? t1 : (int)gl);
    while (lo > t0 && reach_last((float)lo, r) >= x) lo--;            // column lo - 1 ends on lo
    while (lo < t1 && reach_last((float)(lo + 1), r) < x) lo++;
    int full = lo;
    while (full < t1 && reach_last(f32_below((float)(full + 1)), r) < x) full++;
    int hi = gh < (double)t0 ? t0 - 1 : (gh >= (double)t1 ? t1 - 1 : (int)gh);
    while (hi < t1 - 1 && reach_first((float)(hi + 1), r) <= x) hi++;
    while (hi >= t0 && reach_first((float)hi, r) > x) hi--;
    c.lo = lo; c.full = full; c.hi = hi;
    return c;
}

// ---- merge: the tiles [*lo, *hi] of this axis among which every tile whose pixel bounds hold pixel x lies (a superset; tile_pixels decides) ------------
PH_FILM_FN void tiles_holding(int x, float r, int s0, int tile_size, int n_tiles, int* lo, int* hi) {
    const int ext = (int)ceilf(r + 0.5f) + 1;
    *lo = imax((x - ext - s0) / tile_size - 1, 0);      // (the division truncates towards zero where the numerator is negative: the margin of one tile covers it)
    *hi = imin((x + ext - s0) / tile_size + 1, n_tiles - 1);
}

#if defined(__HIPCC__)
// raygen's side of Reach::full, one byte per pixel of the band (every writer writes the same byte): this pixel has a sample ON the next column's or row's coordinate
__device__ __forceinline__ void mark_rounded_up(uint8_t* px_rounded, size_t pix, int sx, int sy, float px, float py) {
    if (rounded_up(px, sx) || rounded_up(py, sy)) px_rounded[pix] = 1u;
}
#endif

}  // namespace phfilm
