// The oracle's MIPMap::lookup (EWA) and MIPMap::triangle (oracle/oracle_texture.hpp) at texel coordinates where the float-to-isize conversions saturate: the footprint loops
// `t0..=t1`, `s0..=s1` (core/src/mipmap/mod.rs:355-357) must run once when both bounds are isize::MAX, and `s0 + 1`, `t0 + 1` of triangle (:293-312) wrap there as the
// reference's release build does.  Builds a 4 x 4 and a 2 x 16 map, calls both functions at st whose texel coordinate st * w - 0.5 is +-2^63, +-2^62, one float32 either side
// of each, and +-3e38, in s, in t and in both, under every wrap mode, and prints the bits of every result.  tests/test_ewa_loop_cpu.py builds it at -O0 and -O2 under the
// address and undefined-behaviour sanitizers (bash scripts/ewa_loop_check.sh <level>) and compares the two outputs.  Needs neither the built library nor a device.
#include "../oracle/oracle_texture.hpp"
#include <cstdio>
#include <cstring>

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void show(const char* what, int map, int wrap, float s, float t, int d, const orc::Spec& v) {
    std::printf("%s map=%d wrap=%d st=%08x,%08x d=%d -> %08x %08x %08x\n", what, map, wrap, bits(s), bits(t), d, bits(v.c[0]), bits(v.c[1]), bits(v.c[2]));
}

int main() {
    const size_t dims[2][2] = {{4, 4}, {2, 16}};
    std::vector<float> coord;   // texel coordinates
    for (float base : {9223372036854775808.0f, 4611686018427387904.0f})
        for (float sign : {1.0f, -1.0f})
            for (float v : {base, std::nextafter(base, 0.0f), std::nextafter(base, 3.0e38f)}) coord.push_back(sign * v);
    coord.push_back(3.0e38f); coord.push_back(-3.0e38f);
    const float derivs[3][4] = {{0.1f, 0.0f, 0.0f, 0.1f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.4f, 0.1f, -0.05f, 0.3f}};
    for (int map = 0; map < 2; map++) {
        const size_t w = dims[map][0], h = dims[map][1];
        std::vector<orc::Spec> img(w * h);
        for (size_t i = 0; i < w * h; i++) img[i] = orc::Spec(0.05f + 0.9f * (float)((i * 7) % 13) / 13.0f, 0.1f + 0.8f * (float)((i * 5) % 11) / 11.0f, 0.9f - 0.7f * (float)((i * 3) % 7) / 7.0f);
        for (int wrap = 0; wrap < 3; wrap++) {
            orc::MipMap m;
            m.filtering = orc::TEX_FILTER_EWA; m.wrap = wrap; m.max_anisotropy = 8.0f; m.is_float = false;
            m.build_from(img, w, h);
            // the case the defect was measured on: st = (2^61, 0.3) on the 4 x 4 map
            show("lookup", map, wrap, 2305843009213693952.0f, 0.3f, 0, m.lookup(orc::V2(2305843009213693952.0f, 0.3f), orc::V2(0.1f, 0.0f), orc::V2(0.0f, 0.1f)));
            for (float c : coord)
                for (int where = 0; where < 3; where++) {   // the coordinate in s, in t, in both; the other one inside the map
                    const float s = where != 1 ? c / (float)w : 0.3f, t = where != 0 ? c / (float)h : 0.3f;
                    for (int d = 0; d < 3; d++)
                        show("lookup", map, wrap, s, t, d, m.lookup(orc::V2(s, t), orc::V2(derivs[d][0], derivs[d][1]), orc::V2(derivs[d][2], derivs[d][3])));
                    for (size_t level = 0; level < m.pyr.size(); level++) {
                        const float sl = where != 1 ? c / (float)m.pyr[level].w : 0.3f, tl = where != 0 ? c / (float)m.pyr[level].h : 0.3f;
                        show("triangle", map, wrap, sl, tl, (int)level, m.triangle(level, orc::V2(sl, tl)));
                    }
                }
        }
    }
    return 0;
}
