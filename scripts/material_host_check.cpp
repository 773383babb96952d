// Host-only check of csrc/material_host.{h,cpp}: call sequences against the material unit, every result written out as text (tests/golden/material_host_sequences.txt
// is this program's output; tests/test_material_host_cpu.py compares).  The sequences: every constructor over black / non-black colours, every setter on every kind, every
// order of the setters that interact on one material, and MixMaterial's snapshots and limits.  In process it asserts that
//   - a refused call changes nothing (the dump of every material before and after is the same text),
//   - the orders of one set of accepted calls all give one result,
//   - the scene flags (the OR over the live materials) never lose a bit, i.e. they are what flags that are only ever set would be.
// Built by scripts/material_host_check.sh with the address and undefined-behaviour sanitizers; CPU only.
// `--report` turns the first two assertions into a report on stderr (used once, to record what the code before this unit did).
#include "material_host.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <sstream>

using namespace phost;

static bool g_report = false;
static int g_failures = 0, g_reported = 0;
static std::ostringstream g_out;
static std::vector<std::string> g_messages;   // every distinct message, numbered in order of appearance (the legend at the end of the output)

static const char* kColName[10] = {"Kd", "Ks", "Kr", "Kt", "opacity", "amount", "eta", "k", "reflect", "transmit"};
static const char* kFltName[4] = {"sigma", "uroughness", "vroughness", "index"};
static const float kRoughness[] = {0.0f, 0.2f, 0.1f, 0.5f};   // every constant roughness a sequence uses

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float roughness_to_alpha(float roughness) {   // as material_host.cpp's, with this machine's logf
    roughness = roughness > 1e-3f ? roughness : 1e-3f;
    const float x = std::log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
static std::string hexf(float f) { char b[16]; std::snprintf(b, sizeof b, "%08x", bits(f)); return b; }
static std::string alpha(float a) {   // an alpha that came through the host's logf is written as what it was made from: the fixture does not depend on a libm
    for (float x : kRoughness) { const float r = roughness_to_alpha(x); if (bits(a) == bits(0.001f > r ? 0.001f : r)) return "remap(" + hexf(x) + ")"; }
    return hexf(a);
}
struct Line {
    std::ostringstream o;
    void u(const char* n, uint32_t v, uint32_t dflt = 0) { if (v != dflt) o << ' ' << n << '=' << v; }
    void f(const char* n, float v, float dflt = 0.0f) { if (bits(v) != bits(dflt)) o << ' ' << n << '=' << hexf(v); }
    void a(const char* n, float v) { if (bits(v) != 0u) o << ' ' << n << '=' << alpha(v); }
    void f3(const char* n, const float v[3]) { if (bits(v[0]) | bits(v[1]) | bits(v[2])) o << ' ' << n << '=' << hexf(v[0]) << ',' << hexf(v[1]) << ',' << hexf(v[2]); }
};
static std::string dump_material(const MaterialRec& m, const LobeRec* lobes) {
    Line r;
    r.o << "    rec:";
    r.f3("kd", m.kd); r.f("sigma", m.sigma); r.f("a", m.a); r.f("b", m.b); r.u("has_bxdf", m.has_bxdf); r.u("n_lobes", m.n_lobes); r.u("sort_class", m.sort_class);
    r.f("bsdf_eta", m.bsdf_eta, 1.0f); r.u("none", m.none); r.u("kd_tex1", m.kd_tex1); r.u("textured", m.textured); r.u("bump_tex1", m.bump_tex1); r.u("sigma_tex1", m.sigma_tex1);
    r.u("opacity_tex1", m.opacity_tex1); r.u("amount_tex1", m.amount_tex1); r.f("bsdf_eta_alt", m.bsdf_eta_alt); r.u("uber_eta", m.uber_eta); r.u("rt_mode", m.rt_mode);
    r.u("refl_tex1", m.refl_tex1); r.u("trans_tex1", m.trans_tex1); r.f3("refl_c", m.refl_c); r.f3("trans_c", m.trans_c); r.u("index_tex1", m.index_tex1);
    r.u("tex_cols", m.tex_cols); r.u("tex_hdr", m.tex_hdr);
    r.o << '\n';
    for (uint32_t k = 0; k < m.n_lobes; k++) {
        const LobeRec& l = lobes[k];
        Line o;
        o.o << "    lobe " << k << ": kind=" << l.kind << " type=" << l.type;
        o.u("fresnel", l.fresnel); o.u("n_scale", l.n_scale); o.f("a", l.a); o.f("b", l.b); o.a("ax", l.ax); o.a("ay", l.ay); o.f("eta_a", l.eta_a, 1.0f); o.f("eta_b", l.eta_b, 1.0f);
        o.u("eta_tex1", l.eta_tex1); o.u("k_tex1", l.k_tex1); o.f3("r", l.r); o.u("r_tex1", l.r_tex1); o.f3("t", l.t); o.u("t_tex1", l.t_tex1); o.f3("c_eta_t", l.c_eta_t); o.u("amt", l.amt);
        o.f3("c_k", l.c_k); o.u("alt", l.alt); o.f3("scale0", l.scale0); o.f("ur_raw", l.ur_raw); o.f3("scale1", l.scale1); o.f("vr_raw", l.vr_raw); o.u("ax_tex1", l.ax_tex1);
        o.u("ay_tex1", l.ay_tex1); o.u("remap", l.remap); o.u("sigma_tex1", l.sigma_tex1); o.u("slot0", l.slot0); o.f3("pre", l.pre); o.u("has_pre", l.has_pre);
        r.o << o.o.str() << '\n';
    }
    return r.o.str();
}
// every material as upload would lay it out (lobe_base normalised away), and the scene flags
static std::string dump(const MaterialHost& h) {
    std::vector<MaterialRec> recs; std::vector<LobeRec> pool;
    layout_lobe_pool(h, recs, pool);
    const MaterialFlags f = h.flags();
    std::ostringstream o;
    o << "  flags: general=" << f.general << " textured=" << f.textured << " bump=" << f.bump << " has_none=" << f.has_none << '\n';
    for (size_t i = 0; i < recs.size(); i++) o << "  material " << i << ":\n" << dump_material(recs[i], pool.data() + recs[i].lobe_base);
    return o.str();
}

static void fail(const std::string& what) { std::fprintf(stderr, "material_host_check: FAILED: %s\n", what.c_str()); g_failures++; }
static void soft(const std::string& what) {   // an assertion that --report turns into a report
    if (g_report) { std::fprintf(stderr, "material_host_check: report: %s\n", what.c_str()); g_reported++; }
    else fail(what);
}
static std::string result(int rc, const std::string& why) {
    if (rc == PBRT_HIP_OK) return "0";
    size_t k = std::find(g_messages.begin(), g_messages.end(), why) - g_messages.begin();
    if (k == g_messages.size()) g_messages.push_back(why);
    return std::to_string(rc) + " M" + std::to_string(k);
}

// One scene of a sequence.  Every call is logged with its result; a refused call must leave every dump as it was, an accepted one may only add scene flags.
struct Scene {
    MaterialHost h;
    std::string name;
    bool quiet = false;   // the permutation runs log through their own summary
    std::vector<int> rcs;
    void log(const std::string& call, int rc, const std::string& why, const std::string& before, const MaterialFlags& fb) {
        rcs.push_back(rc);
        const std::string after = dump(h);
        const MaterialFlags fa = h.flags();
        if ((fb.general && !fa.general) || (fb.textured && !fa.textured) || (fb.bump && !fa.bump) || (fb.has_none && !fa.has_none)) fail(name + ": " + call + " cleared a scene flag");
        if (rc != PBRT_HIP_OK && after != before) soft(name + ": " + call + " was refused and changed the state");
        if (!quiet) g_out << "  " << call << " -> " << result(rc, why) << (rc != PBRT_HIP_OK ? " unchanged" : "") << '\n';
    }
    int add(const MaterialSpec& s, const std::string& what, uint32_t* id = nullptr) {
        const std::string before = dump(h); const MaterialFlags fb = h.flags();
        std::string why; uint32_t got = 0;
        const int rc = add_material(h, s, &got, why);
        if (id) *id = got;
        log("add " + what, rc, why, before, fb);
        return rc;
    }
    // the setters by one number: 0-9 colour parameters, 10-13 float parameters, 14 bump, 15 / 16 unknown colour / float ids; the texture bound is 10 + that number
    int set(uint32_t m, int which, std::string* out_why = nullptr) {
        const std::string before = dump(h); const MaterialFlags fb = h.flags();
        std::string why; int rc;
        const uint32_t tex = 10u + (uint32_t)which;
        if (which < 10) rc = set_colour_texture(h, m, which, tex, why);
        else if (which < 14) {
            float op[3];
            rc = PBRT_HIP_OK;
            if (which - 10 == PH_FPARAM_INDEX && uber_index_needs_opacity(h, m, op)) rc = set_colour_texture(h, m, PBRT_HIP_PARAM_OPACITY, 98u, why);   // the API layer's constant opacity texture
            if (rc == PBRT_HIP_OK) rc = set_float_texture(h, m, which - 10, tex, why);
        }
        else if (which == 14) rc = set_bump_texture(h, m, tex, why);
        else if (which == 15) rc = set_colour_texture(h, m, 10, tex, why);
        else rc = set_float_texture(h, m, 4, tex, why);
        log("set " + setter_name(which) + " on " + std::to_string(m), rc, why, before, fb);
        if (out_why) *out_why = why;
        return rc;
    }
    static std::string setter_name(int which) { return which < 10 ? kColName[which] : which < 14 ? kFltName[which - 10] : which == 14 ? "bump" : which == 15 ? "colour-id-10" : "float-id-4"; }
};
enum { SET_SIGMA = 10, SET_UROUGH = 11, SET_VROUGH = 12, SET_INDEX = 13, SET_BUMP = 14, N_SETTERS = 17 };

// ---- the constructors' cases -----------------------------------------------------------------------------------------------------------
struct Case { std::string name; MaterialSpec spec; };
static void colour(MaterialSpec& s, int p, float r, float g, float b) { s.col[p][0] = r; s.col[p][1] = g; s.col[p][2] = b; }
static MaterialSpec base_spec(MaterialKind k) {   // every colour non-black (one negative channel for clamp_default), opacity 1
    MaterialSpec s; s.kind = k;
    colour(s, PBRT_HIP_PARAM_KD, 0.5f, 0.25f, 0.125f); colour(s, PBRT_HIP_PARAM_KS, 0.3f, 0.2f, -0.1f); colour(s, PBRT_HIP_PARAM_KR, 0.9f, 0.8f, 0.7f); colour(s, PBRT_HIP_PARAM_KT, 0.6f, 0.7f, 0.8f);
    colour(s, PBRT_HIP_PARAM_OPACITY, 1.0f, 1.0f, 1.0f); colour(s, PBRT_HIP_PARAM_AMOUNT, 0.25f, 0.5f, 0.75f); colour(s, PBRT_HIP_PARAM_ETA, 0.2f, 0.9f, 1.1f); colour(s, PBRT_HIP_PARAM_K, 3.9f, 2.4f, 2.2f);
    colour(s, PBRT_HIP_PARAM_REFLECT, 0.5f, 0.5f, 0.25f); colour(s, PBRT_HIP_PARAM_TRANSMIT, 0.25f, 0.5f, 0.5f);
    s.urough = 0.2f; s.vrough = 0.1f;
    return s;
}
// `base` with every colour of `params` non-black, each black in turn, all black
static void colour_cases(std::vector<Case>& out, const std::string& name, const MaterialSpec& base, std::vector<int> params) {
    out.push_back({name, base});
    if (params.size() > 1)
        for (int p : params) { Case c{name + " " + kColName[p] + "=0", base}; colour(c.spec, p, 0, 0, 0); out.push_back(c); }
    Case c{name + " all=0", base};
    for (int p : params) colour(c.spec, p, 0, -1.0f, 0);   // black after clamp_default
    out.push_back(c);
}
static std::vector<Case> constructor_cases() {
    std::vector<Case> out;
    using K = MaterialKind;
    { MaterialSpec s; s.kind = K::None; out.push_back({"none", s}); }
    for (float sigma : {0.0f, 20.0f}) { MaterialSpec s = base_spec(K::Matte); s.sigma = sigma; colour_cases(out, sigma ? "matte sigma=20" : "matte", s, {PBRT_HIP_PARAM_KD}); }
    colour_cases(out, "mirror", base_spec(K::Mirror), {PBRT_HIP_PARAM_KR});
    colour_cases(out, "plastic", base_spec(K::Plastic), {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS});
    { MaterialSpec s = base_spec(K::Plastic); s.remap = true; out.push_back({"plastic remap", s}); }
    for (int remap = 0; remap < 2; remap++)
        for (int r = 0; r < 3; r++) {
            MaterialSpec s = base_spec(K::Glass); s.remap = remap; s.urough = r ? 0.2f : 0.0f; s.vrough = r == 2 ? 0.1f : 0.0f;
            const std::string name = std::string("glass rough=") + (r == 0 ? "0,0" : r == 1 ? "0.2,0" : "0.2,0.1") + (remap ? " remap" : "");
            if (remap) out.push_back({name, s}); else colour_cases(out, name, s, {PBRT_HIP_PARAM_KR, PBRT_HIP_PARAM_KT});
        }
    for (int remap = 0; remap < 2; remap++) { MaterialSpec s = base_spec(K::Metal); s.remap = remap; out.push_back({remap ? "metal remap" : "metal", s}); }
    for (int remap = 0; remap < 2; remap++)
        for (float op : {1.0f, 0.0f, 0.5f}) {
            MaterialSpec s = base_spec(K::Uber); s.remap = remap; colour(s, PBRT_HIP_PARAM_OPACITY, op, op, op);
            if (remap && op != 0.5f) continue;
            const std::string name = std::string("uber opacity=") + (op == 1.0f ? "1" : op == 0.0f ? "0" : "0.5") + (remap ? " remap" : "");
            if (remap) out.push_back({name, s}); else colour_cases(out, name, s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS, PBRT_HIP_PARAM_KR, PBRT_HIP_PARAM_KT});
        }
    colour_cases(out, "substrate", base_spec(K::Substrate), {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS});
    { MaterialSpec s = base_spec(K::Substrate); s.remap = true; out.push_back({"substrate remap", s}); }
    for (int remap = 0; remap < 2; remap++)
        for (int rt = 0; rt < 4; rt++) {   // reflect and transmit each black, and both
            MaterialSpec s = base_spec(K::Translucent); s.remap = remap;
            if (rt & 1) colour(s, PBRT_HIP_PARAM_REFLECT, 0, 0, 0);
            if (rt & 2) colour(s, PBRT_HIP_PARAM_TRANSMIT, 0, 0, 0);
            if (remap && rt) continue;
            const std::string name = std::string("translucent") + (rt & 1 ? " reflect=0" : "") + (rt & 2 ? " transmit=0" : "") + (remap ? " remap" : "");
            if (remap) out.push_back({name, s}); else colour_cases(out, name, s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS});
        }
    return out;
}

// what changed from dump `base` to dump `now`, line by line and field by field (`-name`: a field back at its default); a line with no counterpart is written whole
static std::string diff_dump(const std::string& base, const std::string& now) {
    auto lines = [](const std::string& t) { std::vector<std::string> v; std::istringstream in(t); for (std::string l; std::getline(in, l);) v.push_back(l); return v; };
    auto fields = [](const std::string& l, std::string& head) { const size_t c = l.find(':'); head = l.substr(0, c + 1); std::vector<std::string> v; std::istringstream in(l.substr(c + 1)); for (std::string f; in >> f;) v.push_back(f); return v; };
    const std::vector<std::string> b = lines(base), n = lines(now);
    std::ostringstream o;
    for (size_t i = 0; i < n.size(); i++) {
        std::string hb, hn;
        const std::vector<std::string> fn = fields(n[i], hn), fb = i < b.size() ? fields(b[i], hb) : std::vector<std::string>();
        if (i >= b.size() || hb != hn) { o << n[i] << '\n'; continue; }
        std::string d;
        for (const std::string& f : fn) if (std::find(fb.begin(), fb.end(), f) == fb.end()) d += " " + f;
        for (const std::string& f : fb) { const std::string name = f.substr(0, f.find('=') + 1); bool kept = false; for (const std::string& g : fn) kept = kept || g.compare(0, name.size(), name) == 0; if (!kept) d += " -" + name.substr(0, name.size() - 1); }
        if (!d.empty()) o << hn << d << '\n';
    }
    if (n.size() < b.size()) o << "    (" << b.size() - n.size() << " lines fewer)\n";
    return o.str();
}
// every constructor case, then every setter on a fresh copy of it: the refused ones on one line, the accepted ones with what they changed
static void run_setters(const std::string& name, const std::function<uint32_t(Scene&)>& make) {
    std::string refused;
    std::ostringstream accepted;
    for (int which = 0; which < N_SETTERS; which++) {
        Scene t; t.name = name; t.quiet = true;
        const uint32_t m = make(t);
        const std::string base = dump(t.h);
        std::string why;
        const int rc = t.set(m, which, &why);
        if (rc == PBRT_HIP_OK) accepted << "  set " << Scene::setter_name(which) << " -> 0\n" << diff_dump(base, dump(t.h));
        else refused += " " + Scene::setter_name(which) + ":" + result(rc, why);
    }
    g_out << "  refused, unchanged:" << refused << '\n' << accepted.str();
}
static void run_constructors_and_setters() {
    for (const Case& c : constructor_cases()) {
        g_out << "== " << c.name << '\n';
        Scene sc; sc.name = c.name;
        if (sc.add(c.spec, c.name) != PBRT_HIP_OK) continue;
        g_out << dump(sc.h);
        run_setters(c.name, [&](Scene& t) { uint32_t id = 0; t.add(c.spec, c.name, &id); return id; });
    }
}

// ---- every order of the setters that interact on one material -----------------------------------------------------------------------------
// The orders are grouped by which calls were accepted (a call refused in one order and accepted in another makes two different sequences).  Within a group the result
// must not depend on the order; the group is written once, from the order in which the structural setters come last.
static void run_orders(const std::string& name, const MaterialSpec& spec, std::vector<int> setters, const std::vector<int>& structural) {
    g_out << "== orders: " << name << " {";
    for (int w : setters) g_out << ' ' << Scene::setter_name(w);
    g_out << " }\n";
    std::sort(setters.begin(), setters.end());
    struct Run { std::vector<int> order; std::string text; long rank; };
    std::map<std::string, std::vector<Run>> groups;   // by the accepted calls
    do {
        Scene sc; sc.name = name; sc.quiet = true;
        sc.add(spec, name);
        std::string key; long rank = 0;
        std::map<int, int> rc_of;
        for (size_t i = 0; i < setters.size(); i++) {
            rc_of[setters[i]] = sc.set(0, setters[i]);
            if (std::find(structural.begin(), structural.end(), setters[i]) != structural.end()) rank += (long)i;
        }
        for (auto& kv : rc_of) key += " " + Scene::setter_name(kv.first) + "=" + std::to_string(kv.second);
        groups[key].push_back(Run{setters, dump(sc.h), rank});
    } while (std::next_permutation(setters.begin(), setters.end()));
    for (auto& g : groups) {
        std::vector<Run>& runs = g.second;
        const Run* canon = &runs[0];
        for (const Run& r : runs) if (r.rank > canon->rank) canon = &r;   // the first of the orders with the structural setters last
        size_t differing = 0;
        for (const Run& r : runs) if (r.text != canon->text) differing++;
        g_out << "  accepted:" << g.first << "; " << runs.size() << " orders; written from";
        for (int w : canon->order) g_out << ' ' << Scene::setter_name(w);
        g_out << '\n' << canon->text;
        if (differing) {
            std::string which;
            for (const Run& r : runs) if (r.text != canon->text) { which += " ["; for (int w : r.order) which += " " + Scene::setter_name(w); which += " ]"; }
            soft(name + ":" + g.first + ": " + std::to_string(differing) + " of " + std::to_string(runs.size()) + " orders differ from the one with the structural setters last:" + which);
        }
    }
}
static void run_all_orders() {
    using K = MaterialKind;
    { MaterialSpec s = base_spec(K::Uber); colour(s, PBRT_HIP_PARAM_OPACITY, 0.5f, 0.5f, 0.5f);
      run_orders("uber opacity=0.5", s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_OPACITY, SET_UROUGH, SET_INDEX}, {PBRT_HIP_PARAM_OPACITY, SET_INDEX});
      colour(s, PBRT_HIP_PARAM_OPACITY, 0, 0, 0);   // op * Kd is black until the opacity is a texture
      run_orders("uber opacity=0", s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_OPACITY, SET_UROUGH, SET_INDEX}, {PBRT_HIP_PARAM_OPACITY, SET_INDEX}); }
    { MaterialSpec s = base_spec(K::Glass); s.urough = s.vrough = 0.0f;
      run_orders("glass smooth", s, {PBRT_HIP_PARAM_KR, PBRT_HIP_PARAM_KT, SET_UROUGH, SET_VROUGH, SET_INDEX}, {SET_UROUGH, SET_VROUGH});
      colour(s, PBRT_HIP_PARAM_KR, 0, 0, 0);
      run_orders("glass smooth Kr=0", s, {PBRT_HIP_PARAM_KR, PBRT_HIP_PARAM_KT, SET_UROUGH, SET_VROUGH, SET_INDEX}, {SET_UROUGH, SET_VROUGH}); }
    { MaterialSpec s = base_spec(K::Translucent);
      run_orders("translucent", s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS, PBRT_HIP_PARAM_REFLECT, PBRT_HIP_PARAM_TRANSMIT, SET_UROUGH}, {PBRT_HIP_PARAM_REFLECT, PBRT_HIP_PARAM_TRANSMIT});
      colour(s, PBRT_HIP_PARAM_REFLECT, 0, 0, 0); colour(s, PBRT_HIP_PARAM_TRANSMIT, 0, 0, 0);   // no BSDF until reflect or transmit is a texture
      run_orders("translucent reflect=0 transmit=0", s, {PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KS, PBRT_HIP_PARAM_REFLECT, PBRT_HIP_PARAM_TRANSMIT, SET_UROUGH}, {PBRT_HIP_PARAM_REFLECT, PBRT_HIP_PARAM_TRANSMIT}); }
}

// ---- MixMaterial --------------------------------------------------------------------------------------------------------------------------
static void run_mixes() {
    using K = MaterialKind;
    const float amount[3] = {0.25f, 0.5f, 0.75f};
    auto mix = [&](Scene& sc, uint32_t a, uint32_t b, uint32_t* id = nullptr) { return sc.add(mix_spec(sc.h, a, b, amount), "mix(" + std::to_string(a) + ", " + std::to_string(b) + ")", id); };
    auto begin = [&](Scene& sc, const char* name) { sc.name = name; g_out << "== mix: " << name << '\n'; };
    auto textured_uber = [&](Scene& sc, int n_cols) {   // an uber with constant opacity and its first n_cols colours textured
        uint32_t id; sc.add(base_spec(K::Uber), "uber", &id);
        for (int p = 0; p < n_cols; p++) sc.set(id, p);
        return id;
    };
    { Scene sc; begin(sc, "plastic + matte"); sc.add(base_spec(K::Plastic), "plastic"); sc.add(base_spec(K::Matte), "matte"); mix(sc, 0, 1); g_out << dump(sc.h);
      run_setters("plastic + matte", [&](Scene& t) { t.add(base_spec(K::Plastic), ""); t.add(base_spec(K::Matte), ""); uint32_t id = 0; mix(t, 0, 1, &id); return id; }); }
    { Scene sc; begin(sc, "a textured child"); sc.add(base_spec(K::Plastic), "plastic"); sc.set(0, PBRT_HIP_PARAM_KS); sc.set(0, SET_UROUGH); sc.add(base_spec(K::Matte), "matte"); sc.set(1, PBRT_HIP_PARAM_KD); sc.set(1, SET_SIGMA);
      mix(sc, 0, 1); g_out << dump(sc.h); }
    { Scene sc; begin(sc, "a bumped first child"); sc.add(base_spec(K::Plastic), "plastic"); sc.set(0, SET_BUMP); sc.add(base_spec(K::Matte), "matte"); mix(sc, 0, 1); g_out << dump(sc.h); }
    { Scene sc; begin(sc, "a bumped second child"); sc.add(base_spec(K::Plastic), "plastic"); sc.add(base_spec(K::Matte), "matte"); sc.set(1, SET_BUMP); mix(sc, 0, 1); g_out << dump(sc.h); }
    { Scene sc; begin(sc, "mix of mix, and a third level"); sc.add(base_spec(K::Plastic), "plastic"); sc.add(base_spec(K::Matte), "matte"); mix(sc, 0, 1); mix(sc, 2, 1); g_out << dump(sc.h);
      mix(sc, 3, 0); mix(sc, 0, 3); }
    { Scene sc; begin(sc, "9 lobes"); MaterialSpec u = base_spec(K::Uber); colour(u, PBRT_HIP_PARAM_OPACITY, 0.5f, 0.5f, 0.5f); sc.add(u, "uber opacity=0.5"); sc.add(base_spec(K::Translucent), "translucent");
      mix(sc, 0, 1); mix(sc, 0, 0); }
    { Scene sc; begin(sc, "two opacity-textured ubers"); sc.add(base_spec(K::Uber), "uber"); sc.set(0, PBRT_HIP_PARAM_OPACITY); sc.add(base_spec(K::Uber), "uber"); sc.set(1, PBRT_HIP_PARAM_OPACITY); sc.add(base_spec(K::Matte), "matte");
      mix(sc, 0, 1); mix(sc, 0, 2); g_out << dump(sc.h); }
    { Scene sc; begin(sc, "children a mix cannot hold"); sc.add(base_spec(K::Glass), "glass"); sc.set(0, SET_INDEX); sc.add(base_spec(K::Translucent), "translucent"); sc.set(1, PBRT_HIP_PARAM_REFLECT);
      sc.add(base_spec(K::Matte), "matte"); mix(sc, 0, 2); mix(sc, 2, 1); mix(sc, 2, 2); sc.set(3, PBRT_HIP_PARAM_AMOUNT); mix(sc, 3, 2); }
    { Scene sc; begin(sc, "an amount texture at the colour limit"); const uint32_t a = textured_uber(sc, 3); sc.add(base_spec(K::Plastic), "plastic"); sc.set(a + 1, PBRT_HIP_PARAM_KD); sc.set(a + 1, PBRT_HIP_PARAM_KS);
      uint32_t m; mix(sc, a, a + 1, &m); sc.set(m, PBRT_HIP_PARAM_AMOUNT); g_out << dump(sc.h); }
    { Scene sc; begin(sc, "an amount texture over the colour limit"); const uint32_t a = textured_uber(sc, 3); const uint32_t b = textured_uber(sc, 3);
      uint32_t m; mix(sc, a, b, &m); g_out << dump(sc.h); sc.set(m, PBRT_HIP_PARAM_AMOUNT); }   // refused: `unchanged` is the comparison of the dumps before and after
    { Scene sc; begin(sc, "more textured colours than a mix holds"); const uint32_t a = textured_uber(sc, 4); const uint32_t b = textured_uber(sc, 3); mix(sc, a, b); }
    { Scene sc; begin(sc, "a child changed after the mix was made"); sc.add(base_spec(K::Plastic), "plastic"); sc.add(base_spec(K::Matte), "matte"); mix(sc, 0, 1);
      std::vector<MaterialRec> r0, r1; std::vector<LobeRec> p0, p1;
      layout_lobe_pool(sc.h, r0, p0);
      const std::string before = dump_material(r0[2], p0.data() + r0[2].lobe_base);
      sc.set(0, PBRT_HIP_PARAM_KD); sc.set(1, SET_SIGMA); sc.set(1, SET_BUMP);
      layout_lobe_pool(sc.h, r1, p1);
      if (dump_material(r1[2], p1.data() + r1[2].lobe_base) != before) fail("a texture set on a child reached the mix made before");
      g_out << dump(sc.h); }
}

int main(int argc, char** argv) {
    g_report = argc > 1 && std::string(argv[1]) == "--report";
    run_constructors_and_setters();
    run_all_orders();
    run_mixes();
    g_out << "== messages\n";
    for (size_t k = 0; k < g_messages.size(); k++) g_out << "  M" << k << ": " << g_messages[k] << '\n';
    std::fputs(g_out.str().c_str(), stdout);
    if (g_reported) std::fprintf(stderr, "material_host_check: %d reports\n", g_reported);
    if (g_failures) { std::fprintf(stderr, "material_host_check: %d assertions FAILED\n", g_failures); return 1; }
    std::fprintf(stderr, "material_host_check: order, refusal and flag assertions passed\n");
    return 0;
}
