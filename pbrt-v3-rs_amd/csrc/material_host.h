// The host's description of materials: what the caller said about each one (MaterialSpec) and the one function that turns a description into the record and the
// lobe list the device reads (derive).  Plain C++: no device header, so scripts/material_host_check.cpp runs all of it on the CPU.
#pragma once
#include "../../include/pbrt_hip.h"
#include "scene_types.h"
#include <string>
#include <vector>

namespace phost {

enum class MaterialKind : uint32_t { None, Matte, Mirror, Plastic, Glass, Metal, Uber, Substrate, Translucent, Mix };
enum { PH_FPARAM_SIGMA = 0, PH_FPARAM_UROUGHNESS = 1, PH_FPARAM_VROUGHNESS = 2, PH_FPARAM_INDEX = 3 };   // pbrt_hip_set_material_float_texture's fparam

struct MaterialSpec {
    MaterialKind kind;
    // the constants as passed, by PBRT_HIP_PARAM_* (eta / k: MetalMaterial's spectra), and the texture bound to each: 0, or 1 + its id
    float col[10][3] = {};
    uint32_t col_tex1[10] = {};
    float sigma = 0.0f, urough = 0.0f, vrough = 0.0f, index = 1.5f;   // by PH_FPARAM_*; plastic's and translucent's single `roughness` is urough
    uint32_t flt_tex1[4] = {};
    bool remap = false;
    uint32_t bump_tex1 = 0;
    // MixMaterial only: the two sub-materials' derived lists and records as they were when the mix was made (mix.rs holds its materials; a texture set on one afterwards does not reach the mix)
    std::vector<LobeRec> child_lobes[2];
    MaterialRec child_rec[2] = {};
    explicit MaterialSpec(MaterialKind kind_ = MaterialKind::None, float urough_ = 0.0f, float vrough_ = 0.0f, bool remap_ = false) : kind(kind_), urough(urough_), vrough(vrough_), remap(remap_) {}
    void set(int param, const float c[3]) { for (int i = 0; i < 3; i++) col[param][i] = c[i]; }
};

// The record and the lobe list of a material (the BxDF list compute_scattering_functions builds, materials/src/*.rs; per-hit forms where a structural parameter is a texture).
// lobe_base, slot0, tex_cols and tex_hdr are left to layout_lobe_pool.  A description the renderer does not take: an error code, `why` says which parameter, nothing else written.
int derive(const MaterialSpec& spec, MaterialRec& rec, std::vector<LobeRec>& lobes, std::string& why);

// colour slots of TexOut a lobe's textured colours take (texture.h: eval_lobe_colours / build_hit_lobes fill and read them by the same rule)
uint32_t lobe_tex_cols(const LobeRec& l);

struct MaterialFlags { bool general = false, textured = false, bump = false, has_none = false; };   // what SceneHostState's flags of the same names mean, for one material or for all

struct MaterialHost {
    struct Item { MaterialSpec spec; MaterialRec rec; std::vector<LobeRec> lobes; };
    std::vector<Item> items;
    size_t size() const { return items.size(); }
    MaterialFlags flags() const;   // the OR over the materials
};

int add_material(MaterialHost& h, const MaterialSpec& spec, uint32_t* out_id, std::string& why);
MaterialSpec mix_spec(const MaterialHost& h, uint32_t material1, uint32_t material2, const float amount[3]);
// the setters: the material's description with one field changed is derived again; stored on success, nothing is touched on failure
int set_colour_texture(MaterialHost& h, uint32_t material, int param, uint32_t texture, std::string& why);
int set_float_texture(MaterialHost& h, uint32_t material, int fparam, uint32_t texture, std::string& why);
int set_bump_texture(MaterialHost& h, uint32_t material, uint32_t texture, std::string& why);
// UberMaterial decides BSDF::eta and the pass-through lobe per hit once `index` is a texture: true where the caller has to bind a constant texture of `opacity` first
bool uber_index_needs_opacity(const MaterialHost& h, uint32_t material, float opacity[3]);
// the device arrays: the lists one after the other, lobe_base / slot0 / tex_cols / tex_hdr set
void layout_lobe_pool(const MaterialHost& h, std::vector<MaterialRec>& recs, std::vector<LobeRec>& pool);

}  // namespace phost
