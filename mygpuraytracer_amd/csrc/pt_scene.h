// pt_scene.h -- scene preparation (pt_scene.hip): everything ptx_create computes on the host from the caller's geoms and materials
// before anything is uploaded.  The unit holds no kernel and calls no hip* runtime function, so a CPU program can link it without a GPU
// (tests/scene_prep_check.cpp does, under the sanitizers).  Errors go through ptx_internal_set_error (pt_engine.hip holds the string).
#pragma once
#include "../../include/mi355x_pathtracer.h"
#include "pt_device.h"
#include "pt_bvh.h"

namespace ptd {

// The PTX_DEBUG_* variables this phase depends on, read by ptx_create (pt_prepare_scene reads no environment).
struct SceneSwitches {
    bool no_wide_bvh = false;          // PTX_DEBUG_NO_WIDE_BVH: no four-wide nodes (A/B timing, tests of both walks)
    bool no_chunks = false;            // PTX_DEBUG_NO_CHUNKS: small meshes' loops are not spread over lanes
    bool no_dir_skip = false;          // PTX_DEBUG_NO_DIR_SKIP: every record carries direction and normal
    bool no_normal_codes = false;      // PTX_DEBUG_NO_NORMAL_CODES: every record carries its normal
    bool force_split = false;          // PTX_DEBUG_FORCE_SPLIT: the split mesh search for any scene with a mesh (timing experiments only)
    bool no_objcull = false;           // PTX_DEBUG_NO_OBJCULL: no small mesh gets an object-space box, its candidates come from the world box (A/B timing, tests of both)
};

// What the scene decides about how it is traced: the tracer (ptx_tracer) keeps these by the same names.
struct SceneFacts {
    int ntri = 0, bvh_meshes = 0, bvh_nodes = 0, bvh_stack = BVH_STACK;
    int mesh_chunks = 1;                                 // see DScene::mesh_chunks
    int uses_uv = 0;
    uint32_t cube_bits = 0, sphere_bits = 0, mesh_bits = 0;   // geoms 0..31 by kind, for the candidate masks
    uint32_t bump_bits = 0;
    uint32_t light_bits = 0;                             // geoms 0..31 whose material emits (emittance > 0): DScene::light_bits
    uint32_t objcull_bits = 0;                           // small meshes 0..31 with an entry in HostScene::objcull: DScene::objcull_bits
    int tri_lds = 0, ntri_lds = 0, cull = 0;             // cull: 0 off, 1 candidate masks, 2 candidate masks in a scene where rays can start far out (cullMask)
    bool split_mesh = false;                             // k_bounce as MODE 1 + k_mesh + k_finish + MODE 2 (scenes with BVH meshes)
    unsigned long long dir_bins = ~0ull;                 // BounceParams::dir_bins (all ones: every record carries its direction)
    unsigned long long ntab_bins = 0ull;                 // BounceParams::ntab_bins (none: every record carries its normal)
};

struct HostScene : SceneFacts {
    std::vector<DGeom> geoms;
    std::vector<DMaterial> mats;
    std::vector<float> faces, tri9, gtab, fnorm, cnorm;
    std::vector<float> ctan;                             // DScene::ctan: CTAN_WORDS per geom, the tangent frames of the six normals in cnorm (zeros: not a cube)
    std::vector<uint8_t> texels;
    std::vector<float> aabb, aabb_ch;                    // world boxes, 8 floats per geom: corners (lo xyz, 0, hi xyz, 0) / centre and half extent
    std::vector<float> objcull;                          // DScene::objcull: OBJCULL_WORDS per geom, zeros where objcull_bits has no bit
    std::vector<uint8_t> h_spec;                         // per material: reflective or refractive (ptx_denoise_temporal's rule)
    BvhBuild bvh;                                        // pt_bvh.h: binary nodes, leaf triangles, four-wide nodes of every mesh that has a tree
    std::vector<int32_t> roots, depths, wroots, wneeds;  // per geom (-1 / 0: no tree)
    std::vector<float> ldsblob;                          // DScene::ldsblob: tri9, faces, materials, gtab, fnorm, cnorm as k_bounce stages them
                                                         // (split: without the triangle tables); empty when the tables are not staged
};

// Flattens ptx_geom / ptx_material into the device structs and builds every derived table.  owned = pixels this device owns, nbins =
// material bins of the sort, lds_limit = the device's LDS per workgroup in bytes.  Returns PTX_OK or the error code, its text set.
int pt_prepare_scene(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials, const ptx_options &opt, int owned,
                     int nbins, size_t lds_limit, const SceneSwitches &sw, HostScene &out);

// upload-time triangle table for the intersection loop, 9 floats per face: v0, e1 = v1 - v0, e2 = v2 - v0
std::vector<float> triangle_table(const float *faces15, int nfaces);
void tile_geom_masks(const DCamera &c, int tile_rows, int tile_rank, int tile_world, int owned, int maxTiles, int ngeoms, const float *aabb8,
                     bool dof, std::vector<uint32_t> &masks);
void camera_to_device(const ptx_camera &c, DCamera &d);
int owned_pixels(int W, int H, int tile_rows, int tile_rank, int tile_world);      // pixels of the row blocks this rank owns
// bit g (g < 32): geom g's material has emittance > 0 -- classifyPath's test of a hit's material, per geom
uint32_t light_geom_bits(int nmaterials, const DMaterial *mats, int ngeoms, const int32_t *geom_material);
// The object-space box of one small mesh as cullMask's objBoxReach reads it (OBJCULL_WORDS floats), from the geom's inverse transform
// (16 floats, columns) and its faces.  margin = 1: the derived margins (pt_scene.hip); 0: the bare box, which the CPU tests use to show that
// they can fail.  false (out16 zeroed): no entry -- no faces, a singular or non-finite matrix, numbers out of the derivation's range.
bool objcull_entry(const float *inverse16, const float *faces15, int nfaces, double margin, float out16[OBJCULL_WORDS]);
// A cube's six face normals (cnorm18, index (axis * 2 + (sign > 0)) * 3: boxIntersectionTest's normalize(invTranspose * +-e_axis)) and the
// tangent frame of each (ctan36: perp1 xyz, perp2 xyz per side, the diffuse sampler's tangentFrame of the very floats written to cnorm18),
// from rows 0-2 of the cube's invTranspose as gtab holds them (12 floats).
void cube_face_tables(const float *invT_rows12, float *cnorm18, float *ctan36);

}  // namespace ptd
