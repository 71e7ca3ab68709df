// scene_prep_check.cpp -- stand-alone check of csrc/pt_scene.hip (pt_prepare_scene): what ptx_create computes on the host before it
// uploads, run without a GPU on scenes built in code.  tests/test_scene_prep.py compiles pt_scene.hip (host pass) and this file with
// -fsanitize=address,undefined, links the two objects and runs the result: exit status 0 and no sanitizer report is the test.  Every
// array handed in is a heap array of exactly its size, so a read past a face array, a texture or an index shows.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "pt_scene.h"
#include "pt_kernels.h"

using namespace ptd;

static std::string g_err;
extern "C" void ptx_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }

static int g_fail = 0;
static const char *g_case = "";
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case, #c); g_fail++; } } while (0)

// translate + scale in glm's memory order (columns), with its inverse and inverse transpose
static ptx_geom make_geom(int type, int material, float tx, float ty, float tz, float sx, float sy, float sz) {
    ptx_geom g;
    memset(&g, 0, sizeof g);
    g.type = type; g.materialid = material;
    const float t[3] = {tx, ty, tz}, s[3] = {sx, sy, sz};
    for (int k = 0; k < 3; k++) {
        g.translation[k] = t[k]; g.scale[k] = s[k];
        g.transform[k * 4 + k] = s[k]; g.transform[12 + k] = t[k];
        g.inverseTransform[k * 4 + k] = 1.f / s[k]; g.inverseTransform[12 + k] = -t[k] / s[k];
        g.invTranspose[k * 4 + k] = 1.f / s[k]; g.invTranspose[k * 4 + 3] = -t[k] / s[k];
    }
    g.transform[15] = g.inverseTransform[15] = g.invTranspose[15] = 1.f;
    return g;
}

static void push_tri(std::vector<float> &f, const float a[3], const float b[3], const float c[3]) {
    const float *v[3] = {a, b, c};
    for (int k = 0; k < 3; k++) { f.insert(f.end(), v[k], v[k] + 3); f.push_back(0.25f * k); f.push_back(0.5f); }
}
static std::vector<float> box_mesh() {             // 12 triangles
    std::vector<float> f;
    for (int axis = 0; axis < 3; axis++)
        for (int side = 0; side < 2; side++) {
            float p[4][3];
            for (int k = 0; k < 4; k++) {
                p[k][axis] = side ? 0.5f : -0.5f;
                p[k][(axis + 1) % 3] = (k == 1 || k == 2) ? 0.5f : -0.5f;
                p[k][(axis + 2) % 3] = k >= 2 ? 0.5f : -0.5f;
            }
            push_tri(f, p[0], p[1], p[2]); push_tri(f, p[0], p[2], p[3]);
        }
    return f;
}
static std::vector<float> grid_mesh(int n) {       // n x n quads = 2 n^2 triangles, a gently curved sheet
    std::vector<float> f;
    auto at = [&](int i, int j, float p[3]) { p[0] = (float)i / n - 0.5f; p[2] = (float)j / n - 0.5f; p[1] = 0.1f * sinf(3.f * p[0]) * cosf(2.f * p[2]); };
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            float a[3], b[3], c[3], d[3];
            at(i, j, a); at(i + 1, j, b); at(i + 1, j + 1, c); at(i, j + 1, d);
            push_tri(f, a, b, c); push_tri(f, a, c, d);
        }
    return f;
}

static std::vector<ptx_material> seven_materials() {      // light, white, red, green, mirror, glass, the mesh's
    std::vector<ptx_material> m(7);
    memset(m.data(), 0, sizeof(ptx_material) * m.size());
    for (auto &x : m) { x.color[0] = x.color[1] = x.color[2] = 0.8f; }
    m[0].emittance = 5.f; m[2].color[1] = m[2].color[2] = 0.1f; m[3].color[0] = m[3].color[2] = 0.1f;
    m[4].hasReflective = 1.f; m[5].hasRefractive = 1.f; m[5].indexOfRefraction = 1.5f;
    return m;
}
// a Cornell-like box: light, floor, ceiling, back wall, two side walls (cubes), a mirror sphere and a mesh
static std::vector<ptx_geom> cornell(const std::vector<float> &mesh) {
    std::vector<ptx_geom> g;
    g.push_back(make_geom(G_CUBE, 0, 0.f, 10.f, 0.f, 3.f, 0.3f, 3.f));
    g.push_back(make_geom(G_CUBE, 1, 0.f, 0.f, 0.f, 10.f, 0.01f, 10.f));
    g.push_back(make_geom(G_CUBE, 1, 0.f, 10.f, 0.f, 0.01f + 10.f, 0.01f, 10.f));
    g.push_back(make_geom(G_CUBE, 1, 0.f, 5.f, -5.f, 10.f, 10.f, 0.01f));
    g.push_back(make_geom(G_CUBE, 2, -5.f, 5.f, 0.f, 0.01f, 10.f, 10.f));
    g.push_back(make_geom(G_CUBE, 3, 5.f, 5.f, 0.f, 0.01f, 10.f, 10.f));
    g.push_back(make_geom(G_SPHERE, 4, -1.f, 4.f, -1.f, 3.f, 3.f, 3.f));
    ptx_geom m = make_geom(G_OBJ, 6, 2.f, 2.f, 1.f, 2.f, 2.f, 2.f);
    m.faceSize = (int)(mesh.size() / 15); m.faces = m.faceSize ? mesh.data() : nullptr;
    g.push_back(m);
    return g;
}

static int runs_of(unsigned long long mask) { int n = 0; for (int b = 0; b < 64; b++) n += ((mask >> b) & 1) && !(b && ((mask >> (b - 1)) & 1)); return n; }
static size_t lds_need(int table_words, int nbins) { return sizeof(int32_t) * (bounceLdsWords(table_words, nbins) + QUEUE_WORDS); }
static ptx_options default_options() {          // ptx_default_options
    ptx_options o;
    memset(&o, 0, sizeof o);
    o.cache_first_bounce = 1; o.sort_by_material = 1; o.antialiasing = 1; o.tile_world = 1; o.device = -1;
    return o;
}

// pt_prepare_scene on the scene, then everything that must hold for any scene it accepts
static int prepare(const char *name, const std::vector<ptx_geom> &g, const std::vector<ptx_material> &m, const ptx_options &opt, size_t lds_limit,
                   const SceneSwitches &sw, HostScene &hs, int owned = 480 * 270) {
    g_case = name; g_err.clear();
    const int ng = (int)g.size(), nm = (int)m.size(), nbins = opt.sort_by_material ? (nm > 0 ? nm : 1) : 1;
    const int rc = pt_prepare_scene(ng, ng ? g.data() : nullptr, nm, nm ? m.data() : nullptr, opt, owned, nbins, lds_limit, sw, hs);
    if (rc != PTX_OK) return rc;
    const size_t ng1 = ng > 0 ? ng : 1, nm1 = nm > 0 ? nm : 1, nt1 = hs.ntri > 0 ? hs.ntri : 1;
    int nfaces = 0;
    for (const ptx_geom &x : g) nfaces += x.faceSize;
    CHECK(hs.ntri == nfaces);
    CHECK(hs.geoms.size() == ng1 && hs.mats.size() == nm1 && hs.h_spec.size() == nm1);
    CHECK(hs.faces.size() == nt1 * 15 && hs.tri9.size() == nt1 * 9 && hs.fnorm.size() == nt1 * 3);
    CHECK(hs.gtab.size() == ng1 * GTAB_WORDS && hs.cnorm.size() == ng1 * 18 && hs.aabb.size() == ng1 * 8 && hs.aabb_ch.size() == ng1 * 8);
    CHECK(hs.roots.size() == ng1 && hs.depths.size() == ng1 && hs.wroots.size() == ng1 && hs.wneeds.size() == ng1);
    CHECK(hs.texels.size() >= 16 || hs.uses_uv);
    CHECK(hs.bvh.nodes.size() == 2 * (size_t)hs.bvh_nodes && hs.bvh.tris.size() % BVH_TRI == 0 && hs.bvh.wide.size() % 4 == 0);
    CHECK((hs.bvh_meshes > 0) == !hs.bvh.nodes.empty());
    CHECK(hs.bvh_stack >= 8 && hs.bvh_stack <= BVH_STACK);
    CHECK(hs.ntri_lds == 0 || (hs.tri_lds && hs.ntri_lds == hs.ntri));
    CHECK(!hs.cull || (hs.tri_lds && ng >= 1 && ng <= 32));
    CHECK(!hs.split_mesh || hs.cull);
    CHECK(lds_need(hs.tri_lds ? sceneTableWords(hs.ntri_lds, nm, ng) : 0, nbins) <= lds_limit);
    // the staged blob: its six sections are the separately held tables, word for word
    if (hs.tri_lds) {
        const size_t nl = hs.split_mesh ? 0 : (size_t)hs.ntri_lds;
        const float *part[6] = {hs.tri9.data(), hs.faces.data(), reinterpret_cast<const float *>(hs.mats.data()), hs.gtab.data(), hs.fnorm.data(), hs.cnorm.data()};
        const size_t len[6] = {nl * 9, nl * 15, (size_t)nm * 11, (size_t)ng * GTAB_WORDS, nl * 3, (size_t)ng * 18};
        size_t sum = 0;
        for (size_t l : len) sum += l;
        CHECK(hs.ldsblob.size() == sum);
        CHECK(sum <= (size_t)sceneTableWords((int)nl, nm, ng));
        size_t off = 0;
        for (int k = 0; k < 6 && off + len[k] <= hs.ldsblob.size(); off += len[k], k++)
            CHECK(len[k] == 0 || memcmp(&hs.ldsblob[off], part[k], sizeof(float) * len[k]) == 0);
    } else CHECK(hs.ldsblob.empty());
    CHECK(runs_of(hs.dir_bins) <= 2 || hs.dir_bins == ~0ull);
    CHECK(runs_of(hs.ntab_bins) <= 2);
    if (nbins < 64) CHECK(hs.dir_bins == ~0ull || (hs.dir_bins >> nbins) == 0);
    if (nbins < 64) CHECK((hs.ntab_bins >> nbins) == 0);
    for (int i = 0; i < ng; i++)                    // the centre / half-extent box contains the corner box
        for (int r = 0; r < 3; r++) {
            const float lo = hs.aabb[(size_t)i * 8 + r], hi = hs.aabb[(size_t)i * 8 + 4 + r], c = hs.aabb_ch[(size_t)i * 8 + r], h = hs.aabb_ch[(size_t)i * 8 + 4 + r];
            CHECK(lo <= hi);
            if (std::isfinite(lo) && std::isfinite(hi)) CHECK((double)c - h <= lo && (double)c + h >= hi);
            else CHECK(c == 0.f && std::isinf(h) && h > 0);
        }
    for (int i = 0; i < ng; i++) {                  // per-geom table and the kind masks
        int32_t ints[4];
        memcpy(ints, &hs.gtab[(size_t)i * GTAB_WORDS + 36], sizeof ints);
        CHECK(ints[0] == g[i].type && ints[1] == g[i].materialid && ints[3] == g[i].faceSize);
        if (i < 32) CHECK((((hs.cube_bits | hs.sphere_bits | hs.mesh_bits) >> i) & 1u) == (g[i].type == G_CUBE || g[i].type == G_SPHERE || g[i].type == G_OBJ));
        if (hs.roots[i] >= 0) CHECK(g[i].type == G_OBJ && g[i].faceSize >= BVH_MIN_FACES && hs.roots[i] < hs.bvh_nodes);
    }
    for (size_t k = 0; k < hs.fnorm.size() && hs.ntri; k += 3) {      // unit normals
        const double l = sqrt((double)hs.fnorm[k] * hs.fnorm[k] + (double)hs.fnorm[k + 1] * hs.fnorm[k + 1] + (double)hs.fnorm[k + 2] * hs.fnorm[k + 2]);
        CHECK(fabs(l - 1.0) < 1e-5);
    }
    return rc;
}

int main() {
    const size_t LDS = 160 * 1024;                  // the MI355X's per-workgroup limit
    const ptx_options opt = default_options();
    const SceneSwitches none;
    const std::vector<ptx_material> mats = seven_materials();
    const std::vector<float> box = box_mesh(), grid = grid_mesh(6);
    HostScene hs, base1, base2;

    // 1. the small-mesh path
    CHECK(prepare("cornell + 12-triangle mesh", cornell(box), mats, opt, LDS, none, base1) == PTX_OK);
    CHECK(base1.ntri == 12 && base1.mesh_chunks == (12 + MESH_CHUNK - 1) / MESH_CHUNK && base1.bvh_meshes == 0 && !base1.split_mesh);
    CHECK(base1.tri_lds == 1 && base1.ntri_lds == 12 && base1.cull == 1 && base1.uses_uv == 0 && base1.bump_bits == 0);
    CHECK(base1.cube_bits == 0x3fu && base1.sphere_bits == 0x40u && base1.mesh_bits == 0x80u);
    CHECK(base1.ldsblob.size() == 12 * 27 + 7 * 11 + 8 * 58);
    CHECK(base1.h_spec == std::vector<uint8_t>({0, 0, 0, 0, 1, 1, 0}));
    // bins = 6 - material: mirror (2), glass (1) and the mesh's material (0) need the direction; materials 0 .. 3 are on cubes only (bins 3 .. 6)
    CHECK(base1.dir_bins == 0x7ull && base1.ntab_bins == 0x78ull);
    // 2. a mesh with a BVH: the split mesh search
    CHECK(prepare("cornell + 72-triangle grid", cornell(grid), mats, opt, LDS, none, base2) == PTX_OK);
    CHECK(base2.ntri == 72 && base2.bvh_meshes == 1 && base2.split_mesh && base2.mesh_chunks == 1 && base2.roots[7] >= 0 && base2.depths[7] >= 1);
    CHECK(base2.bvh.tris.size() == 72 * (size_t)BVH_TRI && !base2.bvh.wide.empty() && base2.wroots[7] >= 0 && base2.wneeds[7] >= 1);
    CHECK(base2.ldsblob.size() == 7 * 11 + 8 * 58);          // (split: without the triangle tables)
    for (int i = 0; i < 7; i++) CHECK(base2.roots[i] == -1 && base2.wroots[i] == -1);
    {   // ... and with no_bvh / no_mesh_split
        ptx_options o = opt; o.no_bvh = 1;
        CHECK(prepare("grid, no_bvh", cornell(grid), mats, o, LDS, none, hs) == PTX_OK && hs.bvh_meshes == 0 && !hs.split_mesh && hs.mesh_chunks == (72 + MESH_CHUNK - 1) / MESH_CHUNK);
        o = opt; o.no_mesh_split = 1;
        CHECK(prepare("grid, no_mesh_split", cornell(grid), mats, o, LDS, none, hs) == PTX_OK && hs.bvh_meshes == 1 && !hs.split_mesh);
        CHECK(hs.ldsblob.size() == 72 * 27 + 7 * 11 + 8 * 58);
        o = opt; o.sort_by_material = 0;
        CHECK(prepare("box, one bin", cornell(box), mats, o, LDS, none, hs) == PTX_OK && hs.dir_bins == 1ull && hs.ntab_bins == 0ull);
        o = opt; o.no_cull = 1;
        CHECK(prepare("box, no_cull", cornell(box), mats, o, LDS, none, hs) == PTX_OK && !hs.cull && hs.ntab_bins == 0ull && hs.dir_bins == 0x7ull);
        o = opt; o.no_lds_triangles = 1;
        CHECK(prepare("box, no_lds_triangles", cornell(box), mats, o, LDS, none, hs) == PTX_OK && !hs.tri_lds && !hs.cull && hs.ldsblob.empty());
    }
    // 3. the edges
    CHECK(prepare("nothing", {}, {}, opt, LDS, none, hs) == PTX_OK && hs.ntri == 0 && !hs.cull && hs.ldsblob.empty() && hs.dir_bins == ~0ull);
    {
        std::vector<ptx_geom> g;
        for (int i = 0; i < 33; i++) g.push_back(make_geom(G_CUBE, i % 7, (float)i, 0.f, 0.f, 1.f, 1.f, 1.f));
        CHECK(prepare("33 geoms", g, mats, opt, LDS, none, hs) == PTX_OK && !hs.cull && hs.bump_bits == 0xffffffffu && hs.cube_bits == 0xffffffffu && hs.ntab_bins == 0ull);
    }
    {
        CHECK(prepare("OBJ geom without faces", cornell({}), mats, opt, LDS, none, hs) == PTX_OK && hs.ntri == 0 && hs.mesh_bits == 0x80u);
        CHECK(hs.aabb[7 * 8] == -INFINITY && hs.aabb[7 * 8 + 4] == INFINITY && hs.aabb_ch[7 * 8 + 4] == INFINITY);
    }
    {   // textures: three channels are copied (kd, then the bump map: its geom's normals are not tabulated), two are refused
        std::vector<uint8_t> img3(2 * 2 * 3, 200), img4(3 * 1 * 4, 100), img2(2 * 2 * 2, 50);
        std::vector<ptx_geom> g = cornell(box);
        g[7].kd.width = 2; g[7].kd.height = 2; g[7].kd.channels = 3; g[7].kd.image = img3.data();
        g[7].bump.width = 3; g[7].bump.height = 1; g[7].bump.channels = 4; g[7].bump.image = img4.data();
        CHECK(prepare("textured mesh", g, mats, opt, LDS, none, hs) == PTX_OK && hs.uses_uv == 1 && hs.texels.size() == 24 && hs.bump_bits == 0x80u);
        CHECK(hs.geoms[7].tex[0].off == 0 && hs.geoms[7].tex[3].off == 12 && hs.geoms[7].tex[3].ch == 4 && hs.texels[11] == 200 && hs.texels[12] == 100);
        g[7].ke.width = 2; g[7].ke.height = 2; g[7].ke.channels = 2; g[7].ke.image = img2.data();
        CHECK(prepare("two-channel texture", g, mats, opt, LDS, none, hs) == PTX_ERR_UNSUPPORTED && g_err == "textures need >= 3 channels");
    }
    {   // the LDS limit stepped down: first the triangle tables leave LDS, then all tables, then the scene is refused
        const size_t full = lds_need(sceneTableWords(12, 7, 8), 7), mid = lds_need(sceneTableWords(0, 7, 8), 7), bare = lds_need(0, 7);
        CHECK(prepare("LDS: everything fits", cornell(box), mats, opt, full, none, hs) == PTX_OK && hs.tri_lds && hs.ntri_lds == 12 && hs.cull);
        CHECK(prepare("LDS: no triangle tables", cornell(box), mats, opt, full - 1, none, hs) == PTX_OK && hs.tri_lds && hs.ntri_lds == 0 && hs.cull);
        CHECK(hs.ldsblob.size() == 7 * 11 + 8 * 58);
        CHECK(prepare("LDS: exactly the geom tables", cornell(box), mats, opt, mid, none, hs) == PTX_OK && hs.tri_lds && hs.ntri_lds == 0);
        CHECK(prepare("LDS: no tables", cornell(box), mats, opt, mid - 1, none, hs) == PTX_OK && !hs.tri_lds && !hs.cull && hs.ntab_bins == 0ull);
        CHECK(prepare("LDS: bare", cornell(box), mats, opt, bare, none, hs) == PTX_OK && !hs.tri_lds);
        CHECK(prepare("LDS: refused", cornell(box), mats, opt, bare - 1, none, hs) == PTX_ERR_UNSUPPORTED);
        CHECK(g_err == "material sort over 7 materials needs " + std::to_string(bare) + " bytes of LDS per workgroup, the device offers " +
                       std::to_string(bare - 1) + ": render with sort_by_material = 0 (same image only if the reference is built with SORT_BY_MATERIAL 0 too)");
    }
    {   // the five switches, one at a time
        SceneSwitches sw;
        sw.no_wide_bvh = true;
        CHECK(prepare("NO_WIDE_BVH", cornell(grid), mats, opt, LDS, sw, hs) == PTX_OK && hs.bvh_meshes == 1 && hs.roots[7] >= 0 && hs.wroots[7] == -1 && hs.bvh.wide.empty());
        CHECK(hs.bvh.nodes.size() == base2.bvh.nodes.size() && hs.bvh_stack >= 8);
        sw = SceneSwitches(); sw.no_chunks = true;
        CHECK(prepare("NO_CHUNKS", cornell(box), mats, opt, LDS, sw, hs) == PTX_OK && hs.mesh_chunks == 1 && hs.ldsblob == base1.ldsblob);
        sw = SceneSwitches(); sw.no_dir_skip = true;
        CHECK(prepare("NO_DIR_SKIP", cornell(box), mats, opt, LDS, sw, hs) == PTX_OK && hs.dir_bins == ~0ull && hs.ntab_bins == 0ull);
        sw = SceneSwitches(); sw.no_normal_codes = true;
        CHECK(prepare("NO_NORMAL_CODES", cornell(box), mats, opt, LDS, sw, hs) == PTX_OK && hs.dir_bins == base1.dir_bins && hs.ntab_bins == 0ull);
        sw = SceneSwitches(); sw.force_split = true;
        CHECK(prepare("FORCE_SPLIT", cornell(box), mats, opt, LDS, sw, hs) == PTX_OK && hs.split_mesh && hs.bvh_meshes == 0 && hs.ldsblob.size() == 7 * 11 + 8 * 58);
    }
    // 2^28 owned pixels: no room for the normal code in the pixel slot
    CHECK(prepare("2^28 owned pixels", cornell(box), mats, opt, LDS, none, hs, 1 << 28) == PTX_OK && hs.ntab_bins == 0ull && hs.dir_bins == base1.dir_bins);
    // the triangle table both callers share
    {
        const std::vector<float> t9 = triangle_table(box.data(), 12);
        CHECK(t9.size() == 12 * 9 && memcmp(t9.data(), base1.tri9.data(), sizeof(float) * t9.size()) == 0);
        CHECK(t9[3] == box[5] - box[0] && t9[6] == box[10] - box[0]);
    }
    printf("scene_prep_check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
