// light_bits_check.cpp -- stand-alone check of the emitting-geom mask (csrc/pt_scene.hip: light_geom_bits, SceneFacts::light_bits as
// pt_prepare_scene leaves it, and the device-free entry point ptx_debug_light_bits), run without a GPU on scenes built in code.
// tests/test_light_bits.py compiles pt_scene.hip (host pass) and this file with -fsanitize=address,undefined, links the two objects and
// runs the result: exit status 0 and no sanitizer report is the test.  Every array handed in is a heap array of exactly its size, so a
// read past the materials (a geom's material index is the caller's) or past the geoms shows.
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
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static ptx_geom make_geom(int type, int material, float tx, float ty, float tz, float s) {
    ptx_geom g;
    memset(&g, 0, sizeof g);
    g.type = type; g.materialid = material;
    const float t[3] = {tx, ty, tz};
    for (int k = 0; k < 3; k++) {
        g.translation[k] = t[k]; g.scale[k] = s;
        g.transform[k * 4 + k] = s; g.transform[12 + k] = t[k];
        g.inverseTransform[k * 4 + k] = 1.f / s; g.inverseTransform[12 + k] = -t[k] / s;
        g.invTranspose[k * 4 + k] = 1.f / s; g.invTranspose[k * 4 + 3] = -t[k] / s;
    }
    g.transform[15] = g.inverseTransform[15] = g.invTranspose[15] = 1.f;
    return g;
}

static std::vector<ptx_material> materials(const std::vector<float> &emittance) {
    std::vector<ptx_material> m(emittance.size());
    if (!m.empty()) memset(m.data(), 0, sizeof(ptx_material) * m.size());
    for (size_t k = 0; k < m.size(); k++) { m[k].color[0] = m[k].color[1] = m[k].color[2] = 0.8f; m[k].emittance = emittance[k]; }
    return m;
}

static ptx_options default_options() {
    ptx_options o;
    memset(&o, 0, sizeof o);
    o.cache_first_bounce = 1; o.sort_by_material = 1; o.antialiasing = 1; o.tile_world = 1; o.device = -1;
    return o;
}

// the mask three ways: the rule written out here, pt_prepare_scene's, the entry point's
static void check_scene(const std::vector<ptx_geom> &g, const std::vector<ptx_material> &m) {
    uint32_t want = 0;
    for (size_t i = 0; i < g.size() && i < 32; i++)
        if (g[i].materialid >= 0 && g[i].materialid < (int)m.size() && m[g[i].materialid].emittance > 0.0f) want |= 1u << i;
    HostScene hs;
    const ptx_options opt = default_options();
    const int nm = (int)m.size(), ng = (int)g.size();
    const int rc = pt_prepare_scene(ng, ng ? g.data() : nullptr, nm, nm ? m.data() : nullptr, opt, 64 * 48, nm > 0 ? nm : 1, 160 * 1024, SceneSwitches(), hs);
    CHECK(rc == PTX_OK);
    CHECK(hs.light_bits == want);
    std::vector<int32_t> gm(g.size());                     // (exactly ngeoms entries)
    for (size_t i = 0; i < g.size(); i++) gm[i] = g[i].materialid;
    uint32_t got = 0xdeadbeefu;
    CHECK(ptx_debug_light_bits(nm, nm ? m.data() : nullptr, ng, ng ? gm.data() : nullptr, &got) == 0);
    CHECK(got == want);
}

int main() {
    // a room: light, two walls, a second light that is a sphere, a dark sphere
    check_scene({make_geom(G_CUBE, 0, 0.f, 10.f, 0.f, 3.f), make_geom(G_CUBE, 1, 0.f, 0.f, 0.f, 10.f), make_geom(G_CUBE, 2, -5.f, 5.f, 0.f, 10.f),
                 make_geom(G_SPHERE, 3, 1.f, 3.f, 0.f, 1.5f), make_geom(G_SPHERE, 1, -1.f, 3.f, 0.f, 1.5f)}, materials({5.f, 0.f, 0.f, 0.25f}));
    // nothing emits; nothing at all; no material
    check_scene({make_geom(G_CUBE, 0, 0.f, 10.f, 0.f, 3.f), make_geom(G_SPHERE, 1, 0.f, 3.f, 0.f, 2.f)}, materials({0.f, 0.f}));
    check_scene({}, materials({5.f}));
    check_scene({}, {});
    // a negative emittance is not a light (the test is > 0), nor is a NaN
    check_scene({make_geom(G_CUBE, 0, 0.f, 1.f, 0.f, 1.f), make_geom(G_CUBE, 1, 0.f, 3.f, 0.f, 1.f), make_geom(G_CUBE, 2, 0.f, 5.f, 0.f, 1.f)},
                materials({-1.f, __builtin_nanf(""), 1e-30f}));
    // 32 geoms (bit 31) and 33 (the 33rd has no bit), every other one a light
    for (int n : {32, 33}) {
        std::vector<ptx_geom> g;
        for (int i = 0; i < n; i++) g.push_back(make_geom(i % 3 ? G_CUBE : G_SPHERE, i & 1, (float)(i % 6) - 3.f, 1.f + (float)(i / 6), -1.f, 0.5f));
        check_scene(g, materials({0.f, 2.f}));
    }
    {   // the entry point alone: material indices outside the table set no bit and read nothing; bad arguments are refused
        const std::vector<ptx_material> m = materials({3.f, 0.f});
        const std::vector<int32_t> gm = {0, 1, 2, -1, 0, 1000000};
        uint32_t got = 0;
        CHECK(ptx_debug_light_bits(2, m.data(), (int)gm.size(), gm.data(), &got) == 0 && got == 0x11u);
        CHECK(ptx_debug_light_bits(0, nullptr, (int)gm.size(), gm.data(), &got) == 0 && got == 0u);
        CHECK(ptx_debug_light_bits(2, m.data(), 0, nullptr, &got) == 0 && got == 0u);
        g_err.clear();
        CHECK(ptx_debug_light_bits(2, nullptr, 1, gm.data(), &got) == -1 && !g_err.empty());
        CHECK(ptx_debug_light_bits(2, m.data(), 1, nullptr, &got) == -1);
        CHECK(ptx_debug_light_bits(2, m.data(), 1, gm.data(), nullptr) == -1);
        CHECK(ptx_debug_light_bits(-1, m.data(), 1, gm.data(), &got) == -1);
        CHECK(ptx_debug_light_bits(2, m.data(), -1, gm.data(), &got) == -1);
    }
    printf("light_bits_check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
