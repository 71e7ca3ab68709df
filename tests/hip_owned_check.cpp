// hip_owned_check.cpp -- the owner of events and streams (Owned, mygpuraytracer_amd/csrc/pt_handle.h) with a destroyer that only counts:
// no HIP call is made, so this runs without a GPU, under the host sanitizers (tests/test_hip_owned.py builds and runs it).
#include <cstdio>
#include <utility>
#include <vector>

#include "pt_handle.h"

static int g_destroyed[64];             // per handle value: how often the destroyer saw it
static std::vector<int> g_order;        // the handle values in the order they were destroyed
static void counting_destroy(int h) { g_destroyed[h]++; g_order.push_back(h); }
typedef Owned<int, counting_destroy> Fake;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static int total() { int s = 0; for (int c : g_destroyed) s += c; return s; }
static void clear() { for (int &c : g_destroyed) c = 0; g_order.clear(); }

struct Three { Fake first, second, third; };      // (members go in the reverse of their declaration)

int main() {
    {   // an empty owner destroys nothing -- nor does one that was reset, or reset twice
        { Fake a; CHECK(a == 0 && !a.own); }
        { Fake a; a.reset(); a.reset(); }
        CHECK(total() == 0);
    }
    clear();
    {   // a made one is destroyed exactly once: by its destructor, or by an earlier reset and then no more
        { Fake a; a.adopt(5); CHECK(a == 5 && a.own && total() == 0); }
        CHECK(g_destroyed[5] == 1 && total() == 1);
        { Fake a; a.adopt(6); a.reset(); CHECK(g_destroyed[6] == 1 && a == 0 && !a.own); }
        CHECK(g_destroyed[6] == 1 && total() == 2);
        { Fake a; a.adopt(7); a.adopt(8); CHECK(g_destroyed[7] == 1 && g_destroyed[8] == 0); }      // making it again lets go of the first
        CHECK(g_destroyed[7] == 1 && g_destroyed[8] == 1 && total() == 4);
    }
    clear();
    {   // a borrowed handle is never destroyed; borrowing over a made one destroys the made one alone
        { Fake a; a.borrow(9); CHECK(a == 9 && !a.own); a.reset(); CHECK(a == 0); }
        { Fake a; a.borrow(10); }
        { Fake a; a.adopt(11); a.borrow(12); CHECK(a == 12 && !a.own); }
        CHECK(g_destroyed[9] == 0 && g_destroyed[10] == 0 && g_destroyed[12] == 0 && g_destroyed[11] == 1 && total() == 1);
    }
    clear();
    {   // an array of owners, some left empty and one borrowed: each made element once
        {
            Fake lanes[6];
            for (int l = 1; l < 5; l++) lanes[l].adopt(20 + l);
            lanes[5].borrow(30);
        }
        for (int l = 1; l < 5; l++) CHECK(g_destroyed[20 + l] == 1);
        CHECK(total() == 4);
    }
    clear();
    {   // a std::vector that grows moves its elements: each is destroyed once, when the vector goes, and a moved-from owner is empty
        {
            std::vector<Fake> v;
            for (int k = 0; k < 17; k++) {            // (past several reallocations)
                Fake e;
                e.adopt(40 + k);
                v.push_back(std::move(e));
                CHECK(e == 0 && !e.own);
            }
            CHECK(total() == 0 && v.size() == 17 && v[16] == 56 && v[0] == 40 && v[0].own);
        }
        for (int k = 0; k < 17; k++) CHECK(g_destroyed[40 + k] == 1);
        CHECK(total() == 17);
    }
    clear();
    {   // inside a struct: the reverse of the declaration
        { Three t; t.first.adopt(1); t.second.adopt(2); t.third.adopt(3); }
        CHECK(g_order == std::vector<int>({3, 2, 1}));
        clear();
        { Three t; t.first.adopt(1); t.second.borrow(2); t.third.adopt(3); }
        CHECK(g_order == std::vector<int>({3, 1}));
    }
    printf("hip_owned_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
