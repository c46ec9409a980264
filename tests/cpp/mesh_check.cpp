// mesh_check.cpp -- the host-only part of a mesh's way to the device (roft_amd/csrc/mesh_class.h), without HIP: the array check
// names the offending triangle and vertex, and each of the three upload layouts hands out the triangles and flip bits it promises.
// Built and run by tests/test_meshclass_cpu.py:  g++ -std=c++17 -Wall -Werror -I roft_amd/csrc mesh_check.cpp -x c++ mesh_class.hip
#include "mesh_class.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>

using namespace roft;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: %s (mesh %s)\n", __FILE__, __LINE__, #cond, g_name); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static const char* g_name = "-";

struct Mesh {
    const char* name;
    std::vector<float> v;
    std::vector<int32_t> t;
    bool closed;
    int n_verts() const { return (int)v.size() / 3; }
    int n_tris() const { return (int)t.size() / 3; }
};

static Mesh tetrahedron()
{
    return {"tetrahedron", {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2}, true};
}

static Mesh box12()
{
    Mesh m{"box", {}, {}, true};
    for (int i = 0; i < 8; ++i) {
        m.v.push_back((i & 1) ? 0.08f : -0.08f);
        m.v.push_back((i & 2) ? 0.10f : -0.10f);
        m.v.push_back((i & 4) ? 0.035f : -0.035f);
    }
    m.t = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
    return m;
}

static Mesh box_random_windings()
{
    Mesh m = box12();
    m.name = "box_random_windings";
    unsigned lcg = 12345u;
    for (int t = 0; t < m.n_tris(); ++t) {
        lcg = lcg * 1664525u + 1013904223u;
        if (lcg >> 31) std::swap(m.t[3 * t + 1], m.t[3 * t + 2]);
    }
    return m;
}

static Mesh open_quad()
{
    return {"open_quad", {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0}, {0, 1, 2, 0, 2, 3}, false};
}

static void check_array_check(const Mesh& m)
{
    const int nv = m.n_verts(), nt = m.n_tris();
    CHECK(!check_mesh_arrays(m.v.data(), nv, m.t.data(), nt));
    CHECK(check_mesh_arrays(nullptr, nv, m.t.data(), nt).kind == MeshFault::kNullArray);
    CHECK(check_mesh_arrays(m.v.data(), nv, nullptr, nt).kind == MeshFault::kNullArray);
    CHECK(check_mesh_arrays(nullptr, nv, nullptr, nt).kind == MeshFault::kNullArray);
    const size_t last = m.t.size() - 1;
    const struct { size_t at; int32_t value; } bad[] = {{0, -1}, {0, nv}, {last, -1}, {last, nv}, {last, 1 << 30}, {4, INT32_MIN}, {last / 2, nv + 7}};
    for (const auto& b : bad) {
        std::vector<int32_t> t = m.t;
        t[b.at] = b.value;
        const MeshFault f = check_mesh_arrays(m.v.data(), nv, t.data(), nt);
        CHECK(f && f.kind == MeshFault::kBadIndex);
        CHECK(f.triangle == (long long)(b.at / 3) && f.vertex == b.value);
    }
    // the FIRST offender is the one reported
    std::vector<int32_t> t = m.t;
    t[last] = nv;
    t[3] = -5;
    const MeshFault f = check_mesh_arrays(m.v.data(), nv, t.data(), nt);
    CHECK(f.kind == MeshFault::kBadIndex && f.triangle == 1 && f.vertex == -5);
}

static void check_layouts(const Mesh& m)
{
    const int nv = m.n_verts(), nt = m.n_tris();
    std::vector<uint8_t> flip;
    CHECK(classify_mesh(m.v.data(), nv, m.t.data(), nt, flip) == m.closed);
    PreparedMesh as_is, callers, walk;
    // (dirty structs: a prepare_mesh call leaves nothing of an earlier one)
    as_is.closed = callers.closed = walk.closed = true;
    for (PreparedMesh* p : {&as_is, &callers, &walk}) { p->reordered.assign(5, 7); p->flip.assign(9, 1); }
    prepare_mesh(m.v.data(), nv, m.t.data(), nt, MeshLayout::kAsItIs, as_is);
    prepare_mesh(m.v.data(), nv, m.t.data(), nt, MeshLayout::kCallersOrder, callers);
    prepare_mesh(m.v.data(), nv, m.t.data(), nt, MeshLayout::kWalkOrder, walk);
    // as it is: never classified
    CHECK(!as_is.closed && as_is.flip.empty() && as_is.tris(m.t.data()) == m.t.data());
    CHECK(callers.closed == m.closed && walk.closed == m.closed);
    if (!m.closed) {
        for (const PreparedMesh* p : {&callers, &walk}) CHECK(p->flip.empty() && p->reordered.empty() && p->tris(m.t.data()) == m.t.data());
        return;
    }
    // the caller's order: the caller's pointer, classify_mesh's flips
    CHECK(callers.tris(m.t.data()) == m.t.data() && callers.flip == flip);
    // walk order: a permutation of the caller's triangles, each with its corners in the caller's order, the flips following it
    std::vector<int32_t> order;
    facing_coherent_order(m.v.data(), m.t.data(), nt, flip, order);
    CHECK((int)order.size() == nt);
    std::vector<int32_t> sorted = order, identity((size_t)nt);
    std::sort(sorted.begin(), sorted.end());
    std::iota(identity.begin(), identity.end(), 0);
    CHECK(sorted == identity);
    const int32_t* wt = walk.tris(m.t.data());
    CHECK(wt == walk.reordered.data() && wt != m.t.data() && (int)walk.reordered.size() == 3 * nt && (int)walk.flip.size() == nt);
    for (int k = 0; k < nt; ++k) {
        for (int q = 0; q < 3; ++q) CHECK(wt[3 * k + q] == m.t[3 * order[k] + q]);
        CHECK(walk.flip[k] == callers.flip[order[k]]);
    }
}

int main()
{
    CHECK(has_mesh(1, 1) && !has_mesh(0, 5) && !has_mesh(5, 0) && !has_mesh(-1, 3) && !has_mesh(0, 0));
    struct Counts { int n_verts, n_tris; };
    CHECK(has_mesh(Counts{3, 1}) && !has_mesh(Counts{3, 0}));
    int flipped = 0;
    for (const Mesh& m : {tetrahedron(), box12(), box_random_windings(), open_quad()}) {
        g_name = m.name;
        check_array_check(m);
        check_layouts(m);
        std::vector<uint8_t> flip;
        classify_mesh(m.v.data(), m.n_verts(), m.t.data(), m.n_tris(), flip);
        flipped += (int)std::count(flip.begin(), flip.end(), 1);
    }
    g_name = "-";
    CHECK(flipped > 0);   // (the random windings gave the flip comparison something to compare)
    std::puts("mesh_check ok");
    return 0;
}
