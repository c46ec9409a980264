// raster_shape_check.cpp -- host check of roft_amd/csrc/raster_shape.h: the three launchers' rules against the shapes their
// hand-written predecessors derived, tests/golden/raster_shapes.json (tests/golden/make_raster_shapes.py says how it was recorded and
// what a row holds).  Every field of every row must be equal, the refusals included.  Prints the number of rows compared.
//   g++ -std=c++17 -Wall -Werror -I roft_amd/csrc tests/cpp/raster_shape_check.cpp -o check && ./check tests/golden/raster_shapes.json
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "raster_shape.h"

using namespace roft;

// the fixture holds nothing but section names and integers: the numbers of a section, in file order
static std::map<std::string, std::vector<long long>> read_sections(const char* path)
{
    std::map<std::string, std::vector<long long>> out;
    FILE* f = fopen(path, "r");
    if (!f) return out;
    std::string section;
    for (int c = fgetc(f); c != EOF; c = fgetc(f)) {
        if (c == '"') {
            section.clear();
            while ((c = fgetc(f)) != EOF && c != '"') section.push_back((char)c);
        } else if (isdigit(c)) {
            long long v = c - '0';
            while ((c = fgetc(f)) != EOF && isdigit(c)) v = 10 * v + (c - '0');
            out[section].push_back(v);
        }
    }
    fclose(f);
    return out;
}

static int g_bad = 0;

static void expect(const char* what, const long long* in, const std::vector<long long>& got, const long long* want)
{
    for (size_t k = 0; k < got.size(); ++k)
        if (got[k] != want[k]) {
            if (++g_bad <= 20) fprintf(stderr, "%s(%lld, %lld, %lld): field %zu is %lld, the fixture has %lld\n", what, in[0], in[1], in[2], k, got[k], want[k]);
        }
}

int main(int argc, char** argv)
{
    if (argc == 4) {   // raster_shape_check <max_verts> <target pixels> <window_pixels>: the scene launcher's vcache_cap (tests/test_scene_gpu.py)
        printf("%d\n", scene_window_shape(atoi(argv[1]), (size_t)atoll(argv[2]), atoi(argv[3])).vcache_cap);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: raster_shape_check raster_shapes.json\n"); return 2; }
    auto sec = read_sections(argv[1]);
    const std::vector<long long>&q = sec["quality"], &v = sec["vsd"], &s = sec["scene"];
    if (q.empty() || q.size() % 7 || v.empty() || v.size() % 8 || s.empty() || s.size() % 6) { fprintf(stderr, "unreadable fixture\n"); return 2; }
    size_t rows = 0;
    for (size_t i = 0; i < q.size(); i += 7, ++rows) {
        const RasterShape sh = quality_window_shape((int)q[i], (int)q[i + 1], (int)q[i + 2]);
        expect("quality_window_shape", &q[i], {sh.ok, sh.vcache_cap, sh.win_cap, (long long)sh.lds}, &q[i + 3]);
    }
    for (size_t i = 0; i < v.size(); i += 8, ++rows) {
        const RasterShape sh = vsd_shape((int)v[i], (int)v[i + 1], (int)v[i + 2]);
        expect("vsd_shape", &v[i], {sh.ok, sh.vcache_cap, sh.win_alloc, sh.win_cap, (long long)sh.lds}, &v[i + 3]);
    }
    for (size_t i = 0; i < s.size(); i += 6, ++rows) {
        const RasterShape sh = scene_window_shape((int)s[i], (size_t)s[i + 1], (int)s[i + 2]);
        if (!sh.ok) { ++g_bad; fprintf(stderr, "scene_window_shape refused a target\n"); }
        expect("scene_window_shape", &s[i], {sh.vcache_cap, sh.win_cap, (long long)sh.lds}, &s[i + 3]);
    }
    if (g_bad) { fprintf(stderr, "%d fields differ\n", g_bad); return 1; }
    printf("%zu\n", rows);
    return 0;
}
