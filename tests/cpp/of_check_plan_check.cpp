// of_check_plan_check.cpp -- the slots of a checked chunk (roft_amd/csrc/opticalflow_args.h: of_check_put, of_check_close), host only.
// A chunk of n <= kOfCheckChunk pairs must come out as 2 n Lucas-Kanade problems: slot k the forward problem of pair k, slot n + k
// its backward problem with the pyramids swapped, every problem with a workspace and a level-0 field of its own, the check's
// F / B pointers naming the fields of slots k and n + k.  The workspaces are real heap blocks of exactly the size the engine
// allocates (kOfChunk coarse strides, kOfCheckChunk backward fields) and every region a slot names is written end to end, so
// that -fsanitize=address,undefined sees an overrun.  Prints the number of pairs laid out.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "opticalflow_args.h"

using namespace roft;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static long lay_out(int W, int H, int levels, int n_pairs)
{
    OfGeom g;
    of_geometry(g, W, H, levels, 3, 3, 100.0f);
    const size_t field_floats = (size_t)2 * W * H;
    // the engine's workspaces of ONE chunk
    std::vector<float> coarse((size_t)kOfChunk * g.flow_stride), back((size_t)kOfCheckChunk * field_floats);
    std::vector<std::vector<float>> pyr((size_t)n_pairs + 1, std::vector<float>(g.pyr_stride)), out((size_t)n_pairs, std::vector<float>(field_floats));
    OfPairs pr{};
    OfCheck ck{};
    long done = 0;
    int first = 0;   // pair index of the chunk's slot 0
    auto close_and_check = [&]() {
        const int n = pr.n;
        REQUIRE(n >= 1 && n <= kOfCheckChunk && ck.n == n);
        of_check_close(pr);
        REQUIRE(pr.n == 2 * n && pr.n <= kOfChunk);
        std::set<const void*> spaces;
        for (int k = 0; k < n; ++k) {
            const int i = first + k;
            REQUIRE(pr.pyr0[k] == pyr[i].data() && pr.pyr1[k] == pyr[i + 1].data());           // forward: (prev, cur)
            REQUIRE(pr.pyr0[n + k] == pyr[i + 1].data() && pr.pyr1[n + k] == pyr[i].data());   // backward: swapped
            REQUIRE(pr.field[k] == out[i].data() && ck.fwd[k] == pr.field[k] && ck.bwd[k] == pr.field[n + k]);
            REQUIRE(pr.out_s16[k] == nullptr && pr.out_s16[n + k] == nullptr);
            for (int s : {k, n + k}) {
                REQUIRE(spaces.insert(pr.coarse[s]).second && spaces.insert(pr.field[s]).second);
                for (size_t j = 0; j < g.flow_stride; ++j) pr.coarse[s][j] = (float)s;
                for (size_t j = 0; j < field_floats; ++j) pr.field[s][j] = (float)s;
            }
        }
        // nobody wrote into another slot's space
        for (int s = 0; s < 2 * n; ++s) REQUIRE(pr.coarse[s][0] == (float)s && pr.coarse[s][g.flow_stride - 1] == (float)s &&
                                                pr.field[s][0] == (float)s && pr.field[s][field_floats - 1] == (float)s);
        done += n;
        first += n;
        pr = OfPairs{};
        ck = OfCheck{};
    };
    for (int i = 0; i < n_pairs; ++i) {
        const int k = pr.n;
        of_check_put(pr, ck, pyr[i].data(), pyr[i + 1].data(), out[i].data(), coarse.data() + (size_t)k * g.flow_stride,
                     coarse.data() + (size_t)(kOfCheckChunk + k) * g.flow_stride, back.data() + (size_t)k * field_floats);
        if (pr.n == kOfCheckChunk) close_and_check();
    }
    if (pr.n) close_and_check();
    REQUIRE(done == n_pairs);
    return done;
}

int main()
{
    static_assert(2 * kOfCheckChunk == kOfChunk, "a checked chunk fills the launch's slots");
    long total = 0;
    for (int levels = 1; levels <= 4; ++levels)
        for (int n = 1; n <= 2 * kOfChunk + 1; ++n) total += lay_out(32, 16, levels, n);
    total += lay_out(96, 64, 3, 5);
    std::printf("%ld\n", total);
    return 0;
}
