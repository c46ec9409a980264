// The gate-frame rule of the pose-mask depth gate (roft_amd/csrc/pose_mask_gate.h), against a restatement of the reference's mask
// source: ImageSegmentationOFAidedSource keeps the flows that arrived since the last consumed mask in a buffer, and a new mask is
// chased by ro_mask_propagate (oracle/ro_mask.c:44-48) through flows[start .. n_flows), start = max(n_flows - frames_between, 0) when
// frames_between > 0, else 0.  The gate frame is the frame just before the one that delivered flows[start]; with nothing to chase,
// the delivering frame itself.
//
// The model below keeps the buffer as a list of FRAME NUMBERS, as the source would, and the engine's side as Sched does: a history
// of the last hist_cap valid flows, newest first, each with the frame before it, and a count of the buffered flows.  Swept over
// every history length up to 30, frames_between in {-1, 0, 1, 6, 30}, first mask or not, mask periods, and flow streams with gaps.
// Built against the header alone (no HIP); prints the number of checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pose_mask_gate.h"

using namespace roft::host;

static long checks = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// ro_mask_propagate's start
static int ref_start(int n_flows, int frames_between)
{
    int start = 0;
    if (frames_between > 0) {
        start = n_flows - frames_between;
        if (start < 0) start = 0;
    }
    return start;
}

struct Entry { int frame, before; };   // a valid flow: the frame that delivered it, the object's frame before that one

int main()
{
    const int fbs[] = {-1, 0, 1, 6, 30};
    // 1. the rule as a function, against start: entry k of a newest-first history of n_hist flows is flows[n_flows - 1 - k]
    for (int fb : fbs)
        for (int n_hist = 0; n_hist <= 30; ++n_hist)
            for (int buffered = 0; buffered <= 31; ++buffered)
                for (int first = 0; first < 2; ++first) {
                    const int k = pose_mask_gate_entry(n_hist, fb, buffered, first != 0);
                    if (first) { EXPECT(k == -1); continue; }
                    const int n_flows = buffered < n_hist ? buffered : n_hist;   // what the history can supply
                    const int used = n_flows - ref_start(n_flows, fb);
                    EXPECT(pose_mask_chase_flows(n_hist, fb, buffered, false) == used);
                    EXPECT(k == used - 1);
                    EXPECT(k >= -1 && k < n_hist);
                }
    // 2. a run: frames 0 .. 59, a mask every `period` frames from frame 0, flows with gaps (gap pattern g: frame f has no flow when
    // f % g == g - 1, g == 0: none missing); the engine's history holds hist_cap = frames_between flows (30 when that is unknown)
    for (int fb : fbs)
        for (int period = 1; period <= 12; ++period)
            for (int g = 0; g <= 7; ++g) {
                const int hist_cap = fb > 0 ? fb : 30;
                std::vector<int> buffer;            // the source's flow buffer: delivering frames, oldest first
                std::vector<Entry> hist;            // the engine's history, newest first
                int buffered = 0, prev_frame = -1;  // Sched::flows_buffered; the object's frame before (Sched::depth_prev)
                bool first = true;
                for (int f = 0; f < 60; ++f) {
                    const bool flow = f > 0 && !(g > 0 && f % g == g - 1);
                    if (flow) {
                        buffer.push_back(f);
                        hist.insert(hist.begin(), Entry{f, prev_frame});
                        if ((int)hist.size() > hist_cap) hist.pop_back();
                        buffered = buffered + 1 > 30 ? 30 : buffered + 1;
                    }
                    if (f % period == 0) {
                        const int k = pose_mask_gate_entry((int)hist.size(), fb, buffered, first);
                        const int got = k < 0 ? f : hist[(size_t)k].before;
                        int want = f;
                        if (!first) {
                            int n_flows = (int)buffer.size();
                            if (n_flows > 30) n_flows = 30;   // (ROFT_MAX_FLOW_CHASE: the engine refuses more)
                            const int start = ref_start(n_flows, fb);
                            if (start < n_flows) want = buffer[buffer.size() - (size_t)n_flows + (size_t)start] - 1;
                            buffer.clear();
                            buffered = 0;
                        }
                        if ((int)buffer.size() <= 30) EXPECT(got == want);
                        // with a complete flow stream the gate frame is k - n
                        if (!first && g == 0) EXPECT(got == f - pose_mask_chase_flows((int)hist.size(), fb, period, false));
                        first = false;
                    }
                    prev_frame = f;
                }
            }
    // 3. the predicate and the tolerances
    EXPECT(pose_mask_gate_keep(0.5f, 0.0f, 0.02f, 0.05f));                    // no reading
    EXPECT(pose_mask_gate_keep(0.5f, 0.5f - 0.02f, 0.02f, 0.0f));             // the comparison is strict
    EXPECT(!pose_mask_gate_keep(0.5f, 0.47f, 0.02f, 0.0f));
    EXPECT(pose_mask_gate_keep(0.5f, 9.0f, 0.02f, 0.0f) && !pose_mask_gate_keep(0.5f, 9.0f, 0.02f, 0.05f));
    EXPECT(pose_mask_gate_keep(0.5f, std::nanf(""), 0.02f, 0.05f));
    EXPECT(pose_mask_gate_valid(0.02f, 0.0f) && pose_mask_gate_valid(0.02f, -1.0f) && pose_mask_gate_valid(1e-6f, 3.0f));
    EXPECT(!pose_mask_gate_valid(0.0f, 0.0f) && !pose_mask_gate_valid(-0.02f, 0.0f) && !pose_mask_gate_valid(std::nanf(""), 0.0f));
    EXPECT(!pose_mask_gate_valid(INFINITY, 0.0f) && !pose_mask_gate_valid(0.02f, std::nanf("")) && !pose_mask_gate_valid(0.02f, INFINITY)
           && !pose_mask_gate_valid(0.02f, -INFINITY));
    std::printf("%ld\n", checks);
    return 0;
}
