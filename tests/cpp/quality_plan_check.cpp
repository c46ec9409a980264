// quality_plan_check.cpp -- plan_batch (roft_amd/csrc/batch_plan.h) and track quality: with PlanInputs::quality_frames set the plan
// gains exactly the quality launch, its waits and its event; every other decision is the one of the same batch without it; and
// quality_frames == 0 is the plan of an engine that never heard of the feature.  Prints the number of plans compared.
#include <cstdio>
#include <initializer_list>

#include "batch_plan.h"

using namespace roft::host;

static bool same_lane(const LanePlan& a, const LanePlan& b)
{
    return a.early == b.early && a.wait_relabel == b.wait_relabel && a.release == b.release && a.wait_feat == b.wait_feat &&
           a.wait_prev_vel == b.wait_prev_vel && a.gate_second == b.gate_second && a.ev_done == b.ev_done;
}

// every field of BatchPlan but the four of track quality
static bool same_but_quality(const BatchPlan& a, const BatchPlan& b)
{
    return a.steady == b.steady && a.handoff == b.handoff && a.early_lanes == b.early_lanes && a.prep == b.prep &&
           a.prep_waits_mask == b.prep_waits_mask && a.prep_waits_feat == b.prep_waits_feat && a.wait_up == b.wait_up &&
           a.try_fused == b.try_fused && a.label_ingest == b.label_ingest && a.ev_ctrl == b.ev_ctrl && a.ev_prep == b.ev_prep &&
           a.part_gate == b.part_gate && a.ev_mask == b.ev_mask && a.feat == b.feat && a.ev_feat == b.ev_feat && a.vel_waits == b.vel_waits &&
           a.feat_waits_mask == b.feat_waits_mask && a.ev_skf == b.ev_skf && a.ev_vel == b.ev_vel && same_lane(a.lane[0], b.lane[0]) &&
           same_lane(a.lane[1], b.lane[1]) && a.outlier_div == b.outlier_div;
}

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main()
{
    // (a field added to LanePlan must be added to same_lane)
    static_assert(sizeof(LanePlan) == 16, "LanePlan changed: update same_lane");
    long n = 0;
    auto alone = [] { return true; };
    for (int one_stream = 0; one_stream < 2; ++one_stream)
    for (int timing = 0; timing < 3; ++timing)
    for (int T : {1, 3, 6, 8})
    for (int n_obj : {1, 8, 32, 64})
    for (int batch : {0, 1, 2, 5, 9})   // bursts and steady batches (lead 5 / 6)
    for (int lanes = 0; lanes < 4; ++lanes)
    for (int uploads = 0; uploads < 2; ++uploads)
    for (int feat = 0; feat < 2; ++feat)
    for (int segs : {1, 2}) {
        PlanInputs in;
        in.knobs.one_stream = one_stream != 0;
        in.multi = !one_stream;
        in.timing = timing > 0;
        in.timing_level = timing;
        in.T = T;
        in.n_obj = n_obj;
        in.lead = T == 1 ? 6 : 5;
        in.batch_counter = batch;
        in.completed_batches = batch > 2 ? batch - 2 : 0;
        in.had_uploads = uploads != 0;
        in.plain_mask_frames = uploads ? 1u : 0u;
        in.any_feat = feat != 0;
        in.conflict_free = true;
        in.lin_any[0] = (lanes & 1) != 0;
        in.lin_any[1] = (lanes & 2) != 0;
        in.n_segments[0] = in.n_segments[1] = segs;
        in.lane_objs[0] = in.lane_objs[1] = n_obj;
        in.feat_used_two_back = feat != 0;
        in.vel_used_prev = batch > 0;
        const BatchPlan untouched = plan_batch(in, alone);   // quality_frames at its default
        PlanInputs off = in;
        off.quality_frames = 0;
        const BatchPlan p0 = plan_batch(off, alone);
        REQUIRE(same_but_quality(p0, untouched));
        for (const BatchPlan* p : {&p0, &untouched}) {
            REQUIRE(!p->quality && !p->quality_waits_mask && !p->quality_waits_lane && p->ev_quality == Signal::none);
        }
        for (int qf : {1, T}) {
            PlanInputs on = in;
            on.quality_frames = qf;
            const BatchPlan p1 = plan_batch(on, alone);
            REQUIRE(same_but_quality(p1, p0));   // nothing else moves
            REQUIRE(p1.quality);
            // its event: a stop event, or recorded behind the launch under full timing -- as every span's
            REQUIRE(p1.ev_quality == ((timing > 1) ? Signal::record : Signal::stop));
            // its waits: only between streams; the other lane only where that lane signals
            REQUIRE(p1.quality_waits_mask == in.multi);
            REQUIRE(p1.quality_waits_lane == (in.multi && in.lin_any[0]));
            if (p1.quality_waits_mask) REQUIRE(p1.ev_mask != Signal::none);
            if (p1.quality_waits_lane) REQUIRE(p1.lane[0].ev_done != Signal::none);
            ++n;
        }
        ++n;
    }
    std::printf("%ld\n", n);
    return 0;
}
