// pose_mask_plan_check.cpp -- the case plan_batch (roft_amd/csrc/batch_plan.h) gained with masks from poses, against what
// include/roft_engine.h (section 3e) and DESIGN.md promise for it.  Built with g++ against batch_plan.h alone
// (tests/test_pose_mask_plan_cpu.py).
//   (1) a batch without silhouettes (pose_masks == 0) has no silhouette launch, and its plan is the plan of the same inputs before
//       the case existed -- checked as: pose_masks changes NOTHING of a plan but pose_silhouettes and, in one situation, ev_prep;
//   (2) the silhouette launch is ONE launch, decided by pose_masks > 0 alone: not by how many pairs, objects or frames there are;
//   (3) it is the preparation's last launch, behind the label ingest where there is one: where the preparation runs ahead on the
//       upload stream and nothing else is ingested, ev_prep ends with that launch (stop) instead of being recorded behind a
//       preparation without an ingest kernel;
//   (4) it never rides in the fused control-block launch: try_fused does not depend on it; and the label launch does not depend
//       on it either.
// Prints the number of plan pairs compared.
#include "batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <cstring>

using namespace roft::host;

#define RULE(cond)                                                                                \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "rule broken (line %d): %s\n", __LINE__, #cond);               \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

static bool same_lane(const LanePlan& a, const LanePlan& b)
{
    return a.early == b.early && a.wait_relabel == b.wait_relabel && a.release == b.release && a.wait_feat == b.wait_feat &&
           a.wait_prev_vel == b.wait_prev_vel && a.gate_second == b.gate_second && a.ev_done == b.ev_done;
}

// everything of a plan but pose_silhouettes and ev_prep
static bool same_but_silhouettes(const BatchPlan& a, const BatchPlan& b)
{
    return a.steady == b.steady && a.handoff == b.handoff && a.early_lanes == b.early_lanes && a.prep == b.prep &&
           a.prep_waits_mask == b.prep_waits_mask && a.prep_waits_feat == b.prep_waits_feat && a.wait_up == b.wait_up &&
           a.try_fused == b.try_fused && a.label_ingest == b.label_ingest && a.ev_ctrl == b.ev_ctrl && a.part_gate == b.part_gate && a.ev_mask == b.ev_mask && a.feat == b.feat &&
           a.ev_feat == b.ev_feat && a.vel_waits == b.vel_waits && a.feat_waits_mask == b.feat_waits_mask && a.ev_skf == b.ev_skf &&
           a.ev_vel == b.ev_vel && same_lane(a.lane[0], b.lane[0]) && same_lane(a.lane[1], b.lane[1]) && a.outlier_div == b.outlier_div && a.quality == b.quality &&
           a.quality_waits_mask == b.quality_waits_mask && a.quality_waits_lane == b.quality_waits_lane && a.ev_quality == b.ev_quality;
}

int main()
{
    long pairs = 0, seen_stop_by_silhouettes = 0, seen_prep = 0, seen_fused = 0;
    for (int prep_mode = 0; prep_mode <= 3; ++prep_mode)
    for (int ctrl_ingest = 0; ctrl_ingest <= 1; ++ctrl_ingest)
    for (int multi = 0; multi <= 1; ++multi)
    for (int timing = 0; timing <= 2; ++timing)            // off, level 1, level 2
    for (int T : {1, 2, 6, 8})
    for (int n_obj : {1, 3, 32, 33, 64, 1024})
    for (int batch_counter : {0, 1, 2, 5, 6, 40})
    for (unsigned masks : {0u, 1u, 0x21u, 0xFFu})
    for (int uploads = 0; uploads <= 1; ++uploads)
    for (int up_distinct = 0; up_distinct <= 1; ++up_distinct)
    for (int feat = 0; feat <= 1; ++feat)
    for (int labels = 0; labels <= 1; ++labels)
    for (int alone = 0; alone <= 1; ++alone) {
        PlanInputs in;
        in.knobs.prep_mode = prep_mode;
        in.knobs.ctrl_ingest = ctrl_ingest;
        in.multi = multi != 0;
        in.timing = timing != 0;
        in.timing_level = timing == 1 ? 1 : 2;
        in.T = T; in.n_obj = n_obj; in.cus = 256;
        in.batch_counter = batch_counter; in.lead = T > 1 ? 5 : 6;
        in.plain_mask_frames = masks & ((1u << T) - 1u);
        in.had_uploads = uploads != 0;
        in.up_stream_distinct = up_distinct != 0;
        in.any_feat = feat != 0;
        in.label_sets = labels ? 2 : 0;
        in.quality_frames = feat ? T : 0;
        in.conflict_free = true;
        in.lin_any[0] = in.lin_any[1] = true;
        in.lane_objs[0] = in.lane_objs[1] = n_obj;
        in.n_segments[1] = 2;
        in.lane_old_first[1] = n_obj;
        auto plan = [&](int pairs) { PlanInputs i2 = in; i2.pose_masks = pairs; return plan_batch(i2, [&] { return alone != 0; }); };
        const BatchPlan none = plan(0), one = plan(1), many = plan(T * n_obj);
        const bool full = in.timing && in.timing_level > 1;
        // (1)
        RULE(!none.pose_silhouettes);
        RULE(same_but_silhouettes(none, one) && same_but_silhouettes(none, many));
        // (2)
        RULE(one.pose_silhouettes && many.pose_silhouettes);
        RULE(one.ev_prep == many.ev_prep);
        // (3)
        RULE((none.ev_prep == Signal::none) == !none.prep && (one.ev_prep == Signal::none) == !one.prep);
        if (one.prep) {
            ++seen_prep;
            RULE(one.ev_prep == (full ? Signal::record : Signal::stop));
            if (in.plain_mask_frames == 0 && !labels && !full) { RULE(none.ev_prep == Signal::record); ++seen_stop_by_silhouettes; }
            else RULE(none.ev_prep == one.ev_prep);
        }
        // (4)
        RULE(one.try_fused == (ctrl_ingest != 0 && !one.prep && in.plain_mask_frames != 0 && !in.timing));
        RULE(one.label_ingest == (labels != 0) && none.label_ingest == (labels != 0));
        seen_fused += one.try_fused;
        pairs += 2;
    }
    RULE(seen_prep > 0 && seen_stop_by_silhouettes > 0 && seen_fused > 0);
    std::printf("%ld\n", pairs);
    return 0;
}
