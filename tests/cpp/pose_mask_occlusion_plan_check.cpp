// pose_mask_occlusion_plan_check.cpp -- the fact plan_batch (roft_amd/csrc/batch_plan.h) gained with silhouettes that hide each
// other ("silhouettes to resolve", SubmitFacts::pose_resolve), against what include/roft_engine.h (section 3e) and DESIGN.md
// promise for it.  Built with g++ against batch_plan.h alone (tests/test_pose_mask_occlusion_cpu.py).
//   (1) a batch without pairs to resolve has no resolve launch, and its plan is field for field the plan of the same inputs without
//       the fact: off is off, and so is the mode with nothing to resolve;
//   (2) pairs to resolve without silhouettes do not exist: the fact alone plans nothing;
//   (3) with pairs to resolve the silhouette stage is two launches whatever their number, and NOTHING else of the plan changes,
//       ev_prep included: the stage sits where the silhouette launch sat;
//   (4) the preparation's last launch is the last that exists of mask ingest, label ingest, silhouettes, resolve; where the plan ends
//       the preparation with a launch's stop event (Signal::stop), that launch is the resolve.
// Prints the number of plans compared.
#include "batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

// everything of a plan but pose_resolve
static bool same_but_resolve(const BatchPlan& a, const BatchPlan& b)
{
    return a.steady == b.steady && a.handoff == b.handoff && a.early_lanes == b.early_lanes && a.prep == b.prep &&
           a.prep_waits_mask == b.prep_waits_mask && a.prep_waits_feat == b.prep_waits_feat && a.wait_up == b.wait_up &&
           a.try_fused == b.try_fused && a.label_ingest == b.label_ingest && a.pose_silhouettes == b.pose_silhouettes && a.ev_ctrl == b.ev_ctrl &&
           a.ev_prep == b.ev_prep && a.part_gate == b.part_gate && a.ev_mask == b.ev_mask && a.feat == b.feat && a.ev_feat == b.ev_feat &&
           a.vel_waits == b.vel_waits && a.feat_waits_mask == b.feat_waits_mask && a.ev_skf == b.ev_skf && a.ev_vel == b.ev_vel &&
           same_lane(a.lane[0], b.lane[0]) && same_lane(a.lane[1], b.lane[1]) && a.outlier_div == b.outlier_div && a.quality == b.quality &&
           a.quality_waits_mask == b.quality_waits_mask && a.quality_waits_lane == b.quality_waits_lane && a.ev_quality == b.ev_quality;
}

int main()
{
    long plans = 0, seen_stop = 0, seen_record = 0, seen_no_prep = 0;
    for (int prep_mode = 0; prep_mode <= 3; ++prep_mode)
    for (int ctrl_ingest = 0; ctrl_ingest <= 1; ++ctrl_ingest)
    for (int multi = 0; multi <= 1; ++multi)
    for (int timing = 0; timing <= 2; ++timing)            // off, level 1, level 2
    for (int T : {1, 2, 6, 8})
    for (int n_obj : {2, 3, 33, 64, 1024})
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
        auto plan = [&](int silhouettes, int resolve) {
            PlanInputs i2 = in;
            i2.pose_masks = silhouettes;
            i2.pose_resolve = resolve;
            return plan_batch(i2, [&] { return alone != 0; });
        };
        const bool full = in.timing && in.timing_level > 1;
        const unsigned plain = in.plain_mask_frames;
        for (int silhouettes : {0, 1, T * n_obj}) {
            const BatchPlan off = plan(silhouettes, 0);
            // (1)
            RULE(!off.pose_resolve);
            RULE(pose_silhouette_launches(off) == (silhouettes > 0 ? 1 : 0));
            RULE(prep_last_launch(off, plain) != PrepLaunch::pose_resolve);
            RULE(prep_last_launch(off, plain) == (silhouettes > 0 ? PrepLaunch::pose_silhouettes
                                                  : labels      ? PrepLaunch::label_ingest
                                                  : plain       ? PrepLaunch::mask_ingest : PrepLaunch::none));
            for (int resolve : {2, T * n_obj}) {
                if (resolve > silhouettes && silhouettes > 0) continue;   // (the pairs to resolve are silhouettes)
                const BatchPlan on = plan(silhouettes, resolve);
                RULE(same_but_resolve(off, on));
                if (silhouettes == 0) {
                    // (2)
                    RULE(!on.pose_resolve && pose_silhouette_launches(on) == 0);
                    continue;
                }
                // (3)
                RULE(on.pose_resolve && on.pose_silhouettes && pose_silhouette_launches(on) == 2);
                // (4)
                RULE(prep_last_launch(on, plain) == PrepLaunch::pose_resolve);
                RULE((on.ev_prep == Signal::none) == !on.prep);
                if (on.prep) {
                    RULE(on.ev_prep == (full ? Signal::record : Signal::stop));
                    (on.ev_prep == Signal::stop ? seen_stop : seen_record)++;
                } else {
                    ++seen_no_prep;
                }
                ++plans;
            }
            ++plans;
        }
    }
    RULE(seen_stop > 0 && seen_record > 0 && seen_no_prep > 0);
    std::printf("%ld\n", plans);
    return 0;
}
