// batch_plan_check.cpp -- plan_batch (roft_amd/csrc/batch_plan.h) against the rules the engine PROMISES for a batch's launch
// graph: the progress conditions on top of plan_batch, the description of roft_batch_trace in include/roft_engine.h, the switch
// paragraph of README.md.  Built with g++ against batch_plan.h alone (tests/test_batch_plan_cpu.py); no GPU, no HIP.
//
//   batch_plan_check sweep                          every rule over a sweep of PlanInputs; prints the number of plans checked
//   batch_plan_check trace N CUS LEAD T0 T1 ...     default knobs, N objects, batches of T0, T1, ... frames after a sync:
//                                                   one line "steady handoff outlier_parts_halved" per batch
#include "batch_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace roft::host;

static std::string describe(const PlanInputs& in, bool alone)
{
    char buf[1024];
    const SchedKnobs& k = in.knobs;
    std::snprintf(buf, sizeof(buf),
                  "knobs handoff %d prep %d part %d feat_mask %d lanes_wait_skf %d early %d ctrl_ingest %d div %d | multi %d timing %d/%d wait_value %d "
                  "skf_started %d | T %d n_obj %d cus %d | batch %d idle %d lead %d completed %d | uploads %d new_masks %u feat %d now %d dep %d "
                  "segs %d %d any %d %d objs %d %d old_first %d %d relabel %d %d bands %d | conflict_free %d up_distinct %d alone %d | "
                  "feat_used-2 %d vel_used-1 %d done_used %d %d",
                  k.handoff_mode, k.prep_mode, k.part_mode, k.feat_mask_mode, k.lanes_wait_skf, k.early_lanes, k.ctrl_ingest, k.outlier_steady_div,
                  in.multi, in.timing, in.timing_level, in.wait_value_ok, in.have_skf_started, in.T, in.n_obj, in.cus, in.batch_counter, in.idle_mark,
                  in.lead, in.completed_batches, in.had_uploads, in.plain_mask_frames, in.any_feat, in.any_feat_now, in.feat_dep_in_batch,
                  in.n_segments[0], in.n_segments[1], in.lin_any[0], in.lin_any[1], in.lane_objs[0], in.lane_objs[1], in.lane_old_first[0],
                  in.lane_old_first[1], in.relabel_wait[0], in.relabel_wait[1], in.outlier_bands_per_alternative, in.conflict_free,
                  in.up_stream_distinct, alone, in.feat_used_two_back, in.vel_used_prev, in.done_used_relabel[0], in.done_used_relabel[1]);
    return buf;
}

static const PlanInputs* g_in = nullptr;
static bool g_alone = false;
#define RULE(cond)                                                                                                   \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            std::fprintf(stderr, "rule broken (line %d): %s\n  %s\n", __LINE__, #cond, describe(*g_in, g_alone).c_str()); \
            std::exit(1);                                                                                            \
        }                                                                                                            \
    } while (0)
static bool implies(bool a, bool b) { return !a || b; }

// outcomes the sweep must have produced at least once (a sweep that never releases a lane early proves nothing about early lanes)
static long g_seen[16] = {};
enum { kSeenHandoff, kSeenEarlyBoth, kSeenEarlyOne, kSeenGate, kSeenGateSecond, kSeenEvSkf, kSeenEvVel, kSeenPrep, kSeenPrepFeat, kSeenPart,
       kSeenFused, kSeenFeatMask, kSeenFeatSkf, kSeenWaitFeat, kSeenPrevVel, kSeenRelabel };

static void check_rules(const PlanInputs& in, bool alone)
{
    g_in = &in;
    g_alone = alone;
    bool asked = false;
    const BatchPlan p = plan_batch(in, [&] { asked = true; return alone; });
    const SchedKnobs& k = in.knobs;
    const bool full = in.timing && in.timing_level > 1;
    const bool batch = in.multi && in.T > 1;
    const bool steady = in.batch_counter - in.idle_mark >= in.lead;
    const bool own_sets = in.feat_dep_in_batch || in.any_feat_now;
    const bool spare8 = 8 * in.n_obj <= in.cus, spare16 = 16 * in.n_obj <= in.cus;
    const bool any_early = p.lane[0].early || p.lane[1].early;

    // `steady` is a function of the batch index
    RULE(p.steady == steady);

    // one stream: no cross-stream wait, no hand-over, no preparation ahead, no early lane; only ev_done of the lanes with work
    if (!in.multi) {
        RULE(!p.handoff && !p.prep && !p.part_gate && !any_early && !p.early_lanes);
        RULE(!p.wait_up && !p.prep_waits_mask && !p.prep_waits_feat && p.vel_waits == VelWait::none && !p.feat_waits_mask);
        RULE(p.ev_ctrl == Signal::none && p.ev_prep == Signal::none && p.ev_mask == Signal::none && p.ev_feat == Signal::none &&
             p.ev_skf == Signal::none && p.ev_vel == Signal::none);
        for (const LanePlan& lp : p.lane)
            RULE(!lp.wait_relabel && lp.release == Release::none && !lp.wait_feat && !lp.wait_prev_vel && !lp.gate_second);
    }
    for (int l = 0; l < kPlanLanes; ++l) RULE((p.lane[l].ev_done != Signal::none) == in.lin_any[l]);

    // hand-over: the resident-workgroup gate is a stream wait on a value
    const bool handoff_possible = batch && in.wait_value_ok && in.have_skf_started && !own_sets;
    RULE(implies(p.handoff, handoff_possible));
    RULE(implies(k.handoff_mode == 0, !p.handoff));
    RULE(implies(k.handoff_mode == 2, p.handoff == handoff_possible));
    RULE(implies(k.handoff_mode == 1, p.handoff == (handoff_possible && (!steady || spare8))));
    for (const LanePlan& lp : p.lane) RULE(implies(lp.release == Release::gate || lp.gate_second, p.handoff));

    // early lanes: progress condition (c)
    RULE(implies(asked, p.handoff && !steady && k.early_lanes != 0 && in.conflict_free));   // (the lock is taken last)
    RULE(p.early_lanes == (any_early && spare8));
    for (int l = 0; l < kPlanLanes; ++l) {
        const LanePlan& lp = p.lane[l];
        const bool replay_first = in.lane_old_first[l] > 0 && 8 * (in.lane_objs[l] - in.lane_old_first[l]) <= in.cus &&
                                  2 * in.lane_objs[l] <= in.cus && in.n_segments[l] > 1 && in.T > 1;
        const bool may = p.handoff && !steady && k.early_lanes != 0 && in.conflict_free && alone && (spare8 || replay_first);
        RULE(lp.early == may);   // (=>: the progress condition; <=: bursts release every lane they may)
        RULE(implies(lp.release == Release::ctrl_only, lp.early && in.lin_any[l]));
        // what follows the first segment needs this batch's twists: only with CUs to spare may the whole lane spin for them
        RULE(implies(lp.release == Release::ctrl_only && !spare8, lp.gate_second));
        RULE(implies(lp.gate_second, lp.release == Release::ctrl_only));
    }

    // a lane with work on a stream of its own is released somehow; behind ev_skf only when the features are not its business
    const bool lanes_may_skip_feat = p.feat == FeatRun::behind_skf && !own_sets;
    for (int l = 0; l < kPlanLanes; ++l) {
        const LanePlan& lp = p.lane[l];
        RULE((lp.release != Release::none) == (in.multi && in.lin_any[l]));
        RULE(implies(lp.release == Release::ev_skf, lanes_may_skip_feat && k.lanes_wait_skf != 0));
        RULE(implies(lp.release == Release::ev_vel && lanes_may_skip_feat, k.lanes_wait_skf == 0));
        // a test that reads a set this batch's mask-stream feature kernel buffers waits for that kernel (one-frame batches: only
        // when the set is this very frame's -- older ones are behind ev_vel)
        if ((lp.release == Release::ev_vel || lp.release == Release::ev_skf) && p.feat == FeatRun::mask_stream && in.n_segments[l] > 1 &&
            (in.T > 1 || in.any_feat_now))
            RULE(lp.wait_feat);
        RULE(implies(lp.wait_feat, p.feat == FeatRun::mask_stream));
    }

    // preparation ahead
    const bool prep_possible = batch && in.up_stream_distinct;
    RULE(implies(p.prep, prep_possible));
    RULE(implies(k.prep_mode == 0, !p.prep));
    RULE(implies(k.prep_mode == 2, p.prep == prep_possible));
    RULE(implies(k.prep_mode == 3, p.prep == (prep_possible && steady)));
    RULE(implies(k.prep_mode == 1, p.prep == (prep_possible && steady && !spare8)));
    RULE(p.prep_waits_mask == (p.prep && in.batch_counter >= 2));
    RULE(p.prep_waits_feat == (p.prep_waits_mask && in.feat_used_two_back));
    RULE(implies(p.prep, !p.wait_up && !p.try_fused));
    RULE(implies(in.multi && in.had_uploads && !p.prep, p.wait_up));

    // fused control + ingest launch: never under timing or with the preparation ahead
    RULE(implies(p.try_fused, !in.timing && !p.prep && in.plain_mask_frames != 0 && k.ctrl_ingest != 0));
    RULE(implies(k.ctrl_ingest != 0 && !in.timing && !p.prep && in.plain_mask_frames != 0, p.try_fused));

    // velocity chain released one mask frame early
    RULE(implies(k.part_mode == 0, !p.part_gate));
    RULE(implies(k.part_mode == 2, p.part_gate == batch));
    RULE(implies(k.part_mode == 3, p.part_gate == (batch && !steady)));
    RULE(implies(k.part_mode == 1, p.part_gate == (batch && !steady && spare8)));
    // the flow measurement reads the control blocks and the planes of the frame before
    RULE(implies(in.multi, p.vel_waits == (in.T == 1 ? VelWait::ev_ctrl : p.part_gate ? VelWait::ev_part : VelWait::ev_mask)));
    RULE(implies(p.feat == FeatRun::behind_skf && p.vel_waits == VelWait::ev_part, p.feat_waits_mask));   // (the planes of the last frame)

    // where the feature kernel runs
    RULE((p.feat == FeatRun::none) == !in.any_feat);
    if (in.any_feat) {
        RULE(implies(!batch, p.feat == FeatRun::mask_stream));
        RULE(implies(batch && k.feat_mask_mode == 0, p.feat == FeatRun::behind_skf));
        RULE(implies(k.feat_mask_mode == 2, p.feat == FeatRun::mask_stream));
        RULE(implies(batch && k.feat_mask_mode == 1, (p.feat == FeatRun::mask_stream) == spare16));
    }
    RULE((p.ev_feat != Signal::none) == (in.multi && p.feat == FeatRun::mask_stream));   // (the host and the preparation ahead wait for it)
    RULE((p.ev_vel != Signal::none) == in.multi);

    // outlier bands
    const bool divided = in.outlier_bands_per_alternative == 0 && steady && k.outlier_steady_div > 1;
    RULE(p.outlier_div == (divided ? k.outlier_steady_div : 1));

    // the wait-for graph is acyclic: whatever a stream waits for is signalled by a span enqueued BEFORE it in this batch (chains in
    // the order preparation, mask frames, velocity chain, lanes) or by an earlier batch
    RULE(implies(p.wait_up, in.had_uploads));
    RULE(implies(p.prep, p.ev_prep != Signal::none));   // (the mask stream waits for it)
    RULE(implies(p.prep_waits_mask, in.batch_counter >= 2) && implies(p.prep_waits_feat, in.feat_used_two_back));
    RULE(implies(p.vel_waits == VelWait::ev_ctrl, p.ev_ctrl != Signal::none));
    RULE(implies(p.vel_waits == VelWait::ev_part, p.part_gate));
    RULE(implies(p.vel_waits == VelWait::ev_mask || p.feat_waits_mask, p.ev_mask != Signal::none));
    for (int l = 0; l < kPlanLanes; ++l) {
        const LanePlan& lp = p.lane[l];
        RULE(implies(lp.release == Release::ctrl_only, p.ev_ctrl != Signal::none));
        RULE(implies(lp.release == Release::ev_skf, p.ev_skf != Signal::none));
        RULE(implies(lp.release == Release::ev_vel, p.ev_vel != Signal::none));
        RULE(implies(lp.wait_feat, p.ev_feat != Signal::none));
        RULE(implies(lp.wait_prev_vel, in.batch_counter >= 1 && in.batch_counter - 1 >= in.completed_batches && in.vel_used_prev));
        RULE(implies(lp.wait_prev_vel, lp.release == Release::ctrl_only && in.n_segments[l] > 1));
        RULE(implies(lp.wait_relabel, in.relabel_wait[l] >= in.completed_batches && in.relabel_wait[l] < in.batch_counter && in.done_used_relabel[l]));
        RULE(implies(in.multi && in.relabel_wait[l] >= in.completed_batches && in.relabel_wait[l] < in.batch_counter && in.done_used_relabel[l], lp.wait_relabel));
    }

    // stop event of the span's last kernel, or recorded behind it under full timing (ev_ctrl and ev_part are always stop events; a
    // preparation without a mask to ingest has no kernel to end with ev_prep)
    RULE(p.ev_ctrl != Signal::record);
    RULE(implies(p.prep, (p.ev_prep == Signal::record) == (full || in.plain_mask_frames == 0)));
    for (Signal s : {p.ev_mask, p.ev_feat, p.ev_skf, p.ev_vel, p.lane[0].ev_done, p.lane[1].ev_done})
        RULE(s == Signal::none || (s == Signal::record) == full);

    g_seen[kSeenHandoff] += p.handoff;
    g_seen[kSeenEarlyBoth] += p.early_lanes;
    g_seen[kSeenEarlyOne] += any_early && !p.early_lanes;
    g_seen[kSeenPrep] += p.prep;
    g_seen[kSeenPrepFeat] += p.prep_waits_feat;
    g_seen[kSeenPart] += p.part_gate;
    g_seen[kSeenFused] += p.try_fused;
    g_seen[kSeenFeatMask] += p.feat == FeatRun::mask_stream;
    g_seen[kSeenFeatSkf] += p.feat == FeatRun::behind_skf;
    for (const LanePlan& lp : p.lane) {
        g_seen[kSeenGate] += lp.release == Release::gate;
        g_seen[kSeenGateSecond] += lp.gate_second;
        g_seen[kSeenEvSkf] += lp.release == Release::ev_skf;
        g_seen[kSeenEvVel] += lp.release == Release::ev_vel;
        g_seen[kSeenWaitFeat] += lp.wait_feat;
        g_seen[kSeenPrevVel] += lp.wait_prev_vel;
        g_seen[kSeenRelabel] += lp.wait_relabel;
    }
}

// small deterministic generator: the sweep is the same on every run
static unsigned long long g_rng = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (unsigned)((g_rng >> 20) % n);
}
template <class T, size_t N> static T pick(const T (&v)[N]) { return v[rnd((unsigned)N)]; }

static long sweep()
{
    const int cus = 256, lead = 5;
    // object counts around CUs / 16, CUs / 8, CUs / 2, and both ends
    const int objects[] = {1, 2, 8, 15, 16, 17, 24, 31, 32, 33, 64, 127, 128, 129, 256, 1024};
    const int frames[] = {1, 2, 3, 4, 5, 6, 7, 8};
    const int since_idle[] = {0, 1, 2, lead - 1, lead, lead + 1, 2 * lead, 40};
    long n = 0;
    // every object count x batch length x batch index with the default switches and a plain batch, then the random product
    for (int pass = 0; pass < 2; ++pass)
        for (long i = 0; i < (pass == 0 ? (long)(16 * 8 * 8) : 3000000L); ++i) {
            PlanInputs in;
            in.cus = cus;
            in.lead = lead;
            in.idle_mark = pass == 0 ? 0 : pick({0, 3, 11});
            bool alone = true;
            if (pass == 0) {
                in.n_obj = objects[i % 16];
                in.T = frames[(i / 16) % 8];
                in.batch_counter = since_idle[i / 128];
                in.conflict_free = true;
                in.any_feat = true;
                in.lin_any[0] = in.lin_any[1] = true;
                in.n_segments[1] = 2;
                in.lane_objs[0] = in.lane_objs[1] = in.lane_old_first[1] = in.n_obj;
            } else {
                SchedKnobs& k = in.knobs;
                k.handoff_mode = pick({0, 1, 2});
                k.prep_mode = pick({0, 1, 2, 3});
                k.part_mode = pick({0, 1, 2, 3});
                k.feat_mask_mode = pick({0, 1, 2});
                k.lanes_wait_skf = pick({0, 1});
                k.early_lanes = pick({0, 1, 1});
                k.ctrl_ingest = pick({0, 1});
                k.outlier_steady_div = pick({0, 1, 2, 3});
                k.one_stream = rnd(6) == 0;
                in.multi = !k.one_stream;
                in.timing = rnd(3) == 0;
                in.timing_level = pick({1, 2});
                in.wait_value_ok = rnd(6) != 0;
                in.have_skf_started = rnd(8) != 0;
                in.n_obj = pick(objects);
                in.T = pick(frames);
                in.batch_counter = in.idle_mark + pick(since_idle);
                in.completed_batches = std::max(0, in.batch_counter - (int)rnd(lead + 1));
                in.had_uploads = rnd(2);
                in.plain_mask_frames = pick({0u, 1u, 0x21u}) & ((1u << in.T) - 1);
                in.any_feat = rnd(4) != 0;
                in.any_feat_now = in.any_feat && rnd(6) == 0;
                in.feat_dep_in_batch = in.any_feat && in.T > 1 && rnd(6) == 0;
                in.outlier_bands_per_alternative = pick({0, 0, 4});
                in.conflict_free = rnd(5) != 0;
                alone = rnd(5) != 0;
                in.up_stream_distinct = in.multi && rnd(8) != 0;
                in.feat_used_two_back = rnd(3) == 0;
                in.vel_used_prev = in.multi && rnd(8) != 0;
                for (int l = 0; l < kPlanLanes; ++l) {
                    in.lin_any[l] = rnd(5) != 0;
                    in.n_segments[l] = in.lin_any[l] ? pick({1, 2, 2, 3}) : 1;
                    in.lane_objs[l] = in.lin_any[l] ? 1 + (int)rnd((unsigned)in.n_obj) : 0;
                    const int old_first[] = {0, in.lane_objs[l], std::max(in.lane_objs[l] - 1, 0), std::max(in.lane_objs[l] - cus / 8, 0), in.lane_objs[l] / 2};
                    in.lane_old_first[l] = in.n_segments[l] > 1 ? pick(old_first) : 0;
                    in.relabel_wait[l] = rnd(3) == 0 ? in.batch_counter - 1 - (int)rnd(7) : -1;
                    in.done_used_relabel[l] = in.relabel_wait[l] >= 0 && rnd(4) != 0;
                }
            }
            check_rules(in, alone);
            ++n;
        }
    static const char* names[16] = {"handoff", "both lanes early", "one lane early", "gate", "second segment gated", "behind ev_skf", "behind ev_vel",
                                    "preparation ahead", "preparation waits for ev_feat", "part gate", "fused launch tried", "features on the mask stream",
                                    "features behind the filter", "lane waits for ev_feat", "test waits for the velocity chain before", "relabel wait"};
    for (int i = 0; i < 16; ++i)
        if (g_seen[i] == 0) { std::fprintf(stderr, "the sweep never produced: %s\n", names[i]); std::exit(1); }
    return n;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "sweep")) {
        std::printf("%ld\n", sweep());
        return 0;
    }
    if (argc >= 6 && !std::strcmp(argv[1], "trace")) {
        PlanInputs in;
        in.n_obj = std::atoi(argv[2]);
        in.cus = std::atoi(argv[3]);
        in.lead = std::atoi(argv[4]);
        in.conflict_free = true;
        in.any_feat = true;
        in.lin_any[0] = in.lin_any[1] = true;
        in.lane_objs[0] = in.lane_objs[1] = in.n_obj;
        for (int b = 0; b + 5 < argc; ++b) {
            in.batch_counter = b;
            in.T = std::atoi(argv[5 + b]);
            const BatchPlan p = plan_batch(in, [] { return true; });
            std::printf("%d %d %d\n", (int)p.steady, (int)p.handoff, p.outlier_div > 1 ? 1 : 0);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: batch_plan_check sweep | trace N CUS LEAD T0 T1 ...\n");
    return 2;
}
