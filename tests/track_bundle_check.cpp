// Host check of the bundle binding in csrc/pair_outputs.h and of its scratch in csrc/device_mem.h
// (tests/test_track_bundle_rules_host.py builds it with the address and undefined-behaviour
// sanitizers and runs it; no GPU): the fifth setter's rules, its parameters, the size and the one
// allocation of its scratch, a failure of that allocation, and the TrackArgs a retiring set hands
// to launch_tracks under the four combinations of a refine and a bundle binding.  The HIP calls
// are fake_hip.h's; launch_landmarks and launch_tracks are defined here and record what they are
// given.
#include "fake_hip.h"

#include <cmath>

#include "../droplet_visual_odometry_amd/csrc/pair_outputs.h"

using namespace dvo;

namespace {
std::vector<TrackArgs> g_tr_calls;
int g_lm_calls = 0;
}  // namespace

namespace dvo {
hipError_t launch_landmarks(const GeomArgs&, int, const dvo_pair_record*, const LandmarkScratch&, dvo_landmark*, int32_t*,
                            int, hipStream_t) {
    ++g_lm_calls;
    return hipSuccess;
}
hipError_t launch_tracks(const TrackArgs& a, int, hipStream_t) {
    g_tr_calls.push_back(a);
    return hipSuccess;
}
}  // namespace dvo

namespace {
static_assert(sizeof(BundlePoint) == 32 && kLandmarkTile == 256, "the byte counts below assume these");
constexpr int F = 3;
constexpr size_t HC = 5;
constexpr int kDevice = 2;

dvo_landmark* const LM_OUT = reinterpret_cast<dvo_landmark*>(0x1000);
int32_t* const LM_CNT = reinterpret_cast<int32_t*>(0x2000);
int32_t* const LINK = reinterpret_cast<int32_t*>(0x3000);
dvo_track_scale* const SCALE = reinterpret_cast<dvo_track_scale*>(0x4000);
dvo_track_pose* const POSE = reinterpret_cast<dvo_track_pose*>(0x5000);
dvo_landmark_refined* const REFINED = reinterpret_cast<dvo_landmark_refined*>(0x6000);
dvo_track_id* const ID = reinterpret_cast<dvo_track_id*>(0x7000);
const dvo_pair_record* const REC = reinterpret_cast<const dvo_pair_record*>(0x8000);
const float* const PTS = reinterpret_cast<const float*>(0x9000);
const hipStream_t STREAM = reinterpret_cast<hipStream_t>(0xa000);
dvo_track_bundle* const BUNDLE = reinterpret_cast<dvo_track_bundle*>(0xb000);
dvo_landmark_refined* const POINTS = reinterpret_cast<dvo_landmark_refined*>(0xc000);

const char* const kMsgBd = "track bundle goes with a pending tracks binding that has link and scale buffers";
const char* const kMsgBdArgs = "track bundle: views 2..8, iters <= 16, min_points >= 6, no NaN";

// A stream's shape and the bytes of its bundle scratch, written out: 36 B per slot of every track
// set (32 B of points, 4 B of links) in one allocation.
struct Shape {
    const char* name;
    int cap, track_sets;
    bool own_idx;
    size_t set_slots, all_slots, bytes;
};
const Shape kShapes[] = {
    {"orb 300", 300, 5, true, 900, 4500, 4500 * 36 + 256},
    {"knn 300", 300, 1, false, 900, 900, 900 * 36 + 256},
    {"orb 7", 7, 5, true, 21, 105, 105 * 36 + 256},
    {"knn 7", 7, 1, false, 21, 21, 21 * 36 + 256},
};

void make_sets(PairSets& ps, const Shape& sh) {
    ps.shape(F, sh.cap, HC, sh.track_sets, sh.own_idx);
    CHECK(ps.ensure(sh.track_sets) == hipSuccess);
}

void bind_below(PairOutputs& o, PairSets& ps, bool poses, bool refine) {
    CHECK(o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4).code == DVO_OK);
    CHECK(o.set_tracks(ps, kDevice, LINK, SCALE).code == DVO_OK);
    if (poses) CHECK(o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 0).code == DVO_OK);
    if (refine) CHECK(o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, 0).code == DVO_OK);
}

BindResult bind(PairOutputs& o, PairSets& ps) {
    return o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, 0, 0, 0, 0);
}

bool empty(const TrackBundleBinding& b) {
    return !b && !b.out && !b.points && b.views == 0 && b.iters == 0 && b.min_points == 0 && b.lambda == 0 &&
           b.huber_px == 0 && b.inlier_px == 0 && !b.use_pose;
}

void check_params() {
    TrackBundleBinding b;
    CHECK(track_bundle_params(b, 0, 0, 0, 0, 0, 0));
    CHECK(b.views == 6 && b.iters == 5 && b.lambda == DVO_TRACK_BUNDLE_LAMBDA && b.huber_px == 1.0 && b.inlier_px == 2.0);
    CHECK(b.min_points == 8 && !b && !b.use_pose && DVO_TRACK_BUNDLE_LAMBDA == 1e-6);
    CHECK(track_bundle_params(b, -1, -1, -1.0, -1.0, -1.0, -1) && b.views == 6 && b.iters == 5 && b.min_points == 8);
    CHECK(track_bundle_params(b, 2, 16, 1e-2, 0.5, 3.0, 6));
    CHECK(b.views == 2 && b.iters == 16 && b.lambda == 1e-2 && b.huber_px == 0.5 && b.inlier_px == 3.0 && b.min_points == 6);
    CHECK(track_bundle_params(b, 8, 1, 0, INFINITY, 0, 1000) && b.views == 8 && b.iters == 1 && b.min_points == 1000);
    CHECK(!track_bundle_params(b, 1, 0, 0, 0, 0, 0) && !track_bundle_params(b, 9, 0, 0, 0, 0, 0));
    CHECK(!track_bundle_params(b, 0, 17, 0, 0, 0, 0));
    for (int mp = 1; mp <= 5; ++mp) CHECK(!track_bundle_params(b, 0, 0, 0, 0, 0, mp));
    CHECK(!track_bundle_params(b, 0, 0, NAN, 0, 0, 0) && !track_bundle_params(b, 0, 0, 0, NAN, 0, 0));
    CHECK(!track_bundle_params(b, 0, 0, 0, 0, NAN, 0));
}

void expect(const BindResult& r, int code, const char* msg) {
    CHECK(r.code == code && r.hip == hipSuccess);
    CHECK(msg ? r.what && std::strcmp(r.what, msg) == 0 : r.what == nullptr);
}

void check_rules() {
    PairSets ps;
    make_sets(ps, kShapes[2]);
    PairOutputs o;
    // it needs landmarks and a tracks binding with both buffers; a refine or pose binding is not required
    expect(bind(o, ps), DVO_EINVAL, kMsgBd);
    CHECK(o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4).code == DVO_OK);
    expect(bind(o, ps), DVO_EINVAL, kMsgBd);
    CHECK(o.set_tracks(ps, kDevice, LINK, nullptr).code == DVO_OK);
    expect(bind(o, ps), DVO_EINVAL, kMsgBd);
    CHECK(o.set_tracks(ps, kDevice, nullptr, SCALE).code == DVO_OK);
    expect(bind(o, ps), DVO_EINVAL, kMsgBd);
    CHECK(empty(o.bd) && g_dev.count(ps.tr.table) == 1 && !ps.tr.bx);
    CHECK(o.set_tracks(ps, kDevice, LINK, SCALE).code == DVO_OK);
    reset_log();
    expect(bind(o, ps), DVO_OK, nullptr);
    CHECK(g_devices == std::vector<int>{kDevice});
    CHECK(o.bd.out == BUNDLE && o.bd.points == POINTS && !o.bd.use_pose && o.bd.views == 6 && o.bd.min_points == 8);
    CHECK(!o.tp.out && !o.rf);
    // either output alone is a binding; both null clears, whatever the parameters
    expect(o.set_track_bundle(ps, kDevice, nullptr, POINTS, 4, 3, 1e-3, 0.5, 3.0, 7), DVO_OK, nullptr);
    CHECK(!o.bd.out && o.bd.points == POINTS && o.bd.views == 4 && o.bd.iters == 3 && o.bd.lambda == 1e-3);
    CHECK(o.bd.huber_px == 0.5 && o.bd.inlier_px == 3.0 && o.bd.min_points == 7);
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, nullptr, 0, 0, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(o.bd.out == BUNDLE && !o.bd.points);
    reset_log();
    expect(o.set_track_bundle(ps, kDevice, nullptr, nullptr, 1, 17, NAN, NAN, NAN, 1), DVO_OK, nullptr);
    CHECK(empty(o.bd) && g_devices.empty());
    // a call out of range clears nothing, neither the bundle nor the bindings before it
    bind_below(o, ps, true, true);
    expect(bind(o, ps), DVO_OK, nullptr);
    CHECK(o.bd.use_pose);  // a pose binding was pending
    const int bad[][3] = {{1, 0, 0}, {9, 0, 0}, {0, 17, 0}, {0, 0, 1}, {0, 0, 5}};
    for (const auto& v : bad) {
        reset_log();
        expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, v[0], v[1], 0, 0, 0, v[2]), DVO_EINVAL, kMsgBdArgs);
        CHECK(g_devices.empty());
    }
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, NAN, 0, 0, 0), DVO_EINVAL, kMsgBdArgs);
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, 0, NAN, 0, 0), DVO_EINVAL, kMsgBdArgs);
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, 0, 0, NAN, 0), DVO_EINVAL, kMsgBdArgs);
    CHECK(o.bd.out == BUNDLE && o.bd.points == POINTS && o.bd.views == 6 && o.bd.use_pose);
    CHECK(o.lm.out == LM_OUT && o.tr.link == LINK && o.tr.scale == SCALE && o.tp.out == POSE);
    CHECK(o.rf.refined == REFINED && o.rf.id == ID && o.rf.use_pose);
    // binding it clears nothing else; every earlier setter clears it, a clearing or failing call too
    expect(o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(empty(o.bd) && o.rf && o.tp.out == POSE);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_track_refine(ps, kDevice, REFINED, ID, 2, 0, 0, 0), DVO_EINVAL,
           "track refine: views 3..8, iters <= 16, no NaN");
    CHECK(empty(o.bd) && o.rf);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_track_refine(ps, kDevice, nullptr, nullptr, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(empty(o.bd) && !o.rf && o.tp.out == POSE);
    expect(bind(o, ps), DVO_OK, nullptr);
    CHECK(o.bd.use_pose);
    expect(o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(empty(o.bd) && o.tp.out == POSE);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_track_poses(ps, kDevice, nullptr, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(empty(o.bd) && !o.tp.out);
    expect(bind(o, ps), DVO_OK, nullptr);
    CHECK(!o.bd.use_pose);  // no pose binding pending any more
    expect(o.set_tracks(ps, kDevice, LINK, SCALE), DVO_OK, nullptr);
    CHECK(empty(o.bd) && o.tr.link == LINK);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_landmarks(ps, kDevice, LM_OUT + 1, LM_CNT + 1, 9), DVO_OK, nullptr);  // another landmark buffer: it stays
    CHECK(o.bd.out == BUNDLE);
    expect(o.set_landmarks(ps, kDevice, nullptr, nullptr, 0), DVO_OK, nullptr);
    CHECK(empty(o.bd) && !o.lm.out && !o.tr);
    // take() hands it over with the rest
    bind_below(o, ps, true, false);
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 8, 16, 1e-2, 0.5, 3.0, 6), DVO_OK, nullptr);
    const PairOutputs t = o.take();
    CHECK(empty(o.bd) && !o.lm.out);
    CHECK(t.bd.out == BUNDLE && t.bd.points == POINTS && t.bd.views == 8 && t.bd.iters == 16 && t.bd.lambda == 1e-2);
    CHECK(t.bd.huber_px == 0.5 && t.bd.inlier_px == 3.0 && t.bd.min_points == 6 && t.bd.use_pose && !t.rf);
}

void check_scratch(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    PairOutputs o;
    bind_below(o, ps, true, false);
    CHECK(!ps.tr.bx && !ps.tr.blink && !ps.tr.flink);
    const size_t live = g_dev.size();
    reset_log();
    CHECK(bind(o, ps).code == DVO_OK);
    CHECK(g_mallocs == std::vector<size_t>{sh.bytes} && g_frees == 0 && g_syncs == 0 && g_dev.size() == live + 1);
    CHECK(g_dev.count(ps.tr.bx) == 1 && !ps.tr.flink && !ps.tr.rank);  // no refine scratch comes with it
    CHECK((const char*)ps.tr.blink == (const char*)ps.tr.bx + sh.all_slots * 32);  // the links behind the points
    const BundlePoint* bx = ps.tr.bx;
    // a second binding, and one after a refine binding has brought its scratch, allocate nothing more for it
    reset_log();
    (void)o.take();
    bind_below(o, ps, false, false);
    CHECK(bind(o, ps).code == DVO_OK && g_mallocs.empty());
    bind_below(o, ps, false, true);
    reset_log();
    CHECK(bind(o, ps).code == DVO_OK && g_mallocs.empty() && ps.tr.bx == bx && ps.tr.flink);
    // without the track scratch there is nothing to put it beside
    PairSets fresh;
    make_sets(fresh, sh);
    reset_log();
    const BindResult r = o.set_track_bundle(fresh, kDevice, BUNDLE, POINTS, 0, 0, 0, 0, 0, 0);
    CHECK(r.code == DVO_EHIP && r.hip == hipErrorInvalidValue && g_mallocs.empty() && !fresh.tr.bx);
}

// The one allocation fails: the scratch stays empty, nothing leaks, the earlier bindings are what
// they were and no bundle binding is pending; the same call then succeeds.
void check_failure(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    PairOutputs o;
    bind_below(o, ps, true, true);
    const size_t live = g_dev.size();
    reset_log();
    g_fail_at = 0;
    const BindResult r = bind(o, ps);
    CHECK(r.code == DVO_EHIP && r.hip == hipErrorOutOfMemory && r.what && std::strcmp(r.what, "PairSets::ensure_track_bundle") == 0);
    CHECK(g_mallocs == std::vector<size_t>{sh.bytes} && g_dev.size() == live && !ps.tr.bx && !ps.tr.blink);
    CHECK(empty(o.bd) && o.lm.out == LM_OUT && o.tr.link == LINK && o.tr.scale == SCALE && o.tp.out == POSE);
    CHECK(o.rf.refined == REFINED && o.rf.id == ID && g_devices == std::vector<int>{kDevice});
    reset_log();
    CHECK(bind(o, ps).code == DVO_OK && g_mallocs == std::vector<size_t>{sh.bytes} && g_dev.size() == live + 1);
    CHECK(o.bd.out == BUNDLE && o.bd.use_pose && o.rf.refined == REFINED);
}

// ---- the launches of a retiring set -----------------------------------------------------------
void check_launches(const Shape& sh, bool refine_scratch_first) {
    PairSets ps;
    make_sets(ps, sh);
    GeomArgs g{};
    g.pts_f = PTS;
    g.fx = 700.5, g.fy = 701.5, g.cx = 320.25, g.cy = 240.75;
    g.pts_stride = sh.cap;
    static dvo_dmatch matches[1];
    const TrackIndex caller{&matches->queryIdx, &matches->trainIdx, sh.cap, 4};
    const TrackIndex* idx = sh.own_idx ? nullptr : &caller;
    if (refine_scratch_first) {  // a stream that has bound refine before: its full links are there
        PairOutputs o;
        bind_below(o, ps, false, true);
    }
    for (int round = 0; round < 2; ++round)  // round 1: every scratch is there whatever the batch binds
        for (int k = 0; k < (sh.own_idx ? 3 : 1); ++k)
            for (int combo = 0; combo < 4; ++combo) {
                const bool refine = combo & 1, bundle = combo & 2;
                const bool had_refine = ps.tr.flink != nullptr;
                PairOutputs next;
                bind_below(next, ps, false, refine);
                if (bundle) CHECK(next.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 4, 3, 1e-3, 0.5, 3.0, 7).code == DVO_OK);
                g_tr_calls.clear();
                g_lm_calls = 0;
                CHECK(launch_pair_outputs(next.take(), ps, k, g, 2, REC, idx, STREAM) == hipSuccess);
                CHECK(g_lm_calls == 1 && g_tr_calls.size() == 1);
                const TrackArgs& a = g_tr_calls[0];
                const size_t off = (size_t)k * sh.set_slots;
                CHECK(a.rec == REC && a.link == LINK && a.scale == SCALE && a.cap == 4 && a.pts_stride == sh.cap);
                CHECK(!a.pose && !a.corr);
                if (refine) {
                    CHECK(a.flink == ps.tr.flink + off && a.rank == ps.tr.rank + 2 * off && a.rank_stride == (int64_t)sh.set_slots);
                    CHECK(a.id == ID && a.refined == REFINED && a.rf_views == 6 && a.rf_iters == 5);
                } else {  // no id or refine kernel: the launch takes id / refined for "a refine binding"
                    CHECK(!a.id && !a.refined && !a.rank && a.rank_stride == 0);
                    CHECK(a.rf_views == 0 && a.rf_iters == 0 && a.rf_use_pose == 0 && a.rf_huber_px == 0 && a.rf_inlier_px == 0);
                }
                if (bundle) {
                    CHECK(a.bd_x == ps.tr.bx + off && a.bundle == BUNDLE && a.bd_points == POINTS);
                    CHECK(a.bd_views == 4 && a.bd_iters == 3 && a.bd_lambda == 1e-3 && a.bd_huber_px == 0.5);
                    CHECK(a.bd_inlier_px == 3.0 && a.bd_min_points == 7 && a.bd_use_pose == 0);
                    CHECK(a.pts_f == PTS && a.fx == 700.5 && a.fy == 701.5 && a.cx == 320.25 && a.cy == 240.75);
                    // the full links: the refine scratch's where there is one, else the bundle's own
                    CHECK(a.flink != nullptr);
                    if (!refine) CHECK(a.flink == (had_refine ? ps.tr.flink + off : ps.tr.blink + off));
                } else {
                    CHECK(!a.bd_x && !a.bundle && !a.bd_points && a.bd_views == 0 && a.bd_iters == 0 && a.bd_min_points == 0);
                    CHECK(a.bd_use_pose == 0 && a.bd_lambda == 0 && a.bd_huber_px == 0 && a.bd_inlier_px == 0);
                    if (!refine) CHECK(!a.flink && !a.pts_f && a.fx == 0);
                }
            }
    // a pose binding pending at bind time feeds the bundle's motions
    PairOutputs next;
    bind_below(next, ps, true, false);
    CHECK(bind(next, ps).code == DVO_OK);
    g_tr_calls.clear();
    CHECK(launch_pair_outputs(next.take(), ps, 0, g, 2, REC, idx, STREAM) == hipSuccess);
    const TrackArgs& a = g_tr_calls.at(0);
    CHECK(a.pose == POSE && a.corr == ps.tr.corr && a.bd_use_pose == 1 && a.bd_views == 6 && a.bd_iters == 5);
    CHECK(a.bd_lambda == DVO_TRACK_BUNDLE_LAMBDA && a.bd_min_points == 8 && a.flink && !a.id && !a.refined);
}
}  // namespace

int main() {
    check_params();
    check_rules();
    for (const Shape& sh : kShapes) {
        check_scratch(sh);
        check_failure(sh);
        check_launches(sh, false);
        check_launches(sh, true);
        CHECK(g_dev.empty() && g_pin.empty());
    }
    std::puts("ok");
    return 0;
}
