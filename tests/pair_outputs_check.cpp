// Host check of csrc/pair_outputs.h and the scratch half of csrc/device_mem.h
// (tests/test_pair_outputs_host.py builds it with the address and undefined-behaviour sanitizers
// and runs it; no GPU): the rules of the four binding setters, the sizes and order of the
// scratches they allocate, a failure of each of those allocations, and the launches of a retiring
// pair set field by field.  The HIP calls are fake_hip.h's; launch_landmarks and launch_tracks are
// defined here and record what they are given.
#include "fake_hip.h"

#include <cmath>

#include "../droplet_visual_odometry_amd/csrc/pair_outputs.h"

using namespace dvo;

namespace {
struct LandmarkCall {
    GeomArgs g;
    int pairs;
    const dvo_pair_record* rec;
    LandmarkScratch L;
    dvo_landmark* out;
    int32_t* count;
    int cap;
    hipStream_t s;
};
struct TracksCall {
    TrackArgs a;
    int pairs;
    hipStream_t s;
};
std::vector<LandmarkCall> g_lm_calls;
std::vector<TracksCall> g_tr_calls;
std::vector<char> g_order;  // 'L' / 'T' per launch
}  // namespace

namespace dvo {
hipError_t launch_landmarks(const GeomArgs& g_set, int pairs, const dvo_pair_record* records, const LandmarkScratch& L,
                            dvo_landmark* out, int32_t* count, int cap, hipStream_t s) {
    g_lm_calls.push_back({g_set, pairs, records, L, out, count, cap, s});
    g_order.push_back('L');
    return hipSuccess;
}
hipError_t launch_tracks(const TrackArgs& a, int pairs, hipStream_t s) {
    g_tr_calls.push_back({a, pairs, s});
    g_order.push_back('T');
    return hipSuccess;
}
}  // namespace dvo

namespace {
static_assert(kRansacRounds == 5, "the ORB shape below is written out for five sets");
static_assert(sizeof(LandmarkTmp) == 32 && sizeof(TrackCorr) == 40 && sizeof(TrackRank) == 8 && kLandmarkTile == 256,
              "the byte counts below assume these");
constexpr int F = 3;
constexpr size_t HC = 5;
constexpr int kDevice = 2;

// The caller's buffers: distinct addresses that nothing dereferences.
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

// A stream's shape and what its scratches must come to (the sizes and their order are
// pinned), written out in bytes, not computed through the code under test.  Per set: F = 3 pairs
// of cap slots.  cap 300 is two landmark tiles, cap 7 one.
struct Shape {
    const char* name;
    int cap, track_sets;
    bool own_idx;
    size_t tiles, set_slots, set_tiles;  // per set: F cap slots, F tiles tile counts
    std::vector<size_t> lm, tr, tp, rf;  // the hipMalloc sizes of each first binding, in order
};
const Shape kShapes[] = {
    // the ORB stream: kRansacRounds = 5 sets (15 pairs, 4500 slots) and its own index copies
    {"orb 300", 300, 5, true, 2, 900, 6,
     {3 * 2 * 256 * 32 + 256, 3 * 2 * 4 + 256},                                           // tmp, tcnt
     {4500 * 4 + 256, 4500 * 8 + 256, 15 * 2 * 4 + 256, 4500 * 4 + 256, 4500 * 4 + 256},  // table, ratio, lcnt, iq, it
     {4500 * 40 + 256},                                                                   // corr
     {4500 * 4 + 256, 2 * 4500 * 8 + 256}},                                               // flink, rank
    // the k-NN stream: one set (3 pairs, 900 slots), the caller-side indices
    {"knn 300", 300, 1, false, 2, 900, 6,
     {49408, 280}, {900 * 4 + 256, 900 * 8 + 256, 3 * 2 * 4 + 256}, {900 * 40 + 256}, {900 * 4 + 256, 2 * 900 * 8 + 256}},
    {"orb 7", 7, 5, true, 1, 21, 3,
     {3 * 256 * 32 + 256, 3 * 4 + 256},
     {105 * 4 + 256, 105 * 8 + 256, 15 * 4 + 256, 105 * 4 + 256, 105 * 4 + 256},
     {105 * 40 + 256},
     {105 * 4 + 256, 2 * 105 * 8 + 256}},
    {"knn 7", 7, 1, false, 1, 21, 3,
     {24832, 268}, {21 * 4 + 256, 21 * 8 + 256, 3 * 4 + 256}, {21 * 40 + 256}, {21 * 4 + 256, 2 * 21 * 8 + 256}},
};

void make_sets(PairSets& ps, const Shape& sh) {
    ps.shape(F, sh.cap, HC, sh.track_sets, sh.own_idx);
    CHECK(ps.ensure(1) == hipSuccess);
}

void check_params() {
    TrackPoseBinding p;
    CHECK(track_pose_params(p, 0, 0, 0, 0));
    CHECK(p.iters == 10 && p.huber_px == 1.0 && p.inlier_px == 2.0 && p.min_points == 6 && p.out == nullptr);
    CHECK(track_pose_params(p, 32, 0.5, 3.0, 3));
    CHECK(p.iters == 32 && p.huber_px == 0.5 && p.inlier_px == 3.0 && p.min_points == 3);
    CHECK(track_pose_params(p, -1, -1.0, -1.0, -1) && p.iters == 10 && p.min_points == 6);  // <= 0: the default
    CHECK(!track_pose_params(p, 33, 0, 0, 0));
    CHECK(!track_pose_params(p, 0, 0, 0, 2));
    CHECK(!track_pose_params(p, 0, NAN, 0, 0) && !track_pose_params(p, 0, 0, NAN, 0));
    TrackRefineBinding r;
    CHECK(track_refine_params(r, 0, 0, 0, 0));
    CHECK(r.views == 6 && r.iters == 5 && r.huber_px == 1.0 && r.inlier_px == 2.0 && !r && !r.use_pose);
    CHECK(track_refine_params(r, 3, 16, 0.5, 3.0) && r.views == 3 && r.iters == 16 && r.huber_px == 0.5 && r.inlier_px == 3.0);
    CHECK(track_refine_params(r, 8, 1, 0, 0) && r.views == 8 && r.iters == 1);
    CHECK(!track_refine_params(r, 2, 0, 0, 0) && !track_refine_params(r, 9, 0, 0, 0));
    CHECK(!track_refine_params(r, 0, 17, 0, 0));
    CHECK(!track_refine_params(r, 0, 0, NAN, 0) && !track_refine_params(r, 0, 0, 0, NAN));
}

// ---- the setters' rules ---------------------------------------------------------------------
enum Op {
    LM,         // set_landmarks(out, count, 4)
    LM2,        // set_landmarks(out + 1, count + 1, 9): another binding
    LM_NULL,    // set_landmarks(null, count, 4)
    LM_CAP0,    // set_landmarks(out, count, 0)
    LM_NOCNT,   // set_landmarks(out, null, 4)
    TR_BOTH,    // set_tracks(link, scale)
    TR_LINK,    // set_tracks(link, null)
    TR_SCALE,   // set_tracks(null, scale)
    TR_NULL,    // set_tracks(null, null)
    TP,         // set_track_poses(pose, 0, 0, 0, 0)
    TP_ARGS,    // set_track_poses(pose, 7, 0.5, 3.0, 4)
    TP_NULL,    // set_track_poses(null, 33, ...): the parameters of a clearing call are not read
    TP_ITERS,   // set_track_poses(pose, 33, 0, 0, 0)
    TP_MINPTS,  // set_track_poses(pose, 0, 0, 0, 2)
    TP_NAN,     // set_track_poses(pose, 0, NAN, 0, 0)
    RF_BOTH,    // set_track_refine(refined, id, 0, 0, 0, 0)
    RF_ID,      // set_track_refine(null, id, 4, 3, 0.5, 3.0)
    RF_NULL,    // set_track_refine(null, null, 2, ...): the parameters of a clearing call are not read
    RF_VIEWS2,  // set_track_refine(refined, id, 2, 0, 0, 0)
    RF_VIEWS9,  // set_track_refine(refined, id, 9, 0, 0, 0)
    RF_ITERS,   // set_track_refine(refined, id, 0, 17, 0, 0)
    RF_NAN,     // set_track_refine(refined, id, 0, 0, 0, NAN)
};
// the pending state after a step: which buffers are bound
enum : unsigned { kLm = 1, kLm2 = 2, kLink = 4, kScale = 8, kTp = 16, kRfRefined = 32, kRfId = 64, kUsePose = 128 };
constexpr unsigned kTr = kLink | kScale, kRf = kRfRefined | kRfId;

const char* const kMsgLm = "landmarks need cap >= 1 and a count buffer";
const char* const kMsgTr = "tracks go with a pending landmark binding";
const char* const kMsgTp = "track poses go with a pending tracks binding that has a scale buffer";
const char* const kMsgTpArgs = "track poses: iters <= 32, min_points >= 3, no NaN";
const char* const kMsgRf = "track refine goes with a pending tracks binding that has link and scale buffers";
const char* const kMsgRfArgs = "track refine: views 3..8, iters <= 16, no NaN";

struct Step {
    Op op;
    int code;
    const char* msg;  // of a DVO_EINVAL
    unsigned state;   // pending afterwards
    bool device;      // the call made the device current (it got as far as its scratch)
};

BindResult apply(PairOutputs& o, PairSets& ps, Op op) {
    switch (op) {
        case LM: return o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4);
        case LM2: return o.set_landmarks(ps, kDevice, LM_OUT + 1, LM_CNT + 1, 9);
        case LM_NULL: return o.set_landmarks(ps, kDevice, nullptr, LM_CNT, 4);
        case LM_CAP0: return o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 0);
        case LM_NOCNT: return o.set_landmarks(ps, kDevice, LM_OUT, nullptr, 4);
        case TR_BOTH: return o.set_tracks(ps, kDevice, LINK, SCALE);
        case TR_LINK: return o.set_tracks(ps, kDevice, LINK, nullptr);
        case TR_SCALE: return o.set_tracks(ps, kDevice, nullptr, SCALE);
        case TR_NULL: return o.set_tracks(ps, kDevice, nullptr, nullptr);
        case TP: return o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 0);
        case TP_ARGS: return o.set_track_poses(ps, kDevice, POSE, 7, 0.5, 3.0, 4);
        case TP_NULL: return o.set_track_poses(ps, kDevice, nullptr, 33, NAN, NAN, 1);
        case TP_ITERS: return o.set_track_poses(ps, kDevice, POSE, 33, 0, 0, 0);
        case TP_MINPTS: return o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 2);
        case TP_NAN: return o.set_track_poses(ps, kDevice, POSE, 0, NAN, 0, 0);
        case RF_BOTH: return o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, 0);
        case RF_ID: return o.set_track_refine(ps, kDevice, nullptr, ID, 4, 3, 0.5, 3.0);
        case RF_NULL: return o.set_track_refine(ps, kDevice, nullptr, nullptr, 2, 17, NAN, NAN);
        case RF_VIEWS2: return o.set_track_refine(ps, kDevice, REFINED, ID, 2, 0, 0, 0);
        case RF_VIEWS9: return o.set_track_refine(ps, kDevice, REFINED, ID, 9, 0, 0, 0);
        case RF_ITERS: return o.set_track_refine(ps, kDevice, REFINED, ID, 0, 17, 0, 0);
        case RF_NAN: return o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, NAN);
    }
    die("unknown op", __LINE__);
}

unsigned state_of(const PairOutputs& o) {
    unsigned s = 0;
    if (o.lm.out == LM_OUT) {
        CHECK(o.lm.count == LM_CNT && o.lm.cap == 4);
        s |= kLm;
    } else if (o.lm.out == LM_OUT + 1) {
        CHECK(o.lm.count == LM_CNT + 1 && o.lm.cap == 9);
        s |= kLm2;
    } else {
        CHECK(!o.lm.out && !o.lm.count && o.lm.cap == 0);
    }
    CHECK(!o.tr.link || o.tr.link == LINK);
    CHECK(!o.tr.scale || o.tr.scale == SCALE);
    CHECK(!o.tp.out || o.tp.out == POSE);
    CHECK(!o.rf.refined || o.rf.refined == REFINED);
    CHECK(!o.rf.id || o.rf.id == ID);
    if (o.tr.link) s |= kLink;
    if (o.tr.scale) s |= kScale;
    if (o.tp.out) s |= kTp;
    if (o.rf.refined) s |= kRfRefined;
    if (o.rf.id) s |= kRfId;
    if (o.rf.use_pose) s |= kUsePose;
    // a cleared binding is an empty one, parameters included
    if (!o.tp.out) CHECK(o.tp.iters == 0 && o.tp.min_points == 0 && o.tp.huber_px == 0 && o.tp.inlier_px == 0);
    if (!o.rf) CHECK(o.rf.views == 0 && o.rf.iters == 0 && o.rf.huber_px == 0 && o.rf.inlier_px == 0 && !o.rf.use_pose);
    return s;
}

void run_steps(const std::vector<Step>& steps, PairOutputs o = PairOutputs{}) {
    PairSets ps;
    make_sets(ps, kShapes[2]);
    for (size_t i = 0; i < steps.size(); ++i) {
        const Step& st = steps[i];
        reset_log();
        const BindResult r = apply(o, ps, st.op);
        const unsigned got = state_of(o);
        if (r.code != st.code || got != st.state || (st.msg ? !r.what || std::strcmp(r.what, st.msg) : r.what != nullptr) ||
            r.hip != hipSuccess || g_devices != (st.device ? std::vector<int>{kDevice} : std::vector<int>{})) {
            std::fprintf(stderr, "step %zu (op %d): code %d, state 0x%x, message %s, %zu device calls\n", i, (int)st.op,
                         r.code, got, r.what ? r.what : "(none)", g_devices.size());
            die("a setter step differs from the table", __LINE__);
        }
    }
}

void check_rules() {
    constexpr unsigned kAll = kLm | kTr | kTp | kRf | kUsePose;
    // every binding needs the ones before it
    run_steps({
        {TR_BOTH, DVO_EINVAL, kMsgTr, 0, false},
        {TP, DVO_EINVAL, kMsgTp, 0, false},
        {RF_BOTH, DVO_EINVAL, kMsgRf, 0, false},
        {LM_CAP0, DVO_EINVAL, kMsgLm, 0, false},
        {LM_NOCNT, DVO_EINVAL, kMsgLm, 0, false},
        {LM, DVO_OK, nullptr, kLm, true},
        {TP, DVO_EINVAL, kMsgTp, kLm, false},
        {RF_BOTH, DVO_EINVAL, kMsgRf, kLm, false},
        {TR_LINK, DVO_OK, nullptr, kLm | kLink, true},
        {TP, DVO_EINVAL, kMsgTp, kLm | kLink, false},      // no scale buffer
        {RF_BOTH, DVO_EINVAL, kMsgRf, kLm | kLink, false},  // no scale buffer
        {TR_SCALE, DVO_OK, nullptr, kLm | kScale, true},
        {TP, DVO_OK, nullptr, kLm | kScale | kTp, true},
        {RF_BOTH, DVO_EINVAL, kMsgRf, kLm | kScale | kTp, false},  // no link buffer; nothing cleared
        {TR_BOTH, DVO_OK, nullptr, kLm | kTr, true},               // a tracks binding clears the pose binding
        {RF_BOTH, DVO_OK, nullptr, kLm | kTr | kRf, true},         // no pose binding pending: use_pose off
        {TP, DVO_OK, nullptr, kLm | kTr | kTp, true},              // a pose binding clears the refine binding
        {RF_ID, DVO_OK, nullptr, kLm | kTr | kTp | kRfId | kUsePose, true},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
    });
    // what a failing or clearing call leaves
    run_steps({
        {LM, DVO_OK, nullptr, kLm, true},
        {TR_BOTH, DVO_OK, nullptr, kLm | kTr, true},
        {TP_ARGS, DVO_OK, nullptr, kLm | kTr | kTp, true},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {RF_VIEWS2, DVO_EINVAL, kMsgRfArgs, kAll, false},  // a failing refine call clears nothing
        {RF_VIEWS9, DVO_EINVAL, kMsgRfArgs, kAll, false},
        {RF_ITERS, DVO_EINVAL, kMsgRfArgs, kAll, false},
        {RF_NAN, DVO_EINVAL, kMsgRfArgs, kAll, false},
        {LM_CAP0, DVO_EINVAL, kMsgLm, kAll, false},   // nor does a failing landmark call
        {LM_NOCNT, DVO_EINVAL, kMsgLm, kAll, false},
        {LM2, DVO_OK, nullptr, (kAll & ~kLm) | kLm2, true},  // another landmark buffer: the later bindings stay
        {LM, DVO_OK, nullptr, kAll, true},
        {TP_ITERS, DVO_EINVAL, kMsgTpArgs, kLm | kTr | kTp, false},  // a failing pose call clears the refine binding only
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {TP_MINPTS, DVO_EINVAL, kMsgTpArgs, kLm | kTr | kTp, false},
        {TP_NAN, DVO_EINVAL, kMsgTpArgs, kLm | kTr | kTp, false},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {RF_NULL, DVO_OK, nullptr, kLm | kTr | kTp, false},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {TP_NULL, DVO_OK, nullptr, kLm | kTr, false},
        {RF_BOTH, DVO_OK, nullptr, kLm | kTr | kRf, true},
        {TP, DVO_OK, nullptr, kLm | kTr | kTp, true},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {TR_NULL, DVO_OK, nullptr, kLm, false},
        {TR_BOTH, DVO_OK, nullptr, kLm | kTr, true},
        {TP, DVO_OK, nullptr, kLm | kTr | kTp, true},
        {RF_BOTH, DVO_OK, nullptr, kAll, true},
        {LM_NULL, DVO_OK, nullptr, 0, false},  // clears all four
        {TR_NULL, DVO_OK, nullptr, 0, false},
        {TP_NULL, DVO_OK, nullptr, 0, false},
        {RF_NULL, DVO_OK, nullptr, 0, false},
    });
    // the bindings a failing call finds are cleared whatever made it fail: without a landmark binding
    // (a state the setters themselves do not reach) set_tracks clears poses and refine, and
    // set_track_poses refine, before they fail; set_track_refine nothing
    PairOutputs odd;
    odd.tr = TracksBinding{LINK, SCALE};
    odd.tp.out = POSE;
    odd.rf.refined = REFINED;
    run_steps({{RF_BOTH, DVO_EINVAL, kMsgRf, kTr | kTp | kRfRefined, false},
               {TP, DVO_EINVAL, kMsgTp, kTr | kTp, false},
               {TR_BOTH, DVO_EINVAL, kMsgTr, kTr, false}},
              odd);
    odd.rf.refined = REFINED;
    run_steps({{TR_LINK, DVO_EINVAL, kMsgTr, kTr, false}}, odd);

    // the parameters are stored with their defaults filled in; take() hands over all four
    PairSets ps;
    make_sets(ps, kShapes[2]);
    PairOutputs o;
    CHECK(apply(o, ps, LM).code == DVO_OK && apply(o, ps, TR_BOTH).code == DVO_OK);
    CHECK(apply(o, ps, TP_ARGS).code == DVO_OK && apply(o, ps, RF_ID).code == DVO_OK);
    CHECK(o.tp.iters == 7 && o.tp.huber_px == 0.5 && o.tp.inlier_px == 3.0 && o.tp.min_points == 4);
    CHECK(o.rf.views == 4 && o.rf.iters == 3 && o.rf.huber_px == 0.5 && o.rf.inlier_px == 3.0 && o.rf.use_pose);
    const PairOutputs t = o.take();
    CHECK(state_of(o) == 0);
    CHECK(state_of(t) == (kLm | kTr | kTp | kRfId | kUsePose));
    CHECK(t.tp.iters == 7 && t.tp.min_points == 4 && t.rf.views == 4 && t.rf.iters == 3);
    CHECK(state_of(o.take()) == 0);  // nothing pending: nothing taken
    CHECK(apply(o, ps, LM).code == DVO_OK && apply(o, ps, TR_BOTH).code == DVO_OK);
    CHECK(apply(o, ps, TP).code == DVO_OK && apply(o, ps, RF_BOTH).code == DVO_OK);
    CHECK(o.tp.iters == 10 && o.tp.huber_px == 1.0 && o.tp.inlier_px == 2.0 && o.tp.min_points == 6);
    CHECK(o.rf.views == 6 && o.rf.iters == 5 && o.rf.huber_px == 1.0 && o.rf.inlier_px == 2.0);
}

// ---- the scratches --------------------------------------------------------------------------
std::vector<const void*> scratch_pointers(const PairSets& ps) {
    return {ps.lm.tmp, ps.lm.tcnt, ps.tr.table, ps.tr.ratio, ps.tr.lcnt, ps.tr.iq, ps.tr.it, ps.tr.corr, ps.tr.flink, ps.tr.rank};
}

void check_scratch(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    for (const void* p : scratch_pointers(ps)) CHECK(p == nullptr);  // nothing before the first binding
    PairOutputs o;
    const Op ops[4] = {LM, TR_BOTH, TP, RF_BOTH};
    const std::vector<size_t>* want[4] = {&sh.lm, &sh.tr, &sh.tp, &sh.rf};
    for (int i = 0; i < 4; ++i) {
        reset_log();
        CHECK(apply(o, ps, ops[i]).code == DVO_OK);
        CHECK(g_mallocs == *want[i] && g_frees == 0 && g_syncs == 0);
    }
    const std::vector<const void*> first = scratch_pointers(ps);
    for (size_t i = 0; i < first.size(); ++i)
        CHECK(sh.own_idx || (i != 5 && i != 6) ? g_dev.count(const_cast<void*>(first[i])) == 1 : first[i] == nullptr);
    const size_t live = g_dev.size();
    CHECK(live == 18 + sh.lm.size() + sh.tr.size() + sh.tp.size() + sh.rf.size());
    // a second binding of each allocates nothing
    reset_log();
    (void)o.take();
    for (Op op : ops) CHECK(apply(o, ps, op).code == DVO_OK);
    CHECK(g_mallocs.empty() && g_frees == 0 && scratch_pointers(ps) == first);
    // growing the pair sets afterwards frees the sets' 18 arrays and allocates them anew; the
    // scratches are neither freed nor moved
    reset_log();
    CHECK(ps.ensure(5) == hipSuccess && ps.nsets == 5);
    CHECK(g_mallocs.size() == 18 && g_frees == 18 && g_syncs == 1 && g_dev.size() == live);
    CHECK(scratch_pointers(ps) == first);
    for (const void* p : first) CHECK(!p || g_dev.count(const_cast<void*>(p)) == 1);
    ps.release();  // the sets alone
    CHECK(g_dev.size() == live - 18 && scratch_pointers(ps) == first);
}

// Fail each allocation of each first binding in turn: the scratch stays empty, nothing leaks, the
// pending binding is what it was, and the same call then succeeds.
void check_failures(const Shape& sh) {
    const Op ops[4] = {LM, TR_BOTH, TP, RF_BOTH};
    const std::vector<size_t>* want[4] = {&sh.lm, &sh.tr, &sh.tp, &sh.rf};
    const char* const what[4] = {"PairSets::ensure_landmarks", "PairSets::ensure_tracks", "PairSets::ensure_track_poses",
                                 "PairSets::ensure_track_refine"};
    const unsigned before[4] = {0, kLm, kLm | kTr, kLm | kTr | kTp};
    const unsigned after[4] = {kLm, kLm | kTr, kLm | kTr | kTp, kLm | kTr | kTp | kRf | kUsePose};
    for (int i = 0; i < 4; ++i)
        for (size_t n = 0; n < want[i]->size(); ++n) {
            PairSets ps;
            make_sets(ps, sh);
            PairOutputs o;
            for (int j = 0; j < i; ++j) CHECK(apply(o, ps, ops[j]).code == DVO_OK);
            const std::vector<const void*> ptrs = scratch_pointers(ps);
            const size_t live = g_dev.size();
            reset_log();
            g_fail_at = (int)n;
            const BindResult r = apply(o, ps, ops[i]);
            CHECK(r.code == DVO_EHIP && r.hip == hipErrorOutOfMemory && r.what && std::strcmp(r.what, what[i]) == 0);
            CHECK(g_mallocs.size() == n + 1 && g_dev.size() == live && scratch_pointers(ps) == ptrs);
            CHECK(state_of(o) == before[i] && g_devices == std::vector<int>{kDevice});
            reset_log();
            const BindResult again = apply(o, ps, ops[i]);
            CHECK(again.code == DVO_OK && again.what == nullptr && g_mallocs == *want[i] && state_of(o) == after[i]);
            CHECK(g_dev.size() == live + want[i]->size());
        }
    // a failing scratch is a failing call like another: set_tracks has cleared poses and refine by
    // then and set_track_poses refine, and the binding itself is the one from before
    PairSets ps, fresh;
    make_sets(ps, sh);
    make_sets(fresh, sh);
    PairOutputs o;
    for (Op op : ops) CHECK(apply(o, ps, op).code == DVO_OK);
    const size_t live = g_dev.size();
    reset_log();
    g_fail_at = 0;
    CHECK(o.set_track_refine(fresh, kDevice, nullptr, ID, 0, 0, 0, 0).code == DVO_EHIP);  // no track scratch there
    CHECK(state_of(o) == (kLm | kTr | kTp | kRf | kUsePose) && g_mallocs.empty());
    CHECK(o.set_track_poses(fresh, kDevice, POSE, 5, 0, 0, 0).code == DVO_EHIP);
    CHECK(state_of(o) == (kLm | kTr | kTp) && o.tp.iters == 10 && g_mallocs.empty());
    CHECK(apply(o, ps, RF_BOTH).code == DVO_OK);
    CHECK(o.set_tracks(fresh, kDevice, LINK, nullptr).code == DVO_EHIP);
    CHECK(state_of(o) == (kLm | kTr) && g_mallocs.size() == 1 && g_dev.size() == live);
    for (const void* p : scratch_pointers(fresh)) CHECK(p == nullptr);
}

// ---- the launches of a retiring set -----------------------------------------------------------
void check_launches(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    CHECK(ps.ensure(sh.track_sets) == hipSuccess);
    GeomArgs g{};
    g.pts_f = PTS;
    g.fx = 700.5, g.fy = 701.5, g.cx = 320.25, g.cy = 240.75;
    g.pts_stride = sh.cap;
    static dvo_dmatch matches[1];  // the k-NN stream's caller-side index source
    const TrackIndex caller{&matches->queryIdx, &matches->trainIdx, sh.cap, 4};
    const TrackIndex* idx = sh.own_idx ? nullptr : &caller;
    const int pairs = 2;
    // level 0: no binding; 1: landmarks; 2: + tracks; 3: + poses; 4: + refine.  The scratch of every
    // level is there from the first round on (level 4 of set 0 allocates the last of it), as in a
    // stream that has bound everything once.
    const std::vector<Op> levels[5] = {{}, {LM}, {LM, TR_BOTH}, {LM, TR_BOTH, TP_ARGS}, {LM, TR_BOTH, TP_ARGS, RF_ID}};
    for (int round = 0; round < 2; ++round)
        for (int k = 0; k < (sh.own_idx ? 3 : 1); ++k)
            for (int level = 0; level < 5; ++level) {
                PairOutputs next;
                for (Op op : levels[level]) CHECK(apply(next, ps, op).code == DVO_OK);
                const PairOutputs o = next.take();
                g_lm_calls.clear();
                g_tr_calls.clear();
                g_order.clear();
                CHECK(launch_pair_outputs(o, ps, k, g, pairs, REC, idx, STREAM) == hipSuccess);
                if (level == 0) {
                    CHECK(g_order.empty());
                    continue;
                }
                CHECK(g_order == (level == 1 ? std::vector<char>{'L'} : std::vector<char>{'L', 'T'}));  // landmarks first
                const LandmarkCall& l = g_lm_calls[0];
                CHECK(std::memcmp(&l.g, &g, sizeof(g)) == 0 && l.pairs == pairs && l.rec == REC && l.s == STREAM);
                CHECK(l.L.tmp == ps.lm.tmp && l.L.tcnt == ps.lm.tcnt);  // one copy whatever the set
                CHECK(l.out == LM_OUT && l.count == LM_CNT && l.cap == 4);
                if (level == 1) continue;
                const TracksCall& t = g_tr_calls[0];
                const TrackArgs& a = t.a;
                CHECK(t.pairs == pairs && t.s == STREAM);
                const size_t off = (size_t)k * sh.set_slots;  // set k's slots: k F cap before it
                CHECK(a.L.tmp == ps.lm.tmp && a.L.tcnt == ps.lm.tcnt && a.tiles == (int)sh.tiles);
                CHECK(a.table == ps.tr.table + off && a.kp_cap == sh.cap);
                CHECK(a.ratio == ps.tr.ratio + off && a.pts_stride == sh.cap);
                CHECK(a.lcnt == ps.tr.lcnt + (size_t)k * sh.set_tiles);
                if (sh.own_idx) {
                    CHECK(a.mq == ps.tr.iq + off && a.mt == ps.tr.it + off && a.idx_stride == sh.cap && a.idx_step == 1);
                } else {
                    CHECK(ps.tr.iq == nullptr && ps.tr.it == nullptr);
                    CHECK(a.mq == &matches->queryIdx && a.mt == &matches->trainIdx && a.idx_stride == sh.cap && a.idx_step == 4);
                    CHECK((const char*)a.mt - (const char*)a.mq == 4);
                }
                CHECK(a.rec == REC && a.link == LINK && a.cap == 4 && a.scale == SCALE);
                if (level >= 3) {
                    CHECK(a.pose == POSE && a.corr == ps.tr.corr + off);
                    CHECK(a.pose_iters == 7 && a.pose_min_points == 4 && a.huber_px == 0.5 && a.inlier_px == 3.0);
                    CHECK(a.pts_f == PTS && a.fx == 700.5 && a.fy == 701.5 && a.cx == 320.25 && a.cy == 240.75);
                } else {  // the kernels take corr for "a pose binding": no trace of the scratch without one
                    CHECK(!a.pose && !a.corr && a.pose_iters == 0 && a.pose_min_points == 0 && a.huber_px == 0 && a.inlier_px == 0);
                    CHECK(!a.pts_f && a.fx == 0 && a.fy == 0 && a.cx == 0 && a.cy == 0);
                }
                if (level == 4) {
                    CHECK(a.flink == ps.tr.flink + off && a.rank == ps.tr.rank + 2 * off);
                    CHECK(a.rank_stride == (int64_t)sh.set_slots);
                    CHECK(a.id == ID && a.refined == nullptr && a.rf_views == 4 && a.rf_iters == 3 && a.rf_use_pose == 1);
                    CHECK(a.rf_huber_px == 0.5 && a.rf_inlier_px == 3.0);
                } else {  // and flink for "a refine binding"
                    CHECK(!a.flink && !a.rank && a.rank_stride == 0 && !a.id && !a.refined);
                    CHECK(a.rf_views == 0 && a.rf_iters == 0 && a.rf_use_pose == 0 && a.rf_huber_px == 0 && a.rf_inlier_px == 0);
                }
            }
    // a refine binding without a pose binding: the points and the camera still go along, use_pose off
    PairOutputs next;
    for (Op op : {LM, TR_BOTH, RF_BOTH}) CHECK(apply(next, ps, op).code == DVO_OK);
    g_tr_calls.clear();
    CHECK(launch_pair_outputs(next.take(), ps, 0, g, pairs, REC, idx, STREAM) == hipSuccess);
    const TrackArgs& a = g_tr_calls.at(0).a;
    CHECK(!a.pose && !a.corr && a.flink == ps.tr.flink && a.rank == ps.tr.rank && a.rank_stride == (int64_t)sh.set_slots);
    CHECK(a.id == ID && a.refined == REFINED && a.rf_views == 6 && a.rf_iters == 5 && a.rf_use_pose == 0);
    CHECK(a.pts_f == PTS && a.fx == 700.5 && a.cy == 240.75);
}
}  // namespace

int main() {
    check_params();
    check_rules();
    for (const Shape& sh : kShapes) {
        check_scratch(sh);
        check_failures(sh);
        check_launches(sh);
        CHECK(g_dev.empty() && g_pin.empty());
    }
    std::puts("ok");
    return 0;
}
