// Host check of the PnP binding in csrc/pair_outputs.h and of its scratch in csrc/device_mem.h
// (tests/test_track_pnp_rules_host.py builds it with the address and undefined-behaviour
// sanitizers and runs it; no GPU): the sixth setter's rules, its parameters, which setters clear it
// and that it clears nothing, the size and the one allocation of its scratch, a failure of that
// allocation, and the TrackArgs a retiring set hands to launch_tracks with and without the other
// bindings.  The HIP calls are fake_hip.h's; launch_landmarks and launch_tracks are defined here
// and record what they are given.
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
static_assert(sizeof(PnpCorr) == 48 && sizeof(dvo_track_pnp) == 144 && kLandmarkTile == 256, "the byte counts below assume these");
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
dvo_track_pnp* const PNP = reinterpret_cast<dvo_track_pnp*>(0xd000);
uint8_t* const MASK = reinterpret_cast<uint8_t*>(0xe000);

const char* const kMsgPn = "track pnp goes with a pending tracks binding";
const char* const kMsgPnArgs = "track pnp: hyps <= 512, iters <= 32, min_points >= 4, mask_cap >= 1 with a mask, no NaN";

// A stream's shape and the bytes of its PnP scratch, written out: 48 B per slot of every track set
// and 4 B per tile of 256 slots of each of its F pairs, in one allocation.
struct Shape {
    const char* name;
    int cap, track_sets;
    bool own_idx;
    size_t set_slots, all_slots, tiles, bytes;
};
const Shape kShapes[] = {
    {"orb 300", 300, 5, true, 900, 4500, 5 * 3 * 2, 4500 * 48 + 30 * 4 + 256},
    {"knn 300", 300, 1, false, 900, 900, 3 * 2, 900 * 48 + 6 * 4 + 256},
    {"orb 7", 7, 5, true, 21, 105, 5 * 3 * 1, 105 * 48 + 15 * 4 + 256},
    {"knn 7", 7, 1, false, 21, 21, 3 * 1, 21 * 48 + 3 * 4 + 256},
};

void make_sets(PairSets& ps, const Shape& sh) {
    ps.shape(F, sh.cap, HC, sh.track_sets, sh.own_idx);
    CHECK(ps.ensure(sh.track_sets) == hipSuccess);
}

void bind_below(PairOutputs& o, PairSets& ps, bool poses, bool refine, bool bundle) {
    CHECK(o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4).code == DVO_OK);
    CHECK(o.set_tracks(ps, kDevice, LINK, SCALE).code == DVO_OK);
    if (poses) CHECK(o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 0).code == DVO_OK);
    if (refine) CHECK(o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, 0).code == DVO_OK);
    if (bundle) CHECK(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, 0, 0, 0, 0).code == DVO_OK);
}

BindResult bind(PairOutputs& o, PairSets& ps) { return o.set_track_pnp(ps, kDevice, PNP, MASK, 300, 0, 0, 0, 0, 0, 0); }

bool empty(const TrackPnpBinding& b) {
    return !b.out && !b.mask && b.mask_cap == 0 && b.hyps == 0 && b.iters == 0 && b.min_points == 0 && b.huber_px == 0 &&
           b.inlier_px == 0 && b.seed == 0;
}

void check_params() {
    TrackPnpBinding b;
    CHECK(track_pnp_params(b, 0, 0, 0, 0, 0, 0));
    CHECK(b.hyps == 128 && b.iters == 10 && b.huber_px == 1.0 && b.inlier_px == 2.0 && b.min_points == 6 && b.seed == 0);
    CHECK(track_pnp_params(b, -1, -1, -1.0, -1.0, -1, 0) && b.hyps == 128 && b.iters == 10 && b.min_points == 6);
    CHECK(track_pnp_params(b, 512, 32, 0.5, 3.0, 4, ~0ull));
    CHECK(b.hyps == 512 && b.iters == 32 && b.huber_px == 0.5 && b.inlier_px == 3.0 && b.min_points == 4 && b.seed == ~0ull);
    CHECK(track_pnp_params(b, 1, 1, INFINITY, 0, 1000, 7) && b.hyps == 1 && b.iters == 1 && b.min_points == 1000 && b.seed == 7);
    CHECK(!track_pnp_params(b, 513, 0, 0, 0, 0, 0) && !track_pnp_params(b, 0, 33, 0, 0, 0, 0));
    for (int mp = 1; mp <= 3; ++mp) CHECK(!track_pnp_params(b, 0, 0, 0, 0, mp, 0));
    CHECK(!track_pnp_params(b, 0, 0, NAN, 0, 0, 0) && !track_pnp_params(b, 0, 0, 0, NAN, 0, 0));
}

void expect(const BindResult& r, int code, const char* msg) {
    CHECK(r.code == code && r.hip == hipSuccess);
    CHECK(msg ? r.what && std::strcmp(r.what, msg) == 0 : r.what == nullptr);
}

void check_rules() {
    PairSets ps;
    make_sets(ps, kShapes[2]);
    PairOutputs o;
    // it needs landmarks and a tracks binding; either buffer of that will do
    expect(bind(o, ps), DVO_EINVAL, kMsgPn);
    CHECK(o.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4).code == DVO_OK);
    expect(bind(o, ps), DVO_EINVAL, kMsgPn);
    CHECK(empty(o.pn) && !ps.tr.pc);
    CHECK(o.set_tracks(ps, kDevice, LINK, nullptr).code == DVO_OK);
    reset_log();
    expect(bind(o, ps), DVO_OK, nullptr);
    CHECK(g_devices == std::vector<int>{kDevice});
    CHECK(o.pn.out == PNP && o.pn.mask == MASK && o.pn.mask_cap == 300 && o.pn.hyps == 128 && o.pn.min_points == 6);
    CHECK(o.set_tracks(ps, kDevice, nullptr, SCALE).code == DVO_OK);
    CHECK(empty(o.pn));  // every set_tracks clears it
    expect(bind(o, ps), DVO_OK, nullptr);
    // without a mask the cap is not kept; a mask needs a cap; a null d_pnp clears, whatever the rest
    expect(o.set_track_pnp(ps, kDevice, PNP, nullptr, 77, 64, 3, 0.5, 3.0, 7, 9), DVO_OK, nullptr);
    CHECK(o.pn.out == PNP && !o.pn.mask && o.pn.mask_cap == 0 && o.pn.hyps == 64 && o.pn.iters == 3 && o.pn.seed == 9);
    CHECK(o.pn.huber_px == 0.5 && o.pn.inlier_px == 3.0 && o.pn.min_points == 7);
    expect(o.set_track_pnp(ps, kDevice, PNP, MASK, 0, 0, 0, 0, 0, 0, 0), DVO_EINVAL, kMsgPnArgs);
    expect(o.set_track_pnp(ps, kDevice, PNP, MASK, -4, 0, 0, 0, 0, 0, 0), DVO_EINVAL, kMsgPnArgs);
    CHECK(o.pn.out == PNP && o.pn.hyps == 64);  // a call out of range clears nothing
    reset_log();
    expect(o.set_track_pnp(ps, kDevice, nullptr, MASK, 0, 513, 33, NAN, NAN, 1, 0), DVO_OK, nullptr);
    CHECK(empty(o.pn) && g_devices.empty());
    // out of range: nothing is cleared, neither it nor the bindings beside it
    bind_below(o, ps, true, true, true);
    expect(bind(o, ps), DVO_OK, nullptr);
    const int bad[][3] = {{513, 0, 0}, {0, 33, 0}, {0, 0, 1}, {0, 0, 3}};
    for (const auto& v : bad) {
        reset_log();
        expect(o.set_track_pnp(ps, kDevice, PNP, MASK, 300, v[0], v[1], 0, 0, v[2], 0), DVO_EINVAL, kMsgPnArgs);
        CHECK(g_devices.empty());
    }
    expect(o.set_track_pnp(ps, kDevice, PNP, MASK, 300, 0, 0, NAN, 0, 0, 0), DVO_EINVAL, kMsgPnArgs);
    expect(o.set_track_pnp(ps, kDevice, PNP, MASK, 300, 0, 0, 0, NAN, 0, 0), DVO_EINVAL, kMsgPnArgs);
    CHECK(o.pn.out == PNP && o.pn.mask == MASK && o.pn.hyps == 128);
    // binding it cleared nothing
    CHECK(o.lm.out == LM_OUT && o.tr.link == LINK && o.tr.scale == SCALE && o.tp.out == POSE);
    CHECK(o.rf.refined == REFINED && o.rf.id == ID && o.bd.out == BUNDLE && o.bd.points == POINTS);
    // the pose, refine and bundle setters leave it alone, binding, clearing or failing
    expect(o.set_track_bundle(ps, kDevice, BUNDLE, POINTS, 0, 0, 0, 0, 0, 0), DVO_OK, nullptr);
    expect(o.set_track_bundle(ps, kDevice, nullptr, nullptr, 0, 0, 0, 0, 0, 0), DVO_OK, nullptr);
    expect(o.set_track_refine(ps, kDevice, REFINED, ID, 0, 0, 0, 0), DVO_OK, nullptr);
    expect(o.set_track_refine(ps, kDevice, nullptr, nullptr, 0, 0, 0, 0), DVO_OK, nullptr);
    expect(o.set_track_poses(ps, kDevice, POSE, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(o.set_track_poses(ps, kDevice, POSE, 33, 0, 0, 0).code == DVO_EINVAL);
    expect(o.set_track_poses(ps, kDevice, nullptr, 0, 0, 0, 0), DVO_OK, nullptr);
    CHECK(o.pn.out == PNP && o.pn.mask == MASK && o.pn.mask_cap == 300 && !o.tp.out && !o.rf && !o.bd);
    // another landmark buffer: it stays; set_tracks and set_landmarks(NULL) clear it
    expect(o.set_landmarks(ps, kDevice, LM_OUT + 1, LM_CNT + 1, 9), DVO_OK, nullptr);
    CHECK(o.pn.out == PNP);
    expect(o.set_tracks(ps, kDevice, LINK, SCALE), DVO_OK, nullptr);
    CHECK(empty(o.pn) && o.tr.link == LINK);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_tracks(ps, kDevice, nullptr, nullptr), DVO_OK, nullptr);
    CHECK(empty(o.pn) && !o.tr);
    expect(bind(o, ps), DVO_EINVAL, kMsgPn);
    CHECK(o.set_tracks(ps, kDevice, LINK, SCALE).code == DVO_OK);
    expect(bind(o, ps), DVO_OK, nullptr);
    expect(o.set_landmarks(ps, kDevice, nullptr, nullptr, 0), DVO_OK, nullptr);
    CHECK(empty(o.pn) && !o.lm.out && !o.tr);
    // take() hands it over with the rest
    bind_below(o, ps, true, false, false);
    expect(o.set_track_pnp(ps, kDevice, PNP, MASK, 50, 512, 32, 0.5, 3.0, 4, 11), DVO_OK, nullptr);
    const PairOutputs t = o.take();
    CHECK(empty(o.pn) && !o.lm.out);
    CHECK(t.pn.out == PNP && t.pn.mask == MASK && t.pn.mask_cap == 50 && t.pn.hyps == 512 && t.pn.iters == 32);
    CHECK(t.pn.huber_px == 0.5 && t.pn.inlier_px == 3.0 && t.pn.min_points == 4 && t.pn.seed == 11 && t.tp.out == POSE);
}

void check_scratch(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    PairOutputs o;
    bind_below(o, ps, true, false, false);
    CHECK(!ps.tr.pc && !ps.tr.pc_cnt);
    const size_t live = g_dev.size();
    reset_log();
    CHECK(bind(o, ps).code == DVO_OK);
    CHECK(g_mallocs == std::vector<size_t>{sh.bytes} && g_frees == 0 && g_syncs == 0 && g_dev.size() == live + 1);
    CHECK(g_dev.count(ps.tr.pc) == 1 && !ps.tr.flink && !ps.tr.bx);  // no other scratch comes with it
    CHECK((const char*)ps.tr.pc_cnt == (const char*)ps.tr.pc + sh.all_slots * 48);  // the counts behind the correspondences
    const PnpCorr* pc = ps.tr.pc;
    // a second binding allocates nothing more
    reset_log();
    (void)o.take();
    bind_below(o, ps, false, true, true);
    CHECK(bind(o, ps).code == DVO_OK && ps.tr.pc == pc);
    for (size_t n : g_mallocs) CHECK(n != sh.bytes);
    // without the track scratch there is nothing to put it beside
    PairSets fresh;
    make_sets(fresh, sh);
    reset_log();
    const BindResult r = o.set_track_pnp(fresh, kDevice, PNP, nullptr, 0, 0, 0, 0, 0, 0, 0);
    CHECK(r.code == DVO_EHIP && r.hip == hipErrorInvalidValue && g_mallocs.empty() && !fresh.tr.pc);
}

// The one allocation fails: the scratch stays empty, nothing leaks, the other bindings are what they
// were and no PnP binding is pending; the same call then succeeds.
void check_failure(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    PairOutputs o;
    bind_below(o, ps, true, true, true);
    const size_t live = g_dev.size();
    reset_log();
    g_fail_at = 0;
    const BindResult r = bind(o, ps);
    CHECK(r.code == DVO_EHIP && r.hip == hipErrorOutOfMemory && r.what && std::strcmp(r.what, "PairSets::ensure_track_pnp") == 0);
    CHECK(g_mallocs == std::vector<size_t>{sh.bytes} && g_dev.size() == live && !ps.tr.pc && !ps.tr.pc_cnt);
    CHECK(empty(o.pn) && o.lm.out == LM_OUT && o.tr.link == LINK && o.tr.scale == SCALE && o.tp.out == POSE);
    CHECK(o.rf.refined == REFINED && o.bd.out == BUNDLE && g_devices == std::vector<int>{kDevice});
    reset_log();
    CHECK(bind(o, ps).code == DVO_OK && g_mallocs == std::vector<size_t>{sh.bytes} && g_dev.size() == live + 1);
    CHECK(o.pn.out == PNP && o.rf.refined == REFINED && o.bd.out == BUNDLE);
}

// ---- the launches of a retiring set -----------------------------------------------------------
void check_launches(const Shape& sh) {
    PairSets ps;
    make_sets(ps, sh);
    GeomArgs g{};
    g.pts_f = PTS;
    g.fx = 700.5, g.fy = 701.5, g.cx = 320.25, g.cy = 240.75;
    g.pts_stride = sh.cap;
    static dvo_dmatch matches[1];
    const TrackIndex caller{&matches->queryIdx, &matches->trainIdx, sh.cap, 4};
    const TrackIndex* idx = sh.own_idx ? nullptr : &caller;
    const size_t tiles = (size_t)landmark_tiles(sh.cap);
    for (int round = 0; round < 2; ++round)  // round 1: every scratch is there whatever the batch binds
        for (int k = 0; k < (sh.own_idx ? 3 : 1); ++k)
            for (int combo = 0; combo < 16; ++combo) {
                const bool poses = combo & 1, refine = combo & 2, bundle = combo & 4, pnp = combo & 8;
                PairOutputs next;
                bind_below(next, ps, poses, refine, bundle);
                if (pnp) CHECK(next.set_track_pnp(ps, kDevice, PNP, MASK, 123, 65, 3, 0.5, 3.0, 7, 99).code == DVO_OK);
                g_tr_calls.clear();
                g_lm_calls = 0;
                CHECK(launch_pair_outputs(next.take(), ps, k, g, 2, REC, idx, STREAM) == hipSuccess);
                CHECK(g_lm_calls == 1 && g_tr_calls.size() == 1);
                const TrackArgs& a = g_tr_calls[0];
                const size_t off = (size_t)k * sh.set_slots;
                CHECK(a.rec == REC && a.link == LINK && a.scale == SCALE && a.cap == 4 && a.pts_stride == sh.cap);
                CHECK((a.pose == POSE) == poses && (a.corr != nullptr) == poses);
                CHECK((a.refined == REFINED) == refine && (a.bd_x != nullptr) == bundle && (a.flink != nullptr) == (refine || bundle));
                if (pnp) {
                    CHECK(a.pnp == PNP && a.pnp_mask == MASK && a.pnp_mask_cap == 123);
                    CHECK(a.pnp_corr == ps.tr.pc + off && a.pnp_cnt == ps.tr.pc_cnt + (size_t)k * F * tiles);
                    CHECK(a.pnp_hyps == 65 && a.pnp_iters == 3 && a.pnp_huber_px == 0.5 && a.pnp_inlier_px == 3.0);
                    CHECK(a.pnp_min_points == 7 && a.pnp_seed == 99);
                    CHECK(a.pts_f == PTS && a.fx == 700.5 && a.fy == 701.5 && a.cx == 320.25 && a.cy == 240.75);
                } else {  // no PnP kernels: the launch takes pnp for "a PnP binding", and its scratch is taken out
                    CHECK(!a.pnp && !a.pnp_mask && !a.pnp_corr && !a.pnp_cnt && a.pnp_mask_cap == 0 && a.pnp_hyps == 0);
                    CHECK(a.pnp_iters == 0 && a.pnp_min_points == 0 && a.pnp_huber_px == 0 && a.pnp_inlier_px == 0 && a.pnp_seed == 0);
                    if (!poses && !refine && !bundle) CHECK(!a.pts_f && a.fx == 0);
                }
            }
    // a links-only tracks binding is enough, and the defaults reach the launch
    PairOutputs next;
    CHECK(next.set_landmarks(ps, kDevice, LM_OUT, LM_CNT, 4).code == DVO_OK);
    CHECK(next.set_tracks(ps, kDevice, LINK, nullptr).code == DVO_OK);
    CHECK(next.set_track_pnp(ps, kDevice, PNP, nullptr, 0, 0, 0, 0, 0, 0, 0).code == DVO_OK);
    g_tr_calls.clear();
    CHECK(launch_pair_outputs(next.take(), ps, 0, g, 2, REC, idx, STREAM) == hipSuccess);
    const TrackArgs& a = g_tr_calls.at(0);
    CHECK(a.pnp == PNP && !a.pnp_mask && a.pnp_mask_cap == 0 && a.link == LINK && !a.scale && !a.pose);
    CHECK(a.pnp_hyps == 128 && a.pnp_iters == 10 && a.pnp_huber_px == 1.0 && a.pnp_inlier_px == 2.0 && a.pnp_min_points == 6);
    CHECK(a.pnp_seed == 0 && a.pnp_corr == ps.tr.pc && a.pnp_cnt == ps.tr.pc_cnt);
}
}  // namespace

int main() {
    check_params();
    check_rules();
    for (const Shape& sh : kShapes) {
        check_scratch(sh);
        check_failure(sh);
        check_launches(sh);
        CHECK(g_dev.empty() && g_pin.empty());
    }
    std::puts("ok");
    return 0;
}
