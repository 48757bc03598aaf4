// Host-side ownership of a stream's pair outputs (api.cpp): the caller's landmark, tracks, pose,
// refine, bundle and PnP bindings of a batch, the rules of setting them, and the one launch of what they ask
// for when the batch's pair set retires.  Both frame streams use it.  Host code only.
#pragma once

#include <cmath>
#include <utility>

#include "device_mem.h"
#include "dvo_internal.h"

namespace dvo {

// The caller's buffers of a landmark binding (dvo_stream_set_landmarks): [pairs][cap] entries, [pairs] counts.
struct LandmarkBinding {
    dvo_landmark* out = nullptr;  // null: no binding
    int32_t* count = nullptr;
    int cap = 0;
};

// The caller's buffers of a tracks binding (dvo_stream_set_tracks), beside a landmark binding.
struct TracksBinding {
    int32_t* link = nullptr;  // [pairs][the landmark binding's cap], or null
    dvo_track_scale* scale = nullptr;  // [pairs], or null; both null: no binding
    explicit operator bool() const { return link || scale; }
};

// The caller's buffer and parameters of a pose binding (dvo_stream_set_track_poses), beside a tracks binding.
struct TrackPoseBinding {
    dvo_track_pose* out = nullptr;  // [pairs]; null: no binding
    int iters = 0, min_points = 0;
    double huber_px = 0, inlier_px = 0;
};

// The parameters of a pose binding with the defaults filled in; false: out of range.
inline bool track_pose_params(TrackPoseBinding& b, int iters, double huber_px, double inlier_px, int min_points) {
    if (std::isnan(huber_px) || std::isnan(inlier_px)) return false;
    b.iters = iters > 0 ? iters : 10;
    b.huber_px = huber_px > 0 ? huber_px : 1.0;
    b.inlier_px = inlier_px > 0 ? inlier_px : 2.0;
    b.min_points = min_points > 0 ? min_points : 6;
    return b.iters <= kTrackPoseMaxIters && b.min_points >= 3;
}

// The caller's buffers and parameters of a refine binding (dvo_stream_set_track_refine), beside a tracks binding.
struct TrackRefineBinding {
    dvo_landmark_refined* refined = nullptr;  // [pairs][the landmark binding's cap], or null
    dvo_track_id* id = nullptr;               // the same, or null; both null: no binding
    int views = 0, iters = 0;
    double huber_px = 0, inlier_px = 0;
    bool use_pose = false;  // a pose binding was pending when this one was made
    explicit operator bool() const { return refined || id; }
};

// The parameters of a refine binding with the defaults filled in; false: out of range.
inline bool track_refine_params(TrackRefineBinding& b, int views, int iters, double huber_px, double inlier_px) {
    if (std::isnan(huber_px) || std::isnan(inlier_px)) return false;
    b.views = views > 0 ? views : 6;
    b.iters = iters > 0 ? iters : 5;
    b.huber_px = huber_px > 0 ? huber_px : 1.0;
    b.inlier_px = inlier_px > 0 ? inlier_px : 2.0;
    return b.views >= 3 && b.views <= kTrackRefineMaxViews && b.iters <= kTrackRefineMaxIters;
}

// The caller's buffers and parameters of a bundle binding (dvo_stream_set_track_bundle), beside a tracks binding.
struct TrackBundleBinding {
    dvo_track_bundle* out = nullptr;         // [pairs], or null
    dvo_landmark_refined* points = nullptr;  // [pairs][the landmark binding's cap], or null; both null: no binding
    int views = 0, iters = 0, min_points = 0;
    double lambda = 0, huber_px = 0, inlier_px = 0;
    bool use_pose = false;  // a pose binding was pending when this one was made
    explicit operator bool() const { return out || points; }
};

// The parameters of a bundle binding with the defaults filled in; false: out of range.
inline bool track_bundle_params(TrackBundleBinding& b, int views, int iters, double lambda, double huber_px,
                                double inlier_px, int min_points) {
    if (std::isnan(lambda) || std::isnan(huber_px) || std::isnan(inlier_px)) return false;
    b.views = views > 0 ? views : 6;
    b.iters = iters > 0 ? iters : 5;
    b.lambda = lambda > 0 ? lambda : DVO_TRACK_BUNDLE_LAMBDA;
    b.huber_px = huber_px > 0 ? huber_px : 1.0;
    b.inlier_px = inlier_px > 0 ? inlier_px : 2.0;
    b.min_points = min_points > 0 ? min_points : 8;
    return b.views >= 2 && b.views <= kTrackRefineMaxViews && b.iters <= kTrackBundleMaxIters && b.min_points >= 6;
}

// The caller's buffers and parameters of a PnP binding (dvo_stream_set_track_pnp), beside a tracks binding.
struct TrackPnpBinding {
    dvo_track_pnp* out = nullptr;  // [pairs]; null: no binding
    uint8_t* mask = nullptr;       // [pairs][mask_cap], or null
    int mask_cap = 0;
    int hyps = 0, iters = 0, min_points = 0;
    double huber_px = 0, inlier_px = 0;
    uint64_t seed = 0;
};

// The parameters of a PnP binding with the defaults filled in; false: out of range.
inline bool track_pnp_params(TrackPnpBinding& b, int hyps, int iters, double huber_px, double inlier_px, int min_points,
                             uint64_t seed) {
    if (std::isnan(huber_px) || std::isnan(inlier_px)) return false;
    b.hyps = hyps > 0 ? hyps : 128;
    b.iters = iters > 0 ? iters : 10;
    b.huber_px = huber_px > 0 ? huber_px : 1.0;
    b.inlier_px = inlier_px > 0 ? inlier_px : 2.0;
    b.min_points = min_points > 0 ? min_points : 6;
    b.seed = seed;
    return b.hyps <= kPnpMaxHyps && b.iters <= kTrackPoseMaxIters && b.min_points >= 4;
}

// What a setter answers.  DVO_OK; DVO_EINVAL and the message; or DVO_EHIP, the call that failed
// and its error.
struct BindResult {
    int code = DVO_OK;
    const char* what = nullptr;
    hipError_t hip = hipSuccess;
};

// The six bindings of one batch: pending in a stream until its next batch takes them, then the
// batch's until its pair set retires.  The setters are the dvo_stream_set_* / dvo_knn_stream_set_*
// entry points after their handle check: a later binding reads an earlier one, so setting an
// earlier one clears the later ones, and each first binding sizes its scratch in `sets` (on
// `device`, which is made current only on the way to an allocation).
struct PairOutputs {
    LandmarkBinding lm;
    TracksBinding tr;
    TrackPoseBinding tp;
    TrackRefineBinding rf;
    TrackBundleBinding bd;
    TrackPnpBinding pn;

    PairOutputs take() { return std::exchange(*this, PairOutputs{}); }

    BindResult set_landmarks(PairSets& sets, int device, dvo_landmark* out, int32_t* count, int cap) {
        if (!out) {
            *this = PairOutputs{};
            return {};
        }
        if (cap < 1 || !count) return {DVO_EINVAL, "landmarks need cap >= 1 and a count buffer"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_landmarks, "PairSets::ensure_landmarks");
        if (r.code == DVO_OK) lm = LandmarkBinding{out, count, cap};
        return r;
    }

    BindResult set_tracks(PairSets& sets, int device, int32_t* link, dvo_track_scale* scale) {
        tp = TrackPoseBinding{};    // a pose binding goes after the tracks binding it reads
        rf = TrackRefineBinding{};  // and a refine binding after both
        bd = TrackBundleBinding{};  // and a bundle binding last
        pn = TrackPnpBinding{};     // a PnP binding reads the tracks binding's table
        if (!link && !scale) {
            tr = TracksBinding{};
            return {};
        }
        if (!lm.out) return {DVO_EINVAL, "tracks go with a pending landmark binding"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_tracks, "PairSets::ensure_tracks");
        if (r.code == DVO_OK) tr = TracksBinding{link, scale};
        return r;
    }

    BindResult set_track_poses(PairSets& sets, int device, dvo_track_pose* pose, int iters, double huber_px,
                               double inlier_px, int min_points) {
        rf = TrackRefineBinding{};  // a refine binding goes after the pose binding it may read
        bd = TrackBundleBinding{};  // and so does a bundle binding
        if (!pose) {
            tp = TrackPoseBinding{};
            return {};
        }
        if (!lm.out || !tr.scale)
            return {DVO_EINVAL, "track poses go with a pending tracks binding that has a scale buffer"};
        TrackPoseBinding b;
        if (!track_pose_params(b, iters, huber_px, inlier_px, min_points))
            return {DVO_EINVAL, "track poses: iters <= 32, min_points >= 3, no NaN"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_track_poses, "PairSets::ensure_track_poses");
        b.out = pose;
        if (r.code == DVO_OK) tp = b;
        return r;
    }

    BindResult set_track_refine(PairSets& sets, int device, dvo_landmark_refined* refined, dvo_track_id* id, int views,
                                int iters, double huber_px, double inlier_px) {
        bd = TrackBundleBinding{};  // a bundle binding goes last
        if (!refined && !id) {
            rf = TrackRefineBinding{};
            return {};
        }
        if (!lm.out || !tr.link || !tr.scale)
            return {DVO_EINVAL, "track refine goes with a pending tracks binding that has link and scale buffers"};
        TrackRefineBinding b;
        if (!track_refine_params(b, views, iters, huber_px, inlier_px))
            return {DVO_EINVAL, "track refine: views 3..8, iters <= 16, no NaN"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_track_refine, "PairSets::ensure_track_refine");
        b.refined = refined;
        b.id = id;
        b.use_pose = tp.out != nullptr;
        if (r.code == DVO_OK) rf = b;
        return r;
    }

    BindResult set_track_bundle(PairSets& sets, int device, dvo_track_bundle* bundle, dvo_landmark_refined* points,
                                int views, int iters, double lambda, double huber_px, double inlier_px, int min_points) {
        if (!bundle && !points) {
            bd = TrackBundleBinding{};
            return {};
        }
        if (!lm.out || !tr.link || !tr.scale)
            return {DVO_EINVAL, "track bundle goes with a pending tracks binding that has link and scale buffers"};
        TrackBundleBinding b;
        if (!track_bundle_params(b, views, iters, lambda, huber_px, inlier_px, min_points))
            return {DVO_EINVAL, "track bundle: views 2..8, iters <= 16, min_points >= 6, no NaN"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_track_bundle, "PairSets::ensure_track_bundle");
        b.out = bundle;
        b.points = points;
        b.use_pose = tp.out != nullptr;
        if (r.code == DVO_OK) bd = b;
        return r;
    }

    // Reads the table of a pending tracks binding only, so the pose, refine and bundle setters leave
    // it alone, and it clears nothing.
    BindResult set_track_pnp(PairSets& sets, int device, dvo_track_pnp* pnp, uint8_t* mask, int mask_cap, int hyps,
                             int iters, double huber_px, double inlier_px, int min_points, uint64_t seed) {
        if (!pnp) {
            pn = TrackPnpBinding{};
            return {};
        }
        if (!lm.out || !tr) return {DVO_EINVAL, "track pnp goes with a pending tracks binding"};
        TrackPnpBinding b;
        if (!track_pnp_params(b, hyps, iters, huber_px, inlier_px, min_points, seed) || (mask && mask_cap < 1))
            return {DVO_EINVAL, "track pnp: hyps <= 512, iters <= 32, min_points >= 4, mask_cap >= 1 with a mask, no NaN"};
        const BindResult r = scratch(sets, device, &PairSets::ensure_track_pnp, "PairSets::ensure_track_pnp");
        b.out = pnp;
        b.mask = mask;
        b.mask_cap = mask ? mask_cap : 0;
        if (r.code == DVO_OK) pn = b;
        return r;
    }

    // The caller's side of a retiring set's TrackArgs, over the scratch side (PairSets::track_args,
    // or a test hook's own): the records, the buffers, the parameters, and for a pose or refine
    // binding the points and camera of the set's GeomArgs.  The kernels take corr, id / refined and
    // bd_x for "a pose binding", "a refine binding" and "a bundle binding", so the scratch of an
    // absent binding is taken out; the full links stay where either of the last two is there.
    void fill(TrackArgs& a, const GeomArgs& g, const dvo_pair_record* rec) const {
        a.rec = rec;
        a.link = tr.link;
        a.cap = lm.cap;
        a.scale = tr.scale;
        if (tp.out || rf || bd || pn.out) {
            a.pts_f = g.pts_f;
            a.fx = g.fx, a.fy = g.fy, a.cx = g.cx, a.cy = g.cy;
        }
        if (tp.out) {
            a.pose = tp.out;
            a.pose_iters = tp.iters;
            a.pose_min_points = tp.min_points;
            a.huber_px = tp.huber_px;
            a.inlier_px = tp.inlier_px;
        } else {
            a.corr = nullptr;
        }
        if (rf) {
            a.id = rf.id;
            a.refined = rf.refined;
            a.rf_views = rf.views;
            a.rf_iters = rf.iters;
            a.rf_use_pose = rf.use_pose ? 1 : 0;
            a.rf_huber_px = rf.huber_px;
            a.rf_inlier_px = rf.inlier_px;
        } else {
            if (!bd) a.flink = nullptr;
            a.rank = nullptr;
            a.rank_stride = 0;
        }
        if (bd) {
            a.bundle = bd.out;
            a.bd_points = bd.points;
            a.bd_views = bd.views;
            a.bd_iters = bd.iters;
            a.bd_min_points = bd.min_points;
            a.bd_use_pose = bd.use_pose ? 1 : 0;
            a.bd_lambda = bd.lambda;
            a.bd_huber_px = bd.huber_px;
            a.bd_inlier_px = bd.inlier_px;
        } else {
            a.bd_x = nullptr;
        }
        if (pn.out) {
            a.pnp = pn.out;
            a.pnp_mask = pn.mask;
            a.pnp_mask_cap = pn.mask_cap;
            a.pnp_hyps = pn.hyps;
            a.pnp_iters = pn.iters;
            a.pnp_min_points = pn.min_points;
            a.pnp_huber_px = pn.huber_px;
            a.pnp_inlier_px = pn.inlier_px;
            a.pnp_seed = pn.seed;
        } else {
            a.pnp_corr = nullptr;
            a.pnp_cnt = nullptr;
        }
    }

  private:
    static BindResult scratch(PairSets& sets, int device, hipError_t (PairSets::*ensure)(), const char* what) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return {DVO_EHIP, "hipSetDevice", e};
        e = (sets.*ensure)();  // the first binding sizes the scratch
        return e == hipSuccess ? BindResult{} : BindResult{DVO_EHIP, what, e};
    }
};

// Where the track kernels find a batch's match indices when the set keeps no copy of its own: the
// caller-side arrays, match i of pair p at mq / mt [(p * stride + i) * step].
struct TrackIndex {
    const int32_t *mq, *mt;
    int64_t stride;
    int step;
};

// What the bindings `o` of a batch ask for when its pair set k retires, after the records are
// final (a landmark pair is one whose record got through): the landmarks, and with a tracks
// binding the tracks on the lists the landmark kernels just left.  idx: null for the set's own
// index copy (PairSets::shape own_idx).
inline hipError_t launch_pair_outputs(const PairOutputs& o, const PairSets& sets, int k, const GeomArgs& g_set, int pairs,
                                      const dvo_pair_record* rec, const TrackIndex* idx, hipStream_t s) {
    if (!o.lm.out) return hipSuccess;
    const hipError_t e = launch_landmarks(g_set, pairs, rec, sets.lm, o.lm.out, o.lm.count, o.lm.cap, s);
    if (e != hipSuccess || !o.tr) return e;
    TrackArgs a = sets.track_args(k);
    if (idx) a.mq = idx->mq, a.mt = idx->mt, a.idx_stride = idx->stride, a.idx_step = idx->step;
    o.fill(a, g_set, rec);
    return launch_tracks(a, pairs, s);
}

}  // namespace dvo
