"""Batched frame stream on the GPU: the whole per-pair path of
VisualOdometry.visual_odometry_calculations (visual_odometry_v3.py:384-408) for
many device-resident frames per call.

A call with n frames runs ORB on every frame once, matches each consecutive
pair, runs findEssentialMat(RANSAC) + recoverPose per pair and writes n-1
256-byte pair records (PAIR_RECORD_DTYPE) to device memory.  Torch tensors are
only containers for device memory; all compute is in libdvo_hip.so.

KnnFrameStream is the same for the k-NN modes 'knn_sift', 'surf' and 'flann' (SIFT / SURF,
BFMatcher(NORM_L1).knnMatch(k=2), the ratio test): dvo_knn_stream_process.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes

import numpy as np
import torch

from ._native import (DMATCH_DTYPE, KEYPOINT_DTYPE, LANDMARK_DTYPE, LANDMARK_REFINED_DTYPE, PAIR_RECORD_DTYPE,
                      TRACK_BUNDLE_DTYPE, TRACK_ID_DTYPE, TRACK_PNP_DTYPE, TRACK_POSE_DTYPE, TRACK_SCALE_DTYPE, Context, StreamConfig, _vp, orb_params, ptr)


class Landmarks:
    """Device buffers for one batch's landmarks (dvo_stream_set_landmarks): each pair's matches
    that are inliers of its E and pass recoverPose's tests, with their triangulated positions in
    the previous frame's camera coordinates, in units of the baseline (see include/dvo.h).
    entries: uint8 [n_pairs, cap, 48] (LANDMARK_DTYPE); counts: int32 [n_pairs], the full number
    per pair (above cap: the pair overflowed and holds its first cap), 0 for a failed pair.  Bind
    it with FrameStream.bind_landmarks / KnnFrameStream.bind_landmarks before the batch's call and
    read it after the batch has retired and the stream is synchronised."""

    def __init__(self, n_pairs: int, cap: int, device):
        if n_pairs < 1 or cap < 1:
            raise ValueError("Landmarks needs n_pairs >= 1 and cap >= 1")
        self.n_pairs, self.cap = int(n_pairs), int(cap)
        self.entries = torch.zeros((self.n_pairs, self.cap, LANDMARK_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.counts = torch.zeros(self.n_pairs, dtype=torch.int32, device=device)

    def count(self, pair: int) -> int:
        return int(self.counts[pair].item())

    def numpy(self, pair: int) -> np.ndarray:
        """The pair's first min(count, cap) landmarks (LANDMARK_DTYPE), in ascending match index."""
        n = min(self.count(pair), self.cap)
        return self.entries[pair, :n].cpu().numpy().reshape(-1).view(LANDMARK_DTYPE).copy()


def _bind_landmarks(stream, setter, lm):
    """The one-shot binding of both stream classes; returns what to keep referenced."""
    if lm is None:
        stream.ctx.check(setter(stream.h, None, None, 0))
        return None
    if not isinstance(lm, Landmarks) or lm.entries.device != stream.device or lm.counts.device != stream.device:
        raise ValueError("bind_landmarks takes a Landmarks on the stream's device (or None)")
    stream._after_torch()  # the buffers' fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, lm.entries.data_ptr(), lm.counts.data_ptr(), lm.cap))
    return lm


class Tracks:
    """Device buffers for one batch's tracks (dvo_stream_set_tracks), the companion of a Landmarks
    with the same cap: per landmark slot the ordinal of the same scene point among the previous
    pair's landmarks, and per pair the ratio of its baseline to the previous pair's from the
    shared points (see include/dvo.h).  links: int32 [n_pairs, cap], written for the slots the
    Landmarks holds, -1 where the point has no predecessor; a link can be >= cap when the previous
    pair overflowed.  scales: uint8 [n_pairs, 32] (TRACK_SCALE_DTYPE).  Bind it with bind_tracks
    after bind_landmarks; read it after the batch has retired and the stream is synchronised."""

    def __init__(self, n_pairs: int, cap: int, device):
        if n_pairs < 1 or cap < 1:
            raise ValueError("Tracks needs n_pairs >= 1 and cap >= 1")
        self.n_pairs, self.cap = int(n_pairs), int(cap)
        self.links = torch.full((self.n_pairs, self.cap), -1, dtype=torch.int32, device=device)
        self.scales = torch.zeros((self.n_pairs, TRACK_SCALE_DTYPE.itemsize), dtype=torch.uint8, device=device)

    def numpy(self, pair: int, count: int) -> np.ndarray:
        """The links of the pair's first min(count, cap) landmarks (count: Landmarks.count(pair))."""
        return self.links[pair, :min(int(count), self.cap)].cpu().numpy().copy()

    def scales_numpy(self) -> np.ndarray:
        """TRACK_SCALE_DTYPE [n_pairs]: ratio, q1, q3, n_common, n_prev per pair."""
        return self.scales.cpu().numpy().reshape(-1).view(TRACK_SCALE_DTYPE).copy()


def _bind_tracks(stream, setter, tr):
    """The one-shot tracks binding of both stream classes; returns what to keep referenced."""
    if tr is None:
        stream.ctx.check(setter(stream.h, None, None))
        return None
    lm = stream._lm_next
    if lm is None:
        raise ValueError("bind_tracks goes after bind_landmarks: tracks are a companion of a pending Landmarks")
    if not isinstance(tr, Tracks) or tr.links.device != stream.device or tr.scales.device != stream.device:
        raise ValueError("bind_tracks takes a Tracks on the stream's device (or None)")
    if tr.cap != lm.cap or tr.n_pairs < lm.n_pairs:
        raise ValueError(f"the Tracks ({tr.n_pairs} pairs, cap {tr.cap}) must have the bound Landmarks' cap and "
                         f"pairs ({lm.n_pairs}, cap {lm.cap})")
    stream._after_torch()  # the buffers' fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, tr.links.data_ptr(), tr.scales.data_ptr()))
    return tr


class TrackPoses:
    """Device buffer for one batch's track poses (dvo_stream_set_track_poses), the companion of a
    Tracks: per pair the pose of its second camera refined on the previous pair's landmarks, whose
    translation length `scale` is the baseline ratio without the error of the pair's own t
    direction (see include/dvo.h).  poses: uint8 [n_pairs, 128] (TRACK_POSE_DTYPE).  Bind it with
    bind_track_poses after bind_tracks; read it after the batch has retired and the stream is
    synchronised."""

    def __init__(self, n_pairs: int, device):
        if n_pairs < 1:
            raise ValueError("TrackPoses needs n_pairs >= 1")
        self.n_pairs = int(n_pairs)
        self.poses = torch.zeros((self.n_pairs, TRACK_POSE_DTYPE.itemsize), dtype=torch.uint8, device=device)

    def numpy(self) -> np.ndarray:
        """TRACK_POSE_DTYPE [n_pairs]: R, t, scale, rms, n_used, n_inliers, iters, status per pair."""
        return self.poses.cpu().numpy().reshape(-1).view(TRACK_POSE_DTYPE).copy()


class RefinedLandmarks:
    """Device buffers for one batch's track ids and refined landmarks (dvo_stream_set_track_refine),
    the companion of a Tracks, slot for slot beside the Landmarks of the same cap: per landmark the
    root and age of its track, and its position re-estimated from up to `views` most recent frames
    of the track (see include/dvo.h).  refined: uint8 [n_pairs, cap, 56] (LANDMARK_REFINED_DTYPE);
    ids: uint8 [n_pairs, cap, 16] (TRACK_ID_DTYPE).  Bind it with bind_refine after bind_tracks (and
    after bind_track_poses, where the poses are to feed it); read it after the batch has retired
    and the stream is synchronised."""

    def __init__(self, n_pairs: int, cap: int, device):
        if n_pairs < 1 or cap < 1:
            raise ValueError("RefinedLandmarks needs n_pairs >= 1 and cap >= 1")
        self.n_pairs, self.cap = int(n_pairs), int(cap)
        self.refined = torch.zeros((self.n_pairs, self.cap, LANDMARK_REFINED_DTYPE.itemsize), dtype=torch.uint8,
                                   device=device)
        self.ids = torch.zeros((self.n_pairs, self.cap, TRACK_ID_DTYPE.itemsize), dtype=torch.uint8, device=device)

    def numpy(self, pair: int, count: int) -> np.ndarray:
        """The pair's first min(count, cap) refined landmarks (count: Landmarks.count(pair))."""
        n = min(int(count), self.cap)
        return self.refined[pair, :n].cpu().numpy().reshape(-1).view(LANDMARK_REFINED_DTYPE).copy()

    def ids_numpy(self, pair: int, count: int) -> np.ndarray:
        """The track ids of the pair's first min(count, cap) landmarks."""
        n = min(int(count), self.cap)
        return self.ids[pair, :n].cpu().numpy().reshape(-1).view(TRACK_ID_DTYPE).copy()


def _bind_refine(stream, setter, rf, views, iters, huber_px, inlier_px, ids, refined):
    """The one-shot refine binding of both stream classes; returns what to keep referenced."""
    if rf is None or not (ids or refined):
        stream.ctx.check(setter(stream.h, None, None, 0, 0, 0.0, 0.0))
        return None
    lm, tr = stream._lm_next, stream._tr_next
    if lm is None or tr is None:
        raise ValueError("bind_refine goes after bind_tracks: it is a companion of a pending Tracks")
    if not isinstance(rf, RefinedLandmarks) or rf.refined.device != stream.device or rf.ids.device != stream.device:
        raise ValueError("bind_refine takes a RefinedLandmarks on the stream's device (or None)")
    if rf.cap != lm.cap or rf.n_pairs < lm.n_pairs:
        raise ValueError(f"the RefinedLandmarks ({rf.n_pairs} pairs, cap {rf.cap}) must have the bound Landmarks' cap "
                         f"and pairs ({lm.n_pairs}, cap {lm.cap})")
    stream._after_torch()  # the buffers' fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, rf.refined.data_ptr() if refined else None, rf.ids.data_ptr() if ids else None,
                            int(views), int(iters), float(huber_px), float(inlier_px)))
    return rf


class TrackBundle:
    """Device buffers for one batch's track bundle (dvo_stream_set_track_bundle), the companion of a
    Tracks: per pair the pose, baseline ratio and costs of the joint fit of its window cameras and
    landmarks, and slot for slot beside the Landmarks of the same cap each landmark's fitted
    position (see include/dvo.h).  bundle: uint8 [n_pairs, 160] (TRACK_BUNDLE_DTYPE); points: uint8
    [n_pairs, cap, 56] (LANDMARK_REFINED_DTYPE).  Bind it with bind_bundle, last; read it after the
    batch has retired and the stream is synchronised."""

    def __init__(self, n_pairs: int, cap: int, device):
        if n_pairs < 1 or cap < 1:
            raise ValueError("TrackBundle needs n_pairs >= 1 and cap >= 1")
        self.n_pairs, self.cap = int(n_pairs), int(cap)
        self.bundle = torch.zeros((self.n_pairs, TRACK_BUNDLE_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.points = torch.zeros((self.n_pairs, self.cap, LANDMARK_REFINED_DTYPE.itemsize), dtype=torch.uint8,
                                  device=device)

    def numpy(self) -> np.ndarray:
        """TRACK_BUNDLE_DTYPE [n_pairs]: R, t, ratio, cost0, cost, rms0, rms and the counts per pair."""
        return self.bundle.cpu().numpy().reshape(-1).view(TRACK_BUNDLE_DTYPE).copy()

    def points_numpy(self, pair: int, count: int) -> np.ndarray:
        """The pair's first min(count, cap) fitted landmarks (count: Landmarks.count(pair))."""
        n = min(int(count), self.cap)
        return self.points[pair, :n].cpu().numpy().reshape(-1).view(LANDMARK_REFINED_DTYPE).copy()


def _bind_bundle(stream, setter, bd, views, iters, lam, huber_px, inlier_px, min_points, pairs, points):
    """The one-shot bundle binding of both stream classes; returns what to keep referenced."""
    if bd is None or not (pairs or points):
        stream.ctx.check(setter(stream.h, None, None, 0, 0, 0.0, 0.0, 0.0, 0))
        return None
    lm, tr = stream._lm_next, stream._tr_next
    if lm is None or tr is None:
        raise ValueError("bind_bundle goes after bind_tracks: it is a companion of a pending Tracks")
    if not isinstance(bd, TrackBundle) or bd.bundle.device != stream.device or bd.points.device != stream.device:
        raise ValueError("bind_bundle takes a TrackBundle on the stream's device (or None)")
    if bd.cap != lm.cap or bd.n_pairs < lm.n_pairs:
        raise ValueError(f"the TrackBundle ({bd.n_pairs} pairs, cap {bd.cap}) must have the bound Landmarks' cap "
                         f"and pairs ({lm.n_pairs}, cap {lm.cap})")
    stream._after_torch()  # the buffers' fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, bd.bundle.data_ptr() if pairs else None, bd.points.data_ptr() if points else None,
                            int(views), int(iters), float(lam), float(huber_px), float(inlier_px), int(min_points)))
    return bd


def _bind_track_poses(stream, setter, tp, iters, huber_px, inlier_px, min_points):
    """The one-shot pose binding of both stream classes; returns what to keep referenced."""
    if tp is None:
        stream.ctx.check(setter(stream.h, None, 0, 0.0, 0.0, 0))
        return None
    tr = stream._tr_next
    if tr is None:
        raise ValueError("bind_track_poses goes after bind_tracks: poses are a companion of a pending Tracks")
    if not isinstance(tp, TrackPoses) or tp.poses.device != stream.device:
        raise ValueError("bind_track_poses takes a TrackPoses on the stream's device (or None)")
    if tp.n_pairs < tr.n_pairs:
        raise ValueError(f"the TrackPoses ({tp.n_pairs} pairs) must have the bound Tracks' pairs ({tr.n_pairs})")
    stream._after_torch()  # the buffer's fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, tp.poses.data_ptr(), int(iters), float(huber_px), float(inlier_px),
                            int(min_points)))
    return tp


class TrackPnP:
    """Device buffers for one batch's track PnP (dvo_stream_set_track_pnp), the companion of a Tracks:
    per pair the pose of its second camera from a P3P RANSAC on the previous pair's landmarks and
    the pair's raw matches, which needs neither the pair's own essential matrix nor its landmarks
    (see include/dvo.h).  pnp: uint8 [n_pairs, 144] (TRACK_PNP_DTYPE); mask: uint8 [n_pairs, mask_cap]
    per match 1 for a final inlier (mask_cap 0: none).  Bind it with bind_pnp after bind_tracks;
    read it after the batch has retired and the stream is synchronised."""

    def __init__(self, n_pairs: int, device, mask_cap: int = 0):
        if n_pairs < 1 or mask_cap < 0:
            raise ValueError("TrackPnP needs n_pairs >= 1 and mask_cap >= 0")
        self.n_pairs, self.mask_cap = int(n_pairs), int(mask_cap)
        self.pnp = torch.zeros((self.n_pairs, TRACK_PNP_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.mask = torch.zeros((self.n_pairs, self.mask_cap), dtype=torch.uint8, device=device) if mask_cap else None

    def numpy(self) -> np.ndarray:
        """TRACK_PNP_DTYPE [n_pairs]: R, t, scale, rms, the counts, sample, solution, iters, status per pair."""
        return self.pnp.cpu().numpy().reshape(-1).view(TRACK_PNP_DTYPE).copy()

    def mask_numpy(self) -> np.ndarray:
        """uint8 [n_pairs, mask_cap]."""
        return self.mask.cpu().numpy().copy()

    def tensors(self):
        return (self.pnp,) + (() if self.mask is None else (self.mask,))


def _bind_pnp(stream, setter, pn, hyps, iters, huber_px, inlier_px, min_points, seed):
    """The one-shot PnP binding of both stream classes; returns what to keep referenced."""
    if pn is None:
        stream.ctx.check(setter(stream.h, None, None, 0, 0, 0, 0.0, 0.0, 0, 0))
        return None
    tr = stream._tr_next
    if tr is None:
        raise ValueError("bind_pnp goes after bind_tracks: it is a companion of a pending Tracks")
    if not isinstance(pn, TrackPnP) or pn.pnp.device != stream.device:
        raise ValueError("bind_pnp takes a TrackPnP on the stream's device (or None)")
    if pn.n_pairs < tr.n_pairs:
        raise ValueError(f"the TrackPnP ({pn.n_pairs} pairs) must have the bound Tracks' pairs ({tr.n_pairs})")
    stream._after_torch()  # the buffers' fill ran on torch's stream: order the library's writes after it
    stream.ctx.check(setter(stream.h, pn.pnp.data_ptr(), None if pn.mask is None else pn.mask.data_ptr(), pn.mask_cap,
                            int(hyps), int(iters), float(huber_px), float(inlier_px), int(min_points), int(seed)))
    return pn


def carry_scale(anchor, scales, poses=None, bundle=None, pnp=None) -> np.ndarray:
    """Metric baseline length per pair of one batch: anchor float64 [pairs] holds the marker's scale
    where a marker was seen (the pose tail) and NaN elsewhere; scales is the batch's
    TRACK_SCALE_DTYPE [pairs] (Tracks.scales_numpy).  out[p] = anchor[p] where that is not NaN, else
    out[p - 1] * ratio[p] when n_common[p] >= 1 and out[p - 1] is not NaN, else NaN.  No threshold
    of its own: filter on n_common, q1 and q3 first (set n_common to 0 where the ratio is not trusted).
    poses: the batch's TRACK_POSE_DTYPE [pairs] (TrackPoses.numpy), or None: a pair whose pose has
    status 0 multiplies by poses["scale"][p] instead of the ratio.  bundle: the batch's
    TRACK_BUNDLE_DTYPE [pairs] (TrackBundle.numpy), or None: a pair whose bundle has status 0 and a
    ratio > 0 multiplies by bundle["ratio"][p] instead of either.  pnp: the batch's TRACK_PNP_DTYPE
    [pairs] (TrackPnP.numpy), or None: where all of that leaves out[p] NaN, out[p - 1] is not NaN
    and pnp["status"][p] == 0, out[p] = out[p - 1] * pnp["scale"][p] (a pair whose own essential
    matrix failed has n_common 0 but may still have a PnP pose)."""
    anchor = np.asarray(anchor, np.float64)
    if (anchor.ndim != 1 or len(scales) != len(anchor) or (poses is not None and len(poses) != len(anchor))
            or (bundle is not None and len(bundle) != len(anchor)) or (pnp is not None and len(pnp) != len(anchor))):
        raise ValueError("anchor float64 [pairs], scales [pairs], poses [pairs], bundle [pairs] and pnp [pairs] must agree")
    out = np.full(len(anchor), np.nan)
    for p in range(len(anchor)):
        if not np.isnan(anchor[p]):
            out[p] = anchor[p]
        elif p >= 1 and scales["n_common"][p] >= 1 and not np.isnan(out[p - 1]):
            refined = poses is not None and poses["status"][p] == 0
            if bundle is not None and bundle["status"][p] == 0 and bundle["ratio"][p] > 0:
                out[p] = out[p - 1] * bundle["ratio"][p]
            else:
                out[p] = out[p - 1] * (poses["scale"][p] if refined else scales["ratio"][p])
        if (pnp is not None and np.isnan(out[p]) and p >= 1 and not np.isnan(out[p - 1]) and pnp["status"][p] == 0):
            out[p] = out[p - 1] * pnp["scale"][p]
    return out


class FrameStream:
    def __init__(self, width: int, height: int, K, nfeatures: int = 500, max_frames: int = 64, prob: float = 0.999,
                 threshold: float = 1.0, max_iters: int = 1000, cross_check: int | None = None,
                 dist_thresh: float = 50.0, device: int | None = None, ctx: Context | None = None, opencv="4.x",
                 ratio: float | None = None):
        """opencv: the OpenCV version whose semantics the path reproduces, "4.x"
        (default) or "3.2" (ORB pyramid / retainBest, and cross_check defaults
        to the 3.x reverse pass); see include/dvo.h DVO_OPENCV_*.
        ratio: None / 0 (default) matches with cross_check; a ratio > 0 matches with
        knnMatch(k = 2) and Lowe's ratio test instead (set_ratio_test)."""
        from ._native import opencv_semantics
        sem = opencv_semantics(opencv)
        if cross_check is None:
            cross_check = 2 if sem == 1 else 1
        if ctx is not None and device is not None and device != ctx.device:
            raise ValueError(f"device {device} != context device {ctx.device}")
        self.ctx = ctx if ctx is not None else Context(0 if device is None else device)
        self.device = torch.device("cuda", self.ctx.device)  # the library runs on the context's device
        cfg = StreamConfig()
        cfg.width, cfg.height, cfg.max_frames = int(width), int(height), int(max_frames)
        cfg.orb = orb_params(nfeatures=nfeatures, opencv=opencv)
        K = np.asarray(K, np.float64).reshape(9)
        for i in range(9):
            cfg.K[i] = float(K[i])
        cfg.prob, cfg.threshold, cfg.max_iters = float(prob), float(threshold), int(max_iters)
        cfg.cross_check, cfg.dist_thresh = int(cross_check), float(dist_thresh)
        h = _vp()
        self.ctx.check(self.ctx.lib.dvo_stream_create(self.ctx.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self._ext = torch.cuda.ExternalStream(self.hip_stream, device=self.device)
        self._held = collections.deque()  # (event, tensors) in flight on the library's stream
        # The last process() call's frames and records: the library keeps raw pointers to both
        # (dvo_stream_pose_tail reads the records, get_pyramid(blurred) re-reads level 0 of the
        # frames), so they stay referenced until the next process() or close(), whatever the
        # caller keeps and whether or not sync() has drained _held.
        self._last = ()
        self._pending = {}  # records of submitted, not yet retired batches (by device address)
        self._lm_next = None  # bind_landmarks: the Landmarks the next batch takes
        self._lm_pending = {}  # Landmarks of batches not yet retired, by their records' device address
        self._tr_next = None  # bind_tracks: the Tracks the next batch takes with its Landmarks
        self._tp_next = None  # bind_track_poses: the TrackPoses it takes with them
        self._rf_next = None  # bind_refine: and the RefinedLandmarks
        self._bd_next = None  # bind_bundle: and the TrackBundle
        self._pn_next = None  # bind_pnp: and the TrackPnP
        self.width, self.height, self.max_frames, self.nfeatures = width, height, max_frames, nfeatures
        self.K = K.reshape(3, 3)
        if ratio:
            self.set_ratio_test(ratio)

    @property
    def hip_stream(self) -> int:
        return self.ctx.lib.dvo_stream_hip_stream(self.h) or 0

    def set_ratio_test(self, ratio: float | None):
        """Match every later batch with the Hamming 2-NN and the reference's k-NN filter
        `m.distance < ratio * n.distance` (v3:223-228) instead of the cross check: kept matches in
        ascending queryIdx, n_matches their count, DVO_ENOFEAT for a pair whose current frame has
        fewer than 2 descriptors.  None / 0: back to cross_check.  Refused (DVOError) while
        submitted batches are pending, and for a negative or non-finite ratio."""
        self.ctx.check(self.ctx.lib.dvo_stream_set_ratio_test(self.h, float(0.0 if ratio is None else ratio)))

    def new_records(self, n_pairs: int) -> torch.Tensor:
        return torch.zeros(max(n_pairs, 1) * PAIR_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=self.device)

    def bind_landmarks(self, lm: Landmarks | None):
        """Have the next batch (the next process / process_pairs / submit / submit_pairs call, colour,
        undistorted and JPEG frames included) write its landmarks into `lm` when it retires
        (dvo_stream_set_landmarks); lm needs a row per pair of that batch.  One-shot: the batch
        after it writes nothing.  None clears a binding no batch has taken yet."""
        self._lm_next = _bind_landmarks(self, self.ctx.lib.dvo_stream_set_landmarks, lm)
        if lm is None:
            self._tr_next = self._tp_next = self._rf_next = self._bd_next = self._pn_next = None  # the library clears the companions with it

    def bind_tracks(self, tr: Tracks | None):
        """Have the next batch also write its tracks into `tr` (dvo_stream_set_tracks), after its
        landmarks.  Call it after bind_landmarks (ValueError otherwise), with a Tracks of the
        same cap.  One-shot, like the landmark binding; None clears a pending binding.  Only for
        batches of consecutive frames: process_pairs / submit_pairs raise ValueError."""
        self._tr_next = _bind_tracks(self, self.ctx.lib.dvo_stream_set_tracks, tr)
        self._tp_next = self._rf_next = self._bd_next = self._pn_next = None  # the library's call cleared the later pending bindings

    def bind_track_poses(self, tp: TrackPoses | None, iters: int = 10, huber_px: float = 1.0, inlier_px: float = 2.0,
                         min_points: int = 6):
        """Have the next batch also write its track poses into `tp` (dvo_stream_set_track_poses),
        after its tracks.  Call it after bind_tracks (ValueError otherwise).  iters: Gauss-Newton
        steps (at most 32); huber_px, inlier_px: the Huber width and the inlier bound in pixels;
        min_points: shared landmarks a pair needs (at least 3).  One-shot; None clears a pending
        binding, as bind_tracks and bind_landmarks(None) do."""
        self._rf_next = self._bd_next = None  # the library's call clears pending refine and bundle bindings
        self._tp_next = _bind_track_poses(self, self.ctx.lib.dvo_stream_set_track_poses, tp, iters, huber_px,
                                          inlier_px, min_points)

    def bind_refine(self, rf: RefinedLandmarks | None, views: int = 6, iters: int = 5, huber_px: float = 1.0,
                    inlier_px: float = 2.0, ids: bool = True, refined: bool = True):
        """Have the next batch also write its track ids and refined landmarks into `rf`
        (dvo_stream_set_track_refine), after its tracks and track poses.  Call it last: after
        bind_tracks (ValueError otherwise) and after bind_track_poses where the refined poses are
        to feed the fit.  views: frames of a track a landmark is fitted to (3..8); iters:
        Gauss-Newton steps (at most 16); huber_px, inlier_px as for the poses; ids / refined:
        which of the two outputs to write.  One-shot; None clears a pending binding."""
        self._bd_next = None  # the library's call clears a pending bundle binding: bind the bundle last
        self._rf_next = _bind_refine(self, self.ctx.lib.dvo_stream_set_track_refine, rf, views, iters, huber_px,
                                     inlier_px, ids, refined)

    def bind_bundle(self, bd: TrackBundle | None, views: int = 6, iters: int = 5, lam: float = 0.0, huber_px: float = 1.0,
                    inlier_px: float = 2.0, min_points: int = 8, pairs: bool = True, points: bool = True):
        """Have the next batch also write its track bundle into `bd` (dvo_stream_set_track_bundle),
        after everything else.  Call it last: after bind_tracks (ValueError otherwise), after
        bind_track_poses where the refined poses are to start the fit, and after bind_refine where
        that is bound too (it is not needed).  views: cameras of a pair's window (2..8); iters:
        Gauss-Newton steps (at most 16); lam: the damping (0: the library's default); huber_px,
        inlier_px as for the poses; min_points: landmarks a pair needs (at least 6); pairs / points:
        which of the two outputs to write.  One-shot; None clears a pending binding."""
        self._bd_next = _bind_bundle(self, self.ctx.lib.dvo_stream_set_track_bundle, bd, views, iters, lam, huber_px,
                                     inlier_px, min_points, pairs, points)

    def bind_pnp(self, pn: TrackPnP | None, hyps: int = 128, iters: int = 10, huber_px: float = 1.0,
                 inlier_px: float = 2.0, min_points: int = 6, seed: int = 0):
        """Have the next batch also write its track PnP into `pn` (dvo_stream_set_track_pnp), after
        everything else.  Call it after bind_tracks (ValueError otherwise); the pose, refine and
        bundle bindings neither need nor clear it.  hyps: P3P samples per pair (at most 512); iters:
        polish steps (at most 32); huber_px, inlier_px as for the poses; min_points: correspondences
        and supporters a pair needs (at least 4); seed: of the samples (0: the E-RANSAC's).
        One-shot; None clears a pending binding, as bind_tracks and bind_landmarks(None) do."""
        self._pn_next = _bind_pnp(self, self.ctx.lib.dvo_stream_set_track_pnp, pn, hyps, iters, huber_px, inlier_px,
                                  min_points, seed)

    def _lm_fits(self, pairs: int, shared: bool = True):
        if self._lm_next is not None and self._lm_next.n_pairs < pairs:
            raise ValueError(f"the bound Landmarks holds {self._lm_next.n_pairs} pairs, the batch has {pairs}")
        if self._tr_next is not None and not shared:
            raise ValueError("tracks link consecutive pairs: the pairs of process_pairs / submit_pairs share no frame")

    def process(self, frames: torch.Tensor, records: torch.Tensor | None = None, wait_torch: bool = True,
                undistort=None) -> torch.Tensor:
        """Enqueue the batch on the stream's HIP stream (asynchronous).  With
        wait_torch the batch is ordered after work queued on torch's current
        stream (the frames' producer); pass False for frames already resident.
        Colour frames (uint8 [n, H, W, C], C = 3 or 4: B, G, R first) are converted
        to gray, and undistorted if asked, on the way into the stream's slab."""
        if frames.dim() == 4:
            return self._process_bgr(frames, records, wait_torch, undistort)
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [n, H, W] device tensor")
        n, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != stream {self.width}x{self.height}")
        if frames.stride(2) != 1 or frames.stride(1) < w:
            raise ValueError("frames rows must be contiguous")
        if records is None:
            records = self.new_records(n - 1)
            wait_torch = True  # the zero-fill runs on torch's stream: order the library's writes after it
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        if n > 1:
            self._pending[records.data_ptr()] = records
        if undistort is not None:  # ops.Undistorter: frames are remapped into the stream's slab first
            self.ctx.check(self.ctx.lib.dvo_stream_process_undistorted(
                self.h, undistort.h_, frames.data_ptr(), n, frames.stride(0), frames.stride(1),
                records.data_ptr() if n > 1 else None))
        else:
            self.ctx.check(self.ctx.lib.dvo_stream_process(self.h, frames.data_ptr(), n, frames.stride(0),
                                                           frames.stride(1), records.data_ptr() if n > 1 else None))
        self._take_retired()  # this batch, and any submitted before it (drained)
        self._last = (frames, records)
        self._hold(frames, records)
        return records

    def process_pairs(self, frames: torch.Tensor, records: torch.Tensor | None = None,
                      wait_torch: bool = True) -> torch.Tensor:
        """The reference's schedule (dvo_stream_process_pairs): frames holds 2n
        frames and pair p is frames 2p, 2p+1, each detected on its own, as
        visual_odometry_calculations re-detects both frames of every pair
        (visual_odometry_v3.py:387-392).  Records / pose tail as process()."""
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [2n, H, W] device tensor")
        n2, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != stream {self.width}x{self.height}")
        if n2 % 2 or n2 == 0:
            raise ValueError("frames must hold an even, non-zero number of frames (pairs 2p, 2p+1)")
        if frames.stride(2) != 1 or frames.stride(1) < w:
            raise ValueError("frames rows must be contiguous")
        if records is None:
            records = self.new_records(n2 // 2)
            wait_torch = True
        if wait_torch:
            self._after_torch()
        self._lm_fits(n2 // 2, shared=False)
        self._pending[records.data_ptr()] = records
        self.ctx.check(self.ctx.lib.dvo_stream_process_pairs(self.h, frames.data_ptr(), n2 // 2, frames.stride(0),
                                                             frames.stride(1), records.data_ptr()))
        self._take_retired()
        self._last = (frames, records)
        self._hold(frames, records)
        return records

    # ---- pipelined batches (dvo_stream_submit): see include/dvo.h ------------------------------
    @staticmethod
    def pipeline_depth() -> int:
        from ._native import load_library
        return int(load_library().dvo_pipeline_depth())

    def _check_frames(self, frames, pairs_layout=False):
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [n, H, W] device tensor")
        n, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != stream {self.width}x{self.height}")
        if frames.stride(2) != 1 or frames.stride(1) < w:
            raise ValueError("frames rows must be contiguous")
        if pairs_layout and (n % 2 or n == 0):
            raise ValueError("frames must hold an even, non-zero number of frames (pairs 2p, 2p+1)")
        return n

    def _check_frames_bgr(self, frames, undistort):
        from .ops import check_colour_frames
        n, h, w, c = check_colour_frames(frames, "frames", (self.width, self.height), "stream")
        if undistort is not None and (undistort.w, undistort.h) != (self.width, self.height):
            raise ValueError(f"undistorter size {undistort.w}x{undistort.h} != stream {self.width}x{self.height}")
        return n, c

    def _process_bgr(self, frames, records, wait_torch, undistort):
        """process() of colour frames (dvo_stream_process_bgr)."""
        n, c = self._check_frames_bgr(frames, undistort)
        if records is None:
            records = self.new_records(n - 1)
            wait_torch = True  # the zero-fill runs on torch's stream: order the library's writes after it
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        if n > 1:
            self._pending[records.data_ptr()] = records
        self.ctx.check(self.ctx.lib.dvo_stream_process_bgr(
            self.h, undistort.h_ if undistort is not None else None, frames.data_ptr(), n, frames.stride(0),
            frames.stride(1), c, records.data_ptr() if n > 1 else None))
        self._take_retired()
        self._last = (frames, records)
        self._hold(frames, records)
        return records

    def _submit_bgr(self, frames, records, wait_torch, undistort):
        """submit() of colour frames (dvo_stream_submit_bgr)."""
        n, c = self._check_frames_bgr(frames, undistort)
        if n < 2:
            raise ValueError("a submitted batch needs >= 2 frames")
        if records.numel() < (n - 1) * PAIR_RECORD_DTYPE.itemsize:
            raise ValueError("records too small")
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        self.ctx.check(self.ctx.lib.dvo_stream_submit_bgr(
            self.h, undistort.h_ if undistort is not None else None, frames.data_ptr(), n, frames.stride(0),
            frames.stride(1), c, records.data_ptr()))
        self._pending[records.data_ptr()] = records
        self._hold(frames, records)
        return self._take_retired()

    # ---- JPEG frames (dvo_stream_process_jpeg / _submit_jpeg): see include/dvo.h ---------------
    def _check_jpeg(self, blobs, undistort, n_min):
        from .ops import jpeg_blobs
        arrs, ptrs, lens = jpeg_blobs(blobs, self.max_frames)
        if len(arrs) < n_min:
            raise ValueError(f"a submitted batch needs >= {n_min} frames")
        if undistort is not None and (undistort.w, undistort.h) != (self.width, self.height):
            raise ValueError(f"undistorter size {undistort.w}x{undistort.h} != stream {self.width}x{self.height}")
        return arrs, ptrs, lens

    @property
    def jpeg_decoder(self):
        """The stream's ops.JpegDecoder (made at the first JPEG batch); its status() tells
        which frames of the last JPEG batch were corrupt, after a sync()."""
        if getattr(self, "_jpeg", None) is None:
            from .ops import JpegDecoder
            group = min(int(self.max_frames), JpegDecoder.default_group_frames(self.width, self.height))
            self._jpeg = JpegDecoder(self.width, self.height, group_frames=group, ctx=self.ctx)
        return self._jpeg

    def process_jpeg(self, blobs, records: torch.Tensor | None = None, undistort=None, entropy=None) -> torch.Tensor:
        """process() of a list of JPEG files (bytes-like) of the stream's size: decoded to
        gray on the device, and remapped by `undistort` (ops.Undistorter) if given, into
        the stream's slab; from there exactly process() of colour frames.  entropy:
        "device" or "device_split" (ops.JpegDecoder.decode), kept for the calls that
        follow; None: as it is ("device" at first)."""
        arrs, ptrs, lens = self._check_jpeg(blobs, undistort, 1)
        n = len(arrs)
        dec = self.jpeg_decoder
        if entropy is not None:
            dec.set_stream_entropy(entropy)
        if records is None:
            records = self.new_records(n - 1)
        self._after_torch()
        self._lm_fits(n - 1)
        if n > 1:
            self._pending[records.data_ptr()] = records
        self.ctx.check(self.ctx.lib.dvo_stream_process_jpeg(
            self.h, dec.h_, undistort.h_ if undistort is not None else None, ptrs, lens, n,
            records.data_ptr() if n > 1 else None))
        dec._n = n
        self._take_retired()
        self._last = (records,)
        self._hold(records)
        return records

    def submit_jpeg(self, blobs, records: torch.Tensor, undistort=None, entropy=None) -> list:
        """submit() of a list of JPEG files (see process_jpeg)."""
        arrs, ptrs, lens = self._check_jpeg(blobs, undistort, 2)
        n = len(arrs)
        if not isinstance(records, torch.Tensor) or records.numel() < (n - 1) * PAIR_RECORD_DTYPE.itemsize:
            raise ValueError("records too small")
        dec = self.jpeg_decoder
        if entropy is not None:
            dec.set_stream_entropy(entropy)
        self._after_torch()
        self._lm_fits(n - 1)
        self.ctx.check(self.ctx.lib.dvo_stream_submit_jpeg(
            self.h, dec.h_, undistort.h_ if undistort is not None else None, ptrs, lens, n, records.data_ptr()))
        dec._n = n
        self._pending[records.data_ptr()] = records
        self._hold(records)
        return self._take_retired()

    def submit(self, frames: torch.Tensor, records: torch.Tensor, wait_torch: bool = True, undistort=None) -> list:
        """Pipelined batch (dvo_stream_submit): detection and matching of these
        frames, then one merged RANSAC round of the pending batches.  `records`
        (n - 1 records) is complete once the batch retires, pipeline_depth() - 1
        submits later or at drain(); it is kept referenced until then.  Returns
        the batches this call retired, oldest first, as (records, pairs).
        Colour frames (uint8 [n, H, W, C], C = 3 or 4) are converted to gray, and
        remapped by `undistort` (ops.Undistorter) if given, into the stream's slab
        first.  The library has no undistorting submit for mono8 frames: remap them
        with Undistorter.apply and submit the result."""
        if frames.dim() == 4:
            return self._submit_bgr(frames, records, wait_torch, undistort)
        if undistort is not None:
            raise ValueError("submit(undistort=) takes colour frames; remap mono8 frames with Undistorter.apply first")
        n = self._check_frames(frames)
        if n < 2:
            raise ValueError("a submitted batch needs >= 2 frames")
        if records.numel() < (n - 1) * PAIR_RECORD_DTYPE.itemsize:
            raise ValueError("records too small")
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        self.ctx.check(self.ctx.lib.dvo_stream_submit(self.h, frames.data_ptr(), n, frames.stride(0),
                                                      frames.stride(1), records.data_ptr()))
        self._pending[records.data_ptr()] = records
        self._hold(frames, records)
        return self._take_retired()

    def submit_pairs(self, frames: torch.Tensor, records: torch.Tensor, wait_torch: bool = True) -> list:
        """submit() with the reference's schedule (pair p = frames 2p, 2p+1; process_pairs)."""
        n2 = self._check_frames(frames, pairs_layout=True)
        if records.numel() < (n2 // 2) * PAIR_RECORD_DTYPE.itemsize:
            raise ValueError("records too small")
        if wait_torch:
            self._after_torch()
        self._lm_fits(n2 // 2, shared=False)
        self.ctx.check(self.ctx.lib.dvo_stream_submit_pairs(self.h, frames.data_ptr(), n2 // 2, frames.stride(0),
                                                            frames.stride(1), records.data_ptr()))
        self._pending[records.data_ptr()] = records
        self._hold(frames, records)
        return self._take_retired()

    def drain(self) -> list:
        """Run the pending batches' remaining rounds and retire them (oldest first)."""
        self.ctx.check(self.ctx.lib.dvo_stream_drain(self.h))
        return self._take_retired()

    def _take_retired(self) -> list:
        from ._native import _vp
        cap = 16
        recs = (_vp * cap)()
        pairs = (ctypes.c_int * cap)()
        n = self.ctx.lib.dvo_stream_retired(self.h, recs, pairs, cap)
        # the call just made took the bound Landmarks: it stays referenced with that batch's
        # records (the newest pending ones) until the batch retires
        lm, self._lm_next = self._lm_next, None
        tr, self._tr_next = self._tr_next, None
        tp, self._tp_next = self._tp_next, None
        rf, self._rf_next = self._rf_next, None
        bd, self._bd_next = self._bd_next, None
        pn, self._pn_next = self._pn_next, None
        if lm is not None and self._pending:
            self._lm_pending[next(reversed(self._pending))] = (lm, tr, tp, rf, bd, pn)
        out, lms = [], []
        for i in range(min(n, cap)):
            t = self._pending.pop(recs[i], None)
            if t is None:
                raise RuntimeError("retired records that were not submitted through this FrameStream")
            out.append((t, int(pairs[i])))
            lm, tr, tp, rf, bd, pn = self._lm_pending.pop(recs[i], (None, None, None, None, None, None))
            if lm is not None:
                lms += [lm.entries, lm.counts]
            if tr is not None:
                lms += [tr.links, tr.scales]
            if tp is not None:
                lms += [tp.poses]
            if rf is not None:
                lms += [rf.refined, rf.ids]
            if bd is not None:
                lms += [bd.bundle, bd.points]
            if pn is not None:
                lms += list(pn.tensors())
        if out:
            # the retire kernels (records_kernel, the landmark kernels) writing these buffers are
            # queued on the library's stream by the call that retired them: keep the tensors alive
            # until they have run, whether or not the caller keeps the returned list (process() drops it)
            self._hold(*[t for t, _ in out], *lms)
        return out

    def pose_tail_batch(self, records: torch.Tensor, pairs: int, corners_prev: torch.Tensor,
                        corners_cur: torch.Tensor, marker_length: float, T_rel: torch.Tensor,
                        T_abs: torch.Tensor, wait_torch: bool = False):
        """Device pose tail over a retired batch's records (dvo_stream_pose_tail_batch), on this
        stream's carry (shared with share_pose)."""
        k = corners_prev.shape[1]
        if corners_prev.shape[0] < pairs or corners_cur.shape[0] < pairs or T_rel.shape[0] < pairs \
                or T_abs.shape[0] < pairs:
            raise ValueError("corners / outputs hold fewer pairs than the batch")
        if wait_torch:
            self._after_torch()
        self.ctx.check(self.ctx.lib.dvo_stream_pose_tail_batch(
            self.h, records.data_ptr(), int(pairs), corners_prev.data_ptr(), corners_cur.data_ptr(), k,
            float(marker_length), T_rel.data_ptr(), T_abs.data_ptr()))
        self._hold(records, corners_prev, corners_cur, T_rel, T_abs)
        return T_rel, T_abs

    def _hold(self, *tensors):
        """Keep the tensors the library's stream reads or writes alive until that
        work has finished, so torch's caching allocator cannot hand their blocks
        to a new tensor meanwhile.  (Not record_stream: the allocator would then
        record events on this stream after close() destroyed it.)"""
        ev = torch.cuda.Event()
        ev.record(self._ext)
        self._held.append((ev, tensors))
        while self._held and self._held[0][0].query():
            self._held.popleft()

    def _after_torch(self):
        """Order the library's HIP stream after work already queued on torch's
        current stream (frames / corners produced by torch)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._ext.wait_event(ev)

    def record_event(self) -> torch.cuda.Event:
        """An event on the library's stream after everything enqueued so far."""
        ev = torch.cuda.Event()
        ev.record(self._ext)
        return ev

    def wait_event(self, ev):
        """Order the library's HIP stream after a torch.cuda.Event (e.g. the
        all-gather that last read this stream's records buffer)."""
        if ev is not None:
            self._ext.wait_event(ev)

    def share_pose(self, owner: "FrameStream"):
        """Chain this stream's pose tails on `owner`'s carry (batches alternating
        between streams form one pose stream)."""
        self.ctx.check(self.ctx.lib.dvo_stream_share_pose(self.h, owner.h))

    def reset_pose(self, P0=None, T0=None):
        """Carry-in of the pose tail: P_prev (3x4, default K[I|0] as in controlled
        mode, v3:164-166) and the absolute pose (4x4, default identity)."""
        P0 = self.K @ np.hstack((np.eye(3), np.zeros((3, 1)))) if P0 is None else np.asarray(P0, np.float64)
        T0 = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
        self.ctx.check(self.ctx.lib.dvo_stream_reset_pose(self.h, ptr(np.ascontiguousarray(P0)),
                                                          ptr(np.ascontiguousarray(T0))))

    def pose_tail(self, corners_prev: torch.Tensor, corners_cur: torch.Tensor, marker_length: float,
                  T_rel: torch.Tensor | None = None, T_abs: torch.Tensor | None = None, wait_torch: bool = True):
        """Device pose tail for the last processed batch (see dvo.h); corners are
        float64 [pairs, k, 2] device tensors.  Returns (T_rel, T_abs) [pairs, 4, 4]."""
        pairs, k = corners_prev.shape[0], corners_prev.shape[1]
        if T_rel is None or T_abs is None:
            # blocks fresh from torch's stream may still be in use by work queued there
            wait_torch = True
        if T_rel is None:
            T_rel = torch.empty((pairs, 4, 4), dtype=torch.float64, device=self.device)
        if T_abs is None:
            T_abs = torch.empty((pairs, 4, 4), dtype=torch.float64, device=self.device)
        if wait_torch:
            self._after_torch()
        self.ctx.check(self.ctx.lib.dvo_stream_pose_tail(self.h, corners_prev.data_ptr(), corners_cur.data_ptr(), k,
                                                         float(marker_length), T_rel.data_ptr(), T_abs.data_ptr()))
        self._hold(corners_prev, corners_cur, T_rel, T_abs, *self._last)
        return T_rel, T_abs

    def set_profiling(self, enable: bool = True):
        self.ctx.check(self.ctx.lib.dvo_stream_set_profiling(self.h, int(enable)))

    def stage_times(self):
        """{stage: accumulated device ms} over calls since set_profiling(True), plus call count."""
        from ._native import DVO_NSTAGES, STAGE_NAMES
        ms = np.zeros(DVO_NSTAGES, np.float64)
        calls = ctypes.c_int()
        self.ctx.check(self.ctx.lib.dvo_stream_stage_times(self.h, ptr(ms), ctypes.byref(calls)))
        return dict(zip(STAGE_NAMES, ms.tolist())), calls.value

    def sync(self):
        self.ctx.check(self.ctx.lib.dvo_stream_sync(self.h))
        self._held.clear()

    @staticmethod
    def records_numpy(records: torch.Tensor, n_pairs: int) -> np.ndarray:
        raw = records[: n_pairs * PAIR_RECORD_DTYPE.itemsize].cpu().numpy()
        return raw.view(PAIR_RECORD_DTYPE).copy()

    def features(self, frame: int):
        cap = self.nfeatures + 1024
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = ctypes.c_int()
        self.ctx.check(self.ctx.lib.dvo_stream_get_features(self.h, frame, ptr(kps), ptr(desc), cap, ctypes.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def matches(self, pair: int) -> np.ndarray:
        cap = self.nfeatures + 1024
        out = np.zeros(cap, DMATCH_DTYPE)
        m = ctypes.c_int()
        self.ctx.check(self.ctx.lib.dvo_stream_get_matches(self.h, pair, ptr(out), cap, ctypes.byref(m)))
        return out[:m.value].copy()

    def pyramid(self, frame: int, level: int, blurred: bool = False) -> np.ndarray:
        from .plan import level_sizes
        lw, lh = level_sizes(self.width, self.height)[level]
        out = np.zeros(lw * lh, np.uint8)
        self.ctx.check(self.ctx.lib.dvo_stream_get_pyramid(self.h, frame, level, int(blurred), ptr(out), out.size))
        return out.reshape(lh, lw)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_stream_destroy(self.h)  # synchronises the stream first
            self.h = None
            if getattr(self, "_jpeg", None) is not None:  # its work ran on the stream just synchronised
                self._jpeg.close()
                self._jpeg = None
            if getattr(self, "_held", None):
                self._held.clear()
            self._last = ()
            self._pending = {}
            self._lm_next, self._lm_pending, self._tr_next, self._tp_next, self._rf_next = None, {}, None, None, None
            self._bd_next = self._pn_next = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KnnFrameStream:
    """The batched frame stream of the k-NN modes 'knn_sift' and 'surf' (dvo_knn_stream_process):
    n device-resident frames per call are detected once each (SIFT or SURF), every consecutive
    pair goes through BFMatcher(NORM_L1).knnMatch(k=2), the ratio test and keypoint gather,
    findEssentialMat(RANSAC) and recoverPose, and n - 1 pair records (PAIR_RECORD_DTYPE) land in
    device memory; nothing is read back on the way.  The records equal ops.KnnPairStream.pair's
    on the same frames (n_hypotheses aside) and feed stream.PoseTail.run as they are.

    feat_cap: features kept per frame (None: the detector's list capacity, 65536 for SIFT, which
    costs 44 MB per frame slot: give the count you expect).  A frame with more features marks its
    two pairs DVO_ECAP.  The calls run on the context's HIP stream, asynchronously; sync() waits.

    detect_group (SIFT only): 0 detects frame by frame; G >= 1 detects G frames per launch
    (dvo_knn_stream_set_detect_group, the detector of ops.SiftBatch) straight into the frame slots,
    for ops.SiftBatch.scratch_bytes(width, height, G) more device memory.  Same records either way.

    surf_group (SURF only): the same for detector="surf" (dvo_knn_stream_set_surf_group, the detector
    of ops.SurfBatch with the stream's hessian_threshold), for ops.SurfBatch.scratch_bytes(width,
    height, G) more device memory.  Same records either way.

    nfeatures (SIFT only; dvo_knn_stream_set_nfeatures): SIFT_create(nfeatures).  0 keeps everything
    a frame's detector finds, so one textured frame can pass feat_cap.  N > 0 keeps each frame's best
    N by response as OpenCV 4.x's retainBest does (ops.sift_detect_and_compute(img, nfeatures=N)'s
    features, in that order, boundary ties included), frame by frame and with a detect_group, for
    both matchers; only a frame whose kept count passes feat_cap is DVO_ECAP.  Give feat_cap = N
    plus room for boundary ties.  ops.SiftBatch.retain_bytes(1), and retain_bytes(G) with a
    detect_group, more device memory.

    matcher: "bf" (the default) or "flann", the reference's 'flann' mode (dvo_knn_stream_set_flann):
    every pair's randomized kd-forest (trees) is built and searched (checks) on the device in place
    of BFMatcher, with no read-back, for ops.knn_stream_flann_bytes(max_frames, feat_cap, trees)
    more device memory.  The records are ops.KnnPairStream(matcher="flann").pair's chained through
    its returned state: the stream keeps cv::theRNG()'s state on the device (rng_state; enabling
    sets ops.THE_RNG_SEED, rng_state=... another start), advances it by trees (2 nt - 1) draws per
    built pair, and carries it from call to call, so the records do not depend on the split.

    process() is detect() followed by finish(); a stream sharded across ranks (dist.ShardedKnnRunner)
    calls the two phases itself, with the all-gather of the ranks' draws words between them.

    raw_input (dvo_knn_stream_set_raw_input): the stream also takes what a camera delivers, as
    FrameStream does: colour frames ([n, H, W, 3 or 4], cv.cvtColor), distorted frames (undistort=
    an ops.Undistorter, cv.undistort) and JPEG files (process_jpeg / detect_jpeg, cv.imdecode).  One
    launch on the stream's own HIP stream brings them to gray in a slab of
    ops.knn_stream_raw_input_bytes(width, height, max_frames) more device memory, and detection
    runs there; the records are those of process() on the gray frames ops.bgr2gray_device,
    Undistorter.apply or JpegDecoder.decode make.  Construct the stream with the new camera matrix
    as K when its frames are undistorted.  Plain mono frames stay in place, slab or not."""

    def __init__(self, width: int, height: int, K, max_frames: int, detector="sift", feat_cap: int | None = None,
                 hessian_threshold: float = 400.0, ratio: float = 0.75, prob: float = 0.999, threshold: float = 1.0,
                 max_iters: int = 1000, dist_thresh: float = 50.0, ctx: Context | None = None, *,
                 detect_group: int = 0, surf_group: int = 0, matcher: str = "bf", trees: int = 5, checks: int = 50,
                 rng_state: int | None = None, raw_input: bool = False, nfeatures: int = 0):
        from ._native import KnnStreamConfig
        from .ops import KNN_DETECTORS, KNN_MATCHERS
        self.h = None
        if matcher not in KNN_MATCHERS:
            raise ValueError(f"matcher must be one of {sorted(KNN_MATCHERS)}")
        if matcher == "bf" and rng_state is not None:
            raise ValueError("rng_state needs matcher='flann'")
        if matcher == "flann" and not (1 <= int(trees) <= 64 and int(checks) >= 1):
            raise ValueError("matcher='flann' needs trees in 1..64 and checks >= 1")
        self.ctx = ctx if ctx is not None else Context.default()
        self.device = torch.device("cuda", self.ctx.device)
        cfg = KnnStreamConfig()
        cfg.width, cfg.height, cfg.max_frames = int(width), int(height), int(max_frames)
        cfg.detector = KNN_DETECTORS[detector] if isinstance(detector, str) else int(detector)
        cfg.feat_cap = 0 if feat_cap is None else int(feat_cap)
        cfg.hessian_threshold, cfg.ratio = float(hessian_threshold), float(ratio)
        K = np.asarray(K, np.float64).reshape(9)
        for i in range(9):
            cfg.K[i] = float(K[i])
        cfg.prob, cfg.threshold, cfg.max_iters = float(prob), float(threshold), int(max_iters)
        cfg.dist_thresh = float(dist_thresh)
        h = _vp()
        self.ctx.check(self.ctx.lib.dvo_knn_stream_create(self.ctx.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.detect_group = 0
        if detect_group:
            self.set_detect_group(detect_group)
        self.surf_group = 0
        if surf_group:
            self.set_surf_group(surf_group)
        self.nfeatures = 0
        self._pending = 0
        if nfeatures:
            self.set_nfeatures(nfeatures)
        self.trees = self.checks = 0
        if matcher == "flann":
            self.set_flann(trees, checks)
            if rng_state is not None:
                self.rng_state = rng_state
        self.raw_input = False
        self._jpeg = None
        if raw_input:
            self.set_raw_input(True)
        self._ext = torch.cuda.ExternalStream(self.hip_stream, device=self.device)
        self._held = collections.deque()  # (event, tensors) in flight on the library's stream
        self._pending = 0  # frames of the last detect() (sizes finish()'s records)
        self._lm_next = None  # bind_landmarks: the Landmarks the next process() / finish() takes
        self._tr_next = None  # bind_tracks: the Tracks it takes with them
        self._tp_next = None  # bind_track_poses: and the TrackPoses
        self._rf_next = None  # bind_refine: and the RefinedLandmarks
        self._bd_next = None  # bind_bundle: and the TrackBundle
        self._pn_next = None  # bind_pnp: and the TrackPnP
        self.width, self.height, self.max_frames = int(width), int(height), int(max_frames)
        self.dim = 64 if cfg.detector == 1 else 128
        self.K = K.reshape(3, 3)

    @property
    def hip_stream(self) -> int:
        return self.ctx.lib.dvo_knn_stream_hip_stream(self.h) or 0

    def new_records(self, n_pairs: int) -> torch.Tensor:
        return torch.zeros(max(n_pairs, 1) * PAIR_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=self.device)

    def bind_landmarks(self, lm: Landmarks | None):
        """Have the next batch (the next process*() or finish(); detect*() alone does not take it)
        write its landmarks into `lm` (dvo_knn_stream_set_landmarks); lm needs a row per pair of
        that batch.  One-shot: the batch after it writes nothing.  None clears a pending binding."""
        self._lm_next = _bind_landmarks(self, self.ctx.lib.dvo_knn_stream_set_landmarks, lm)
        if lm is None:
            self._tr_next = self._tp_next = self._rf_next = self._bd_next = self._pn_next = None  # the library clears the companions with it

    def bind_tracks(self, tr: Tracks | None):
        """Have the next batch also write its tracks into `tr` (dvo_knn_stream_set_tracks), after
        its landmarks.  Call it after bind_landmarks (ValueError otherwise), with a Tracks of the
        same cap.  One-shot; None clears a pending binding; detect*() alone does not take it."""
        self._tr_next = _bind_tracks(self, self.ctx.lib.dvo_knn_stream_set_tracks, tr)
        self._tp_next = self._rf_next = self._bd_next = self._pn_next = None  # the library's call cleared the later pending bindings

    def bind_track_poses(self, tp: TrackPoses | None, iters: int = 10, huber_px: float = 1.0, inlier_px: float = 2.0,
                         min_points: int = 6):
        """Have the next batch also write its track poses into `tp` (dvo_knn_stream_set_track_poses),
        after its tracks.  Call it after bind_tracks (ValueError otherwise); the parameters are
        FrameStream.bind_track_poses's.  One-shot; None clears a pending binding; detect*() alone
        does not take it."""
        self._rf_next = self._bd_next = None  # the library's call clears pending refine and bundle bindings
        self._tp_next = _bind_track_poses(self, self.ctx.lib.dvo_knn_stream_set_track_poses, tp, iters, huber_px,
                                          inlier_px, min_points)

    def bind_refine(self, rf: RefinedLandmarks | None, views: int = 6, iters: int = 5, huber_px: float = 1.0,
                    inlier_px: float = 2.0, ids: bool = True, refined: bool = True):
        """Have the next batch also write its track ids and refined landmarks into `rf`
        (dvo_knn_stream_set_track_refine), after its tracks and track poses; the parameters are
        FrameStream.bind_refine's.  Call it last.  One-shot; None clears a pending binding;
        detect*() alone does not take it."""
        self._bd_next = None  # the library's call clears a pending bundle binding: bind the bundle last
        self._rf_next = _bind_refine(self, self.ctx.lib.dvo_knn_stream_set_track_refine, rf, views, iters, huber_px,
                                     inlier_px, ids, refined)

    def bind_bundle(self, bd: TrackBundle | None, views: int = 6, iters: int = 5, lam: float = 0.0, huber_px: float = 1.0,
                    inlier_px: float = 2.0, min_points: int = 8, pairs: bool = True, points: bool = True):
        """Have the next batch also write its track bundle into `bd` (dvo_knn_stream_set_track_bundle),
        after everything else; the parameters are FrameStream.bind_bundle's.  Call it last.
        One-shot; None clears a pending binding; detect*() alone does not take it."""
        self._bd_next = _bind_bundle(self, self.ctx.lib.dvo_knn_stream_set_track_bundle, bd, views, iters, lam,
                                     huber_px, inlier_px, min_points, pairs, points)

    def bind_pnp(self, pn: TrackPnP | None, hyps: int = 128, iters: int = 10, huber_px: float = 1.0,
                 inlier_px: float = 2.0, min_points: int = 6, seed: int = 0):
        """Have the next batch also write its track PnP into `pn` (dvo_knn_stream_set_track_pnp), after
        everything else; the parameters are FrameStream.bind_pnp's.  Call it after bind_tracks.
        One-shot; None clears a pending binding; detect*() alone does not take it."""
        self._pn_next = _bind_pnp(self, self.ctx.lib.dvo_knn_stream_set_track_pnp, pn, hyps, iters, huber_px,
                                  inlier_px, min_points, seed)

    def _lm_fits(self, pairs: int):
        if self._lm_next is not None and self._lm_next.n_pairs < pairs:
            raise ValueError(f"the bound Landmarks holds {self._lm_next.n_pairs} pairs, the batch has {pairs}")

    def _lm_taken(self):
        """The tensors of the Landmarks the call just made took (to keep alive with its records)."""
        lm, self._lm_next = self._lm_next, None
        tr, self._tr_next = self._tr_next, None
        tp, self._tp_next = self._tp_next, None
        rf, self._rf_next = self._rf_next, None
        bd, self._bd_next = self._bd_next, None
        pn, self._pn_next = self._pn_next, None
        return ((() if lm is None else (lm.entries, lm.counts)) + (() if tr is None else (tr.links, tr.scales))
                + (() if tp is None else (tp.poses,)) + (() if rf is None else (rf.refined, rf.ids))
                + (() if bd is None else (bd.bundle, bd.points)) + (() if pn is None else pn.tensors()))

    def set_detect_group(self, group: int):
        """SIFT frames per detection launch from the next process() on (0: frame by frame).  Waits
        for the stream and allocates or frees the group's scratch; DVOError(DVO_EINVAL) on a SURF stream."""
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_detect_group(self.h, int(group)))
        self.detect_group, self._pending = int(group), 0  # a pending detect() is dropped

    def set_surf_group(self, group: int):
        """SURF frames per detection launch from the next process() on (0: frame by frame).  Waits
        for the stream and allocates or frees the group's scratch; DVOError(DVO_EINVAL) on a SIFT stream."""
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_surf_group(self.h, int(group)))
        self.surf_group, self._pending = int(group), 0  # a pending detect() is dropped

    def set_nfeatures(self, nfeatures: int):
        """SIFT_create(nfeatures) from the next detection on (0: everything is kept).  A change waits
        for the stream, allocates the retain stage's scratch once and drops a pending detect();
        DVOError(DVO_EINVAL) on a SURF stream or a negative value."""
        from .ops import _check_nfeatures
        n = _check_nfeatures(nfeatures)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_nfeatures(self.h, n))
        if n != self.nfeatures:
            self.nfeatures, self._pending = n, 0

    def set_flann(self, trees: int, checks: int = 50):
        """The FLANN kd-forest matcher from the next process() on: trees 1..64 and checks >= 1; trees
        0 returns to BFMatcher.  Waits for the stream, allocates or frees the mode's scratch and sets
        rng_state to ops.THE_RNG_SEED; DVOError(DVO_EINVAL) on bad arguments."""
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_flann(self.h, int(trees), int(checks)))
        self.trees, self.checks = int(trees), int(checks) if trees else 0
        self._pending = 0  # a pending detect() is dropped

    def set_raw_input(self, enable: bool = True):
        """Colour, distorted and JPEG input from the next call on (False: mono frames only).  A change
        waits for the stream, allocates or frees the gray slab and drops a pending detect()."""
        enable = bool(enable)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_raw_input(self.h, int(enable)))
        if enable != self.raw_input:
            self.raw_input, self._pending = enable, 0

    @property
    def matcher(self) -> str:
        return "flann" if self.trees else "bf"

    @property
    def rng_state(self) -> int:
        """cv::theRNG()'s state after the calls enqueued so far (waits for them); setting it is ordered
        after them.  DVOError(DVO_EINVAL) on a stream that matches with BFMatcher."""
        st = ctypes.c_uint64()
        self.ctx.check(self.ctx.lib.dvo_knn_stream_get_rng_state(self.h, ctypes.byref(st)))
        return int(st.value)

    @rng_state.setter
    def rng_state(self, state: int):
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_rng_state(self.h, ctypes.c_uint64(int(state))))

    def process(self, frames, records: torch.Tensor | None = None, wait_torch: bool = True,
                undistort=None) -> torch.Tensor:
        """Enqueue the batch (asynchronous).  frames: a uint8 [n, H, W] device tensor (rows contiguous,
        any row pitch) or a numpy array, which is uploaded first.  With wait_torch the batch is
        ordered after work queued on torch's current stream; pass False for frames already resident.
        On a raw_input stream: colour frames (uint8 [n, H, W, C], C = 3 or 4: B, G, R first) are
        converted to gray, and with undistort (an ops.Undistorter) colour or mono frames are
        remapped, into the stream's slab on the way (dvo_knn_stream_process_raw)."""
        if self._is_raw(frames, undistort):
            frames, wait_torch, c = self._check_raw(frames, wait_torch, undistort)
        else:
            (frames, wait_torch), c = self._check_frames(frames, wait_torch), 0
        n = frames.shape[0]
        if records is None:
            records = self.new_records(n - 1)
            wait_torch = True  # the zero-fill runs on torch's stream: order the library's writes after it
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        if c:
            self.ctx.check(self.ctx.lib.dvo_knn_stream_process_raw(
                self.h, undistort.h_ if undistort is not None else None, frames.data_ptr(), n, frames.stride(0),
                frames.stride(1), c, records.data_ptr() if n > 1 else None))  # a refused call changes nothing
            self._pending = 0
        else:
            self._pending = 0  # process replaces a pending detect()
            self.ctx.check(self.ctx.lib.dvo_knn_stream_process(self.h, frames.data_ptr() if n else None, n,
                                                               frames.stride(0), frames.stride(1),
                                                               records.data_ptr() if n > 1 else None))
        self._hold(frames, records, *self._lm_taken())
        return records

    @staticmethod
    def _is_raw(frames, undistort) -> bool:
        """Whether the batch takes the raw-input path: colour frames, or any frames to be undistorted."""
        return undistort is not None or (isinstance(frames, np.ndarray) and frames.ndim == 4) \
            or (isinstance(frames, torch.Tensor) and frames.dim() == 4)

    def _check_undistort(self, undistort):
        if not self.raw_input:
            raise ValueError("the stream takes mono frames only: construct it with raw_input=True or call "
                             "set_raw_input(True)")
        if undistort is not None and (undistort.w, undistort.h) != (self.width, self.height):
            raise ValueError(f"undistorter size {undistort.w}x{undistort.h} != stream {self.width}x{self.height}")

    def _check_raw(self, frames, wait_torch, undistort):
        """(device frames, wait_torch, channels) of a raw-input batch; ValueError before any library call."""
        from .ops import check_colour_frames
        if isinstance(frames, np.ndarray) and frames.ndim == 4:
            if frames.dtype != np.uint8 or frames.shape[3] not in (3, 4):
                raise ValueError("frames must be uint8 [n, H, W, 3 or 4]")
            frames = torch.from_numpy(np.ascontiguousarray(frames)).to(self.device)
            wait_torch = True
        if isinstance(frames, torch.Tensor) and frames.dim() == 4:
            n, _, _, c = check_colour_frames(frames, "frames", (self.width, self.height), "stream")
        else:
            (frames, wait_torch), c = self._check_frames(frames, wait_torch), 1
            n = frames.shape[0]
        if n < 1:
            raise ValueError("frames is empty")
        self._check_undistort(undistort)
        return frames, wait_torch, c

    def _check_frames(self, frames, wait_torch):
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or frames.ndim != 3:
                raise ValueError("frames must be uint8 [n, H, W]")
            frames = torch.from_numpy(np.ascontiguousarray(frames)).to(self.device)
            wait_torch = True
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [n, H, W] device tensor or numpy array")
        n, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != stream {self.width}x{self.height}")
        if n and (frames.stride(2) != 1 or frames.stride(1) < w):
            raise ValueError("frames rows must be contiguous")
        return frames, wait_torch

    def _after_torch(self):
        """Order the library's stream after the work queued on torch's current stream."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._ext.wait_event(ev)

    def _hold(self, *tensors):
        """Keep the tensors alive until the library's stream is past them."""
        ev = torch.cuda.Event()
        ev.record(self._ext)
        self._held.append((ev, tensors))
        while self._held and self._held[0][0].query():
            self._held.popleft()

    def record_event(self) -> torch.cuda.Event:
        """An event on the library's stream after everything enqueued so far."""
        ev = torch.cuda.Event()
        ev.record(self._ext)
        return ev

    def wait_event(self, ev):
        """Order the library's stream after a torch.cuda.Event (None: nothing to wait for)."""
        if ev is not None:
            self._ext.wait_event(ev)

    @staticmethod
    def _word_tensor(t, n, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint64, torch.int64) \
                or t.dim() != 1 or t.numel() != n or (n > 1 and t.stride(0) != 1):
            raise ValueError(f"{what} must be a contiguous uint64 or int64 device tensor of {n} element(s)")
        return t

    def detect(self, frames, draws: torch.Tensor | None = None, wait_torch: bool = True, undistort=None):
        """The first phase of process() (dvo_knn_stream_detect, asynchronous): the frames are detected
        and features() works; finish() does the rest.  draws: a 1-element uint64 or int64 device
        tensor (or such a view into a larger one, a rank's slot of a gather buffer) that receives
        the theRNG draws the call's pairs will consume, 0 on a BFMatcher stream.  A detect while
        another is pending replaces it.  Returns the device frames.  Colour frames and undistort=
        as in process() (dvo_knn_stream_detect_raw); such a call, when refused, leaves a pending
        detection as it was."""
        if self._is_raw(frames, undistort):
            frames, wait_torch, c = self._check_raw(frames, wait_torch, undistort)
        else:
            (frames, wait_torch), c = self._check_frames(frames, wait_torch), 0
        n = frames.shape[0]
        self._check_draws(draws)
        if wait_torch:
            self._after_torch()
        if c:
            self.ctx.check(self.ctx.lib.dvo_knn_stream_detect_raw(
                self.h, undistort.h_ if undistort is not None else None, frames.data_ptr(), n, frames.stride(0),
                frames.stride(1), c, None if draws is None else draws.data_ptr()))
        else:
            self._pending = 0  # a refused call leaves nothing pending
            self.ctx.check(self.ctx.lib.dvo_knn_stream_detect(self.h, frames.data_ptr() if n else None, n,
                                                              frames.stride(0), frames.stride(1),
                                                              None if draws is None else draws.data_ptr()))
        self._pending = n
        self._hold(frames, draws)
        return frames

    def _check_draws(self, draws):
        if draws is not None:
            self._word_tensor(draws, 1, "draws")
            if draws.device != self.device:
                raise ValueError("draws must live on the stream's device")

    # ---- JPEG frames (dvo_knn_stream_process_jpeg / _detect_jpeg): see include/dvo.h -----------
    @property
    def jpeg_decoder(self):
        """The stream's ops.JpegDecoder (made at the first JPEG call); its status() tells which
        frames of the last JPEG call were corrupt, after a sync()."""
        if self._jpeg is None:
            from .ops import JpegDecoder
            group = min(int(self.max_frames), JpegDecoder.default_group_frames(self.width, self.height))
            self._jpeg = JpegDecoder(self.width, self.height, group_frames=group, ctx=self.ctx)
        return self._jpeg

    def _check_jpeg(self, blobs, undistort, entropy):
        from .ops import JPEG_ENTROPY, jpeg_blobs
        arrs, ptrs, lens = jpeg_blobs(blobs, self.max_frames)
        self._check_undistort(undistort)
        if entropy is not None and entropy not in JPEG_ENTROPY:
            raise ValueError(f"entropy must be one of {sorted(JPEG_ENTROPY)}")
        dec = self.jpeg_decoder
        if entropy is not None:
            dec.set_stream_entropy(entropy)
        return arrs, ptrs, lens, dec

    def process_jpeg(self, blobs, records: torch.Tensor | None = None, undistort=None, entropy=None) -> torch.Tensor:
        """process() of a list of JPEG files (bytes-like) of the stream's size, on a raw_input stream:
        decoded to gray on the device, and remapped by `undistort` (ops.Undistorter) if given, into
        the stream's slab.  entropy: "device" or "device_split" (ops.JpegDecoder.decode), kept for
        the calls that follow; None: as it is ("device" at first).  A frame with corrupt
        entropy-coded data does not fail the call: jpeg_decoder.status() names it."""
        arrs, ptrs, lens, dec = self._check_jpeg(blobs, undistort, entropy)
        n = len(arrs)
        if records is None:
            records = self.new_records(n - 1)
        self._after_torch()
        self._lm_fits(n - 1)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_process_jpeg(
            self.h, dec.h_, undistort.h_ if undistort is not None else None, ptrs, lens, n,
            records.data_ptr() if n > 1 else None))
        dec._n = n
        self._pending = 0
        self._hold(records, *self._lm_taken())
        return records

    def detect_jpeg(self, blobs, draws: torch.Tensor | None = None, undistort=None, entropy=None):
        """detect() of a list of JPEG files (see process_jpeg); finish() does the rest.  Returns the
        number of frames."""
        arrs, ptrs, lens, dec = self._check_jpeg(blobs, undistort, entropy)
        n = len(arrs)
        self._check_draws(draws)
        self._after_torch()
        self.ctx.check(self.ctx.lib.dvo_knn_stream_detect_jpeg(
            self.h, dec.h_, undistort.h_ if undistort is not None else None, ptrs, lens, n,
            None if draws is None else draws.data_ptr()))
        dec._n = n
        self._pending = n
        self._hold(draws)
        return n

    def finish(self, records: torch.Tensor | None = None, shard_draws: torch.Tensor | None = None, rank: int = 0,
               wait_torch: bool = True) -> torch.Tensor:
        """The second phase (dvo_knn_stream_finish, asynchronous): matching or forests, ratio test,
        geometry and the records of the frames detect() left pending.  shard_draws: a device tensor
        of one draws word per rank of a sharded stream (its length is the world size; entry
        [rank] is not read): a FLANN stream plans its pairs after the draws of the ranks below
        `rank` and leaves rng_state past the whole window; a BFMatcher stream ignores it.  With
        wait_torch the phase is ordered after work queued on torch's current stream (the zero-fill
        of new records, the collective that wrote shard_draws).  DVOError(DVO_EINVAL) when nothing
        is pending."""
        n = self._pending
        world = 1
        if shard_draws is not None:
            world = shard_draws.numel() if isinstance(shard_draws, torch.Tensor) else 0
            self._word_tensor(shard_draws, world, "shard_draws")
            if shard_draws.device != self.device:
                raise ValueError("shard_draws must live on the stream's device")
        if records is None:
            records = self.new_records(n - 1)
            wait_torch = True
        elif records.dtype != torch.uint8 or not records.is_cuda or not records.is_contiguous() \
                or records.numel() < max(n - 1, 0) * PAIR_RECORD_DTYPE.itemsize:
            raise ValueError(f"records must be a contiguous uint8 device tensor of {max(n - 1, 0)} records or more")
        if wait_torch:
            self._after_torch()
        self._lm_fits(n - 1)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_finish(self.h, records.data_ptr(),
                                                          None if shard_draws is None else shard_draws.data_ptr(),
                                                          int(world), int(rank)))
        self._pending = 0  # (a refused call leaves the detection pending)
        self._hold(records, shard_draws, *self._lm_taken())
        return records

    def sync(self):
        self.ctx.check(self.ctx.lib.dvo_knn_stream_sync(self.h))
        self._held.clear()

    records_numpy = staticmethod(FrameStream.records_numpy)

    def features(self, frame: int):
        """(keypoints KEYPOINT_DTYPE[N], descriptors float32[N, dim]) of frame `frame` of the last call."""
        from ._native import DVO_ECAP
        n = ctypes.c_int()
        rc = self.ctx.lib.dvo_knn_stream_get_features(self.h, int(frame), None, None, 0, ctypes.byref(n))
        if rc != DVO_ECAP:
            self.ctx.check(rc)
        kps = np.zeros(max(n.value, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(n.value, 1), self.dim), np.float32)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_get_features(self.h, int(frame), ptr(kps), ptr(desc), len(kps),
                                                                ctypes.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def matches(self, pair: int) -> np.ndarray:
        """Pair `pair`'s kept matches of the last call (DMATCH_DTYPE), in ascending queryIdx."""
        from ._native import DVO_ECAP
        m = ctypes.c_int()
        rc = self.ctx.lib.dvo_knn_stream_get_matches(self.h, int(pair), None, 0, ctypes.byref(m))
        if rc != DVO_ECAP:
            self.ctx.check(rc)
        out = np.zeros(max(m.value, 1), DMATCH_DTYPE)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_get_matches(self.h, int(pair), ptr(out), len(out), ctypes.byref(m)))
        return out[:m.value].copy()

    def set_profiling(self, enable: bool = True):
        self.ctx.check(self.ctx.lib.dvo_knn_stream_set_profiling(self.h, int(enable)))

    def stage_times(self):
        """Device ms of the last profiled call: detection, matching + ratio test, geometry + records."""
        ms = np.zeros(3, np.float64)
        self.ctx.check(self.ctx.lib.dvo_knn_stream_stage_times(self.h, ptr(ms)))
        return dict(zip(("detect", "match", "geometry"), ms.tolist()))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_knn_stream_destroy(self.h)  # synchronises the stream first
            self.h = None
            if getattr(self, "_jpeg", None) is not None:  # its work ran on the stream just synchronised
                self._jpeg.close()
                self._jpeg = None
            if getattr(self, "_held", None):
                self._held.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_side_streams = {}


@contextlib.contextmanager
def ordered_side_stream(device):
    """A HIP stream handle for a library call that must behave as if it ran on
    torch's current stream.  The C API reads a NULL stream as "the context's
    stream" (non-blocking, unordered with torch's default stream), so calls
    are made on a per-device side stream that waits for torch's current stream
    before the call, and that torch's current stream waits for after it."""
    cur = torch.cuda.current_stream(device)
    side = _side_streams.get(device)
    if side is None:
        side = _side_streams[device] = torch.cuda.Stream(device)
    side.wait_stream(cur)
    yield side.cuda_stream
    cur.wait_stream(side)


class PoseChain:
    """Absolute-pose chain T_abs[p] = T_abs[p-1] . T_rel[p] (v3:367) on the
    device (dvo_pose_chain) with a persistent carry: the reassembly step of a
    sharded pose stream (dist.ShardedPoseStream).  Runs on torch's current
    stream, where the all-gather that produced T_rel ran (ordered_side_stream)."""

    def __init__(self, ctx: Context | None = None, device: int | None = None, T0=None):
        self.ctx = ctx if ctx is not None else Context(0 if device is None else device)
        self.device = torch.device("cuda", self.ctx.device)
        self.carry = torch.empty(16, dtype=torch.float64, device=self.device)
        self.reset(T0)

    def reset(self, T0=None):
        T0 = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
        self.carry.copy_(torch.from_numpy(np.ascontiguousarray(T0).reshape(16)))

    def run(self, T_rel: torch.Tensor, T_abs: torch.Tensor | None = None) -> torch.Tensor:
        if T_rel.dtype != torch.float64 or not T_rel.is_cuda or not T_rel.is_contiguous():
            raise ValueError("T_rel must be a contiguous float64 [n, 4, 4] device tensor")
        n = T_rel.shape[0]
        if T_abs is None:
            T_abs = torch.empty((n, 4, 4), dtype=torch.float64, device=self.device)
        if T_abs.shape[0] < n or not T_abs.is_contiguous():
            raise ValueError("T_abs must be a contiguous float64 [>= n, 4, 4] device tensor")
        with ordered_side_stream(self.device) as st:
            self.ctx.check(self.ctx.lib.dvo_pose_chain(self.ctx.h, T_rel.data_ptr(), n, self.carry.data_ptr(),
                                                       T_abs.data_ptr(), st))
        return T_abs



class HostPoseChain:
    """The absolute chain T_abs[p] = T_abs[p-1] . T_rel[p] (v3:367) on a host thread
    (dvo_pose_chain_host, the device kernel's arithmetic bit for bit): rank 0 of a sharded stream
    (dist.ShardedStreamRunner).  submit(T_rel) copies the device T_rel into a pinned slot on
    torch's current stream and returns a Future of the window's T_abs (host, [n, 4, 4] float64);
    one worker thread chains the windows in submission order, waiting for each copy's event, while
    the GPU goes on with the next batches.  The carry (16 doubles) continues across windows."""

    def __init__(self, max_pairs: int, slots: int, device, T0=None):
        import concurrent.futures
        from ._native import load_library
        self.lib = load_library()
        self.device = torch.device(device)
        self.carry = np.ascontiguousarray(np.eye(4) if T0 is None else np.asarray(T0, np.float64)).reshape(16).copy()
        self.pinned = [torch.empty((max_pairs, 4, 4), dtype=torch.float64, pin_memory=True) for _ in range(slots)]
        self.pending = [None] * slots
        self.n = 0
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)

    def reset(self, T0=None):
        """The absolute pose before the next submitted window (default identity); waits for the
        windows already submitted, which chain on the old carry."""
        self.wait()
        self.carry[:] = np.asarray(np.eye(4) if T0 is None else T0, np.float64).reshape(16)

    def submit(self, T_rel: torch.Tensor):
        n = T_rel.shape[0]
        k = self.n % len(self.pinned)
        self.n += 1
        if self.pending[k] is not None:
            self.pending[k].result()  # the slot's previous chain has read its pinned buffer
        buf = self.pinned[k]
        buf[:n].copy_(T_rel, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))

        def work():
            ev.synchronize()
            out = np.empty((n, 4, 4), np.float64)
            src = buf[:n].numpy()
            rc = self.lib.dvo_pose_chain_host(src.ctypes.data, n, self.carry.ctypes.data, out.ctypes.data)
            if rc != 0:
                raise RuntimeError(f"dvo_pose_chain_host failed ({rc})")
            return out

        fut = self.pool.submit(work)
        self.pending[k] = fut
        return fut

    def wait(self):
        """Block until every submitted window is chained (raises a chain's error)."""
        for f in self.pending:
            if f is not None:
                f.result()

    def close(self):
        self.pool.shutdown(wait=True)


class PoseTail:
    """Pose tail over pair records (dvo_pose_tail_records): the marker-scaled
    relative poses (v3:309-345) and the absolute chain (v3:367) for records
    that arrive from elsewhere -- the reassembly step of a sharded pose stream
    (dist.ShardedPoseStream), run by rank 0 over the whole window in pair order.
    Same kernels and record fields as FrameStream.pose_tail, so the result is
    bit-identical to one rank's stream.  The carry (P_prev | T_abs) persists
    across calls on the device.  Runs on torch's current stream, where the
    all-gather that produced the records ran (ordered_side_stream)."""

    def __init__(self, K, marker_length: float, ctx: Context | None = None, device: int | None = None):
        self.ctx = ctx if ctx is not None else Context(0 if device is None else device)
        self.device = torch.device("cuda", self.ctx.device)
        self.K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        self.marker_length = float(marker_length)
        self.carry = torch.empty(28, dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self, P0=None, T0=None):
        """P_prev (3x4, default K[I|0] as in controlled mode, v3:164-166) and the
        absolute pose (4x4, default identity) before the next record."""
        P0 = self.K @ np.hstack((np.eye(3), np.zeros((3, 1)))) if P0 is None else np.asarray(P0, np.float64)
        T0 = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
        c = np.concatenate([np.asarray(P0, np.float64).reshape(12), np.asarray(T0, np.float64).reshape(16)])
        self.carry.copy_(torch.from_numpy(c))

    def run(self, records: torch.Tensor, corners_prev: torch.Tensor, corners_cur: torch.Tensor,
            T_rel: torch.Tensor | None = None, T_abs: torch.Tensor | None = None):
        """records: uint8 device tensor of n x 256 B; corners: float64 [n, k, 2]
        device tensors.  Returns (T_rel, T_abs) [n, 4, 4]."""
        rb = PAIR_RECORD_DTYPE.itemsize
        if records.dtype != torch.uint8 or not records.is_cuda or not records.is_contiguous() or records.numel() % rb:
            raise ValueError("records must be a contiguous uint8 device tensor of whole 256-B records")
        n = records.numel() // rb
        for c in (corners_prev, corners_cur):
            if c.dtype != torch.float64 or not c.is_cuda or not c.is_contiguous() or c.dim() != 3 \
                    or c.shape[0] != n or c.shape[2] != 2:
                raise ValueError(f"corners must be contiguous float64 [{n}, k, 2] device tensors")
        k = corners_prev.shape[1]
        if corners_cur.shape[1] != k:
            raise ValueError("previous and current corners differ in k")
        if T_rel is None:
            T_rel = torch.empty((n, 4, 4), dtype=torch.float64, device=self.device)
        if T_abs is None:
            T_abs = torch.empty((n, 4, 4), dtype=torch.float64, device=self.device)
        for T in (T_rel, T_abs):
            if T.dtype != torch.float64 or not T.is_contiguous() or T.shape[0] < n:
                raise ValueError(f"T_rel / T_abs must be contiguous float64 [>= {n}, 4, 4] device tensors")
        with ordered_side_stream(self.device) as st:
            self.ctx.check(self.ctx.lib.dvo_pose_tail_records(
                self.ctx.h, records.data_ptr(), n, ptr(self.K), corners_prev.data_ptr(), corners_cur.data_ptr(), k,
                self.marker_length, self.carry.data_ptr(), T_rel.data_ptr(), T_abs.data_ptr(), st))
        return T_rel, T_abs

    def rel_range(self, records: torch.Tensor, corners_prev: torch.Tensor, corners_cur: torch.Tensor, p0: int,
                  n: int, T_rel: torch.Tensor) -> torch.Tensor:
        """The pair-parallel half over pairs [p0, p0 + n) of a gathered window (dvo_pose_rel_range):
        T_rel[0 .. n), then the P_prev carry advanced past the whole window.  Every rank of a sharded
        stream runs it over its own pairs; rank 0 chains the gathered T_rel with chain()."""
        rb = PAIR_RECORD_DTYPE.itemsize
        pairs = records.numel() // rb
        k = corners_prev.shape[1]
        if corners_prev.shape[0] != pairs or corners_cur.shape[0] != pairs:
            raise ValueError("corners must cover the window's pairs")
        if T_rel.shape[0] < n or not T_rel.is_contiguous() or T_rel.dtype != torch.float64:
            raise ValueError("T_rel must be a contiguous float64 [>= n, 4, 4] device tensor")
        with ordered_side_stream(self.device) as st:
            self.ctx.check(self.ctx.lib.dvo_pose_rel_range(
                self.ctx.h, records.data_ptr(), pairs, int(p0), int(n), ptr(self.K), corners_prev.data_ptr(),
                corners_cur.data_ptr(), k, self.marker_length, self.carry.data_ptr(), T_rel.data_ptr(), st))
        return T_rel

    def chain(self, T_rel: torch.Tensor, T_abs: torch.Tensor, detached: bool = False) -> torch.Tensor:
        """The serial absolute chain (dvo_pose_chain) on this tail's T_abs carry.  detached: on the
        tail's own chain stream, after the work queued on torch's current stream so far, WITHOUT
        ordering torch's stream after it -- the chain (one wave's dependency chain over the
        window) then stays off the path of the next collectives; chains still run in call
        order.  Read T_abs after torch.cuda.synchronize() (or chain_event())."""
        n = T_rel.shape[0]
        if not detached:
            with ordered_side_stream(self.device) as st:
                self.ctx.check(self.ctx.lib.dvo_pose_chain(self.ctx.h, T_rel.data_ptr(), n,
                                                           self.carry.data_ptr() + 12 * 8, T_abs.data_ptr(), st))
            return T_abs
        if getattr(self, "_chain_stream", None) is None:
            self._chain_stream = torch.cuda.Stream(self.device)
        cs = self._chain_stream
        cs.wait_stream(torch.cuda.current_stream(self.device))
        self.ctx.check(self.ctx.lib.dvo_pose_chain(self.ctx.h, T_rel.data_ptr(), n, self.carry.data_ptr() + 12 * 8,
                                                   T_abs.data_ptr(), cs.cuda_stream))
        T_rel.record_stream(cs)  # torch's allocator keeps T_rel / T_abs until the chain has read / written them
        T_abs.record_stream(cs)
        return T_abs

    def chain_event(self):
        """An event after the detached chains queued so far (None if there were none)."""
        cs = getattr(self, "_chain_stream", None)
        if cs is None:
            return None
        ev = torch.cuda.Event()
        ev.record(cs)
        return ev
