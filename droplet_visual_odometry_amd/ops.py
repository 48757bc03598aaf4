"""numpy-level wrappers of the per-call C-ABI entry points (include/dvo.h).

Each function replaces one OpenCV operator of the reference's hot path and
mirrors its argument meaning, output layout and failure points:

  detect_and_compute   cv::ORB::detectAndCompute          visual_odometry_v3.py:373
  sift_detect_and_compute  cv::SIFT::detectAndCompute    visual_odometry_v3.py:100, :373
  SiftBatch            cv::SIFT::detectAndCompute of device-resident frames, a group per launch
                                                          visual_odometry_v3.py:373
  surf_detect_and_compute  xfeatures2d::SURF::detectAndCompute  visual_odometry_v3.py:104, :373
  SurfBatch            the same of device-resident frames, a group per launch
  bf_match             cv::BFMatcher(NORM_HAMMING).match  visual_odometry_v3.py:75, :219
  bf_knn_float         cv::BFMatcher(NORM_L1).knnMatch / .match, FLANN knnMatch
                                                          visual_odometry_v3.py:99-106, :200-215
  flann_knn            cv::FlannBasedMatcher(KDTREE).knnMatch  visual_odometry_v3.py:206-212
  KnnPairStream        detect + knnMatch + ratio test + E + recoverPose of one pair in the
                       knn_sift / surf / flann modes      visual_odometry_v3.py:373, :204-238, :297, :303
  stream.KnnFrameStream  the same for a batch of device-resident frames (matcher="bf" | "flann"; the
                       FLANN forests are built on the device: test_flann_batch, flann_rng_plan_host,
                       knn_stream_flann_bytes below; sharded across ranks by dist.ShardedKnnRunner, whose
                       theRNG hand-off flann_rng_shard_host repeats on the host)
  find_essential_mat   cv::findEssentialMat(RANSAC)       visual_odometry_v3.py:297-300
  recover_pose         cv::recoverPose                    visual_odometry_v3.py:303-306
  triangulate_points   cv::triangulatePoints              visual_odometry_v3.py:265
  get_optimal_new_camera_matrix, Undistorter
                       cv::getOptimalNewCameraMatrix, cv::undistort  v3:117, v3:120
  bgr2gray, bgr2gray_device
                       cv::cvtColor(COLOR_BGR2GRAY)       visual_odometry_v3.py:132
  JpegDecoder, jpeg_probe, jpeg_entropy_host, jpeg_entropy_split_host
                       cv::imdecode(IMREAD_COLOR) of baseline JPEGs  visual_odometry_v3.py:127
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import (DMATCH_DTYPE, DVO_ECAP, DVO_ECORRUPT, DVO_EINVAL, DVO_EUNSUPPORTED, DVO_OK, KEYPOINT_DTYPE, PAIR_RECORD_DTYPE, Context, DVOError, StreamConfig,
                      load_library, orb_params, ptr)


def _ctx(ctx):
    return ctx if ctx is not None else Context.default()


def detect_and_compute(img: np.ndarray, nfeatures: int = 500, fast_threshold: int = 20, opencv="4.x", ctx=None):
    """ORB keypoints (structured KEYPOINT_DTYPE array) and uint8[N, 32] descriptors.
    opencv: "4.x" (default) or "3.2" semantics (include/dvo.h DVO_OPENCV_*)."""
    c = _ctx(ctx)
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise DVOError(-1, "detect_and_compute expects a mono8 image (uint8[H, W])")
    h, w = img.shape
    prm = orb_params(nfeatures=nfeatures, fast_threshold=fast_threshold, opencv=opencv)
    cap = nfeatures + 512
    while True:
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = ctypes.c_int()
        rc = c.lib.dvo_orb_detect_and_compute(c.h, ctypes.byref(prm), ptr(img), w, h, img.strides[0], ptr(kps),
                                              ptr(desc), cap, ctypes.byref(n))
        if rc == DVO_ECAP and n.value > cap:
            cap = n.value
            continue
        c.check(rc)
        return kps[:n.value].copy(), desc[:n.value].copy()


def _check_nfeatures(nfeatures) -> int:
    """SIFT_create's nfeatures as the library takes it: an integer >= 0 (0 keeps everything)."""
    if isinstance(nfeatures, bool) or int(nfeatures) != nfeatures or int(nfeatures) < 0:
        raise DVOError(DVO_EINVAL, "nfeatures must be an integer >= 0")
    return int(nfeatures)


def sift_detect_and_compute(img: np.ndarray, ctx=None, nfeatures: int = 0):
    """SIFT_create(nfeatures).detectAndCompute(img, None): keypoints (KEYPOINT_DTYPE, in
    OpenCV's removeDuplicatedSorted order) and float32[N, 128] descriptors.  nfeatures > 0
    (dvo_sift_detect_and_compute_n): the keypoints OpenCV 4.x's retainBest keeps, in the order
    libstdc++'s nth_element + partition leave them; ties at the boundary response are all kept,
    so N can exceed nfeatures."""
    c = _ctx(ctx)
    nfeatures = _check_nfeatures(nfeatures)
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise DVOError(-1, "sift_detect_and_compute expects a mono8 image (uint8[H, W])")
    h, w = img.shape
    cap = 8192
    while True:
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 128), np.float32)
        n = ctypes.c_int()
        rc = c.lib.dvo_sift_detect_and_compute_n(c.h, ptr(img), w, h, img.strides[0], nfeatures, ptr(kps), ptr(desc),
                                                 cap, ctypes.byref(n))
        if rc == DVO_ECAP and n.value > cap:
            cap = n.value
            continue
        c.check(rc)
        return kps[:n.value].copy(), desc[:n.value].copy()


class SiftBatch:
    """SIFT_create().detectAndCompute (visual_odometry_v3.py:373) of device-resident frames of one
    size, `group` frames per launch (dvo_sift_batch_detect): every stage of the detector runs once
    over the group.  Every frame's features are bit-identical to sift_detect_and_compute's,
    whatever the group.  The scratch (scratch_bytes: about 83 MB per frame of the group at
    640x480) is allocated here, none in detect.  nfeatures > 0 (SIFT_create(nfeatures), also
    set_nfeatures): retainBest runs over the group before the descriptors, on each frame's whole
    list; the counts are then the kept counts, and retain_bytes(group) more bytes are allocated."""

    SIFT_LIST_CAP = 65536

    def __init__(self, width: int, height: int, group: int, ctx=None, nfeatures: int = 0):
        self.h = None
        self.ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_sift_batch_create(self.ctx.h, int(width), int(height), int(group),
                                                          ctypes.byref(h)))
        self.h = h
        self.width, self.height, self.group = int(width), int(height), int(group)
        self._ext = None
        self.nfeatures = 0
        if nfeatures:
            self.set_nfeatures(nfeatures)

    def set_nfeatures(self, nfeatures: int):
        """dvo_sift_batch_set_nfeatures: SIFT_create(nfeatures) for the detect calls that follow
        (0: everything is kept, and no retain launch)."""
        self.ctx.check(self.ctx.lib.dvo_sift_batch_set_nfeatures(self.h, _check_nfeatures(nfeatures)))
        self.nfeatures = int(nfeatures)

    @staticmethod
    def retain_bytes(group: int) -> int:
        """dvo_sift_retain_bytes: the extra device bytes of the retain stage for `group` frames
        (host arithmetic only; 0 for a group outside 1..64)."""
        return int(load_library().dvo_sift_retain_bytes(int(group)))

    @staticmethod
    def scratch_bytes(width: int, height: int, group: int) -> int:
        """dvo_sift_batch_bytes: the device bytes a SiftBatch of this size and group allocates
        (host arithmetic only; raises ValueError for arguments the constructor would reject)."""
        b = int(load_library().dvo_sift_batch_bytes(int(width), int(height), int(group)))
        if b < 0:
            raise ValueError("sides must be 1..4095 and group 1..64")
        return b

    def detect_device(self, frames, feat_cap: int, out=None):
        """The device form: frames uint8 [n, H, W] on the device (rows contiguous, any row pitch and
        frame stride) or a numpy array, which is uploaded.  Returns device tensors (keypoints uint8
        [n, feat_cap, 28] (KEYPOINT_DTYPE records), descriptors float32 [n, feat_cap, 128], counts
        int32 [n, 2]): frame f holds min(counts[f, 0], feat_cap) features, counts[f, 0] is the
        detector's count and counts[f, 1] its overflow flags.  Entries past a frame's count are
        not written.  out: contiguous tensors of at least those sizes to write into.  Nothing is
        read back; the work is ordered after torch's current stream, and torch's current stream
        after it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or frames.ndim != 3:
                raise ValueError("frames must be uint8 [n, H, W]")
            frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [n, H, W] device tensor or numpy array")
        n, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != detector {self.width}x{self.height}")
        if n and (frames.stride(2) != 1 or frames.stride(1) < w):
            raise ValueError("frames rows must be contiguous")
        cap = int(feat_cap)
        if out is None:
            out = (torch.empty((n, cap, KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                   torch.empty((n, cap, 128), dtype=torch.float32, device=dev),
                   torch.empty((n, 2), dtype=torch.int32, device=dev))
        kps, desc, counts = out
        for t, dt, need in ((kps, torch.uint8, n * cap * KEYPOINT_DTYPE.itemsize), (desc, torch.float32, n * cap * 128),
                            (counts, torch.int32, n * 2)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() < need:
                raise ValueError("out must hold contiguous device tensors: uint8 keypoints, float32 descriptors, "
                                 "int32 counts of at least n * feat_cap entries")
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(self.ctx.lib.dvo_sift_batch_hip_stream(self.h) or 0, device=dev)
        cur = torch.cuda.current_stream(dev)
        ev = torch.cuda.Event()
        ev.record(cur)
        self._ext.wait_event(ev)
        self.ctx.check(self.ctx.lib.dvo_sift_batch_detect(self.h, frames.data_ptr() if n else None, n, frames.stride(0),
                                                          frames.stride(1), cap, kps.data_ptr(), desc.data_ptr(),
                                                          counts.data_ptr()))
        cur.wait_stream(self._ext)
        return kps, desc, counts

    def detect(self, frames, feat_cap: int | None = None):
        """A list of (keypoints KEYPOINT_DTYPE[N], descriptors float32[N, 128]), one per frame.
        feat_cap: features kept per frame; a frame with more raises DVOError(DVO_ECAP), as
        KnnFrameStream.features does.  None: 8192, grown to the largest count if a frame has more."""
        cap = min(8192 if feat_cap is None else int(feat_cap), self.SIFT_LIST_CAP)
        while True:
            kps, desc, counts = self.detect_device(frames, cap)
            c = counts.cpu().numpy()
            if c[:, 1].any():
                raise DVOError(DVO_ECAP, "SIFT: more extrema / keypoints than the device lists hold")
            if c[:, 0].max() <= cap:
                break
            if feat_cap is not None:
                raise DVOError(DVO_ECAP, "a frame has more features than feat_cap")
            cap = int(c[:, 0].max())
        res = []
        for f, n in enumerate(c[:, 0].tolist()):
            k = kps[f, :n].cpu().numpy().reshape(-1).view(KEYPOINT_DTYPE).copy()
            res.append((k, desc[f, :n].cpu().numpy().copy()))
        return res

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_sift_batch_destroy(self.h)  # synchronises the stream first
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def surf_detect_and_compute(img: np.ndarray, hessian_threshold: float = 400.0, ctx=None):
    """xfeatures2d.SURF_create(hessian_threshold).detectAndCompute(img, None) on
    the GPU (dvo_surf_detect_and_compute): KEYPOINT_DTYPE array (OpenCV's
    KeypointGreater order) and float32[N, 64] descriptors."""
    c = _ctx(ctx)
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise DVOError(-1, "surf_detect_and_compute expects a mono8 image (uint8[H, W])")
    h, w = img.shape
    cap = 8192
    while True:
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 64), np.float32)
        n = ctypes.c_int()
        rc = c.lib.dvo_surf_detect_and_compute(c.h, ptr(img), w, h, img.strides[0], float(hessian_threshold), ptr(kps),
                                               ptr(desc), cap, ctypes.byref(n))
        if rc == DVO_ECAP and n.value > cap:
            cap = n.value
            continue
        c.check(rc)
        return kps[:n.value].copy(), desc[:n.value].copy()


class SurfBatch:
    """SURF_create(hessian_threshold).detectAndCompute (visual_odometry_v3.py:104, :373) of
    device-resident frames of one size, `group` frames per launch (dvo_surf_batch_detect): every
    stage of the detector runs once over the group.  Every frame's features are bit-identical to
    surf_detect_and_compute's, whatever the group.  The scratch (scratch_bytes: about 19 MB per
    frame of the group at 640x480) is allocated here, none in detect.  The threshold belongs to
    the call."""

    def __init__(self, width: int, height: int, group: int, ctx=None):
        self.h = None
        self.ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_surf_batch_create(self.ctx.h, int(width), int(height), int(group),
                                                          ctypes.byref(h)))
        self.h = h
        self.width, self.height, self.group = int(width), int(height), int(group)
        self.list_cap = max(4096, self.width * self.height // 64)  # the detector's keypoint list
        self._ext = None

    def set_nfeatures(self, nfeatures: int):
        """Refused: nfeatures is SIFT's (SiftBatch.set_nfeatures)."""
        raise DVOError(DVO_EINVAL, "nfeatures is SIFT's: OpenCV's SURF_create has no such parameter")

    @staticmethod
    def scratch_bytes(width: int, height: int, group: int) -> int:
        """dvo_surf_batch_bytes: the device bytes a SurfBatch of this size and group allocates
        (host arithmetic only; raises ValueError for arguments the constructor would reject)."""
        b = int(load_library().dvo_surf_batch_bytes(int(width), int(height), int(group)))
        if b < 0:
            raise ValueError("sides must be 1..4095 and group 1..64")
        return b

    def detect_device(self, frames, feat_cap: int, hessian_threshold: float = 400.0, out=None):
        """The device form: frames uint8 [n, H, W] on the device (rows contiguous, any row pitch and
        frame stride) or a numpy array, which is uploaded.  Returns device tensors (keypoints uint8
        [n, feat_cap, 28] (KEYPOINT_DTYPE records), descriptors float32 [n, feat_cap, 64], counts
        int32 [n, 2]): frame f holds min(counts[f, 0], feat_cap) features, counts[f, 0] is the
        detector's count and counts[f, 1] its flags (2: list overflow, 4: a window above 768).
        Entries past a frame's count are not written.  out: contiguous tensors of at least those
        sizes to write into.  Nothing is read back; the work is ordered after torch's current
        stream, and torch's current stream after it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or frames.ndim != 3:
                raise ValueError("frames must be uint8 [n, H, W]")
            frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 [n, H, W] device tensor or numpy array")
        n, h, w = frames.shape
        if (h, w) != (self.height, self.width):
            raise ValueError(f"frame size {w}x{h} != detector {self.width}x{self.height}")
        if n and (frames.stride(2) != 1 or frames.stride(1) < w):
            raise ValueError("frames rows must be contiguous")
        cap = int(feat_cap)
        if out is None:
            slots = max(cap, 0)  # a bad feat_cap is the library's to reject
            out = (torch.empty((n, slots, KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                   torch.empty((n, slots, 64), dtype=torch.float32, device=dev),
                   torch.empty((n, 2), dtype=torch.int32, device=dev))
        kps, desc, counts = out
        for t, dt, need in ((kps, torch.uint8, n * cap * KEYPOINT_DTYPE.itemsize), (desc, torch.float32, n * cap * 64),
                            (counts, torch.int32, n * 2)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() < need:
                raise ValueError("out must hold contiguous device tensors: uint8 keypoints, float32 descriptors, "
                                 "int32 counts of at least n * feat_cap entries")
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(self.ctx.lib.dvo_surf_batch_hip_stream(self.h) or 0, device=dev)
        cur = torch.cuda.current_stream(dev)
        ev = torch.cuda.Event()
        ev.record(cur)
        self._ext.wait_event(ev)
        self.ctx.check(self.ctx.lib.dvo_surf_batch_detect(self.h, frames.data_ptr() if n else None, n, frames.stride(0),
                                                          frames.stride(1), float(hessian_threshold), cap,
                                                          kps.data_ptr(), desc.data_ptr(), counts.data_ptr()))
        cur.wait_stream(self._ext)
        return kps, desc, counts

    def detect(self, frames, hessian_threshold: float = 400.0, feat_cap: int | None = None):
        """A list of (keypoints KEYPOINT_DTYPE[N], descriptors float32[N, 64]), one per frame.
        feat_cap: features kept per frame; a frame with more raises DVOError(DVO_ECAP), as
        KnnFrameStream.features does.  None: 8192, grown to the largest count if a frame has more."""
        cap = min(8192 if feat_cap is None else int(feat_cap), self.list_cap)
        while True:
            kps, desc, counts = self.detect_device(frames, cap, hessian_threshold)
            c = counts.cpu().numpy()
            if c[:, 1].any():
                raise DVOError(DVO_ECAP, "SURF: more keypoints than the device lists hold")
            if c[:, 0].max() <= cap:
                break
            if feat_cap is not None:
                raise DVOError(DVO_ECAP, "a frame has more features than feat_cap")
            cap = int(c[:, 0].max())
        res = []
        for f, n in enumerate(c[:, 0].tolist()):
            k = kps[f, :n].cpu().numpy().reshape(-1).view(KEYPOINT_DTYPE).copy()
            res.append((k, desc[f, :n].cpu().numpy().copy()))
        return res

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_surf_batch_destroy(self.h)  # synchronises the stream first
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bf_match(dq: np.ndarray, dt: np.ndarray, cross_check: int = 1, ctx=None) -> np.ndarray:
    """DMATCH_DTYPE array in queryIdx order (OpenCV's output order)."""
    c = _ctx(ctx)
    dq = np.ascontiguousarray(dq, np.uint8).reshape(-1, 32)
    dt = np.ascontiguousarray(dt, np.uint8).reshape(-1, 32)
    out = np.zeros(max(len(dq), 1), DMATCH_DTYPE)
    m = ctypes.c_int()
    c.check(c.lib.dvo_bf_match_hamming(c.h, ptr(dq), len(dq), ptr(dt), len(dt), int(cross_check), ptr(out), len(out),
                                       ctypes.byref(m)))
    return out[:m.value].copy()


NORM_L1, NORM_L2SQR = 0, 1


def bf_knn_float(dq: np.ndarray, dt: np.ndarray, k: int = 2, norm: int = NORM_L1, ctx=None):
    """k nearest trains of each float query: (train_idx int32[nq, k], dist
    float32[nq, k]) in OpenCV's order (ascending distance, lower train index
    first on ties); -1 / FLT_MAX pad queries with fewer than k trains.
    norm NORM_L1 (BFMatcher(NORM_L1)) or NORM_L2SQR (FLANN's squared L2)."""
    c = _ctx(ctx)
    dq = np.ascontiguousarray(dq, np.float32)
    dt = np.ascontiguousarray(dt, np.float32)
    if dq.ndim != 2 or dt.ndim != 2 or (len(dt) and dt.shape[1] != dq.shape[1]):
        raise DVOError(-1, "descriptors must be float32[n, dim] with the same dim")
    nq, nt, dim = dq.shape[0], dt.shape[0], dq.shape[1]
    idx = np.zeros((max(nq, 1), k), np.int32)
    dist = np.zeros((max(nq, 1), k), np.float32)
    c.check(c.lib.dvo_bf_knn_float(c.h, ptr(dq), nq, ptr(dt), nt, dim, int(k), int(norm), ptr(idx), ptr(dist)))
    return idx[:nq].copy(), dist[:nq].copy()


def bf_knn_hamming(dq: np.ndarray, dt: np.ndarray, k: int = 2, tsplit: int = 0, ctx=None):
    """BFMatcher(NORM_HAMMING).knnMatch(dq, dt, k) on 32-byte descriptors, k 1 or 2: (train_idx
    int32[nq, k], dist float32[nq, k]) in OpenCV's order (ascending distance, lower train index
    first on ties); -1 / FLT_MAX where fewer than k trains exist.  tsplit (tests, timing): the
    train splits per query block, 0 = the library's choice; the result does not depend on it."""
    c = _ctx(ctx)
    dq = np.ascontiguousarray(dq, np.uint8).reshape(-1, 32)
    dt = np.ascontiguousarray(dt, np.uint8).reshape(-1, 32)
    nq, nt = len(dq), len(dt)
    idx = np.zeros((max(nq, 1), k), np.int32)
    dist = np.zeros((max(nq, 1), k), np.float32)
    if tsplit:
        c.check(c.lib.dvo_test_bf_knn_hamming(c.h, ptr(dq), nq, ptr(dt), nt, int(k), int(tsplit), ptr(idx), ptr(dist)))
    else:
        c.check(c.lib.dvo_bf_knn_hamming(c.h, ptr(dq), nq, ptr(dt), nt, int(k), ptr(idx), ptr(dist)))
    return idx[:nq].copy(), dist[:nq].copy()


THE_RNG_SEED = 0xFFFFFFFF  # cv::theRNG() of a fresh thread (cv::RNG() state)


def flann_knn(dq: np.ndarray, dt: np.ndarray, k: int = 2, trees: int = 5, checks: int = 50,
              rng_state: int = THE_RNG_SEED, ctx=None):
    """FlannBasedMatcher(KDTREE trees, checks).knnMatch(dq, dt, k) on the GPU
    (dvo_flann_knn): (train_idx int32[nq, k], squared L2 float32[nq, k], the
    cv::theRNG() state after the call).  The randomized kd-forest and its
    approximate search reproduce OpenCV's, given the theRNG state before."""
    c = _ctx(ctx)
    dq = np.ascontiguousarray(dq, np.float32)
    dt = np.ascontiguousarray(dt, np.float32)
    if dq.ndim != 2 or dt.ndim != 2 or (len(dt) and len(dq) and dt.shape[1] != dq.shape[1]):
        raise DVOError(-1, "descriptors must be float32[n, dim] with the same dim")
    nq, nt, dim = dq.shape[0], dt.shape[0], dq.shape[1] if dq.size else dt.shape[1]
    idx = np.zeros((max(nq, 1), k), np.int32)
    dist = np.zeros((max(nq, 1), k), np.float32)
    st = ctypes.c_uint64(int(rng_state))
    c.check(c.lib.dvo_flann_knn(c.h, ptr(dq), nq, ptr(dt), nt, dim, int(k), int(trees), int(checks), ctypes.byref(st),
                                ptr(idx), ptr(dist)))
    return idx[:nq].copy(), dist[:nq].copy(), int(st.value)


def _pts(p):
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 2))
    return p


def find_essential_mat(p1, p2, K, prob=0.999, threshold=1.0, max_iters=1000, ctx=None):
    """(E float64[3k, 3], mask uint8[M, 1]).  Raises DVOError where OpenCV returns an empty E."""
    c = _ctx(ctx)
    p1, p2 = _pts(p1), _pts(p2)
    if len(p1) != len(p2):
        raise DVOError(-1, "findEssentialMat: point arrays differ in length")
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    m = len(p1)
    E = np.zeros(90, np.float64)
    rows = ctypes.c_int()
    mask = np.zeros(max(m, 1), np.uint8)
    c.check(c.lib.dvo_find_essential_mat(c.h, ptr(p1), ptr(p2), m, ptr(K), float(prob), float(threshold),
                                         int(max_iters), ptr(E), ctypes.byref(rows), ptr(mask)))
    return E[:3 * rows.value].reshape(rows.value, 3).copy(), mask[:m].reshape(m, 1).copy()


def recover_pose(E, p1, p2, K, distance_thresh=50.0, mask=None, ctx=None):
    """(good, R float64[3,3], t float64[3,1], mask uint8[M,1] of 0/255)."""
    c = _ctx(ctx)
    E = np.ascontiguousarray(E, np.float64)
    if E.ndim != 2 or E.shape[1] != 3 or E.shape[0] != 3:
        raise DVOError(-1, "recoverPose: E must be 3x3")
    p1, p2 = _pts(p1), _pts(p2)
    m = len(p1)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    R = np.zeros(9, np.float64)
    t = np.zeros(3, np.float64)
    mo = np.zeros(max(m, 1), np.uint8)
    good = ctypes.c_int()
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1), np.uint8)
    c.check(c.lib.dvo_recover_pose(c.h, ptr(E), 3, ptr(p1), ptr(p2), m, ptr(K), float(distance_thresh), ptr(mk),
                                   ptr(R), ptr(t), ptr(mo), ctypes.byref(good)))
    return good.value, R.reshape(3, 3), t.reshape(3, 1), mo[:m].reshape(m, 1).copy()


def triangulate_points(P1, P2, x1, x2, ctx=None) -> np.ndarray:
    """float64[4, K] homogeneous points; x1/x2 are 2 x K (or K x 2 with channels)."""
    c = _ctx(ctx)
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    if x1.ndim == 2 and x1.shape[0] != 2 and x1.shape[1] == 2:
        x1, x2 = x1.T, x2.T
    x1 = np.ascontiguousarray(x1.reshape(2, -1))
    x2 = np.ascontiguousarray(x2.reshape(2, -1))
    k = x1.shape[1]
    X = np.zeros((4, k), np.float64)
    c.check(c.lib.dvo_triangulate_points(c.h, ptr(np.ascontiguousarray(P1, np.float64)),
                                         ptr(np.ascontiguousarray(P2, np.float64)), ptr(x1), ptr(x2), k, ptr(X)))
    return X


# ---- device test hooks --------------------------------------------------------
def test_retain_best(resp, n_points, depth=-1, opencv="4.x", ctx=None):
    from ._native import opencv_semantics
    c = _ctx(ctx)
    resp = np.ascontiguousarray(resp, np.float32)
    perm = np.zeros(max(len(resp), 1), np.int32)
    k = ctypes.c_int()
    c.check(c.lib.dvo_test_retain_best(c.h, ptr(resp), len(resp), int(n_points), int(depth),
                                       opencv_semantics(opencv), ptr(perm), ctypes.byref(k)))
    return perm[:k.value].copy()


def test_update_num_iters(p, eps, model_points, max_iters, ctx=None):
    c = _ctx(ctx)
    eps = np.ascontiguousarray(eps, np.float64)
    out = np.zeros(max(len(eps), 1), np.int32)
    c.check(c.lib.dvo_test_update_num_iters(c.h, float(p), ptr(eps), len(eps), int(model_points), int(max_iters),
                                            ptr(out)))
    return out[:len(eps)]


def test_ransac_subsets(m, n, ctx=None):
    """Device getSubset draws for n hypotheses over m correspondences (n x 5)."""
    c = _ctx(ctx)
    idx = np.zeros((n, 5), np.int32)
    c.check(c.lib.dvo_test_ransac_subsets(c.h, int(m), int(n), ptr(idx)))
    return idx


def test_ransac_replay(nmod, cnt, m, prob=0.999, max_iters=1000, ctx=None):
    """Device RANSAC bookkeeping: (iterations, niters, max good, best h, best model)."""
    c = _ctx(ctx)
    nmod = np.ascontiguousarray(nmod, np.int32)
    cnt = np.ascontiguousarray(cnt, np.int32).reshape(-1, 10)
    out = np.zeros(5, np.int32)
    c.check(c.lib.dvo_test_ransac_replay(c.h, ptr(nmod), ptr(cnt), len(nmod), int(m), float(prob), int(max_iters),
                                         ptr(out)))
    return tuple(int(v) for v in out)


RANSAC_SCHEDULES = {"CALL": 0, "BATCH_ONE": 1, "BATCH_ROUNDS": 2}  # include/dvo.h DVO_TEST_SCHED_*


def test_ransac_hypotheses(sets, K, n_hyp, schedule, threshold=1.0, prob=0.999, ctx=None):
    """Everything the production RANSAC kernels computed for the first n_hyp hypotheses of each
    point set of `sets` (a list of (p1, p2), m x 2 pixel coordinates each, m may be 0), launched
    together under `schedule` ("CALL": the per-call findEssentialMat, one set; "BATCH_ONE": the
    batch kernels as one round; "BATCH_ROUNDS": the stream's round schedule).  Returns a dict:
    subsets (P, n, 5), nmod (P, n) (-1: not evaluated), models (P, n, 10, 9), cnt (P, n, 10),
    state (P, 5) (iterations, niters, max good, best h, best model), bounds (the round bounds),
    and for the one-round schedules path (P, n) and parked (4,), else None."""
    c = _ctx(ctx)
    P = len(sets)
    ms = np.array([len(np.asarray(p1).reshape(-1, 2)) for p1, _ in sets], np.int32)
    stride = max(int(ms.max()) if P else 0, 1)
    pts = np.zeros((max(P, 1), stride, 4), np.float64)
    for k, (p1, p2) in enumerate(sets):
        pts[k, :ms[k], :2] = np.asarray(p1, np.float64).reshape(-1, 2)
        pts[k, :ms[k], 2:] = np.asarray(p2, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    n = int(n_hyp)
    out = {"subsets": np.zeros((P, n, 5), np.int32), "nmod": np.zeros((P, n), np.int32),
           "models": np.zeros((P, n, 10, 9), np.float64), "cnt": np.zeros((P, n, 10), np.int32),
           "state": np.zeros((P, 5), np.int32)}
    bounds = np.zeros(8, np.int32)
    nr = ctypes.c_int()
    path = np.zeros((P, n), np.int32)
    parked = np.zeros(4, np.int32)
    c.check(c.lib.dvo_test_ransac_hypotheses(c.h, ptr(pts), ptr(ms), P, stride, ptr(K), float(prob), float(threshold),
                                             n, RANSAC_SCHEDULES[schedule], ptr(out["subsets"]), ptr(out["nmod"]),
                                             ptr(out["models"]), ptr(out["cnt"]), ptr(out["state"]), ptr(bounds),
                                             ctypes.byref(nr), ptr(path), ptr(parked)))
    out["bounds"] = bounds[:nr.value].copy()
    one = schedule != "BATCH_ROUNDS"
    out["path"] = path if one else None
    out["parked"] = parked if one else None
    return out


def test_five_point(q1, q2, ctx=None):
    c = _ctx(ctx)
    q1 = np.ascontiguousarray(q1, np.float64).reshape(10)
    q2 = np.ascontiguousarray(q2, np.float64).reshape(10)
    models = np.zeros(90, np.float64)
    n = ctypes.c_int()
    c.check(c.lib.dvo_test_five_point(c.h, ptr(q1), ptr(q2), ptr(models), ctypes.byref(n)))
    return models[:9 * n.value].reshape(n.value, 3, 3).copy()


def test_sampson(E, pts, t, ctx=None):
    """Device f32 Sampson decision (1 / 0 / -1 undecided) and the f64 test, per point."""
    c = _ctx(ctx)
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 4)
    n = len(pts)
    dec = np.zeros(n, np.int8)
    ex = np.zeros(n, np.uint8)
    c.check(c.lib.dvo_test_sampson(c.h, ptr(E), ptr(pts), n, float(t), ptr(dec), ptr(ex)))
    return dec, ex.astype(bool)


# ---- image pre-processing (visual_odometry_v3.py:110-135) ----
def get_optimal_new_camera_matrix(K, dist, size, alpha=1.0, new_size=None) -> np.ndarray:
    """cv.getOptimalNewCameraMatrix(K, dist, size, alpha, new_size)[0] (v3:117)."""
    lib = load_library()
    d = np.ascontiguousarray(np.asarray(dist, np.float64).ravel())
    w, h = size
    nw, nh = (w, h) if new_size is None else new_size
    out = np.zeros(9, np.float64)
    rc = lib.dvo_get_optimal_new_camera_matrix(ptr(np.ascontiguousarray(K, np.float64).reshape(9)), ptr(d), len(d),
                                               int(w), int(h), float(alpha), int(nw), int(nh), ptr(out))
    if rc != DVO_OK:
        raise DVOError(rc, "getOptimalNewCameraMatrix: bad arguments (distortion needs 0, 4, 5, 8 or 12 values)")
    return out.reshape(3, 3)


def _colour_image(img) -> np.ndarray:
    """A host H x W x C colour image (uint8, C = 3 or 4: B, G, R first), rows contiguous."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"expected a uint8 [H, W, 3 or 4] colour image, got {img.dtype} {img.shape}")
    return np.ascontiguousarray(img)


def check_colour_frames(src, what="frames", size=None, owner=""):
    """(n, H, W, C) of a colour batch: a uint8 [n, H, W, C] torch device tensor, C = 3 or 4,
    with the channels of a pixel and the pixels of a row adjacent (stride(3) == 1,
    stride(2) == C, stride(1) >= W * C), of `owner`'s size = (W, H) if given.
    ValueError otherwise, before any library call."""
    import torch
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 4:
        raise ValueError(f"{what} must be a uint8 [n, H, W, C] device tensor")
    n, h, w, c = src.shape
    if c not in (3, 4):
        raise ValueError(f"{what} must have 3 or 4 channels (B, G, R first), got {c}")
    if src.stride(3) != 1 or src.stride(2) != c or src.stride(1) < w * c:
        raise ValueError(f"{what} must keep a pixel's channels and a row's pixels adjacent "
                         "(stride(3) == 1, stride(2) == C, stride(1) >= W * C)")
    if size is not None and (w, h) != tuple(size):
        raise ValueError(f"frame size {w}x{h} != {owner} size {size[0]}x{size[1]}")
    if not src.is_cuda:
        raise ValueError(f"{what} must be a device tensor")
    return n, h, w, c


def _check_gray_frames(dst, n, h, w, device):
    import torch
    if not isinstance(dst, torch.Tensor) or dst.dtype != torch.uint8 or dst.dim() != 3 \
            or tuple(dst.shape) != (n, h, w):
        raise ValueError(f"dst must be a uint8 [{n}, {h}, {w}] device tensor")
    if dst.stride(2) != 1 or dst.stride(1) < w:
        raise ValueError("dst rows must be contiguous")
    if dst.device != device:
        raise ValueError("dst must be on the frames' device")


def _on_stream(device, hip_stream, call):
    if hip_stream:
        call(hip_stream)
    else:
        from .stream import ordered_side_stream
        with ordered_side_stream(device) as st:
            call(st)


def bgr2gray(img: np.ndarray, ctx=None) -> np.ndarray:
    """cv.cvtColor(img, COLOR_BGR2GRAY) (v3:132) of a host H x W x C image (C = 3 or 4,
    B, G, R first; a fourth channel is ignored) on the GPU: H x W mono8."""
    img = _colour_image(img)
    h, w, ch = img.shape
    c = _ctx(ctx)
    out = np.empty((h, w), np.uint8)
    c.check(c.lib.dvo_bgr2gray_image(c.h, ptr(img), w, h, img.strides[0], ch, ptr(out), out.strides[0]))
    return out


def bgr2gray_device(src, dst, stream=None, ctx=None):
    """cv.cvtColor(COLOR_BGR2GRAY) (v3:132) of n device frames: uint8 torch tensors
    [n, H, W, C] -> [n, H, W] (which must not overlap), on `stream` (a non-NULL
    hipStream_t handle), by default ordered with torch's current stream."""
    n, h, w, ch = check_colour_frames(src, "src")
    _check_gray_frames(dst, n, h, w, src.device)
    c = ctx if ctx is not None else Context.default(src.device.index or 0)

    def call(st):
        c.check(c.lib.dvo_bgr2gray(c.h, src.data_ptr(), n, src.stride(0), src.stride(1), ch, w, h, dst.data_ptr(),
                                   dst.stride(0), dst.stride(1), ctypes.c_void_p(st)))
    _on_stream(src.device, stream, call)
    return dst


class Undistorter:
    """cv.undistort(img, K, dist, None, newK) (v3:120) with the remap table built
    once on the device.  image(): host in/out; apply(): device frames.  Both take
    colour input too (a trailing channel axis of 3 or 4: B, G, R first) and then
    return the undistorted GRAY image, cvtColor + undistort (v3:132-133) in one kernel."""

    def __init__(self, K, dist, newK, width: int, height: int, ctx=None):
        self.ctx = _ctx(ctx)
        self.w, self.h = int(width), int(height)
        d = np.ascontiguousarray(np.asarray(dist, np.float64).ravel())
        nk = None if newK is None else np.ascontiguousarray(newK, np.float64).reshape(9)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_undistort_create(self.ctx.h, ptr(np.ascontiguousarray(K, np.float64).reshape(9)),
                                                         ptr(d), len(d), ptr(nk), self.w, self.h, ctypes.byref(h)))
        self.h_ = h

    def _image_bgr(self, img) -> np.ndarray:
        img = _colour_image(img)
        if img.shape[:2] != (self.h, self.w):
            raise ValueError(f"image {img.shape[:2]} != undistorter size {(self.h, self.w)}")
        out = np.empty((self.h, self.w), np.uint8)
        self.ctx.check(self.ctx.lib.dvo_undistort_image_bgr(self.h_, ptr(img), img.strides[0], img.shape[2], ptr(out),
                                                            out.strides[0]))
        return out

    def _apply_bgr(self, src, dst, hip_stream):
        n, h, w, ch = check_colour_frames(src, "src", (self.w, self.h), "undistorter")
        _check_gray_frames(dst, n, h, w, src.device)

        def call(st):
            self.ctx.check(self.ctx.lib.dvo_undistort_apply_bgr(self.h_, src.data_ptr(), n, src.stride(0), src.stride(1),
                                                                ch, dst.data_ptr(), dst.stride(0), dst.stride(1),
                                                                ctypes.c_void_p(st)))
        _on_stream(src.device, hip_stream, call)

    def image(self, img: np.ndarray) -> np.ndarray:
        if np.ndim(img) == 3:  # H x W x C colour: the undistorted gray image
            return self._image_bgr(img)
        img = np.ascontiguousarray(img, np.uint8)
        if img.shape != (self.h, self.w):
            raise DVOError(-1, f"image {img.shape} != undistorter size {(self.h, self.w)}")
        out = np.empty_like(img)
        self.ctx.check(self.ctx.lib.dvo_undistort_image(self.h_, ptr(img), img.strides[0], ptr(out), out.strides[0]))
        return out

    def apply(self, src, dst, hip_stream=None):
        """Remap n device frames (uint8 torch tensors [n, H, W], rows contiguous)
        on `hip_stream` (a non-NULL hipStream_t handle), by default ordered
        with torch's current stream.  Colour frames [n, H, W, C] (C = 3 or 4) are
        converted and remapped in one kernel into the same [n, H, W] dst."""
        if src.dim() == 4:
            return self._apply_bgr(src, dst, hip_stream)
        n = src.shape[0]

        def call(st):
            self.ctx.check(self.ctx.lib.dvo_undistort_apply(self.h_, src.data_ptr(), n, src.stride(0), src.stride(1),
                                                            dst.data_ptr(), dst.stride(0), dst.stride(1),
                                                            ctypes.c_void_p(st)))
        if hip_stream:
            call(hip_stream)
        else:
            from .stream import ordered_side_stream
            with ordered_side_stream(src.device) as st:
                call(st)

    def map(self):
        xy = np.zeros((self.h, self.w, 2), np.int16)
        fr = np.zeros((self.h, self.w), np.uint16)
        self.ctx.check(self.ctx.lib.dvo_undistort_get_map(self.h_, ptr(xy), ptr(fr)))
        return xy, fr

    def close(self):
        if getattr(self, "h_", None):
            self.ctx.lib.dvo_undistort_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- JPEG frames: cv.imdecode(np_arr, IMREAD_COLOR) (v3:127) of baseline JPEGs ----
JPEG_COLORS = {"gray": 1, "bgr": 3, "bgra": 4}
JPEG_ENTROPY = {"host": 0, "device": 1, "device_split": 2}
# the faster of the two at 256 frames of 1280x720 4:2:0 without restart markers (tools/time_jpeg.py)
JPEG_DEFAULT_ENTROPY = "device"
JPEG_SPLIT_BYTES_DEFAULT = 256  # include/dvo.h's DVO_JPEG_SPLIT_BYTES_DEFAULT: scan bytes per lane of "device_split"


def jpeg_blobs(blobs, max_frames=None):
    """A batch of JPEG files as (uint8 arrays, pointer array, length array): a non-empty
    list of bytes-like objects (bytes, bytearray, memoryview, uint8 numpy arrays).
    ValueError otherwise, before any library call."""
    if isinstance(blobs, (bytes, bytearray, memoryview, np.ndarray, str)) or not hasattr(blobs, "__len__"):
        raise ValueError("blobs must be a list of bytes-like JPEG files")
    if len(blobs) == 0:
        raise ValueError("blobs is empty")
    if max_frames is not None and len(blobs) > max_frames:
        raise ValueError(f"{len(blobs)} frames > the maximum of {max_frames}")
    arrs = []
    for i, b in enumerate(blobs):
        if isinstance(b, np.ndarray):
            if b.dtype != np.uint8 or b.ndim != 1:
                raise ValueError(f"blob {i}: expected a 1-D uint8 array")
            a = np.ascontiguousarray(b)
        elif isinstance(b, (bytes, bytearray, memoryview)):
            try:
                a = np.frombuffer(b, np.uint8)
            except (ValueError, TypeError) as e:
                raise ValueError(f"blob {i}: {e}") from e
        else:
            raise ValueError(f"blob {i}: not bytes-like ({type(b).__name__})")
        if a.size == 0:
            raise ValueError(f"blob {i} is empty")
        arrs.append(a)
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_int64 * len(arrs))(*[a.size for a in arrs])
    return arrs, ptrs, lens


def _jpeg_bytes(blob) -> np.ndarray:
    """One JPEG file as a uint8 array, without a copy where the object allows it."""
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob, np.uint8).ravel()
    return np.frombuffer(blob, np.uint8)


def _jpeg_error(rc):
    return DVOError(rc, "unsupported JPEG" if rc == DVO_EUNSUPPORTED else "corrupt JPEG")


def jpeg_probe(blob):
    """(width, height, components, sampling) of a JPEG header, on the host; sampling is the
    luma factors h << 4 | v.  DVOError with code DVO_EUNSUPPORTED or DVO_ECORRUPT otherwise."""
    lib = load_library()
    a = _jpeg_bytes(blob)
    w, h, nc, sm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.dvo_jpeg_probe(ptr(a), a.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(nc), ctypes.byref(sm))
    if rc != DVO_OK:
        raise _jpeg_error(rc)
    return w.value, h.value, nc.value, sm.value


def jpeg_entropy_host(blob):
    """Parser + Huffman decoder of one JPEG on the host (dvo_jpeg_entropy_host): the
    layout (_native.JpegLayout), the int16 coefficients and the entropy status."""
    from ._native import JpegLayout
    lib = load_library()
    a = _jpeg_bytes(blob)
    lay = JpegLayout()
    rc = lib.dvo_jpeg_entropy_host(ptr(a), a.size, ctypes.byref(lay), None, 0, None)
    if rc != DVO_OK:
        raise _jpeg_error(rc)
    coef = np.zeros(lay.coef_count, np.int16)
    st = ctypes.c_int()
    rc = lib.dvo_jpeg_entropy_host(ptr(a), a.size, ctypes.byref(lay), ptr(coef), coef.size, ctypes.byref(st))
    if rc != DVO_OK:
        raise DVOError(rc, "dvo_jpeg_entropy_host failed")
    return lay, coef, st.value


def jpeg_entropy_split_host(blob, split_bytes):
    """The host model of entropy="device_split" (dvo_jpeg_entropy_split_host): jpeg_entropy_host's
    coefficients and status by the split kernel's functions and schedule with `split_bytes`
    scan bytes per lane, and the most synchronisation passes a segment took."""
    from ._native import JpegLayout
    lib = load_library()
    a = _jpeg_bytes(blob)
    lay = JpegLayout()
    rc = lib.dvo_jpeg_entropy_host(ptr(a), a.size, ctypes.byref(lay), None, 0, None)
    if rc != DVO_OK:
        raise _jpeg_error(rc)
    coef = np.zeros(lay.coef_count, np.int16)
    st, passes = ctypes.c_int(), ctypes.c_int()
    rc = lib.dvo_jpeg_entropy_split_host(ptr(a), a.size, int(split_bytes), ptr(coef), coef.size, ctypes.byref(st),
                                         ctypes.byref(passes))
    if rc != DVO_OK:
        raise DVOError(rc, "dvo_jpeg_entropy_split_host failed")
    return coef, st.value, passes.value


class JpegDecoder:
    """cv.imdecode(buf, IMREAD_COLOR) (v3:127) of baseline JPEGs on the GPU, byte for
    byte libjpeg-turbo's default decode, for batches of frames of one size up to
    max_w x max_h.  Scratch (about 7 device and 5 pinned host bytes per pixel of a frame) is sized here for one
    group of `group_frames` frames; a batch runs group after group.  The device entropy
    decoder takes a group's restart segments one lane each: files without restart
    markers decode `group_frames` at a time, which is what the default is for.
    entropy="device_split" gives a long segment a workgroup instead, one lane per
    `split_bytes` bytes of it (a power of two in 16..4096; None: the library's default)."""

    @staticmethod
    def default_group_frames(max_w: int, max_h: int) -> int:
        """256 frames, fewer where that would take more than 2 GiB of device memory."""
        return max(1, min(256, (2 << 30) // (7 * int(max_w) * int(max_h))))

    def __init__(self, max_w: int, max_h: int, group_frames: int | None = None, ctx=None, split_bytes=None):
        self.ctx = _ctx(ctx)
        if group_frames is None:
            group_frames = self.default_group_frames(max_w, max_h)
        self.max_w, self.max_h, self.group_frames = int(max_w), int(max_h), int(group_frames)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_jpeg_create(self.ctx.h, self.max_w, self.max_h, self.group_frames,
                                                    ctypes.byref(h)))
        self.h_ = h
        self._n = 0
        if split_bytes is not None:
            self.split_bytes = split_bytes

    probe = staticmethod(jpeg_probe)

    @property
    def split_bytes(self) -> int:
        """Scan bytes per lane of entropy="device_split"."""
        v = ctypes.c_int()
        self.ctx.check(self.ctx.lib.dvo_jpeg_get_split(self.h_, ctypes.byref(v)))
        return v.value

    @split_bytes.setter
    def split_bytes(self, v):
        self.ctx.check(self.ctx.lib.dvo_jpeg_set_split(self.h_, int(v)))

    def set_stream_entropy(self, entropy):
        """The mode FrameStream.process_jpeg / submit_jpeg decode with: "device" or "device_split"."""
        if entropy not in JPEG_ENTROPY:
            raise ValueError(f"entropy must be one of {sorted(JPEG_ENTROPY)}")
        self.ctx.check(self.ctx.lib.dvo_jpeg_set_stream_entropy(self.h_, JPEG_ENTROPY[entropy]))

    def split_info(self):
        """Test hook, of the last "device_split" call: (most synchronisation passes of a
        segment, segments the split kernel took, of them decoded again by one lane)."""
        v = [ctypes.c_int() for _ in range(3)]
        self.ctx.check(self.ctx.lib.dvo_jpeg_get_split_info(self.h_, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def decode(self, blobs, color="gray", entropy=None, out=None, stream=None):
        """n JPEG files of one size -> a uint8 device tensor [n, H, W] (gray:
        cvtColor(BGR2GRAY) of the decoded bytes) or [n, H, W, 3 | 4] (bgr, bgra),
        asynchronously on `stream` (a hipStream_t handle; default: ordered with torch's
        current stream).  entropy: "device", "device_split" or "host" Huffman decoding
        (default JPEG_DEFAULT_ENTROPY).  status() tells which frames were corrupt."""
        import torch
        if color not in JPEG_COLORS:
            raise ValueError(f"color must be one of {sorted(JPEG_COLORS)}")
        entropy = JPEG_DEFAULT_ENTROPY if entropy is None else entropy
        if entropy not in JPEG_ENTROPY:
            raise ValueError(f"entropy must be one of {sorted(JPEG_ENTROPY)}")
        arrs, ptrs, lens = jpeg_blobs(blobs, 65536)
        ch = JPEG_COLORS[color]
        w, h, _, _ = jpeg_probe(arrs[0])
        n = len(arrs)
        shape = (n, h, w) if ch == 1 else (n, h, w, ch)
        dev = torch.device("cuda", self.ctx.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape \
                or not out.is_cuda or out.stride(-1) != 1 or (ch > 1 and out.stride(2) != ch) \
                or out.stride(1) < w * ch:
            raise ValueError(f"out must be a uint8 {list(shape)} device tensor with adjacent pixels")

        def call(st):
            self.ctx.check(self.ctx.lib.dvo_jpeg_decode(self.h_, ptrs, lens, n, ch, out.data_ptr(), out.stride(0),
                                                        out.stride(1), JPEG_ENTROPY[entropy], ctypes.c_void_p(st)))
        _on_stream(out.device, stream, call)
        self._n = n
        return out

    def decode_image(self, blob, color="bgr") -> np.ndarray:
        """One host JPEG -> a host image (H x W, or H x W x 3 | 4), synchronously."""
        if color not in JPEG_COLORS:
            raise ValueError(f"color must be one of {sorted(JPEG_COLORS)}")
        a = _jpeg_bytes(blob)
        w, h, _, _ = jpeg_probe(a)
        ch = JPEG_COLORS[color]
        out = np.empty((h, w) if ch == 1 else (h, w, ch), np.uint8)
        self.ctx.check(self.ctx.lib.dvo_jpeg_decode_image(self.h_, ptr(a), a.size, ch, ptr(out), out.strides[0]))
        self._n = 1
        return out

    def undistort_image(self, undistorter, blob) -> np.ndarray:
        """undistort(cvtColor(imdecode(blob))) (v3:127-133) of one host JPEG: mono8."""
        a = _jpeg_bytes(blob)
        out = np.empty((undistorter.h, undistorter.w), np.uint8)
        self.ctx.check(self.ctx.lib.dvo_undistort_image_jpeg(undistorter.h_, self.h_, ptr(a), a.size, ptr(out),
                                                             out.strides[0]))
        self._n = 1
        return out

    def status(self, n=None) -> np.ndarray:
        """Per frame of the last call, after synchronising: 0 or DVO_ECORRUPT."""
        n = self._n if n is None else int(n)
        st = np.zeros(n, np.int32)
        self.ctx.check(self.ctx.lib.dvo_jpeg_status(self.h_, ptr(st), n))
        return st

    def coefficients(self, frame: int) -> np.ndarray:
        """Test hook: the coefficients of a frame of the last group decoded."""
        n = ctypes.c_int64()
        out = np.zeros(1, np.int16)
        rc = self.ctx.lib.dvo_jpeg_get_coefficients(self.h_, int(frame), ptr(out), 0, ctypes.byref(n))  # the count
        if rc != DVO_ECAP:
            self.ctx.check(rc)
        out = np.zeros(n.value, np.int16)
        self.ctx.check(self.ctx.lib.dvo_jpeg_get_coefficients(self.h_, int(frame), ptr(out), out.size, ctypes.byref(n)))
        return out

    def close(self):
        if getattr(self, "h_", None):
            self.ctx.lib.dvo_jpeg_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PairStream:
    """One pair of host frames per call through the whole per-pair path
    (dvo_stream_pair): detectAndCompute of both frames, BFMatcher.match with
    crossCheck, findEssentialMat(RANSAC, prob, threshold, maxIters) and
    recoverPose (visual_odometry_v3.py:384-408 up to v3:303) in one
    synchronous library call, the 256-B pair record back.  With
    reuse_prev=True the previous frame is the last call's current frame and
    only the current one is detected.  The drop-in's fused path (D7) uses it;
    no torch involved."""

    def __init__(self, width, height, K, nfeatures=500, fast_threshold=20, cross_check=1, opencv="4.x", prob=0.999,
                 threshold=1.0, max_iters=1000, dist_thresh=50.0, ctx=None, ratio=None):
        """ratio: None / 0 matches with cross_check; a ratio > 0 with knnMatch(k = 2) and the ratio
        test instead (set_ratio_test)."""
        self.ctx = _ctx(ctx)
        cfg = StreamConfig()
        cfg.width, cfg.height, cfg.max_frames = int(width), int(height), 2
        cfg.orb = orb_params(nfeatures=nfeatures, fast_threshold=fast_threshold, opencv=opencv)
        K = np.asarray(K, np.float64).reshape(9)
        for i in range(9):
            cfg.K[i] = float(K[i])
        cfg.prob, cfg.threshold, cfg.max_iters = float(prob), float(threshold), int(max_iters)
        cfg.cross_check, cfg.dist_thresh = int(cross_check), float(dist_thresh)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_stream_create(self.ctx.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.width, self.height = int(width), int(height)
        if ratio:
            self.set_ratio_test(ratio)

    def set_ratio_test(self, ratio):
        """Match later pairs with the Hamming 2-NN and `m.distance < ratio * n.distance`
        (dvo_stream_set_ratio_test); None / 0: back to cross_check."""
        self.ctx.check(self.ctx.lib.dvo_stream_set_ratio_test(self.h, float(ratio or 0.0)))

    def pair(self, prev_img, cur_img, reuse_prev=False) -> np.ndarray:
        cur = np.ascontiguousarray(cur_img, np.uint8)
        if cur.shape != (self.height, self.width):
            raise ValueError(f"frame shape {cur.shape} != {(self.height, self.width)}")
        prev = None
        if not reuse_prev:
            prev = np.ascontiguousarray(prev_img, np.uint8)
            if prev.shape != cur.shape:
                raise ValueError("previous and current frames differ in shape")
        rec = np.zeros(1, PAIR_RECORD_DTYPE)
        self.ctx.check(self.ctx.lib.dvo_stream_pair(self.h, ptr(prev), ptr(cur), self.width, int(bool(reuse_prev)),
                                                    ptr(rec)))
        return rec[0]

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def test_ratio_gather(idx, dist, kq, kt, ratio=0.75, squared=False, ctx=None):
    """Device ratio test + ordered keypoint gather (ratio_gather_kernel) on a matcher's
    k = 2 output: (pts float32[M, 4], matches DMATCH_DTYPE[M], missing_second flag)."""
    c = _ctx(ctx)
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 2)
    dist = np.ascontiguousarray(dist, np.float32).reshape(-1, 2)
    kq = np.ascontiguousarray(kq, KEYPOINT_DTYPE)
    kt = np.ascontiguousarray(kt, KEYPOINT_DTYPE)
    nq = len(idx)
    pts = np.zeros((max(nq, 1), 4), np.float32)
    matches = np.zeros(max(nq, 1), DMATCH_DTYPE)
    m, miss = ctypes.c_int(), ctypes.c_int()
    c.check(c.lib.dvo_test_ratio_gather(c.h, ptr(idx), ptr(dist), nq, ptr(kq), len(kq), ptr(kt), len(kt), float(ratio),
                                        int(bool(squared)), ptr(pts), ptr(matches), ctypes.byref(m), ctypes.byref(miss)))
    return pts[:m.value].copy(), matches[:m.value].copy(), bool(miss.value)


def test_knn_batch(desc, kps, counts, ranges=0, ratio=0.75, ctx=None):
    """The matching stages of dvo_knn_stream_process (frame state, byte pack, batched k-NN, batched
    ratio test and gather) on host arrays: desc float32[F, cap, dim] frame slots, kps
    KEYPOINT_DTYPE[F, cap], counts int[F]; pair p is frames p, p + 1; ranges = train ranges (0: the
    library's choice).  Returns a dict of per-pair arrays: idx int32[P, cap, 2], dist float32[P, cap, 2]
    (rows < nq of a pair are written), nmatch int32[P], matches DMATCH_DTYPE[P, cap], pts
    float32[P, cap, 4] (entries < nmatch), hdr int32[P, 4] (counts, flags, 0), missing int32[P], and
    ranges_used."""
    c = _ctx(ctx)
    desc = np.ascontiguousarray(desc, np.float32)
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    counts = np.ascontiguousarray(counts, np.int32)
    if desc.ndim != 3 or kps.shape != desc.shape[:2] or counts.shape != desc.shape[:1]:
        raise DVOError(-1, "desc float32[F, cap, dim], kps [F, cap] and counts [F] must agree")
    F, cap, dim = desc.shape
    P = max(F - 1, 1)
    out = dict(idx=np.zeros((P, cap, 2), np.int32), dist=np.zeros((P, cap, 2), np.float32),
               nmatch=np.zeros(P, np.int32), matches=np.zeros((P, cap), DMATCH_DTYPE),
               pts=np.zeros((P, cap, 4), np.float32), hdr=np.zeros((P, 4), np.int32), missing=np.zeros(P, np.int32))
    used = ctypes.c_int()
    c.check(c.lib.dvo_test_knn_batch(c.h, ptr(desc), ptr(kps), ptr(counts), F, cap, dim, int(ranges), float(ratio),
                                     ptr(out["idx"]), ptr(out["dist"]), ptr(out["nmatch"]), ptr(out["matches"]),
                                     ptr(out["pts"]), ptr(out["hdr"]), ptr(out["missing"]), ctypes.byref(used)))
    out["ranges_used"] = used.value
    return out


def test_hamming_ratio_batch(desc, kps, counts, ratio=0.75, ctx=None):
    """The ratio-mode match stage of FrameStream(ratio=) (Hamming 2-NN, ratio test, gather) and the
    pair statuses on host arrays: desc uint8[F, cap, 32] frame slots, kps KEYPOINT_DTYPE[F, cap],
    counts int[F] (0..cap); pair p is frames p (queries), p + 1 (trains).  Returns a dict of per-pair
    arrays: top2 int32[P, cap, 2] (packed distance << 16 | trainIdx of the nearest and the second, -1
    none), nmatch int32[P], matches DMATCH_DTYPE[P, cap] and pts float32[P, cap, 4] (entries <
    nmatch), status int32[P] (0 or DVO_ENOFEAT)."""
    c = _ctx(ctx)
    desc = np.ascontiguousarray(desc, np.uint8)
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    counts = np.ascontiguousarray(counts, np.int32)
    if desc.ndim != 3 or desc.shape[2] != 32 or kps.shape != desc.shape[:2] or counts.shape != desc.shape[:1]:
        raise DVOError(-1, "desc uint8[F, cap, 32], kps [F, cap] and counts [F] must agree")
    F, cap, _ = desc.shape
    P = max(F - 1, 1)
    out = dict(top2=np.zeros((P, cap, 2), np.int32), nmatch=np.zeros(P, np.int32),
               matches=np.zeros((P, cap), DMATCH_DTYPE), pts=np.zeros((P, cap, 4), np.float32),
               status=np.zeros(P, np.int32))
    c.check(c.lib.dvo_test_hamming_ratio_batch(c.h, ptr(desc), ptr(kps), ptr(counts), F, cap, float(ratio),
                                               ptr(out["top2"]), ptr(out["nmatch"]), ptr(out["matches"]),
                                               ptr(out["pts"]), ptr(out["status"])))
    return out


def test_landmarks(pts, m, K, cap, out=None, prob=0.999, threshold=1.0, max_iters=1000, dist_thresh=50.0, ctx=None):
    """The landmark kernels of the streams (stream.Landmarks) on host arrays: pts float32[P, stride, 4]
    pixel coordinates (x1, y1, x2, y2), m int[P] counts (5..stride).  findEssentialMat, the
    stream's retire and the landmarks of all pairs.  out: LANDMARK_DTYPE[P, cap] whose bytes the
    kernels leave alone outside the written slots (default zeros).  Returns (out, count int32[P],
    records PAIR_RECORD_DTYPE[P])."""
    from ._native import LANDMARK_DTYPE
    c = _ctx(ctx)
    pts = np.ascontiguousarray(pts, np.float32)
    m = np.ascontiguousarray(m, np.int32)
    if pts.ndim != 3 or pts.shape[2] != 4 or m.shape != pts.shape[:1]:
        raise DVOError(-1, "pts float32[P, stride, 4] and m [P] must agree")
    P, stride, _ = pts.shape
    out = np.zeros((P, cap), LANDMARK_DTYPE) if out is None else out
    if out.dtype != LANDMARK_DTYPE or out.shape != (P, cap) or not out.flags.c_contiguous:
        raise DVOError(-1, "out must be a contiguous LANDMARK_DTYPE[P, cap] array")
    count = np.zeros(P, np.int32)
    rec = np.zeros(P, PAIR_RECORD_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    c.check(c.lib.dvo_test_landmarks(c.h, ptr(pts), ptr(m), P, stride, ptr(K), float(prob), float(threshold),
                                     int(max_iters), float(dist_thresh), int(cap), ptr(out), ptr(count), ptr(rec)))
    return out, count, rec


def test_tracks(lm, count, mq, mt, m, rec, kp_cap, cap_out=None, link=None, ctx=None):
    """The track kernels of the streams (stream.Tracks) on host arrays: lm LANDMARK_DTYPE[P, cap] the
    full landmark lists (count int[P] of them, match ascending), mq / mt int32[P, stride] the match
    indices (m int[P] of them, each below kp_cap), rec PAIR_RECORD_DTYPE[P] (R and t are read).
    link: int32[P, cap_out] whose bytes the kernels leave alone outside the written slots (default
    -1; cap_out defaults to cap).  Returns (link, scale TRACK_SCALE_DTYPE[P])."""
    from ._native import LANDMARK_DTYPE, TRACK_SCALE_DTYPE
    c = _ctx(ctx)
    mq = np.ascontiguousarray(mq, np.int32)
    mt = np.ascontiguousarray(mt, np.int32)
    count = np.ascontiguousarray(count, np.int32)
    m = np.ascontiguousarray(m, np.int32)
    if (lm.dtype != LANDMARK_DTYPE or lm.ndim != 2 or not lm.flags.c_contiguous or mq.ndim != 2 or mq.shape != mt.shape
            or not (len(lm) == len(mq) == len(count) == len(m) == len(rec))):
        raise DVOError(-1, "lm LANDMARK_DTYPE[P, cap], mq / mt int32[P, stride], count, m and rec [P] must agree")
    rec = np.ascontiguousarray(rec, PAIR_RECORD_DTYPE)
    P, cap = lm.shape
    cap_out = cap if cap_out is None else int(cap_out)
    link = np.full((P, cap_out), -1, np.int32) if link is None else link
    if link.dtype != np.int32 or link.shape != (P, cap_out) or not link.flags.c_contiguous:
        raise DVOError(-1, "link must be a contiguous int32[P, cap_out] array")
    scale = np.zeros(P, TRACK_SCALE_DTYPE)
    c.check(c.lib.dvo_test_tracks(c.h, ptr(lm), ptr(count), ptr(mq), ptr(mt), ptr(m), ptr(rec), P, cap, mq.shape[1],
                                  int(kp_cap), cap_out, ptr(link), ptr(scale)))
    return link, scale


def test_track_poses(lm, count, mq, mt, m, rec, kp_cap, K, iters=10, huber_px=1.0, inlier_px=2.0, min_points=6,
                     cap_out=None, link=None, ctx=None):
    """test_tracks with the pose kernel (stream.TrackPoses): each landmark's x2, y2 are read too, K is
    the camera matrix and the four parameters are bind_track_poses's (zero or negative: the default).
    Returns (link, scale TRACK_SCALE_DTYPE[P], pose TRACK_POSE_DTYPE[P])."""
    from ._native import LANDMARK_DTYPE, TRACK_POSE_DTYPE, TRACK_SCALE_DTYPE
    c = _ctx(ctx)
    mq = np.ascontiguousarray(mq, np.int32)
    mt = np.ascontiguousarray(mt, np.int32)
    count = np.ascontiguousarray(count, np.int32)
    m = np.ascontiguousarray(m, np.int32)
    if (lm.dtype != LANDMARK_DTYPE or lm.ndim != 2 or not lm.flags.c_contiguous or mq.ndim != 2 or mq.shape != mt.shape
            or not (len(lm) == len(mq) == len(count) == len(m) == len(rec))):
        raise DVOError(-1, "lm LANDMARK_DTYPE[P, cap], mq / mt int32[P, stride], count, m and rec [P] must agree")
    rec = np.ascontiguousarray(rec, PAIR_RECORD_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    P, cap = lm.shape
    cap_out = cap if cap_out is None else int(cap_out)
    link = np.full((P, cap_out), -1, np.int32) if link is None else link
    if link.dtype != np.int32 or link.shape != (P, cap_out) or not link.flags.c_contiguous:
        raise DVOError(-1, "link must be a contiguous int32[P, cap_out] array")
    scale = np.zeros(P, TRACK_SCALE_DTYPE)
    pose = np.zeros(P, TRACK_POSE_DTYPE)
    c.check(c.lib.dvo_test_track_poses(c.h, ptr(lm), ptr(count), ptr(mq), ptr(mt), ptr(m), ptr(rec), P, cap,
                                       mq.shape[1], int(kp_cap), cap_out, ptr(K), int(iters), float(huber_px),
                                       float(inlier_px), int(min_points), ptr(link), ptr(scale), ptr(pose)))
    return link, scale, pose


def test_track_pnp(lm, count, mq, mt, m, rec, kp_cap, K, xy2, hyps=128, iters=10, huber_px=1.0, inlier_px=2.0,
                   min_points=6, seed=0, mask=None, pose_params=(10, 1.0, 2.0, 6), cap_out=None, link=None, ctx=None):
    """test_track_poses with the PnP kernels after it (stream.TrackPnP): xy2 float32[P, stride, 2] are
    the second-frame pixels of every match, the record's n_matches is taken as m, and hyps, iters,
    huber_px, inlier_px, min_points, seed are bind_pnp's (zero or negative: the default; seed 0: the
    E-RANSAC's).  mask: uint8[P, mask_cap] whose bytes the kernels leave alone outside the written
    range, or None.  Returns (link, scale, pose, pnp TRACK_PNP_DTYPE[P], mask)."""
    from ._native import LANDMARK_DTYPE, TRACK_PNP_DTYPE, TRACK_POSE_DTYPE, TRACK_SCALE_DTYPE
    c = _ctx(ctx)
    mq = np.ascontiguousarray(mq, np.int32)
    mt = np.ascontiguousarray(mt, np.int32)
    count = np.ascontiguousarray(count, np.int32)
    m = np.ascontiguousarray(m, np.int32)
    if (lm.dtype != LANDMARK_DTYPE or lm.ndim != 2 or not lm.flags.c_contiguous or mq.ndim != 2 or mq.shape != mt.shape
            or not (len(lm) == len(mq) == len(count) == len(m) == len(rec))):
        raise DVOError(-1, "lm LANDMARK_DTYPE[P, cap], mq / mt int32[P, stride], count, m and rec [P] must agree")
    rec = np.ascontiguousarray(rec, PAIR_RECORD_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    P, cap = lm.shape
    xy2 = np.ascontiguousarray(xy2, np.float32)
    if xy2.shape != (P, mq.shape[1], 2):
        raise DVOError(-1, "xy2 must be float32[P, stride, 2]")
    cap_out = cap if cap_out is None else int(cap_out)
    link = np.full((P, cap_out), -1, np.int32) if link is None else link
    if link.dtype != np.int32 or link.shape != (P, cap_out) or not link.flags.c_contiguous:
        raise DVOError(-1, "link must be a contiguous int32[P, cap_out] array")
    if mask is not None and (mask.dtype != np.uint8 or mask.ndim != 2 or len(mask) != P or not mask.flags.c_contiguous):
        raise DVOError(-1, "mask must be a contiguous uint8[P, mask_cap] array")
    scale = np.zeros(P, TRACK_SCALE_DTYPE)
    pose = np.zeros(P, TRACK_POSE_DTYPE)
    pnp = np.zeros(P, TRACK_PNP_DTYPE)
    pi, ph, pin, pm = pose_params
    c.check(c.lib.dvo_test_track_pnp(c.h, ptr(lm), ptr(count), ptr(mq), ptr(mt), ptr(m), ptr(rec), P, cap, mq.shape[1],
                                     int(kp_cap), cap_out, ptr(K), int(pi), float(ph), float(pin), int(pm), ptr(link),
                                     ptr(scale), ptr(pose), ptr(xy2), int(hyps), int(iters), float(huber_px),
                                     float(inlier_px), int(min_points), int(seed), ptr(pnp),
                                     ptr(mask) if mask is not None else None,
                                     mask.shape[1] if mask is not None else 0))
    return link, scale, pose, pnp, mask


def track_pnp_samples(n, hyps=128, seed=0):
    """The PnP sample generator on the host (dvo_track_pnp_samples_host): int32[hyps, 3], a void sample -1."""
    from ._native import load_library
    out = np.zeros((int(hyps), 3), np.int32)
    rc = load_library().dvo_track_pnp_samples_host(int(n), int(hyps), int(seed), ptr(out))
    if rc != 0:
        raise DVOError(rc, "dvo_track_pnp_samples_host: n >= 1, hyps 1..512")
    return out


def p3p(Y, nunv):
    """The P3P solver on the host (dvo_p3p_host): Y [3, 3] points, nunv [3, 2] normalised pixels.
    Returns (R [n, 3, 3], t [n, 3]) of the n kept solutions."""
    import ctypes
    from ._native import load_library
    Y = np.ascontiguousarray(Y, np.float64).reshape(9)
    nunv = np.ascontiguousarray(nunv, np.float64).reshape(6)
    R, t, n = np.zeros((4, 9)), np.zeros((4, 3)), ctypes.c_int(0)
    rc = load_library().dvo_p3p_host(ptr(Y), ptr(nunv), ptr(R), ptr(t), ctypes.byref(n))
    if rc != 0:
        raise DVOError(rc, "dvo_p3p_host")
    return R[:n.value].reshape(-1, 3, 3), t[:n.value]


def test_track_refine(lm, count, mq, mt, m, rec, kp_cap, K, views=6, iters=5, huber_px=1.0, inlier_px=2.0,
                      use_poses=False, pose_params=(10, 1.0, 2.0, 6), cap_out=None, link=None, refined=None, ids=None,
                      want_refined=True, want_ids=True, ctx=None):
    """test_track_poses with the id and refine kernels (stream.RefinedLandmarks): each landmark's x1, y1
    are read too; views, iters, huber_px, inlier_px are bind_refine's (zero or negative: the default),
    use_poses whether the poses feed the unit motions, pose_params bind_track_poses's four.  refined
    LANDMARK_REFINED_DTYPE[P, cap_out] and ids TRACK_ID_DTYPE[P, cap_out] keep their bytes outside the
    written slots (default: 0xff fill); want_refined / want_ids False passes NULL for that output.
    Returns (link, scale, pose, refined or None, ids or None)."""
    from ._native import LANDMARK_DTYPE, LANDMARK_REFINED_DTYPE, TRACK_ID_DTYPE, TRACK_POSE_DTYPE, TRACK_SCALE_DTYPE
    c = _ctx(ctx)
    mq = np.ascontiguousarray(mq, np.int32)
    mt = np.ascontiguousarray(mt, np.int32)
    count = np.ascontiguousarray(count, np.int32)
    m = np.ascontiguousarray(m, np.int32)
    if (lm.dtype != LANDMARK_DTYPE or lm.ndim != 2 or not lm.flags.c_contiguous or mq.ndim != 2 or mq.shape != mt.shape
            or not (len(lm) == len(mq) == len(count) == len(m) == len(rec))):
        raise DVOError(-1, "lm LANDMARK_DTYPE[P, cap], mq / mt int32[P, stride], count, m and rec [P] must agree")
    rec = np.ascontiguousarray(rec, PAIR_RECORD_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    P, cap = lm.shape
    cap_out = cap if cap_out is None else int(cap_out)
    link = np.full((P, cap_out), -1, np.int32) if link is None else link
    if link.dtype != np.int32 or link.shape != (P, cap_out) or not link.flags.c_contiguous:
        raise DVOError(-1, "link must be a contiguous int32[P, cap_out] array")
    if want_refined and refined is None:
        refined = np.frombuffer(b"\xff" * (P * cap_out * 56), LANDMARK_REFINED_DTYPE).reshape(P, cap_out).copy()
    if want_ids and ids is None:
        ids = np.frombuffer(b"\xff" * (P * cap_out * 16), TRACK_ID_DTYPE).reshape(P, cap_out).copy()
    for arr, dt in ((refined, LANDMARK_REFINED_DTYPE), (ids, TRACK_ID_DTYPE)):
        if arr is not None and (arr.dtype != dt or arr.shape != (P, cap_out) or not arr.flags.c_contiguous):
            raise DVOError(-1, "refined / ids must be contiguous [P, cap_out] arrays of their dtypes")
    scale = np.zeros(P, TRACK_SCALE_DTYPE)
    pose = np.zeros(P, TRACK_POSE_DTYPE)
    pi, ph, pin, pm = pose_params
    c.check(c.lib.dvo_test_track_refine(c.h, ptr(lm), ptr(count), ptr(mq), ptr(mt), ptr(m), ptr(rec), P, cap,
                                        mq.shape[1], int(kp_cap), cap_out, ptr(K), int(pi), float(ph), float(pin),
                                        int(pm), ptr(link), ptr(scale), ptr(pose), int(views), int(iters),
                                        float(huber_px), float(inlier_px), int(bool(use_poses)),
                                        ptr(refined) if want_refined else None, ptr(ids) if want_ids else None))
    return link, scale, pose, refined if want_refined else None, ids if want_ids else None


def test_track_bundle(lm, count, mq, mt, m, rec, kp_cap, K, views=6, iters=5, lam=0.0, huber_px=1.0, inlier_px=2.0,
                      min_points=8, use_poses=False, pose_params=(10, 1.0, 2.0, 6), cap_out=None, link=None, bundle=None,
                      points=None, want_bundle=True, want_points=True, ctx=None):
    """test_track_poses with the bundle kernel (stream.TrackBundle) and no refine binding: each
    landmark's x1, y1 are read too; views, iters, lam, huber_px, inlier_px, min_points are
    bind_bundle's (zero or negative: the default), use_poses whether the poses feed the unit motions,
    pose_params bind_track_poses's four.  bundle TRACK_BUNDLE_DTYPE[P] and points
    LANDMARK_REFINED_DTYPE[P, cap_out] keep their bytes outside what is written (default: 0xff
    fill); want_bundle / want_points False passes NULL for that output.
    Returns (link, scale, pose, bundle or None, points or None)."""
    from ._native import (LANDMARK_DTYPE, LANDMARK_REFINED_DTYPE, TRACK_BUNDLE_DTYPE, TRACK_POSE_DTYPE,
                          TRACK_SCALE_DTYPE)
    c = _ctx(ctx)
    mq = np.ascontiguousarray(mq, np.int32)
    mt = np.ascontiguousarray(mt, np.int32)
    count = np.ascontiguousarray(count, np.int32)
    m = np.ascontiguousarray(m, np.int32)
    if (lm.dtype != LANDMARK_DTYPE or lm.ndim != 2 or not lm.flags.c_contiguous or mq.ndim != 2 or mq.shape != mt.shape
            or not (len(lm) == len(mq) == len(count) == len(m) == len(rec))):
        raise DVOError(-1, "lm LANDMARK_DTYPE[P, cap], mq / mt int32[P, stride], count, m and rec [P] must agree")
    rec = np.ascontiguousarray(rec, PAIR_RECORD_DTYPE)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    P, cap = lm.shape
    cap_out = cap if cap_out is None else int(cap_out)
    link = np.full((P, cap_out), -1, np.int32) if link is None else link
    if link.dtype != np.int32 or link.shape != (P, cap_out) or not link.flags.c_contiguous:
        raise DVOError(-1, "link must be a contiguous int32[P, cap_out] array")
    if want_bundle and bundle is None:
        bundle = np.frombuffer(b"\xff" * (P * 160), TRACK_BUNDLE_DTYPE).copy()
    if want_points and points is None:
        points = np.frombuffer(b"\xff" * (P * cap_out * 56), LANDMARK_REFINED_DTYPE).reshape(P, cap_out).copy()
    if bundle is not None and (bundle.dtype != TRACK_BUNDLE_DTYPE or bundle.shape != (P,) or not bundle.flags.c_contiguous):
        raise DVOError(-1, "bundle must be a contiguous TRACK_BUNDLE_DTYPE[P] array")
    if points is not None and (points.dtype != LANDMARK_REFINED_DTYPE or points.shape != (P, cap_out)
                               or not points.flags.c_contiguous):
        raise DVOError(-1, "points must be a contiguous LANDMARK_REFINED_DTYPE[P, cap_out] array")
    scale = np.zeros(P, TRACK_SCALE_DTYPE)
    pose = np.zeros(P, TRACK_POSE_DTYPE)
    pi, ph, pin, pm = pose_params
    c.check(c.lib.dvo_test_track_bundle(c.h, ptr(lm), ptr(count), ptr(mq), ptr(mt), ptr(m), ptr(rec), P, cap,
                                        mq.shape[1], int(kp_cap), cap_out, ptr(K), int(pi), float(ph), float(pin),
                                        int(pm), ptr(link), ptr(scale), ptr(pose), int(views), int(iters), float(lam),
                                        float(huber_px), float(inlier_px), int(min_points), int(bool(use_poses)),
                                        ptr(bundle) if want_bundle else None, ptr(points) if want_points else None))
    return link, scale, pose, bundle if want_bundle else None, points if want_points else None


def test_flann_batch(desc, counts, trees=5, checks=50, rng_state=None, levels=0, ctx=None):
    """The batched kd-forest build and search of dvo_knn_stream_process's FLANN mode
    (stream.KnnFrameStream(matcher="flann")) on host arrays: desc float32[F, cap, dim] frame slots,
    counts int[F] (a count above cap marks the frame); pair p is frames p (queries), p + 1 (trains);
    rng_state: the incoming theRNG state (default THE_RNG_SEED); levels: level launches per tree
    before the tail kernel (0: the library's choice).  Returns a dict: idx int32[P, cap, 2], dist
    float32[P, cap, 2] (squared L2; rows < nq of a built pair are written), starts uint64[P] (the
    state each pair starts from), state (after the call), n_global (queries that took the
    global-heap pass) and depth (the deepest tree level reached, counted from 1)."""
    c = _ctx(ctx)
    desc = np.ascontiguousarray(desc, np.float32)
    counts = np.ascontiguousarray(counts, np.int32)
    if desc.ndim != 3 or counts.shape != desc.shape[:1]:
        raise DVOError(-1, "desc float32[F, cap, dim] and counts [F] must agree")
    F, cap, dim = desc.shape
    P = max(F - 1, 1)
    out = dict(idx=np.zeros((P, cap, 2), np.int32), dist=np.zeros((P, cap, 2), np.float32), starts=np.zeros(P, np.uint64))
    st, ng, depth = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
    c.check(c.lib.dvo_test_flann_batch(c.h, ptr(desc), ptr(counts), F, cap, dim, int(trees), int(checks),
                                       ctypes.c_uint64(THE_RNG_SEED if rng_state is None else int(rng_state)),
                                       int(levels), ptr(out["idx"]), ptr(out["dist"]), ptr(out["starts"]),
                                       ctypes.byref(st), ctypes.byref(ng), ctypes.byref(depth)))
    out.update(state=int(st.value), n_global=ng.value, depth=depth.value)
    return out


def flann_rng_plan_host(counts, cap, trees=5, rng_state=THE_RNG_SEED):
    """The FLANN stream's RNG plan on the host (dvo_flann_rng_plan_host, the device kernel's text; no
    GPU needed): (starts uint64[F - 1], the state after the call) for detector counts counts[F]."""
    from ._native import load_library
    counts = np.ascontiguousarray(counts, np.int32)
    starts = np.zeros(max(len(counts) - 1, 1), np.uint64)
    st = ctypes.c_uint64()
    rc = load_library().dvo_flann_rng_plan_host(ctypes.c_uint64(int(rng_state)), ptr(counts), len(counts), int(cap),
                                                int(trees), ptr(starts), ctypes.byref(st))
    if rc:
        raise DVOError(rc, "dvo_flann_rng_plan_host: bad arguments")
    return starts[:len(counts) - 1].copy(), int(st.value)


def flann_rng_shard_host(counts, cap, trees=5, rng_state=THE_RNG_SEED, shard_draws=None, world=1, rank=0):
    """One rank's RNG plan of a sharded FLANN stream on the host (dvo_flann_rng_shard_host, the
    text of dvo_knn_stream_finish's plan; no GPU needed).  counts: the detector counts of the rank's
    frames (empty or one frame: a rank without pairs); shard_draws: every rank's draws word for
    the window (entry [rank] is not read; None: nothing before or after).  Returns (starts
    uint64[len(counts) - 1], the state after the whole window, the rank's own draws word)."""
    from ._native import load_library
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    starts = np.zeros(max(len(counts) - 1, 1), np.uint64)
    sd = None
    if shard_draws is not None:
        sd = np.ascontiguousarray(shard_draws, np.uint64).reshape(-1)
        if len(sd) != int(world):
            raise ValueError("shard_draws must hold one word per rank")
    st, own = ctypes.c_uint64(), ctypes.c_uint64()
    rc = load_library().dvo_flann_rng_shard_host(ctypes.c_uint64(int(rng_state)), ptr(counts) if len(counts) else None,
                                                 len(counts), int(cap), int(trees), None if sd is None else ptr(sd),
                                                 int(world), int(rank), ptr(starts), ctypes.byref(st), ctypes.byref(own))
    if rc:
        raise DVOError(rc, "dvo_flann_rng_shard_host: bad arguments")
    return starts[:max(len(counts) - 1, 0)].copy(), int(st.value), int(own.value)


def knn_stream_flann_bytes(max_frames, feat_cap, trees=5) -> int:
    """Device bytes stream.KnnFrameStream(matcher="flann") allocates beside the BF stream's
    (dvo_knn_stream_flann_bytes): P (84 C + 32 T C + 512 T + 20) + 512 C + 24 with P = max_frames - 1,
    C = feat_cap, T = trees; 0 for arguments out of range."""
    from ._native import load_library
    return int(load_library().dvo_knn_stream_flann_bytes(int(max_frames), int(feat_cap), int(trees)))


def knn_stream_raw_input_bytes(width, height, max_frames) -> int:
    """Device bytes stream.KnnFrameStream(raw_input=True) allocates beside the mono stream's
    (dvo_knn_stream_raw_input_bytes): the gray slab, max_frames * ((width + 15) & ~15) * height;
    0 for an argument below 1."""
    from ._native import load_library
    return int(load_library().dvo_knn_stream_raw_input_bytes(int(width), int(height), int(max_frames)))


KNN_DETECTORS = {"sift": 0, "surf": 1}
KNN_MATCHERS = {"bf": 0, "flann": 1}


class KnnPairStream:
    """One pair of host frames per call through the whole per-pair path of the
    k-NN modes (dvo_knn_pair_run): SIFT / SURF detectAndCompute of both frames,
    knnMatch(k=2) with BFMatcher(NORM_L1) or the FLANN kd-forest, the ratio test
    and keypoint gather, findEssentialMat(RANSAC) and recoverPose
    (visual_odometry_v3.py:384-408 up to v3:303) in one synchronous library
    call: one frame up, the 256-B pair record back.  With reuse_prev=True the
    previous frame is the last call's current frame (allowed after a pair whose
    record status is 0).  The drop-in's fused path (D8) uses it; no torch involved.
    nfeatures > 0 (SIFT only): SIFT_create(nfeatures), both frames' features are
    sift_detect_and_compute(img, nfeatures=N)'s."""

    def __init__(self, width, height, K, detector="sift", matcher="bf", hessian_threshold=400.0, trees=5, checks=50,
                 ratio=0.75, prob=0.999, threshold=1.0, max_iters=1000, dist_thresh=50.0, ctx=None, nfeatures=0):
        from ._native import KnnPairConfig
        self.ctx = _ctx(ctx)
        cfg = KnnPairConfig()
        cfg.width, cfg.height = int(width), int(height)
        cfg.detector = KNN_DETECTORS[detector] if isinstance(detector, str) else int(detector)
        cfg.matcher = KNN_MATCHERS[matcher] if isinstance(matcher, str) else int(matcher)
        cfg.hessian_threshold, cfg.trees, cfg.checks = float(hessian_threshold), int(trees), int(checks)
        cfg.ratio = float(ratio)
        K = np.asarray(K, np.float64).reshape(9)
        for i in range(9):
            cfg.K[i] = float(K[i])
        cfg.prob, cfg.threshold, cfg.max_iters = float(prob), float(threshold), int(max_iters)
        cfg.dist_thresh = float(dist_thresh)
        self.h = None
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dvo_knn_pair_create(self.ctx.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.width, self.height = int(width), int(height)
        self.dim = 64 if cfg.detector == 1 else 128
        self.flann = cfg.matcher == 1
        self.nfeatures = 0
        self._redetect = False
        if nfeatures:
            self.set_nfeatures(nfeatures)

    def set_nfeatures(self, nfeatures):
        """dvo_knn_pair_set_nfeatures: SIFT_create(nfeatures) for the pairs that follow.  A change
        drops the cached previous-frame features: the next pair(reuse_prev=True) must be given the
        previous frame too and detects it again.  DVOError(DVO_EINVAL) on a SURF handle."""
        n = _check_nfeatures(nfeatures)
        self.ctx.check(self.ctx.lib.dvo_knn_pair_set_nfeatures(self.h, n))
        if n != self.nfeatures:
            self._redetect = True
        self.nfeatures = n

    def pair(self, prev_img, cur_img, reuse_prev=False, rng_state=None):
        """(record, theRNG state after the call); rng_state: cv::theRNG()'s state before it
        (FLANN; default a fresh thread's)."""
        cur = np.ascontiguousarray(cur_img, np.uint8)
        if cur.shape != (self.height, self.width):
            raise ValueError(f"frame shape {cur.shape} != {(self.height, self.width)}")
        if reuse_prev and self._redetect:  # the cache holds features retained under another nfeatures
            if prev_img is None:
                raise DVOError(DVO_EINVAL, "nfeatures changed: pair(reuse_prev=True) needs the previous frame again")
            reuse_prev = False
        self._redetect = False
        prev = None
        if not reuse_prev:
            prev = np.ascontiguousarray(prev_img, np.uint8)
            if prev.shape != cur.shape:
                raise ValueError("previous and current frames differ in shape")
        rec = np.zeros(1, PAIR_RECORD_DTYPE)
        st = ctypes.c_uint64(THE_RNG_SEED if rng_state is None else int(rng_state))
        self.ctx.check(self.ctx.lib.dvo_knn_pair_run(self.h, ptr(prev), ptr(cur), self.width, int(bool(reuse_prev)),
                                                     ctypes.byref(st), ptr(rec)))
        return rec[0], int(st.value)

    def matches(self) -> np.ndarray:
        """The last pair's kept matches (DMATCH_DTYPE), in ascending queryIdx."""
        m = ctypes.c_int()
        rc = self.ctx.lib.dvo_knn_pair_get_matches(self.h, None, 0, ctypes.byref(m))
        if rc != DVO_ECAP:
            self.ctx.check(rc)
        out = np.zeros(max(m.value, 1), DMATCH_DTYPE)
        self.ctx.check(self.ctx.lib.dvo_knn_pair_get_matches(self.h, ptr(out), len(out), ctypes.byref(m)))
        return out[:m.value].copy()

    def features(self, which):
        """(keypoints KEYPOINT_DTYPE[N], descriptors float32[N, dim]) of the last pair's
        previous (which = 0) or current (1) frame."""
        n = ctypes.c_int()
        rc = self.ctx.lib.dvo_knn_pair_get_features(self.h, int(which), None, None, 0, ctypes.byref(n))
        if rc != DVO_ECAP:
            self.ctx.check(rc)
        kps = np.zeros(max(n.value, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(n.value, 1), self.dim), np.float32)
        self.ctx.check(self.ctx.lib.dvo_knn_pair_get_features(self.h, int(which), ptr(kps), ptr(desc), len(kps),
                                                              ctypes.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dvo_knn_pair_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
