/* droplet_visual_odometry_amd — C ABI of the MI355X visual-odometry front end.
 *
 * This is the drop-in boundary underneath the reference's Python call surface
 * (scripts/visual_odometry_v3.py, scripts/pose_estimation_module.py).  Each
 * per-call entry point replaces exactly one OpenCV operator the reference
 * invokes on its hot path; the batched stream API runs the whole per-pair path
 * (v3:384-408) for many frames per launch.  All compute runs in hand-written
 * HIP kernels for gfx950; there is no CPU fallback.
 *
 * Conventions: plain pointers and sizes, caller-owned outputs, int status
 * (DVO_OK or a negative DVO_E* code, message via dvo_last_error).  No C++
 * exceptions cross this boundary.  One context per host thread.
 */
#ifndef DVO_H_
#define DVO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVO_OK 0
#define DVO_EINVAL (-1)   /* bad argument (cv2.error analogue)                     */
#define DVO_ENOFEAT (-2)  /* no descriptors where the reference would hit None     */
#define DVO_EFEWPTS (-3)  /* fewer than 5 correspondences: findEssentialMat empty  */
#define DVO_EHIP (-4)     /* HIP runtime failure                                   */
#define DVO_ECAP (-5)     /* caller buffer too small; *_out holds the needed size  */
#define DVO_ENOMODEL (-6) /* RANSAC found no model (E empty)                       */
#define DVO_EUNSUPPORTED (-7) /* a legal JPEG outside the supported set            */
#define DVO_ECORRUPT (-8) /* malformed JPEG header or entropy-coded data           */

typedef struct dvo_ctx dvo_ctx;
typedef struct dvo_stream dvo_stream;
typedef struct dvo_undistort dvo_undistort;
typedef struct dvo_jpeg dvo_jpeg;

/* cv::KeyPoint as the reference's Python sees it (28 bytes). */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} dvo_keypoint;

/* cv::DMatch (16 bytes). */
typedef struct {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} dvo_dmatch;

/* OpenCV version whose ORB / BFMatcher semantics the path reproduces.  The
 * reference pins none (package.xml:21-30); its Python 2.7 .pyc files and ROS
 * Melodic docs point at OpenCV 3.2.  4.x is the default.
 * DVO_OPENCV_32: the pyramid is resize(INTER_LINEAR) with 11-bit weights and
 * the SSE2 vertical pass (4.x: INTER_LINEAR_EXACT), and retainBest runs
 * nth_element at n instead of n - 1; everything else is common to both. */
#define DVO_OPENCV_4X 0
#define DVO_OPENCV_32 1

/* cv.ORB_create() parameters (visual_odometry_v3.py:96 uses the defaults).
 * Only the defaults other than nfeatures are implemented; others -> DVO_EINVAL. */
typedef struct {
    int32_t nfeatures;      /* 500   */
    float scale_factor;     /* 1.2f  */
    int32_t nlevels;        /* 8     */
    int32_t edge_threshold; /* 31    */
    int32_t first_level;    /* 0     */
    int32_t wta_k;          /* 2     */
    int32_t score_type;     /* 0 = HARRIS_SCORE */
    int32_t patch_size;     /* 31    */
    int32_t fast_threshold; /* 20    */
    int32_t opencv_semantics; /* DVO_OPENCV_4X (0) or DVO_OPENCV_32 */
} dvo_orb_params;

int dvo_version(void);
/* Source hash the library was built from (16 hex digits; build.py source_hash). */
const char* dvo_build_id(void);
int dvo_ctx_create(dvo_ctx** out, int device);
void dvo_ctx_destroy(dvo_ctx* ctx);
const char* dvo_last_error(const dvo_ctx* ctx);

/* Replaces cv::ORB::detectAndCompute(img, None) — visual_odometry_v3.py:373.
 * img: host mono8, `stride` bytes per row.  Writes up to `cap` keypoints and
 * cap*32 descriptor bytes; *n_out = number found (DVO_ECAP if > cap). */
int dvo_orb_detect_and_compute(dvo_ctx* ctx, const dvo_orb_params* params, const uint8_t* img, int w, int h,
                               int stride, dvo_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Replaces cv::BFMatcher(NORM_HAMMING, crossCheck).match(query, train) —
 * visual_odometry_v3.py:75 (construction) and :219 (call).  Output in
 * queryIdx order, as OpenCV returns it.  cross_check: 0 off, 1 OpenCV 4.x
 * mutual nearest neighbour, 2 OpenCV 3.x reverse-pass semantics. */
int dvo_bf_match_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int cross_check,
                         dvo_dmatch* out, int cap, int* m_out);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, k) on 32-byte descriptors,
 * k 1 or 2, nq and nt 0..8192 as dvo_bf_match_hamming.  Per query, train_idx /
 * dist get k entries in OpenCV's order (ascending distance, lower train index
 * first on ties); -1 / FLT_MAX where fewer than k trains exist. */
int dvo_bf_knn_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int k, int32_t* train_idx,
                       float* dist);

/* Replaces cv::BFMatcher(NORM_L1).knnMatch(query, train, k) (k = 1: .match) on
 * float descriptors — the SIFT/SURF modes, visual_odometry_v3.py:99-106
 * (construction) and :200-204, :214-215 (calls) — and, with DVO_NORM_L2SQR,
 * serves cv::FlannBasedMatcher(KDTREE).knnMatch (:206-212) by exact search
 * (FLANN reports squared L2; its randomized kd-trees are approximate, so
 * exact results are the FLANN result whenever FLANN finds the true
 * neighbours).  dq: nq x dim, dt: nt x dim floats, dim 64 (SURF) or 128
 * (SIFT), k 1..4.  Per query, train_idx/dist get k entries in OpenCV's
 * order (ascending distance, lower train index first on ties); -1 / FLT_MAX
 * pad queries with fewer than k trains. */
#define DVO_NORM_L1 0
#define DVO_NORM_L2SQR 1
int dvo_bf_knn_float(dvo_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, int norm,
                     int32_t* train_idx, float* dist);

/* Replaces cv::FlannBasedMatcher(dict(algorithm=FLANN_INDEX_KDTREE, trees),
 * dict(checks)).knnMatch(query, train, k) on float descriptors — the 'flann'
 * mode, visual_odometry_v3.py:206-212 (trees 5, checks 50, k 2), whose ratio
 * test follows at :223-228.  OpenCV's randomized kd-forest (FLANN 1.6 as
 * bundled with OpenCV 4.x, restated in oracle/flann.cpp) is built over the
 * train set and searched approximately, on the device: the same trees, the
 * same visiting order, the same neighbours.  The trees are drawn from
 * cv::theRNG(), process state in the reference; *rng_state carries it: the
 * state before the call on entry (a fresh thread's is 0xFFFFFFFF) and after
 * it on return (advanced trees * (2 nt - 1) draws).  dist: squared L2 (as
 * FLANN reports it; FlannBasedMatcher returns its square root); per query k
 * entries ascending by (distance, train index).  dim a multiple of 4 up to
 * 256, k <= nt (else DVO_EINVAL, where FLANN asserts), nt <= 65536.  An empty
 * query or train set returns at once without touching the state. */
int dvo_flann_knn(dvo_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, int trees,
                  int checks, uint64_t* rng_state, int32_t* train_idx, float* dist);

/* Replaces cv::xfeatures2d::SIFT_create().detectAndCompute(img, None) — the
 * detector of the 'sift' / 'knn_sift' / 'flann' modes, visual_odometry_v3.py:100
 * (construction) and :373 (call).  Default parameters (nfeatures 0, 3 octave
 * layers, contrast 0.04, edge 10, sigma 1.6, input upscaled 2x).  img: host
 * mono8.  kps: keypoints in OpenCV's removeDuplicatedSorted order; desc: n x
 * 128 floats (integer values 0..255).  *n_out = count (DVO_ECAP if > cap). */
int dvo_sift_detect_and_compute(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, dvo_keypoint* kps,
                                float* desc, int cap, int* n_out);

/* cv::xfeatures2d::SIFT_create(nfeatures).detectAndCompute(img, None) (visual_odometry_v3.py:100
 * construction, :373 call) with the detector's first constructor argument; the other parameters
 * at their defaults.  nfeatures == 0 is dvo_sift_detect_and_compute.  nfeatures > 0: OpenCV 4.x's
 * KeyPointsFilter::retainBest(keypoints, nfeatures) runs on the device between
 * removeDuplicatedSorted and the descriptors: nothing where the list has at most nfeatures
 * entries; else libstdc++'s nth_element(begin, begin + nfeatures - 1, end, response >), the
 * boundary response read at nfeatures - 1, std::partition(begin + nfeatures, end, response >=
 * boundary), and the list cut there.  Keypoints and descriptors come out in the order those two
 * leave, not sorted by response, and every keypoint that ties with the boundary is kept, so the
 * count can exceed nfeatures (the extra orientations of an extremum share its response).  The
 * descriptors are computed for the kept keypoints only.  *n_out = the kept count (DVO_ECAP if >
 * cap).  The first call with nfeatures > 0 on a context allocates the retain stage's scratch,
 * dvo_sift_retain_bytes(1) bytes.  DVO_EINVAL: nfeatures < 0, and as dvo_sift_detect_and_compute. */
int dvo_sift_detect_and_compute_n(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, int nfeatures,
                                  dvo_keypoint* kps, float* desc, int cap, int* n_out);
/* The extra device bytes of the retain stage for `group` frames per launch (host only: no context,
 * no device; 0 for a group outside 1..64): per frame one keypoint list, the responses, their
 * positions and two position arrays of 65537, group * (65536 * (28 + 4 + 4) + 2 * 65537 * 4),
 * 2.9 MB a frame.  A handle whose nfeatures was never set allocates none of it.  (v3:100, :373) */
int64_t dvo_sift_retain_bytes(int group);

/* The same SIFT_create().detectAndCompute (visual_odometry_v3.py:373) for DEVICE-resident
 * frames of one size, a group of frames per launch: every stage of the detector (upscale, the
 * blurs, downsample, DoG, extrema, refine, sort, descriptor) is one launch over `group` frames,
 * the frame a grid dimension (a blur is one launch, row and column pass fused through LDS,
 * where the octave and the group are large enough to fill the card with its tiles, else two).
 * Keypoints and descriptors of every frame are bit-identical to dvo_sift_detect_and_compute's
 * whatever the group.
 *
 * dvo_sift_batch_create allocates the whole scratch (after synchronising the context's stream);
 * a detect call allocates nothing.  Bytes, which dvo_sift_batch_bytes returns (host only: no
 * context, no device; DVO_EINVAL for arguments create would reject), with S the sum over the
 * octaves of their pixels (octave 0 is 2w x 2h, each next one half of it, truncated; the octave
 * count is cvRound(log2(min(2w, 2h)) - 2) + 1, ended early where a side reaches 0):
 *   group * (4 * (6 S + 5 S + 2w * 2h)    Gaussian pyramid, DoG, row-pass buffer (floats)
 *            + 16 * 262144                candidate list (2^18 extrema)
 *            + 28 * 65536                 raw keypoint list
 *            + 4 * 65536                  sort scratch
 *            + 16)                        the frame's four counters
 *   + 400                                 one table of the 6 Gaussian kernels (11 + 11 + 13 + 17 + 21 + 27 taps)
 * which is 83.3 MB per frame of the group at 640 x 480 and 237.3 MB at 1280 x 720.
 *
 * dvo_sift_batch_detect: n_frames >= 1 mono8 frames on the device, frame f at d_frames +
 * f * frame_stride, rows `stride` >= w bytes apart, read in place.  Asynchronous on the context's
 * stream, nothing is read back; more frames than `group` run in chunks of `group` on that stream,
 * and the results do not depend on the group.  Frame f's keypoints go to d_kps + f * feat_cap
 * (removeDuplicatedSorted order), its descriptors to d_desc + f * feat_cap * 128, entries below
 * feat_cap only; d_counts[2 f] is the detector's count even where it exceeds feat_cap and
 * d_counts[2 f + 1] the detector's flags (1: more than 2^18 extrema, 2: more than 65536 raw
 * keypoints; a frame is complete when the flags are 0 and the count <= feat_cap).
 *
 * DVO_EINVAL, before any allocation: a side outside 1..4095, group outside 1..64; detect:
 * n_frames < 1, stride < w, feat_cap outside 1..65536, a null buffer. */
typedef struct dvo_sift_batch dvo_sift_batch;
int64_t dvo_sift_batch_bytes(int w, int h, int group);
int dvo_sift_batch_create(dvo_ctx* ctx, int w, int h, int group, dvo_sift_batch** out);
void dvo_sift_batch_destroy(dvo_sift_batch* b);
int dvo_sift_batch_detect(dvo_sift_batch* b, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          int feat_cap, dvo_keypoint* d_kps, float* d_desc, int32_t* d_counts);
/* The HIP stream the detect calls run on (the context's). */
void* dvo_sift_batch_hip_stream(dvo_sift_batch* b);
/* SIFT_create(nfeatures) (v3:100, :373) for the detect calls that follow: retainBest as in
 * dvo_sift_detect_and_compute_n, one more launch over the group between the sort and the
 * descriptors; 0 (the default) launches and allocates what the handle always did.  Retain sees a
 * frame's whole list, also where that is longer than feat_cap: d_counts[2 f] is the KEPT count,
 * and a frame is complete when that is <= feat_cap (give feat_cap = nfeatures plus room for
 * boundary ties).  Every frame's features equal dvo_sift_detect_and_compute_n's.  A setter that
 * changes the value to one > 0 synchronises the context's stream and allocates
 * dvo_sift_retain_bytes(group) bytes once; detect allocates nothing; dvo_sift_batch_bytes keeps
 * its value.  DVO_EINVAL: nfeatures < 0. */
int dvo_sift_batch_set_nfeatures(dvo_sift_batch* b, int nfeatures);

/* Replaces cv::xfeatures2d::SURF_create(hessianThreshold).detectAndCompute(img,
 * None) — the detector of the 'surf' mode, visual_odometry_v3.py:104
 * (SURF_create(400)) and :373 (call).  Other parameters at their defaults
 * (nOctaves 4, nOctaveLayers 3, extended false, upright false).  img: host
 * mono8.  kps: keypoints in OpenCV's KeypointGreater order (response, size,
 * octave descending, then y descending, x ascending), class_id = sign of the
 * Hessian trace; desc: n x 64 floats, unit norm.  *n_out = count (DVO_ECAP if
 * > cap). */
int dvo_surf_detect_and_compute(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, double hessian_threshold,
                                dvo_keypoint* kps, float* desc, int cap, int* n_out);

/* The same SURF_create(hessianThreshold).detectAndCompute (visual_odometry_v3.py:104, :373) for
 * DEVICE-resident frames of one size, a group of frames per launch: every stage of the detector
 * (the integral image's row and column scan, the Hessian layers, the extrema, the sort, the
 * descriptors, the compaction) is one launch over `group` frames, the frame a grid dimension.
 * Keypoints and descriptors of every frame are bit-identical to dvo_surf_detect_and_compute's
 * whatever the group.
 *
 * dvo_surf_batch_create allocates the whole scratch (after synchronising the context's stream);
 * a detect call allocates nothing.  Bytes, which dvo_surf_batch_bytes returns (host only: no
 * context, no device; DVO_EINVAL for arguments create would reject), with
 * cells = 5 * sum over o < 4 of (h >> o) * (w >> o), kp_cap = max(4096, w * h / 64) and n2 the
 * power of two >= kp_cap:
 *   group * (4 * (w + 1) * (h + 1)        integral image
 *            + 8 * cells                  det and trace of the 20 layers (floats), adjacent
 *            + 2 * 28 * kp_cap            raw and sorted keypoint lists
 *            + 256 * kp_cap               descriptors in sorted order
 *            + 4 * n2                     sort scratch
 *            + 16)                        the frame's counters
 *   + 4000 + 226 + 452                    one set of tables: 200 Haar boxes of 20 bytes, the 113
 *                                         orientation samples (2 bytes each) and their weights
 * which is 19.1 MB per frame of the group at 640 x 480 and 57.2 MB at 1280 x 720.
 *
 * dvo_surf_batch_detect: n_frames >= 1 mono8 frames on the device, frame f at d_frames +
 * f * frame_stride, rows `stride` >= w bytes apart, read in place.  hessian_threshold belongs to
 * the call, not to the handle.  Asynchronous on the context's stream, nothing is read back; more
 * frames than `group` run in chunks of `group` on that stream, and the results do not depend on
 * the group.  Frame f's keypoints go to d_kps + f * feat_cap (KeypointGreater order), its
 * descriptors to d_desc + f * feat_cap * 64, entries below feat_cap only; d_counts[2 f] is the
 * detector's count even where it exceeds feat_cap and d_counts[2 f + 1] the detector's flags
 * (2: more than kp_cap extrema, 4: a descriptor window above 768 pixels; a frame is complete
 * when the flags are 0 and the count <= feat_cap).
 *
 * DVO_EINVAL, before any allocation: a side outside 1..4095, group outside 1..64; detect:
 * n_frames < 1, stride < w, feat_cap outside 1..kp_cap, hessian_threshold not >= 0, a null
 * buffer or handle. */
typedef struct dvo_surf_batch dvo_surf_batch;
int64_t dvo_surf_batch_bytes(int w, int h, int group);
int dvo_surf_batch_create(dvo_ctx* ctx, int w, int h, int group, dvo_surf_batch** out);
void dvo_surf_batch_destroy(dvo_surf_batch* b);
int dvo_surf_batch_detect(dvo_surf_batch* b, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          double hessian_threshold, int feat_cap, dvo_keypoint* d_kps, float* d_desc,
                          int32_t* d_counts);
/* The HIP stream the detect calls run on (the context's). */
void* dvo_surf_batch_hip_stream(dvo_surf_batch* b);

/* Replaces cv::findEssentialMat(points1, points2, K, RANSAC, prob, threshold,
 * maxIters) — visual_odometry_v3.py:297-300.  p1/p2: m x 2 doubles (pixel
 * coords, the float32 KeyPoint_convert output widened).  E receives 3 rows
 * (or 3*k rows when m == 5, as OpenCV); cap 90 doubles.  mask: m bytes 0/1.
 * prob outside (0, 1), threshold non-finite or <= 0, max_iters < 1 -> DVO_EINVAL. */
int dvo_find_essential_mat(dvo_ctx* ctx, const double* p1, const double* p2, int m, const double* K, double prob,
                           double threshold, int max_iters, double* E, int* e_rows, uint8_t* mask);

/* Replaces cv::recoverPose(E, points1, points2, K, distanceThresh=50, mask) —
 * visual_odometry_v3.py:303-306.  R row-major 3x3, t unit 3-vector,
 * mask_out m bytes 0/255 (with mask_in: mask_in & that, byte for byte, as
 * OpenCV's bitwise_and), *good = cheirality count (the Python retval).  A
 * non-finite dist_thresh -> DVO_EINVAL. */
int dvo_recover_pose(dvo_ctx* ctx, const double* E, int e_rows, const double* p1, const double* p2, int m,
                     const double* K, double dist_thresh, const uint8_t* mask_in, double* R, double* t,
                     uint8_t* mask_out, int* good);

/* Replaces cv::triangulatePoints(P1, P2, x1, x2) — visual_odometry_v3.py:265.
 * P1/P2 row-major 3x4; x1/x2 2 x k row-major; X 4 x k row-major. */
int dvo_triangulate_points(dvo_ctx* ctx, const double* P1, const double* P2, const double* x1, const double* x2,
                           int k, double* X);

/* ---------------------------------------------------------------------------
 * Image pre-processing of ros_img_msg_to_opencv_image (visual_odometry_v3.py:110-135).
 * dist: k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] (ndist 0, 4, 5, 8 or 12). */

/* Replaces cv::getOptimalNewCameraMatrix(K, dist, (w, h), alpha, (new_w, new_h))
 * — visual_odometry_v3.py:117.  Host arithmetic; newK row-major 3x3. */
int dvo_get_optimal_new_camera_matrix(const double* K, const double* dist, int ndist, int w, int h, double alpha,
                                      int new_w, int new_h, double* newK);

/* Replaces cv::undistort(img, K, dist, None, newK) — visual_odometry_v3.py:120.
 * The remap table (OpenCV's striped initUndistortRectifyMap, CV_16SC2 + 1/32
 * fractions) is built once on the device; apply = remap(INTER_LINEAR,
 * BORDER_CONSTANT) of n device frames (dst may be a dvo_stream's input);
 * hip_stream NULL = the context's stream. newK NULL = K. */
int dvo_undistort_create(dvo_ctx* ctx, const double* K, const double* dist, int ndist, const double* newK, int w,
                         int h, dvo_undistort** out);
void dvo_undistort_destroy(dvo_undistort* u);
int dvo_undistort_apply(dvo_undistort* u, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch,
                        uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream);
/* Host image in, host image out (synchronous; the drop-in's cv.undistort). */
int dvo_undistort_image(dvo_undistort* u, const uint8_t* img, int stride, uint8_t* out, int out_stride);
/* Test hook: the device remap table (w*h*2 int16, w*h uint16). */
int dvo_undistort_get_map(dvo_undistort* u, int16_t* xy, uint16_t* frac);

/* Colour frames.  A colour image has `channels` = 3 or 4 bytes per pixel in B, G, R
 * order (a fourth byte is ignored); its rows hold w * channels bytes, `src_pitch`
 * (`stride`) bytes apart.  Gray is cv::cvtColor(COLOR_BGR2GRAY)'s 8-bit fixed point,
 *   Y = (B 1868 + G 9617 + R 4899 + 8192) >> 14.
 * Source and destination must not overlap.  Pitches need no alignment (4-byte
 * aligned rows take the wide loads).  DVO_EINVAL: channels not 3 or 4, src_pitch <
 * w * channels, dst_pitch < w, a null pointer with n > 0; n == 0 launches nothing. */
/* Replaces cv::cvtColor(image_np, COLOR_BGR2GRAY) — visual_odometry_v3.py:132 — for n
 * device frames (frame i at d_src + i * src_frame_stride -> d_dst + i * dst_frame_stride).
 * Asynchronous on hip_stream; NULL = the context's stream. */
int dvo_bgr2gray(dvo_ctx* ctx, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch, int channels,
                 int w, int h, uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream);
/* Replaces cv::cvtColor(image_np, COLOR_BGR2GRAY) — visual_odometry_v3.py:132.  Host
 * image in, host image out (synchronous; the counterpart of dvo_undistort_image). */
int dvo_bgr2gray_image(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, int channels, uint8_t* out,
                       int out_stride);
/* Replaces cv::cvtColor followed by cv::undistort — visual_odometry_v3.py:132-133 — in
 * one kernel: dvo_undistort_apply of the gray image of n colour device frames, byte for
 * byte, without storing that image (each bilinear tap is converted on its own; a tap
 * outside the source is gray 0 and is not read).  Frames are u's w x h. */
int dvo_undistort_apply_bgr(dvo_undistort* u, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch,
                            int channels, uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream);
/* Replaces cv::cvtColor followed by cv::undistort — visual_odometry_v3.py:132-133.
 * Host colour image in, host mono8 image out (synchronous; ros_img_msg_to_opencv_image). */
int dvo_undistort_image_bgr(dvo_undistort* u, const uint8_t* img, int stride, int channels, uint8_t* out,
                            int out_stride);

/* ---------------------------------------------------------------------------
 * Batched frame stream: the whole per-pair path of visual_odometry_calculations
 * (v3:384-408: detect both frames, match, E/RANSAC, recoverPose) for n_frames
 * device-resident frames -> n_frames-1 pair records, one launch sequence on the
 * stream's HIP stream.  Each frame is detected once and its features serve both
 * pairs it belongs to (identical outputs to re-detecting, v3:387-392). */
typedef struct {
    int32_t width, height, max_frames;
    dvo_orb_params orb;
    double K[9];
    double prob;        /* 0.999 */
    double threshold;   /* 1.0   */
    int32_t max_iters;  /* 1000  */
    int32_t cross_check;/* 1     */
    double dist_thresh; /* 50.0  */
} dvo_stream_config;

/* One pair's result, 256 bytes, gathered across ranks by RCCL all-gather. */
typedef struct {
    double R[9];
    double t[3];
    double E[9];
    int32_t n_kp_prev, n_kp_cur, n_matches, n_inliers;
    int32_t n_good, ransac_iters, status, n_models;
    int32_t n_hypotheses;  /* 5-point samples solved on the device (>= ransac_iters: rounds overshoot) */
    int32_t pad0;
    double reserved[6];
} dvo_pair_record;

/* prob, threshold, max_iters and dist_thresh are checked as in dvo_find_essential_mat /
 * dvo_recover_pose (DVO_EINVAL). */
int dvo_stream_create(dvo_ctx* ctx, const dvo_stream_config* cfg, dvo_stream** out);
void dvo_stream_destroy(dvo_stream* s);
/* d_frames: device pointer, frame i at d_frames + i*frame_stride, rows `stride`
 * bytes apart.  d_records: device pointer to n_frames-1 records.  Asynchronous
 * on the stream's HIP stream; call dvo_stream_sync before reading results. */
int dvo_stream_process(dvo_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                       dvo_pair_record* d_records);
int dvo_stream_sync(dvo_stream* s);
/* The reference's own schedule: visual_odometry_calculations (v3:384-408) runs
 * compute_current_image_elements on BOTH frames of every pair (v3:387-392), so
 * each frame is detected twice in a stream.  d_frames holds 2 n_pairs frames;
 * pair p is frames 2p (previous) and 2p + 1 (current), each detected on its own.
 * Records, matches and the pose tail are per pair exactly as after
 * dvo_stream_process (the pair's outputs are identical: detection is a function
 * of the frame).  2 n_pairs <= max_frames.  Used for the reference-equivalent
 * timing leg of bench.py. */
int dvo_stream_process_pairs(dvo_stream* s, const uint8_t* d_frames, int n_pairs, int64_t frame_stride, int stride,
                             dvo_pair_record* d_records);
/* Pipelined batches.  findEssentialMat's RANSAC loop (RANSACPointSetRegistrator::run,
 * the hot part of v3:297) runs in rounds of hypotheses, [0, 32), [32, 64), [64, 128),
 * [128, 256), then the rest up to the adaptive bound, each round stopping where the
 * sequential loop would (the result is the loop's, bit for bit, whatever the rounds).
 * dvo_stream_process runs a batch's rounds back to back.  dvo_stream_submit runs
 * detection and matching of its batch and then ONE merged round in which each of the
 * last dvo_pipeline_depth() submitted batches takes its next round; the batch whose last
 * round ran is retired (recoverPose, its records written), so a batch's records are
 * complete dvo_pipeline_depth() - 1 submits later, or after dvo_stream_drain.  The
 * records buffer and frames of every pending batch must stay allocated until then
 * (frames only until the submit's detection has run).  dvo_stream_retired lists the
 * batches the last submit / drain / process call retired, oldest first (their records
 * pointers and pair counts), returning how many; dvo_stream_pose_tail_batch runs the
 * pose tail over one of them.  Records are identical to dvo_stream_process's.
 * Footprint: the per-pair geometry (points, RANSAC models and state, pose buffers) is
 * held once per pair set, about 0.9 MB per pair at 1280x720, N 2000, maxIters 1000
 * (the models, max_iters x 720 B, dominate).  A stream is created with one set; its
 * first submit grows it to dvo_pipeline_depth() sets (synchronising the stream once),
 * so streams that only process / pair never pay for the pipeline.  If that grow runs out
 * of device memory the submit returns DVO_EHIP and the stream holds no pair set; it stays
 * usable: the next process / pair call allocates one set again, the next submit retries
 * the grow. */
int dvo_pipeline_depth(void);
int dvo_stream_submit(dvo_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                      dvo_pair_record* d_records);
int dvo_stream_submit_pairs(dvo_stream* s, const uint8_t* d_frames, int n_pairs, int64_t frame_stride, int stride,
                            dvo_pair_record* d_records);
int dvo_stream_drain(dvo_stream* s);
int dvo_stream_retired(dvo_stream* s, void** records, int* pairs, int cap);
/* One pair of HOST frames through the whole per-pair path in one synchronous
 * call: the device half of visual_odometry_calculations (v3:384-408) up to
 * recoverPose (v3:303) -- detectAndCompute of both frames (v3:387-392),
 * BFMatcher.match + crossCheck (v3:219), findEssentialMat(RANSAC, 0.999, 1.0)
 * (v3:297) and recoverPose (v3:303) -- returning the pair's record (R, t, E,
 * counts, status) in rec_out.  It replaces the drop-in's six separate operator
 * calls per pair (their host round trips and Python glue) with one; E, R and t
 * equal the operator-by-operator path's (the per-call RANSAC schedule: one
 * round, n_hypotheses as dvo_find_essential_mat).  reuse_prev = 1: the
 * previous frame is the last call's current frame, whose features the stream
 * kept on the device (prev_img may be NULL), so only cur_img is detected;
 * that cache is valid only after a call that returned DVO_OK (a failing call
 * invalidates it, and reuse_prev is then refused).  After a reuse_prev call,
 * dvo_stream_get_pyramid has frame 1 only (the previous frame's pyramid is not
 * kept); get_features has both frames.
 * Images: w x h mono8, rows `stride` bytes apart.  Needs max_frames >= 2. */
int dvo_stream_pair(dvo_stream* s, const uint8_t* prev_img, const uint8_t* cur_img, int stride, int reuse_prev,
                    dvo_pair_record* rec_out);
/* One pair of HOST frames through the whole per-pair path of the k-NN modes
 * ('knn_sift', 'surf', 'flann') in one synchronous call: the device half of
 * visual_odometry_calculations (v3:384-408) --
 *   detectAndCompute with SIFT or SURF (v3:373; construction v3:100, :104),
 *   knnMatch(k = 2) through BFMatcher(NORM_L1) (v3:204, :215) or the FLANN
 *     kd-forest (v3:206-212),
 *   the ratio test `m.distance < ratio * n.distance` and the keypoint gather
 *     (v3:223-238) with KeyPoint_convert (v3:355, :358), in ascending queryIdx
 *     order, evaluated as Python does: float32 distances (for FLANN the float32
 *     square root of its squared L2), double product, strict compare,
 *   findEssentialMat(RANSAC, prob, threshold) (v3:297) and recoverPose (v3:303)
 * -- returning the pair's record.  Descriptors, neighbour lists and kept points
 * never leave the device: one frame goes up, 256 bytes come back.  E, R, t and
 * the counts are those of the per-call operators (dvo_sift_ / dvo_surf_detect_and_compute,
 * dvo_bf_knn_float / dvo_flann_knn, dvo_find_essential_mat, dvo_recover_pose)
 * on the same frames.  Runs on the context's stream; synchronous at return.
 *
 * The handle keeps two feature slots (keypoints, descriptors, count at the
 * detector's list capacity).  reuse_prev = 1: the previous frame is the last
 * call's current frame (prev_img may be NULL) and only cur_img is detected.  That
 * is allowed only after a call that returned DVO_OK with record status DVO_OK; any
 * other call invalidates the cache and reuse_prev is then refused (DVO_EINVAL).
 *
 * Record: n_kp_prev / n_kp_cur are the detector counts, n_matches the kept
 * matches.  status DVO_ENOFEAT: a frame without keypoints (knnMatch on None
 * raises), fewer than 2 train descriptors or a query without a second
 * neighbour (`for m, n in matches` cannot unpack, v3:223); DVO_EFEWPTS: fewer
 * than 5 kept matches; the geometry's statuses otherwise.  The call returns
 * DVO_ECAP when a detector list overflowed.
 * rng_state (FLANN): cv::theRNG()'s state, in/out as in dvo_flann_knn; it
 * advances (trees * (2 n_kp_cur - 1) draws) only when the forest was built and
 * the call returned DVO_OK.  With DVO_MATCH_BF_L1 it may be NULL.
 * DVO_EINVAL (create, before any allocation): width / height outside 1..4095,
 * unknown detector or matcher, ratio not finite or <= 0, hessian_threshold < 0,
 * trees outside 1..64, checks < 1, and prob / threshold / max_iters /
 * dist_thresh as in dvo_find_essential_mat / dvo_recover_pose. */
typedef struct dvo_knn_pair dvo_knn_pair;
#define DVO_DETECT_SIFT 0
#define DVO_DETECT_SURF 1
#define DVO_MATCH_BF_L1 0
#define DVO_MATCH_FLANN 1
typedef struct {
    int32_t width, height;
    int32_t detector, matcher;
    double hessian_threshold;   /* SURF, 400 */
    int32_t trees, checks;      /* FLANN, 5 / 50 */
    double ratio;               /* 0.75 */
    double K[9];
    double prob, threshold; int32_t max_iters; double dist_thresh;
} dvo_knn_pair_config;
int dvo_knn_pair_create(dvo_ctx* ctx, const dvo_knn_pair_config* cfg, dvo_knn_pair** out);
void dvo_knn_pair_destroy(dvo_knn_pair* p);
/* SIFT_create(nfeatures) (v3:100, :373) for the runs that follow: both frames' features are
 * dvo_sift_detect_and_compute_n's (retainBest before the descriptors; FLANN's draws follow the
 * kept train count).  0 is the default.  A call that changes the value invalidates the cached
 * previous-frame features: the next dvo_knn_pair_run must detect both frames (reuse_prev is
 * DVO_EINVAL until a run succeeded), and allocates the context's retain scratch,
 * dvo_sift_retain_bytes(1) bytes, once.  A call that changes nothing does nothing.
 * DVO_EINVAL: a SURF handle (OpenCV's SURF_create has no such parameter), nfeatures < 0. */
int dvo_knn_pair_set_nfeatures(dvo_knn_pair* p, int nfeatures);
int dvo_knn_pair_run(dvo_knn_pair* p, const uint8_t* prev_img, const uint8_t* cur_img, int stride, int reuse_prev,
                     uint64_t* rng_state /* FLANN: in/out as dvo_flann_knn; else may be NULL */, dvo_pair_record* rec_out);
/* The last pair's kept matches (queryIdx, trainIdx, 0, distance), ascending queryIdx; *m = count (DVO_ECAP if > cap). */
int dvo_knn_pair_get_matches(dvo_knn_pair* p, dvo_dmatch* out, int cap, int* m);
/* The last pair's features: which 0 previous, 1 current frame; desc n x 128 (SIFT) or n x 64 (SURF) floats. */
int dvo_knn_pair_get_features(dvo_knn_pair* p, int which, dvo_keypoint* kps, float* desc, int cap, int* n);
/* The same per-pair path for a batch of DEVICE-resident frames in modes 'knn_sift' and
 * 'surf' (BFMatcher(NORM_L1)) and, after dvo_knn_stream_set_flann, 'flann': n_frames w x h mono8 frames, laid
 * out as for dvo_stream_process, give n_frames - 1 records on the device; pair p is
 * frames p (query, previous) and p + 1 (train, current), each frame detected once.
 * dvo_knn_stream_process is asynchronous on the context's stream (the detector's plan
 * and scratch belong to the context): it makes no host synchronisation and no
 * device-to-host copy, and its launch shapes depend on feat_cap, max_iters and n_frames
 * only; wait with dvo_knn_stream_sync.
 *
 * One call: the frames are detected one after another (SIFT / SURF as dvo_knn_pair_run,
 * in place on the caller's frames) into frame slots of feat_cap features; one launch
 * packs every frame's SIFT descriptors to bytes; the k-NN, ratio-test and gather
 * kernels take every pair in one launch each, with the counts read on the device;
 * findEssentialMat runs the stream's round schedule and recoverPose follows, so a
 * record does not depend on how the frames are split into calls.  Every field of a
 * record equals dvo_knn_pair_run's on the same two frames, except n_hypotheses
 * (the per-call path solves one round).
 *
 * Record status: as dvo_knn_pair_run (DVO_ENOFEAT: a frame without keypoints or
 * fewer than 2 train descriptors, with the counts and zeros elsewhere), and DVO_ECAP
 * for both pairs of a frame that has more features than feat_cap or whose detector
 * list overflowed (the call itself returns DVO_OK; such a frame brings no feature).
 *
 * Memory, all allocated at create (F = max_frames, P = F - 1, C = feat_cap, D = 128
 * SIFT / 64 SURF, H = max_iters), in bytes:
 *   frame slots  F (28 C + 4 D C + 16), SIFT also F (D C + 4 C + 4) (packed rows, norms, flag)
 *   match        P (48 C + 4) (neighbour lists, matches, point quads) + 16 C L, L the most
 *                (pair, range) partial lists a call can have (0 when no call splits the trains)
 *   geometry     P (32 C + 784 H + 1.5 K) (a dvo_stream's per-pair arrays)
 *                + 64 K per five-point block of the largest round + 12 per its hypotheses.
 * feat_cap = 0 takes the detector's list capacity (65536 SIFT, max(4096, w h / 64) SURF):
 * 44 MB per SIFT frame slot, so give the count you expect.
 *
 * DVO_EINVAL (create, before any allocation): as dvo_knn_pair_create, max_frames < 2 or
 * > 65536, feat_cap not 0 and outside 2..the detector's list capacity.  process:
 * n_frames outside 1..max_frames, stride < width, a null buffer.  n_frames == 1 detects
 * the frame and writes no record. */
typedef struct dvo_knn_stream dvo_knn_stream;
typedef struct {
    int32_t width, height, max_frames;
    int32_t detector;            /* DVO_DETECT_SIFT | DVO_DETECT_SURF */
    int32_t feat_cap;            /* features kept per frame; 0 = the detector's list capacity */
    double hessian_threshold;    /* SURF, 400 */
    double ratio;                /* 0.75 */
    double K[9];
    double prob, threshold; int32_t max_iters; double dist_thresh;
} dvo_knn_stream_config;
int dvo_knn_stream_create(dvo_ctx* ctx, const dvo_knn_stream_config* cfg, dvo_knn_stream** out);
void dvo_knn_stream_destroy(dvo_knn_stream* s);
int dvo_knn_stream_process(dvo_knn_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                           dvo_pair_record* d_records);
/* dvo_knn_stream_process in two phases, for a stream sharded across ranks (a collective runs
 * between them); process is detect(..., NULL) followed by finish(records, NULL, 1, 0) and launches
 * the same kernels.  Neither phase synchronises, reads back or allocates.
 *
 * detect: detection of the n_frames frames (frame by frame or through a group detector) and the
 * frame state.  With d_draws non-NULL (DEVICE memory, e.g. this rank's slot of an all-gather
 * buffer) one more kernel writes a 64-bit word there: the theRNG draws the call's pairs will
 * consume, the sum over its pairs of trees (2 nt - 1) for a pair that builds (nq >= 1, nt >= 2),
 * 0 on a BFMatcher stream.  The stream is then "detected, pending": dvo_knn_stream_get_features
 * works, dvo_knn_stream_get_matches does not until finish.  A detect while another is pending
 * replaces it.  DVO_EINVAL as process (d_records aside).
 *
 * finish: matching or forests, ratio test, geometry, records and the status rewrite of the pending
 * frames.  d_shard_draws NULL: exactly process's second half.  Non-NULL: `world` DEVICE words, the
 * draws word of every rank for this window (entry [rank] is never read); a FLANN stream's RNG plan
 * then starts from the stream's state jumped by pre = the sum of the entries below `rank` and
 * leaves the state jumped by pre + own + post, post = the sum of the entries above `rank` and own
 * counted from the frames, so every rank's state word is the state after the whole window, and
 * the window's records equal one stream's over all its frames.  A call with a single pending
 * frame has no pair and plans nothing, as in process: its state does not move, so a sharded
 * stream gives every rank at least one pair per window.  A BFMatcher stream ignores the array.  dvo_knn_stream_set_rng_state between the phases is allowed and ordered before the plan;
 * dvo_knn_stream_set_detect_group, _set_surf_group, _set_flann and (where it changes the value)
 * _set_nfeatures drop the pending detection.
 * dvo_knn_stream_stage_times keeps its three figures across the two calls (a collective the
 * caller orders between them counts into the matching figure).
 * DVO_EINVAL: nothing pending, world outside 1..1024, rank outside 0..world - 1, d_records NULL
 * with more than one pending frame. */
int dvo_knn_stream_detect(dvo_knn_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          uint64_t* d_draws);
int dvo_knn_stream_finish(dvo_knn_stream* s, dvo_pair_record* d_records, const uint64_t* d_shard_draws, int world,
                          int rank);
int dvo_knn_stream_sync(dvo_knn_stream* s);
/* The HIP stream the calls run on (the context's). */
void* dvo_knn_stream_hip_stream(dvo_knn_stream* s);
/* SIFT detection (v3:373) of the process calls that follow through the group detector
 * (dvo_sift_batch_detect's path): `group` frames per launch, written straight into the stream's
 * frame slots.  0 (the default) keeps the frame-by-frame detection.  Records, features and
 * matches are the same either way.  The setter synchronises the context's stream and allocates
 * (or frees) the group's scratch, dvo_sift_batch_bytes(width, height, group) bytes; process
 * allocates nothing.  DVO_EINVAL: a SURF stream, group outside 0..64. */
int dvo_knn_stream_set_detect_group(dvo_knn_stream* s, int group);
/* The same for a SURF stream (dvo_surf_batch_detect's path, with the stream's hessian_threshold):
 * `group` frames per launch straight into the frame slots, 0 (the default) frame by frame on the
 * context's plan, which a grouped process call does not touch.  Same records, features and
 * matches either way.  The setter synchronises the context's stream and allocates (or frees)
 * dvo_surf_batch_bytes(width, height, group) bytes.  DVO_EINVAL: a SIFT stream, group outside 0..64. */
int dvo_knn_stream_set_surf_group(dvo_knn_stream* s, int group);
/* SIFT_create(nfeatures) (v3:100, :373) for the detections that follow, in both routes: frame by
 * frame retainBest runs inside the context's detector, with a detect group inside the group
 * detector, where it sees a frame's whole list before anything is cut at feat_cap.  Every frame
 * slot then holds dvo_sift_detect_and_compute_n's features, a record's counts are the kept
 * counts, both matchers take the kept features (FLANN's draws follow the kept train counts, in one
 * call, in two phases and sharded), and a frame is DVO_ECAP only where its KEPT count exceeds
 * feat_cap: give feat_cap = nfeatures plus room for boundary ties.  0 (the default) launches and
 * allocates what the stream always did.  A call that changes the value drops a pending detection,
 * synchronises the context's stream and, for a value > 0, allocates the retain scratch once:
 * dvo_sift_retain_bytes(1) on the context and dvo_sift_retain_bytes(group) with a detect group
 * (dvo_knn_stream_set_detect_group allocates the latter when it follows).  A call that changes
 * nothing does nothing.  DVO_EINVAL: a SURF stream (OpenCV's SURF_create has no such parameter),
 * nfeatures < 0. */
int dvo_knn_stream_set_nfeatures(dvo_knn_stream* s, int nfeatures);
/* The 'flann' mode in the batch (v3:207-212: FlannBasedMatcher(KDTREE, trees = 5), checks = 50):
 * trees 1..64 with checks >= 1 makes the process calls that follow build the randomized
 * kd-forest of every pair's train frame and search k = 2 for every query on the device, in
 * place of BFMatcher; trees = 0 (the default) returns to BFMatcher and frees the scratch.  It
 * works for SIFT and SURF streams and together with the group detectors.  The setter
 * synchronises the context's stream and allocates everything the mode needs,
 * dvo_knn_stream_flann_bytes(max_frames, feat_cap, trees) bytes; process allocates nothing,
 * makes no host synchronisation and no device-to-host copy, and its 3 + trees (levels + 8)
 * forest launches (levels = 24 level launches per tree, then a tail kernel that finishes
 * deeper trees) have shapes that depend on feat_cap, n_frames and trees only.
 *
 * Records are dvo_knn_pair_run's with DVO_MATCH_FLANN, chained: the stream keeps cv::theRNG()'s
 * state in device memory; enabling sets it to a fresh thread's (0xFFFFFFFF).  Pair p's forest is
 * built iff the pair brings nq >= 1 and nt >= 2 features; it starts from the state left by the
 * built pairs before it, in this call and in earlier ones, and advances it by trees (2 nt - 1)
 * draws.  A marked (DVO_ECAP) or empty frame builds nothing and advances nothing.  Every record
 * field equals the pair path's on the same frames with the same incoming state (n_hypotheses
 * aside), whatever the split into calls; dvo_knn_stream_get_matches gives
 * dvo_knn_pair_get_matches's list (distances sqrtf of the squared L2).  One difference: a query
 * without a second neighbour although nt >= 2 (it needs a non-finite distance, which no detector
 * produces) marks the pair DVO_ENOFEAT with zeros elsewhere, where the pair path keeps the
 * geometry's fields.
 *
 * Scratch in bytes (P = max_frames - 1, C = feat_cap, T = trees):
 *   P (84 C + 32 T C + 512 T + 20) + 512 C + 24
 * (per pair: draws 8 C, shuffle buckets and point orders 24 C + 4, split scratch 12 C, nodes
 * 32 T C, open lists 32 C, level counts 4 C + 8, overflow list 4 C, chunk states 512 T, start
 * state 8; per stream: 64 global heaps of C entries, the state and two counters).
 * DVO_EINVAL: a null handle, trees outside 0..64, checks < 1 with trees > 0. */
int dvo_knn_stream_set_flann(dvo_knn_stream* s, int trees, int checks);
/* The FLANN mode's theRNG state: the setter is ordered on the stream (the calls before it use
 * the old state), the getter synchronises.  DVO_EINVAL on a stream that matches with BFMatcher. */
int dvo_knn_stream_set_rng_state(dvo_knn_stream* s, uint64_t state);
int dvo_knn_stream_get_rng_state(dvo_knn_stream* s, uint64_t* state);
/* Host only: the bytes dvo_knn_stream_set_flann allocates (the formula above; feat_cap is the
 * stream's effective capacity); 0 for max_frames outside 2..65536, feat_cap outside 2..65536 or
 * trees outside 1..64. */
size_t dvo_knn_stream_flann_bytes(int max_frames, int feat_cap, int trees);
/* Host only: the FLANN mode's RNG plan for `frames` frames with detector counts counts[frames]
 * (a count above cap marks the frame): starts[frames - 1] = the state each pair's forest starts
 * from (also of pairs that build nothing), *state_out = the state after the call.  The device
 * kernel runs the same text. */
int dvo_flann_rng_plan_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees, uint64_t* starts,
                            uint64_t* state_out);
/* Host only: the sharded plan of dvo_knn_stream_finish for one rank: counts[frames] are the
 * detector counts of the rank's frames (frames >= 0; fewer than 2 is a rank without pairs),
 * shard_draws[world] the ranks' draws words (NULL: nothing before or after; entry [rank] is not
 * read).  starts[frames - 1], *final_state = the state after the whole window, *own_draws = the
 * rank's draws word (any of the three may be NULL, starts only with frames < 2).  DVO_EINVAL:
 * world outside 1..1024, rank outside 0..world - 1, cap < 1, trees outside 1..64. */
int dvo_flann_rng_shard_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees,
                             const uint64_t* shard_draws, int world, int rank, uint64_t* starts, uint64_t* final_state,
                             uint64_t* own_draws);
/* After the last process call (these synchronise): frame `frame`'s features, desc n x 128 (SIFT)
 * or n x 64 (SURF) floats, *n = the detector's count (DVO_ECAP if > cap or the frame is marked);
 * pair `pair`'s kept matches in ascending queryIdx, *m = count (DVO_ECAP if > cap). */
int dvo_knn_stream_get_features(dvo_knn_stream* s, int frame, dvo_keypoint* kps, float* desc, int cap, int* n);
int dvo_knn_stream_get_matches(dvo_knn_stream* s, int pair, dvo_dmatch* out, int cap, int* m);
/* Device time of the last process call's stages, for tools: enable = 1 records events on the
 * stream from the next call on; ms[3] = detection, matching + ratio test, geometry + records
 * (synchronises; DVO_EINVAL before a profiled call). */
int dvo_knn_stream_set_profiling(dvo_knn_stream* s, int enable);
int dvo_knn_stream_stage_times(dvo_knn_stream* s, double* ms);
/* Raw input for the k-NN stream: colour (cv.cvtColor, v3:132), distorted (cv.undistort, v3:133)
 * and JPEG (cv.imdecode, v3:127) frames, as dvo_stream_process_bgr / _undistorted / _jpeg take
 * them for the ORB stream.  The input is brought to gray in a slab of the stream's own, on the
 * stream's HIP stream, by one launch per call (the decoder: its launches per group), and
 * detection runs on the slab; everything after is dvo_knn_stream_detect / _finish unchanged, so
 * records, features and matches equal those of dvo_knn_stream_process on the gray frames that
 * dvo_bgr2gray, dvo_undistort_apply(_bgr) or dvo_jpeg_decode make.
 *
 * set_raw_input: enable != 0 allocates the slab, max_frames frames of ((width + 15) & ~15)-byte
 * rows = dvo_knn_stream_raw_input_bytes(width, height, max_frames) bytes; 0 frees it.  A change
 * synchronises the stream and drops a pending detection; a call that changes nothing does
 * nothing.  A stream that never enables it allocates nothing more.  The detect and process calls
 * allocate nothing and make no synchronisation and no device-to-host copy (the decoder waits for
 * its own staging half, as in dvo_jpeg_decode, and queues its status copy).
 *
 * detect_raw / process_raw: d_frames holds n_frames frames of `channels` bytes per pixel (1 mono,
 * 3 BGR, 4 BGRA), rows `stride` bytes apart, frames frame_stride bytes apart; u may be NULL.
 * channels == 1 without u is dvo_knn_stream_detect / _process (in place, no slab).  Otherwise:
 * colour -> bgr2gray, colour with u -> the fused gray + remap, mono with u -> the remap.
 * detect_jpeg / process_jpeg: n baseline JPEGs of the stream's size, decoded with j's stream
 * entropy mode (dvo_jpeg_set_stream_entropy) and remapped by u if given.  Corrupt entropy-coded
 * data does not fail the call: dvo_jpeg_status names the frame and its records come from what
 * the decoder left.  The process forms are the detect form and dvo_knn_stream_finish(records,
 * NULL, 1, 0).  d_draws as in dvo_knn_stream_detect.
 * dvo_knn_stream_stage_times: the first figure of these calls is input + detection.
 *
 * Refused before anything is launched, with a pending detection, the frame slots and the FLANN
 * state left as they were: DVO_EINVAL for channels outside {1, 3, 4}, stride < width * channels,
 * a null buffer, n outside 1..max_frames, null records with n > 1 (process forms), an
 * undistorter of another size, an undistorter or decoder of another device, a slab that is
 * needed and not enabled, a JPEG of another size; the parser's DVO_EUNSUPPORTED or DVO_ECORRUPT
 * for a JPEG whose header cannot be taken. */
int dvo_knn_stream_set_raw_input(dvo_knn_stream* s, int enable);
/* Host only: the slab's bytes, max_frames * ((width + 15) & ~15) * height; 0 for an argument < 1. */
size_t dvo_knn_stream_raw_input_bytes(int width, int height, int max_frames);
int dvo_knn_stream_detect_raw(dvo_knn_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                              int64_t frame_stride, int stride, int channels, uint64_t* d_draws);
int dvo_knn_stream_process_raw(dvo_knn_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                               int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records);
int dvo_knn_stream_detect_jpeg(dvo_knn_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                               const int64_t* lens, int n, uint64_t* d_draws);
int dvo_knn_stream_process_jpeg(dvo_knn_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                                const int64_t* lens, int n, dvo_pair_record* d_records);
/* dvo_stream_process on undistorted frames: the n raw frames are remapped by u
 * into the stream's own frame slab first (same HIP stream), as the reference
 * undistorts every frame before detection (v3:120, v3:135). */
int dvo_stream_process_undistorted(dvo_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                                   int64_t frame_stride, int stride, dvo_pair_record* d_records);
/* dvo_stream_process / dvo_stream_submit on colour frames (channels = 3 or 4 bytes per
 * pixel, B G R first; rows `stride` >= width * channels bytes apart), as the reference
 * converts and undistorts every frame before detection — visual_odometry_v3.py:132-133
 * (u given), v3:132 alone (u NULL: no undistortion).  The frames are converted
 * (dvo_bgr2gray), or converted and remapped (dvo_undistort_apply_bgr), into the
 * stream's own frame slab on the stream's HIP stream, outside the stage timers; the
 * batch then runs on the slab exactly as after dvo_stream_process_undistorted, so
 * records and features are those of dvo_stream_process / _submit on the gray frames.
 * The caller's frames may be released once the conversion has run.
 * dvo_stream_submit_bgr reuses the slab at every submit.  That is safe: a submit
 * queues its batch's whole detection (pyramid to descriptors, the only readers of the
 * frames) on the same HIP stream before it returns, so the next submit's conversion is
 * ordered after it, and what a pair's record needs from its frames is kept with the
 * pair set, not read from the frames when the batch retires.  dvo_stream_get_pyramid
 * (blurred) after a submit reads the slab, i.e. the last submitted batch's frames.
 * DVO_EINVAL: channels not 3 or 4, u's size != the stream's, n_frames outside
 * 1..max_frames (submit: 2..max_frames), null frames, stride < width * channels,
 * null records with n_frames > 1. */
int dvo_stream_process_bgr(dvo_stream* s, dvo_undistort* u /* NULL: no undistortion */, const uint8_t* d_frames,
                           int n_frames, int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records);
int dvo_stream_submit_bgr(dvo_stream* s, dvo_undistort* u /* NULL: no undistortion */, const uint8_t* d_frames,
                          int n_frames, int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records);
/* HIP stream the batch runs on (hipStream_t as void*; each dvo_stream owns
 * one, so batches on different dvo_streams may overlap on the device). */
void* dvo_stream_hip_stream(dvo_stream* s);
/* Pose tail of get_transformation_between_two_frames (v3:309-345) and
 * previous_current_matching (v3:367) for the pairs of the last
 * dvo_stream_process (read from that call's d_records, which must stay
 * allocated until the tail has run), on the device:
 *   P_cur = K [R | t];  X = triangulatePoints(P_prev, P_cur, c_prev, c_cur);
 *   d = |X[:3,0] - X[:3,1]| (homogeneous, not divided by W: D3);  s = L / d;
 *   T_rel = translation_matrix(t s) . euler_matrix(euler_from_matrix(R,'rxyz'),'sxyz');
 *   T_abs = T_abs_prev . T_rel.
 * P_prev / T_abs_prev carry over between calls on the device; set them with
 * dvo_stream_reset_pose (controlled mode: P0 = K [I | 0], v3:164-166).
 * d_corners_*: device [pairs][k][2] doubles (k >= 2).  Outputs device [pairs][16]. */
int dvo_stream_reset_pose(dvo_stream* s, const double* P0 /* host 12 */, const double* T0 /* host 16 */);
/* Make s use owner's pose carry, so batches alternating between streams (each
 * stream runs on its own HIP stream; batches overlap on the device) chain one
 * pose stream: pose tails on a shared carry run in call order via HIP events. */
int dvo_stream_share_pose(dvo_stream* s, dvo_stream* owner);
int dvo_stream_pose_tail(dvo_stream* s, const double* d_corners_prev, const double* d_corners_cur, int k,
                         double marker_length, double* d_T_rel, double* d_T_abs);
/* The same for a retired batch's records (pipelined submits; pairs = its pair count). */
int dvo_stream_pose_tail_batch(dvo_stream* s, const dvo_pair_record* d_records, int pairs, const double* d_corners_prev,
                               const double* d_corners_cur, int k, double marker_length, double* d_T_rel,
                               double* d_T_abs);

/* The same pose tail over caller-supplied pair records: the reassembly step of
 * one pose stream sharded across ranks.  Every rank computes
 * the records of its run of pairs (dvo_stream_process), the ranks all-gather
 * records and per-pair marker corners, and rank 0 runs this over the whole
 * window in pair order.  The tail reads only R, t, status and n_models of each
 * record (a pair counts as successful iff status == DVO_OK and n_models == 1,
 * as in dvo_stream_pose_tail), so P_prev of the first pair of a run is the
 * last successful pair's even when it lies on another rank: the result is
 * bit-identical to one rank running dvo_stream_pose_tail over the stream.
 * K: host 9 doubles.  d_carry: device 28 doubles, P_prev (3x4) | T_abs (4x4),
 * the state before the first pair on entry and after the last on return
 * (controlled mode: P0 = K [I | 0], v3:164-166).  Asynchronous on hip_stream
 * (NULL = the context's stream). */
int dvo_pose_tail_records(dvo_ctx* ctx, const dvo_pair_record* d_records, int pairs, const double* K,
                          const double* d_corners_prev, const double* d_corners_cur, int k, double marker_length,
                          double* d_carry, double* d_T_rel, double* d_T_abs, void* hip_stream);

/* The pair-parallel half of that tail on one rank's run of a gathered window:
 * T_rel of pairs [p0, p0 + n) of the window's `pairs` records (d_T_rel[0 .. n)),
 * each triangulating against the last successful pair before it in the window
 * (or d_P_carry, 12 doubles, when none is), then d_P_carry advanced past the
 * window (to its last successful pair's K [R | t]).  Every rank runs it over its
 * own pairs, rank 0 gathers the T_rel and runs dvo_pose_chain: the same values,
 * bit for bit, as dvo_pose_tail_records over the window on one rank.  Corner
 * arrays are the window's ([pairs][k][2]).  Asynchronous on hip_stream. */
int dvo_pose_rel_range(dvo_ctx* ctx, const dvo_pair_record* d_records, int pairs, int p0, int n, const double* K,
                       const double* d_corners_prev, const double* d_corners_cur, int k, double marker_length,
                       double* d_P_carry, double* d_T_rel, void* hip_stream);

/* The same chain on the host (host arrays; the device kernel's arithmetic, bit for bit): the
 * chain is one sequential product per pair, which a CPU core runs in ~50 ns per pair while
 * the GPU is busy with the next batches, where the one-wave kernel slows to ~1.5 us per pair
 * (round 5).  Rank 0 of a sharded stream chains the gathered T_rel here. */
int dvo_pose_chain_host(const double* T_rel, int n, double* T_carry, double* T_abs);

/* The absolute-pose chain of previous_current_matching (v3:367,
 * T_robot_cur = T_robot_prev . T_prev->cur) on its own, for pose streams
 * reassembled from sharded runs: rank 0 all-gathers every
 * rank's T_rel and chains them in pair order with the same arithmetic as
 * dvo_stream_pose_tail, so the result is bit-identical to one rank chaining the
 * whole stream.  d_T_rel: device [n][16]; d_T_carry: device 16 doubles, the pose
 * before the first pair on entry and after the last on return; d_T_abs: device
 * [n][16].  Asynchronous on hip_stream (NULL = the context's stream). */
int dvo_pose_chain(dvo_ctx* ctx, const double* d_T_rel, int n, double* d_T_carry, double* d_T_abs, void* hip_stream);

/* ---------------------------------------------------------------------------
 * JPEG frames: cv.imdecode(np_arr, IMREAD_COLOR) (v3:127) of baseline JPEGs on the
 * device, byte for byte what libjpeg-turbo's default decode (JDCT_ISLOW, fancy
 * upsampling: cv.imdecode's and Pillow's) gives, and the cvtColor that follows.
 *
 * Supported: SOF0, 8-bit, Huffman, one interleaved scan; 1 component, or 3 (YCbCr)
 * with Cb = Cr = 1x1 and Y 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0); any 8-bit DQT,
 * any DHT, any restart interval, any size >= 1.  DVO_EUNSUPPORTED, found in the
 * header before anything is launched: progressive, arithmetic, 12-bit, 16-bit
 * quantisation tables, 4 components, Adobe transform 0, component ids R G B, other
 * sampling factors, more than one scan.  A malformed header is DVO_ECORRUPT in the
 * same way; malformed entropy-coded data is found while decoding and gives the
 * frame the status DVO_ECORRUPT (dvo_jpeg_status): its blocks from the first bad
 * one of a segment on stay zero, and the call itself succeeds.
 * --------------------------------------------------------------------------- */

/* Header of one JPEG, on the host (ctx-free).  sampling: luma factors h << 4 | v
 * (0x11, 0x21, 0x22; 0x11 for one component).  DVO_OK, DVO_EUNSUPPORTED, DVO_ECORRUPT. */
int dvo_jpeg_probe(const uint8_t* buf, int64_t len, int* w, int* h, int* components, int* sampling);

/* What the entropy decoder produces for one image: int16 coefficients in natural
 * order, per component [block row][block column][64] padded to whole MCUs
 * (blocks_w x blocks_h blocks from element coef_offset), coef_count in all. */
typedef struct {
    int32_t width, height, components, sampling;
    int32_t restart_interval, segments;
    int32_t blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];
    int64_t coef_count;
    uint16_t quant[3][64]; /* per component, natural order */
} dvo_jpeg_layout;

/* Parser + entropy decoder of one image on the host (ctx-free): the layout, and,
 * when coef is not NULL, coef_count coefficients (DVO_ECAP if cap is smaller) with
 * *status = DVO_OK or DVO_ECORRUPT for the entropy-coded data. */
int dvo_jpeg_entropy_host(const uint8_t* buf, int64_t len, dvo_jpeg_layout* layout, int16_t* coef, int64_t cap,
                          int* status);

/* A decoder for frames up to max_w x max_h.  All its scratch (pinned staging, plans,
 * coefficients, component planes, a gray frame group) is sized here for one group of
 * group_frames frames (of 4:2:2 at half a byte of scan per pixel: about 7 bytes of
 * device and 5 of pinned host memory per pixel of the maximum size and frame; frames that need more close their group
 * early); a batch runs group after group and nothing is allocated per call.  The device
 * entropy decoder works on one group's segments at a time, one lane each, so frames
 * without restart markers decode as many at a time as the group holds.  A decoder
 * serves one HIP stream at a time. */
/* The host model of DVO_JPEG_ENTROPY_DEVICE_SPLIT (ctx-free): dvo_jpeg_entropy_host by the
 * split kernel's functions and schedule, the lanes taken one after the other.  Every
 * segment of at least two runs of split_bytes bytes is split.  coef: coef_count
 * coefficients in dvo_jpeg_entropy_host's layout (DVO_ECAP if cap is smaller), equal to
 * its output, as is *status; *passes: the most synchronisation passes a segment took. */
int dvo_jpeg_entropy_split_host(const uint8_t* buf, int64_t len, int split_bytes, int16_t* coef, int64_t cap, int* status,
                                int* passes);

int dvo_jpeg_create(dvo_ctx* ctx, int max_w, int max_h, int group_frames, dvo_jpeg** out);
void dvo_jpeg_destroy(dvo_jpeg* j);

#define DVO_JPEG_ENTROPY_HOST 0   /* Huffman decoding on the calling thread     */
#define DVO_JPEG_ENTROPY_DEVICE 1 /* one GPU lane per restart segment (default) */
/* Long segments (at least 16 runs of split_bytes bytes) by one workgroup each, lane i on
 * the i-th run: lanes start from guessed decoder states and take over their left
 * neighbour's exit state until none changes (self-synchronising Huffman decoding), at
 * most as many passes as the segment has runs; shorter segments as under _DEVICE.  The
 * output is _DEVICE's on every input; a corrupt segment is decoded again by one lane. */
#define DVO_JPEG_ENTROPY_DEVICE_SPLIT 2

/* Scan bytes per lane under DVO_JPEG_ENTROPY_DEVICE_SPLIT: a power of two in 16..4096
 * (a symbol is at most 31 bits, so none jumps over 16 bytes), else DVO_EINVAL.
 * The default, DVO_JPEG_SPLIT_BYTES_DEFAULT, is the fastest of 32, 64, 128, 256 and 512
 * on 256 restart-free 1280x720 frames per group (tools/time_jpeg.py; DESIGN.md, "JPEG input"). */
#define DVO_JPEG_SPLIT_BYTES_DEFAULT 256
int dvo_jpeg_set_split(dvo_jpeg* j, int split_bytes);
int dvo_jpeg_get_split(dvo_jpeg* j, int* split_bytes);
/* The mode dvo_stream_process_jpeg / dvo_stream_submit_jpeg decode with:
 * DVO_JPEG_ENTROPY_DEVICE (initially) or DVO_JPEG_ENTROPY_DEVICE_SPLIT; the host mode is
 * not used on that path: DVO_EINVAL. */
int dvo_jpeg_set_stream_entropy(dvo_jpeg* j, int entropy);

/* n JPEGs of one size w x h <= max (sampling, tables and restart interval may differ
 * per frame) -> n device frames of out_channels bytes per pixel: 1 gray
 * (cvtColor(BGR2GRAY) of the decoded bytes, not the Y plane), 3 BGR, 4 BGRA (A 255).
 * Asynchronous on hip_stream (NULL = the context's); the byte buffers are free at
 * return.  An unsupported or header-corrupt frame fails the call before anything is
 * launched, and dvo_last_error names its index.  n == 0 launches nothing.  At most
 * 65536 frames per call. */
int dvo_jpeg_decode(dvo_jpeg* j, const uint8_t* const* bufs, const int64_t* lens, int n, int out_channels,
                    uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, int entropy, void* hip_stream);
/* After synchronising: DVO_OK or DVO_ECORRUPT per frame of the last decode (or stream) call. */
int dvo_jpeg_status(dvo_jpeg* j, int* st, int n);
/* Host in, host out, synchronous, host entropy; size the output with dvo_jpeg_probe.
 * DVO_ECORRUPT (with the decodable part written) if the entropy-coded data is corrupt. */
int dvo_jpeg_decode_image(dvo_jpeg* j, const uint8_t* buf, int64_t len, int out_channels, uint8_t* out,
                          int out_stride);
/* imdecode + cvtColor + undistort (v3:127-133) of one host JPEG of u's size: mono8 out. */
int dvo_undistort_image_jpeg(dvo_undistort* u, dvo_jpeg* j, const uint8_t* buf, int64_t len, uint8_t* out,
                             int out_stride);
/* dvo_stream_process / dvo_stream_submit of n JPEG frames of the stream's size: decoded to
 * gray into the stream's frame slab on its HIP stream (with u: into j's gray frame group,
 * then dvo_undistort_apply into the slab), outside the stage timers; from there exactly
 * dvo_stream_process_bgr / dvo_stream_submit_bgr. */
int dvo_stream_process_jpeg(dvo_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                            const int64_t* lens, int n, dvo_pair_record* d_records);
int dvo_stream_submit_jpeg(dvo_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                           const int64_t* lens, int n, dvo_pair_record* d_records);
/* Test hook: the coefficients of frame `frame` of the last frame group decoded
 * (dvo_jpeg_entropy_host's layout); *n_out is their count, DVO_ECAP if cap is
 * smaller; synchronises. */
int dvo_jpeg_get_coefficients(dvo_jpeg* j, int frame, int16_t* out, int64_t cap, int64_t* n_out);
/* Test hook: of the last DVO_JPEG_ENTROPY_DEVICE_SPLIT call, the most synchronisation
 * passes a segment took, the segments the split kernel decoded and how many of them
 * it gave to the one-lane decoder as corrupt; synchronises. */
int dvo_jpeg_get_split_info(dvo_jpeg* j, int* max_passes, int* segments, int* fallbacks);

/* Per-stage device time via HIP events recorded on the stream's HIP stream
 * around each kernel group (0 pyramid, 1 blur, 2 fast, 3 select+harris,
 * 4 describe, 5 match, 6 ransac, 7 recoverPose+records, 8 pose tail).  Accumulated over
 * every dvo_stream_process since profiling was enabled. */
#define DVO_NSTAGES 9  /* ... 8 pose tail */
int dvo_stream_set_profiling(dvo_stream* s, int enable);
int dvo_stream_stage_times(dvo_stream* s, double* ms /* DVO_NSTAGES */, int* calls);

/* Opt-in match filter of the ORB stream: knnMatch(k = 2) and Lowe's ratio test
 * (visual_odometry_v3.py:223-228, `m.distance < ratio * n.distance` in Python
 * floats) instead of the cross check.  ratio 0 (the default): off, the stream
 * matches with cfg.cross_check.  A finite ratio > 0: every later process /
 * process_pairs / submit / submit_pairs / pair call and the undistorted, BGR and
 * JPEG input calls match with the Hamming 2-NN and keep query q when the test
 * passes; cfg.cross_check is ignored.  Kept matches are in ascending queryIdx
 * (the k-NN modes' order, not the cross check's (distance, queryIdx)), and
 * n_matches counts them.  A pair whose current frame has fewer than 2
 * descriptors (the reference's `for m, n in matches` raises) gets DVO_ENOFEAT,
 * the counts filled, zeros elsewhere; a pair without a query descriptor keeps
 * the record it gets with the ratio test off.  DVO_EINVAL for a NaN, infinite or
 * negative ratio, and while submitted batches are pending. */
int dvo_stream_set_ratio_test(dvo_stream* s, double ratio);

/* Host copies of intermediate results of the last dvo_stream_process (tests).
 * get_pyramid(blurred = 1): the detection path blurs only the 39 x 44 descriptor
 * windows inside the describe kernel, so the whole GaussianBlur of the level is
 * computed on this call from the last process's frames, which must still be
 * alive (device frames passed to dvo_stream_process, or the stream's own upload
 * slab). */
int dvo_stream_get_features(dvo_stream* s, int frame, dvo_keypoint* kps, uint8_t* desc, int cap, int* n);
int dvo_stream_get_matches(dvo_stream* s, int pair, dvo_dmatch* out, int cap, int* m);
int dvo_stream_get_pyramid(dvo_stream* s, int frame, int level, int blurred, uint8_t* out, int cap);

/* ---------------------------------------------------------------------------
 * Landmarks: the triangulated inlier points of each pair of a stream batch, what
 * cv.recoverPose(E, p1, p2, K, distanceThresh, mask, triangulatedPoints) hands back
 * at v3:303, restricted to the matches both masks keep.
 * Correspondence i of a pair whose record has status DVO_OK and n_models 1 (in the
 * order of get_matches, the order findEssentialMat saw) is a landmark iff
 *   1. it is an inlier of the record's E: findEssentialMat's mask, the Sampson test
 *      at threshold / ((fx + fy) / 2); all five when the pair has five matches; and
 *   2. it passes recoverPose's four tests (X2 X3 > 0, both depths in (0, dist_thresh))
 *      for the decomposition recoverPose chose, on its own DLT triangulation against
 *      that decomposition's [R | t].
 * Its position is (X0 / X3, X1 / X3, X2 / X3) in double: the previous frame's camera
 * coordinates, in units of the baseline (recoverPose's |t| = 1).  Metric scale is the
 * consumer's: multiply by the pair's scale from the pose tail.
 * Per pair, landmarks go in ascending i to slots [0, min(count, cap)) of the pair's
 * cap entries; count[pair] is the full number (above cap: an overflow), 0 for a pair
 * that failed.  Bytes of the entry buffer outside the written slots are not touched. */
typedef struct {              /* 48 bytes */
    int32_t match, reserved;  /* index into the pair's match list; 0 */
    float x1, y1, x2, y2;     /* the pixel coordinates the stream's point buffer holds */
    double X, Y, Z;
} dvo_landmark;
/* Binds device buffers, d_out [pairs][cap] entries and d_count [pairs], for the NEXT batch
 * only: the next dvo_stream_process / _process_pairs / _submit / _submit_pairs call or one of
 * their undistorted, BGR or JPEG variants (v3:303, recoverPose(..., triangulatedPoints)).  The
 * binding travels with that batch as its records pointer does and is written when the batch
 * retires, on the stream's HIP stream, after the records; the buffers must stay allocated
 * until then.  d_out == NULL clears a pending binding.  DVO_EINVAL for a non-null d_out with
 * cap < 1 or d_count == NULL.  The first binding allocates the kernel's scratch (32 B per
 * slot of a set's point buffer, rounded up to 256 slots per pair); a stream that never binds
 * launches and holds what it did before.  dvo_stream_pair does not take a binding. */
int dvo_stream_set_landmarks(dvo_stream* s, dvo_landmark* d_out, int32_t* d_count, int cap);
/* The same for a k-NN stream (v3:303, recoverPose(..., triangulatedPoints)): the next batch is
 * the next dvo_knn_stream_process* or dvo_knn_stream_finish; a detect call alone does not
 * consume the binding. */
int dvo_knn_stream_set_landmarks(dvo_knn_stream* s, dvo_landmark* d_out, int32_t* d_count, int cap);

/* ---------------------------------------------------------------------------
 * Tracks: the landmarks of consecutive pairs of one batch joined on the keypoint they
 * share, and the ratio of the two baselines from the shared points.  An opt-in companion
 * of a landmark binding.  The reference has metric scale only where a STag marker is
 * seen (v3:263-291, 319-325); the ratios carry it through the pairs in between.
 *
 * Pair p has a full landmark list in ascending match order: the list count[p] counts,
 * not the cap-limited slots.  A landmark's ORDINAL is its position in that list; below
 * cap it is also its slot.  Frame j is detected once, so pair p - 1's trainIdx and pair
 * p's queryIdx index the same keypoint array.
 *
 * Link.  Landmark o of pair p >= 1 with match (q, t) links to the ordinal of the landmark
 * of pair p - 1 whose match has trainIdx == q; the smallest such ordinal if several
 * qualify (the ratio-test modes can keep a train index for several queries).  -1 if
 * none does, if p == 0, or if either pair has no landmarks.  A link may be >= cap when
 * pair p - 1 overflowed the caller's landmark buffer: that is valid and says so.
 *
 * Ratio.  A linked landmark at Xb = (Xb, Yb, Zb) in pair p and Xa = (X, Y, Z) in pair
 * p - 1, with R, t of pair p - 1's record, has ratio |R Xa + t| / |Xb|: baseline p over
 * baseline p - 1, so a metric baseline length s obeys s[p] = ratio * s[p - 1].  In double,
 * every operation rounded once, in this order:
 *   y_i   = ((R[i][0] * X + R[i][1] * Y) + R[i][2] * Z) + t[i]
 *   num   = sqrt((y0 * y0 + y1 * y1) + y2 * y2)
 *   den   = sqrt((Xb * Xb + Yb * Yb) + Zb * Zb)
 *   ratio = num / den
 * Both depths lie in (0, dist_thresh) by recoverPose's tests, so it is finite and positive.
 *
 * Per pair.  n_common is the number of linked landmarks and r[0..n) their ratios in
 * ascending order: ratio = r[(n - 1) / 2] (the lower median), q1 = r[(n - 1) / 4],
 * q3 = r[3 (n - 1) / 4], integer divisions; all three 0.0 when n_common < 1.  n_common
 * is -1 for pair 0 of a batch, which has no predecessor.  n_prev is the predecessor's
 * full landmark count: 0 for pair 0 and where the predecessor failed.
 * Links and statistics do not depend on cap.  The chain does not cross a batch boundary:
 * a caller who needs it unbroken overlaps consecutive batches by one pair (two frames). */
typedef struct {            /* 32 bytes */
    double ratio, q1, q3;
    int32_t n_common, n_prev;
} dvo_track_scale;
/* Binds device buffers for the NEXT batch only, beside the landmark binding pending for that
 * batch: d_link [pairs][cap] with that binding's cap, written for slots [0, min(count, cap))
 * (bytes outside them are not touched), and d_scale [pairs].  Either may be NULL (links only,
 * scales only); both NULL clears a pending tracks binding, as clearing the landmark binding
 * does.  DVO_EINVAL when no landmark binding is pending.  The binding travels with the batch
 * as the landmark binding does and is written when the batch retires, after the landmarks,
 * on the stream's HIP stream with no read-back.  dvo_stream_process_pairs and
 * dvo_stream_submit_pairs build pairs that share no frame: such a call with a tracks binding
 * pending returns DVO_EINVAL and consumes both bindings.
 * The first tracks binding allocates the scratch, once, for every pair set the stream can
 * hold (dvo_pipeline_depth()): per set and per slot of its point buffer 4 B of keypoint table
 * ([pairs][kp_cap] int32), 8 B of ratios ([pairs][pts_stride] double) and 8 B for the set's
 * own copy of (queryIdx, trainIdx), 20 B in all, and 4 B per 256 slots.  The copy is taken
 * right after matching, only for batches that carry a tracks binding: the stream's match
 * indices belong to the stream, and under pipelined submits a later batch has overwritten
 * them when an earlier one retires.  A stream that never binds tracks launches and holds
 * what it did before, and a landmarks-only batch writes what it wrote. */
int dvo_stream_set_tracks(dvo_stream* s, int32_t* d_link, dvo_track_scale* d_scale);
/* The same for a k-NN stream, whose one pair set retires inside the call and reads its
 * dvo_dmatch array directly: 12 B of scratch per slot and 4 B per 256 slots.  A detect call
 * alone consumes nothing. */
int dvo_knn_stream_set_tracks(dvo_knn_stream* s, int32_t* d_link, dvo_track_scale* d_scale);

/* ---------------------------------------------------------------------------
 * Track poses: each pair's 6-DoF pose refined on the previous pair's landmarks.  An opt-in
 * companion of a tracks binding.  The ratio above inherits the error of each pair's t
 * direction; here camera j + 1 of pair p (frames j, j + 1) is fitted to 3-D to 2-D
 * correspondences that use neither pair p's triangulation nor its t, and the length of the
 * fitted translation is the baseline ratio.
 *
 * Correspondences.  For pair p they are its linked landmarks in ascending ordinal, k = 0..n-1
 * with n = n_common.  Correspondence k has
 *   Y = (y0, y1, y2)   the y_i of the ratio above, unchanged: the point in camera j, in units
 *                      of pair p - 1's baseline;
 *   (nu, nv)           the landmark's float x2, y2 normalised as the stream normalises them, in
 *                      double: nu = x2 * ax + bx, nv = y2 * ay + by with ax = 1 / fx,
 *                      bx = -cx * ax, ay = 1 / fy, by = -cy * ay.
 *
 * Start.  R = rec[p].R, t_i = scale[p].ratio * rec[p].t[i].
 *
 * One step.  In double, every operation rounded once, in the written order.  Per k:
 *   P_i = ((R[i][0] * y0 + R[i][1] * y1) + R[i][2] * y2) + t[i]
 *   a correspondence with !(P2 > 0) contributes +0.0 to every sum; otherwise
 *   a = 1 / P2, u = P0 * a, v = P1 * a, ru = u - nu, rv = v - nv, e2 = ru * ru + rv * rv
 *   w = 1 if e2 <= kh * kh, else kh / sqrt(e2), with kh = huber_px / ((fx + fy) / 2)
 *   b = -(u * a), c = -(v * a)
 *   Ju = (b * P1, a * P2 - b * P0, -(a * P1), a, 0, b)
 *   Jv = (c * P1 - a * P2, -(c * P0), a * P0, 0, a, c)
 * (the left perturbation P <- omega x P + dt, omega first).  The 21 terms of H are
 * w * (Ju_i * Ju_j + Jv_i * Jv_j) for i <= j, the upper triangle row by row; the 6 terms of g
 * are w * (Ju_i * ru + Jv_i * rv).
 *
 * Sum order, of each of the 27 terms alone:
 *   1. lane l of 256 adds the terms of k = l, l + 256, ... in ascending k onto +0.0;
 *   2. inside each group of 64 lanes, for s = 32, 16, 8, 4, 2, 1, lane l < s adds lane l + s;
 *   3. the four group totals are added as ((g0 + g1) + g2) + g3.
 *
 * Solve H d = -g by LDL^T without pivoting, H[i][j] for i > j being H[j][i]:
 *   for j = 0..5:  D[j] = H[j][j], then for k = 0..j-1: D[j] = D[j] - (L[j][k] * L[j][k]) * D[k]
 *                  the step fails unless D[j] > 0
 *                  for i = j+1..5: x = H[j][i], then for k = 0..j-1:
 *                                  x = x - (L[i][k] * L[j][k]) * D[k];  L[i][j] = x / D[j]
 *   for i = 0..5:  z[i] = -g[i], then for k = 0..i-1: z[i] = z[i] - L[i][k] * z[k]
 *   for i = 0..5:  y[i] = z[i] / D[i]
 *   for i = 5..0:  d[i] = y[i], then for k = i+1..5: d[i] = d[i] - L[k][i] * d[k]
 *                  the step fails unless every d[i] is finite
 * A step that fails ends the pair with status DEGENERATE and the pose of the step before.
 *
 * Update by the Cayley map (no transcendental function): v = d[0..3) * 0.5,
 * vv = (vx * vx + vy * vy) + vz * vz,
 *   C = [ (1 - vv) + 2 (vx vx)   2 (vx vy) - 2 vz       2 (vx vz) + 2 vy     ]
 *       [ 2 (vx vy) + 2 vz       (1 - vv) + 2 (vy vy)   2 (vy vz) - 2 vx     ]
 *       [ 2 (vx vz) - 2 vy       2 (vy vz) + 2 vx       (1 - vv) + 2 (vz vz) ]
 * every entry then divided by 1 + vv; R <- C R and t <- C t + d[3..6), an entry of C R or C t
 * formed as (x0 + x1) + x2 and d[3 + i] added last.
 *
 * Exactly `iters` steps are taken unless one fails: there is no convergence test, so the
 * result depends on no tolerance and the loop's length on no data.
 *
 * Final pass, on the last pose, with P, a, u, v, ru, rv as above:
 *   n_used     the correspondences with P2 > 0;
 *   inlier     P2 > 0 and e = (fx * ru) * (fx * ru) + (fy * rv) * (fy * rv) <= inlier_px * inlier_px;
 *   n_inliers  their number;
 *   rms        sqrt(sum of the inliers' e in the order above (others +0.0) / n_inliers), 0.0 with none;
 *   scale      sqrt((t0 * t0 + t1 * t1) + t2 * t2).
 *
 * Status.  DVO_TRACK_POSE_NONE: pair 0 of a batch and every pair with n_common < min_points (a
 * pair whose record, or whose predecessor's record, failed has n_common 0).  Such a pair holds
 * the start values in R, t and scale (all zero where n_common < 1: there is no ratio), and 0
 * in rms, n_used, n_inliers, iters.  DVO_TRACK_POSE_DEGENERATE: see Solve; the final pass runs
 * on the pose it kept.  iters is the number of steps taken.  Nothing depends on the landmark
 * cap. */
#define DVO_TRACK_POSE_OK 0
#define DVO_TRACK_POSE_NONE 1
#define DVO_TRACK_POSE_DEGENERATE 2
typedef struct {              /* 128 bytes */
    double R[9], t[3];        /* camera j + 1 from camera j: x' = R x + t, |t| in units of pair p - 1's baseline */
    double scale, rms;        /* |t|: baseline p over baseline p - 1; pixels */
    int32_t n_used, n_inliers, iters, status;
} dvo_track_pose;
/* Binds d_pose [pairs] for the NEXT batch only, beside the tracks binding pending for it:
 * DVO_EINVAL unless a tracks binding with a non-NULL d_scale is pending (the start reads the
 * ratio).  iters, huber_px, inlier_px, min_points: zero or negative means the default (10,
 * 1.0, 2.0, 6); DVO_EINVAL for iters > 32, min_points 1 or 2, or a NaN.  huber_px = INFINITY
 * weights every correspondence 1.  d_pose == NULL clears a pending binding, as clearing the
 * landmark binding and every dvo_stream_set_tracks call do: bind poses last.  The binding
 * travels with the batch and is written when it retires, after the tracks; a *_pairs call
 * refuses it as it refuses tracks.  The first binding allocates 40 B per slot of the point
 * buffer for every pair set, once; a stream that never binds poses launches and holds what it
 * did before, and the landmark, link and scale bytes of a batch do not depend on the binding. */
int dvo_stream_set_track_poses(dvo_stream* s, dvo_track_pose* d_pose, int iters, double huber_px, double inlier_px,
                               int min_points);
/* The same for a k-NN stream. */
int dvo_knn_stream_set_track_poses(dvo_knn_stream* s, dvo_track_pose* d_pose, int iters, double huber_px,
                                   double inlier_px, int min_points);

/* ---------------------------------------------------------------------------
 * Track ids and refined landmarks: for every landmark the track it belongs to, and its position
 * re-estimated from the most recent frames of that track.  An opt-in companion of a tracks
 * binding.  A landmark's X, Y, Z is the two-view DLT point of one pair; under narrow-baseline
 * motion its depth is the noisiest quantity a batch holds, and a point seen in several
 * consecutive frames has wider parallax and more observations than any pair offers.  Both
 * outputs are laid out [pairs][cap] in parallel with the landmark slots and computed on the full
 * lists and full links: nothing depends on cap.  Slots [0, min(count, cap)) are written; bytes
 * outside them are not touched.
 *
 * Chain.  link(p, o) is the link above, of the full list.  The chain of landmark (p, o) is
 * c_0 = (p, o) and c_{k+1} = (p - k - 1, link(c_k)) while that link is >= 0.  By the link rule a
 * landmark has at most one predecessor, and the smallest ordinal wins a shared one, so chains
 * are simple paths; they never cross a failed or empty pair and never leave the batch.
 *
 * Ids.  age = the number of links to the chain's end (0 without a predecessor), root_pair =
 * p - age, root_ord = the ordinal of the chain's last element in pair root_pair's full list (it
 * may be >= cap, as a link may), reserved = 0.  Exact integers.
 *
 * Unit motion of pair q: (R_q, d_q, rho_q), camera q + 1 from camera q with |d_q| = 1 and rho_q =
 * baseline q over baseline q - 1.  Where a track-poses binding was pending when this one was
 * made and pose[q].status == DVO_TRACK_POSE_OK:  R_q = pose[q].R, d_q[i] = pose[q].t[i] /
 * pose[q].scale, rho_q = pose[q].scale.  Otherwise R_q = rec[q].R, d_q = rec[q].t, rho_q =
 * scale[q].ratio.
 *
 * Window cameras of pair p, the same for every landmark of the pair: camera p - k from the
 * landmark's own frame p, in units of baseline p.  In double, every operation rounded once, in
 * the written order.  A_0 = I, b_0 = 0, sigma_0 = 1; for k = 1, 2, ... with q = p - k:
 *   the window ends before k if q < 0, if pair q or pair q + 1 has no landmarks, or if
 *   !(rho_{q+1} > 0) (a pair that links nothing has ratio 0.0, so the first two follow from the
 *   third);
 *   sigma_k = sigma_{k-1} / rho_{q+1};  the window ends before k if sigma_k is not finite;
 *   A_k[i][j] = (R_q[0][i] * A_{k-1}[0][j] + R_q[1][i] * A_{k-1}[1][j]) + R_q[2][i] * A_{k-1}[2][j]
 *   c[i]      = b_{k-1}[i] - sigma_k * d_q[i]
 *   b_k[i]    = (R_q[0][i] * c[0] + R_q[1][i] * c[1]) + R_q[2][i] * c[2]
 * (A_k = R_q^T A_{k-1}, b_k = R_q^T (b_{k-1} - sigma_k d_q)).  W is the number of cameras k >= 1.
 *
 * Views of landmark (p, o).  n = min(chain length, views - 1, W + 1) chain elements give n + 1
 * views: v = 0 is camera (I, 0) with (x1, y1) of c_0; v = 1 is camera (R_p, d_p) with (x2, y2)
 * of c_0; v = k + 1 for k = 1..n-1 is camera (A_k, b_k) with (x1, y1) of c_k, the floats of the
 * stream's point buffer at c_k's match.  Pixels go to double and are normalised as the track
 * poses normalise them: nu = x * ax + bx, nv = y * ay + by.
 *
 * Fit.  X = the landmark's own (X, Y, Z).  One step, the views in ascending v, every sum
 * starting at +0.0 and taking the views' terms in that order; per view with camera (A, b):
 *   P_i = ((A[i][0] * X0 + A[i][1] * X1) + A[i][2] * X2) + b[i]
 *   a view with !(P2 > 0) contributes nothing; otherwise
 *   a = 1 / P2, u = P0 * a, v = P1 * a, ru = u - nu, rv = v - nv, e2 = ru * ru + rv * rv
 *   w = 1 if e2 <= kh * kh, else kh / sqrt(e2), with kh = huber_px / ((fx + fy) / 2)
 *   Ju[j] = a * (A[0][j] - u * A[2][j]),  Jv[j] = a * (A[1][j] - v * A[2][j])
 * The 6 terms of H are w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]) for i <= j, the upper triangle row by
 * row; the 3 terms of g are w * (Ju[i] * ru + Jv[i] * rv).  H d = -g by the LDL^T of the track
 * poses with 3 in place of 6, the same loops; the step fails unless every D[j] > 0 and every
 * d[i] is finite.  X <- X + d, entry by entry.  Exactly `iters` steps are taken unless one fails:
 * no convergence test.  A step that fails ends the landmark DEGENERATE on the X it started from.
 *
 * Final pass on the last X, with P, a, u, v, ru, rv as above: n_used = the views with P2 > 0;
 * an inlier has P2 > 0 and e = (fx * ru) * (fx * ru) + (fy * rv) * (fy * rv) <= inlier_px *
 * inlier_px; n_inliers their number; rms = sqrt(sum of the inliers' e in ascending v onto +0.0 /
 * n_inliers), 0.0 with none.
 *
 * Status.  DVO_TRACK_REFINE_OK: X, Y, Z refined, views = n + 1, iters = the steps taken.
 * DVO_TRACK_REFINE_NONE: fewer than 3 views (no predecessor, pair 0 of the batch, W = 0): the
 * landmark's own X, Y, Z, views = 2, zero in rms, n_used, n_inliers, iters.
 * DVO_TRACK_REFINE_DEGENERATE: a step failed; the final pass runs on the X that was kept.
 * The refined point stands where the raw one stands: camera of frame p, units of baseline p. */
#define DVO_TRACK_REFINE_OK 0
#define DVO_TRACK_REFINE_NONE 1
#define DVO_TRACK_REFINE_DEGENERATE 2
typedef struct {              /* 16 bytes */
    int32_t root_pair, root_ord, age, reserved;
} dvo_track_id;
typedef struct {              /* 56 bytes */
    double X, Y, Z, rms;      /* rms in pixels */
    int32_t views, n_used, n_inliers, iters, status, reserved;
} dvo_landmark_refined;
#ifdef __cplusplus
static_assert(sizeof(dvo_track_id) == 16 && sizeof(dvo_landmark_refined) == 56, "layout");
#else
_Static_assert(sizeof(dvo_track_id) == 16 && sizeof(dvo_landmark_refined) == 56, "layout");
#endif
/* Binds d_refined and d_id, each [pairs][the landmark binding's cap], for the NEXT batch only.
 * Either may be NULL (ids only, refined only); both NULL clears a pending binding.  DVO_EINVAL
 * unless a tracks binding with non-NULL d_link and d_scale is pending.  A pose binding is
 * optional and feeds the unit motions when it is pending at the time of this call.  views 3..8
 * (default 6), iters 1..16 (default 5), huber_px (default 1.0; INFINITY weights every view 1),
 * inlier_px (default 2.0): zero or negative means the default; DVO_EINVAL above the ranges, for
 * views 1 or 2, or for a NaN.  Bind refine last: clearing the landmark binding and every
 * dvo_stream_set_tracks and dvo_stream_set_track_poses call clear a pending refine binding.  It
 * travels with the batch and is written when it retires, after the tracks and the track poses,
 * on the stream's HIP stream with no read-back; a *_pairs call refuses it as it refuses tracks.
 * The first binding allocates 20 B per slot of the point buffer for every pair set (4 B of full
 * links, 16 B for the id kernel's two buffers), once; a stream that never binds it launches and
 * holds what it did before, and the landmark, link, scale and pose bytes of a batch do not
 * depend on the binding. */
int dvo_stream_set_track_refine(dvo_stream* s, dvo_landmark_refined* d_refined, dvo_track_id* d_id, int views,
                                int iters, double huber_px, double inlier_px);
/* The same for a k-NN stream; a detect call alone consumes nothing. */
int dvo_knn_stream_set_track_refine(dvo_knn_stream* s, dvo_landmark_refined* d_refined, dvo_track_id* d_id, int views,
                                    int iters, double huber_px, double inlier_px);

/* ---------------------------------------------------------------------------
 * Track bundle: each pair's window cameras and landmarks fitted jointly.  An opt-in companion of a
 * tracks binding.  The track poses fit a camera to fixed points and the refined landmarks fit a
 * point to fixed cameras, so each stops at the other's error; here the cameras of pair p's window
 * and all its landmarks move together, by damped Gauss-Newton steps with the points eliminated
 * (a Schur complement).  One window per pair: the windows of neighbouring pairs overlap and are
 * fitted independently, and the fitted cameras of the older frames are not an output.
 *
 * Pairs that take part.  Pair p with n landmarks in its full list takes part if n >= 1 and
 * n >= min_points (a pair whose record failed has none).  Nothing depends on the landmark cap.
 *
 * Cameras.  With (R_q, d_q, rho_q) the unit motions and (A_k, b_k), W the window cameras of the
 * section above computed with this binding's `views` (the poses feed the unit motions where a
 * track-poses binding was pending when this binding was made): V = W + 2 <= views cameras, each
 * (A, b) with x' = A x + b.  Camera 0 = (I, 0), frame p, fixed.  Camera 1 = (R_p, d_p), frame
 * p + 1.  Camera k + 1 = (A_k, b_k), frame p - k, for k = 1..W.  V = 2 where the window is empty
 * (pair 0 of a batch, a pair after a failed one, views = 2).
 *
 * Points.  Landmark o starts at its own X, Y, Z.  Its views are the "Views of landmark (p, o)"
 * of the section above with V in place of `views`: view v is seen by camera v, so a landmark with
 * m views sees cameras 0..m-1.  Pixels are normalised as there.
 *
 * One step, in double, every operation rounded once, in the written order.  kh = huber_px /
 * ((fx + fy) / 2).  Per landmark, its views in ascending v, every sum starting at +0.0; per view
 * with camera (A, b):
 *   P_i = ((A[i][0] * X0 + A[i][1] * X1) + A[i][2] * X2) + b[i]
 *   a view with !(P2 > 0) contributes +0.0 to every term below; otherwise
 *   a = 1 / P2, u = P0 * a, v = P1 * a, ru = u - nu, rv = v - nv, e2 = ru * ru + rv * rv
 *   w = 1 if e2 <= kh * kh, else kh / sqrt(e2)
 *   Ju[j] = a * (A[0][j] - u * A[2][j]),  Jv[j] = a * (A[1][j] - v * A[2][j])      (the point, j < 3)
 *   and for v >= 1, with b = -(u * a), c = -(v * a) (the left perturbation P <- omega x P + dt):
 *   Cu = (b * P1, a * P2 - b * P0, -(a * P1), a, 0, b)
 *   Cv = (c * P1 - a * P2, -(c * P0), a * P0, 0, a, c)
 * The landmark's sums over its views: the 6 terms w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]), i <= j row
 * by row, of V, and the 3 terms w * (Ju[i] * ru + Jv[i] * rv) of g.  Per camera c >= 1 it sees, one
 * view's terms each: W_c[r][j] = w * (Cu[r] * Ju[j] + Cv[r] * Jv[j]) (6 x 3), its 21 terms
 * w * (Cu[r] * Cu[s] + Cv[r] * Cv[s]), r <= s row by row, of U_c and its 6 terms
 * w * (Cu[r] * ru + Cv[r] * rv) of h_c.
 *   Damping: V[j][j] = V[j][j] + lambda * V[j][j].
 *   V = L D L^T by the loops of the track poses with 3 in place of 6.  A landmark with a pivot not
 *   > 0 contributes nothing to this step and keeps its X.
 *   V x = q for a right-hand side q: z[i] = q[i], then for k = 0..i-1: z[i] = z[i] - L[i][k] * z[k];
 *   y[i] = z[i] / D[i];  for i = 2..0: x[i] = y[i], then for k = i+1..2: x[i] = x[i] - L[k][i] * x[k].
 *   Y_c[r] = the solution for q = W_c[r] (6 rows of 3).
 * Reduced system of 6 (V - 1) unknowns, camera c's six at 6 (c - 1).  Every scalar below is one
 * chain: the landmarks' terms in ascending ordinal added onto +0.0 one at a time, a landmark that
 * failed above or does not see the camera (the later camera of the two) adding nothing:
 *   T_cc'[r][s] = sum of (Y_c[r][0] * W_c'[s][0] + Y_c[r][1] * W_c'[s][1]) + Y_c[r][2] * W_c'[s][2]
 *   Tg_c[r]     = sum of (Y_c[r][0] * g[0] + Y_c[r][1] * g[1]) + Y_c[r][2] * g[2]
 *   U_c[r][s], h_c[r] = the sums of the landmarks' terms
 * and then, the subtraction made last: for c < c': S_cc'[r][s] = -T_cc'[r][s];  S_cc[r][s] =
 * U_c[r][s] - T_cc[r][s] for r < s, and (U_c[r][r] + lambda * U_c[r][r]) - T_cc[r][r] on the
 * diagonal;  r_c[r] = h_c[r] - Tg_c[r].  Only the upper triangle of S is formed.  The order of a
 * sum depends on no workgroup size and no tiling.
 *   S delta = -r by the LDL^T of the track poses with 6 (V - 1) in place of 6, the same loops; a
 *   pivot not > 0 or a non-finite delta ends the pair DEGENERATE on the state before this step.
 *   Back-substitution per landmark that did not fail: q[j] = -g[j]; then for the cameras c >= 1 it
 *   sees, in ascending c, with dc = delta's six of camera c:
 *     t = W_c[0][j] * dc[0], then for r = 1..5: t = t + W_c[r][j] * dc[r];  q[j] = q[j] - t
 *   dx = the solution of V dx = q as above, X[j] = X[j] + dx[j].
 *   Cameras c >= 1: A <- C A, b <- C b + dc[3..6) by the Cayley map of the track poses on dc.
 * Exactly `iters` steps are taken unless one fails: no convergence test, no accept / reject inside
 * the loop.
 *
 * Cost of a state: per landmark, over its views in ascending v onto +0.0, rho = e2 if e2 <= kh *
 * kh, else (2 * kh) * sqrt(e2) - kh * kh (a view with !(P2 > 0) adds +0.0); the landmarks' values
 * in ascending ordinal onto +0.0.  cost0 is the cost of the start state, cost that of the state
 * after the last step taken.
 *
 * Guard and gauge.  s = sqrt((b0 * b0 + b1 * b1) + b2 * b2) of camera 1 after the last step.  The
 * fit is kept if at least one step was taken, s > 0 with 1 / s finite, and cost <= cost0.  A kept
 * fit is divided by s: every b[i] of the cameras c >= 1 and every X[j] of every landmark becomes
 * itself / s, so that |t| = 1 and the points stand where the raw ones stand (camera of frame p,
 * units of baseline p); ratio = 1 / sqrt((b0 * b0 + b1 * b1) + b2 * b2) of camera 2 after that
 * division (baseline p over baseline p - 1, what scale[p].ratio and pose[p].scale estimate), 0.0
 * when V = 2.  The scale is left to the damping during the steps: the cost does not change along
 * it.  A fit that is not kept leaves the start values in every output, byte for byte: R_p, d_p,
 * the raw X, and ratio = rho_p (0.0 when V = 2); cost still reports the last state's cost.  A
 * caller never gets a worse state than it put in.
 *
 * Final pass on the output state, as in the section above: per landmark n_used, n_inliers, rms
 * and views; its iters = the steps that moved it, its status DVO_TRACK_REFINE_OK where every step
 * taken moved it, DVO_TRACK_REFINE_DEGENERATE where its own factorisation failed in one, and
 * DVO_TRACK_REFINE_NONE with iters 0 where the fit was not kept.  Per pair n_points = n, n_obs =
 * the sum of the landmarks' views, n_inliers = the sum of theirs, rms = sqrt(the landmarks'
 * inlier sums of e in ascending ordinal onto +0.0 / n_inliers), 0.0 with none; rms0 is the same
 * on the start state.
 *
 * Status.  DVO_TRACK_BUNDLE_OK.  DVO_TRACK_BUNDLE_NONE: the pair does not take part: R_p, d_p,
 * and 0 in every other field; its landmarks' slots hold the raw X, views 2, DVO_TRACK_REFINE_NONE.
 * DVO_TRACK_BUNDLE_DEGENERATE: a step failed (the steps before it count, and are kept if the
 * guard lets them), or s was not usable.  DVO_TRACK_BUNDLE_NOT_IMPROVED: !(cost <= cost0).
 * V comes from the window, not from the chains: a window camera that no landmark of the pair sees
 * (every track shorter than the window) has a zero block in S, the first step fails and the pair
 * ends DEGENERATE on its start values; where tracks are short, bind fewer views. */
#define DVO_TRACK_BUNDLE_OK 0
#define DVO_TRACK_BUNDLE_NONE 1
#define DVO_TRACK_BUNDLE_DEGENERATE 2
#define DVO_TRACK_BUNDLE_NOT_IMPROVED 3
#define DVO_TRACK_BUNDLE_LAMBDA 1e-6 /* the default damping */
typedef struct {              /* 160 bytes */
    double R[9], t[3];        /* camera p + 1 from camera p: x' = R x + t, |t| = 1 for a kept fit */
    double ratio;             /* baseline p over baseline p - 1; 0.0 when n_cams = 2 */
    double cost0, cost;       /* the Huber cost of the start and of the last state, normalised units squared */
    double rms0, rms;         /* the inliers' rms in pixels on the start and on the output state */
    int32_t n_points, n_obs, n_inliers, n_cams, iters, status;
} dvo_track_bundle;
#ifdef __cplusplus
static_assert(sizeof(dvo_track_bundle) == 160, "layout");
#else
_Static_assert(sizeof(dvo_track_bundle) == 160, "layout");
#endif
/* Binds d_bundle [pairs] and d_points [pairs][the landmark binding's cap] (laid slot for slot
 * beside the landmarks; slots [0, min(count, cap)) are written, bytes outside them are not
 * touched) for the NEXT batch only.  Either may be NULL; both NULL clears a pending binding.
 * DVO_EINVAL unless a tracks binding with non-NULL d_link and d_scale is pending.  A pose binding
 * is optional and feeds the unit motions when it is pending at the time of this call; a refine
 * binding is not required.  views 2..8 (default 6), iters 1..16 (default 5), lambda (default
 * DVO_TRACK_BUNDLE_LAMBDA), huber_px (default 1.0; INFINITY weights every view 1), inlier_px
 * (default 2.0), min_points >= 6 (default 8): zero or negative means the default; DVO_EINVAL above
 * the ranges, for views 1, for min_points 1..5, or for a NaN.  Bind the bundle last: clearing the
 * landmark binding and every dvo_stream_set_tracks, dvo_stream_set_track_poses and
 * dvo_stream_set_track_refine call clear a pending bundle binding.  It travels with the batch and
 * is written when it retires, after the refine outputs, on the stream's HIP stream with no
 * read-back; a *_pairs call refuses it as it refuses tracks.  The first binding allocates 36 B
 * per slot of the point buffer for every pair set (32 B for a landmark's current X and step
 * count, 4 B of full links for batches without a refine binding), once; a stream that never
 * binds it launches and holds what it did before, and the landmark, link, scale, pose, id and
 * refined bytes of a batch do not depend on the binding. */
int dvo_stream_set_track_bundle(dvo_stream* s, dvo_track_bundle* d_bundle, dvo_landmark_refined* d_points, int views,
                                int iters, double lambda, double huber_px, double inlier_px, int min_points);
/* The same for a k-NN stream; a detect call alone consumes nothing. */
int dvo_knn_stream_set_track_bundle(dvo_knn_stream* s, dvo_track_bundle* d_bundle, dvo_landmark_refined* d_points,
                                    int views, int iters, double lambda, double huber_px, double inlier_px,
                                    int min_points);

/* ---------------------------------------------------------------------------
 * Track PnP: each pair's 6-DoF pose from a P3P RANSAC on the previous pair's landmarks.  An
 * opt-in companion of a tracks binding.  Every output above rests on pair p's own essential
 * matrix: a pair whose five-point RANSAC or recoverPose fails (a near-pure rotation, a short
 * baseline, a planar scene) has no landmarks, links nothing, gets DVO_TRACK_POSE_NONE and
 * breaks the chain of scales.  The previous pair has already put 3-D points into camera j, and
 * pair p's raw match list says where those keypoints are in frame j + 1: a pose from 3-D to 2-D
 * correspondences needs neither pair p's E nor its triangulation.  Raw matches are not filtered
 * by E, hence the minimal-solver RANSAC in front of the track-pose steps.
 *
 * Correspondences of pair p >= 1 (frames j, j + 1).  Match i of pair p's match list, in the
 * order of dvo_stream_get_matches, i < rec[p].n_matches, whatever rec[p].status is, has (q, t)
 * and second-frame pixels (x2, y2).  It is a correspondence iff pair p - 1's landmarks hold
 * one whose match has trainIdx == q; the smallest such ordinal if several qualify, as the link
 * takes it.  Correspondences go in ascending i, k = 0..n-1 with n = n_corr.  Correspondence k has
 *   Y = (y0, y1, y2)   the y_i of the tracks section from that landmark and pair p - 1's record;
 *   (nu, nv)           x2, y2 normalised as in the track-pose section;
 *   f = (nu / l, nv / l, 1 / l) with l = sqrt((nu * nu + nv * nv) + 1), its unit bearing.
 * Pair 0 of a batch has none, and neither has a pair whose predecessor has no landmarks.
 *
 * Samples.  `hyps` samples per pair, h = 0..hyps-1.  With mwc_step the cv::RNG step
 * s' = (uint32)s * 4164903690 + (s >> 32) and seed' = seed, or (uint64)-1 (the E-RANSAC's) where
 * seed == 0: the state of sample h is the one 8 h steps after seed'.  A draw is s = mwc_step(s),
 * idx = (uint32)s % n.  i0 is the first draw, i1 the first later draw != i0, i2 the first later
 * draw not in {i0, i1}.  A sample takes at most 8 draws; one that has not found three indices by
 * then is void.  The samples depend on n, h and the seed only.
 *
 * P3P, per sample, on (Y_0, f_0), (Y_1, f_1), (Y_2, f_2) in the sample's order.  In double, every
 * operation one of + - * / sqrt rounded once, in the written order; negation, comparison, |x| and
 * max select exactly.  Polynomials are listed from the constant term up.
 *   c01 = (f0x * f1x + f0y * f1y) + f0z * f1z, c02 and c12 alike
 *   e1 = Y_1 - Y_0, e2 = Y_2 - Y_0, g = Y_2 - Y_1
 *   a01 = (e1x * e1x + e1y * e1y) + e1z * e1z, a02 from e2 and a12 from g alike
 * With depths d1 = u d0, d2 = v d0 the three side equations
 * d_i^2 + d_j^2 - 2 d_i d_j c_ij = a_ij leave two quadratics in u,
 * p2 u^2 + p1 u + P0(v) = 0 and q2 u^2 + Q1(v) u + Q0(v) = 0:
 *   p2 = a02, p1 = -((2 * a02) * c01), q2 = a12 - a01
 *   P0 = (a02 - a01, (2 * a01) * c02, -a01)
 *   Q1 = (-((2 * a12) * c01), (2 * a01) * c12),  Q0 = (a12, 0, -a01)
 *   A_k = p2 * Q0_k - P0_k * q2  (k = 0, 1, 2)
 *   B_0 = p2 * Q1_0 - p1 * q2,  B_1 = p2 * Q1_1
 *   C_0 = p1 * Q0_0 - P0_0 * Q1_0
 *   C_1 = p1 * Q0_1 - (P0_0 * Q1_1 + P0_1 * Q1_0)
 *   C_2 = p1 * Q0_2 - (P0_1 * Q1_1 + P0_2 * Q1_0)
 *   C_3 = -(P0_2 * Q1_1)
 * Their resultant G = A^2 - B C is a quartic in v:
 *   G_0 = A_0 * A_0 - B_0 * C_0
 *   G_1 = 2 * (A_0 * A_1) - (B_0 * C_1 + B_1 * C_0)
 *   G_2 = (2 * (A_0 * A_2) + A_1 * A_1) - (B_0 * C_2 + B_1 * C_1)
 *   G_3 = 2 * (A_1 * A_2) - (B_0 * C_3 + B_1 * C_2)
 *   G_4 = A_2 * A_2 - B_1 * C_3
 * Ferrari.  b = G_3 / G_4, c = G_2 / G_4, d = G_1 / G_4, e = G_0 / G_4, b2 = b * b,
 *   p = c - 0.375 * b2
 *   q = (d - 0.5 * (b * c)) + 0.125 * (b2 * b)
 *   r = ((e - 0.25 * (b * d)) + 0.0625 * (b2 * c)) - 0.01171875 * (b2 * b2)
 * The resolvent g(m) = ((m + k2) * m + k1) * m + k0 with k2 = p, k1 = 0.25 * (p * p) - r,
 * k0 = -(0.125 * (q * q)) has g(0) <= 0.  From lo = 0, hi = 1 + max(|k2|, |k1|, |k0|), exactly
 * 100 times: mid = 0.5 * (lo + hi); hi = mid if g(mid) > 0, else lo = mid.  Then m = hi,
 *   s = sqrt(2 * m), hh = 0.5 * p + m, w = q / (2 * s)
 *   rt0 = sqrt(s * s - 4 * (hh + w)), rt1 = sqrt(s * s - 4 * (hh - w))
 *   y = 0.5 * (s + rt0), 0.5 * (s - rt0), 0.5 * (rt1 - s), 0.5 * (-s - rt1)   candidates 0..3
 * Per candidate: v = y - 0.25 * b, u = -(((A_2 * v + A_1) * v + A_0) / (B_1 * v + B_0)),
 *   d0 = sqrt(a02 / ((1 + v * v) - (2 * v) * c02)), d1 = u * d0, d2 = v * d0
 * then exactly 5 Newton steps on the three depths:
 *   r0 = ((d0 * d0 + d1 * d1) - (2 * (d0 * d1)) * c01) - a01, r1 (d0, d2, c02, a02) and
 *   r2 (d1, d2, c12, a12) alike
 *   j00 = 2 * (d0 - d1 * c01), j01 = 2 * (d1 - d0 * c01), j10 = 2 * (d0 - d2 * c02),
 *   j12 = 2 * (d2 - d0 * c02), j21 = 2 * (d1 - d2 * c12), j22 = 2 * (d2 - d1 * c12)
 *   det = -(j00 * (j12 * j21) + j01 * (j10 * j22)),  x = r1 * j22 - j12 * r2
 *   n0 = -(r0 * (j12 * j21)) - j01 * x
 *   n1 = j00 * x - r0 * (j10 * j22)
 *   n2 = (r0 * (j10 * j21) - j00 * (r1 * j21)) - j01 * (j10 * r2)
 *   d_i = d_i - n_i / det
 * Alignment of the two triangles.  The frame of three points Z_0, Z_1, Z_2:
 *   z1 = Z_1 - Z_0, z2 = Z_2 - Z_0, F1 = z1 / sqrt((z1x * z1x + z1y * z1y) + z1z * z1z)
 *   n = F1 x z2 (n0 = F1y * z2z - F1z * z2y, cyclically), F3 = n / sqrt((n0 * n0 + n1 * n1) + n2 * n2)
 *   F2 = F3 x F1
 * with E from the Y_i (z1 = e1, z2 = e2, the first norm sqrt(a01)) and F from X_i = d_i * f_i
 * (X_0 subtracted after the products):
 *   R[i][j] = (F1_i * E1_j + F2_i * E2_j) + F3_i * E3_j
 *   t_i = X_0i - ((R[i][0] * Y_0x + R[i][1] * Y_0y) + R[i][2] * Y_0z)
 * A candidate is kept iff d0, d1, d2 > 0 and every entry of R and t is finite.  The kept
 * candidates, in candidate order, are the sample's solutions 0, 1, ...: up to 4.
 *
 * Score and choice.  A correspondence supports a pose iff it is an inlier of the track-pose
 * final pass under that pose: P2 > 0 and (fx * ru) * (fx * ru) + (fy * rv) * (fy * rv) <=
 * inlier_px * inlier_px.  A pose's score is the integer count of its supporters, so no sum order
 * enters the choice.  The winner has the largest count; ties go to the smaller h, then to the
 * smaller solution index.  n_best is its count, sample and solution its indices.
 *
 * Polish.  The polish set is the winner's supporters, fixed from here on, in ascending k; its
 * j-th member takes the place of correspondence j in the track-pose section's "One step" (the
 * same 27 terms, Huber weight, lane, tree and group sum order, LDL^T and Cayley update).  `iters`
 * steps from the winner's R, t; then the track-pose final pass over all n correspondences gives
 * n_used, n_inliers, rms and scale = |t|.
 *
 * Status.  DVO_TRACK_PNP_NONE: pair 0 of a batch, or n_corr < min_points; the struct is zero
 * apart from status and n_corr.  DVO_TRACK_PNP_NO_MODEL: no sample has a kept solution (n_best
 * 0, sample and solution -1), or n_best < min_points (n_best, sample and solution of the best
 * found); R, t, scale, rms, n_used, n_inliers and iters are zero.  DVO_TRACK_PNP_DEGENERATE: a
 * polish step failed; the pose of the step before is kept, the final pass runs on it and iters is
 * the number of steps taken.
 *
 * Mask (optional).  d_mask [pairs][mask_cap] bytes: for match index i < min(n_matches, mask_cap)
 * 1 where match i is a correspondence and a final-pass inlier, 0 otherwise (all 0 for a NONE or
 * NO_MODEL pair); bytes outside that range are not touched.
 *
 * Out of scope: landmarks triangulated from the PnP pose (the pair after a failed pair still has
 * no correspondences), chains across a batch boundary, the sharded runners, the single-pair calls
 * and early termination of the hypothesis loop. */
#define DVO_TRACK_PNP_OK 0
#define DVO_TRACK_PNP_NONE 1
#define DVO_TRACK_PNP_DEGENERATE 2
#define DVO_TRACK_PNP_NO_MODEL 3
typedef struct {              /* 144 bytes */
    double R[9], t[3];        /* camera j + 1 from camera j: x' = R x + t, |t| in units of pair p - 1's baseline */
    double scale, rms;        /* |t|: baseline p over baseline p - 1, as dvo_track_pose; pixels */
    int32_t n_corr, n_best, n_used, n_inliers, sample, solution, iters, status;
} dvo_track_pnp;
#ifdef __cplusplus
static_assert(sizeof(dvo_track_pnp) == 144, "layout");
#else
_Static_assert(sizeof(dvo_track_pnp) == 144, "layout");
#endif
/* Binds d_pnp [pairs] and, where d_mask is not NULL, d_mask [pairs][mask_cap] for the NEXT batch
 * only.  DVO_EINVAL unless a tracks binding is pending (either of its buffers will do: only the
 * table of landmarks is read), or where d_mask goes with mask_cap < 1.  hyps 1..512 (default 128),
 * iters 1..32 (default 10), huber_px (default 1.0; INFINITY weights every correspondence 1),
 * inlier_px (default 2.0), min_points >= 4 (default 6): zero or negative means the default;
 * DVO_EINVAL above the ranges, for min_points 1..3, or for a NaN.  seed: 0 means (uint64)-1.
 * d_pnp == NULL clears a pending binding, as clearing the landmark binding and every
 * dvo_stream_set_tracks call do; the pose, refine and bundle setters leave it alone, and it clears
 * nothing.  It travels with the batch and is written last when the batch retires, on the stream's
 * HIP stream with no read-back; a *_pairs call refuses it as it refuses tracks.  The first binding
 * allocates 48 B per slot of the point buffer (a correspondence's Y, nu, nv, its match index and
 * the polish set's index) and 4 B per 256 slots for every pair set, once; a stream that never
 * binds it launches and holds what it did before, and no other output of a batch depends on the
 * binding. */
int dvo_stream_set_track_pnp(dvo_stream* s, dvo_track_pnp* d_pnp, uint8_t* d_mask, int mask_cap, int hyps, int iters,
                             double huber_px, double inlier_px, int min_points, uint64_t seed);
/* The same for a k-NN stream; a detect call alone consumes nothing. */
int dvo_knn_stream_set_track_pnp(dvo_knn_stream* s, dvo_track_pnp* d_pnp, uint8_t* d_mask, int mask_cap, int hyps,
                                 int iters, double huber_px, double inlier_px, int min_points, uint64_t seed);
/* The samples of n >= 1 correspondences on the host (the kernel's text): out[hyps][3], a void
 * sample -1, -1, -1.  DVO_EINVAL for n < 1 or hyps outside 1..512. */
int dvo_track_pnp_samples_host(int n, int hyps, uint64_t seed, int32_t* out);
/* The P3P solver on the host (the kernel's text): Y the three points, nunv their (nu, nv);
 * R[4][9], t[4][3] the kept solutions in order, *n_solutions their number. */
int dvo_p3p_host(const double* Y, const double* nunv, double* R, double* t, int* n_solutions);

/* Test hooks: exercise one device algorithm in isolation. */
/* KeyPointsFilter::retainBest permutation on `n` float responses (GPU emulation
 * of libstdc++ nth_element + partition); depth < 0 = libstdc++ default. */
int dvo_test_retain_best(dvo_ctx* ctx, const float* resp, int n, int n_points, int depth, int semantics,
                         int32_t* perm, int* k_out);
/* RANSACUpdateNumIters on the device for a batch of (ep) values. */
int dvo_test_update_num_iters(dvo_ctx* ctx, double p, const double* ep, int n, int model_points, int max_iters,
                              int32_t* out);
/* findEssentialMat's RANSAC sampler (getSubset with cv::RNG((uint64)-1)) for
 * one pair of m >= 6 correspondences: idx gets n x 5 indices. */
int dvo_test_ransac_subsets(dvo_ctx* ctx, int m, int n, int32_t* idx);
/* The RANSAC bookkeeping (best model / niters / stop) over n hypotheses'
 * model counts (nmod: n, cnt: n x 10); out = {iterations, niters, max good,
 * best hypothesis, best model}. */
int dvo_test_ransac_replay(dvo_ctx* ctx, const int32_t* nmod, const int32_t* cnt, int n, int m, double prob,
                           int max_iters, int32_t* out);
/* Everything findEssentialMat's RANSAC kernels compute for the first n_hyp hypotheses
 * (hyp_cap = max_iters = n_hyp) of P >= 1 point sets, under one of the production schedules:
 *   DVO_TEST_SCHED_CALL          what dvo_find_essential_mat launches (one round, 16-lane
 *                                Durand-Kerner, stage C by rows, small score blocks); P = 1
 *   DVO_TEST_SCHED_BATCH_ONE     the stream batch kernels over [0, n_hyp) as one round
 *   DVO_TEST_SCHED_BATCH_ROUNDS  the stream batch schedule, round after round
 * pts: P x stride x {x1, y1, x2, y2} pixel coordinates, m: P counts (0 <= m[p] <= stride).
 * Per pair and hypothesis, copied from the kernels' arrays: subsets (x 5), nmod (-1: the
 * hypothesis was not evaluated), models (x 10 x 9) and cnt (x 10; a model that cannot exceed
 * max(4, the best count when its round started) may hold a partial count).  state: P x
 * {iterations, niters, max good, best hypothesis, best model}.  bounds: the *n_rounds round bounds
 * used (up to 8).  The one-round schedules also report path (P x n_hyp: 0 the fast Durand-Kerner
 * kernel's roots, 1 the trimmed-degree solver, 2 coincident roots redone in stage C, -1 not
 * evaluated) and parked (4: polynomials parked after Durand-Kerner pass k); BATCH_ROUNDS sets
 * both to -1 (its hypothesis records are round-local). */
#define DVO_TEST_SCHED_CALL 0
#define DVO_TEST_SCHED_BATCH_ONE 1
#define DVO_TEST_SCHED_BATCH_ROUNDS 2
int dvo_test_ransac_hypotheses(dvo_ctx* ctx, const double* pts, const int32_t* m, int P, int stride, const double* K,
                               double prob, double threshold, int n_hyp, int schedule, int32_t* subsets,
                               int32_t* nmod, double* models, int32_t* cnt, int32_t* state, int32_t* bounds,
                               int* n_rounds, int32_t* path, int32_t* parked);
/* 5-point kernel on one sample of 5 normalised correspondences. */
int dvo_test_five_point(dvo_ctx* ctx, const double* q1, const double* q2, double* models, int* n);
/* The batched RANSAC score's single-precision Sampson decision on one model E
 * (9 doubles) and n normalised correspondences (n x {x1, y1, x2, y2}) at the
 * squared threshold t: dec[i] = 1 inlier / 0 outlier / -1 left to the f64 test,
 * exact[i] = the f64 test (computeError, err <= t). */
int dvo_test_sampson(dvo_ctx* ctx, const double* E, const double* pts, int n, float t, int8_t* dec,
                     uint8_t* exact);
/* The ratio test and keypoint gather of dvo_knn_pair_run (v3:223-238) on a matcher's
 * k = 2 output: idx / dist nq x 2 (squared = 1: dist holds FLANN's squared L2), kq
 * (nkq >= nq) and kt the query and train keypoints.  Query q is kept when
 * (double)d0 < ratio * (double)d1.  pts: m x (x1, y1, x2, y2) floats, matches: m
 * entries, both in ascending q (caller buffers of nq entries); *missing_second = 1
 * when some idx[q][1] < 0. */
int dvo_test_ratio_gather(dvo_ctx* ctx, const int32_t* idx, const float* dist, int nq, const dvo_keypoint* kq, int nkq,
                          const dvo_keypoint* kt, int nkt, double ratio, int squared, float* pts, dvo_dmatch* matches,
                          int* m, int* missing_second);
/* The matching stages of dvo_knn_stream_process (frame state, byte pack, batched k-NN,
 * batched ratio test and gather) through the production launches, on host arrays:
 * `frames` frame slots of cap rows, desc [frames][cap][dim] (dim 128 or 64), kps
 * [frames][cap], counts [frames] (a count above cap marks the frame), ranges = train ranges
 * (0: the library's choice for frames - 1 pairs).  Per pair p = frames p, p + 1:
 * idx / dist [P][cap][2] (the first nq rows of a pair are written), nmatch [P], matches
 * [P][cap], pts [P][cap][4], hdr [P][4] (PairHeader: counts, flags, 0), missing [P];
 * *ranges_used = the ranges the launch ran with.  The arrays come back whole from the
 * context's reused device buffers: rows past a pair's nq (idx / dist) or nmatch (matches,
 * pts) hold whatever an earlier call left there. */
int dvo_test_knn_batch(dvo_ctx* ctx, const float* desc, const dvo_keypoint* kps, const int32_t* counts, int frames,
                       int cap, int dim, int ranges, double ratio, int32_t* idx, float* dist, int32_t* nmatch,
                       dvo_dmatch* matches, float* pts, int32_t* hdr, int32_t* missing, int* ranges_used);
/* dvo_bf_knn_hamming with the train stages split over tsplit workgroups per query block
 * (1..16; 0: the library's choice by size, what dvo_bf_knn_hamming runs).  The result does
 * not depend on tsplit. */
int dvo_test_bf_knn_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int k, int tsplit,
                            int32_t* train_idx, float* dist);
/* The ratio-mode match stage of dvo_stream (dvo_stream_set_ratio_test) through the production
 * launches, on host arrays: `frames` frame slots of cap rows (cap <= 8192), desc
 * [frames][cap][32], kps [frames][cap], counts [frames] (0..cap).  Per pair p = frames p, p + 1:
 * top2 [P][cap][2] the packed (Hamming << 16 | trainIdx) nearest and second words of the first
 * nq queries, -1 where there is none (and in the rows past nq), nmatch [P], matches [P][cap]
 * (entries past nmatch are (-1, -1, 0, 0)), pts [P][cap][4] (rows below nmatch are written),
 * status [P]: the status the pair's record gets before RANSAC (DVO_OK, DVO_ENOFEAT). */
int dvo_test_hamming_ratio_batch(dvo_ctx* ctx, const uint8_t* desc, const dvo_keypoint* kps, const int32_t* counts,
                                 int frames, int cap, double ratio, int32_t* top2, int32_t* nmatch, dvo_dmatch* matches,
                                 float* pts, int32_t* status);
/* The batched kd-forest build and search of dvo_knn_stream_process's FLANN mode through the
 * production launches, on host arrays: desc [frames][cap][dim], counts [frames] (a count above
 * cap marks the frame), state = the incoming theRNG state, levels = level launches per tree
 * before the tail kernel (0: the library's 24).  idx / dist [P][cap][2] (squared L2; the first
 * nq rows of a pair are written, other rows hold whatever an earlier call left), starts [P] the
 * state each pair starts from, *state_out the state after the call, *n_global the queries that
 * took the global-heap pass, *depth the deepest tree level reached, counted from 1. */
int dvo_test_flann_batch(dvo_ctx* ctx, const float* desc, const int32_t* counts, int frames, int cap, int dim, int trees,
                         int checks, uint64_t state, int levels, int32_t* idx, float* dist, uint64_t* starts,
                         uint64_t* state_out, int* n_global, int* depth);
/* The landmark kernels (dvo_stream_set_landmarks; v3:303, recoverPose(..., triangulatedPoints))
 * on host arrays, at sizes no detector produces on demand: pts [pairs][stride][4] pixel
 * coordinates, m [pairs] counts (5 <= m[p] <= stride; stride need not be a multiple of 64).
 * Normalise and findEssentialMat under the per-call RANSAC schedule pair by pair, then the
 * stream's retire (E, recoverPose, the records) and the landmarks of all pairs at once.  out
 * [pairs][cap] is copied up whole before the run and back whole after it, so untouched slots
 * keep the caller's bytes; count [pairs]; rec [pairs] the records (n_kp_prev = n_kp_cur = m). */
int dvo_test_landmarks(dvo_ctx* ctx, const float* pts, const int32_t* m, int pairs, int stride, const double* K,
                       double prob, double threshold, int max_iters, double dist_thresh, int cap, dvo_landmark* out,
                       int32_t* count, dvo_pair_record* rec);
/* The three track kernels the streams launch (dvo_stream_set_tracks), on host arrays so that the
 * sizes can be set exactly: lm [pairs][cap] the FULL landmark lists (count[p] <= cap; only match,
 * X, Y, Z are read; match ascending and below m[p]), mq / mt [pairs][stride] the match indices
 * (m[p] <= stride of them, each in [0, kp_cap)), rec [pairs] the records (R and t are read).  The
 * lists are laid out tile by tile as the landmark kernels leave them (landmark i / 256 of the
 * match index).  link [pairs][cap_out] is copied up whole before the run and back whole after
 * it; cap_out may be below the counts.  scale [pairs]. */
int dvo_test_tracks(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq, const int32_t* mt,
                    const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride, int kp_cap,
                    int cap_out, int32_t* link, dvo_track_scale* scale);
/* dvo_test_tracks with the pose kernel (dvo_stream_set_track_poses): each landmark's x2, y2 are
 * read too (the pixel position in the pair's second frame), K [9] is the camera matrix and the
 * four parameters are the binding's, defaults included.  pose [pairs]. */
int dvo_test_track_poses(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                         const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                         int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                         int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose);
/* dvo_test_track_poses with the id and refine kernels (dvo_stream_set_track_refine): each
 * landmark's x1, y1 are read too, rf_views, rf_iters, rf_huber_px and rf_inlier_px are the
 * binding's four parameters, defaults included, and use_poses says whether the poses feed the
 * unit motions (a pose binding pending when refine was bound).  refined and id [pairs][cap_out]
 * are copied up whole before the run and back whole after it; either may be NULL. */
int dvo_test_track_refine(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                          const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                          int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                          int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, int rf_views,
                          int rf_iters, double rf_huber_px, double rf_inlier_px, int use_poses,
                          dvo_landmark_refined* refined, dvo_track_id* id);
/* dvo_test_track_poses with the bundle kernel (dvo_stream_set_track_bundle) and no refine binding:
 * each landmark's x1, y1 are read too, the six bd_ parameters are the binding's, defaults
 * included, and use_poses says whether the poses feed the unit motions.  bundle [pairs] and points
 * [pairs][cap_out] are copied up whole before the run and back whole after it; either may be NULL. */
int dvo_test_track_bundle(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                          const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                          int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                          int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, int bd_views,
                          int bd_iters, double bd_lambda, double bd_huber_px, double bd_inlier_px, int bd_min_points,
                          int use_poses, dvo_track_bundle* bundle, dvo_landmark_refined* points);
/* dvo_test_track_poses with the PnP kernels (dvo_stream_set_track_pnp) after it: xy2 [pairs][stride][2]
 * are the second-frame pixels of every match (a landmark's x2, y2 is overridden by its match's),
 * rec[p].n_matches is taken as m[p], and the six pnp_ parameters are the binding's, defaults
 * included.  pnp [pairs]; mask [pairs][mask_cap] is copied up whole before the run and back whole
 * after it, or NULL (then mask_cap is ignored). */
int dvo_test_track_pnp(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                       const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                       int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                       int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, const float* xy2,
                       int pnp_hyps, int pnp_iters, double pnp_huber_px, double pnp_inlier_px, int pnp_min_points,
                       uint64_t pnp_seed, dvo_track_pnp* pnp, uint8_t* mask, int mask_cap);

#ifdef __cplusplus
}
#endif
#endif /* DVO_H_ */
