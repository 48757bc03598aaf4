// Internal declarations shared by the HIP translation units of libdvo_hip.so.
//
// Numerics contract: every file is compiled with
// -ffp-contract=off and IEEE-correct f32/f64 division and sqrt, so each float
// expression is evaluated in source order exactly like the CPU restatement of
// OpenCV (no FMA contraction, round-to-nearest-even), which makes the device
// results bit-identical to the oracle, not merely close.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvo.h"

namespace dvo {


constexpr int kMaxLevels = 8;
// OpenCV semantics of the ORB path (dvo_orb_params.opencv_semantics): 4.x or 3.2.
constexpr int kOcv4 = DVO_OPENCV_4X, kOcv32 = DVO_OPENCV_32;
// FAST tile height (output rows).  Two-stream bench, 1280x720, round 2 kernel: 16 rows
// 66.8-67.2 K frames/s, 20: 67.7 K, 24: 68.2-69.1 K, 28: 65.7-66.1 K, 32: 67.1-67.9 K.  Round 3
// (per-wave compass/segment/score, word candidate lists, no separate blur pass;
// profiles/r03p_ab_fast_band_rows.txt, r03q_*): 20 73.7 K, 24 75.0 K, 28 75.9 K, 32 77.9 K
// (26 KB of LDS, still 6 workgroups per CU), 40 77.8 K (5 per CU), 48 76.9 K, 64 75.7 K:
// taller tiles cost fewer barriers and carried rows per output row.
#ifndef DVO_BAND_ROWS
#define DVO_BAND_ROWS 32
#endif
constexpr int kBandRows = DVO_BAND_ROWS;
constexpr int kFastTW = 124;        // FAST tile width (output columns; score columns 126 = LDS words 1..32)
constexpr int kBorder = 31;         // edgeThreshold == runByImageBorder border
constexpr int kMaxW = 4096;         // keys pack x, y in 12 bits each
#ifndef DVO_BLUR_TH
#define DVO_BLUR_TH 96
#endif
constexpr int kBlurTW = 248, kBlurTH = DVO_BLUR_TH;  // blur tile: 62 lanes x 4 columns, 4 waves x kBlurTH / 4 rows

// Per-level geometry of one ORB plan (identical for every frame of a stream).
struct LevelGeom {
    int w, h;
    float scale;          // getScale(l) = (float)pow(double(1.2f), l)
    int nper;             // features per level
    int pitch;            // row pitch of level l (l >= 1) in the pyramid slab, multiple of 16
    int bpitch;           // row pitch of level l in the blurred slab, multiple of 16
    int64_t pyr_off;      // byte offset of level l (l >= 1) in a frame's pyramid slab
    int64_t blur_off;     // byte offset of level l in a frame's blurred slab
    int xcoef_off, ycoef_off;  // resize coefficient tables of level l (l >= 1) in Buffers::coef
    int nbands;           // FAST tile rows (kBandRows each) over rows [31, h-31)
    int ntx;              // FAST tile columns (kFastTW each) over columns [31, w-31)
    int band_base;        // first FAST tile of this level within a frame (tile = band * ntx + col)
    int strip_base;       // first FAST column strip of this level within a frame (strip = level's col)
    int band_cap;         // candidate capacity per FAST tile
    int64_t band_cand_off;// u32 offset of this level's first tile slot within a frame
    int cand_cap;         // candidate capacity of the level (>= sum of its band caps)
    int64_t cand_off;     // u32 offset of this level's gathered list within a frame
    int tile_base;        // first blur tile of this level within a frame
    int tiles_x, tiles_y; // blur tiling
    int l32_x, l32_y;     // OpenCV 3.2 INTER_LINEAR tables of level l (l >= 1) in Buffers::coef32 (int4 entries)
    int l32_xs;           // columns below this take 3.2's SSE2 vertical pass, the rest the scalar one
};

struct Plan {
    int w, h, nlevels, nfeatures, kp_cap, fast_threshold;
    LevelGeom L[kMaxLevels];
    int64_t pyr_stride;       // bytes per frame (levels 1..7)
    int64_t blur_stride;      // bytes per frame (levels 0..7)
    int total_bands;          // FAST tiles per frame
    int total_strips;         // FAST column strips per frame (one workgroup each)
    int64_t band_cand_stride; // u32 per frame
    int64_t cand_stride;      // u32 per frame
    int total_tiles;          // blur tiles per frame
    int coef_total;           // ints in the resize coefficient table
    int coef32_total;         // ints in the OpenCV 3.2 resize tables
    int semantics;            // kOcv4 / kOcv32
};

// Resize coefficient of one destination column/row (resize.cpp INTER_LINEAR_EXACT):
// bits 0..12 source offset, 13..21 c1 (0..256, c0 = 256 - c1), 22..23 mode
// (0 interior, 1 clamp to src[0], 2 clamp to src[last]).
__host__ __device__ inline int coef_ofs(int c) { return c & 0x1FFF; }
__host__ __device__ inline int coef_c1(int c) { return (c >> 13) & 0x1FF; }
__host__ __device__ inline int coef_mode(int c) { return (c >> 22) & 3; }

// Device buffers of one stream (all sized for max_frames).
// Per-pair RANSAC state carried between the batch-wide round kernels
// (geometry.hip: sample -> solve -> score -> replay, at most two rounds).
struct RansacState {
    uint64_t rng;      // cv::RNG state after the last sampled subset
    int32_t niters;    // current adaptive iteration bound
    int32_t iter;      // iterations replayed so far
    int32_t maxgood;   // best inlier count so far
    int32_t h0, h1;    // hypotheses sampled in the current round: [h0, h1)
    int32_t m;         // correspondences
    int32_t best_h, best_i;  // best model: hypothesis, root
    int32_t pad[2];
};
constexpr int kDkMaxPasses = 4;  // Durand-Kerner passes per round (geometry.hip kDkBudgets)
// RANSAC rounds of a stream batch: round r solves hypotheses [bound[r-1], min(bound[r], niters)),
// the last round everything left.  A batch's pairs take one round per dvo_stream_submit call
// (the rounds of kRansacRounds consecutive batches run as ONE merged launch sequence), so a
// round costs no extra Durand-Kerner tail; dvo_stream_process runs them back to back.
// Hypotheses solved per pair at 1280x720 / 2000 features (oracle replay, tools/ransac_schedule_sim.py,
// profiles/r05c_*): 64 | rest 177.8, 32 | 64 | 128 | 256 | rest 141.9, for 132.2 iterations used.
#ifndef DVO_RANSAC_BOUNDS
#define DVO_RANSAC_BOUNDS 32, 64, 128, 256
#endif
constexpr int kRansacBounds[] = {DVO_RANSAC_BOUNDS, 1 << 30};
constexpr int kRansacRounds = sizeof(kRansacBounds) / sizeof(int);
constexpr int kMaxSets = 8;  // pair sets (batches in flight) of a merged round
static_assert(kRansacRounds <= kMaxSets, "one pair set per round in flight");
// One merged RANSAC round: launch pairs [0, nsets F) are nsets sets of F pairs (set k = pairs
// [k F, (k + 1) F), one stream batch each); set k runs round[k] (-1: idle) over its first
// npairs[k] pairs.  Round 0 starts a set's pairs (RNG, niters = maxIters).
struct RoundSpec {
    int nsets, F;
    int round[kMaxSets];
    int npairs[kMaxSets];
    int bound[kMaxSets];  // hypotheses bound of round r (the last: 1 << 30)
};
// Per-pair values the record needs from the frames (records_kernel), kept with the pair's set
// because the frames' buffers are rewritten by the next batch before the set retires.
struct PairHeader {
    int32_t nkp_prev, nkp_cur, flags, pad;
};

struct Buffers {
    uint8_t* pyr;
    uint8_t* blur;
    int32_t* coef;        // resize coefficient tables (Plan::coef_total ints)
    int32_t* coef32;      // OpenCV 3.2 resize tables (Plan::coef32_total ints)
    int32_t* band_cnt;    // [F][total_bands][kBandRows] FAST keeps per tile row
    uint32_t* band_cand;
    uint32_t* cand;       // gathered candidate keys (score<<24 | y<<12 | x)
    float* resp;          // Harris responses parallel to cand
    int32_t* sel_tmp;     // 2 * cand_stride per frame (Lpos / Rasc)
    int32_t* cnt1;        // [F][8] after FAST retainBest
    int32_t* cnt2;        // [F][8] after Harris retainBest
    dvo_keypoint* kps;    // [F][kp_cap]
    uint8_t* desc;        // [F][kp_cap][32] (also the matcher's operands, expanded in registers)
    int32_t* nkp;         // [F]
    int32_t* nn;          // [2][F][kp_cap] packed (dist << 16 | idx), -1 none
    int32_t* mq;          // [F][kp_cap] match queryIdx (sorted by (dist, q))
    int32_t* mt;          // [F][kp_cap] match trainIdx
    float* md;            // [F][kp_cap] match distance
    int32_t* status;      // [F] per-frame error flags
    // the match stage's outputs, in the pair set the batch fills (PairSets::view, device_mem.h)
    int32_t* nmatch;      // [F]
    float* pts;           // [F][kp_cap][4] (x1, y1, x2, y2) KeyPoint_convert pixel coords
    PairHeader* hdr;      // [F]
};


struct StreamParams {   // passed by value to every batch kernel
    Plan plan;
    Buffers buf;
    const uint8_t* frames;
    int64_t frame_stride;
    int in_pitch;
    int nframes;
    // Pair layout: 1 = a stream (pair p is frames p, p+1: each frame detected once and shared by two
    // pairs); 2 = independent pairs (pair p is frames 2p, 2p+1), the reference's own schedule, which
    // detects both frames of every pair (visual_odometry_v3.py:387-392).
    int pair_step;
};

__host__ __device__ inline int stream_pairs(const StreamParams& P) {
    return P.pair_step == 2 ? P.nframes / 2 : P.nframes - 1;
}
__host__ __device__ inline int pair_frame(const StreamParams& P, int p) { return P.pair_step == 2 ? 2 * p : p; }

__host__ __device__ inline const uint8_t* level_ptr(const StreamParams& P, int f, int l) {
    return l == 0 ? P.frames + (int64_t)f * P.frame_stride : P.buf.pyr + (int64_t)f * P.plan.pyr_stride + P.plan.L[l].pyr_off;
}
__host__ __device__ inline int level_pitch(const StreamParams& P, int l) { return l == 0 ? P.in_pitch : P.plan.L[l].pitch; }
__host__ __device__ inline uint8_t* blur_ptr(const StreamParams& P, int f, int l) {
    return P.buf.blur + (int64_t)f * P.plan.blur_stride + P.plan.L[l].blur_off;
}

// ---- numerics helpers shared by device code ----------------------------------
__device__ __forceinline__ int cv_round_f(float v) { return (int)__builtin_rintf(v); }
__device__ __forceinline__ int cv_round_d(double v) { return (int)__builtin_rint(v); }
__device__ __forceinline__ int cv_floor_d(double v) { int i = (int)v; return i - (i > v); }

__device__ __forceinline__ unsigned long long ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int lane_id() { return __lane_id(); }

// Arguments of the geometry kernels (findEssentialMat / recoverPose), shared by
// the batched stream and the per-call C-ABI entry points.
struct GeomArgs {
    const float* pts_f;     // [pairs][pts_stride][4] pixel coords (x1, y1, x2, y2) or null
    const double* pts_d;    // same layout in double, or null
    const int32_t* m_arr;   // [pairs] correspondence counts (device) or null
    int m_const;
    int64_t pts_stride;
    double fx, fy, cx, cy;
    double prob, threshold;
    int max_iters;
    double dist_thresh;
    double* npts;           // [pairs][pts_stride][4] normalised
    double* models;         // [pairs][hyp_cap][10][9] hypothesis models
    int32_t* nmod;          // [pairs][hyp_cap] models per hypothesis
    int32_t* cnt;           // [pairs][hyp_cap][10] inlier counts
    int32_t* subsets;       // [pairs][hyp_cap][5] sampled point indices
    RansacState* rs;        // [pairs]
    double* fprec;          // [round blocks][128][64] five-point records of the round (block = a_off[p] + (h - h0) / 64)
    int32_t* dk_off;        // [pairs + 1] round work-list offsets
    int32_t* a_off;         // [pairs + 1] 64-hypothesis blocks of the round before each pair
    int32_t* s_off;         // [pairs + 1] score blocks of the round before each pair
    int32_t* dk_ctl;        // [2 + kDkMaxPasses] -, pass-0 items, parked after pass k
    int32_t* dk_list;       // [kDkMaxPasses - 1][dk_list_cap] parked polynomials (work-list items)
    int64_t dk_list_cap;    // >= pairs * hyp_cap
    int hyp_cap;            // max(max_iters, 1)
    double* E;              // [pairs][90]
    int32_t* info;          // [pairs][4] rows, inliers, iters, status
    uint8_t* mask;          // [pairs][pts_stride] findEssentialMat mask, or null
    const uint8_t* mask_in; // [pairs][pts_stride] recoverPose input mask, or null
    double* Rt;             // [pairs][12] R row-major then t
    int32_t* good;          // [pairs]
    int32_t* pick;          // [pairs] chosen decomposition 0..3, or null
    uint8_t* pose_mask;     // [pairs][pts_stride][4] per-decomposition masks, or null
    double* pose_P;         // [pairs][72] decompositions [R1|t], [R2|t], [R1|-t], [R2|-t]; R1, R2, t
    int32_t* pose_cnt;      // [pairs][5] valid flag, cheirality counts of the 4 decompositions
};

constexpr int kStageNormalize = 1, kStageRansac = 2, kStagePose = 4, kStageFinish = 16;
// kStageOneRound: the per-call findEssentialMat (one pair): a single RANSAC round
// over every hypothesis up to maxIters, solved with one lane per root.  Stream
// batches keep the two-round schedule, so their records (n_hypotheses) do not
// depend on how a stream is split into batches or shards.
constexpr int kStageOneRound = 8;

// SIFT_create().detectAndCompute of one image (sift.hip).  Octave o has
// size ow[o] x oh[o] (octave 0 = the 2x upscaled input); its Gaussian layer l
// (0..5) starts at gp + gp_off[o * 6 + l] and DoG layer l (0..4) at
// dog + dog_off[o * 5 + l] (floats, rows of ow[o]).
constexpr int kSiftMaxOct = 16;
struct SiftLayout {         // what depends on the image size only
    int64_t gp_off[kSiftMaxOct * 6];
    int64_t dog_off[kSiftMaxOct * 5];
    int ow[kSiftMaxOct], oh[kSiftMaxOct];
    int noct;
    int cand_cap;
    int kp_cap;
};
struct SiftBufs {           // one frame's scratch and lists
    float* gp;
    float* dog;
    float* tmp;             // row-pass buffer, ow[0] * oh[0]
    int4* cand;             // (octave, layer, row, col) extrema
    int* ncand;
    dvo_keypoint* raw;      // refined, oriented keypoints (unsorted)
    int* nraw;
    int32_t* order;         // sort scratch, next power of two >= kp_cap
    dvo_keypoint* kps;      // final keypoints (sorted, deduplicated, input-image units)
    int* nkp;
    float* desc;            // kp_cap x 128
    int* flags;             // 1: candidate overflow, 2: keypoint overflow
};
struct SiftArgs : SiftLayout, SiftBufs {};

// The same for a group of frames of one size (launch_sift_group): b is frame 0's scratch, frame f's
// is b's pointers advanced by f strides (in elements; cand by cand_cap, raw by kp_cap, the four
// counters ncand / nraw / nkp / flags by 4).  b.kps and b.desc are unused: the final keypoints and
// descriptors go to the caller's slots, frame f's at out_kps + f * feat_cap and out_desc +
// f * feat_cap * 128 (entries below feat_cap only), its (count, flags) to out_n + 2 f.
struct SiftGroupArgs {
    SiftLayout l;
    SiftBufs b;
    int64_t gp_stride, dog_stride, tmp_stride, order_stride;
    dvo_keypoint* out_kps;
    float* out_desc;
    int32_t* out_n;
    int feat_cap;
    int fused_blur;  // the blurs of layers 1..5 in one launch each (blur_fused_group_kernel), not a row and a column pass
};

// SIFT_create(nfeatures).detectAndCompute's retainBest (retain_kernel / retain_group_kernel), between
// the sort and the descriptors.  With nfeatures > 0 the sort writes the whole deduplicated list (up
// to kp_cap) to `list`, and retain gathers the kept keypoints from there, in libstdc++'s order, into
// the detector's output list.  Frame f of a group has its arrays f strides further: list, resp and
// idx by kp_cap, lpos and rasc by kp_cap + 1.
struct SiftRetainArgs {
    int nfeatures;       // > 0
    dvo_keypoint* list;  // the sorted, deduplicated list retain reads
    float* resp;         // the responses retain_best_block permutes
    int32_t* idx;        // their positions in list, permuted with them
    int32_t* lpos;       // retain_best_block's position arrays, kp_cap + 1 each
    int32_t* rasc;
};

// SURF_create(hessianThreshold).detectAndCompute (surf.hip): nOctaves 4,
// nOctaveLayers 3, 64-d descriptors, orientation on.
constexpr int kSurfOct = 4, kSurfLayers = 5, kSurfTot = kSurfOct * kSurfLayers;
struct SurfHaar {  // resizeHaarPattern output: 4 corner offsets + weight (host-built)
    int p0, p1, p2, p3;
    float w;
};
struct SurfLayout {         // what depends on the image size only (and the call's threshold)
    int w, h, pitch;        // pitch: row pitch of img
    int64_t off[kSurfTot];  // element offset of each layer in det / trace
    int size[kSurfTot];     // (9 + 6 layer) << octave
    int rows[kSurfOct], cols[kSurfOct];
    const SurfHaar* haar;   // [kSurfTot][10]: Dx (3), Dy (3), Dxy (4) of calcLayerDetAndTrace
    const int8_t* apt;      // 113 x (i, j): the orientation disc, apt[n] = Point(i, j)
    const float* aptw;      // 113 weights gori[i + 6] * gori[j + 6]
    float thr;              // hessianThreshold
    int kp_cap;
    int nori;               // samples in the orientation disc (113)
    float gdesc[20];        // getGaussianKernel(20, 3.3)
};
struct SurfBufs {           // one frame's image, scratch and lists
    const uint8_t* img;     // the image on the device (rows SurfLayout::pitch apart)
    int32_t* sum;           // integral image, (h + 1) x (w + 1)
    float* det;             // per layer: rows x cols of the layer's octave
    float* trace;
    dvo_keypoint* raw;      // extrema after interpolation (unsorted)
    int* nraw;
    int32_t* order;         // sort scratch, next power of two >= kp_cap
    dvo_keypoint* kps;      // sorted (KeypointGreater), then oriented; size -1 = dropped
    float* dtmp;            // kp_cap x 64, descriptors in sorted order
    dvo_keypoint* out;      // compacted keypoints
    float* desc;            // compacted descriptors
    int* nout;
    int* flags;             // 2: keypoint overflow, 4: a descriptor window above 768
};
struct SurfArgs : SurfBufs, SurfLayout {};

// The same for a group of frames of one size (launch_surf_group): b is frame 0's scratch, frame f's
// is b's pointers advanced by f strides (in elements; raw and kps by kp_cap, dtmp by kp_cap * 64,
// the counters nraw / nout / flags by 4) and b.img the first frame of the chunk, frame f's image
// frame_stride bytes further per frame.  b.out and b.desc are unused: the kept keypoints and
// descriptors go to the caller's slots, frame f's at out_kps + f * feat_cap and out_desc +
// f * feat_cap * 64 (entries below feat_cap only), its (count, flags) to out_n + 2 f.
struct SurfGroupArgs {
    SurfLayout l;
    SurfBufs b;
    int64_t frame_stride, sum_stride, cell_stride, order_stride;  // cell_stride: det and trace
    dvo_keypoint* out_kps;
    float* out_desc;
    int32_t* out_n;
    int feat_cap;
    int large_first;  // describe serves the chunk's large windows (octaves 2 and 3) first, from per-frame queues
};

// ---- host entry points of the kernels (implemented in the .hip files) -------
// ev: optional table of 2*DVO_NSTAGES events recorded around each stage.
inline void mark(hipEvent_t* ev, int stage, int end, hipStream_t s) {
    if (ev) hipEventRecord(ev[2 * stage + end], s);
}
// group_ev: when the batch's detection runs in frame groups (orb_groups(F) > 0), 2 x 5 events per
// group (stages 0..4 of group g at group_ev[10 g ..]) instead of ev's stages 0..4.
hipError_t launch_orb(const StreamParams& P, hipStream_t s, hipEvent_t* ev = nullptr, hipEvent_t* group_ev = nullptr);
int orb_groups(int nframes);
// dvo_stream_pair's feature bookkeeping in one launch, per 4-byte word i of the frame-0 / frame-1 / cache
// feature arrays (keypoints, descriptors, count, status): rotate = 1 (frame 0 holds the new current
// frame): frame 1 <- frame 0, frame 0 <- cache, cache <- frame 0; rotate = 0: cache <- frame 1.
struct FeatSlots {
    uint32_t* a[3][4];  // [frame 0, frame 1, cache][kps, desc, count, status]
    int words[4];
};
hipError_t launch_feature_rotate(const FeatSlots& f, int rotate, hipStream_t s);
// GaussianBlur of every level into Buffers::blur, for dvo_stream_get_pyramid(blurred): the
// detection path blurs only the pixels describe_kernel samples.
hipError_t launch_blur(const StreamParams& P, hipStream_t s);
// tsplit > 1 splits every pair's train stages over tsplit workgroups (one pair alone fills the chip)
hipError_t launch_match(const StreamParams& P, int cross_check, hipStream_t s, hipEvent_t* ev = nullptr, int tsplit = 1);
// one_round: a single RANSAC round over every hypothesis up to maxIters on the 16-lane Durand-Kerner
// (kStageOneRound, the per-call schedule: E, R, t are the same, n_hypotheses differs)
hipError_t launch_geometry(const StreamParams& P, const GeomArgs& g, dvo_pair_record* records, hipStream_t s,
                           hipEvent_t* ev = nullptr, bool one_round = false);
hipError_t launch_geometry_args(const GeomArgs& g, int pairs, int stages, hipStream_t s);
// Stream batches (api.cpp dvo_stream_submit): the per-set pieces.  g_all spans every set (pairs
// [0, nsets F)); g_set is one set's view (PairSets::view).  Both frame streams launch a retiring
// set's landmarks and tracks through launch_pair_outputs (pair_outputs.h).
hipError_t launch_pair_header(const StreamParams& P, PairHeader* hdr, hipStream_t s);
hipError_t launch_ransac_round(const GeomArgs& g_all, const RoundSpec& spec, hipStream_t s);
hipError_t launch_retire(const GeomArgs& g_set, int pairs, const PairHeader* hdr, dvo_pair_record* records,
                         hipStream_t s);
// The landmarks of a retired set (dvo_stream_set_landmarks), after its records are final: per
// (tile of kLandmarkTile matches, pair) the inlier test, the chosen decomposition's
// triangulation and tests and an ordered compaction inside the tile into L.tmp / L.tcnt, then a
// scan over the pair's tile counts and the copy into the caller's slots.  g_set.pts_f holds the
// pixel coordinates.  The scratch is live only between the two launches.
constexpr int kLandmarkTile = 256;
struct LandmarkTmp {  // a landmark inside its tile
    double X, Y, Z;
    int32_t match, pad;
};
struct LandmarkScratch {
    LandmarkTmp* tmp = nullptr;  // [pairs][tiles][kLandmarkTile]
    int32_t* tcnt = nullptr;     // [pairs][tiles]
};
inline int landmark_tiles(int64_t pts_stride) { return (int)((pts_stride + kLandmarkTile - 1) / kLandmarkTile); }
hipError_t launch_landmarks(const GeomArgs& g_set, int pairs, const dvo_pair_record* records, const LandmarkScratch& L,
                            dvo_landmark* out, int32_t* count, int cap, hipStream_t s);
// The tracks of a retired set (dvo_stream_set_tracks; tracks.hip), right after its landmarks while
// L still holds the set's full lists: the table kernel (each landmark's ordinal, atomicMin, at its
// trainIdx), the link kernel (pair p's queryIdx looked up in pair p - 1's table; the link into the
// caller's slot, the ratio compacted in order into the pair's ratio array) and the select kernel
// (a workgroup per pair: exact radix select of the three ranks).  Match i of pair p has its
// indices at mq / mt [(p * idx_stride + i) * idx_step]: separate arrays (step 1), or the two
// fields of a dvo_dmatch array (step 4).  Only table rows [0, pairs) are preset.
constexpr int32_t kTrackEmpty = 0x7f7f7f7f;  // a table cell no landmark reached (the memset byte 0x7f)
constexpr int kTrackLds = 2048;              // ratios of a pair the select kernel keeps in LDS
// Track poses (dvo_stream_set_track_poses): with TrackArgs::pose set, the link kernel also writes a
// linked landmark's 3-D to 2-D correspondence (the header's Y, nu, nv) at the slot its ratio goes
// to, and after the select kernel the pose kernel (a workgroup per pair) moves the tiles'
// correspondences together, runs the header's Gauss-Newton steps on them from the record's R and
// ratio * t, and writes the caller's dvo_track_pose.
constexpr int kTrackPoseLds = 1024;  // correspondences of a pair the pose kernel keeps in LDS (40 KB)
constexpr int kTrackPoseMaxIters = 32;
struct TrackCorr {  // 40 B
    double y[3], nu, nv;
};
// Track ids and refined landmarks (dvo_stream_set_track_refine): with TrackArgs::flink set, the link
// kernel also writes every landmark's full link at its ordinal (the caller's d_link is capped and
// cannot serve a walk); after the pose kernel the id kernel ranks the lists by pointer jumping
// (1 + ceil(log2(pairs - 1)) launches, ping-pong over `rank`) and the refine kernel (grid as the
// link kernel) forms the pair's window cameras in LDS, walks at most views - 2 links per landmark
// and runs the header's Gauss-Newton steps from registers.
constexpr int kTrackRefineMaxViews = 8;
constexpr int kTrackRefineMaxIters = 16;
struct TrackRank {  // 8 B: the links followed so far and the ordinal reached, in pair p - age
    int32_t age, ord;
};
// Track bundle (dvo_stream_set_track_bundle): with TrackArgs::bd_x set the link kernel writes the
// full links as for a refine binding, and after the refine kernel the bundle kernel (a workgroup per
// pair) fits the pair's window cameras and all its landmarks jointly: per step the landmarks are
// linearised kBundleTile at a time into LDS, every entry of the reduced system is summed by its
// owner lane in ordinal order, the system is factored across lanes and solved on lane 0, and the
// landmarks back-substitute.  A landmark's current X and the steps that moved it live in bd_x.
constexpr int kTrackBundleMaxIters = 16;
struct BundlePoint {  // 32 B
    double X[3];
    int32_t steps, pad;
};
// Track PnP (dvo_stream_set_track_pnp): with TrackArgs::pnp set, after everything else the
// correspondence kernel (grid as the link kernel, over the pair's raw matches) looks every match's
// queryIdx up in pair p - 1's table and compacts the hits of its tile, in match order, into
// pnp_corr from slot tile * kLandmarkTile on (their number into pnp_cnt), and the PnP kernel (a
// workgroup per pair) moves the tiles' hits together, draws and solves the samples (p3p.h) in
// rounds of kPnpRound, a lane per sample, counts every pose's supporters (a wave per sample's
// poses, ballots), and polishes the winner with the pose kernel's step and final pass.
constexpr int kPnpRound = 64;      // samples solved per round: their poses take 24 KB of LDS
constexpr int kPnpMaxHyps = 512;
struct PnpCorr {  // 48 B
    double y[3], nu, nv;
    int32_t match;  // the match index i
    int32_t sel;    // slot j: the j-th correspondence of the polish set (written by the PnP kernel)
};
struct TrackScratch {
    int32_t* table = nullptr;  // [sets][pairs][kp_cap] smallest landmark ordinal per trainIdx
    double* ratio = nullptr;   // [sets][pairs][pts_stride] a tile's linked ratios from its first ordinal on
    int32_t* lcnt = nullptr;   // [sets][pairs][tiles] linked landmarks per tile
    int32_t* iq = nullptr;     // [sets][pairs][pts_stride] the ORB stream's copy of queryIdx, trainIdx
    int32_t* it = nullptr;
    TrackCorr* corr = nullptr;  // [sets][pairs][pts_stride] a tile's correspondences, as ratio (first pose binding)
    int32_t* flink = nullptr;   // [sets][pairs][pts_stride] every landmark's full link at its ordinal (first refine binding)
    TrackRank* rank = nullptr;  // [sets][2][pairs][pts_stride] the id kernel's ping-pong buffers (first refine binding)
    BundlePoint* bx = nullptr;  // [sets][pairs][pts_stride] the bundle kernel's points (first bundle binding)
    int32_t* blink = nullptr;   // [sets][pairs][pts_stride] full links of its own, behind bx in the same allocation
    PnpCorr* pc = nullptr;      // [sets][pairs][pts_stride] the PnP correspondences (first PnP binding)
    int32_t* pc_cnt = nullptr;  // [sets][pairs][tiles] correspondences per tile, behind pc in the same allocation
};
struct TrackArgs {
    LandmarkScratch L;  // the set's full landmark lists
    int tiles;
    const int32_t *mq, *mt;
    int64_t idx_stride;
    int idx_step;
    const dvo_pair_record* rec;
    int32_t* table;
    int kp_cap;
    double* ratio;
    int64_t pts_stride;
    int32_t* lcnt;
    int32_t* link;  // the caller's [pairs][cap], or null
    int cap;
    dvo_track_scale* scale;  // the caller's [pairs], or null
    // track poses; all unused while pose is null
    dvo_track_pose* pose;  // the caller's [pairs], or null (needs scale)
    const float* pts_f;    // [pairs][pts_stride][4] the set's pixel coordinates (x2, y2 are read)
    double fx, fy, cx, cy;
    TrackCorr* corr;  // [pairs][pts_stride]
    int pose_iters, pose_min_points;  // 1..kTrackPoseMaxIters, >= 3
    double huber_px, inlier_px;       // > 0
    // track ids and refined landmarks; all unused while flink is null (pts_f and the camera are read too)
    int32_t* flink;                 // [pairs][pts_stride]
    TrackRank* rank;                // [2][pairs][pts_stride]; the second buffer starts at rank + rank_stride
    int64_t rank_stride;
    dvo_track_id* id;               // the caller's [pairs][cap], or null
    dvo_landmark_refined* refined;  // the caller's [pairs][cap], or null
    int rf_views, rf_iters;         // 3..kTrackRefineMaxViews, 1..kTrackRefineMaxIters
    int rf_use_pose;                // the unit motions come from `pose` where its status is OK
    double rf_huber_px, rf_inlier_px;  // > 0
    // track bundle; all unused while bd_x is null (flink, pts_f, scale and the camera are read too)
    BundlePoint* bd_x;                // [pairs][pts_stride]
    dvo_track_bundle* bundle;         // the caller's [pairs], or null
    dvo_landmark_refined* bd_points;  // the caller's [pairs][cap], or null
    int bd_views, bd_iters;           // 2..kTrackRefineMaxViews, 1..kTrackBundleMaxIters
    int bd_min_points, bd_use_pose;   // >= 6; the unit motions come from `pose` where its status is OK
    double bd_lambda, bd_huber_px, bd_inlier_px;  // > 0
    // track PnP; all unused while pnp is null (rec's n_matches, pts_f and the camera are read too)
    dvo_track_pnp* pnp;   // the caller's [pairs], or null
    uint8_t* pnp_mask;    // the caller's [pairs][pnp_mask_cap], or null
    int pnp_mask_cap;
    PnpCorr* pnp_corr;    // [pairs][pts_stride]
    int32_t* pnp_cnt;     // [pairs][tiles]
    int pnp_hyps, pnp_iters, pnp_min_points;  // 1..kPnpMaxHyps, 1..kTrackPoseMaxIters, >= 4
    double pnp_huber_px, pnp_inlier_px;       // > 0
    uint64_t pnp_seed;                        // 0: the E-RANSAC's
};
hipError_t launch_tracks(const TrackArgs& a, int pairs, hipStream_t s);
// five-point record blocks a merged round can need (sizes the stream's GeomArgs::fprec, dk_list)
int64_t round_blocks_bound(int F, int hyp_cap);
int64_t round_items_bound(int F, int hyp_cap);
// Undistortion (undistort.hip): camera K, distortion k1 k2 p1 p2 k3 k4 k5 k6 s1..s4.
struct UndistortGeom {
    int w, h, stripe;
    double K[9];
    double dist[12];
};
hipError_t launch_undistort_map(const UndistortGeom& U, const double* d_ir, int16_t* d_xy, uint16_t* d_frac,
                                hipStream_t s);
hipError_t launch_undistort_remap(const UndistortGeom& U, const int16_t* d_xy, const uint16_t* d_frac,
                                  const uint8_t* d_src, int n, int64_t src_fstride, int src_pitch, uint8_t* d_dst,
                                  int64_t dst_fstride, int dst_pitch, hipStream_t s);
// Colour input (color.hip): gray = (B cb + G cg + R cr + (1 << (shift - 1))) >> shift, the pixel's
// bytes in B, G, R order (a fourth byte is ignored).  The kernels take the set as an argument;
// kGray14 is cv.cvtColor(COLOR_BGR2GRAY)'s, the only one the ABI exposes.
struct GrayCoef {
    int cb, cg, cr, shift;
};
constexpr GrayCoef kGray14{1868, 9617, 4899, 14};
// n frames of w x h pixels of `channels` (3 or 4) bytes -> n mono8 frames; src and dst must not overlap
hipError_t launch_bgr2gray(const GrayCoef& c, const uint8_t* d_src, int n, int64_t src_fstride, int src_pitch,
                           int channels, int w, int h, uint8_t* d_dst, int64_t dst_fstride, int dst_pitch,
                           hipStream_t s);
// launch_undistort_remap of the gray image of colour frames, without storing that image
hipError_t launch_undistort_remap_bgr(const UndistortGeom& U, const int16_t* d_xy, const uint16_t* d_frac,
                                      const GrayCoef& c, const uint8_t* d_src, int n, int64_t src_fstride,
                                      int src_pitch, int channels, uint8_t* d_dst, int64_t dst_fstride,
                                      int dst_pitch, hipStream_t s);

// Baseline JPEG frames (jpeg.hip; plans and segments: jpeg.h).  Entropy: every segment of a frame
// group into the frames' zeroed coefficients, status[frame] = DVO_ECORRUPT where one is corrupt.
// IDCT: coefficients -> u8 component planes.  Colour: planes -> gray (1), BGR (3) or BGRA (4) frames.
namespace jpeg {
struct FramePlan;
struct Segment;
}  // namespace jpeg
hipError_t launch_jpeg_entropy(const jpeg::FramePlan* d_plans, const jpeg::Segment* d_segs, int nseg,
                               const uint8_t* d_bytes, int16_t* d_coef, int32_t* d_status, hipStream_t s);
// The segments of a group that are long enough to be split (jpeg_split.h): one workgroup each, lane i
// on the i-th run of split_bytes bytes; max_runs: the most runs a segment of the list has.  d_info:
// 3 counters (most synchronisation passes, segments, one-lane fallbacks), or null.
hipError_t launch_jpeg_entropy_split(const jpeg::FramePlan* d_plans, const jpeg::Segment* d_segs, int nseg, int split_bytes,
                                     int max_runs, const uint8_t* d_bytes, int16_t* d_coef, int32_t* d_status,
                                     int32_t* d_info, hipStream_t s);
hipError_t launch_jpeg_idct(const jpeg::FramePlan* d_plans, int nframes, int max_nblk, const int16_t* d_coef,
                            uint8_t* d_planes, hipStream_t s);
hipError_t launch_jpeg_color(const GrayCoef& c, const jpeg::FramePlan* d_plans, int nframes, int w, int h,
                             const uint8_t* d_planes, int out_channels, uint8_t* d_dst, int64_t dst_fstride,
                             int dst_pitch, hipStream_t s);

// carry: device [12 P_prev | 16 T_abs_prev]; updated in place.
// rec: the pairs' records (R, t, status, n_models are read).
hipError_t launch_pose_tail(const dvo_pair_record* rec, int pairs, const double* K, const double* cprev, const double* ccur, int k, double marker_length,
                            double* carry, double* T_rel, double* T_abs, hipStream_t s);
// T_abs[p] = T_carry . T_rel[0] ... T_rel[p] in pair order (the pose_tail chain on
// its own: the reassembled pose stream of a sharded run); T_carry is updated.
hipError_t launch_pose_chain(const double* T_rel /*[n][16]*/, int n, double* T_carry /*16*/, double* T_abs,
                             hipStream_t s);
// The pair-parallel half of the pose tail for pairs [p0, p0 + n) of a window of `pairs` records
// (T_rel[0 .. n)), then P_carry (12 doubles) advanced past the whole window.
hipError_t launch_pose_rel_range(const dvo_pair_record* rec, int pairs, int p0, int n, const double* K,
                                 const double* cprev, const double* ccur, int k, double marker_length, double* P_carry,
                                 double* T_rel, hipStream_t s);
hipError_t launch_triangulate(const double* d_P /*24*/, const double* d_x /*4 x k*/, int k, double* d_X, hipStream_t s);
// Float-descriptor kNN (NORM_L1 / squared L2), dim 64 or 128, k 1..4, over
// `ranges` = knn_ranges(nq, nt, CU count) train ranges; d_part / d_pidx hold
// ranges * nq * k partial slots (unused when ranges == 1).
int knn_ranges(int nq, int nt, int cus);
// d_bytes: knn_bytes_size(nq, nt, dim) bytes of workspace for the byte-valued fast path.
size_t knn_bytes_size(int nq, int nt, int dim);
hipError_t launch_knn_float(const float* d_q, int nq, const float* d_t, int nt, int dim, int k, int norm, int ranges,
                            void* d_bytes, float* d_part, int32_t* d_pidx, float* d_dist, int32_t* d_idx,
                            hipStream_t s);
// One-pair Hamming match (dvo_bf_match_hamming) on the stream's MFMA matcher;
// d_work: match_pair_work_size(nq, nt) bytes.  Output in queryIdx order.
size_t match_pair_work_size(int nq, int nt);
// d_taps: the 6 Gaussian kernels (initial blur, layers 1..5) back to back.
// R (nfeatures > 0): retainBest between the sort and the descriptors; null: everything is kept.
hipError_t launch_sift(const SiftArgs& A, const uint8_t* d_img, int w, int h, int stride, const float* d_taps,
                       const int* tap_off, const int* tap_n, hipStream_t s, const SiftRetainArgs* R = nullptr);
// The same stages for `frames` frames (<= the frames G's scratch holds), one launch per stage with
// the frame as a grid dimension; frame f's image is d_frames + f * frame_stride.  The caller has
// cleared the frames' counters.
hipError_t launch_sift_group(const SiftGroupArgs& G, int frames, const uint8_t* d_frames, int64_t frame_stride, int w,
                             int h, int stride, const float* d_taps, const int* tap_off, const int* tap_n,
                             hipStream_t s, const SiftRetainArgs* R = nullptr);
hipError_t launch_surf(const SurfArgs& a, hipStream_t s);
// The same stages for `frames` frames (<= the frames G's scratch holds), one launch per stage with
// the frame as a grid dimension.  The caller has cleared the frames' counters, det and trace.
hipError_t launch_surf_group(const SurfGroupArgs& G, int frames, hipStream_t s);
hipError_t launch_match_pair(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int cross_check, void* d_work,
                             dvo_dmatch* d_out, int* d_m, hipStream_t s);
// Hamming 2-NN + ratio test, the ORB stream's opt-in matcher (dvo_stream_set_ratio_test): what
// launch_match leaves for the geometry stage (mq / mt / md / pts / nmatch), kept matches in ascending
// queryIdx; P.buf.nn holds the packed nearest (forward half) and second (the other half) words.
hipError_t launch_match_ratio(const StreamParams& P, double ratio, hipStream_t s, hipEvent_t* ev = nullptr);
// its second step (ratio.hip): the ratio test and gather of every pair from the packed words
hipError_t launch_hamming_ratio(const StreamParams& P, double ratio, hipStream_t s);
// The reference raises in `for m, n in matches` on a pair whose train frame has fewer than 2
// descriptors: records[p] (null: none) becomes DVO_ENOFEAT with the counts, zeros elsewhere, unless
// the pair is DVO_ECAP or has no query (those keep their record); status[p] (null: none) the
// pair's status before RANSAC: DVO_ECAP, DVO_ENOFEAT or DVO_OK.
hipError_t launch_hamming_ratio_status(const PairHeader* hdr, int pairs, dvo_pair_record* records, int32_t* status,
                                       hipStream_t s);
// One pair's BFMatcher(NORM_HAMMING).knnMatch (k 1 or 2) on nn2_mfma_kernel: tsplit train splits
// (hamming_knn_split picks), d_work of hamming_knn_work_size(nq, tsplit) bytes, rows of k
// (index, distance), (-1, FLT_MAX) where fewer than k trains exist.
int hamming_knn_split(int nq, int nt);
size_t hamming_knn_work_size(int nq, int tsplit);
hipError_t launch_knn_hamming_pair(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int k, int tsplit,
                                   void* d_work, int32_t* d_idx, float* d_dist, hipStream_t s);
// FLANN randomized kd-tree k-NN (flann.hip; the 'flann' mode's FlannBasedMatcher).
struct FlannBuildArgs {
    const float* data;  // train set [n][dim]
    int n, dim;
    int* ind;           // [n]
    float* xv;          // [n]
    int* sl;            // [n]
    int* sr;            // [n]
    const uint32_t* R;  // [2n - 1] draws of the tree
    int4* nodes;        // [2n - 1] nodes of the tree
    int4* open0;        // [n] open nodes, even levels
    int4* open1;        // [n] open nodes, odd levels
    int* cnt;           // [n + 2] open nodes per level
};
struct FlannSearchArgs {
    const float* q;
    const float* t;
    const int4* nodes;  // [trees][2n - 1]
    int nq, n, dim, k, trees, checks;
    int32_t* idx;       // [nq][k]
    float* dist;        // [nq][k] squared L2
    int32_t* flag;      // [nq]
};
size_t flann_search_lds(int n);
hipError_t launch_flann_draws(const uint64_t* d_chunk_state, int nchunk, int total, uint32_t* d_R, hipStream_t s);
hipError_t launch_flann_shuffle(const uint32_t* d_R, int n, int* d_cnt, int* d_off, int* d_fill, int* d_list,
                                const int* d_ind, int* d_new_ind, hipStream_t s);
hipError_t launch_flann_root(const FlannBuildArgs& a, hipStream_t s);
hipError_t launch_flann_level(const FlannBuildArgs& a, int level, int max_open, hipStream_t s);
hipError_t launch_flann_search(const FlannSearchArgs& a, hipStream_t s);
hipError_t launch_flann_redo_list(const int32_t* d_flag, int nq, int32_t* d_list, int32_t* d_count, hipStream_t s);
hipError_t launch_flann_search_global(const FlannSearchArgs& a, const int32_t* d_list, int count, float* d_heap_d,
                                      int32_t* d_heap_n, hipStream_t s);
// ---- the batched kd-forest (dvo_knn_stream's FLANN mode): every pair's forest and search per launch ----
// Pair p is frame slots p (queries) and p + 1 (trains) of `cap` rows; its forest is built iff
// fstate gives it nq >= 1 and nt >= 2.  Nothing is read back: the theRNG state lives in *state,
// and the launch shapes depend on cap, frames, trees and the level count only.
constexpr int kFlannChunks = 64;    // draw chunks per tree (as flann_knn_device)
constexpr int kFlannLevels = 24;    // divideTree level launches per tree; the tail kernel runs what is left
constexpr int kFlannRedoPool = 64;  // workgroups of the global-heap pass, a heap of cap entries each
struct FlannBatchArgs {
    const float* desc;      // [F][cap][dim]
    const int32_t* fstate;  // [F][2]
    int cap, dim, trees, checks;
    int32_t* idx;           // [P][cap][2]
    float* dist;            // [P][cap][2] squared L2
    uint64_t* state;        // [1] theRNG state: read, and advanced past the built forests, by every launch
    int32_t* ctl;           // [4] {queries sent to the global-heap pass, deepest level + 1, 0, 0} of the last launch
    uint64_t* starts;       // [P] the state pair p's forest starts from
    uint64_t* cs;           // [P][trees][kFlannChunks] chunk start states
    uint32_t* R;            // [P][2 cap] the current tree's draws
    int* bcnt;              // [P][cap] shuffle buckets: count, fill, list, and offsets [P][cap + 1]
    int* bfill;
    int* blist;
    int* boff;
    int* ind;               // [P][cap] the point order, ping-pong between trees
    int* ind2;
    float* xv;              // [P][cap]
    int* sl;                // [P][cap]
    int* sr;                // [P][cap]
    int4* nodes;            // [P][trees][2 cap] (tree t of a pair at t (2 nt - 1))
    int4* open;             // [P][2][cap] open nodes, even / odd levels
    int* lev;               // [P][cap + 2] open nodes per level
    uint32_t* redo;         // [P cap] pair * cap + query of the queries whose heap outgrew LDS
    float* gheap_d;         // [kFlannRedoPool][cap]
    int32_t* gheap_n;
};
// The scratch arrays of P pairs (everything but desc, fstate, idx, dist): take(pointer, bytes)
// per array, false from take stops the walk.  flann_batch_bytes sums the same sizes.
template <class Take>
bool flann_batch_layout(FlannBatchArgs& a, int P_, int cap, int trees, Take&& take) {
    const size_t P = (size_t)P_, C = (size_t)cap, T = (size_t)trees;
    return take(a.state, 8) && take(a.ctl, 16) && take(a.starts, P * 8) && take(a.cs, P * T * kFlannChunks * 8) &&
           take(a.R, P * C * 8) && take(a.bcnt, P * C * 4) && take(a.bfill, P * C * 4) && take(a.blist, P * C * 4) &&
           take(a.boff, P * (C + 1) * 4) && take(a.ind, P * C * 4) && take(a.ind2, P * C * 4) && take(a.xv, P * C * 4) &&
           take(a.sl, P * C * 4) && take(a.sr, P * C * 4) && take(a.nodes, P * T * C * 32) && take(a.open, P * C * 32) &&
           take(a.lev, P * (C + 2) * 4) && take(a.redo, P * C * 4) && take(a.gheap_d, kFlannRedoPool * C * 4) &&
           take(a.gheap_n, kFlannRedoPool * C * 4);
}
size_t flann_batch_bytes(int pairs, int cap, int trees);
// RNG plan, then per tree draws / shuffle / root / `levels` level launches / tail, then the search
// and the global-heap pass of frames - 1 pairs: 3 + trees (levels + 8) launches.
// shard (a sharded stream's call, dvo_knn_stream_finish): draws[world] device words, the draws of
// every rank's pairs of the window; the plan starts after those of the ranks below `rank` and
// leaves the state past all of them.  draws[rank] is not read (the plan counts its own pairs).
struct FlannShard {
    const uint64_t* draws;
    int world, rank;  // world 1..kFlannShardMax
};
constexpr int kFlannShardMax = 1024;  // one entry per lane of the plan's workgroup
hipError_t launch_flann_batch(const FlannBatchArgs& a, int frames, int levels, hipStream_t s,
                              const FlannShard* shard = nullptr);
hipError_t launch_flann_set_state(uint64_t* d_state, uint64_t value, hipStream_t s);
// *d_draws = the draws the frames - 1 pairs of fstate will consume (0 with trees == 0), one workgroup.
hipError_t launch_flann_shard_draws(const int32_t* d_fstate, int frames, int trees, uint64_t* d_draws, hipStream_t s);
// The RNG plan's arithmetic on the host (the kernel's __host__ __device__ text): counts are
// detector counts (one above cap marks the frame), starts[frames - 1], *state_out after the call.
void flann_rng_plan_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees, uint64_t* starts,
                         uint64_t* state_out);
// The sharded plan on the host: one rank's frames (frames >= 0; fewer than 2 is a rank without
// pairs) with the ranks' draw counts shard_draws[world] (NULL: none before or after).  starts,
// state_out and own_draws may be NULL.
void flann_rng_shard_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees,
                          const uint64_t* shard_draws, int world, int rank, uint64_t* starts, uint64_t* state_out,
                          uint64_t* own_draws);
// The k-NN modes' ratio test, ordered compaction and keypoint gather (ratio.hip): query q of the
// matcher's k = 2 output is kept when (double)d0 < ratio * (double)d1, d the float32 values
// DMatch.distance holds (squared: sqrtf of FLANN's squared L2).  Kept matches in ascending q.
struct RatioArgs {
    const int32_t* idx;       // [nq][2] train indices (-1: no such neighbour)
    const float* dist;        // [nq][2]
    const dvo_keypoint* kq;   // [nkq] query (previous frame) keypoints, nkq >= nq
    const dvo_keypoint* kt;   // [nkt] train (current frame) keypoints
    int nq, nkq, nkt;
    double ratio;
    int squared;
    float* pts;               // [nq][4] (x1, y1, x2, y2): GeomArgs::pts_f
    dvo_dmatch* matches;      // [nq] (q, idx[q][0], 0, d0)
    int32_t* nmatch;          // kept count: GeomArgs::m_arr
    PairHeader* hdr;          // {nkq, nkt, 0, 0}
    int32_t* missing;         // 1 when some query has idx[q][1] < 0
};
hipError_t launch_ratio_gather(const RatioArgs& a, hipStream_t s);
// dvo_knn_pair_run: min(*cnt, kp_cap) keypoints and dim-float descriptors of a detection into a
// feature slot, dn = {*cnt, *flags}
hipError_t launch_feature_copy(const dvo_keypoint* skps, const float* sdesc, const int32_t* cnt, const int32_t* flags,
                               int kp_cap, int dim, dvo_keypoint* dkps, float* ddesc, int32_t* dn, hipStream_t s);
// ---- the batched k-NN path (dvo_knn_stream): many pairs per launch, counts read on the device ----
// Frame slots hold `cap` features each; pair p is frames p (queries) and p + 1 (trains).
// fstate[f] = {features the frame brings to its pairs, marked}: a frame whose detector count
// exceeds cap or whose detector flagged an overflow is marked and brings 0 features.
hipError_t launch_knn_frame_state(const int32_t* d_n /*[F][2] count, flags*/, int frames, int cap,
                                  int32_t* d_fstate /*[F][2]*/, hipStream_t s);
struct KnnBatchArgs {
    const float* desc;        // [F][cap][dim]
    const int32_t* fstate;    // [F][2]
    uint32_t* bytes;          // [F][cap][dim / 4] byte-packed rows (dim 128 only; null: no byte path)
    uint32_t* norms;          // [F][cap] squared norms of the packed rows
    int32_t* rejected;        // [F] 1: the frame holds a value that is not an integer in [0, 255]
    int cap, dim;
    float* dist;              // [P][cap][2] the k = 2 lists
    int32_t* idx;
    float* pdist;             // [P][ranges][cap][2] partial lists (ranges > 1)
    int32_t* pidx;
};
// Train ranges of a batch launch: about two rounds of resident workgroups over all pairs.
int knn_batch_ranges(int cap, int pairs, int cus);
// BFMatcher(NORM_L1).knnMatch(k = 2) of `pairs` pairs: pack (dim 128), byte / float scan, merge.
hipError_t launch_knn_batch(const KnnBatchArgs& a, int frames, int ranges, hipStream_t s);
struct RatioBatchArgs {
    const int32_t* idx;       // [P][cap][2]
    const float* dist;
    const dvo_keypoint* kps;  // [F][cap]
    const int32_t* n;         // [F][2] detector count, flags
    const int32_t* fstate;    // [F][2]
    int cap;
    double ratio;
    float* pts;               // [P][cap][4]
    dvo_dmatch* matches;      // [P][cap]
    int32_t* nmatch;          // [P]
    PairHeader* hdr;          // [P] {detector counts, marked(prev) | marked(cur), 0}
    int32_t* missing;         // [P]
    int squared = 0;          // 1: dist holds FLANN's squared L2 (RatioArgs::squared)
};
hipError_t launch_ratio_gather_batch(const RatioBatchArgs& a, int pairs, hipStream_t s);
// The records of pairs the reference raises on before findEssentialMat (no query, fewer than 2
// trains, a query without a second neighbour): status DVO_ENOFEAT, the counts, zeros elsewhere.
// Pairs of a marked frame keep records_kernel's DVO_ECAP.
hipError_t launch_knn_status(const int32_t* d_n, const int32_t* d_fstate, const int32_t* d_missing, int pairs,
                             dvo_pair_record* records, hipStream_t s);
hipError_t launch_test_retain_best(float* d_resp, uint32_t* d_payload, int32_t* d_tmp, int n, int n_points, int depth,
                                   int semantics, int* d_k, hipStream_t s);
hipError_t launch_test_update_num_iters(double p, const double* d_ep, int n, int model_points, int max_iters,
                                        int32_t* d_out, hipStream_t s);
hipError_t launch_test_ransac_sample(const GeomArgs& g, hipStream_t s);
hipError_t launch_test_ransac_replay(const GeomArgs& g, hipStream_t s);
hipError_t launch_test_ransac_one_round(const GeomArgs& g, int pairs, hipStream_t s);
int64_t test_record_generic_offset(int64_t item);
hipError_t launch_test_five_point(const double* d_q, double* d_models, int* d_n, hipStream_t s);
hipError_t launch_test_sampson(const double* d_E, const double* d_pts, int n, float t, int8_t* d_dec, uint8_t* d_ex,
                               hipStream_t s);

}  // namespace dvo
