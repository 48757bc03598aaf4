// C-ABI of libdvo_hip.so (include/dvo.h): contexts, ORB plans, device buffers
// and the per-call entry points that replace the reference's OpenCV calls.
// Host code only sizes buffers and moves bytes; every computation runs in the
// HIP kernels of orb.hip, match.hip and geometry.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"
#include "dvo_internal.h"
#include "jpeg_entropy.h"
#include "jpeg_split.h"
#include "p3p.h"
#include "pair_outputs.h"

using namespace dvo;

struct SiftPlanDev {  // per-size device buffers of dvo_sift_detect_and_compute
    int w = 0, h = 0;
    SiftArgs a{};
    float* taps = nullptr;
    int tap_off[6] = {0}, tap_n[6] = {0};
    uint8_t* img = nullptr;
    int pitch = 0;
    DeviceAllocs mem;
};

// Scratch of the group SIFT detector (launch_sift_group): `group` copies of what sift_plan
// allocates per frame, kps / desc / the image copy aside (the results go to the caller's slots,
// the frames are read in place), and one taps table.  Allocated whole by sift_group_alloc.
struct SiftGroupDev {
    int w = 0, h = 0, group = 0;
    SiftGroupArgs g{};
    float* taps = nullptr;
    int tap_off[6] = {0}, tap_n[6] = {0};
    DeviceAllocs mem;
};

// Scratch of SIFT's retain stage (SIFT_create(nfeatures > 0)) for `frames` frames of a launch: what
// SiftRetainArgs describes.  Empty until an nfeatures setter or dvo_sift_detect_and_compute_n asks
// for it (sift_retain_ensure).  a.nfeatures stays 0 here: a call fills in its handle's value.
struct SiftRetainDev {
    int frames = 0;
    SiftRetainArgs a{};
    DeviceAllocs mem;
};

struct SurfPlanDev {  // per-size device buffers of dvo_surf_detect_and_compute
    int w = 0, h = 0;
    SurfArgs a{};
    uint8_t* img = nullptr;
    DeviceAllocs mem;
};

// Scratch of the group SURF detector (launch_surf_group): `group` copies of what surf_plan
// allocates per frame, out / desc / the image copy aside (the results go to the caller's slots,
// the frames are read in place), det and trace of a frame adjacent, and one set of the Haar and
// orientation tables.  Allocated whole by surf_group_alloc.
struct SurfGroupDev {
    int w = 0, h = 0, group = 0;
    SurfGroupArgs g{};
    DeviceAllocs mem;
};

struct dvo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    SiftPlanDev sift;
    SiftRetainDev sift_retain;  // one frame's retain scratch, for launch_sift on the plan above (any size)
    SurfPlanDev surf;
    CallSlots call;  // grow-only device and pinned buffers of the per-call entry points (CallMem)
    dvo_stream* call_stream = nullptr;  // cached plan for detectAndCompute
    int call_w = 0, call_h = 0, call_nf = 0;
};

struct dvo_stream {
    dvo_ctx* ctx = nullptr;
    dvo_stream_config cfg{};
    Plan plan{};
    Buffers buf{};  // pts, nmatch, hdr stay null here: params_of fills them from a pair set's view
    DeviceAllocs mem;
    uint8_t* d_frames = nullptr;  // per-call upload slab (max_frames images)
    double* d_carry = nullptr;    // pose tail carry: P_prev (12) | T_abs_prev (16)
    hipEvent_t carry_ev = nullptr;  // recorded after every pose tail on this carry
    bool carry_ev_valid = false;
    dvo_stream* carry_owner = nullptr;  // stream whose carry this one uses (itself by default)
    bool own_hs = false;
    double ratio = 0;  // > 0: match with Hamming 2-NN + this ratio test, not cfg.cross_check (dvo_stream_set_ratio_test)
    int last_nframes = 0;
    int last_pairs = 0;           // pairs of that call (n - 1 for a stream, n / 2 for independent pairs)
    bool last_has_pairs = false;  // the last call ran match + geometry
    const dvo_pair_record* last_rec = nullptr;  // the caller's records of that call (read by the pose tail)
    const uint8_t* last_frames = nullptr;       // the frames of that call (get_pyramid recomputes blurred levels)
    int64_t last_fstride = 0;
    int last_pitch = 0;
    hipStream_t hs = nullptr;
    // dvo_stream_pair: the last pair's current-frame features (the next pair's previous frame) and
    // the device record of one pair, allocated by the first call
    dvo_keypoint* fc_kps = nullptr;
    uint8_t* fc_desc = nullptr;
    int32_t* fc_n = nullptr;  // nkp, status
    dvo_pair_record* pair_rec = nullptr;
    bool fc_valid = false;
    bool last_reuse = false;  // the last call was dvo_stream_pair(reuse_prev): pyramid slot 0 holds frame 1
    // Pair sets (dvo_stream_submit): set k holds one batch's pairs from its submit until it
    // retires kRansacRounds - 1 submits later (or at a drain); every submit / drain step runs one
    // merged RANSAC round in which each occupied set takes its next round.
    struct PairSet {
        bool used = false;
        int round = 0;  // the round this set runs next
        int pairs = 0;
        dvo_pair_record* rec = nullptr;  // the caller's records of the batch
        PairOutputs out;  // the batch's bindings, written when the set retires (with tracks, the set's index copy was taken at the match)
    };
    PairOutputs next;  // dvo_stream_set_landmarks / _tracks / _track_poses / _track_refine / _track_bundle: taken by the next batch
    PairSet sets[kMaxSets];
    // their arrays: 1 set until the first submit, then kRansacRounds; pairs.all.g is the stream's GeomArgs
    PairSets pairs;
    int next_set = 0;  // the set the next submit fills (sets are taken in ring order)
    int last_set = 0;  // the set of the last submitted batch (get_matches)
    int retired = 0;   // batches retired by the last submit / drain / process call
    int last_sub_pairs = 0;  // pairs of the last submitted batch (get_matches)
    dvo_pair_record* retired_rec[kMaxSets] = {};
    int retired_pairs[kMaxSets] = {};
    // profiling: event tables per in-flight call, accumulated on query
    bool profiling = false;
    std::vector<std::vector<hipEvent_t>> ev_pending;
    std::vector<int> ev_groups;  // per pending table: detection frame groups (orb_groups), 0 = none
    std::vector<std::vector<hipEvent_t>> ev_free;
    double stage_ms[DVO_NSTAGES] = {0};
    int prof_calls = 0;

    ~dvo_stream() {  // the members free the device memory
        for (auto* pool : {&ev_pending, &ev_free})
            for (auto& e : *pool)
                for (auto x : e) hipEventDestroy(x);
        if (carry_ev) hipEventDestroy(carry_ev);
        if (own_hs) hipStreamDestroy(hs);
    }
};

namespace {

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            if (ctx) ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);       \
            return DVO_EHIP;                                                             \
        }                                                                                \
    } while (0)

int fail(dvo_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// What a PairOutputs setter answered, as an entry point returns it.
int bind_status(dvo_ctx* ctx, const BindResult& r) {
    if (r.code == DVO_EHIP) return fail(ctx, r.code, std::string(r.what) + ": " + hipGetErrorString(r.hip));
    return r.code == DVO_OK ? DVO_OK : fail(ctx, r.code, r.what);
}

int cv_round_f(float v) { return (int)lrintf(v); }

void set_camera(GeomArgs& g, const double* K) { g.fx = K[0], g.fy = K[4], g.cx = K[2], g.cy = K[5]; }

// orb.cpp computeKeyPoints: features per level (float arithmetic as OpenCV).
void features_per_level(int nfeatures, int nlevels, int* out) {
    const double sf = (double)1.2f;
    float factor = (float)(1.0 / sf);
    float ndesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        out[l] = cv_round_f(ndesired);
        sum += out[l];
        ndesired *= factor;
    }
    out[nlevels - 1] = std::max(nfeatures - sum, 0);
}

// OpenCV 3.2 resize(INTER_LINEAR) on x86: VResizeLinearVec_32s8u (SSE2) covers
// the columns before the point where its 16-wide loop (x <= W - 16) and then
// its 4-wide loop (x < W - 4) stop; VResizeLinear's scalar loop does the rest.
int ocv32_simd_end(int width) {
    int x = 0;
    for (; x <= width - 16; x += 16) {
    }
    for (; x < width - 4; x += 4) {
    }
    return x;
}

Plan make_plan(int w, int h, int nfeatures, int fast_threshold, int semantics) {
    Plan p{};
    p.semantics = semantics;
    p.w = w;
    p.h = h;
    p.nlevels = kMaxLevels;
    p.nfeatures = nfeatures;
    p.fast_threshold = fast_threshold;
    int nper[kMaxLevels];
    features_per_level(nfeatures, kMaxLevels, nper);
    int64_t pyr = 0, blur = 0, bcand = 0, cand = 0;
    int bands = 0, strips = 0, tiles = 0, coef = 0, coef32 = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        LevelGeom& G = p.L[l];
        G.scale = (float)std::pow((double)1.2f, (double)l);  // getScale
        float inv = 1.0f / G.scale;
        G.w = l == 0 ? w : cv_round_f(w * inv);
        G.h = l == 0 ? h : cv_round_f(h * inv);
        G.nper = nper[l];
        G.pitch = (G.w + 15) & ~15;
        G.bpitch = G.pitch;
        G.pyr_off = l == 0 ? 0 : pyr;
        if (l > 0) pyr += (int64_t)G.pitch * G.h;
        G.blur_off = blur;
        blur += (int64_t)G.bpitch * G.h;
        // x table padded to a multiple of 4 entries at a 16-byte aligned offset (one int4 per 4 columns)
        G.xcoef_off = l == 0 ? 0 : coef;
        G.ycoef_off = l == 0 ? 0 : coef + ((G.w + 3) & ~3);
        if (l > 0) coef += ((G.w + 3) & ~3) + ((G.h + 7) & ~7);  // y table padded to 8 rows (resize_level_lds_kernel)
        G.l32_x = l == 0 ? 0 : coef32;
        G.l32_y = l == 0 ? 0 : coef32 + 4 * G.w;
        if (l > 0) coef32 += 4 * (G.w + G.h);
        G.l32_xs = ocv32_simd_end(G.w);
        const bool usable = G.w > 2 * kBorder && G.h > 2 * kBorder;
        const int rows = usable ? G.h - 2 * kBorder : 0;
        const int wc = usable ? G.w - 2 * kBorder : 0;
        G.nbands = (rows + kBandRows - 1) / kBandRows;
        G.ntx = (wc + kFastTW - 1) / kFastTW;
        G.band_base = bands;
        bands += G.nbands * G.ntx;
        G.strip_base = strips;
        strips += G.nbands > 0 ? G.ntx : 0;
        G.band_cap = (kBandRows / 2) * (kFastTW / 2) + 4;  // strict NMS: <= 1 keep per 2x2
        G.band_cand_off = bcand;
        bcand += (int64_t)G.nbands * G.ntx * G.band_cap;
        G.cand_cap = (kBandRows / 2) * G.nbands * ((wc + 1) / 2) + 4;
        G.cand_off = cand;
        cand += G.cand_cap;
        G.tiles_x = (G.w + kBlurTW - 1) / kBlurTW;
        G.tiles_y = (G.h + kBlurTH - 1) / kBlurTH;
        G.tile_base = tiles;
        tiles += G.tiles_x * G.tiles_y;
    }
    p.pyr_stride = (pyr + 255) & ~(int64_t)255;
    p.blur_stride = (blur + 255) & ~(int64_t)255;
    p.total_bands = bands;
    p.total_strips = strips;
    p.band_cand_stride = (bcand + 63) & ~(int64_t)63;
    p.cand_stride = (cand + 63) & ~(int64_t)63;
    p.total_tiles = tiles;
    p.coef_total = coef;
    p.coef32_total = coef32;
    p.kp_cap = ((nfeatures + 256) + 63) & ~63;
    return p;
}

// resize.cpp INTER_LINEAR_EXACT coefficient of destination index `val` (double
// arithmetic as OpenCV's softdouble path; host and device agree bit for bit
// because both are IEEE double without contraction).  Clamped positions store
// the clamped source index with weight c1 = 0, so the kernel never branches on
// the mode: (h0 * 256 + h1 * 0 + 2^15) >> 16 == (h0 + 128) >> 8.
int lin_coef_packed(int val, int srcsize, int dstsize) {
    const double inv_scale = (double)dstsize / srcsize;
    const double scale = 1.0 / inv_scale;
    const double fval = scale * ((double)val + 0.5) - 0.5;
    const int ival = (int)std::floor(fval);
    if (ival >= 0 && srcsize > 1) {
        if (ival < srcsize - 1) {
            const int c1 = (int)std::nearbyint((fval - (double)ival) * 256.0);
            return ival | (c1 << 13);
        }
        return (srcsize - 1) | (2 << 22);
    }
    return 1 << 22;
}

std::vector<int32_t> resize_coefs(const Plan& p) {
    std::vector<int32_t> c(std::max(p.coef_total, 1));
    for (int l = 1; l < p.nlevels; ++l) {
        const LevelGeom &S = p.L[l - 1], &D = p.L[l];
        for (int x = 0; x < ((D.w + 3) & ~3); ++x) c[D.xcoef_off + x] = lin_coef_packed(std::min(x, D.w - 1), S.w, D.w);
        for (int y = 0; y < ((D.h + 7) & ~7); ++y) c[D.ycoef_off + y] = lin_coef_packed(std::min(y, D.h - 1), S.h, D.h);
    }
    return c;
}

// OpenCV 3.2 resize(INTER_LINEAR) tables (imgwarp.cpp resize; oracle/orb.cpp
// resize_linear_32): fx = (float)((d + 0.5) * scale - 0.5) in double rounded to
// float, sx = cvFloor(fx), weights saturate_cast<short>(w * 2048.f) each
// rounded half to even.  Columns: {sx, sx + 1, a0 | a1 << 16, 0}, the
// positions past xmax {W-1, W-1, 2048, 0}; rows: {clip(sy), clip(sy + 1),
// b0 | b1 << 16, 0}.
std::vector<int32_t> resize_coefs_32(const Plan& p) {
    std::vector<int32_t> c(std::max(p.coef32_total, 4));
    auto wgt = [](float v) { return (int32_t)std::max(-32768, std::min(32767, cv_round_f(v))); };
    for (int l = 1; l < p.nlevels; ++l) {
        const LevelGeom &S = p.L[l - 1], &D = p.L[l];
        const double sx_scale = 1. / ((double)D.w / S.w), sy_scale = 1. / ((double)D.h / S.h);
        int xmax = D.w;
        for (int dx = 0; dx < D.w; ++dx) {
            float fx = (float)((dx + 0.5) * sx_scale - 0.5);
            int sx = (int)std::floor(fx);
            fx -= (float)sx;
            if (sx < 0) fx = 0, sx = 0;
            if (sx + 1 >= S.w) {
                xmax = std::min(xmax, dx);
                if (sx >= S.w - 1) fx = 0, sx = S.w - 1;
            }
            int32_t* e = &c[D.l32_x + 4 * dx];
            if (dx < xmax) {
                e[0] = sx;
                e[1] = sx + 1;
                e[2] = (wgt((1.f - fx) * 2048) & 0xFFFF) | (wgt(fx * 2048) << 16);
            } else {
                e[0] = e[1] = sx;
                e[2] = 2048;
            }
            e[3] = 0;
        }
        auto clip = [](int x, int a, int b) { return x >= a ? (x < b ? x : b - 1) : a; };
        for (int dy = 0; dy < D.h; ++dy) {
            float fy = (float)((dy + 0.5) * sy_scale - 0.5);
            const int sy = (int)std::floor(fy);
            fy -= (float)sy;
            int32_t* e = &c[D.l32_y + 4 * dy];
            e[0] = clip(sy, 0, S.h);
            e[1] = clip(sy + 1, 0, S.h);
            e[2] = (wgt((1.f - fy) * 2048) & 0xFFFF) | (wgt(fy * 2048) << 16);
            e[3] = 0;
        }
    }
    return c;
}

int check_orb_params(dvo_ctx* ctx, const dvo_orb_params* o) {
    if (!o) return fail(ctx, DVO_EINVAL, "null ORB parameters");
    if (o->nfeatures <= 0 || o->nfeatures > 7680) return fail(ctx, DVO_EINVAL, "nfeatures out of range (1..7680)");
    if (o->scale_factor != 1.2f || o->nlevels != 8 || o->edge_threshold != 31 || o->first_level != 0 || o->wta_k != 2 ||
        o->score_type != 0 || o->patch_size != 31)
        return fail(ctx, DVO_EINVAL,
                    "only cv.ORB_create() defaults (scaleFactor 1.2, nlevels 8, edgeThreshold 31, firstLevel 0, "
                    "WTA_K 2, HARRIS_SCORE, patchSize 31) are implemented");
    if (o->fast_threshold < 0 || o->fast_threshold > 255) return fail(ctx, DVO_EINVAL, "fastThreshold out of range");
    if (o->opencv_semantics != DVO_OPENCV_4X && o->opencv_semantics != DVO_OPENCV_32)
        return fail(ctx, DVO_EINVAL, "opencv_semantics must be DVO_OPENCV_4X or DVO_OPENCV_32");
    return DVO_OK;
}

template <class T>
int dalloc(dvo_stream* s, T** p, size_t n) {
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(s->mem.alloc(p, n * sizeof(T) + 256));
    return DVO_OK;
}

// The parameter block of a batch whose match stage writes pair set `set`.
StreamParams params_of(dvo_stream* s, const uint8_t* frames, int nframes, int64_t frame_stride, int pitch, int set = 0) {
    StreamParams P{};
    P.plan = s->plan;
    P.buf = s->buf;
    const PairArrays v = s->pairs.view(set);
    P.buf.pts = v.pts;
    P.buf.nmatch = v.nmatch;
    P.buf.hdr = v.hdr;
    P.frames = frames;
    P.frame_stride = frame_stride;
    P.in_pitch = pitch;
    P.nframes = nframes;
    P.pair_step = 1;
    return P;
}

// Row pitch of the internal frame slab (word-aligned rows for the byte kernels).
int frame_pitch(const dvo_stream* s) { return (s->cfg.width + 15) & ~15; }

size_t hyp_cap(const dvo_stream* s) { return (size_t)(s->cfg.max_iters > 1 ? s->cfg.max_iters : 1); }

// At least `want` pair sets (PairSets::ensure).  After a failure the stream has none, and the
// next call that needs one allocates it.
int ensure_sets(dvo_stream* s, int want) {
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(s->pairs.ensure(want));
    return DVO_OK;
}

// A stream's geometry, for both frame streams (cfg: its configuration): the shape of its pair sets
// (F pairs per set of cap points and hc hypotheses; track_sets, own_idx: PairSets::shape), the
// configuration of its GeomArgs (sets.all.g), the first pair set, and into `mem` the round-local
// arrays: the five-point records and parked Durand-Kerner lists of one merged round (a bound over
// any number of sets: one set at each round).
template <class Config>
hipError_t stream_geometry(PairSets& sets, DeviceAllocs& mem, const Config& cfg, int F, int cap, size_t hc, int track_sets,
                           bool own_idx, hipStream_t hs) {
    sets.shape(F, cap, hc, track_sets, own_idx);
    sets.stream = hs;
    GeomArgs& g = sets.all.g;
    g.pts_stride = cap;
    set_camera(g, cfg.K);
    g.prob = cfg.prob;
    g.threshold = cfg.threshold;
    g.max_iters = cfg.max_iters;
    g.dist_thresh = cfg.dist_thresh;
    g.hyp_cap = (int)hc;
    g.dk_list_cap = std::max<int64_t>(round_items_bound(F, (int)hc), (int64_t)hc);
    const size_t blocks = (size_t)std::max<int64_t>(round_blocks_bound(F, (int)hc), (int64_t)(hc + 63) / 64);
    hipError_t e = sets.ensure(1);
    if (e == hipSuccess) e = mem.alloc(&g.fprec, blocks * 128 * 64 * sizeof(double) + 256);
    if (e == hipSuccess) e = mem.alloc(&g.dk_ctl, (size_t)(2 + kDkMaxPasses) * sizeof(int32_t) + 256);
    if (e == hipSuccess) e = mem.alloc(&g.dk_list, (size_t)(kDkMaxPasses - 1) * g.dk_list_cap * sizeof(int32_t) + 256);
    return e;
}

// The geometry arrays of a per-call entry point, from its CallMem, for `pairs` pairs of `pts`
// points and hc hypotheses each, a group on request.  kGeomRansac: what the normalize and RANSAC
// stages use and leave (E, info), with hyp_cap and dk_list_cap; fprec has `blocks` five-point
// blocks, by default what one round over every hypothesis of every pair needs, each pair's
// hypotheses rounded up to whole blocks.  kGeomPose: what recoverPose leaves.
constexpr int kGeomRansac = 1, kGeomPose = 2;
void call_geometry(GeomArgs& g, CallMem& mem, int groups, size_t pairs, size_t pts, size_t hc, size_t blocks = 0) {
    const size_t PH = pairs * hc;
    if (groups & kGeomRansac) {
        g.npts = mem.dev<double>(pairs * pts * 4);
        g.models = mem.dev<double>(PH * 90);
        g.nmod = mem.dev<int32_t>(PH);
        g.cnt = mem.dev<int32_t>(PH * 10);
        g.subsets = mem.dev<int32_t>(PH * 5);
        g.rs = mem.dev<RansacState>(pairs);
        g.fprec = mem.dev<double>((blocks ? blocks : (PH + 63) / 64 + pairs - 1) * 128 * 64);
        g.dk_off = mem.dev<int32_t>(pairs + 1);
        g.a_off = mem.dev<int32_t>(pairs + 1);
        g.s_off = mem.dev<int32_t>(pairs + 1);
        g.dk_ctl = mem.dev<int32_t>(2 + kDkMaxPasses);
        g.dk_list_cap = (int64_t)PH;
        g.dk_list = mem.dev<int32_t>((size_t)(kDkMaxPasses - 1) * PH);
        g.hyp_cap = (int)hc;
        g.E = mem.dev<double>(pairs * 90);
        g.info = mem.dev<int32_t>(pairs * 4);
    }
    if (groups & kGeomPose) {
        g.Rt = mem.dev<double>(pairs * 12);
        g.good = mem.dev<int32_t>(pairs);
        g.pose_P = mem.dev<double>(pairs * 72);
        g.pose_cnt = mem.dev<int32_t>(pairs * 5);
    }
}

int stream_alloc(dvo_stream* s) {
    const int F = s->cfg.max_frames;
    const Plan& p = s->plan;
    Buffers& b = s->buf;
    const int cap = p.kp_cap;
    int rc;
#define A(ptr, n)                              \
    if ((rc = dalloc(s, &(ptr), (size_t)(n)))) \
        return rc;
    A(b.pyr, (size_t)F * p.pyr_stride);
    A(b.blur, (size_t)F * p.blur_stride);
    A(b.coef, (size_t)std::max(p.coef_total, 1));
    A(b.coef32, (size_t)std::max(p.coef32_total, 4));
    A(b.band_cnt, (size_t)F * (p.total_bands + 1) * kBandRows);
    A(b.band_cand, (size_t)F * p.band_cand_stride);
    A(b.cand, (size_t)F * p.cand_stride);
    A(b.resp, (size_t)F * p.cand_stride);
    A(b.sel_tmp, (size_t)F * 2 * p.cand_stride);
    A(b.cnt1, (size_t)F * kMaxLevels);
    A(b.cnt2, (size_t)F * kMaxLevels);
    A(b.kps, (size_t)F * cap);
    A(b.desc, (size_t)F * cap * 32);
    A(b.nkp, (size_t)F);
    A(b.nn, (size_t)2 * F * cap);
    A(b.mq, (size_t)F * cap);
    A(b.mt, (size_t)F * cap);
    A(b.md, (size_t)F * cap);
    // the stream's GeomArgs and its round-local arrays, once; the track scratch covers every set a
    // pipelined stream will hold, each with its own copy of the match indices
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(stream_geometry(s->pairs, s->mem, s->cfg, F, cap, hyp_cap(s), kRansacRounds, true, s->hs));
    A(b.status, (size_t)F);
    A(s->d_frames, (size_t)F * frame_pitch(s) * s->cfg.height);
    A(s->d_carry, (size_t)28);
#undef A
    return DVO_OK;
}

dvo_orb_params default_orb(int nfeatures) {
    dvo_orb_params o{};
    o.nfeatures = nfeatures;
    o.scale_factor = 1.2f;
    o.nlevels = 8;
    o.edge_threshold = 31;
    o.first_level = 0;
    o.wta_k = 2;
    o.score_type = 0;
    o.patch_size = 31;
    o.fast_threshold = 20;
    return o;
}

// A table: 2 events per stage, then 2 x 5 per detection frame group (launch_orb's group_ev).
int acquire_events(dvo_stream* s, int groups, hipEvent_t** ev) {
    dvo_ctx* ctx = s->ctx;
    std::vector<hipEvent_t> e;
    if (!s->ev_free.empty()) {
        e = std::move(s->ev_free.back());
        s->ev_free.pop_back();
    } else {
        e.resize(2 * DVO_NSTAGES + 10 * orb_groups(s->cfg.max_frames));
        for (auto& x : e) HIP_TRY(hipEventCreate(&x));
    }
    s->ev_pending.push_back(std::move(e));
    s->ev_groups.push_back(groups);
    *ev = s->ev_pending.back().data();
    return DVO_OK;
}

// Drain completed event tables into the per-stage totals (blocks on the last).
int collect_events(dvo_stream* s) {
    dvo_ctx* ctx = s->ctx;
    for (size_t i = 0; i < s->ev_pending.size(); ++i) {
        auto& e = s->ev_pending[i];
        const int groups = s->ev_groups[i];
        HIP_TRY(hipEventSynchronize(e[2 * DVO_NSTAGES - 1]));
        for (int st = 0; st < DVO_NSTAGES; ++st) {
            float ms = 0;
            if (st <= 4 && groups > 0) {  // detection in frame groups: the stage's time summed over them
                for (int g = 0; g < groups; ++g)
                    if (hipEventElapsedTime(&ms, e[2 * DVO_NSTAGES + 10 * g + 2 * st],
                                            e[2 * DVO_NSTAGES + 10 * g + 2 * st + 1]) == hipSuccess)
                        s->stage_ms[st] += ms;
            } else if (hipEventElapsedTime(&ms, e[2 * st], e[2 * st + 1]) == hipSuccess) {
                s->stage_ms[st] += ms;
            }
        }
        s->prof_calls++;
        s->ev_free.push_back(std::move(e));
    }
    s->ev_pending.clear();
    s->ev_groups.clear();
    return DVO_OK;
}

// One merged RANSAC round: every occupied set that has rounds left takes its next one.
int merged_round(dvo_stream* s) {
    dvo_ctx* ctx = s->ctx;
    RoundSpec sp{};
    sp.nsets = s->pairs.nsets;
    sp.F = s->cfg.max_frames;
    bool any = false;
    for (int r = 0; r < kRansacRounds; ++r) sp.bound[r] = kRansacBounds[r];  // indexed by round
    for (int k = 0; k < s->pairs.nsets; ++k) {
        auto& st = s->sets[k];
        const bool run = st.used && st.round < kRansacRounds;
        sp.round[k] = run ? st.round : -1;
        sp.npairs[k] = run ? st.pairs : 0;
        any |= run;
    }
    if (!any) return DVO_OK;
    HIP_TRY(launch_ransac_round(s->pairs.all.g, sp, s->hs));
    for (auto& st : s->sets)
        if (st.used && st.round < kRansacRounds) ++st.round;
    return DVO_OK;
}

// Retire the sets whose last round has run, oldest first: E, recoverPose, the records.
int retire_sets(dvo_stream* s) {
    dvo_ctx* ctx = s->ctx;
    // ring order from the oldest set (the one after the newest)
    for (int j = 1; j <= kRansacRounds; ++j) {
        const int k = (s->last_set + j) % kRansacRounds;
        auto& st = s->sets[k];
        if (!st.used || st.round < kRansacRounds) continue;
        const PairArrays v = s->pairs.view(k);
        HIP_TRY(launch_retire(v.g, st.pairs, v.hdr, st.rec, s->hs));
        if (s->ratio > 0) HIP_TRY(launch_hamming_ratio_status(v.hdr, st.pairs, st.rec, nullptr, s->hs));
        HIP_TRY(launch_pair_outputs(st.out, s->pairs, k, v.g, st.pairs, st.rec, nullptr, s->hs));  // with the set's own indices
        s->retired_rec[s->retired] = st.rec;
        s->retired_pairs[s->retired] = st.pairs;
        ++s->retired;
        s->last_rec = st.rec;
        s->last_pairs = st.pairs;
        s->last_has_pairs = true;
        st = dvo_stream::PairSet{};
    }
    return DVO_OK;
}

bool sets_pending(const dvo_stream* s) {
    for (const auto& st : s->sets)
        if (st.used) return true;
    return false;
}

// Detection of n frames, then (unless detect_only) matching of their pairs into the next pair
// set and one merged RANSAC round; drain: rounds until every set is done, then retire them all
// (dvo_stream_process: this batch's records are complete when the call's work is).
int run_stream(dvo_stream* s, const uint8_t* d_frames, int n, int64_t fstride, int pitch, dvo_pair_record* d_rec,
               bool detect_only, int pair_step = 1, bool drain = true) {
    dvo_ctx* ctx = s->ctx;
    // the bindings are for this batch alone, whether or not the call gets as far as its pairs
    const PairOutputs out = detect_only ? PairOutputs{} : s->next.take();
    if (out.tr && pair_step != 1)  // every binding is consumed
        return fail(ctx, DVO_EINVAL, "tracks need consecutive pairs: the pairs of a *_pairs call share no frame");
    const int want = drain ? 1 : kRansacRounds;
    if (!detect_only && s->pairs.nsets < want) {
        // the first pipelined submit grows the sets; a drained call after a failed grow allocates one
        // (before params_of: the parameter block carries the buffer pointers)
        if (sets_pending(s)) return fail(ctx, DVO_EINVAL, "pair sets occupied at the first submit");
        s->next_set = s->last_set = s->last_sub_pairs = 0;  // the last batch's matches go with the old sets
        int rc = ensure_sets(s, want);
        if (rc) return rc;
    }
    const int k = s->next_set;
    StreamParams P = params_of(s, d_frames, n, fstride, pitch, k);
    P.pair_step = pair_step;
    const int pairs = detect_only ? 0 : stream_pairs(P);
    hipEvent_t* ev = nullptr;
    const int groups = orb_groups(n);
    if (s->profiling && pairs >= 1) {
        int rc = acquire_events(s, groups, &ev);
        if (rc) return rc;
    }
    s->retired = 0;
    s->last_has_pairs = false;  // set again when a batch retires: the pose tail reads its records
    if (pairs >= 1 && s->sets[k].used) {  // the ring is full (cannot happen in lockstep): finish its oldest
        int rc;
        while (s->sets[k].used && s->sets[k].round < kRansacRounds)
            if ((rc = merged_round(s))) return rc;
        if ((rc = retire_sets(s))) return rc;
    }
    HIP_TRY(hipMemsetAsync(s->buf.status, 0, sizeof(int32_t) * n, s->hs));
    HIP_TRY(launch_orb(P, s->hs, ev, ev && groups ? ev + 2 * DVO_NSTAGES : nullptr));
    s->last_nframes = n;
    s->last_reuse = false;
    s->last_frames = d_frames;
    s->last_fstride = fstride;
    s->last_pitch = pitch;
    s->last_sub_pairs = pairs;
    if (detect_only) return DVO_OK;
    if (pairs >= 1) {
        // match into set k (its KeyPoint_convert points and counts), the frame-side record values
        if (s->ratio > 0)
            HIP_TRY(launch_match_ratio(P, s->ratio, s->hs, ev));
        else
            HIP_TRY(launch_match(P, s->cfg.cross_check, s->hs, ev));
        HIP_TRY(launch_pair_header(P, P.buf.hdr, s->hs));
        if (out.lm.out && out.tr) {
            // the match indices are the stream's, not the set's: a later batch overwrites them
            // before this one retires, so a batch with tracks keeps its own copy
            const size_t off = (size_t)k * s->pairs.set_slots(), nb = (size_t)pairs * s->plan.kp_cap * 4;
            HIP_TRY(hipMemcpyAsync(s->pairs.tr.iq + off, s->buf.mq, nb, hipMemcpyDeviceToDevice, s->hs));
            HIP_TRY(hipMemcpyAsync(s->pairs.tr.it + off, s->buf.mt, nb, hipMemcpyDeviceToDevice, s->hs));
        }
        HIP_TRY(launch_geometry_args(s->pairs.view(k).g, pairs, kStageNormalize, s->hs));
        s->sets[k] = dvo_stream::PairSet{true, 0, pairs, d_rec, out};
        s->last_set = k;
        // nsets >= 1 here: every path that matches has passed ensure_sets above
        s->next_set = (k + 1) % s->pairs.nsets;
    }
    if (pairs < 1 && !drain) return DVO_OK;
    int rc;
    mark(ev, 6, 0, s->hs);
    if ((rc = merged_round(s))) return rc;
    if (drain)
        while (sets_pending(s)) {
            bool left = false;
            for (const auto& st : s->sets) left |= st.used && st.round < kRansacRounds;
            if (!left) break;
            if ((rc = merged_round(s))) return rc;
        }
    mark(ev, 6, 1, s->hs);
    mark(ev, 7, 0, s->hs);
    if ((rc = retire_sets(s))) return rc;
    mark(ev, 7, 1, s->hs);
    mark(ev, 8, 0, s->hs);  // pose-tail pair defaults to 0 ms; dvo_stream_pose_tail re-records it
    mark(ev, 8, 1, s->hs);
    return DVO_OK;
}

}  // namespace

extern "C" {

int dvo_version(void) { return 1; }

#ifndef DVO_BUILD_ID
#define DVO_BUILD_ID "unstamped0000000"
#endif
// "DVO_BUILD_ID=" + 16 hex digits: build.py finds it in the file without loading it
static const char kBuildTag[] = "DVO_BUILD_ID=" DVO_BUILD_ID;
const char* dvo_build_id(void) { return kBuildTag + 13; }

int dvo_ctx_create(dvo_ctx** out, int device) {
    if (!out) return DVO_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DVO_EHIP;
    if (device < 0 || device >= n) return DVO_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return DVO_EHIP;
    dvo_ctx* ctx = new dvo_ctx();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return DVO_EHIP;
    }
    *out = ctx;
    return DVO_OK;
}

void dvo_ctx_destroy(dvo_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->call_stream) dvo_stream_destroy(ctx->call_stream);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* dvo_last_error(const dvo_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dvo_stream_create(dvo_ctx* ctx, const dvo_stream_config* cfg, dvo_stream** out) {
    if (!ctx || !cfg || !out) return fail(ctx, DVO_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_orb_params(ctx, &cfg->orb);
    if (rc) return rc;
    if (cfg->width < 8 || cfg->height < 8 || cfg->width >= kMaxW || cfg->height >= kMaxW)
        return fail(ctx, DVO_EINVAL, "frame size out of range (8..4095)");
    if (cfg->max_frames < 1) return fail(ctx, DVO_EINVAL, "max_frames < 1");
    if (cfg->cross_check < 0 || cfg->cross_check > 2) return fail(ctx, DVO_EINVAL, "cross_check must be 0, 1 or 2");
    if (!(cfg->prob > 0 && cfg->prob < 1)) return fail(ctx, DVO_EINVAL, "prob must be in (0, 1)");
    if (!(cfg->threshold > 0) || !std::isfinite(cfg->threshold))
        return fail(ctx, DVO_EINVAL, "threshold must be finite and > 0");
    if (cfg->max_iters < 1) return fail(ctx, DVO_EINVAL, "max_iters must be >= 1");
    if (!std::isfinite(cfg->dist_thresh)) return fail(ctx, DVO_EINVAL, "dist_thresh must be finite");
    HIP_TRY(hipSetDevice(ctx->device));
    auto s = std::make_unique<dvo_stream>();
    s->ctx = ctx;
    s->cfg = *cfg;
    s->plan = make_plan(cfg->width, cfg->height, cfg->orb.nfeatures, cfg->orb.fast_threshold, cfg->orb.opencv_semantics);
    if (s->plan.kp_cap > 65535) return fail(ctx, DVO_EINVAL, "too many features");
    if (hipStreamCreateWithFlags(&s->hs, hipStreamNonBlocking) != hipSuccess)
        return fail(ctx, DVO_EHIP, "hipStreamCreate failed");
    s->own_hs = true;
    s->carry_owner = s.get();
    if (hipEventCreateWithFlags(&s->carry_ev, hipEventDisableTiming) != hipSuccess)
        return fail(ctx, DVO_EHIP, "hipEventCreate failed");
    rc = stream_alloc(s.get());
    if (!rc) {
        const std::vector<int32_t> coefs = resize_coefs(s->plan), coefs32 = resize_coefs_32(s->plan);
        if (hipMemcpy(s->buf.coef, coefs.data(), coefs.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(s->buf.coef32, coefs32.data(), coefs32.size() * sizeof(int32_t), hipMemcpyHostToDevice) !=
                hipSuccess)
            rc = fail(ctx, DVO_EHIP, "coefficient upload failed");
    }
    if (rc) return rc;
    *out = s.release();
    return DVO_OK;
}

void dvo_stream_destroy(dvo_stream* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->hs);
    delete s;
}

int dvo_stream_reset_pose(dvo_stream* s, const double* P0, const double* T0) {
    if (!s || !P0 || !T0) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    dvo_stream* o = s->carry_owner;
    double c[28];
    std::memcpy(c, P0, 12 * sizeof(double));
    std::memcpy(c + 12, T0, 16 * sizeof(double));
    if (o->carry_ev_valid) HIP_TRY(hipStreamWaitEvent(s->hs, o->carry_ev, 0));
    HIP_TRY(hipMemcpyAsync(o->d_carry, c, sizeof(c), hipMemcpyHostToDevice, s->hs));
    HIP_TRY(hipEventRecord(o->carry_ev, s->hs));
    o->carry_ev_valid = true;
    HIP_TRY(hipStreamSynchronize(s->hs));
    return DVO_OK;
}

int dvo_stream_share_pose(dvo_stream* s, dvo_stream* owner) {
    if (!s || !owner || owner->carry_owner != owner) return DVO_EINVAL;
    s->carry_owner = owner;
    return DVO_OK;
}

int dvo_stream_pose_tail(dvo_stream* s, const double* d_corners_prev, const double* d_corners_cur, int k,
                         double marker_length, double* d_T_rel, double* d_T_abs) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (!s->last_has_pairs) return fail(ctx, DVO_EINVAL, "pose tail needs a preceding dvo_stream_process");
    return dvo_stream_pose_tail_batch(s, s->last_rec, s->last_pairs, d_corners_prev, d_corners_cur, k, marker_length,
                                      d_T_rel, d_T_abs);
}

int dvo_stream_pose_tail_batch(dvo_stream* s, const dvo_pair_record* d_records, int pairs, const double* d_corners_prev,
                               const double* d_corners_cur, int k, double marker_length, double* d_T_rel,
                               double* d_T_abs) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (k < 2 || !d_corners_prev || !d_corners_cur || !d_T_rel || !d_T_abs)
        return fail(ctx, DVO_EINVAL, "pose tail needs >= 2 corners per frame and output buffers");
    if (!d_records || pairs < 1) return fail(ctx, DVO_EINVAL, "pose tail needs records");
    HIP_TRY(hipSetDevice(ctx->device));
    hipEvent_t* ev = (s->profiling && !s->ev_pending.empty()) ? s->ev_pending.back().data() : nullptr;
    dvo_stream* o = s->carry_owner;  // pose tails on one carry run in call order, across streams
    if (o->carry_ev_valid) HIP_TRY(hipStreamWaitEvent(s->hs, o->carry_ev, 0));
    mark(ev, 8, 0, s->hs);
    HIP_TRY(launch_pose_tail(d_records, pairs, s->cfg.K, d_corners_prev, d_corners_cur, k, marker_length,
                             o->d_carry, d_T_rel, d_T_abs, s->hs));
    mark(ev, 8, 1, s->hs);
    HIP_TRY(hipEventRecord(o->carry_ev, s->hs));
    o->carry_ev_valid = true;
    return DVO_OK;
}

int dvo_pose_tail_records(dvo_ctx* ctx, const dvo_pair_record* d_records, int pairs, const double* K,
                          const double* d_corners_prev, const double* d_corners_cur, int k, double marker_length,
                          double* d_carry, double* d_T_rel, double* d_T_abs, void* hip_stream) {
    if (!ctx) return DVO_EINVAL;
    if (pairs < 0 || !K) return fail(ctx, DVO_EINVAL, "pose tail needs pairs >= 0 and K");
    if (pairs == 0) return DVO_OK;
    if (k < 2 || !d_records || !d_corners_prev || !d_corners_cur || !d_carry || !d_T_rel || !d_T_abs)
        return fail(ctx, DVO_EINVAL, "pose tail needs records, >= 2 corners per frame, the carry and output buffers");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_pose_tail(d_records, pairs, K, d_corners_prev, d_corners_cur, k, marker_length, d_carry, d_T_rel,
                             d_T_abs, hip_stream ? (hipStream_t)hip_stream : ctx->stream));
    return DVO_OK;
}

int dvo_pose_rel_range(dvo_ctx* ctx, const dvo_pair_record* d_records, int pairs, int p0, int n, const double* K,
                       const double* d_corners_prev, const double* d_corners_cur, int k, double marker_length,
                       double* d_P_carry, double* d_T_rel, void* hip_stream) {
    if (!ctx) return DVO_EINVAL;
    if (pairs < 0 || p0 < 0 || n < 0 || p0 + n > pairs || !K)
        return fail(ctx, DVO_EINVAL, "pose range needs 0 <= p0 <= p0 + n <= pairs and K");
    if (pairs == 0) return DVO_OK;
    if (!d_records || !d_P_carry || (n > 0 && (k < 2 || !d_corners_prev || !d_corners_cur || !d_T_rel)))
        return fail(ctx, DVO_EINVAL, "pose range needs records, the P carry, >= 2 corners per frame and T_rel");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_pose_rel_range(d_records, pairs, p0, n, K, d_corners_prev, d_corners_cur, k, marker_length,
                                  d_P_carry, d_T_rel, hip_stream ? (hipStream_t)hip_stream : ctx->stream));
    return DVO_OK;
}

// The chain on the host, in the device kernel's arithmetic order (pose_chain_kernel: element
// (r, c) = ((t_r0 A_0c + t_r1 A_1c) + t_r2 A_2c) + t_r3 A_3c; this file is built with
// -ffp-contract=off, so each product and sum rounds as written).
int dvo_pose_chain_host(const double* T_rel, int n, double* T_carry, double* T_abs) {
    if (n < 0 || (n > 0 && (!T_rel || !T_carry || !T_abs))) return DVO_EINVAL;
    if (n == 0) return DVO_OK;  // nothing to chain; T_carry may be NULL (as dvo_pose_chain)
    double t[16];
    std::memcpy(t, T_carry, sizeof(t));
    for (int p = 0; p < n; ++p) {
        const double* A = T_rel + (size_t)p * 16;
        double u[16];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                const double m0 = t[r * 4 + 0] * A[0 * 4 + c], m1 = t[r * 4 + 1] * A[1 * 4 + c];
                const double m2 = t[r * 4 + 2] * A[2 * 4 + c], m3 = t[r * 4 + 3] * A[3 * 4 + c];
                u[r * 4 + c] = ((m0 + m1) + m2) + m3;
            }
        std::memcpy(t, u, sizeof(t));
        std::memcpy(T_abs + (size_t)p * 16, t, sizeof(t));
    }
    std::memcpy(T_carry, t, sizeof(t));
    return DVO_OK;
}

int dvo_pose_chain(dvo_ctx* ctx, const double* d_T_rel, int n, double* d_T_carry, double* d_T_abs, void* hip_stream) {
    if (!ctx) return DVO_EINVAL;
    if (n < 0 || (n > 0 && (!d_T_rel || !d_T_carry || !d_T_abs)))
        return fail(ctx, DVO_EINVAL, "pose chain needs T_rel, the carry and an output buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_pose_chain(d_T_rel, n, d_T_carry, d_T_abs,
                              hip_stream ? (hipStream_t)hip_stream : ctx->stream));
    return DVO_OK;
}

int dvo_stream_set_profiling(dvo_stream* s, int enable) {
    if (!s) return DVO_EINVAL;
    int rc = collect_events(s);
    if (rc) return rc;
    s->profiling = enable != 0;
    for (double& v : s->stage_ms) v = 0;
    s->prof_calls = 0;
    return DVO_OK;
}

int dvo_stream_stage_times(dvo_stream* s, double* ms, int* calls) {
    if (!s || !ms) return DVO_EINVAL;
    int rc = collect_events(s);
    if (rc) return rc;
    for (int i = 0; i < DVO_NSTAGES; ++i) ms[i] = s->stage_ms[i];
    if (calls) *calls = s->prof_calls;
    return DVO_OK;
}

void* dvo_stream_hip_stream(dvo_stream* s) { return s ? (void*)s->hs : nullptr; }

static int process_frames(dvo_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                   dvo_pair_record* d_records, int pair_step, bool drain = true) {
    dvo_ctx* ctx = s->ctx;
    if (!d_frames || stride < s->cfg.width) return fail(ctx, DVO_EINVAL, "bad frame buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    if (((uintptr_t)d_frames | (uintptr_t)frame_stride | (uintptr_t)stride) & 3) {
        // the byte kernels read level 0 in 4-byte words: realign into the slab
        const int pw = frame_pitch(s);
        for (int i = 0; i < n_frames; ++i)
            HIP_TRY(hipMemcpy2DAsync(s->d_frames + (size_t)i * pw * s->cfg.height, pw, d_frames + i * frame_stride,
                                     stride, s->cfg.width, s->cfg.height, hipMemcpyDeviceToDevice, s->hs));
        return run_stream(s, s->d_frames, n_frames, (int64_t)pw * s->cfg.height, pw, d_records, false, pair_step,
                          drain);
    }
    return run_stream(s, d_frames, n_frames, frame_stride, stride, d_records, false, pair_step, drain);
}

int dvo_stream_process(dvo_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                       dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (n_frames < 1 || n_frames > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range");
    if (n_frames > 1 && !d_records) return fail(ctx, DVO_EINVAL, "null records");
    return process_frames(s, d_frames, n_frames, frame_stride, stride, d_records, 1);
}

int dvo_pipeline_depth(void) { return kRansacRounds; }

int dvo_stream_submit(dvo_stream* s, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                      dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (n_frames < 2 || n_frames > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range (2..max)");
    if (!d_records) return fail(ctx, DVO_EINVAL, "null records");
    return process_frames(s, d_frames, n_frames, frame_stride, stride, d_records, 1, false);
}

int dvo_stream_submit_pairs(dvo_stream* s, const uint8_t* d_frames, int n_pairs, int64_t frame_stride, int stride,
                            dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (n_pairs < 1 || 2 * (int64_t)n_pairs > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_pairs out of range");
    if (!d_records) return fail(ctx, DVO_EINVAL, "null records");
    return process_frames(s, d_frames, 2 * n_pairs, frame_stride, stride, d_records, 2, false);
}

int dvo_stream_drain(dvo_stream* s) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    s->retired = 0;
    s->last_has_pairs = false;
    int rc;
    for (;;) {
        bool left = false;
        for (const auto& st : s->sets) left |= st.used && st.round < kRansacRounds;
        if (!left) break;
        if ((rc = merged_round(s))) return rc;
    }
    return retire_sets(s);
}

int dvo_stream_retired(dvo_stream* s, void** records, int* pairs, int cap) {
    if (!s || (cap > 0 && (!records || !pairs))) return DVO_EINVAL;
    for (int i = 0; i < s->retired && i < cap; ++i) {
        records[i] = s->retired_rec[i];
        pairs[i] = s->retired_pairs[i];
    }
    return s->retired;
}

int dvo_stream_process_pairs(dvo_stream* s, const uint8_t* d_frames, int n_pairs, int64_t frame_stride, int stride,
                             dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (n_pairs < 1 || 2 * (int64_t)n_pairs > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_pairs out of range");
    if (!d_records) return fail(ctx, DVO_EINVAL, "null records");
    return process_frames(s, d_frames, 2 * n_pairs, frame_stride, stride, d_records, 2);
}

// One pair of host frames through the whole per-pair path in one synchronous call
// (dvo.h dvo_stream_pair).  Slot 0 of the stream's frame slab / feature buffers is the
// previous frame, slot 1 the current one.  With reuse_prev the current frame is detected
// alone (as frame 0, the ORB kernels' per-call launch shapes), its features are moved
// to slot 1 and the cached ones of the last call's current frame to slot 0; then the
// matcher (train stages split over workgroups: one pair alone fills the chip), the
// per-call RANSAC schedule (one round, 16-lane Durand-Kerner), recoverPose and the
// record, and one device-to-host copy of the record.
int dvo_stream_pair(dvo_stream* s, const uint8_t* prev_img, const uint8_t* cur_img, int stride, int reuse_prev,
                    dvo_pair_record* rec_out) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    const int w = s->cfg.width, h = s->cfg.height;
    if (s->cfg.max_frames < 2) return fail(ctx, DVO_EINVAL, "dvo_stream_pair needs max_frames >= 2");
    if (!cur_img || !rec_out || stride < w || (!reuse_prev && !prev_img)) return fail(ctx, DVO_EINVAL, "bad image buffer");
    if (reuse_prev && !s->fc_valid) return fail(ctx, DVO_EINVAL, "reuse_prev needs a preceding dvo_stream_pair");
    if (sets_pending(s)) return fail(ctx, DVO_EINVAL, "dvo_stream_pair: submitted batches are pending (dvo_stream_drain)");
    // the feature cache is valid only after a call that succeeds (a failing call may have left
    // its frame half-way through the rotation)
    s->fc_valid = false;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t kc = (size_t)s->plan.kp_cap;
    if (!s->pair_rec) {  // each buffer once: a partial failure leaves the rest to the next call
        int rc;
        if ((!s->fc_kps && (rc = dalloc(s, &s->fc_kps, kc))) || (!s->fc_desc && (rc = dalloc(s, &s->fc_desc, kc * 32))) ||
            (!s->fc_n && (rc = dalloc(s, &s->fc_n, 2))) || (rc = dalloc(s, &s->pair_rec, 1)))
            return rc;
    }
    int rc = ensure_sets(s, 1);  // set 0 takes the pair
    if (rc) return rc;
    CallMem mem(ctx->call, s->hs);
    const size_t img_bytes = (size_t)w * h;
    const int pw = frame_pitch(s);
    // host frames go through pinned buffers: one host copy, one asynchronous DMA each
    auto upload = [&](uint8_t* dst, const uint8_t* img) -> hipError_t {
        uint8_t* hp = mem.host(img_bytes);
        if (!hp) return mem.error();
        if (stride == w) {
            std::memcpy(hp, img, img_bytes);
        } else {
            for (int y = 0; y < h; ++y) std::memcpy(hp + (size_t)y * w, img + (size_t)y * stride, w);
        }
        return hipMemcpy2DAsync(dst, pw, hp, w, w, h, hipMemcpyHostToDevice, s->hs);
    };
    const int64_t fst = (int64_t)pw * h;
    const Buffers& b = s->buf;
    // after the first upload, an error drains the stream before returning: its DMAs read the
    // context's pinned buffers, which the next per-call entry point rewrites (or frees to grow them)
    auto body = [&]() -> int {
    // the feature arrays of frame 0, frame 1 and the cache (the last current frame's), in 4-byte words
    FeatSlots fsl{};
    auto slot = [&](int k, void* kps, void* desc, int32_t* n, int32_t* stt) {
        fsl.a[k][0] = (uint32_t*)kps;
        fsl.a[k][1] = (uint32_t*)desc;
        fsl.a[k][2] = (uint32_t*)n;
        fsl.a[k][3] = (uint32_t*)stt;
    };
    slot(0, b.kps, b.desc, b.nkp, b.status);
    slot(1, b.kps + kc, b.desc + kc * 32, b.nkp + 1, b.status + 1);
    slot(2, s->fc_kps, s->fc_desc, s->fc_n, s->fc_n + 1);
    fsl.words[0] = (int)(kc * sizeof(dvo_keypoint) / 4);
    fsl.words[1] = (int)(kc * 32 / 4);
    fsl.words[2] = fsl.words[3] = 1;
    if (reuse_prev) {
        HIP_TRY(upload(s->d_frames, cur_img));
        if ((rc = run_stream(s, s->d_frames, 1, fst, pw, nullptr, true))) return rc;
        // frame 1 <- the new frame's features (frame 0), frame 0 <- the cached previous frame's, and the
        // cache <- the new frame's (the next pair's previous frame): one launch, element by element
        HIP_TRY(launch_feature_rotate(fsl, 1, s->hs));
    } else {
        HIP_TRY(upload(s->d_frames, prev_img));
        HIP_TRY(upload(s->d_frames + fst, cur_img));
        if ((rc = run_stream(s, s->d_frames, 2, fst, pw, nullptr, true))) return rc;
        HIP_TRY(launch_feature_rotate(fsl, 0, s->hs));  // the current frame's features are the next previous
    }
    StreamParams P = params_of(s, s->d_frames, 2, fst, pw);
    const int nqb = ((int)kc + 255) / 256, nst = ((int)kc + 63) / 64;
    int tsplit = 1;
    while (tsplit < 16 && nqb * tsplit * 2 <= 256 && nst >= tsplit * 8) tsplit *= 2;
    if (s->ratio > 0)
        HIP_TRY(launch_match_ratio(P, s->ratio, s->hs));
    else
        HIP_TRY(launch_match(P, s->cfg.cross_check, s->hs, nullptr, tsplit));
    HIP_TRY(launch_geometry(P, s->pairs.all.g, s->pair_rec, s->hs, nullptr, true));
    if (s->ratio > 0) HIP_TRY(launch_hamming_ratio_status(P.buf.hdr, 1, s->pair_rec, nullptr, s->hs));
    uint8_t* hr = nullptr;
    HIP_TRY(mem.get(s->pair_rec, sizeof(dvo_pair_record), &hr));
    HIP_TRY(hipStreamSynchronize(s->hs));
    std::memcpy(rec_out, hr, sizeof(dvo_pair_record));
    return DVO_OK;
    };
    if ((rc = body())) {
        (void)hipStreamSynchronize(s->hs);
        return rc;
    }
    s->fc_valid = true;
    s->last_reuse = reuse_prev != 0;
    s->last_nframes = 2;
    s->last_pairs = 1;
    s->last_sub_pairs = 1;
    s->last_set = 0;
    s->last_has_pairs = true;
    s->last_rec = s->pair_rec;
    s->last_frames = s->d_frames;
    s->last_fstride = fst;
    s->last_pitch = pw;
    return DVO_OK;
}

int dvo_stream_set_ratio_test(dvo_stream* s, double ratio) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (!std::isfinite(ratio) || ratio < 0) return fail(ctx, DVO_EINVAL, "ratio must be finite and >= 0 (0: off)");
    if (sets_pending(s))
        return fail(ctx, DVO_EINVAL, "dvo_stream_set_ratio_test: submitted batches are pending (dvo_stream_drain)");
    s->ratio = ratio;
    return DVO_OK;
}

int dvo_stream_set_landmarks(dvo_stream* s, dvo_landmark* d_out, int32_t* d_count, int cap) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_landmarks(s->pairs, s->ctx->device, d_out, d_count, cap));
}

int dvo_stream_set_tracks(dvo_stream* s, int32_t* d_link, dvo_track_scale* d_scale) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_tracks(s->pairs, s->ctx->device, d_link, d_scale));
}

int dvo_stream_set_track_poses(dvo_stream* s, dvo_track_pose* d_pose, int iters, double huber_px, double inlier_px,
                               int min_points) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_poses(s->pairs, s->ctx->device, d_pose, iters, huber_px, inlier_px, min_points));
}

int dvo_stream_set_track_refine(dvo_stream* s, dvo_landmark_refined* d_refined, dvo_track_id* d_id, int views,
                                int iters, double huber_px, double inlier_px) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx,
                       s->next.set_track_refine(s->pairs, s->ctx->device, d_refined, d_id, views, iters, huber_px, inlier_px));
}

int dvo_stream_set_track_bundle(dvo_stream* s, dvo_track_bundle* d_bundle, dvo_landmark_refined* d_points, int views,
                                int iters, double lambda, double huber_px, double inlier_px, int min_points) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_bundle(s->pairs, s->ctx->device, d_bundle, d_points, views, iters, lambda,
                                                        huber_px, inlier_px, min_points));
}

int dvo_stream_set_track_pnp(dvo_stream* s, dvo_track_pnp* d_pnp, uint8_t* d_mask, int mask_cap, int hyps, int iters,
                             double huber_px, double inlier_px, int min_points, uint64_t seed) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_pnp(s->pairs, s->ctx->device, d_pnp, d_mask, mask_cap, hyps, iters, huber_px,
                                                     inlier_px, min_points, seed));
}

int dvo_track_pnp_samples_host(int n, int hyps, uint64_t seed, int32_t* out) {
    if (n < 1 || hyps < 1 || hyps > kPnpMaxHyps || !out) return DVO_EINVAL;
    for (int h = 0; h < hyps; ++h) {
        int idx[3] = {-1, -1, -1};
        p3p_sample(seed, h, n, idx);
        for (int j = 0; j < 3; ++j) out[3 * h + j] = idx[j];
    }
    return DVO_OK;
}

int dvo_p3p_host(const double* Y, const double* nunv, double* R, double* t, int* n_solutions) {
    if (!Y || !nunv || !R || !t || !n_solutions) return DVO_EINVAL;
    double Rs[4][9], ts[4][3];
    const int n = p3p_solve(Y, nunv, Rs, ts);
    for (int s = 0; s < n; ++s) {
        for (int i = 0; i < 9; ++i) R[9 * s + i] = Rs[s][i];
        for (int i = 0; i < 3; ++i) t[3 * s + i] = ts[s][i];
    }
    *n_solutions = n;
    return DVO_OK;
}

int dvo_stream_sync(dvo_stream* s) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipStreamSynchronize(s->hs));
    HIP_TRY(hipGetLastError());
    return DVO_OK;
}

int dvo_stream_get_features(dvo_stream* s, int frame, dvo_keypoint* kps, uint8_t* desc, int cap, int* n) {
    if (!s || !n) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (frame < 0 || frame >= s->last_nframes) return fail(ctx, DVO_EINVAL, "frame out of range");
    HIP_TRY(hipStreamSynchronize(s->hs));
    int nk = 0, st = 0;
    HIP_TRY(hipMemcpy(&nk, s->buf.nkp + frame, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&st, s->buf.status + frame, sizeof(int), hipMemcpyDeviceToHost));
    *n = nk;
    if (st) return fail(ctx, DVO_ECAP, "keypoint capacity exceeded (Harris ties)");
    if (nk > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (nk > 0) {
        if (kps)
            HIP_TRY(hipMemcpy(kps, s->buf.kps + (size_t)frame * s->plan.kp_cap, sizeof(dvo_keypoint) * nk,
                              hipMemcpyDeviceToHost));
        if (desc)
            HIP_TRY(hipMemcpy(desc, s->buf.desc + (size_t)frame * s->plan.kp_cap * 32, 32 * (size_t)nk,
                              hipMemcpyDeviceToHost));
    }
    return DVO_OK;
}

int dvo_stream_get_matches(dvo_stream* s, int pair, dvo_dmatch* out, int cap, int* m) {
    if (!s || !m) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (pair < 0 || pair >= s->last_sub_pairs) return fail(ctx, DVO_EINVAL, "pair out of range");
    HIP_TRY(hipStreamSynchronize(s->hs));
    int nm = 0;
    HIP_TRY(hipMemcpy(&nm, s->pairs.view(s->last_set).nmatch + pair, sizeof(int), hipMemcpyDeviceToHost));
    *m = nm;
    if (nm > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    std::vector<int32_t> q(nm), t(nm);
    std::vector<float> d(nm);
    const size_t off = (size_t)pair * s->plan.kp_cap;
    if (nm) {
        HIP_TRY(hipMemcpy(q.data(), s->buf.mq + off, 4 * (size_t)nm, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t.data(), s->buf.mt + off, 4 * (size_t)nm, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(d.data(), s->buf.md + off, 4 * (size_t)nm, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < nm; ++i) out[i] = dvo_dmatch{q[i], t[i], 0, d[i]};
    return DVO_OK;
}

int dvo_stream_get_pyramid(dvo_stream* s, int frame, int level, int blurred, uint8_t* out, int cap) {
    if (!s || !out) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (frame < 0 || frame >= s->last_nframes || level < 0 || level >= s->plan.nlevels)
        return fail(ctx, DVO_EINVAL, "frame/level out of range");
    int nfr = s->last_nframes;
    if (s->last_reuse) {  // dvo_stream_pair(reuse_prev) detected frame 1 alone, into pyramid slot 0
        if (frame == 0)
            return fail(ctx, DVO_EINVAL, "after dvo_stream_pair(reuse_prev) only frame 1's pyramid is kept");
        frame = 0;
        nfr = 1;
    }
    const LevelGeom& G = s->plan.L[level];
    if (cap < G.w * G.h) return fail(ctx, DVO_ECAP, "capacity too small");
    HIP_TRY(hipStreamSynchronize(s->hs));
    if (blurred) {
        // the detection path blurs only the descriptor windows (describe_kernel): the whole blurred
        // pyramid is recomputed here from the last call's frames, which must still be alive
        HIP_TRY(launch_blur(params_of(s, s->last_frames, nfr, s->last_fstride, s->last_pitch), s->hs));
        HIP_TRY(hipStreamSynchronize(s->hs));
    }
    if (blurred) {
        HIP_TRY(hipMemcpy2D(out, G.w, s->buf.blur + (size_t)frame * s->plan.blur_stride + G.blur_off, G.bpitch, G.w,
                            G.h, hipMemcpyDeviceToHost));
    } else {
        if (level == 0) return fail(ctx, DVO_EINVAL, "level 0 is the input frame");
        HIP_TRY(hipMemcpy2D(out, G.w, s->buf.pyr + (size_t)frame * s->plan.pyr_stride + G.pyr_off, G.pitch, G.w,
                            G.h, hipMemcpyDeviceToHost));
    }
    return DVO_OK;
}

// ---------------------------------------------------------------------------
int dvo_orb_detect_and_compute(dvo_ctx* ctx, const dvo_orb_params* params, const uint8_t* img, int w, int h,
                               int stride, dvo_keypoint* kps, uint8_t* desc, int cap, int* n_out) {
    if (!ctx) return DVO_EINVAL;
    int rc = check_orb_params(ctx, params);
    if (rc) return rc;
    if (!img || !n_out || stride < w) return fail(ctx, DVO_EINVAL, "bad image buffer");
    if (w < 8 || h < 8 || w >= kMaxW || h >= kMaxW) return fail(ctx, DVO_EINVAL, "image size out of range (8..4095)");
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->call_stream || ctx->call_w != w || ctx->call_h != h || ctx->call_nf != params->nfeatures ||
        ctx->call_stream->cfg.orb.fast_threshold != params->fast_threshold ||
        ctx->call_stream->cfg.orb.opencv_semantics != params->opencv_semantics) {
        if (ctx->call_stream) dvo_stream_destroy(ctx->call_stream);
        ctx->call_stream = nullptr;
        dvo_stream_config cfg{};
        cfg.width = w;
        cfg.height = h;
        cfg.max_frames = 2;
        cfg.orb = *params;
        cfg.K[0] = cfg.K[4] = cfg.K[8] = 1.0;
        cfg.prob = 0.999;
        cfg.threshold = 1.0;
        cfg.max_iters = 1000;
        cfg.cross_check = 1;
        cfg.dist_thresh = 50.0;
        rc = dvo_stream_create(ctx, &cfg, &ctx->call_stream);
        if (rc) return rc;
        ctx->call_w = w;
        ctx->call_h = h;
        ctx->call_nf = params->nfeatures;
    }
    dvo_stream* s = ctx->call_stream;
    const int pw = frame_pitch(s);
    const size_t kc = (size_t)s->plan.kp_cap;
    CallMem mem(ctx->call, s->hs);
    HIP_TRY(hipMemcpy2DAsync(s->d_frames, pw, img, stride, w, h, hipMemcpyHostToDevice, s->hs));
    rc = run_stream(s, s->d_frames, 1, (int64_t)pw * h, pw, nullptr, true);
    if (rc) return rc;
    // dvo_stream_get_features of frame 0, with every list copied back at once (capacity-sized)
    uint8_t *hn, *hst, *hk = nullptr, *hd = nullptr;
    HIP_TRY(mem.get(s->buf.nkp, sizeof(int), &hn));
    HIP_TRY(mem.get(s->buf.status, sizeof(int), &hst));
    if (kps) HIP_TRY(mem.get(s->buf.kps, kc * sizeof(dvo_keypoint), &hk));
    if (desc) HIP_TRY(mem.get(s->buf.desc, kc * 32, &hd));
    HIP_TRY(hipStreamSynchronize(s->hs));
    int nk = 0, stt = 0;
    std::memcpy(&nk, hn, sizeof(int));
    std::memcpy(&stt, hst, sizeof(int));
    *n_out = nk;
    if (stt) return fail(ctx, DVO_ECAP, "keypoint capacity exceeded (Harris ties)");
    if (nk > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (nk > 0) {
        if (kps) std::memcpy(kps, hk, sizeof(dvo_keypoint) * nk);
        if (desc) std::memcpy(desc, hd, 32 * (size_t)nk);
    }
    return DVO_OK;
}

int dvo_bf_match_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int cross_check,
                         dvo_dmatch* out, int cap, int* m_out) {
    if (!ctx || !m_out) return DVO_EINVAL;
    *m_out = 0;
    if (cross_check < 0 || cross_check > 2) return fail(ctx, DVO_EINVAL, "cross_check must be 0, 1 or 2");
    if (nq < 0 || nt < 0 || nq > 8192 || nt > 8192)
        return fail(ctx, DVO_EINVAL, "descriptor count out of range (0..8192)");
    if (nq == 0 || nt == 0) return DVO_OK;  // BFMatcher returns no matches
    if (!dq || !dt || !out) return fail(ctx, DVO_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* bq = mem.dev<uint8_t>((size_t)nq * 32);
    uint8_t* bt = mem.dev<uint8_t>((size_t)nt * 32);
    uint8_t* bnn = mem.dev<uint8_t>(match_pair_work_size(nq, nt));
    dvo_dmatch* bout = mem.dev<dvo_dmatch>(nq);
    int* bm = mem.dev<int>(16);
    HIP_TRY(mem.error());
    HIP_TRY(mem.put(bq, dq, (size_t)nq * 32));
    HIP_TRY(mem.put(bt, dt, (size_t)nt * 32));
    HIP_TRY(launch_match_pair(bq, nq, bt, nt, cross_check, bnn, bout, bm, ctx->stream));
    uint8_t *hm, *hout;
    HIP_TRY(mem.get(bm, sizeof(int), &hm));
    HIP_TRY(mem.get(bout, (size_t)nq * sizeof(dvo_dmatch), &hout));  // at most one match per query
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int m = 0;
    std::memcpy(&m, hm, sizeof(int));
    *m_out = m;
    if (m > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (m) std::memcpy(out, hout, (size_t)m * sizeof(dvo_dmatch));
    return DVO_OK;
}

int dvo_test_bf_knn_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int k, int tsplit,
                            int32_t* train_idx, float* dist) {
    if (!ctx) return DVO_EINVAL;
    if (k < 1 || k > 2) return fail(ctx, DVO_EINVAL, "k must be 1 or 2");
    if (tsplit < 0 || tsplit > 16) return fail(ctx, DVO_EINVAL, "tsplit must be 0 (chosen by size) .. 16");
    if (nq < 0 || nt < 0 || nq > 8192 || nt > 8192)
        return fail(ctx, DVO_EINVAL, "descriptor count out of range (0..8192)");
    if (nq == 0) return DVO_OK;
    if (!dq || !train_idx || !dist || (nt > 0 && !dt)) return fail(ctx, DVO_EINVAL, "null buffer");
    if (nt == 0) {  // batchDistance leaves every slot at (-1, FLT_MAX)
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            train_idx[i] = -1;
            dist[i] = FLT_MAX;
        }
        return DVO_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (tsplit == 0) tsplit = hamming_knn_split(nq, nt);
    const size_t out_n = (size_t)nq * k;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* bq = mem.dev<uint8_t>((size_t)nq * 32);
    uint8_t* bt = mem.dev<uint8_t>((size_t)nt * 32);
    uint8_t* bw = mem.dev<uint8_t>(hamming_knn_work_size(nq, tsplit));
    int32_t* bi = mem.dev<int32_t>(out_n);
    float* bd = mem.dev<float>(out_n);
    HIP_TRY(mem.error());
    uint8_t *hi = nullptr, *hd = nullptr;
    // after the first upload an error drains the stream before returning (the copies use the
    // context's pinned buffers, which the next per-call entry point rewrites)
    auto body = [&]() -> int {
        HIP_TRY(mem.put(bq, dq, (size_t)nq * 32));
        HIP_TRY(mem.put(bt, dt, (size_t)nt * 32));
        HIP_TRY(launch_knn_hamming_pair(bq, nq, bt, nt, k, tsplit, bw, bi, bd, ctx->stream));
        HIP_TRY(mem.get(bi, out_n * 4, &hi));
        HIP_TRY(mem.get(bd, out_n * 4, &hd));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DVO_OK;
    };
    if (int rc = body()) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    std::memcpy(train_idx, hi, out_n * 4);
    std::memcpy(dist, hd, out_n * 4);
    return DVO_OK;
}

int dvo_bf_knn_hamming(dvo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int k, int32_t* train_idx,
                       float* dist) {
    return dvo_test_bf_knn_hamming(ctx, dq, nq, dt, nt, k, 0, train_idx, dist);
}

int dvo_bf_knn_float(dvo_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, int norm,
                     int32_t* train_idx, float* dist) {
    if (!ctx) return DVO_EINVAL;
    if (norm != DVO_NORM_L1 && norm != DVO_NORM_L2SQR) return fail(ctx, DVO_EINVAL, "norm must be DVO_NORM_L1 or DVO_NORM_L2SQR");
    if (dim != 64 && dim != 128) return fail(ctx, DVO_EINVAL, "descriptor length must be 64 (SURF) or 128 (SIFT)");
    if (k < 1 || k > 4) return fail(ctx, DVO_EINVAL, "k must be 1..4");
    if (nq < 0 || nt < 0 || nq > (1 << 20) || nt > (1 << 20))
        return fail(ctx, DVO_EINVAL, "descriptor count out of range (0..2^20)");
    if (nq == 0) return DVO_OK;
    if (!dq || !train_idx || !dist || (nt > 0 && !dt)) return fail(ctx, DVO_EINVAL, "null buffer");
    if (nt == 0) {  // batchDistance leaves every slot at (-1, FLT_MAX)
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            train_idx[i] = -1;
            dist[i] = FLT_MAX;
        }
        return DVO_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int ranges = knn_ranges(nq, nt, cus);
    const size_t out_n = (size_t)nq * k, part_n = ranges > 1 ? (size_t)ranges * nq * k : 1;
    CallMem mem(ctx->call, ctx->stream);
    float* bq = mem.dev<float>((size_t)nq * dim);
    float* bt = mem.dev<float>((size_t)nt * dim);
    float* bd = mem.dev<float>(out_n);
    int32_t* bi = mem.dev<int32_t>(out_n);
    float* bpd = mem.dev<float>(part_n);
    int32_t* bpi = mem.dev<int32_t>(part_n);
    uint8_t* bb = mem.dev<uint8_t>(knn_bytes_size(nq, nt, dim));
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpyAsync(bq, dq, (size_t)nq * dim * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(bt, dt, (size_t)nt * dim * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_knn_float(bq, nq, bt, nt, dim, k, norm, ranges, bb, bpd, bpi, bd, bi, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dist, bd, out_n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(train_idx, bi, out_n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

namespace {
// cv::theRNG()'s multiply-with-carry s' = (u32)s * A + (s >> 32) is s' = s * A mod m,
// m = A * 2^32 - 1, for every state below m (all but a few seeds): jump k steps ahead.
constexpr uint64_t kTheRngA = 4164903690ull;
uint64_t therng_jump(uint64_t s, uint64_t k) {
    const unsigned __int128 m = ((unsigned __int128)kTheRngA << 32) - 1;
    if (k > 0 && (unsigned __int128)s >= m) {  // a seed at or above m: one plain step lands below m
        s = (uint64_t)(uint32_t)s * kTheRngA + (s >> 32);
        --k;
    }
    unsigned __int128 r = s, b = kTheRngA;
    for (; k; k >>= 1) {
        if (k & 1) r = r * b % m;
        b = b * b % m;
    }
    return (uint64_t)r;
}
}  // namespace

// The kd-forest build and search of dvo_flann_knn on device descriptors (bq: nq x dim, bt: nt x dim,
// already validated: nq, nt >= 1, k <= nt): scratch and the results (*d_idx, *d_dist: nq x k, valid
// once the stream has run) come from the call's CallMem.  rng_state is the theRNG state before
// the call; the caller advances it (flann_rng_after) when its call succeeds.
static int flann_knn_device(dvo_ctx* ctx, CallMem& mem, const float* bq, int nq, const float* bt, int nt, int dim,
                            int k, int trees, int checks, uint64_t rng_state, int32_t** d_idx, float** d_dist) {
    const int n = nt, draws = 2 * n - 1, nodes_per_tree = 2 * n - 1;
    constexpr int kChunks = 64;
    hipStream_t s = ctx->stream;
    uint32_t* bR = mem.dev<uint32_t>(draws);
    uint64_t* bcs = mem.dev<uint64_t>((size_t)trees * kChunks);
    int* bcnt = mem.dev<int>(n);
    int* boff = mem.dev<int>(n + 1);
    int* bfill = mem.dev<int>(n);
    int* blist = mem.dev<int>(n);
    int* ind = mem.dev<int>(n);
    int* ind2 = mem.dev<int>(n);
    float* bxv = mem.dev<float>(n);
    int* bsl = mem.dev<int>(n);
    int* bsr = mem.dev<int>(n);
    int4* bnodes = mem.dev<int4>((size_t)trees * nodes_per_tree);
    int4* bopen = mem.dev<int4>((size_t)2 * n);
    int* blev = mem.dev<int>(n + 2);
    int32_t* bidx = mem.dev<int32_t>((size_t)nq * k);
    float* bdist = mem.dev<float>((size_t)nq * k);
    int32_t* bflag = mem.dev<int32_t>(nq);
    int32_t* bredo = mem.dev<int32_t>(nq + 1);
    HIP_TRY(mem.error());
    // the multiply-with-carry state at the start of every draw chunk of every tree (tree t's draws
    // begin t (2n - 1) steps after the call's state)
    std::vector<uint64_t> cs((size_t)trees * kChunks);
    for (int t = 0; t < trees; ++t)
        for (int c = 0; c < kChunks; ++c)
            cs[(size_t)t * kChunks + c] =
                therng_jump(rng_state, (uint64_t)t * draws + (uint64_t)((int64_t)draws * c / kChunks));
    HIP_TRY(mem.put(bcs, cs.data(), cs.size() * 8));
    // ind = 0..n-1 once; every tree shuffles the previous tree's final order (KDTreeIndex::buildIndex)
    {
        std::vector<int32_t> iota(n);
        for (int i = 0; i < n; ++i) iota[i] = i;
        HIP_TRY(hipMemcpyAsync(ind, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));  // the pageable copy must finish before iota goes out of scope
    }
    int32_t* hcnt = reinterpret_cast<int32_t*>(mem.host(4));
    int32_t* hredo = reinterpret_cast<int32_t*>(mem.host(4));
    HIP_TRY(mem.error());
    for (int t = 0; t < trees; ++t) {
        HIP_TRY(launch_flann_draws(bcs + (size_t)t * kChunks, kChunks, draws, bR, s));
        HIP_TRY(launch_flann_shuffle(bR, n, bcnt, boff, bfill, blist, ind, ind2, s));
        std::swap(ind, ind2);
        FlannBuildArgs a{bt, n, dim, ind, bxv, bsl, bsr, bR, bnodes + (size_t)t * nodes_per_tree, bopen, bopen + n, blev};
        HIP_TRY(hipMemsetAsync(blev, 0, (size_t)(n + 2) * 4, s));
        HIP_TRY(launch_flann_root(a, s));
        // level-synchronous divideTree: a level has at most min(2^d, n / 2) open nodes; levels go in
        // batches of 8, then the host reads whether the next level has any
        for (int d = 0; d < n; d += 8) {
            for (int e = d; e < d + 8 && e < n; ++e)
                HIP_TRY(launch_flann_level(a, e, (int)std::min<int64_t>(int64_t(1) << std::min(e, 20), n / 2 + 1), s));
            HIP_TRY(hipMemcpyAsync(hcnt, blev + std::min(d + 8, n + 1), 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*hcnt == 0) break;
        }
    }
    FlannSearchArgs sa{bq, bt, bnodes, nq, n, dim, k, trees, checks, bidx, bdist, bflag};
    HIP_TRY(launch_flann_search(sa, s));
    HIP_TRY(launch_flann_redo_list(bflag, nq, bredo + 1, bredo, s));
    HIP_TRY(hipMemcpyAsync(hredo, bredo, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // queries whose heap outgrew LDS, with the heap in global memory: batches of at most 256
    const size_t heap_n = (size_t)std::min(*hredo, 256) * n;
    float* bhd = mem.dev<float>(heap_n);
    int32_t* bhn = mem.dev<int32_t>(heap_n);
    HIP_TRY(mem.error());
    for (int done = 0; done < *hredo;) {
        const int batch = std::min(*hredo - done, 256);
        HIP_TRY(launch_flann_search_global(sa, bredo + 1 + done, batch, bhd, bhn, s));
        done += batch;
    }
    *d_idx = bidx;
    *d_dist = bdist;
    return DVO_OK;
}
// the theRNG state after a forest of `trees` trees over nt points: trees (2 nt - 1) draws on
static uint64_t flann_rng_after(uint64_t state, int trees, int nt) {
    return therng_jump(state, (uint64_t)trees * (uint64_t)(2 * nt - 1));
}

// Replaces cv::FlannBasedMatcher(KDTREE, trees).knnMatch(query, train, k) with
// search checks (the 'flann' mode, visual_odometry_v3.py:206-212); flann.hip.
int dvo_flann_knn(dvo_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, int trees,
                  int checks, uint64_t* rng_state, int32_t* train_idx, float* dist) {
    if (!ctx) return DVO_EINVAL;
    if (!rng_state) return fail(ctx, DVO_EINVAL, "null theRNG state");
    if (dim < 4 || dim > 256 || dim % 4) return fail(ctx, DVO_EINVAL, "dim must be a multiple of 4 in 4..256");
    if (k < 1 || k > 4) return fail(ctx, DVO_EINVAL, "k must be 1..4");
    if (trees < 1 || trees > 64 || checks < 1) return fail(ctx, DVO_EINVAL, "trees 1..64 and checks >= 1");
    if (nq < 0 || nt < 0 || nq > (1 << 20) || nt > (1 << 16))
        return fail(ctx, DVO_EINVAL, "descriptor counts out of range (queries 0..2^20, train 0..2^16)");
    // DescriptorMatcher::knnMatch returns before training on an empty query or train set
    if (nq == 0 || nt == 0) return DVO_OK;
    if (!dq || !dt || !train_idx || !dist) return fail(ctx, DVO_EINVAL, "null buffer");
    if (k > nt) return fail(ctx, DVO_EINVAL, "k exceeds the train set (FLANN asserts knn <= index size)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CallMem mem(ctx->call, s);
    float* bq = mem.dev<float>((size_t)nq * dim);
    float* bt = mem.dev<float>((size_t)nt * dim);
    HIP_TRY(mem.error());
    HIP_TRY(mem.put(bq, dq, (size_t)nq * dim * 4));
    HIP_TRY(mem.put(bt, dt, (size_t)nt * dim * 4));
    int32_t* bidx = nullptr;
    float* bdist = nullptr;
    int rc = flann_knn_device(ctx, mem, bq, nq, bt, nt, dim, k, trees, checks, *rng_state, &bidx, &bdist);
    if (rc) return rc;
    uint8_t *hi, *hd;
    HIP_TRY(mem.get(bidx, (size_t)nq * k * 4, &hi));
    HIP_TRY(mem.get(bdist, (size_t)nq * k * 4, &hd));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(train_idx, hi, (size_t)nq * k * 4);
    std::memcpy(dist, hd, (size_t)nq * k * 4);
    *rng_state = flann_rng_after(*rng_state, trees, nt);
    return DVO_OK;
}

namespace {
// Keypoint list capacity of the detectors' plans (SiftArgs / SurfArgs::kp_cap).
constexpr int kSiftKpCap = 1 << 16;
int surf_kp_cap(int w, int h) { return std::max(4096, (w * h) / 64); }

// getGaussianKernel(ksize = cvRound(sigma * 8 + 1) | 1, sigma, CV_32F), as oracle/sift.cpp gauss_kernel
std::vector<float> sift_gauss_taps(double sigma) {
    const int n = (int)std::nearbyint(sigma * 4 * 2 + 1) | 1;
    std::vector<float> k(n);
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        k[i] = (float)std::exp(scale2X * x * x);
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
    return k;
}

// The octave layout of a w x h image and the list capacities: what sift_plan and the group
// detector's scratch (sift_group_alloc, dvo_sift_batch_bytes) both size their buffers from.
// *gp_floats / *dog_floats: the pyramid's and the DoG's floats (6 S and 5 S, S the octaves' pixels).
void sift_layout(int w, int h, SiftLayout& A, int64_t* gp_floats, int64_t* dog_floats) {
    const int W = 2 * w, H = 2 * h;  // firstOctave = -1
    A.noct = (int)std::nearbyint(std::log((double)std::min(W, H)) / std::log(2.) - 2) + 1;
    A.noct = std::max(1, std::min(A.noct, kSiftMaxOct));
    int64_t gp = 0, dg = 0;
    for (int o = 0; o < A.noct; ++o) {
        A.ow[o] = o == 0 ? W : A.ow[o - 1] / 2;
        A.oh[o] = o == 0 ? H : A.oh[o - 1] / 2;
        if (A.ow[o] < 1 || A.oh[o] < 1) {  // as small as the pyramid goes
            A.noct = o;
            break;
        }
        const int64_t px = (int64_t)A.ow[o] * A.oh[o];
        for (int l = 0; l < 6; ++l) A.gp_off[o * 6 + l] = gp + l * px;
        for (int l = 0; l < 5; ++l) A.dog_off[o * 5 + l] = dg + l * px;
        gp += 6 * px;
        dg += 5 * px;
    }
    A.cand_cap = 1 << 18;
    A.kp_cap = kSiftKpCap;
    *gp_floats = gp;
    *dog_floats = dg;
}

int sift_order_n(int kp_cap) {  // the sort scratch: the next power of two >= kp_cap
    int order_n = 1;
    while (order_n < kp_cap) order_n <<= 1;
    return order_n;
}

// The 6 Gaussian kernels (initial blur, layers 1..5) back to back.
std::vector<float> sift_taps(int* tap_off, int* tap_n) {
    std::vector<float> taps;
    const double sig0 = std::sqrt(std::max(1.6f * 1.6f - 0.5f * 0.5f * 4, 0.01f));
    std::vector<double> sig(6);
    sig[0] = sig0;
    const double k = std::pow(2., 1. / 3);
    for (int i = 1; i < 6; ++i) {
        // buildGaussianPyramid uses SIFT_Impl's double member sigma (1.6, not 1.6f);
        // only createInitialImage and adjustLocalExtrema take it as float
        const double sig_prev = std::pow(k, (double)(i - 1)) * 1.6, sig_total = sig_prev * k;
        sig[i] = std::sqrt(sig_total * sig_total - sig_prev * sig_prev);
    }
    for (int i = 0; i < 6; ++i) {
        const std::vector<float> t = sift_gauss_taps(i == 0 ? (double)(float)sig0 : sig[i]);
        tap_off[i] = (int)taps.size();
        tap_n[i] = (int)t.size();
        taps.insert(taps.end(), t.begin(), t.end());
    }
    return taps;
}

int sift_plan(dvo_ctx* ctx, int w, int h) {
    SiftPlanDev& P = ctx->sift;
    if (P.w == w && P.h == h) return DVO_OK;
    P = SiftPlanDev{};
    SiftArgs& A = P.a;
    const int W = 2 * w, H = 2 * h;
    int64_t gp = 0, dg = 0;
    sift_layout(w, h, A, &gp, &dg);
    const std::vector<float> taps = sift_taps(P.tap_off, P.tap_n);
    P.pitch = (w + 255) & ~255;
    auto A_ = [&](auto*& p, size_t bytes) { return P.mem.alloc(&p, bytes ? bytes : 16) == hipSuccess; };
    const int order_n = sift_order_n(A.kp_cap);
    int* counters = nullptr;
    if (!A_(A.gp, (size_t)gp * 4) || !A_(A.dog, (size_t)dg * 4) || !A_(A.tmp, (size_t)W * H * 4) ||
        !A_(A.cand, (size_t)A.cand_cap * sizeof(int4)) || !A_(A.raw, (size_t)A.kp_cap * sizeof(dvo_keypoint)) ||
        !A_(A.order, (size_t)order_n * 4) || !A_(A.kps, (size_t)A.kp_cap * sizeof(dvo_keypoint)) ||
        !A_(A.desc, (size_t)A.kp_cap * 128 * 4) || !A_(counters, 64) || !A_(P.taps, taps.size() * 4) ||
        !A_(P.img, (size_t)P.pitch * h)) {
        P = SiftPlanDev{};
        return fail(ctx, DVO_EHIP, "SIFT buffers: hipMalloc failed");
    }
    A.ncand = counters;
    A.nraw = counters + 1;
    A.nkp = counters + 2;
    A.flags = counters + 3;
    if (hipMemcpy(P.taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(ctx, DVO_EHIP, "SIFT taps upload failed");
    P.w = w;
    P.h = h;
    return DVO_OK;
}

// One frame's share of a group's scratch, array by array (bytes).
struct SiftGroupBytes {
    int64_t gp, dog, tmp, cand, raw, order, counters;
    int64_t frame() const { return gp + dog + tmp + cand + raw + order + counters; }
};
SiftGroupBytes sift_group_bytes(int w, int h, SiftLayout& L) {
    int64_t gp = 0, dg = 0;
    sift_layout(w, h, L, &gp, &dg);
    SiftGroupBytes b;
    b.gp = gp * 4;
    b.dog = dg * 4;
    b.tmp = (int64_t)4 * w * h * 4;
    b.cand = (int64_t)L.cand_cap * (int64_t)sizeof(int4);
    b.raw = (int64_t)L.kp_cap * (int64_t)sizeof(dvo_keypoint);
    b.order = (int64_t)sift_order_n(L.kp_cap) * 4;
    b.counters = 16;
    return b;
}

constexpr int kSiftGroupMax = 64;

// Allocates a group's whole scratch and uploads the taps, after waiting for the context's stream
// (nothing is allocated later, inside a detect / process call).  D is empty on failure.
int sift_group_alloc(dvo_ctx* ctx, int w, int h, int group, SiftGroupDev& D) {
    D = SiftGroupDev{};
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    SiftGroupArgs& g = D.g;
    const SiftGroupBytes b = sift_group_bytes(w, h, g.l);
    const std::vector<float> taps = sift_taps(D.tap_off, D.tap_n);
    const int64_t G = group;
    int* counters = nullptr;
    hipError_t e = hipSuccess;
    auto A_ = [&](auto*& p, int64_t bytes) {
        if (e == hipSuccess) e = D.mem.alloc(&p, (size_t)bytes);
    };
    A_(g.b.gp, G * b.gp);
    A_(g.b.dog, G * b.dog);
    A_(g.b.tmp, G * b.tmp);
    A_(g.b.cand, G * b.cand);
    A_(g.b.raw, G * b.raw);
    A_(g.b.order, G * b.order);
    A_(counters, G * b.counters);
    A_(D.taps, (int64_t)taps.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(D.taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        D = SiftGroupDev{};
        return fail(ctx, DVO_EHIP, std::string("SIFT group buffers: ") + hipGetErrorString(e));
    }
    g.b.ncand = counters;
    g.b.nraw = counters + 1;
    g.b.nkp = counters + 2;
    g.b.flags = counters + 3;
    g.gp_stride = b.gp / 4;
    g.dog_stride = b.dog / 4;
    g.tmp_stride = b.tmp / 4;
    g.order_stride = b.order / 4;
    // DVO_SIFT_FUSED_BLUR=0 (read here, when the scratch is made) keeps the two-pass blurs: the A/B of
    // tools/time_sift_batch.py.  The results are the same either way.
    const char* fb = std::getenv("DVO_SIFT_FUSED_BLUR");
    g.fused_blur = !(fb && fb[0] == '0');
    D.w = w;
    D.h = h;
    D.group = group;
    return DVO_OK;
}

// One frame's share of the retain stage's scratch (SiftRetainArgs): the list, the responses, their
// positions and the two position arrays of kp_cap + 1.
int64_t sift_retain_frame_bytes() {
    return (int64_t)kSiftKpCap * ((int64_t)sizeof(dvo_keypoint) + 8) + 2 * (int64_t)(kSiftKpCap + 1) * 4;
}

// The retain scratch for at least `frames` frames, allocated whole after waiting for the context's
// stream (a setter's or a synchronous call's job: nothing is allocated inside a detect call).
// D is empty on failure.
int sift_retain_ensure(dvo_ctx* ctx, SiftRetainDev& D, int frames) {
    if (D.frames >= frames) return DVO_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the old scratch may be in use
    D = SiftRetainDev{};
    const int64_t G = frames, C = kSiftKpCap;
    hipError_t e = hipSuccess;
    auto A_ = [&](auto*& p, int64_t n) {
        if (e == hipSuccess) e = D.mem.alloc(&p, (size_t)n * sizeof(*p));
    };
    A_(D.a.list, G * C);
    A_(D.a.resp, G * C);
    A_(D.a.idx, G * C);
    A_(D.a.lpos, G * (C + 1));
    A_(D.a.rasc, G * (C + 1));
    if (e != hipSuccess) {
        D = SiftRetainDev{};
        return fail(ctx, DVO_EHIP, std::string("SIFT retain buffers: ") + hipGetErrorString(e));
    }
    D.frames = frames;
    return DVO_OK;
}

// n frames through the group detector, in chunks of D.group on stream s: frame f's keypoints and
// descriptors go to kps + f * feat_cap and desc + f * feat_cap * 128, its (count, flags) to counts + 2 f.
// nfeatures > 0: retainBest before the descriptors, on R's scratch (D.group frames of it).
int sift_group_detect(dvo_ctx* ctx, const SiftGroupDev& D, const uint8_t* d_frames, int n, int64_t frame_stride, int stride,
                      int feat_cap, dvo_keypoint* kps, float* desc, int32_t* counts, hipStream_t s, int nfeatures = 0,
                      const SiftRetainDev* R = nullptr) {
    SiftRetainArgs ra{};
    if (nfeatures > 0) {
        if (!R || R->frames < D.group) return fail(ctx, DVO_EINVAL, "SIFT retain scratch is missing");
        ra = R->a;
        ra.nfeatures = nfeatures;
    }
    for (int f0 = 0; f0 < n; f0 += D.group) {
        const int frames = std::min(D.group, n - f0);
        SiftGroupArgs g = D.g;
        g.out_kps = kps + (size_t)f0 * feat_cap;
        g.out_desc = desc + (size_t)f0 * feat_cap * 128;
        g.out_n = counts + 2 * (size_t)f0;
        g.feat_cap = feat_cap;
        HIP_TRY(hipMemsetAsync(g.b.ncand, 0, (size_t)frames * 16, s));  // the chunk's counters, all four per frame
        HIP_TRY(launch_sift_group(g, frames, d_frames + (int64_t)f0 * frame_stride, frame_stride, D.w, D.h, stride, D.taps,
                                  D.tap_off, D.tap_n, s, nfeatures > 0 ? &ra : nullptr));
    }
    return DVO_OK;
}
}  // namespace

struct dvo_sift_batch {
    dvo_ctx* ctx = nullptr;
    SiftGroupDev d;
    int nfeatures = 0;     // dvo_sift_batch_set_nfeatures
    SiftRetainDev retain;  // its scratch, d.group frames once nfeatures was set
};

int64_t dvo_sift_batch_bytes(int w, int h, int group) {
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW || group < 1 || group > kSiftGroupMax) return DVO_EINVAL;
    SiftLayout L{};
    int off[6], n[6];
    return group * sift_group_bytes(w, h, L).frame() + (int64_t)sift_taps(off, n).size() * 4;
}

int64_t dvo_sift_retain_bytes(int group) {
    return group < 1 || group > kSiftGroupMax ? 0 : group * sift_retain_frame_bytes();
}

int dvo_sift_batch_set_nfeatures(dvo_sift_batch* b, int nfeatures) {
    if (!b) return DVO_EINVAL;
    dvo_ctx* ctx = b->ctx;
    if (nfeatures < 0) return fail(ctx, DVO_EINVAL, "nfeatures must be >= 0");
    if (nfeatures == b->nfeatures) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nfeatures > 0) {
        const int rc = sift_retain_ensure(ctx, b->retain, b->d.group);
        if (rc) return rc;
    }
    b->nfeatures = nfeatures;
    return DVO_OK;
}

int dvo_sift_batch_create(dvo_ctx* ctx, int w, int h, int group, dvo_sift_batch** out) {
    if (!ctx || !out) return DVO_EINVAL;
    *out = nullptr;
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW) return fail(ctx, DVO_EINVAL, "image size out of range (1..4095)");
    if (group < 1 || group > kSiftGroupMax) return fail(ctx, DVO_EINVAL, "group out of range (1..64)");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvo_sift_batch> b(new dvo_sift_batch);
    b->ctx = ctx;
    const int rc = sift_group_alloc(ctx, w, h, group, b->d);
    if (rc) return rc;
    *out = b.release();
    return DVO_OK;
}

void dvo_sift_batch_destroy(dvo_sift_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    delete b;
}

void* dvo_sift_batch_hip_stream(dvo_sift_batch* b) { return b ? (void*)b->ctx->stream : nullptr; }

int dvo_sift_batch_detect(dvo_sift_batch* b, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          int feat_cap, dvo_keypoint* d_kps, float* d_desc, int32_t* d_counts) {
    if (!b) return DVO_EINVAL;
    dvo_ctx* ctx = b->ctx;
    if (n_frames < 1) return fail(ctx, DVO_EINVAL, "n_frames must be >= 1");
    if (!d_frames || !d_kps || !d_desc || !d_counts || stride < b->d.w)
        return fail(ctx, DVO_EINVAL, "bad frame or output buffer");
    if (feat_cap < 1 || feat_cap > kSiftKpCap) return fail(ctx, DVO_EINVAL, "feat_cap out of range (1..65536)");
    HIP_TRY(hipSetDevice(ctx->device));
    return sift_group_detect(ctx, b->d, d_frames, n_frames, frame_stride, stride, feat_cap, d_kps, d_desc, d_counts,
                             ctx->stream, b->nfeatures, &b->retain);
}

namespace {
// getGaussianKernel(n, sigma, CV_32F) as oracle/surf.cpp restates it
std::vector<float> surf_gauss(int n, double sigma) {
    std::vector<float> k(n);
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        k[i] = (float)std::exp(scale2X * x * x);
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
    return k;
}

// resizeHaarPattern (surf.cpp) on the host: offsets in an integral image of row step `step`
void surf_haar(const int src[][5], SurfHaar* dst, int n, int old_size, int new_size, int step) {
    const float ratio = (float)new_size / old_size;
    for (int k = 0; k < n; ++k) {
        const int dx1 = (int)std::nearbyint(ratio * src[k][0]), dy1 = (int)std::nearbyint(ratio * src[k][1]);
        const int dx2 = (int)std::nearbyint(ratio * src[k][2]), dy2 = (int)std::nearbyint(ratio * src[k][3]);
        dst[k].p0 = dy1 * step + dx1;
        dst[k].p1 = dy2 * step + dx1;
        dst[k].p2 = dy1 * step + dx2;
        dst[k].p3 = dy2 * step + dx2;
        dst[k].w = src[k][4] / ((float)(dx2 - dx1) * (dy2 - dy1));
    }
}

// The host tables of a w x h image: the layer geometry in A (w, h, off, size, rows, cols, nori,
// gdesc, kp_cap; pitch, thr and the table pointers are the caller's) and the three device tables'
// contents.  What surf_plan and the group detector's scratch (surf_group_alloc) both start from.
struct SurfTables {
    std::vector<SurfHaar> haar;
    std::vector<int8_t> apt;
    std::vector<float> aptw;
    int64_t cells = 0;  // floats of det (and of trace): all 20 layers
};
SurfTables surf_tables(int w, int h, SurfLayout& A) {
    SurfTables T;
    A.w = w;
    A.h = h;
    const int sw = w + 1;
    static const int dx_s[3][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1}};
    static const int dy_s[3][5] = {{2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1}};
    static const int dxy_s[4][5] = {{1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};
    std::vector<SurfHaar>& haar = T.haar;
    haar.resize((size_t)kSurfTot * 10);
    int64_t cells = 0;
    for (int o = 0; o < kSurfOct; ++o) {
        const int step = 1 << o;
        A.rows[o] = h / step;
        A.cols[o] = w / step;
        for (int l = 0; l < kSurfLayers; ++l) {
            const int L = o * kSurfLayers + l;
            A.size[L] = (9 + 6 * l) << o;
            A.off[L] = cells;
            cells += (int64_t)A.rows[o] * A.cols[o];
            surf_haar(dx_s, &haar[L * 10], 3, 9, A.size[L], sw);
            surf_haar(dy_s, &haar[L * 10 + 3], 3, 9, A.size[L], sw);
            surf_haar(dxy_s, &haar[L * 10 + 6], 4, 9, A.size[L], sw);
        }
    }
    // SURF_ORI_SIGMA 2.5f, SURF_DESC_SIGMA 3.3f: float constants widened to double
    const std::vector<float> go = surf_gauss(13, (double)2.5f), gd = surf_gauss(20, (double)3.3f);
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j)
            if (i * i + j * j <= 36) {
                T.apt.push_back((int8_t)i);
                T.apt.push_back((int8_t)j);
                T.aptw.push_back(go[i + 6] * go[j + 6]);
            }
    A.nori = (int)T.aptw.size();
    for (int i = 0; i < 20; ++i) A.gdesc[i] = gd[i];
    A.kp_cap = surf_kp_cap(w, h);
    T.cells = cells;
    return T;
}

int surf_order_n(int kp_cap) {  // the sort scratch: the next power of two >= kp_cap
    int order_n = 1;
    while (order_n < kp_cap) order_n <<= 1;
    return order_n;
}

int surf_plan(dvo_ctx* ctx, int w, int h) {
    SurfPlanDev& P = ctx->surf;
    if (P.w == w && P.h == h) return DVO_OK;
    P = SurfPlanDev{};
    SurfArgs& A = P.a;
    A.pitch = (w + 255) & ~255;
    const int sw = w + 1;
    const SurfTables T = surf_tables(w, h, A);
    const std::vector<SurfHaar>& haar = T.haar;
    const std::vector<int8_t>& apt = T.apt;
    const std::vector<float>& aptw = T.aptw;
    const int64_t cells = T.cells;
    const int order_n = surf_order_n(A.kp_cap);
    auto A_ = [&](auto*& p, size_t bytes) { return P.mem.alloc(&p, bytes ? bytes : 16) == hipSuccess; };
    int* counters = nullptr;
    SurfHaar* d_haar = nullptr;
    int8_t* d_apt = nullptr;
    float* d_aptw = nullptr;
    if (!A_(A.sum, (size_t)sw * (h + 1) * 4) || !A_(A.det, (size_t)cells * 4) || !A_(A.trace, (size_t)cells * 4) ||
        !A_(A.raw, (size_t)A.kp_cap * sizeof(dvo_keypoint)) || !A_(A.order, (size_t)order_n * 4) ||
        !A_(A.kps, (size_t)A.kp_cap * sizeof(dvo_keypoint)) || !A_(A.dtmp, (size_t)A.kp_cap * 64 * 4) ||
        !A_(A.out, (size_t)A.kp_cap * sizeof(dvo_keypoint)) || !A_(A.desc, (size_t)A.kp_cap * 64 * 4) ||
        !A_(counters, 64) || !A_(d_haar, haar.size() * sizeof(SurfHaar)) || !A_(d_apt, apt.size()) ||
        !A_(d_aptw, aptw.size() * 4) || !A_(P.img, (size_t)A.pitch * h)) {
        P = SurfPlanDev{};
        return fail(ctx, DVO_EHIP, "SURF buffers: hipMalloc failed");
    }
    A.nraw = counters;
    A.nout = counters + 1;
    A.flags = counters + 2;
    A.haar = d_haar;
    A.apt = d_apt;
    A.aptw = d_aptw;
    A.img = P.img;
    if (hipMemcpy(d_haar, haar.data(), haar.size() * sizeof(SurfHaar), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_apt, apt.data(), apt.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_aptw, aptw.data(), aptw.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(ctx, DVO_EHIP, "SURF tables upload failed");
    P.w = w;
    P.h = h;
    return DVO_OK;
}

// One frame's share of a group's scratch, array by array (bytes), and the tables the group shares.
struct SurfGroupBytes {
    int64_t sum, cells, raw, kps, dtmp, order, counters, tables;
    int64_t frame() const { return sum + cells + raw + kps + dtmp + order + counters; }
};
SurfGroupBytes surf_group_bytes(int w, int h) {
    const int64_t kp_cap = surf_kp_cap(w, h);
    int64_t cells = 0;
    for (int o = 0; o < kSurfOct; ++o) cells += (int64_t)kSurfLayers * (h >> o) * (w >> o);
    SurfGroupBytes b;
    b.sum = (int64_t)4 * (w + 1) * (h + 1);
    b.cells = 8 * cells;  // det and trace
    b.raw = kp_cap * (int64_t)sizeof(dvo_keypoint);
    b.kps = b.raw;
    b.dtmp = kp_cap * 64 * 4;
    b.order = (int64_t)surf_order_n((int)kp_cap) * 4;
    b.counters = 16;
    b.tables = (int64_t)kSurfTot * 10 * (int64_t)sizeof(SurfHaar) + 113 * 2 + 113 * 4;
    return b;
}

constexpr int kSurfGroupMax = 64;

// Allocates a group's whole scratch and uploads the tables, after waiting for the context's stream
// (nothing is allocated later, inside a detect / process call).  D is empty on failure.
int surf_group_alloc(dvo_ctx* ctx, int w, int h, int group, SurfGroupDev& D) {
    D = SurfGroupDev{};
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    SurfGroupArgs& g = D.g;
    const SurfTables T = surf_tables(w, h, g.l);
    const SurfGroupBytes b = surf_group_bytes(w, h);
    const int64_t G = group;
    int* counters = nullptr;
    SurfHaar* d_haar = nullptr;
    int8_t* d_apt = nullptr;
    float* d_aptw = nullptr;
    hipError_t e = hipSuccess;
    auto A_ = [&](auto*& p, int64_t bytes) {
        if (e == hipSuccess) e = D.mem.alloc(&p, (size_t)bytes);
    };
    A_(g.b.sum, G * b.sum);
    A_(g.b.det, G * b.cells);  // frame f: its det, then its trace (one clear covers a chunk's both)
    A_(g.b.raw, G * b.raw);
    A_(g.b.kps, G * b.kps);
    A_(g.b.dtmp, G * b.dtmp);
    A_(g.b.order, G * b.order);
    A_(counters, G * b.counters);
    A_(d_haar, (int64_t)(T.haar.size() * sizeof(SurfHaar)));
    A_(d_apt, (int64_t)T.apt.size());
    A_(d_aptw, (int64_t)T.aptw.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_haar, T.haar.data(), T.haar.size() * sizeof(SurfHaar), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_apt, T.apt.data(), T.apt.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_aptw, T.aptw.data(), T.aptw.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        D = SurfGroupDev{};
        return fail(ctx, DVO_EHIP, std::string("SURF group buffers: ") + hipGetErrorString(e));
    }
    g.b.trace = g.b.det + T.cells;
    g.b.nraw = counters;
    g.b.nout = counters + 1;
    g.b.flags = counters + 2;
    g.l.haar = d_haar;
    g.l.apt = d_apt;
    g.l.aptw = d_aptw;
    g.sum_stride = b.sum / 4;
    g.cell_stride = 2 * T.cells;
    g.order_stride = b.order / 4;
    // DVO_SURF_LARGE_FIRST=0 (read here, when the scratch is made) keeps describe's plain stride over
    // each frame's list: the A/B of tools/time_surf_batch.py.  The results are the same either way.
    const char* lf = std::getenv("DVO_SURF_LARGE_FIRST");
    g.large_first = !(lf && lf[0] == '0');
    D.w = w;
    D.h = h;
    D.group = group;
    return DVO_OK;
}

// n frames through the group detector, in chunks of D.group on stream s: frame f's keypoints and
// descriptors go to kps + f * feat_cap and desc + f * feat_cap * 64, its (count, flags) to counts + 2 f.
int surf_group_detect(dvo_ctx* ctx, const SurfGroupDev& D, const uint8_t* d_frames, int n, int64_t frame_stride, int stride,
                      double hessian_threshold, int feat_cap, dvo_keypoint* kps, float* desc, int32_t* counts,
                      hipStream_t s) {
    for (int f0 = 0; f0 < n; f0 += D.group) {
        const int frames = std::min(D.group, n - f0);
        SurfGroupArgs g = D.g;
        g.l.pitch = stride;
        g.l.thr = (float)hessian_threshold;
        g.b.img = d_frames + (int64_t)f0 * frame_stride;
        g.frame_stride = frame_stride;
        g.out_kps = kps + (size_t)f0 * feat_cap;
        g.out_desc = desc + (size_t)f0 * feat_cap * 64;
        g.out_n = counts + 2 * (size_t)f0;
        g.feat_cap = feat_cap;
        HIP_TRY(hipMemsetAsync(g.b.nraw, 0, (size_t)frames * 16, s));  // the chunk's counters
        HIP_TRY(hipMemsetAsync(g.b.det, 0, (size_t)frames * (size_t)g.cell_stride * 4, s));  // its det and trace
        HIP_TRY(launch_surf_group(g, frames, s));
    }
    return DVO_OK;
}
}  // namespace

struct dvo_surf_batch {
    dvo_ctx* ctx = nullptr;
    SurfGroupDev d;
};

int64_t dvo_surf_batch_bytes(int w, int h, int group) {
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW || group < 1 || group > kSurfGroupMax) return DVO_EINVAL;
    const SurfGroupBytes b = surf_group_bytes(w, h);
    return group * b.frame() + b.tables;
}

int dvo_surf_batch_create(dvo_ctx* ctx, int w, int h, int group, dvo_surf_batch** out) {
    if (!ctx || !out) return DVO_EINVAL;
    *out = nullptr;
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW) return fail(ctx, DVO_EINVAL, "image size out of range (1..4095)");
    if (group < 1 || group > kSurfGroupMax) return fail(ctx, DVO_EINVAL, "group out of range (1..64)");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvo_surf_batch> b(new dvo_surf_batch);
    b->ctx = ctx;
    const int rc = surf_group_alloc(ctx, w, h, group, b->d);
    if (rc) return rc;
    *out = b.release();
    return DVO_OK;
}

void dvo_surf_batch_destroy(dvo_surf_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    delete b;
}

void* dvo_surf_batch_hip_stream(dvo_surf_batch* b) { return b ? (void*)b->ctx->stream : nullptr; }

int dvo_surf_batch_detect(dvo_surf_batch* b, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          double hessian_threshold, int feat_cap, dvo_keypoint* d_kps, float* d_desc, int32_t* d_counts) {
    if (!b) return DVO_EINVAL;
    dvo_ctx* ctx = b->ctx;
    if (n_frames < 1) return fail(ctx, DVO_EINVAL, "n_frames must be >= 1");
    if (!d_frames || !d_kps || !d_desc || !d_counts || stride < b->d.w)
        return fail(ctx, DVO_EINVAL, "bad frame or output buffer");
    if (feat_cap < 1 || feat_cap > surf_kp_cap(b->d.w, b->d.h))
        return fail(ctx, DVO_EINVAL, "feat_cap out of range (1..the detector's list capacity)");
    if (!(hessian_threshold >= 0)) return fail(ctx, DVO_EINVAL, "hessianThreshold must be >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    return surf_group_detect(ctx, b->d, d_frames, n_frames, frame_stride, stride, hessian_threshold, feat_cap, d_kps,
                             d_desc, d_counts, ctx->stream);
}

int dvo_surf_detect_and_compute(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, double hessian_threshold,
                                dvo_keypoint* kps, float* desc, int cap, int* n_out) {
    if (!ctx || !n_out) return DVO_EINVAL;
    *n_out = 0;
    if (!img || stride < w) return fail(ctx, DVO_EINVAL, "bad image buffer");
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW) return fail(ctx, DVO_EINVAL, "image size out of range (1..4095)");
    if (!(hessian_threshold >= 0)) return fail(ctx, DVO_EINVAL, "hessianThreshold must be >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = surf_plan(ctx, w, h);
    if (rc) return rc;
    SurfPlanDev& P = ctx->surf;
    P.a.thr = (float)hessian_threshold;
    HIP_TRY(hipMemsetAsync(P.a.nraw, 0, 16, ctx->stream));
    const int64_t cells = P.a.off[kSurfTot - 1] + (int64_t)P.a.rows[kSurfOct - 1] * P.a.cols[kSurfOct - 1];
    HIP_TRY(hipMemsetAsync(P.a.det, 0, (size_t)cells * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(P.a.trace, 0, (size_t)cells * 4, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(P.img, P.a.pitch, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_surf(P.a, ctx->stream));
    int cnt[3];
    HIP_TRY(hipMemcpyAsync(cnt, P.a.nraw, 12, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cnt[2]) return fail(ctx, DVO_ECAP, "SURF: more keypoints than the device lists hold");
    const int n = cnt[1];
    *n_out = n;
    if (n > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (n) {
        if (kps) HIP_TRY(hipMemcpyAsync(kps, P.a.out, (size_t)n * sizeof(dvo_keypoint), hipMemcpyDeviceToHost, ctx->stream));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, P.a.desc, (size_t)n * 64 * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return DVO_OK;
}

int dvo_sift_detect_and_compute(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, dvo_keypoint* kps,
                                float* desc, int cap, int* n_out) {
    return dvo_sift_detect_and_compute_n(ctx, img, w, h, stride, 0, kps, desc, cap, n_out);
}

int dvo_sift_detect_and_compute_n(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, int nfeatures,
                                  dvo_keypoint* kps, float* desc, int cap, int* n_out) {
    if (!ctx || !n_out) return DVO_EINVAL;
    *n_out = 0;
    if (nfeatures < 0) return fail(ctx, DVO_EINVAL, "nfeatures must be >= 0");
    if (!img || stride < w) return fail(ctx, DVO_EINVAL, "bad image buffer");
    if (w < 1 || h < 1 || w >= kMaxW || h >= kMaxW) return fail(ctx, DVO_EINVAL, "image size out of range (1..4095)");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = sift_plan(ctx, w, h);
    if (rc) return rc;
    SiftPlanDev& P = ctx->sift;
    SiftRetainArgs ra{};
    if (nfeatures > 0) {  // a synchronous call: the scratch is made here, once, before anything is launched
        if ((rc = sift_retain_ensure(ctx, ctx->sift_retain, 1))) return rc;
        ra = ctx->sift_retain.a;
        ra.nfeatures = nfeatures;
    }
    HIP_TRY(hipMemsetAsync(P.a.ncand, 0, 16, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(P.img, P.pitch, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_sift(P.a, P.img, w, h, P.pitch, P.taps, P.tap_off, P.tap_n, ctx->stream, nfeatures > 0 ? &ra : nullptr));
    int cnt[4];
    HIP_TRY(hipMemcpyAsync(cnt, P.a.ncand, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cnt[3]) return fail(ctx, DVO_ECAP, "SIFT: more extrema / keypoints than the device lists hold");
    const int n = cnt[2];
    *n_out = n;
    if (n > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (n) {
        if (kps) HIP_TRY(hipMemcpyAsync(kps, P.a.kps, (size_t)n * sizeof(dvo_keypoint), hipMemcpyDeviceToHost, ctx->stream));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, P.a.desc, (size_t)n * 128 * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return DVO_OK;
}

// The correspondences as the geometry kernels read them: [m][4] (x1, y1, x2, y2), on the device.
static int upload_points(dvo_ctx* ctx, CallMem& mem, const double* p1, const double* p2, int m, const double** dpts) {
    double* d = mem.dev<double>((size_t)m * 4);
    double* h = reinterpret_cast<double*>(mem.host((size_t)m * 32));
    HIP_TRY(mem.error());
    for (int i = 0; i < m; ++i) {
        h[4 * i] = p1[2 * i];
        h[4 * i + 1] = p1[2 * i + 1];
        h[4 * i + 2] = p2[2 * i];
        h[4 * i + 3] = p2[2 * i + 1];
    }
    HIP_TRY(mem.send(d, reinterpret_cast<const uint8_t*>(h), (size_t)m * 32));
    *dpts = d;
    return DVO_OK;
}

int dvo_find_essential_mat(dvo_ctx* ctx, const double* p1, const double* p2, int m, const double* K, double prob,
                           double threshold, int max_iters, double* E, int* e_rows, uint8_t* mask) {
    if (!ctx || !K || !E || !e_rows) return DVO_EINVAL;
    *e_rows = 0;
    if (m < 0 || (m > 0 && (!p1 || !p2))) return fail(ctx, DVO_EINVAL, "bad point arrays");
    if (!(prob > 0 && prob < 1)) return fail(ctx, DVO_EINVAL, "prob must be in (0, 1)");
    if (!(threshold > 0) || !std::isfinite(threshold)) return fail(ctx, DVO_EINVAL, "threshold must be finite and > 0");
    if (max_iters < 1) return fail(ctx, DVO_EINVAL, "max_iters must be >= 1");
    if (m < 5) return fail(ctx, DVO_EFEWPTS, "fewer than 5 correspondences");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t hc = (size_t)(max_iters > 1 ? max_iters : 1);
    CallMem mem(ctx->call, ctx->stream);
    GeomArgs g{};
    g.m_const = m;
    g.pts_stride = m;
    set_camera(g, K);
    g.prob = prob;
    g.threshold = threshold;
    g.max_iters = max_iters;
    call_geometry(g, mem, kGeomRansac, 1, (size_t)m, hc);
    g.mask = mem.dev<uint8_t>(m);
    int rc = upload_points(ctx, mem, p1, p2, m, &g.pts_d);
    if (rc) return rc;
    HIP_TRY(launch_geometry_args(g, 1, kStageNormalize | kStageRansac | kStageOneRound, ctx->stream));
    uint8_t *hinfo, *hE, *hmask = nullptr;
    HIP_TRY(mem.get(g.info, 16, &hinfo));
    HIP_TRY(mem.get(g.E, 90 * 8, &hE));  // every row the kernel may write (<= 10 models)
    if (mask) HIP_TRY(mem.get(g.mask, (size_t)m, &hmask));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int info[4];
    std::memcpy(info, hinfo, sizeof(info));
    if (info[3] != DVO_OK) return fail(ctx, info[3], "findEssentialMat: no model (E is empty)");
    *e_rows = info[0];
    std::memcpy(E, hE, sizeof(double) * 3 * info[0]);
    if (mask) std::memcpy(mask, hmask, (size_t)m);
    return DVO_OK;
}

int dvo_recover_pose(dvo_ctx* ctx, const double* E, int e_rows, const double* p1, const double* p2, int m,
                     const double* K, double dist_thresh, const uint8_t* mask_in, double* R, double* t,
                     uint8_t* mask_out, int* good) {
    if (!ctx || !E || !K || !R || !t || !good) return DVO_EINVAL;
    if (e_rows != 3) return fail(ctx, DVO_EINVAL, "recoverPose: E must be 3x3 (decomposeEssentialMat reshape)");
    if (m < 0 || (m > 0 && (!p1 || !p2))) return fail(ctx, DVO_EINVAL, "bad point arrays");
    if (!std::isfinite(dist_thresh)) return fail(ctx, DVO_EINVAL, "distanceThresh must be finite");
    HIP_TRY(hipSetDevice(ctx->device));
    const int mm = m > 0 ? m : 1;
    CallMem mem(ctx->call, ctx->stream);
    GeomArgs g{};
    g.m_const = m;
    g.pts_stride = mm;
    set_camera(g, K);
    g.dist_thresh = dist_thresh;
    call_geometry(g, mem, kGeomPose, 1, (size_t)mm, 0);
    // no RANSAC here: of that group only the normalised points, and E and info as inputs; and what
    // only this entry point has: the chosen decomposition, the four masks, the caller's mask
    g.npts = mem.dev<double>((size_t)mm * 4);
    g.E = mem.dev<double>(90);
    g.info = mem.dev<int32_t>(4);
    g.pick = mem.dev<int32_t>(2);
    g.pose_mask = mem.dev<uint8_t>((size_t)mm * 4);
    uint8_t* dmin = mask_in ? mem.dev<uint8_t>(mm) : nullptr;
    g.mask_in = dmin;
    int rc = upload_points(ctx, mem, p1, p2, m, &g.pts_d);
    if (rc) return rc;
    if (mask_in) HIP_TRY(mem.put(dmin, mask_in, (size_t)m));
    const int info[4] = {3, 0, 0, DVO_OK};
    HIP_TRY(mem.put(g.E, E, 9 * sizeof(double)));
    HIP_TRY(mem.put(g.info, info, sizeof(info)));
    HIP_TRY(launch_geometry_args(g, 1, kStageNormalize | kStagePose, ctx->stream));
    uint8_t *hRt, *hgood, *hpick, *hpm = nullptr;
    HIP_TRY(mem.get(g.Rt, 12 * sizeof(double), &hRt));
    HIP_TRY(mem.get(g.good, sizeof(int), &hgood));
    HIP_TRY(mem.get(g.pick, sizeof(int), &hpick));
    if (mask_out && m > 0) HIP_TRY(mem.get(g.pose_mask, (size_t)m * 4, &hpm));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(R, hRt, 9 * sizeof(double));
    std::memcpy(t, hRt + 9 * sizeof(double), 3 * sizeof(double));
    int pick = 0;
    std::memcpy(good, hgood, sizeof(int));
    std::memcpy(&pick, hpick, sizeof(int));
    if (hpm)
        for (int i = 0; i < m; ++i) mask_out[i] = hpm[(size_t)i * 4 + pick];
    return DVO_OK;
}

int dvo_triangulate_points(dvo_ctx* ctx, const double* P1, const double* P2, const double* x1, const double* x2,
                           int k, double* X) {
    if (!ctx || !P1 || !P2 || !X || k < 0 || (k > 0 && (!x1 || !x2))) return DVO_EINVAL;
    if (k == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    double* dP = mem.dev<double>(24);
    double* dx = mem.dev<double>((size_t)k * 4);
    double* dX = mem.dev<double>((size_t)k * 4);
    uint8_t* hP = mem.host(24 * 8);
    uint8_t* hx = mem.host((size_t)k * 32);
    HIP_TRY(mem.error());
    std::memcpy(hP, P1, 12 * sizeof(double));
    std::memcpy(hP + 12 * sizeof(double), P2, 12 * sizeof(double));
    HIP_TRY(mem.send(dP, hP, 24 * 8));
    std::memcpy(hx, x1, (size_t)k * 16);
    std::memcpy(hx + (size_t)k * 16, x2, (size_t)k * 16);
    HIP_TRY(mem.send(dx, hx, (size_t)k * 32));
    HIP_TRY(launch_triangulate(dP, dx, k, dX, ctx->stream));
    uint8_t* hX;
    HIP_TRY(mem.get(dX, (size_t)k * 32, &hX));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(X, hX, (size_t)k * 32);
    return DVO_OK;
}

// ---------------------------------------------------------------------------
// The k-NN modes' pair path (knn_sift, surf, flann): detectAndCompute (v3:373), knnMatch(k = 2)
// (v3:204, :212, :215), the ratio test and keypoint gather (v3:223-238, :355, :358),
// findEssentialMat (v3:297) and recoverPose (v3:303) of one pair of host frames in one call.
struct dvo_knn_pair {
    dvo_ctx* ctx = nullptr;
    dvo_knn_pair_config cfg{};
    int dim = 0, kp_cap = 0, cus = 0;
    int nfeatures = 0;  // dvo_knn_pair_set_nfeatures (SIFT): retainBest on the context's retain scratch
    struct Slot {  // one frame's features on the device
        dvo_keypoint* kps = nullptr;
        float* desc = nullptr;
        int32_t* n = nullptr;  // device: count, detector overflow flags
        int count = 0;         // the count, once read
    };
    Slot slot[2];
    int prev = 0, cur = 1;      // the slots of the last pair's previous and current frame
    bool cache_valid = false;   // slot[cur] may serve as the next pair's previous frame
    bool have_pair = false;     // the slots and the match list describe the last call's pair
    int last_m = 0;
    float* pts = nullptr;            // [kp_cap][4]
    dvo_dmatch* matches = nullptr;   // [kp_cap]
    int32_t* words = nullptr;        // nmatch, missing-second-neighbour flag
    PairHeader* hdr = nullptr;
    dvo_pair_record* rec = nullptr;
    DeviceAllocs mem;
};

namespace {
int check_knn_pair_config(dvo_ctx* ctx, const dvo_knn_pair_config* c) {
    if (c->width < 1 || c->height < 1 || c->width >= kMaxW || c->height >= kMaxW)
        return fail(ctx, DVO_EINVAL, "image size out of range (1..4095)");
    if (c->detector != DVO_DETECT_SIFT && c->detector != DVO_DETECT_SURF)
        return fail(ctx, DVO_EINVAL, "detector must be DVO_DETECT_SIFT or DVO_DETECT_SURF");
    if (c->matcher != DVO_MATCH_BF_L1 && c->matcher != DVO_MATCH_FLANN)
        return fail(ctx, DVO_EINVAL, "matcher must be DVO_MATCH_BF_L1 or DVO_MATCH_FLANN");
    if (c->detector == DVO_DETECT_SURF && !(c->hessian_threshold >= 0))
        return fail(ctx, DVO_EINVAL, "hessianThreshold must be >= 0");
    if (c->matcher == DVO_MATCH_FLANN && (c->trees < 1 || c->trees > 64 || c->checks < 1))
        return fail(ctx, DVO_EINVAL, "trees 1..64 and checks >= 1");
    if (!std::isfinite(c->ratio) || !(c->ratio > 0)) return fail(ctx, DVO_EINVAL, "ratio must be finite and > 0");
    if (!(c->prob > 0 && c->prob < 1)) return fail(ctx, DVO_EINVAL, "prob must be in (0, 1)");
    if (!(c->threshold > 0) || !std::isfinite(c->threshold))
        return fail(ctx, DVO_EINVAL, "threshold must be finite and > 0");
    if (c->max_iters < 1) return fail(ctx, DVO_EINVAL, "max_iters must be >= 1");
    if (!std::isfinite(c->dist_thresh)) return fail(ctx, DVO_EINVAL, "distanceThresh must be finite");
    return DVO_OK;
}

int knn_pair_plan(dvo_knn_pair* p) {
    return p->cfg.detector == DVO_DETECT_SIFT ? sift_plan(p->ctx, p->cfg.width, p->cfg.height)
                                              : surf_plan(p->ctx, p->cfg.width, p->cfg.height);
}
}  // namespace

int dvo_knn_pair_create(dvo_ctx* ctx, const dvo_knn_pair_config* cfg, dvo_knn_pair** out) {
    if (!ctx || !cfg || !out) return DVO_EINVAL;
    *out = nullptr;
    int rc = check_knn_pair_config(ctx, cfg);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvo_knn_pair> p(new dvo_knn_pair);
    p->ctx = ctx;
    p->cfg = *cfg;
    HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    if ((rc = knn_pair_plan(p.get()))) return rc;  // the context's detector plan sets the list capacity
    const bool sift = cfg->detector == DVO_DETECT_SIFT;
    p->dim = sift ? 128 : 64;
    p->kp_cap = sift ? ctx->sift.a.kp_cap : ctx->surf.a.kp_cap;
    const size_t kc = (size_t)p->kp_cap;
    for (auto& sl : p->slot) {
        HIP_TRY(p->mem.alloc(&sl.kps, kc * sizeof(dvo_keypoint)));
        HIP_TRY(p->mem.alloc(&sl.desc, kc * p->dim * sizeof(float)));
        HIP_TRY(p->mem.alloc(&sl.n, 2 * sizeof(int32_t)));
    }
    HIP_TRY(p->mem.alloc(&p->pts, kc * 4 * sizeof(float)));
    HIP_TRY(p->mem.alloc(&p->matches, kc * sizeof(dvo_dmatch)));
    HIP_TRY(p->mem.alloc(&p->words, 2 * sizeof(int32_t)));
    HIP_TRY(p->mem.alloc(&p->hdr, sizeof(PairHeader)));
    HIP_TRY(p->mem.alloc(&p->rec, sizeof(dvo_pair_record)));
    *out = p.release();
    return DVO_OK;
}

int dvo_knn_pair_set_nfeatures(dvo_knn_pair* p, int nfeatures) {
    if (!p) return DVO_EINVAL;
    dvo_ctx* ctx = p->ctx;
    if (p->cfg.detector != DVO_DETECT_SIFT)
        return fail(ctx, DVO_EINVAL, "nfeatures is SIFT's: OpenCV's SURF_create has no such parameter");
    if (nfeatures < 0) return fail(ctx, DVO_EINVAL, "nfeatures must be >= 0");
    if (nfeatures == p->nfeatures) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nfeatures > 0) {
        const int rc = sift_retain_ensure(ctx, ctx->sift_retain, 1);
        if (rc) return rc;
    }
    p->nfeatures = nfeatures;
    p->cache_valid = false;  // the cached previous-frame features were retained under the old value
    return DVO_OK;
}

void dvo_knn_pair_destroy(dvo_knn_pair* p) {
    if (!p) return;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    delete p;
}

int dvo_knn_pair_run(dvo_knn_pair* p, const uint8_t* prev_img, const uint8_t* cur_img, int stride, int reuse_prev,
                     uint64_t* rng_state, dvo_pair_record* rec_out) {
    if (!p) return DVO_EINVAL;
    dvo_ctx* ctx = p->ctx;
    const dvo_knn_pair_config& c = p->cfg;
    const int w = c.width, h = c.height;
    const bool sift = c.detector == DVO_DETECT_SIFT, flann = c.matcher == DVO_MATCH_FLANN;
    if (!cur_img || !rec_out || stride < w || (!reuse_prev && !prev_img)) return fail(ctx, DVO_EINVAL, "bad image buffer");
    if (flann && !rng_state) return fail(ctx, DVO_EINVAL, "null theRNG state");
    if (reuse_prev && !p->cache_valid)
        return fail(ctx, DVO_EINVAL, "reuse_prev needs a preceding dvo_knn_pair_run that succeeded");
    // the slots swap roles: the last pair's current frame is this pair's previous one
    const int sp = reuse_prev ? p->cur : 0, sc = 1 - sp;
    p->cache_valid = false;
    p->have_pair = false;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = knn_pair_plan(p);  // another size may have taken the context's plan since
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    CallMem mem(ctx->call, s);
    dvo_knn_pair::Slot &P = p->slot[sp], &C = p->slot[sc];
    // host frames go up through pinned staging; the detection's n features go device to device into the slot
    auto detect = [&](const uint8_t* img, dvo_knn_pair::Slot& sl) -> int {
        uint8_t* hp = mem.host((size_t)w * h);
        HIP_TRY(mem.error());
        for (int y = 0; y < h; ++y) std::memcpy(hp + (size_t)y * w, img + (size_t)y * stride, w);
        if (sift) {
            SiftPlanDev& D = ctx->sift;
            HIP_TRY(hipMemsetAsync(D.a.ncand, 0, 16, s));
            HIP_TRY(hipMemcpy2DAsync(D.img, D.pitch, hp, w, w, h, hipMemcpyHostToDevice, s));
            if (p->nfeatures > 0 && ctx->sift_retain.frames < 1) return fail(ctx, DVO_EINVAL, "SIFT retain scratch is missing");
            SiftRetainArgs ra = ctx->sift_retain.a;
            ra.nfeatures = p->nfeatures;
            HIP_TRY(launch_sift(D.a, D.img, w, h, D.pitch, D.taps, D.tap_off, D.tap_n, s, p->nfeatures > 0 ? &ra : nullptr));
            HIP_TRY(launch_feature_copy(D.a.kps, D.a.desc, D.a.nkp, D.a.flags, p->kp_cap, 128, sl.kps, sl.desc, sl.n, s));
        } else {
            SurfPlanDev& D = ctx->surf;
            D.a.thr = (float)c.hessian_threshold;
            HIP_TRY(hipMemsetAsync(D.a.nraw, 0, 16, s));
            const int64_t cells = D.a.off[kSurfTot - 1] + (int64_t)D.a.rows[kSurfOct - 1] * D.a.cols[kSurfOct - 1];
            HIP_TRY(hipMemsetAsync(D.a.det, 0, (size_t)cells * 4, s));
            HIP_TRY(hipMemsetAsync(D.a.trace, 0, (size_t)cells * 4, s));
            HIP_TRY(hipMemcpy2DAsync(D.img, D.a.pitch, hp, w, w, h, hipMemcpyHostToDevice, s));
            HIP_TRY(launch_surf(D.a, s));
            HIP_TRY(launch_feature_copy(D.a.out, D.a.desc, D.a.nout, D.a.flags, p->kp_cap, 64, sl.kps, sl.desc, sl.n, s));
        }
        return DVO_OK;
    };
    int m_kept = 0;
    // after the first upload an error drains the stream before returning: its DMAs read the context's
    // pinned buffers, which the next per-call entry point rewrites
    auto body = [&]() -> int {
        if (!reuse_prev && (rc = detect(prev_img, P))) return rc;
        if ((rc = detect(cur_img, C))) return rc;
        uint8_t *hnp = nullptr, *hnc = nullptr;
        if (!reuse_prev) HIP_TRY(mem.get(P.n, 8, &hnp));
        HIP_TRY(mem.get(C.n, 8, &hnc));
        HIP_TRY(hipStreamSynchronize(s));
        int32_t np2[2] = {P.count, 0}, nc2[2];
        if (hnp) std::memcpy(np2, hnp, 8);
        std::memcpy(nc2, hnc, 8);
        if (np2[1] || nc2[1] || np2[0] > p->kp_cap || nc2[0] > p->kp_cap)
            return fail(ctx, DVO_ECAP, sift ? "SIFT: more extrema / keypoints than the device lists hold"
                                            : "SURF: more keypoints than the device lists hold");
        const int nq = P.count = np2[0], nt = C.count = nc2[0];
        dvo_pair_record r{};
        r.n_kp_prev = nq;
        r.n_kp_cur = nt;
        // no descriptors (knnMatch on None raises, v3:204-215), or one train: `for m, n in matches`
        // cannot unpack (v3:223) / FLANN asserts knn <= index size
        if (nq == 0 || nt < 2) {
            r.status = DVO_ENOFEAT;
            *rec_out = r;
            return DVO_OK;
        }
        int32_t* d_idx = nullptr;
        float* d_dist = nullptr;
        if (flann) {
            if ((rc = flann_knn_device(ctx, mem, P.desc, nq, C.desc, nt, p->dim, 2, c.trees, c.checks, *rng_state, &d_idx,
                                       &d_dist)))
                return rc;
        } else {
            const int ranges = knn_ranges(nq, nt, p->cus);
            const size_t out_n = (size_t)nq * 2, part_n = ranges > 1 ? (size_t)ranges * nq * 2 : 1;
            d_dist = mem.dev<float>(out_n);
            d_idx = mem.dev<int32_t>(out_n);
            float* bpd = mem.dev<float>(part_n);
            int32_t* bpi = mem.dev<int32_t>(part_n);
            uint8_t* bb = mem.dev<uint8_t>(knn_bytes_size(nq, nt, p->dim));
            HIP_TRY(mem.error());
            HIP_TRY(launch_knn_float(P.desc, nq, C.desc, nt, p->dim, 2, DVO_NORM_L1, ranges, bb, bpd, bpi, d_dist, d_idx, s));
        }
        RatioArgs ra{d_idx, d_dist, P.kps, C.kps, nq, nq, nt, c.ratio, flann ? 1 : 0, p->pts, p->matches, p->words,
                     p->hdr, p->words + 1};
        HIP_TRY(launch_ratio_gather(ra, s));
        // findEssentialMat and recoverPose as the per-call operators run them, on the kernel's count
        const size_t hc = (size_t)c.max_iters;
        GeomArgs g{};
        g.pts_f = p->pts;
        g.m_arr = p->words;
        g.pts_stride = nq;
        set_camera(g, c.K);
        g.prob = c.prob;
        g.threshold = c.threshold;
        g.max_iters = c.max_iters;
        g.dist_thresh = c.dist_thresh;
        call_geometry(g, mem, kGeomRansac | kGeomPose, 1, (size_t)nq, hc);
        HIP_TRY(mem.error());
        HIP_TRY(launch_geometry_args(g, 1, kStageNormalize | kStageRansac | kStageOneRound, s));
        HIP_TRY(launch_retire(g, 1, p->hdr, p->rec, s));  // kStagePose and the record
        uint8_t *hr = nullptr, *hw = nullptr;
        HIP_TRY(mem.get(p->rec, sizeof(dvo_pair_record), &hr));
        HIP_TRY(mem.get(p->words, 8, &hw));
        HIP_TRY(hipStreamSynchronize(s));
        int32_t words[2];
        std::memcpy(&r, hr, sizeof(r));
        std::memcpy(words, hw, 8);
        // a query without a second neighbour (FLANN's approximate search only): `for m, n in matches` raises
        if (words[1]) r.status = DVO_ENOFEAT;
        m_kept = words[0];
        *rec_out = r;
        if (flann) *rng_state = flann_rng_after(*rng_state, c.trees, nt);
        return DVO_OK;
    };
    if ((rc = body())) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    p->prev = sp;
    p->cur = sc;
    p->last_m = m_kept;
    p->have_pair = true;
    // the current frame's features serve the next pair only after a pair that got through: a failing
    // pair (a status in the record, or an error) is redone from both frames
    p->cache_valid = rec_out->status == DVO_OK;
    return DVO_OK;
}

int dvo_knn_pair_get_matches(dvo_knn_pair* p, dvo_dmatch* out, int cap, int* m) {
    if (!p || !m) return DVO_EINVAL;
    dvo_ctx* ctx = p->ctx;
    *m = 0;
    if (!p->have_pair) return fail(ctx, DVO_EINVAL, "no pair has run");
    *m = p->last_m;
    if (p->last_m > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (p->last_m == 0) return DVO_OK;
    if (!out) return fail(ctx, DVO_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, p->matches, (size_t)p->last_m * sizeof(dvo_dmatch), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_knn_pair_get_features(dvo_knn_pair* p, int which, dvo_keypoint* kps, float* desc, int cap, int* n) {
    if (!p || !n) return DVO_EINVAL;
    dvo_ctx* ctx = p->ctx;
    *n = 0;
    if (which != 0 && which != 1) return fail(ctx, DVO_EINVAL, "which must be 0 (previous) or 1 (current)");
    if (!p->have_pair) return fail(ctx, DVO_EINVAL, "no pair has run");
    const dvo_knn_pair::Slot& sl = p->slot[which ? p->cur : p->prev];
    *n = sl.count;
    if (sl.count > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (sl.count == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (kps) HIP_TRY(hipMemcpyAsync(kps, sl.kps, (size_t)sl.count * sizeof(dvo_keypoint), hipMemcpyDeviceToHost, ctx->stream));
    if (desc) HIP_TRY(hipMemcpyAsync(desc, sl.desc, (size_t)sl.count * p->dim * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

// Test hook: ratio_gather_kernel on host arrays.
int dvo_test_ratio_gather(dvo_ctx* ctx, const int32_t* idx, const float* dist, int nq, const dvo_keypoint* kq, int nkq,
                          const dvo_keypoint* kt, int nkt, double ratio, int squared, float* pts, dvo_dmatch* matches,
                          int* m, int* missing_second) {
    if (!ctx || !m || !missing_second) return DVO_EINVAL;
    *m = 0;
    *missing_second = 0;
    if (nq < 0 || nq > (1 << 20) || nkq < nq || nkt < 0 || nkq > (1 << 20) || nkt > (1 << 20))
        return fail(ctx, DVO_EINVAL, "counts out of range (0 <= nq <= nkq <= 2^20, 0 <= nkt <= 2^20)");
    if (!std::isfinite(ratio) || !(ratio > 0)) return fail(ctx, DVO_EINVAL, "ratio must be finite and > 0");
    if (nq > 0 && (!idx || !dist || !kq || !pts || !matches || (nkt > 0 && !kt))) return fail(ctx, DVO_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    const size_t n1 = (size_t)std::max(nq, 1);
    int32_t* d_idx = mem.dev<int32_t>(n1 * 2);
    float* d_dist = mem.dev<float>(n1 * 2);
    dvo_keypoint* d_kq = mem.dev<dvo_keypoint>((size_t)std::max(nkq, 1));
    dvo_keypoint* d_kt = mem.dev<dvo_keypoint>((size_t)std::max(nkt, 1));
    float* d_pts = mem.dev<float>(n1 * 4);
    dvo_dmatch* d_m = mem.dev<dvo_dmatch>(n1);
    int32_t* d_words = mem.dev<int32_t>(2);
    PairHeader* d_hdr = mem.dev<PairHeader>(1);
    HIP_TRY(mem.error());
    HIP_TRY(mem.put(d_idx, idx, (size_t)nq * 8));
    HIP_TRY(mem.put(d_dist, dist, (size_t)nq * 8));
    HIP_TRY(mem.put(d_kq, kq, (size_t)nkq * sizeof(dvo_keypoint)));
    HIP_TRY(mem.put(d_kt, kt, (size_t)nkt * sizeof(dvo_keypoint)));
    RatioArgs ra{d_idx, d_dist, d_kq, d_kt, nq, nkq, nkt, ratio, squared ? 1 : 0, d_pts, d_m, d_words, d_hdr, d_words + 1};
    HIP_TRY(launch_ratio_gather(ra, ctx->stream));
    uint8_t *hw, *hp, *hm;
    HIP_TRY(mem.get(d_words, 8, &hw));
    HIP_TRY(mem.get(d_pts, (size_t)nq * 16, &hp));
    HIP_TRY(mem.get(d_m, (size_t)nq * sizeof(dvo_dmatch), &hm));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int32_t words[2];
    std::memcpy(words, hw, 8);
    *m = words[0];
    *missing_second = words[1];
    if (words[0] > 0) {
        std::memcpy(pts, hp, (size_t)words[0] * 16);
        std::memcpy(matches, hm, (size_t)words[0] * sizeof(dvo_dmatch));
    }
    return DVO_OK;
}

// ---------------------------------------------------------------------------
// The k-NN modes' batched stream (dvo_knn_stream): dvo_knn_pair_run's path for many device-resident
// frames per call, nothing read back on the way.
extern "C++" {  // KnnBatch has a member template
namespace {
// Frame slots and per-pair match arrays of the batched k-NN path: what dvo_knn_pair_run keeps in
// its two slots and takes from CallMem, for F frames and F - 1 pairs.
struct KnnBatch {
    int F = 0, cap = 0, dim = 0, cus = 0;
    int fixed_ranges = 0;    // > 0: every call runs this many train ranges (the test hook)
    size_t part_lists = 0;   // (pair, range) partial lists pdist / pidx hold
    dvo_keypoint* kps = nullptr;  // [F][cap]
    float* desc = nullptr;        // [F][cap][dim]
    int32_t* n = nullptr;         // [F][2] detector count, flags (feature_copy_kernel)
    int32_t* fstate = nullptr;    // [F][2] features brought to the pairs, marked
    uint32_t* bytes = nullptr;    // SIFT: [F][cap][dim / 4]
    uint32_t* norms = nullptr;    // SIFT: [F][cap]
    int32_t* rejected = nullptr;  // SIFT: [F]
    float* dist = nullptr;        // [P][cap][2]
    int32_t* idx = nullptr;
    float* pdist = nullptr;       // [part_lists][cap][2]
    int32_t* pidx = nullptr;
    dvo_dmatch* matches = nullptr;  // [P][cap]
    int32_t* missing = nullptr;     // [P]

    int ranges_of(int pairs) const { return fixed_ranges > 0 ? fixed_ranges : knn_batch_ranges(cap, pairs, cus); }

    // take(pointer, bytes) per array; false from take stops the walk
    template <class Take>
    bool layout(int F_, int cap_, int dim_, int cus_, int fixed_ranges_, Take&& take) {
        F = F_, cap = cap_, dim = dim_, cus = cus_, fixed_ranges = fixed_ranges_;
        const size_t P = (size_t)std::max(F - 1, 1), C = (size_t)cap;
        part_lists = 0;
        for (int p = 1; p < F; ++p) {
            const size_t r = (size_t)ranges_of(p);
            if (r > 1) part_lists = std::max(part_lists, r * p);
        }
        const size_t L = std::max<size_t>(part_lists, 1);
        bool ok = take(kps, F * C * sizeof(dvo_keypoint)) && take(desc, F * C * dim * 4) && take(n, (size_t)F * 8) &&
                  take(fstate, (size_t)F * 8) && take(dist, P * C * 8) && take(idx, P * C * 8) &&
                  take(pdist, L * C * 8) && take(pidx, L * C * 8) && take(matches, P * C * sizeof(dvo_dmatch)) &&
                  take(missing, P * 4);
        if (ok && dim == 128)  // SURF rows are never byte-valued: neither the pack nor the byte kernel runs
            ok = take(bytes, F * C * dim) && take(norms, F * C * 4) && take(rejected, (size_t)F * 4);
        return ok;
    }

    // Steps 2 to 4 of a call over `frames` slots: frame state, pack + k-NN (+ merge), ratio test and gather.
    // fl (the FLANN mode's scratch): the kd-forests and their search take the k-NN's place, and
    // the lists hold squared L2.
    // state_done: step 2 ran already (dvo_knn_stream_detect).  shard: a sharded FLANN call's hand-off.
    hipError_t match(int frames, double ratio, float* pts, int32_t* nmatch, PairHeader* hdr, hipStream_t s,
                     const FlannBatchArgs* fl = nullptr, int levels = 0, bool state_done = false,
                     const FlannShard* shard = nullptr) const {
        hipError_t e = state_done ? hipSuccess : launch_knn_frame_state(n, frames, cap, fstate, s);
        if (e != hipSuccess || frames < 2) return e;
        if (fl) {
            FlannBatchArgs fa = *fl;
            fa.desc = desc, fa.fstate = fstate, fa.cap = cap, fa.dim = dim, fa.idx = idx, fa.dist = dist;
            e = launch_flann_batch(fa, frames, levels, s, shard);
        } else {
            const KnnBatchArgs ka{desc, fstate, bytes, norms, rejected, cap, dim, dist, idx, pdist, pidx};
            e = launch_knn_batch(ka, frames, ranges_of(frames - 1), s);
        }
        if (e != hipSuccess) return e;
        const RatioBatchArgs ra{idx, dist, kps, n, fstate, cap, ratio, pts, matches, nmatch, hdr, missing, fl ? 1 : 0};
        return launch_ratio_gather_batch(ra, frames - 1, s);
    }
};

constexpr int kKnnStreamMaxFrames = 65536;  // pairs ride a grid's y / z dimension
}  // namespace
}  // extern "C++"

struct dvo_knn_stream {
    dvo_ctx* ctx = nullptr;
    dvo_knn_stream_config cfg{};
    KnnBatch b;
    PairSets pairs;    // one set of max_frames - 1 pairs: pairs.all.g is the stream's GeomArgs
    DeviceAllocs mem;  // the frame slots, the match arrays and the round-local geometry arrays
    SiftGroupDev grp;  // dvo_knn_stream_set_detect_group: grp.group > 0 detects through launch_sift_group
    int nfeatures = 0;     // dvo_knn_stream_set_nfeatures (SIFT): retainBest in either detection route
    SiftRetainDev retain;  // the group route's retain scratch (the frame-by-frame route uses the context's)
    SurfGroupDev sgrp;  // dvo_knn_stream_set_surf_group: sgrp.group > 0 detects through launch_surf_group
    FlannBatchArgs fl{};  // dvo_knn_stream_set_flann: fl.trees > 0 matches through launch_flann_batch
    DeviceAllocs fl_mem;  // its scratch and the theRNG state word
    int last_frames = 0;     // frames whose features the slots hold (dvo_knn_stream_get_features)
    int pending = 0;         // frames detected by dvo_knn_stream_detect and not yet finished
    int matched_frames = 0;  // frames of the last finished call (dvo_knn_stream_get_matches)
    bool pending_timed = false;  // the pending detection recorded ev[0], ev[1]
    bool profiling = false, timed = false;
    bool times_read = false;  // times_ms holds the figures of the last timed call (read once: a later
    double times_ms[3] = {};  // hipEventElapsedTime of the same events may differ in the last digit)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // dvo_knn_stream_set_raw_input: max_frames gray frames of raw_pitch-byte rows, what a colour,
    // distorted or JPEG call detects on
    DeviceAllocs raw_mem;
    uint8_t* raw = nullptr;
    int raw_pitch = 0;
    PairOutputs next;  // dvo_knn_stream_set_landmarks / _tracks / _track_poses / _track_refine / _track_bundle: taken by the next finish
    // A raw-input call records ev_in[k] before its input launch, k the one the last accepted call
    // does not use (first_ev; -1: that call began at ev[0]), so a refused call disturbs no figure.
    hipEvent_t ev_in[2] = {nullptr, nullptr};
    int first_ev = -1;

    ~dvo_knn_stream() {
        for (auto e : {ev[0], ev[1], ev[2], ev[3], ev_in[0], ev_in[1]})
            if (e) hipEventDestroy(e);
    }
};

namespace {
int knn_stream_plan(dvo_knn_stream* s) {
    return s->cfg.detector == DVO_DETECT_SIFT ? sift_plan(s->ctx, s->cfg.width, s->cfg.height)
                                              : surf_plan(s->ctx, s->cfg.width, s->cfg.height);
}
}  // namespace

int dvo_knn_stream_create(dvo_ctx* ctx, const dvo_knn_stream_config* cfg, dvo_knn_stream** out) {
    if (!ctx || !cfg || !out) return DVO_EINVAL;
    *out = nullptr;
    dvo_knn_pair_config pc{};
    pc.width = cfg->width, pc.height = cfg->height;
    pc.detector = cfg->detector, pc.matcher = DVO_MATCH_BF_L1;
    pc.hessian_threshold = cfg->hessian_threshold;
    pc.ratio = cfg->ratio;
    pc.prob = cfg->prob, pc.threshold = cfg->threshold, pc.max_iters = cfg->max_iters, pc.dist_thresh = cfg->dist_thresh;
    int rc = check_knn_pair_config(ctx, &pc);
    if (rc) return rc;
    if (cfg->max_frames < 2 || cfg->max_frames > kKnnStreamMaxFrames)
        return fail(ctx, DVO_EINVAL, "max_frames out of range (2..65536)");
    const bool sift = cfg->detector == DVO_DETECT_SIFT;
    const int det_cap = sift ? kSiftKpCap : surf_kp_cap(cfg->width, cfg->height);
    if (cfg->feat_cap != 0 && (cfg->feat_cap < 2 || cfg->feat_cap > det_cap))
        return fail(ctx, DVO_EINVAL, "feat_cap must be 0 or 2..the detector's list capacity");
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<dvo_knn_stream> s(new dvo_knn_stream);
    s->ctx = ctx;
    s->cfg = *cfg;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    if ((rc = knn_stream_plan(s.get()))) return rc;
    const int F = cfg->max_frames, P = F - 1, cap = cfg->feat_cap ? cfg->feat_cap : det_cap;
    hipError_t he = hipSuccess;
    s->b.layout(F, cap, sift ? 128 : 64, cus, 0, [&](auto*& p, size_t bytes) {
        he = s->mem.alloc(&p, bytes);
        return he == hipSuccess;
    });
    HIP_TRY(he);
    // the geometry as a dvo_stream has it: one set of P pairs, whose tracks read the batch's DMatch array
    HIP_TRY(stream_geometry(s->pairs, s->mem, *cfg, P, cap, (size_t)cfg->max_iters, 1, false, ctx->stream));
    *out = s.release();
    return DVO_OK;
}

void dvo_knn_stream_destroy(dvo_knn_stream* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    delete s;
}

int dvo_knn_stream_process(dvo_knn_stream* st, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                           dvo_pair_record* d_records) {
    if (!st) return DVO_EINVAL;
    if (n_frames > 1 && n_frames <= st->cfg.max_frames && !d_records)
        return fail(st->ctx, DVO_EINVAL, "bad frame or record buffer");
    const int rc = dvo_knn_stream_detect(st, d_frames, n_frames, frame_stride, stride, nullptr);
    return rc ? rc : dvo_knn_stream_finish(st, d_records, nullptr, 1, 0);
}

namespace {
// Detection of n_frames gray frames (d_frames, frame_stride, stride: the caller's, or the raw-input
// slab) and the frame state: dvo_knn_stream_detect after its argument checks.  ev_in: the event a
// raw-input call recorded before its input launch; it takes ev[0]'s place in the stage times.
int knn_stream_detect_gray(dvo_knn_stream* st, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                           uint64_t* d_draws, int ev_in = -1) {
    dvo_ctx* ctx = st->ctx;
    const dvo_knn_stream_config& c = st->cfg;
    const int w = c.width, h = c.height;
    HIP_TRY(hipSetDevice(ctx->device));
    // a group detector has its own scratch: the context's plan is not used
    const bool grouped = st->grp.group > 0 || st->sgrp.group > 0;
    int rc = grouped ? DVO_OK : knn_stream_plan(st);  // another size may have taken the context's plan since
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const KnnBatch& b = st->b;
    const bool sift = c.detector == DVO_DETECT_SIFT;
    hipEvent_t* ev = st->profiling ? st->ev : nullptr;
    st->last_frames = st->pending = st->matched_frames = 0;  // a pending detection is replaced
    st->timed = st->pending_timed = st->times_read = false;
    if (ev && ev_in < 0) HIP_TRY(hipEventRecord(ev[0], s));
    st->first_ev = ev_in;
    // detection in place on the caller's frames: a group of frames per launch straight into the
    // frame slots, or frame by frame on the plan's single scratch
    if (st->grp.group > 0)
        rc = sift_group_detect(ctx, st->grp, d_frames, n_frames, frame_stride, stride, b.cap, b.kps, b.desc, b.n, s,
                               st->nfeatures, &st->retain);
    else if (st->sgrp.group > 0)
        rc = surf_group_detect(ctx, st->sgrp, d_frames, n_frames, frame_stride, stride, c.hessian_threshold, b.cap, b.kps,
                               b.desc, b.n, s);
    if (rc) return rc;
    for (int f = 0; f < n_frames && !grouped; ++f) {
        const uint8_t* img = d_frames + (int64_t)f * frame_stride;
        dvo_keypoint* kps = b.kps + (size_t)f * b.cap;
        float* desc = b.desc + (size_t)f * b.cap * b.dim;
        int32_t* dn = b.n + 2 * (size_t)f;
        if (sift) {
            SiftPlanDev& D = ctx->sift;
            HIP_TRY(hipMemsetAsync(D.a.ncand, 0, 16, s));
            if (st->nfeatures > 0 && ctx->sift_retain.frames < 1) return fail(ctx, DVO_EINVAL, "SIFT retain scratch is missing");
            SiftRetainArgs ra = ctx->sift_retain.a;
            ra.nfeatures = st->nfeatures;
            HIP_TRY(launch_sift(D.a, img, w, h, stride, D.taps, D.tap_off, D.tap_n, s, st->nfeatures > 0 ? &ra : nullptr));
            HIP_TRY(launch_feature_copy(D.a.kps, D.a.desc, D.a.nkp, D.a.flags, b.cap, 128, kps, desc, dn, s));
        } else {
            SurfPlanDev& D = ctx->surf;
            D.a.thr = (float)c.hessian_threshold;
            HIP_TRY(hipMemsetAsync(D.a.nraw, 0, 16, s));
            const int64_t cells = D.a.off[kSurfTot - 1] + (int64_t)D.a.rows[kSurfOct - 1] * D.a.cols[kSurfOct - 1];
            HIP_TRY(hipMemsetAsync(D.a.det, 0, (size_t)cells * 4, s));
            HIP_TRY(hipMemsetAsync(D.a.trace, 0, (size_t)cells * 4, s));
            SurfArgs a = D.a;
            a.img = img;
            a.pitch = stride;
            HIP_TRY(launch_surf(a, s));
            HIP_TRY(launch_feature_copy(D.a.out, D.a.desc, D.a.nout, D.a.flags, b.cap, 64, kps, desc, dn, s));
        }
    }
    if (ev) HIP_TRY(hipEventRecord(ev[1], s));
    HIP_TRY(launch_knn_frame_state(b.n, n_frames, b.cap, b.fstate, s));
    if (d_draws) HIP_TRY(launch_flann_shard_draws(b.fstate, n_frames, st->fl.trees, d_draws, s));
    st->last_frames = st->pending = n_frames;
    st->pending_timed = ev != nullptr;
    return DVO_OK;
}
}  // namespace

int dvo_knn_stream_detect(dvo_knn_stream* st, const uint8_t* d_frames, int n_frames, int64_t frame_stride, int stride,
                          uint64_t* d_draws) {
    if (!st) return DVO_EINVAL;
    dvo_ctx* ctx = st->ctx;
    const dvo_knn_stream_config& c = st->cfg;
    if (n_frames < 1 || n_frames > c.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range (1..max_frames)");
    if (!d_frames || stride < c.width) return fail(ctx, DVO_EINVAL, "bad frame or record buffer");
    return knn_stream_detect_gray(st, d_frames, n_frames, frame_stride, stride, d_draws);
}

int dvo_knn_stream_finish(dvo_knn_stream* st, dvo_pair_record* d_records, const uint64_t* d_shard_draws, int world,
                          int rank) {
    if (!st) return DVO_EINVAL;
    dvo_ctx* ctx = st->ctx;
    const dvo_knn_stream_config& c = st->cfg;
    const int n_frames = st->pending;
    if (n_frames < 1) return fail(ctx, DVO_EINVAL, "no pending dvo_knn_stream_detect");
    if (world < 1 || world > kFlannShardMax || rank < 0 || rank >= world)
        return fail(ctx, DVO_EINVAL, "world out of range (1..1024) or rank outside it");
    if (n_frames > 1 && !d_records) return fail(ctx, DVO_EINVAL, "bad frame or record buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const KnnBatch& b = st->b;
    hipEvent_t* ev = st->profiling && st->pending_timed ? st->ev : nullptr;
    st->pending = 0;
    const PairOutputs out = st->next.take();  // for this batch alone
    const int pairs = n_frames - 1;
    const PairArrays& v = st->pairs.all;
    const bool flann = st->fl.trees > 0;
    const FlannShard shard{d_shard_draws, world, rank};
    HIP_TRY(b.match(n_frames, c.ratio, v.pts, v.nmatch, v.hdr, s, flann ? &st->fl : nullptr, 0, true,
                    flann && d_shard_draws ? &shard : nullptr));
    if (ev) HIP_TRY(hipEventRecord(ev[2], s));
    if (pairs >= 1) {
        // the stream's round schedule (not kStageOneRound): a record does not depend on the split into calls
        HIP_TRY(launch_geometry_args(v.g, pairs, kStageNormalize | kStageRansac, s));
        HIP_TRY(launch_retire(v.g, pairs, v.hdr, d_records, s));
        HIP_TRY(launch_knn_status(b.n, b.fstate, b.missing, pairs, d_records, s));
        // the batch's DMatch array is still its own
        const TrackIndex idx{&b.matches->queryIdx, &b.matches->trainIdx, b.cap, (int)(sizeof(dvo_dmatch) / sizeof(int32_t))};
        HIP_TRY(launch_pair_outputs(out, st->pairs, 0, v.g, pairs, d_records, &idx, s));
    }
    if (ev) {
        HIP_TRY(hipEventRecord(ev[3], s));
        st->timed = true;
        st->times_read = false;
    }
    st->matched_frames = n_frames;
    return DVO_OK;
}

int dvo_knn_stream_set_landmarks(dvo_knn_stream* s, dvo_landmark* d_out, int32_t* d_count, int cap) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_landmarks(s->pairs, s->ctx->device, d_out, d_count, cap));
}

int dvo_knn_stream_set_tracks(dvo_knn_stream* s, int32_t* d_link, dvo_track_scale* d_scale) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_tracks(s->pairs, s->ctx->device, d_link, d_scale));
}

int dvo_knn_stream_set_track_poses(dvo_knn_stream* s, dvo_track_pose* d_pose, int iters, double huber_px,
                                   double inlier_px, int min_points) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_poses(s->pairs, s->ctx->device, d_pose, iters, huber_px, inlier_px, min_points));
}

int dvo_knn_stream_set_track_refine(dvo_knn_stream* s, dvo_landmark_refined* d_refined, dvo_track_id* d_id, int views,
                                    int iters, double huber_px, double inlier_px) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx,
                       s->next.set_track_refine(s->pairs, s->ctx->device, d_refined, d_id, views, iters, huber_px, inlier_px));
}

int dvo_knn_stream_set_track_bundle(dvo_knn_stream* s, dvo_track_bundle* d_bundle, dvo_landmark_refined* d_points,
                                    int views, int iters, double lambda, double huber_px, double inlier_px,
                                    int min_points) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_bundle(s->pairs, s->ctx->device, d_bundle, d_points, views, iters, lambda,
                                                        huber_px, inlier_px, min_points));
}

int dvo_knn_stream_set_track_pnp(dvo_knn_stream* s, dvo_track_pnp* d_pnp, uint8_t* d_mask, int mask_cap, int hyps,
                                 int iters, double huber_px, double inlier_px, int min_points, uint64_t seed) {
    if (!s) return DVO_EINVAL;
    return bind_status(s->ctx, s->next.set_track_pnp(s->pairs, s->ctx->device, d_pnp, d_mask, mask_cap, hyps, iters, huber_px,
                                                     inlier_px, min_points, seed));
}

int dvo_knn_stream_sync(dvo_knn_stream* s) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    return DVO_OK;
}

void* dvo_knn_stream_hip_stream(dvo_knn_stream* s) { return s ? (void*)s->ctx->stream : nullptr; }

int dvo_knn_stream_set_detect_group(dvo_knn_stream* s, int group) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (s->cfg.detector != DVO_DETECT_SIFT) return fail(ctx, DVO_EINVAL, "the group detector is SIFT only");
    if (group < 0 || group > kSiftGroupMax) return fail(ctx, DVO_EINVAL, "group out of range (0..64)");
    s->pending = 0;  // a detection waiting for dvo_knn_stream_finish is dropped
    if (group == s->grp.group) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the old scratch may be in use
    s->grp = SiftGroupDev{};
    if (!group) return DVO_OK;
    int rc = sift_group_alloc(ctx, s->cfg.width, s->cfg.height, group, s->grp);
    if (rc || s->nfeatures == 0) return rc;
    if ((rc = sift_retain_ensure(ctx, s->retain, group))) s->grp = SiftGroupDev{};  // no group detector without it
    return rc;
}

int dvo_knn_stream_set_nfeatures(dvo_knn_stream* s, int nfeatures) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (s->cfg.detector != DVO_DETECT_SIFT)
        return fail(ctx, DVO_EINVAL, "nfeatures is SIFT's: OpenCV's SURF_create has no such parameter");
    if (nfeatures < 0) return fail(ctx, DVO_EINVAL, "nfeatures must be >= 0");
    if (nfeatures == s->nfeatures) return DVO_OK;
    s->pending = 0;  // a detection waiting for dvo_knn_stream_finish is dropped
    HIP_TRY(hipSetDevice(ctx->device));
    if (nfeatures > 0) {  // both routes' scratch now: dvo_knn_stream_set_detect_group may be switched off later
        int rc = sift_retain_ensure(ctx, ctx->sift_retain, 1);
        if (!rc && s->grp.group > 0) rc = sift_retain_ensure(ctx, s->retain, s->grp.group);
        if (rc) return rc;
    }
    s->nfeatures = nfeatures;
    return DVO_OK;
}

int dvo_knn_stream_set_surf_group(dvo_knn_stream* s, int group) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (s->cfg.detector != DVO_DETECT_SURF) return fail(ctx, DVO_EINVAL, "the group SURF detector needs a SURF stream");
    if (group < 0 || group > kSurfGroupMax) return fail(ctx, DVO_EINVAL, "group out of range (0..64)");
    s->pending = 0;  // a detection waiting for dvo_knn_stream_finish is dropped
    if (group == s->sgrp.group) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the old scratch may be in use
    s->sgrp = SurfGroupDev{};
    return group ? surf_group_alloc(ctx, s->cfg.width, s->cfg.height, group, s->sgrp) : DVO_OK;
}

int dvo_knn_stream_set_flann(dvo_knn_stream* s, int trees, int checks) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (trees < 0 || trees > 64) return fail(ctx, DVO_EINVAL, "trees out of range (0..64)");
    if (trees > 0 && checks < 1) return fail(ctx, DVO_EINVAL, "checks must be >= 1");
    s->pending = 0;  // a detection waiting for dvo_knn_stream_finish is dropped
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the old scratch may be in use
    if (trees != s->fl.trees) {
        s->fl = FlannBatchArgs{};
        s->fl_mem.release();
        if (trees == 0) return DVO_OK;
        FlannBatchArgs a{};
        hipError_t he = hipSuccess;
        flann_batch_layout(a, s->b.F - 1, s->b.cap, trees, [&](auto*& p, size_t bytes) {
            he = s->fl_mem.alloc(&p, bytes);
            return he == hipSuccess;
        });
        if (he != hipSuccess) s->fl_mem.release();
        HIP_TRY(he);
        a.trees = trees;
        s->fl = a;
    }
    if (trees == 0) return DVO_OK;
    s->fl.checks = checks;
    HIP_TRY(launch_flann_set_state(s->fl.state, 0xFFFFFFFFull, ctx->stream));  // cv::theRNG() of a fresh thread
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_knn_stream_set_rng_state(dvo_knn_stream* s, uint64_t state) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (s->fl.trees == 0) return fail(ctx, DVO_EINVAL, "the stream matches with BFMatcher: no theRNG state");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_flann_set_state(s->fl.state, state, ctx->stream));
    return DVO_OK;
}

int dvo_knn_stream_get_rng_state(dvo_knn_stream* s, uint64_t* state) {
    if (!s || !state) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (s->fl.trees == 0) return fail(ctx, DVO_EINVAL, "the stream matches with BFMatcher: no theRNG state");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(state, s->fl.state, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

size_t dvo_knn_stream_flann_bytes(int max_frames, int feat_cap, int trees) {
    if (max_frames < 2 || max_frames > kKnnStreamMaxFrames || feat_cap < 2 || feat_cap > (1 << 16) || trees < 1 || trees > 64)
        return 0;
    return flann_batch_bytes(max_frames - 1, feat_cap, trees);
}

int dvo_flann_rng_plan_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees, uint64_t* starts,
                            uint64_t* state_out) {
    if (!counts || !state_out || frames < 1 || cap < 1 || trees < 1 || trees > 64 || (frames > 1 && !starts))
        return DVO_EINVAL;
    flann_rng_plan_host(state, counts, frames, cap, trees, starts, state_out);
    return DVO_OK;
}

int dvo_flann_rng_shard_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees,
                             const uint64_t* shard_draws, int world, int rank, uint64_t* starts, uint64_t* final_state,
                             uint64_t* own_draws) {
    if (frames < 0 || (frames > 0 && !counts) || cap < 1 || trees < 1 || trees > 64 || (frames > 1 && !starts) ||
        world < 1 || world > kFlannShardMax || rank < 0 || rank >= world)
        return DVO_EINVAL;
    flann_rng_shard_host(state, counts, frames, cap, trees, shard_draws, world, rank, starts, final_state, own_draws);
    return DVO_OK;
}

int dvo_knn_stream_set_profiling(dvo_knn_stream* s, int enable) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (enable)
        for (hipEvent_t* e : {&s->ev[0], &s->ev[1], &s->ev[2], &s->ev[3], &s->ev_in[0], &s->ev_in[1]})
            if (!*e) HIP_TRY(hipEventCreate(e));
    s->profiling = enable != 0;
    s->timed = s->times_read = false;
    return DVO_OK;
}

int dvo_knn_stream_stage_times(dvo_knn_stream* s, double* ms) {
    if (!s || !ms) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (!s->timed) return fail(ctx, DVO_EINVAL, "no profiled dvo_knn_stream_process call");
    if (!s->times_read) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipEventSynchronize(s->ev[3]));
        for (int k = 0; k < 3; ++k) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, k == 0 && s->first_ev >= 0 ? s->ev_in[s->first_ev] : s->ev[k], s->ev[k + 1]));
            s->times_ms[k] = t;
        }
        s->times_read = true;
    }
    for (int k = 0; k < 3; ++k) ms[k] = s->times_ms[k];
    return DVO_OK;
}

int dvo_knn_stream_get_features(dvo_knn_stream* s, int frame, dvo_keypoint* kps, float* desc, int cap, int* n) {
    if (!s || !n) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    *n = 0;
    if (frame < 0 || frame >= s->last_frames) return fail(ctx, DVO_EINVAL, "frame outside the last call");
    const KnnBatch& b = s->b;
    HIP_TRY(hipSetDevice(ctx->device));
    int32_t cf[2];
    HIP_TRY(hipMemcpyAsync(cf, b.n + 2 * (size_t)frame, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n = cf[0];
    if (cf[1] || cf[0] > b.cap) return fail(ctx, DVO_ECAP, "the frame has more features than the stream keeps (feat_cap)");
    if (cf[0] > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (cf[0] <= 0) return DVO_OK;
    if (kps)
        HIP_TRY(hipMemcpyAsync(kps, b.kps + (size_t)frame * b.cap, (size_t)cf[0] * sizeof(dvo_keypoint), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (desc)
        HIP_TRY(hipMemcpyAsync(desc, b.desc + (size_t)frame * b.cap * b.dim, (size_t)cf[0] * b.dim * 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_knn_stream_get_matches(dvo_knn_stream* s, int pair, dvo_dmatch* out, int cap, int* m) {
    if (!s || !m) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    *m = 0;
    if (pair < 0 || pair >= s->matched_frames - 1) return fail(ctx, DVO_EINVAL, "pair outside the last call");
    HIP_TRY(hipSetDevice(ctx->device));
    int32_t nm = 0;
    HIP_TRY(hipMemcpyAsync(&nm, s->pairs.all.nmatch + pair, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *m = nm;
    if (nm > cap) return fail(ctx, DVO_ECAP, "caller capacity too small");
    if (nm <= 0) return DVO_OK;
    if (!out) return fail(ctx, DVO_EINVAL, "null buffer");
    HIP_TRY(hipMemcpyAsync(out, s->b.matches + (size_t)pair * s->b.cap, (size_t)nm * sizeof(dvo_dmatch),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

// Test hook: the matching stages of dvo_knn_stream_process on host arrays.
int dvo_test_knn_batch(dvo_ctx* ctx, const float* desc, const dvo_keypoint* kps, const int32_t* counts, int frames,
                       int cap, int dim, int ranges, double ratio, int32_t* idx, float* dist, int32_t* nmatch,
                       dvo_dmatch* matches, float* pts, int32_t* hdr, int32_t* missing, int* ranges_used) {
    if (!ctx || !desc || !kps || !counts || !idx || !dist || !nmatch || !matches || !pts || !hdr || !missing ||
        !ranges_used)
        return DVO_EINVAL;
    if (frames < 2 || frames > 4096 || cap < 2 || cap > (1 << 16) || (dim != 128 && dim != 64) || ranges < 0 ||
        ranges > cap)
        return fail(ctx, DVO_EINVAL, "frames 2..4096, cap 2..65536, dim 64 or 128, ranges 0..cap");
    if (!std::isfinite(ratio) || !(ratio > 0)) return fail(ctx, DVO_EINVAL, "ratio must be finite and > 0");
    for (int f = 0; f < frames; ++f)
        if (counts[f] < 0) return fail(ctx, DVO_EINVAL, "negative count");
    HIP_TRY(hipSetDevice(ctx->device));
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    hipStream_t s = ctx->stream;
    CallMem mem(ctx->call, s);
    KnnBatch b;
    b.layout(frames, cap, dim, cus, ranges, [&](auto*& p, size_t bytes) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(mem.dev<uint8_t>(bytes));
        return true;
    });
    const size_t P = (size_t)frames - 1, C = (size_t)cap;
    float* d_pts = mem.dev<float>(P * C * 4);
    int32_t* d_nmatch = mem.dev<int32_t>(P);
    PairHeader* d_hdr = mem.dev<PairHeader>(P);
    HIP_TRY(mem.error());
    std::vector<int32_t> n2(2 * (size_t)frames, 0);
    for (int f = 0; f < frames; ++f) n2[2 * (size_t)f] = counts[f];
    *ranges_used = b.ranges_of(frames - 1);
    uint8_t *hi, *hd, *hn, *hm, *hp, *hh, *hs;
    // after the first upload an error drains the stream before returning (the copies use the
    // context's pinned buffers, which the next per-call entry point rewrites)
    auto body = [&]() -> int {
        HIP_TRY(mem.put(b.desc, desc, (size_t)frames * C * dim * 4));
        HIP_TRY(mem.put(b.kps, kps, (size_t)frames * C * sizeof(dvo_keypoint)));
        HIP_TRY(mem.put(b.n, n2.data(), n2.size() * 4));
        HIP_TRY(b.match(frames, ratio, d_pts, d_nmatch, d_hdr, s));
        HIP_TRY(mem.get(b.idx, P * C * 8, &hi));
        HIP_TRY(mem.get(b.dist, P * C * 8, &hd));
        HIP_TRY(mem.get(d_nmatch, P * 4, &hn));
        HIP_TRY(mem.get(b.matches, P * C * sizeof(dvo_dmatch), &hm));
        HIP_TRY(mem.get(d_pts, P * C * 16, &hp));
        HIP_TRY(mem.get(d_hdr, P * sizeof(PairHeader), &hh));
        HIP_TRY(mem.get(b.missing, P * 4, &hs));
        HIP_TRY(hipStreamSynchronize(s));
        return DVO_OK;
    };
    if (int rc = body()) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::memcpy(idx, hi, P * C * 8);
    std::memcpy(dist, hd, P * C * 8);
    std::memcpy(nmatch, hn, P * 4);
    std::memcpy(matches, hm, P * C * sizeof(dvo_dmatch));
    std::memcpy(pts, hp, P * C * 16);
    std::memcpy(hdr, hh, P * sizeof(PairHeader));
    std::memcpy(missing, hs, P * 4);
    return DVO_OK;
}

// Test hook: the ORB stream's ratio-mode match stage (launch_match_ratio) and pair statuses on host arrays.
int dvo_test_hamming_ratio_batch(dvo_ctx* ctx, const uint8_t* desc, const dvo_keypoint* kps, const int32_t* counts,
                                 int frames, int cap, double ratio, int32_t* top2, int32_t* nmatch, dvo_dmatch* matches,
                                 float* pts, int32_t* status) {
    if (!ctx || !desc || !kps || !counts || !top2 || !nmatch || !matches || !pts || !status) return DVO_EINVAL;
    if (frames < 2 || frames > 4096 || cap < 1 || cap > 8192)
        return fail(ctx, DVO_EINVAL, "frames 2..4096, cap 1..8192");
    if (!std::isfinite(ratio) || !(ratio > 0)) return fail(ctx, DVO_EINVAL, "ratio must be finite and > 0");
    for (int f = 0; f < frames; ++f)
        if (counts[f] < 0 || counts[f] > cap) return fail(ctx, DVO_EINVAL, "count out of range (0..cap)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CallMem mem(ctx->call, s);
    const size_t F = (size_t)frames, P = F - 1, C = (size_t)cap;
    StreamParams sp{};
    sp.plan.kp_cap = cap;
    sp.nframes = frames;
    sp.pair_step = 1;
    Buffers& b = sp.buf;
    b.desc = mem.dev<uint8_t>(F * C * 32);
    b.kps = mem.dev<dvo_keypoint>(F * C);
    b.nkp = mem.dev<int32_t>(F);
    b.status = mem.dev<int32_t>(F);
    b.nn = mem.dev<int32_t>(2 * F * C);
    b.mq = mem.dev<int32_t>(F * C);
    b.mt = mem.dev<int32_t>(F * C);
    b.md = mem.dev<float>(F * C);
    b.pts = mem.dev<float>(F * C * 4);
    b.nmatch = mem.dev<int32_t>(F);
    b.hdr = mem.dev<PairHeader>(F);
    int32_t* d_status = mem.dev<int32_t>(F);
    HIP_TRY(mem.error());
    uint8_t *hw, *hn, *hq, *ht, *hd, *hp, *hs;
    auto body = [&]() -> int {
        HIP_TRY(mem.put(b.desc, desc, F * C * 32));
        HIP_TRY(mem.put(b.kps, kps, F * C * sizeof(dvo_keypoint)));
        HIP_TRY(mem.put(b.nkp, counts, F * 4));
        HIP_TRY(hipMemsetAsync(b.status, 0, F * 4, s));
        HIP_TRY(hipMemsetAsync(b.nn, 0xFF, 2 * F * C * 4, s));  // slots the kernels leave read as "none"
        HIP_TRY(launch_match_ratio(sp, ratio, s));
        HIP_TRY(launch_pair_header(sp, b.hdr, s));
        HIP_TRY(launch_hamming_ratio_status(b.hdr, (int)P, nullptr, d_status, s));
        HIP_TRY(mem.get(b.nn, 2 * F * C * 4, &hw));
        HIP_TRY(mem.get(b.nmatch, P * 4, &hn));
        HIP_TRY(mem.get(b.mq, P * C * 4, &hq));
        HIP_TRY(mem.get(b.mt, P * C * 4, &ht));
        HIP_TRY(mem.get(b.md, P * C * 4, &hd));
        HIP_TRY(mem.get(b.pts, P * C * 16, &hp));
        HIP_TRY(mem.get(d_status, P * 4, &hs));
        HIP_TRY(hipStreamSynchronize(s));
        return DVO_OK;
    };
    if (int rc = body()) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::memcpy(nmatch, hn, P * 4);
    std::memcpy(status, hs, P * 4);
    std::memcpy(pts, hp, P * C * 16);
    const int32_t *w = (const int32_t*)hw, *mq = (const int32_t*)hq, *mt = (const int32_t*)ht;
    const float* md = (const float*)hd;
    for (size_t p = 0; p < P; ++p) {
        for (size_t q = 0; q < C; ++q) {  // [P][cap][2]: nearest, second
            top2[(p * C + q) * 2] = w[p * C + q];
            top2[(p * C + q) * 2 + 1] = w[(F + p) * C + q];
        }
        const size_t m = (size_t)std::min(std::max(nmatch[p], 0), cap);
        for (size_t i = 0; i < C; ++i)
            matches[p * C + i] = i < m ? dvo_dmatch{mq[p * C + i], mt[p * C + i], 0, md[p * C + i]} : dvo_dmatch{-1, -1, 0, 0.f};
    }
    return DVO_OK;
}

// Test hook: the batched kd-forest build and search of dvo_knn_stream_process's FLANN mode on host arrays.
int dvo_test_flann_batch(dvo_ctx* ctx, const float* desc, const int32_t* counts, int frames, int cap, int dim, int trees,
                         int checks, uint64_t state, int levels, int32_t* idx, float* dist, uint64_t* starts,
                         uint64_t* state_out, int* n_global, int* depth) {
    if (!ctx || !desc || !counts || !idx || !dist || !starts || !state_out || !n_global || !depth) return DVO_EINVAL;
    if (frames < 2 || frames > 4096 || cap < 2 || cap > (1 << 16) || (dim != 128 && dim != 64) || trees < 1 || trees > 64 ||
        checks < 1 || levels < 0 || levels > 1024)
        return fail(ctx, DVO_EINVAL, "frames 2..4096, cap 2..65536, dim 64 or 128, trees 1..64, checks >= 1, levels 0..1024");
    for (int f = 0; f < frames; ++f)
        if (counts[f] < 0) return fail(ctx, DVO_EINVAL, "negative count");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CallMem mem(ctx->call, s);
    const size_t P = (size_t)frames - 1, C = (size_t)cap;
    FlannBatchArgs a{};
    a.desc = mem.dev<float>((size_t)frames * C * dim);
    int32_t* d_n = mem.dev<int32_t>(2 * (size_t)frames);
    int32_t* d_fstate = mem.dev<int32_t>(2 * (size_t)frames);
    a.fstate = d_fstate;
    a.cap = cap, a.dim = dim, a.trees = trees, a.checks = checks;
    a.idx = mem.dev<int32_t>(P * C * 2);
    a.dist = mem.dev<float>(P * C * 2);
    flann_batch_layout(a, frames - 1, cap, trees, [&](auto*& p, size_t bytes) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(mem.dev<uint8_t>(bytes));
        return true;
    });
    HIP_TRY(mem.error());
    std::vector<int32_t> n2(2 * (size_t)frames, 0);
    for (int f = 0; f < frames; ++f) n2[2 * (size_t)f] = counts[f];
    uint8_t *hi, *hd, *hs, *hst, *hc;
    auto body = [&]() -> int {
        HIP_TRY(mem.put(const_cast<float*>(a.desc), desc, (size_t)frames * C * dim * 4));
        HIP_TRY(mem.put(d_n, n2.data(), n2.size() * 4));
        HIP_TRY(launch_flann_set_state(a.state, state, s));
        HIP_TRY(launch_knn_frame_state(d_n, frames, cap, d_fstate, s));
        HIP_TRY(launch_flann_batch(a, frames, levels, s));
        HIP_TRY(mem.get(a.idx, P * C * 8, &hi));
        HIP_TRY(mem.get(a.dist, P * C * 8, &hd));
        HIP_TRY(mem.get(a.starts, P * 8, &hs));
        HIP_TRY(mem.get(a.state, 8, &hst));
        HIP_TRY(mem.get(a.ctl, 16, &hc));
        HIP_TRY(hipStreamSynchronize(s));
        return DVO_OK;
    };
    if (int rc = body()) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::memcpy(idx, hi, P * C * 8);
    std::memcpy(dist, hd, P * C * 8);
    std::memcpy(starts, hs, P * 8);
    std::memcpy(state_out, hst, 8);
    int32_t ctl[4];
    std::memcpy(ctl, hc, 16);
    *n_global = ctl[0];
    *depth = ctl[1];
    return DVO_OK;
}

// ---------------------------------------------------------------------------
int dvo_test_retain_best(dvo_ctx* ctx, const float* resp, int n, int n_points, int depth, int semantics,
                         int32_t* perm, int* k_out) {
    if (!ctx || !resp || !perm || !k_out || n < 0) return DVO_EINVAL;
    if (semantics != DVO_OPENCV_4X && semantics != DVO_OPENCV_32) return fail(ctx, DVO_EINVAL, "bad semantics");
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    float* dv = mem.dev<float>((size_t)n + 1);
    uint32_t* dk = mem.dev<uint32_t>((size_t)n + 1);
    int32_t* dt = mem.dev<int32_t>((size_t)2 * n + 2);
    int* dkk = mem.dev<int>(2);
    HIP_TRY(mem.error());
    std::vector<uint32_t> ids(n);
    for (int i = 0; i < n; ++i) ids[i] = (uint32_t)i;
    if (n) {
        HIP_TRY(hipMemcpy(dv, resp, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dk, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_test_retain_best(dv, dk, dt, n, n_points, depth, semantics, dkk, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int k = 0;
    HIP_TRY(hipMemcpy(&k, dkk, sizeof(int), hipMemcpyDeviceToHost));
    *k_out = k;
    if (k) HIP_TRY(hipMemcpy(perm, dk, (size_t)k * 4, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_test_update_num_iters(dvo_ctx* ctx, double p, const double* ep, int n, int model_points, int max_iters,
                              int32_t* out) {
    if (!ctx || !ep || !out || n < 0) return DVO_EINVAL;
    if (n == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    double* de = mem.dev<double>(n);
    int32_t* dout = mem.dev<int32_t>(n);
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpy(de, ep, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(launch_test_update_num_iters(p, de, n, model_points, max_iters, dout, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_test_ransac_subsets(dvo_ctx* ctx, int m, int n, int32_t* idx) {
    if (!ctx || !idx || m < 6 || n < 1) return DVO_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    RansacState* drs = mem.dev<RansacState>(1);
    int32_t* dsub = mem.dev<int32_t>((size_t)n * 5);
    HIP_TRY(mem.error());
    RansacState S{};
    S.rng = ~0ull;
    S.m = m;
    S.niters = n;  // round 2 of the sampler covers [h1, niters) = [0, n)
    HIP_TRY(hipMemcpyAsync(drs, &S, sizeof(S), hipMemcpyHostToDevice, ctx->stream));
    GeomArgs g{};
    g.rs = drs;
    g.subsets = dsub;
    g.hyp_cap = n;
    g.m_const = m;
    HIP_TRY(launch_test_ransac_sample(g, ctx->stream));
    HIP_TRY(hipMemcpyAsync(idx, dsub, (size_t)n * 20, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_test_ransac_replay(dvo_ctx* ctx, const int32_t* nmod, const int32_t* cnt, int n, int m, double prob,
                           int max_iters, int32_t* out) {
    if (!ctx || !nmod || !cnt || !out || n < 1 || m < 6) return DVO_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    RansacState* drs = mem.dev<RansacState>(1);
    int32_t* dn = mem.dev<int32_t>(n);
    int32_t* dc = mem.dev<int32_t>((size_t)n * 10);
    HIP_TRY(mem.error());
    RansacState S{};
    S.m = m;
    S.niters = max_iters > 1 ? max_iters : 1;
    S.h0 = 0;
    S.h1 = n < S.niters ? n : S.niters;
    S.best_h = S.best_i = -1;
    HIP_TRY(hipMemcpyAsync(drs, &S, sizeof(S), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dn, nmod, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dc, cnt, (size_t)n * 40, hipMemcpyHostToDevice, ctx->stream));
    GeomArgs g{};
    g.rs = drs;
    g.nmod = dn;
    g.cnt = dc;
    g.hyp_cap = n;
    g.prob = prob;
    HIP_TRY(launch_test_ransac_replay(g, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&S, drs, sizeof(S), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    out[0] = S.iter;
    out[1] = S.niters;
    out[2] = S.maxgood;
    out[3] = S.best_h;
    out[4] = S.best_i;
    return DVO_OK;
}

int dvo_test_ransac_hypotheses(dvo_ctx* ctx, const double* pts, const int32_t* m, int P, int stride, const double* K,
                               double prob, double threshold, int n_hyp, int schedule, int32_t* subsets,
                               int32_t* nmod, double* models, int32_t* cnt, int32_t* state, int32_t* bounds,
                               int* n_rounds, int32_t* path, int32_t* parked) {
    if (!ctx || !pts || !m || !K || !subsets || !nmod || !models || !cnt || !state || !bounds || !n_rounds || !path ||
        !parked)
        return DVO_EINVAL;
    if (P < 1 || stride < 1 || n_hyp < 1 || n_hyp > (1 << 20) || (int64_t)P * n_hyp > (1 << 24))
        return fail(ctx, DVO_EINVAL, "bad pair or hypothesis count");
    if (schedule != DVO_TEST_SCHED_CALL && schedule != DVO_TEST_SCHED_BATCH_ONE &&
        schedule != DVO_TEST_SCHED_BATCH_ROUNDS)
        return fail(ctx, DVO_EINVAL, "unknown schedule");
    if (schedule == DVO_TEST_SCHED_CALL && P != 1) return fail(ctx, DVO_EINVAL, "the per-call schedule takes one pair");
    if (!(prob > 0 && prob < 1) || !(threshold > 0) || !std::isfinite(threshold))
        return fail(ctx, DVO_EINVAL, "bad prob or threshold");
    for (int p = 0; p < P; ++p)
        if (m[p] < 0 || m[p] > stride) return fail(ctx, DVO_EINVAL, "m[p] must be in [0, stride]");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t hc = (size_t)n_hyp, PH = (size_t)P * hc, npt = (size_t)P * stride * 4;
    const size_t nblocks = (PH + 63) / 64 + 1, nrec = nblocks * 128 * 64;
    const bool one = schedule != DVO_TEST_SCHED_BATCH_ROUNDS;
    CallMem mem(ctx->call, ctx->stream);
    GeomArgs g{};
    double* dpts = mem.dev<double>(npt);
    int32_t* dm = mem.dev<int32_t>(P);
    g.pts_d = dpts;
    g.m_arr = dm;
    g.pts_stride = stride;
    set_camera(g, K);
    g.prob = prob;
    g.threshold = threshold;
    g.max_iters = n_hyp;
    call_geometry(g, mem, kGeomRansac, (size_t)P, (size_t)stride, hc, nblocks);  // fprec: the nrec records read back below
    HIP_TRY(mem.error());
    HIP_TRY(mem.put(dpts, pts, npt * 8));
    HIP_TRY(mem.put(dm, m, (size_t)P * 4));
    // what a launch does not write stays recognisable: nmod -1 (hypothesis not evaluated), the rest 0
    HIP_TRY(hipMemsetAsync(g.nmod, 0xFF, PH * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.models, 0, PH * 90 * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.cnt, 0, PH * 10 * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.subsets, 0, PH * 5 * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.rs, 0, (size_t)P * sizeof(RansacState), ctx->stream));
    HIP_TRY(hipMemsetAsync(g.fprec, 0, nrec * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.dk_off, 0, ((size_t)P + 1) * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(g.dk_ctl, 0, (2 + kDkMaxPasses) * 4, ctx->stream));
    if (schedule == DVO_TEST_SCHED_CALL) {
        HIP_TRY(launch_geometry_args(g, 1, kStageNormalize | kStageRansac | kStageOneRound, ctx->stream));
    } else if (schedule == DVO_TEST_SCHED_BATCH_ONE) {
        HIP_TRY(launch_test_ransac_one_round(g, P, ctx->stream));
    } else {
        HIP_TRY(launch_geometry_args(g, P, kStageNormalize | kStageRansac, ctx->stream));
    }
    uint8_t *hsub, *hnmod, *hmodels, *hcnt, *hrs, *hrec = nullptr, *hoff = nullptr, *hctl = nullptr;
    HIP_TRY(mem.get(g.subsets, PH * 5 * 4, &hsub));
    HIP_TRY(mem.get(g.nmod, PH * 4, &hnmod));
    HIP_TRY(mem.get(g.models, PH * 90 * 8, &hmodels));
    HIP_TRY(mem.get(g.cnt, PH * 10 * 4, &hcnt));
    HIP_TRY(mem.get(g.rs, (size_t)P * sizeof(RansacState), &hrs));
    if (one) {
        HIP_TRY(mem.get(g.fprec, nrec * 8, &hrec));
        HIP_TRY(mem.get(g.dk_off, ((size_t)P + 1) * 4, &hoff));
        HIP_TRY(mem.get(g.dk_ctl, (2 + kDkMaxPasses) * 4, &hctl));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(subsets, hsub, PH * 5 * 4);
    std::memcpy(nmod, hnmod, PH * 4);
    std::memcpy(models, hmodels, PH * 90 * 8);
    std::memcpy(cnt, hcnt, PH * 10 * 4);
    for (int p = 0; p < P; ++p) {
        RansacState S;
        std::memcpy(&S, hrs + (size_t)p * sizeof(S), sizeof(S));
        const int32_t st[5] = {S.iter, S.niters, S.maxgood, S.best_h, S.best_i};
        std::memcpy(state + 5 * p, st, sizeof(st));
    }
    if (one) {
        *n_rounds = 1;
        bounds[0] = 1 << 30;
        // the one round's records: hypothesis h of pair p is work item dk_off[p] + h (h0 = 0)
        const double* rec = reinterpret_cast<const double*>(hrec);
        const int32_t* off = reinterpret_cast<const int32_t*>(hoff);
        for (int p = 0; p < P; ++p)
            for (size_t h = 0; h < hc; ++h) {
                const size_t o = (size_t)p * hc + h;
                const int64_t item = (int64_t)off[p] + (int64_t)h;
                path[o] = nmod[o] < 0 || item >= off[p + 1] ? -1 : (int32_t)rec[test_record_generic_offset(item)];
            }
        std::memcpy(parked, hctl + 2 * 4, kDkMaxPasses * 4);
    } else {
        *n_rounds = kRansacRounds;
        for (int r = 0; r < kRansacRounds; ++r) bounds[r] = kRansacBounds[r];
        for (size_t o = 0; o < PH; ++o) path[o] = -1;
        for (int k = 0; k < kDkMaxPasses; ++k) parked[k] = -1;
    }
    return DVO_OK;
}

int dvo_test_landmarks(dvo_ctx* ctx, const float* pts, const int32_t* m, int pairs, int stride, const double* K,
                       double prob, double threshold, int max_iters, double dist_thresh, int cap, dvo_landmark* out,
                       int32_t* count, dvo_pair_record* rec) {
    if (!ctx || !pts || !m || !K || !out || !count || !rec) return DVO_EINVAL;
    if (pairs < 1 || pairs > 65535 || stride < 1 || cap < 1) return fail(ctx, DVO_EINVAL, "bad pair count, stride or cap");
    if (!(prob > 0 && prob < 1) || !(threshold > 0) || !std::isfinite(threshold) || max_iters < 1 ||
        max_iters > (1 << 20) || !std::isfinite(dist_thresh))
        return fail(ctx, DVO_EINVAL, "bad prob, threshold, max_iters or dist_thresh");
    for (int p = 0; p < pairs; ++p)
        if (m[p] < 5 || m[p] > stride) return fail(ctx, DVO_EINVAL, "m[p] must be in [5, stride]");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t P = (size_t)pairs, hc = (size_t)max_iters, PH = P * hc, npt = P * stride * 4;
    const size_t tiles = (size_t)landmark_tiles(stride);
    CallMem mem(ctx->call, ctx->stream);
    GeomArgs g{};
    float* dpts = mem.dev<float>(npt);
    int32_t* dm = mem.dev<int32_t>(P);
    g.pts_f = dpts;
    g.m_arr = dm;
    g.pts_stride = stride;
    set_camera(g, K);
    g.prob = prob;
    g.threshold = threshold;
    g.max_iters = max_iters;
    g.dist_thresh = dist_thresh;
    call_geometry(g, mem, kGeomRansac | kGeomPose, P, (size_t)stride, hc);
    PairHeader* dhdr = mem.dev<PairHeader>(P);
    dvo_pair_record* drec = mem.dev<dvo_pair_record>(P);
    LandmarkScratch L;
    L.tmp = mem.dev<LandmarkTmp>(P * tiles * kLandmarkTile);
    L.tcnt = mem.dev<int32_t>(P * tiles);
    dvo_landmark* dout = mem.dev<dvo_landmark>(P * (size_t)cap);
    int32_t* dcount = mem.dev<int32_t>(P);
    HIP_TRY(mem.error());
    std::vector<PairHeader> hdr(P);
    for (int p = 0; p < pairs; ++p) hdr[p] = PairHeader{m[p], m[p], 0, 0};
    HIP_TRY(mem.put(dpts, pts, npt * sizeof(float)));
    HIP_TRY(mem.put(dm, m, P * 4));
    HIP_TRY(mem.put(dhdr, hdr.data(), P * sizeof(PairHeader)));
    HIP_TRY(mem.put(dout, out, P * (size_t)cap * sizeof(dvo_landmark)));
    for (int p = 0; p < pairs; ++p) {  // findEssentialMat pair by pair, as dvo_find_essential_mat launches it
        GeomArgs gp = g;
        gp.pts_f += (size_t)p * stride * 4;
        gp.m_arr += p;
        gp.npts += (size_t)p * stride * 4;
        gp.models += (size_t)p * hc * 90;
        gp.nmod += (size_t)p * hc;
        gp.cnt += (size_t)p * hc * 10;
        gp.subsets += (size_t)p * hc * 5;
        gp.rs += p;
        gp.E += (size_t)p * 90;
        gp.info += (size_t)p * 4;
        HIP_TRY(launch_geometry_args(gp, 1, kStageNormalize | kStageRansac | kStageOneRound, ctx->stream));
    }
    HIP_TRY(launch_retire(g, pairs, dhdr, drec, ctx->stream));  // every pair at once, as a stream's set retires
    HIP_TRY(launch_landmarks(g, pairs, drec, L, dout, dcount, cap, ctx->stream));
    uint8_t *hout, *hcount, *hrec;
    HIP_TRY(mem.get(dout, P * (size_t)cap * sizeof(dvo_landmark), &hout));
    HIP_TRY(mem.get(dcount, P * 4, &hcount));
    HIP_TRY(mem.get(drec, P * sizeof(dvo_pair_record), &hrec));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(out, hout, P * (size_t)cap * sizeof(dvo_landmark));
    std::memcpy(count, hcount, P * 4);
    std::memcpy(rec, hrec, P * sizeof(dvo_pair_record));
    return DVO_OK;
}

// dvo_test_tracks, and with tp (a binding without its buffer), K and pose dvo_test_track_poses, and
// with rf (its parameters and use_pose) dvo_test_track_refine, refined and id each optional, and
// with bd (its parameters and use_pose) dvo_test_track_bundle, bundle and points each optional
static int test_tracks_run(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                           const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                           int kp_cap, int cap_out, int32_t* link, dvo_track_scale* scale, const double* K,
                           const TrackPoseBinding* tp, dvo_track_pose* pose, const TrackRefineBinding* rf = nullptr,
                           dvo_landmark_refined* refined = nullptr, dvo_track_id* id = nullptr,
                           const TrackBundleBinding* bd = nullptr, dvo_track_bundle* bundle = nullptr,
                           dvo_landmark_refined* points = nullptr, const TrackPnpBinding* pn = nullptr,
                           const float* xy2 = nullptr, dvo_track_pnp* pnp = nullptr, uint8_t* mask = nullptr) {
    if (!ctx || !lm || !count || !mq || !mt || !m || !rec || !link || !scale) return DVO_EINVAL;
    if (pairs < 1 || pairs > 65535 || cap < 1 || stride < 1 || kp_cap < 1 || cap_out < 1)
        return fail(ctx, DVO_EINVAL, "bad pair count, cap, stride, kp_cap or cap_out");
    const size_t P = (size_t)pairs, tiles = (size_t)landmark_tiles(stride);
    std::vector<LandmarkTmp> tmp(P * tiles * kLandmarkTile);
    std::vector<int32_t> tcnt(P * tiles, 0);
    for (int p = 0; p < pairs; ++p) {
        if (m[p] < 0 || m[p] > stride || count[p] < 0 || count[p] > cap || count[p] > m[p])
            return fail(ctx, DVO_EINVAL, "need 0 <= count[p] <= min(cap, m[p]) and m[p] <= stride");
        for (int i = 0; i < m[p]; ++i) {
            const size_t at = (size_t)p * stride + i;
            if (mq[at] < 0 || mq[at] >= kp_cap || mt[at] < 0 || mt[at] >= kp_cap)
                return fail(ctx, DVO_EINVAL, "match index outside [0, kp_cap)");
        }
        for (int o = 0; o < count[p]; ++o) {  // into the tile of its match, as landmark_tile_kernel compacts
            const dvo_landmark& e = lm[(size_t)p * cap + o];
            if (e.match < 0 || e.match >= m[p] || (o > 0 && e.match <= lm[(size_t)p * cap + o - 1].match))
                return fail(ctx, DVO_EINVAL, "landmark matches must ascend inside [0, m[p])");
            const size_t t = (size_t)p * tiles + e.match / kLandmarkTile;
            tmp[t * kLandmarkTile + tcnt[t]++] = LandmarkTmp{e.X, e.Y, e.Z, e.match, 0};
        }
    }
    std::vector<float> pts;  // the point buffer the pose binding reads: each landmark's x2, y2 at its match
    if (tp) {
        pts.assign(P * stride * 4, 0.f);
        for (int p = 0; p < pairs; ++p)
            for (int o = 0; o < count[p]; ++o) {
                const dvo_landmark& e = lm[(size_t)p * cap + o];
                float* q = &pts[((size_t)p * stride + e.match) * 4];
                q[0] = e.x1, q[1] = e.y1, q[2] = e.x2, q[3] = e.y2;
            }
        if (pn)  // every match's second-frame pixel
            for (int p = 0; p < pairs; ++p)
                for (int i = 0; i < m[p]; ++i) {
                    float* q = &pts[((size_t)p * stride + i) * 4];
                    q[2] = xy2[((size_t)p * stride + i) * 2], q[3] = xy2[((size_t)p * stride + i) * 2 + 1];
                }
    }
    std::vector<dvo_pair_record> rec_pn;  // the PnP kernels read the match count from the record
    if (pn) {
        rec_pn.assign(rec, rec + pairs);
        for (int p = 0; p < pairs; ++p) rec_pn[p].n_matches = m[p];
        rec = rec_pn.data();
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    TrackArgs a{};
    LandmarkTmp* dtmp = mem.dev<LandmarkTmp>(tmp.size());
    int32_t* dtcnt = mem.dev<int32_t>(tcnt.size());
    int32_t* dq = mem.dev<int32_t>(P * stride);
    int32_t* dt = mem.dev<int32_t>(P * stride);
    dvo_pair_record* drec = mem.dev<dvo_pair_record>(P);
    a.table = mem.dev<int32_t>(P * kp_cap);
    a.ratio = mem.dev<double>(P * stride);
    a.lcnt = mem.dev<int32_t>(P * tiles);
    a.link = mem.dev<int32_t>(P * cap_out);
    a.scale = mem.dev<dvo_track_scale>(P);
    float* dpts = tp ? mem.dev<float>(pts.size()) : nullptr;
    TrackCorr* dcorr = tp ? mem.dev<TrackCorr>(P * stride) : nullptr;
    dvo_track_pose* dpose = tp ? mem.dev<dvo_track_pose>(P) : nullptr;
    int32_t* dflink = rf || bd ? mem.dev<int32_t>(P * stride) : nullptr;
    TrackRank* drank = rf ? mem.dev<TrackRank>(2 * P * stride) : nullptr;
    dvo_landmark_refined* drefined = rf && refined ? mem.dev<dvo_landmark_refined>(P * cap_out) : nullptr;
    dvo_track_id* did = rf && id ? mem.dev<dvo_track_id>(P * cap_out) : nullptr;
    BundlePoint* dbx = bd ? mem.dev<BundlePoint>(P * stride) : nullptr;
    dvo_track_bundle* dbundle = bd && bundle ? mem.dev<dvo_track_bundle>(P) : nullptr;
    dvo_landmark_refined* dpoints = bd && points ? mem.dev<dvo_landmark_refined>(P * cap_out) : nullptr;
    PnpCorr* dpc = pn ? mem.dev<PnpCorr>(P * stride) : nullptr;
    int32_t* dpcnt = pn ? mem.dev<int32_t>(P * tiles) : nullptr;
    dvo_track_pnp* dpnp = pn ? mem.dev<dvo_track_pnp>(P) : nullptr;
    uint8_t* dmask = pn && mask ? mem.dev<uint8_t>(P * pn->mask_cap) : nullptr;
    HIP_TRY(mem.error());
    // the scratch side by hand (what PairSets::track_args gives a stream), the caller's side as the streams fill it
    a.L.tmp = dtmp;
    a.L.tcnt = dtcnt;
    a.tiles = (int)tiles;
    a.mq = dq;
    a.mt = dt;
    a.idx_stride = stride;
    a.idx_step = 1;
    a.kp_cap = kp_cap;
    a.pts_stride = stride;
    a.corr = dcorr;
    a.flink = dflink;
    a.rank = drank;
    a.rank_stride = (int64_t)P * stride;
    a.bd_x = dbx;
    a.pnp_corr = dpc;
    a.pnp_cnt = dpcnt;
    PairOutputs o;
    o.lm.cap = cap_out;
    o.tr = TracksBinding{a.link, a.scale};
    if (tp) o.tp = *tp, o.tp.out = dpose;
    if (rf) o.rf = *rf, o.rf.refined = drefined, o.rf.id = did;
    if (bd) o.bd = *bd, o.bd.out = dbundle, o.bd.points = dpoints;
    if (pn) o.pn = *pn, o.pn.out = dpnp, o.pn.mask = dmask, o.pn.mask_cap = dmask ? pn->mask_cap : 0;
    GeomArgs g{};
    g.pts_f = dpts;
    if (tp) set_camera(g, K);
    o.fill(a, g, drec);
    HIP_TRY(mem.put(dtmp, tmp.data(), tmp.size() * sizeof(LandmarkTmp)));
    HIP_TRY(mem.put(dtcnt, tcnt.data(), tcnt.size() * 4));
    HIP_TRY(mem.put(dq, mq, P * stride * 4));
    HIP_TRY(mem.put(dt, mt, P * stride * 4));
    HIP_TRY(mem.put(drec, rec, P * sizeof(dvo_pair_record)));
    HIP_TRY(mem.put(a.link, link, P * cap_out * 4));
    if (tp) HIP_TRY(mem.put(dpts, pts.data(), pts.size() * sizeof(float)));
    if (drefined) HIP_TRY(mem.put(drefined, refined, P * cap_out * sizeof(dvo_landmark_refined)));
    if (did) HIP_TRY(mem.put(did, id, P * cap_out * sizeof(dvo_track_id)));
    if (dbundle) HIP_TRY(mem.put(dbundle, bundle, P * sizeof(dvo_track_bundle)));
    if (dpoints) HIP_TRY(mem.put(dpoints, points, P * cap_out * sizeof(dvo_landmark_refined)));
    if (dmask) HIP_TRY(mem.put(dmask, mask, P * pn->mask_cap));
    HIP_TRY(launch_tracks(a, pairs, ctx->stream));
    uint8_t *hpnp = nullptr, *hmask = nullptr;
    if (dpnp) HIP_TRY(mem.get(dpnp, P * sizeof(dvo_track_pnp), &hpnp));
    if (dmask) HIP_TRY(mem.get(dmask, P * pn->mask_cap, &hmask));
    uint8_t *hlink, *hscale, *hpose = nullptr, *hrefined = nullptr, *hid = nullptr, *hbundle = nullptr, *hpoints = nullptr;
    if (dbundle) HIP_TRY(mem.get(dbundle, P * sizeof(dvo_track_bundle), &hbundle));
    if (dpoints) HIP_TRY(mem.get(dpoints, P * cap_out * sizeof(dvo_landmark_refined), &hpoints));
    if (drefined) HIP_TRY(mem.get(drefined, P * cap_out * sizeof(dvo_landmark_refined), &hrefined));
    if (did) HIP_TRY(mem.get(did, P * cap_out * sizeof(dvo_track_id), &hid));
    HIP_TRY(mem.get(a.link, P * cap_out * 4, &hlink));
    HIP_TRY(mem.get(a.scale, P * sizeof(dvo_track_scale), &hscale));
    if (tp) HIP_TRY(mem.get(dpose, P * sizeof(dvo_track_pose), &hpose));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(link, hlink, P * cap_out * 4);
    std::memcpy(scale, hscale, P * sizeof(dvo_track_scale));
    if (tp) std::memcpy(pose, hpose, P * sizeof(dvo_track_pose));
    if (hrefined) std::memcpy(refined, hrefined, P * cap_out * sizeof(dvo_landmark_refined));
    if (hid) std::memcpy(id, hid, P * cap_out * sizeof(dvo_track_id));
    if (hbundle) std::memcpy(bundle, hbundle, P * sizeof(dvo_track_bundle));
    if (hpoints) std::memcpy(points, hpoints, P * cap_out * sizeof(dvo_landmark_refined));
    if (hpnp) std::memcpy(pnp, hpnp, P * sizeof(dvo_track_pnp));
    if (hmask) std::memcpy(mask, hmask, P * pn->mask_cap);
    return DVO_OK;
}

int dvo_test_tracks(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq, const int32_t* mt,
                    const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride, int kp_cap,
                    int cap_out, int32_t* link, dvo_track_scale* scale) {
    return test_tracks_run(ctx, lm, count, mq, mt, m, rec, pairs, cap, stride, kp_cap, cap_out, link, scale, nullptr,
                           nullptr, nullptr);
}

int dvo_test_track_poses(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                         const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                         int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                         int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose) {
    if (!ctx || !K || !pose) return DVO_EINVAL;
    TrackPoseBinding b;
    if (!track_pose_params(b, iters, huber_px, inlier_px, min_points))
        return fail(ctx, DVO_EINVAL, "track poses: iters <= 32, min_points >= 3, no NaN");
    return test_tracks_run(ctx, lm, count, mq, mt, m, rec, pairs, cap, stride, kp_cap, cap_out, link, scale, K, &b, pose);
}

int dvo_test_track_refine(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                          const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                          int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                          int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, int rf_views,
                          int rf_iters, double rf_huber_px, double rf_inlier_px, int use_poses,
                          dvo_landmark_refined* refined, dvo_track_id* id) {
    if (!ctx || !K || !pose || (!refined && !id)) return DVO_EINVAL;
    TrackPoseBinding b;
    if (!track_pose_params(b, iters, huber_px, inlier_px, min_points))
        return fail(ctx, DVO_EINVAL, "track poses: iters <= 32, min_points >= 3, no NaN");
    TrackRefineBinding r;
    if (!track_refine_params(r, rf_views, rf_iters, rf_huber_px, rf_inlier_px))
        return fail(ctx, DVO_EINVAL, "track refine: views 3..8, iters <= 16, no NaN");
    r.use_pose = use_poses != 0;
    return test_tracks_run(ctx, lm, count, mq, mt, m, rec, pairs, cap, stride, kp_cap, cap_out, link, scale, K, &b, pose,
                           &r, refined, id);
}

int dvo_test_track_bundle(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                          const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                          int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                          int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, int bd_views,
                          int bd_iters, double bd_lambda, double bd_huber_px, double bd_inlier_px, int bd_min_points,
                          int use_poses, dvo_track_bundle* bundle, dvo_landmark_refined* points) {
    if (!ctx || !K || !pose || (!bundle && !points)) return DVO_EINVAL;
    TrackPoseBinding b;
    if (!track_pose_params(b, iters, huber_px, inlier_px, min_points))
        return fail(ctx, DVO_EINVAL, "track poses: iters <= 32, min_points >= 3, no NaN");
    TrackBundleBinding d;
    if (!track_bundle_params(d, bd_views, bd_iters, bd_lambda, bd_huber_px, bd_inlier_px, bd_min_points))
        return fail(ctx, DVO_EINVAL, "track bundle: views 2..8, iters <= 16, min_points >= 6, no NaN");
    d.use_pose = use_poses != 0;
    return test_tracks_run(ctx, lm, count, mq, mt, m, rec, pairs, cap, stride, kp_cap, cap_out, link, scale, K, &b, pose,
                           nullptr, nullptr, nullptr, &d, bundle, points);
}

int dvo_test_track_pnp(dvo_ctx* ctx, const dvo_landmark* lm, const int32_t* count, const int32_t* mq,
                       const int32_t* mt, const int32_t* m, const dvo_pair_record* rec, int pairs, int cap, int stride,
                       int kp_cap, int cap_out, const double* K, int iters, double huber_px, double inlier_px,
                       int min_points, int32_t* link, dvo_track_scale* scale, dvo_track_pose* pose, const float* xy2,
                       int pnp_hyps, int pnp_iters, double pnp_huber_px, double pnp_inlier_px, int pnp_min_points,
                       uint64_t pnp_seed, dvo_track_pnp* pnp, uint8_t* mask, int mask_cap) {
    if (!ctx || !K || !pose || !xy2 || !pnp) return DVO_EINVAL;
    TrackPoseBinding b;
    if (!track_pose_params(b, iters, huber_px, inlier_px, min_points))
        return fail(ctx, DVO_EINVAL, "track poses: iters <= 32, min_points >= 3, no NaN");
    TrackPnpBinding n;
    if (!track_pnp_params(n, pnp_hyps, pnp_iters, pnp_huber_px, pnp_inlier_px, pnp_min_points, pnp_seed) ||
        (mask && mask_cap < 1))
        return fail(ctx, DVO_EINVAL, "track pnp: hyps <= 512, iters <= 32, min_points >= 4, mask_cap >= 1 with a mask, no NaN");
    n.mask_cap = mask ? mask_cap : 0;
    return test_tracks_run(ctx, lm, count, mq, mt, m, rec, pairs, cap, stride, kp_cap, cap_out, link, scale, K, &b, pose,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, xy2, pnp, mask);
}

int dvo_test_five_point(dvo_ctx* ctx, const double* q1, const double* q2, double* models, int* n) {
    if (!ctx || !q1 || !q2 || !models || !n) return DVO_EINVAL;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    double* dq = mem.dev<double>(20);
    double* dm = mem.dev<double>(90);
    int* dn = mem.dev<int>(2);
    HIP_TRY(mem.error());
    double q[20];
    for (int i = 0; i < 5; ++i) {
        q[4 * i] = q1[2 * i];
        q[4 * i + 1] = q1[2 * i + 1];
        q[4 * i + 2] = q2[2 * i];
        q[4 * i + 3] = q2[2 * i + 1];
    }
    HIP_TRY(hipMemcpy(dq, q, sizeof(q), hipMemcpyHostToDevice));
    HIP_TRY(launch_test_five_point(dq, dm, dn, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(n, dn, sizeof(int), hipMemcpyDeviceToHost));
    if (*n > 0) HIP_TRY(hipMemcpy(models, dm, (size_t)*n * 72, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_test_sampson(dvo_ctx* ctx, const double* E, const double* pts, int n, float t, int8_t* dec,
                     uint8_t* exact) {
    if (!ctx || !E || n < 0 || (n > 0 && (!pts || !dec || !exact))) return DVO_EINVAL;
    if (n == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallMem mem(ctx->call, ctx->stream);
    double* dE = mem.dev<double>(9);
    double* dp = mem.dev<double>((size_t)n * 4);
    int8_t* dd = mem.dev<int8_t>(n);
    uint8_t* dx = mem.dev<uint8_t>(n);
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpy(dE, E, 9 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp, pts, (size_t)n * 32, hipMemcpyHostToDevice));
    HIP_TRY(launch_test_sampson(dE, dp, n, t, dd, dx, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(dec, dd, (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(exact, dx, (size_t)n, hipMemcpyDeviceToHost));
    return DVO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Image pre-processing: cv.getOptimalNewCameraMatrix / cv.undistort
// (visual_odometry_v3.py:110-135).
namespace {

int load_dist12(dvo_ctx* ctx, const double* dist, int ndist, double* k) {
    for (int i = 0; i < 12; ++i) k[i] = 0.0;
    if (ndist < 0 || (ndist > 0 && !dist)) return fail(ctx, DVO_EINVAL, "bad distortion coefficients");
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8 || ndist == 12))
        return fail(ctx, DVO_EINVAL, "distortion must have 4, 5, 8 or 12 coefficients (tilt models unsupported)");
    for (int i = 0; i < ndist; ++i) k[i] = dist[i];
    return DVO_OK;
}

// undistort.dispatch.cpp cvUndistortPointsInternal (R = P = I, 5 iterations),
// float points in and out.
void undistort_points_f(float* pts, int n, const double* A, const double* k) {
    const double fx = A[0], fy = A[4], ifx = 1. / fx, ify = 1. / fy, cx = A[2], cy = A[5];
    for (int i = 0; i < n; ++i) {
        double x = pts[2 * i], y = pts[2 * i + 1];
        const double u = x, v = y;
        x = (x - cx) * ifx;
        y = (y - cy) * ify;
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; ++j) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            if (icdist < 0) {
                x = (u - cx) * ifx;
                y = (v - cy) * ify;
                break;
            }
            const double dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
            const double dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
        const double ww = 1. / (0. * x + 0. * y + 1.);
        pts[2 * i] = (float)((1. * x + 0. * y + 0.) * ww);
        pts[2 * i + 1] = (float)((0. * x + 1. * y + 0.) * ww);
    }
}

// Mat::inv(DECOMP_LU) of a 3x3 (LU with partial pivoting on [A | I]).
bool inv3(const double* M, double* out) {
    double A[9], b[9];
    std::memcpy(A, M, sizeof(A));
    for (int i = 0; i < 9; ++i) b[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++) {
        int k = i;
        for (int j = i + 1; j < 3; j++)
            if (std::fabs(A[j * 3 + i]) > std::fabs(A[k * 3 + i])) k = j;
        if (std::fabs(A[k * 3 + i]) < DBL_EPSILON * 100) return false;
        if (k != i) {
            for (int j = i; j < 3; j++) std::swap(A[i * 3 + j], A[k * 3 + j]);
            for (int j = 0; j < 3; j++) std::swap(b[i * 3 + j], b[k * 3 + j]);
        }
        const double d = -1 / A[i * 3 + i];
        for (int j = i + 1; j < 3; j++) {
            const double alpha = A[j * 3 + i] * d;
            for (int c = i + 1; c < 3; c++) A[j * 3 + c] += alpha * A[i * 3 + c];
            for (int c = 0; c < 3; c++) b[j * 3 + c] += alpha * b[i * 3 + c];
        }
    }
    for (int i = 2; i >= 0; i--)
        for (int j = 0; j < 3; j++) {
            double s = b[i * 3 + j];
            for (int k = i + 1; k < 3; k++) s -= A[i * 3 + k] * b[k * 3 + j];
            b[i * 3 + j] = s / A[i * 3 + i];
        }
    std::memcpy(out, b, sizeof(b));
    return true;
}

}  // namespace

struct dvo_undistort {
    dvo_ctx* ctx = nullptr;
    UndistortGeom U{};
    DeviceAllocs mem;
    double* d_ir = nullptr;
    int16_t* d_xy = nullptr;
    uint16_t* d_frac = nullptr;
};

int dvo_get_optimal_new_camera_matrix(const double* K, const double* dist, int ndist, int w, int h, double alpha,
                                      int new_w, int new_h, double* newK) {
    if (!K || !newK || w <= 0 || h <= 0) return DVO_EINVAL;
    double k[12];
    if (load_dist12(nullptr, dist, ndist, k)) return DVO_EINVAL;
    if (new_w * new_h == 0) {
        new_w = w;
        new_h = h;
    }
    // calibration.cpp icvGetRectangles: a 9 x 9 grid over the image, undistorted
    const int N = 9;
    float pts[2 * N * N];
    for (int y = 0, i = 0; y < N; y++)
        for (int x = 0; x < N; x++, i++) {
            pts[2 * i] = (float)x * w / (N - 1);
            pts[2 * i + 1] = (float)y * h / (N - 1);
        }
    undistort_points_f(pts, N * N, K, k);
    float iX0 = -FLT_MAX, iX1 = FLT_MAX, iY0 = -FLT_MAX, iY1 = FLT_MAX;
    float oX0 = FLT_MAX, oX1 = -FLT_MAX, oY0 = FLT_MAX, oY1 = -FLT_MAX;
    for (int y = 0, i = 0; y < N; y++)
        for (int x = 0; x < N; x++, i++) {
            const float px = pts[2 * i], py = pts[2 * i + 1];
            oX0 = std::min(oX0, px);
            oX1 = std::max(oX1, px);
            oY0 = std::min(oY0, py);
            oY1 = std::max(oY1, py);
            if (x == 0) iX0 = std::max(iX0, px);
            if (x == N - 1) iX1 = std::min(iX1, px);
            if (y == 0) iY0 = std::max(iY0, py);
            if (y == N - 1) iY1 = std::min(iY1, py);
        }
    const float in_w = iX1 - iX0, in_h = iY1 - iY0, ou_w = oX1 - oX0, ou_h = oY1 - oY0;
    std::memcpy(newK, K, 9 * sizeof(double));
    const double fx0 = (new_w - 1) / in_w, fy0 = (new_h - 1) / in_h, cx0 = -fx0 * iX0, cy0 = -fy0 * iY0;
    const double fx1 = (new_w - 1) / ou_w, fy1 = (new_h - 1) / ou_h, cx1 = -fx1 * oX0, cy1 = -fy1 * oY0;
    newK[0] = fx0 * (1 - alpha) + fx1 * alpha;
    newK[4] = fy0 * (1 - alpha) + fy1 * alpha;
    newK[2] = cx0 * (1 - alpha) + cx1 * alpha;
    newK[5] = cy0 * (1 - alpha) + cy1 * alpha;
    return DVO_OK;
}

int dvo_undistort_create(dvo_ctx* ctx, const double* K, const double* dist, int ndist, const double* newK, int w,
                         int h, dvo_undistort** out) {
    if (!ctx || !K || !out) return DVO_EINVAL;
    *out = nullptr;
    if (w < 2 || h < 2 || w >= 32768 || h >= 32768) return fail(ctx, DVO_EINVAL, "image size out of range");
    auto u = std::make_unique<dvo_undistort>();
    u->ctx = ctx;
    UndistortGeom& U = u->U;
    int rc = load_dist12(ctx, dist, ndist, U.dist);
    if (rc) return rc;
    U.w = w;
    U.h = h;
    std::memcpy(U.K, K, sizeof(U.K));
    // cv::undistort: stripes of min(max(1, 4096 / cols), rows) rows, principal
    // point of new_K shifted by the stripe's first row, one LU inverse each
    U.stripe = std::min(std::max(1, (1 << 12) / w), h);
    const int nstripes = (h + U.stripe - 1) / U.stripe;
    std::vector<double> ir((size_t)nstripes * 9);
    double Ar[9];
    std::memcpy(Ar, newK ? newK : K, sizeof(Ar));
    const double v0 = Ar[5];
    for (int s = 0; s < nstripes; ++s) {
        Ar[5] = v0 - (double)(s * U.stripe);
        if (!inv3(Ar, &ir[(size_t)s * 9])) return fail(ctx, DVO_EINVAL, "new camera matrix is singular");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    bool ok = u->mem.alloc(&u->d_ir, ir.size() * sizeof(double)) == hipSuccess &&
              u->mem.alloc(&u->d_xy, (size_t)w * h * 2 * sizeof(int16_t)) == hipSuccess &&
              u->mem.alloc(&u->d_frac, (size_t)w * h * sizeof(uint16_t)) == hipSuccess;
    if (ok) ok = hipMemcpy(u->d_ir, ir.data(), ir.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = launch_undistort_map(U, u->d_ir, u->d_xy, u->d_frac, ctx->stream) == hipSuccess;
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) return fail(ctx, DVO_EHIP, "undistort map construction failed");
    *out = u.release();
    return DVO_OK;
}

void dvo_undistort_destroy(dvo_undistort* u) {
    if (!u) return;
    hipSetDevice(u->ctx->device);
    delete u;
}

int dvo_undistort_apply(dvo_undistort* u, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch,
                        uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream) {
    if (!u) return DVO_EINVAL;
    dvo_ctx* ctx = u->ctx;
    if (n < 0 || (n > 0 && (!d_src || !d_dst)) || src_pitch < u->U.w || dst_pitch < u->U.w)
        return fail(ctx, DVO_EINVAL, "bad frame buffers");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    HIP_TRY(launch_undistort_remap(u->U, u->d_xy, u->d_frac, d_src, n, src_frame_stride, src_pitch, d_dst,
                                   dst_frame_stride, dst_pitch, s));
    return DVO_OK;
}

int dvo_undistort_get_map(dvo_undistort* u, int16_t* xy, uint16_t* frac) {
    if (!u || !xy || !frac) return DVO_EINVAL;
    dvo_ctx* ctx = u->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(xy, u->d_xy, (size_t)u->U.w * u->U.h * 2 * sizeof(int16_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(frac, u->d_frac, (size_t)u->U.w * u->U.h * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return DVO_OK;
}

int dvo_undistort_image(dvo_undistort* u, const uint8_t* img, int stride, uint8_t* out, int out_stride) {
    if (!u || !img || !out) return DVO_EINVAL;
    dvo_ctx* ctx = u->ctx;
    const int w = u->U.w, h = u->U.h;
    if (stride < w || out_stride < w) return fail(ctx, DVO_EINVAL, "bad strides");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = (w + 15) & ~15;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* dsrc = mem.dev<uint8_t>((size_t)pw * h);
    uint8_t* ddst = mem.dev<uint8_t>((size_t)pw * h);
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpy2DAsync(dsrc, pw, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_undistort_remap(u->U, u->d_xy, u->d_frac, dsrc, 1, 0, pw, ddst, 0, pw, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, ddst, pw, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_stream_process_undistorted(dvo_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                                   int64_t frame_stride, int stride, dvo_pair_record* d_records) {
    if (!s || !u) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if (u->U.w != s->cfg.width || u->U.h != s->cfg.height) return fail(ctx, DVO_EINVAL, "undistort size != stream size");
    if (n_frames < 1 || n_frames > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range");
    if (!d_frames || stride < s->cfg.width) return fail(ctx, DVO_EINVAL, "bad frame buffer");
    if (n_frames > 1 && !d_records) return fail(ctx, DVO_EINVAL, "null records");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = frame_pitch(s);
    const int64_t fs = (int64_t)pw * s->cfg.height;
    HIP_TRY(launch_undistort_remap(u->U, u->d_xy, u->d_frac, d_frames, n_frames, frame_stride, stride, s->d_frames, fs,
                                   pw, s->hs));
    return run_stream(s, s->d_frames, n_frames, fs, pw, d_records, false);
}

// ---------------------------------------------------------------------------
// Colour frames: cv.cvtColor(image_np, COLOR_BGR2GRAY) (v3:132), alone and fused
// into the undistortion that follows it (v3:133).  Kernels in color.hip.
// ---------------------------------------------------------------------------
namespace {

bool channels_ok(int channels) { return channels == 3 || channels == 4; }

// the colour batch of a stream call, then the stream's size against the undistorter's
int check_stream_bgr(dvo_stream* s, const dvo_undistort* u, const uint8_t* d_frames, int n_frames, int n_min,
                     int stride, int channels, const dvo_pair_record* d_records) {
    dvo_ctx* ctx = s->ctx;
    if (!channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 3 or 4");
    if (u && (u->U.w != s->cfg.width || u->U.h != s->cfg.height))
        return fail(ctx, DVO_EINVAL, "undistort size != stream size");
    if (n_frames < n_min || n_frames > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range");
    if (!d_frames || (int64_t)stride < (int64_t)s->cfg.width * channels)
        return fail(ctx, DVO_EINVAL, "bad frame buffer (null, or rows shorter than width * channels)");
    if (n_frames > 1 && !d_records) return fail(ctx, DVO_EINVAL, "null records");
    return DVO_OK;
}

// colour frames -> (undistorted) gray in the stream's slab on its HIP stream, then the batch
int run_stream_bgr(dvo_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames, int64_t frame_stride,
                   int stride, int channels, dvo_pair_record* d_records, bool drain) {
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = frame_pitch(s);
    const int64_t fs = (int64_t)pw * s->cfg.height;
    if (u)
        HIP_TRY(launch_undistort_remap_bgr(u->U, u->d_xy, u->d_frac, kGray14, d_frames, n_frames, frame_stride, stride,
                                           channels, s->d_frames, fs, pw, s->hs));
    else
        HIP_TRY(launch_bgr2gray(kGray14, d_frames, n_frames, frame_stride, stride, channels, s->cfg.width,
                                s->cfg.height, s->d_frames, fs, pw, s->hs));
    return run_stream(s, s->d_frames, n_frames, fs, pw, d_records, false, 1, drain);
}

}  // namespace

int dvo_bgr2gray(dvo_ctx* ctx, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch, int channels,
                 int w, int h, uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream) {
    if (!ctx) return DVO_EINVAL;
    if (!channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 3 or 4");
    if (w < 1 || h < 1 || w >= 32768 || h >= 32768) return fail(ctx, DVO_EINVAL, "image size out of range");
    if (n < 0 || (n > 0 && (!d_src || !d_dst))) return fail(ctx, DVO_EINVAL, "bad frame buffers");
    if (src_pitch < w * channels || dst_pitch < w)
        return fail(ctx, DVO_EINVAL, "bad pitches (source rows hold width * channels bytes, destination rows width)");
    if (n == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_bgr2gray(kGray14, d_src, n, src_frame_stride, src_pitch, channels, w, h, d_dst, dst_frame_stride,
                            dst_pitch, hip_stream ? (hipStream_t)hip_stream : ctx->stream));
    return DVO_OK;
}

int dvo_bgr2gray_image(dvo_ctx* ctx, const uint8_t* img, int w, int h, int stride, int channels, uint8_t* out,
                       int out_stride) {
    if (!ctx || !img || !out) return DVO_EINVAL;
    if (!channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 3 or 4");
    if (w < 1 || h < 1 || w >= 32768 || h >= 32768) return fail(ctx, DVO_EINVAL, "image size out of range");
    if (stride < w * channels || out_stride < w) return fail(ctx, DVO_EINVAL, "bad strides");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = (w + 15) & ~15, ps = (w * channels + 15) & ~15;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* dsrc = mem.dev<uint8_t>((size_t)ps * h);
    uint8_t* ddst = mem.dev<uint8_t>((size_t)pw * h);
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpy2DAsync(dsrc, ps, img, stride, (size_t)w * channels, h, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_bgr2gray(kGray14, dsrc, 1, 0, ps, channels, w, h, ddst, 0, pw, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, ddst, pw, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_undistort_apply_bgr(dvo_undistort* u, const uint8_t* d_src, int n, int64_t src_frame_stride, int src_pitch,
                            int channels, uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, void* hip_stream) {
    if (!u) return DVO_EINVAL;
    dvo_ctx* ctx = u->ctx;
    if (!channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 3 or 4");
    if (n < 0 || (n > 0 && (!d_src || !d_dst))) return fail(ctx, DVO_EINVAL, "bad frame buffers");
    if (src_pitch < u->U.w * channels || dst_pitch < u->U.w)
        return fail(ctx, DVO_EINVAL, "bad pitches (source rows hold width * channels bytes, destination rows width)");
    if (n == 0) return DVO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_undistort_remap_bgr(u->U, u->d_xy, u->d_frac, kGray14, d_src, n, src_frame_stride, src_pitch,
                                       channels, d_dst, dst_frame_stride, dst_pitch,
                                       hip_stream ? (hipStream_t)hip_stream : ctx->stream));
    return DVO_OK;
}

int dvo_undistort_image_bgr(dvo_undistort* u, const uint8_t* img, int stride, int channels, uint8_t* out,
                            int out_stride) {
    if (!u || !img || !out) return DVO_EINVAL;
    dvo_ctx* ctx = u->ctx;
    const int w = u->U.w, h = u->U.h;
    if (!channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 3 or 4");
    if (stride < w * channels || out_stride < w) return fail(ctx, DVO_EINVAL, "bad strides");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = (w + 15) & ~15, ps = (w * channels + 15) & ~15;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* dsrc = mem.dev<uint8_t>((size_t)ps * h);
    uint8_t* ddst = mem.dev<uint8_t>((size_t)pw * h);
    HIP_TRY(mem.error());
    HIP_TRY(hipMemcpy2DAsync(dsrc, ps, img, stride, (size_t)w * channels, h, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_undistort_remap_bgr(u->U, u->d_xy, u->d_frac, kGray14, dsrc, 1, 0, ps, channels, ddst, 0, pw,
                                       ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, ddst, pw, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DVO_OK;
}

int dvo_stream_process_bgr(dvo_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                           int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    int rc = check_stream_bgr(s, u, d_frames, n_frames, 1, stride, channels, d_records);
    if (rc) return rc;
    return run_stream_bgr(s, u, d_frames, n_frames, frame_stride, stride, channels, d_records, true);
}

int dvo_stream_submit_bgr(dvo_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                          int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    int rc = check_stream_bgr(s, u, d_frames, n_frames, 2, stride, channels, d_records);
    if (rc) return rc;
    return run_stream_bgr(s, u, d_frames, n_frames, frame_stride, stride, channels, d_records, false);
}

// ---------------------------------------------------------------------------
// JPEG frames: cv.imdecode (v3:127) of baseline JPEGs.  Parser in jpeg_parse.cpp, the entropy
// decoder (host and device) in jpeg_entropy.h, its many-lane form in jpeg_split.h, kernels in jpeg.hip.
// ---------------------------------------------------------------------------
struct dvo_jpeg {
    dvo_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0, group = 0;
    size_t frame_elems = 0;  // coefficients (and plane bytes) of the largest frame: 3 components at 16-pixel MCUs
    size_t coef_cap = 0;     // coefficients (and plane bytes) of a group
    size_t stage_cap = 0;    // scan bytes of a group
    size_t seg_cap = 0;      // segments of a group
    int gray_pitch = 0;
    DeviceAllocs mem;
    PinnedAllocs pin;
    // Pinned staging in two halves: the host fills one while the copies out of the other run.
    // ev[k] follows the last copy out of half k.
    uint8_t* h_bytes[2] = {nullptr, nullptr};
    jpeg::FramePlan* h_plans[2] = {nullptr, nullptr};
    jpeg::Segment* h_segs[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    int half = 0;
    int16_t* h_coef = nullptr;  // host entropy: a group's coefficients 
    hipEvent_t ev_coef = nullptr;
    bool ev_coef_used = false;
    int32_t* h_status = nullptr;  // [kMaxCall] the device statuses of the last call, after its copies ran
    uint8_t* d_bytes = nullptr;
    jpeg::FramePlan* d_plans = nullptr;
    jpeg::Segment* d_segs = nullptr;
    int16_t* d_coef = nullptr;
    uint8_t* d_planes = nullptr;
    uint8_t* d_gray = nullptr;  // a group of gray frames (decode -> undistort)
    int32_t* d_status = nullptr;
    int split_bytes = DVO_JPEG_SPLIT_BYTES_DEFAULT;
    int stream_entropy = DVO_JPEG_ENTROPY_DEVICE;  // what dvo_stream_*_jpeg decode with
    int32_t* d_split_info = nullptr;  // [3] of the last split call: most passes, segments split, fallbacks
    std::vector<jpeg::Segment> split_segs;  // a group's segments for the split kernel
    std::vector<int> host_status;  // per frame of the last call: what the host found
    std::vector<jpeg::Parsed> parsed;
    std::vector<int64_t> last_base, last_count;  // the last group's frames in d_coef
    hipStream_t last_stream = nullptr;
    static constexpr int kMaxCall = 65536;

    ~dvo_jpeg() {
        for (hipEvent_t e : {ev[0], ev[1], ev_coef})
            if (e) hipEventDestroy(e);
    }
};

namespace {

// Runs of split_bytes from which a segment gets a workgroup of its own.  A split segment costs its
// wave about 2 + passes walks of one run (guess, passes, write) where its one lane costs as many as
// it has runs, and up to 11 passes were seen at 128 to 256 bytes per run ("JPEG input").
constexpr uint32_t kSplitMinRuns = 16;

void fill_layout(const jpeg::Parsed& P, dvo_jpeg_layout* L) {
    const jpeg::FramePlan& p = P.plan;
    std::memset(L, 0, sizeof(*L));
    L->width = p.w, L->height = p.h, L->components = p.ncomp, L->sampling = p.hs << 4 | p.vs;
    L->restart_interval = p.restart, L->segments = (int)P.segs.size();
    for (int c = 0; c < p.ncomp; ++c) {
        L->blocks_w[c] = p.bw[c], L->blocks_h[c] = p.bh[c], L->coef_offset[c] = (int64_t)p.blk0[c] * 64;
        std::memcpy(L->quant[c], p.qt[c], sizeof(L->quant[c]));
    }
    L->coef_count = (int64_t)p.nblk * 64;
}

// every segment of a parsed file into zeroed coefficients; kOk or kCorrupt
int entropy_host(const jpeg::Parsed& P, const uint8_t* buf, int16_t* coef) {
    int st = P.scan_status;
    for (const jpeg::Segment& sg : P.segs)
        if (jpeg::decode_segment(P.plan, buf + sg.offset, sg.length, sg.mcu0, sg.nmcu, coef)) st = jpeg::kCorrupt;
    return st;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// n JPEGs -> n frames of out_channels bytes per pixel at d_dst, group after group on st; with u
// (out_channels 1) each group is decoded into j->d_gray and remapped into d_dst.  need_w/need_h:
// the size every frame must have (0: that of the first frame).
int jpeg_decode_impl(dvo_jpeg* j, const uint8_t* const* bufs, const int64_t* lens, int n, int out_channels,
                     uint8_t* d_dst, int64_t dst_fstride, int dst_pitch, int entropy, hipStream_t st, dvo_undistort* u,
                     int need_w, int need_h) {
    dvo_ctx* ctx = j->ctx;
    if (n < 0 || n > dvo_jpeg::kMaxCall) return fail(ctx, DVO_EINVAL, "frame count out of range (0..65536)");
    if (out_channels != 1 && out_channels != 3 && out_channels != 4)
        return fail(ctx, DVO_EINVAL, "out_channels must be 1, 3 or 4");
    if (entropy != DVO_JPEG_ENTROPY_HOST && entropy != DVO_JPEG_ENTROPY_DEVICE && entropy != DVO_JPEG_ENTROPY_DEVICE_SPLIT)
        return fail(ctx, DVO_EINVAL, "entropy must be DVO_JPEG_ENTROPY_HOST, _DEVICE or _DEVICE_SPLIT");
    if (n > 0 && (!bufs || !lens || !d_dst)) return fail(ctx, DVO_EINVAL, "null buffer");
    j->host_status.assign((size_t)n, DVO_OK);
    j->last_base.clear();
    j->last_count.clear();
    if (n == 0) return DVO_OK;
    // every header first: nothing is launched for a batch with a frame that cannot be decoded
    if ((int)j->parsed.size() < n) j->parsed.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
        if (!bufs[f] || lens[f] < 0) return fail(ctx, DVO_EINVAL, "frame " + std::to_string(f) + ": null buffer");
        jpeg::Parsed& P = j->parsed[(size_t)f];
        const int rc = jpeg::parse(bufs[f], (size_t)lens[f], &P);
        if (rc) return fail(ctx, rc, "frame " + std::to_string(f) + ": " + P.why);
        if (f == 0 && !need_w) need_w = P.plan.w, need_h = P.plan.h;
        if (P.plan.w != need_w || P.plan.h != need_h)
            return fail(ctx, DVO_EINVAL, "frame " + std::to_string(f) + ": size " + std::to_string(P.plan.w) + "x" +
                                             std::to_string(P.plan.h) + ", expected " + std::to_string(need_w) + "x" +
                                             std::to_string(need_h));
        if (P.plan.w > j->max_w || P.plan.h > j->max_h)
            return fail(ctx, DVO_EINVAL, "frame " + std::to_string(f) + ": larger than the decoder's maximum");
        if (align_up(P.scan_end - P.scan_begin, 16) > j->stage_cap)
            return fail(ctx, DVO_ECAP, "frame " + std::to_string(f) + ": scan larger than the decoder's staging buffer");
        j->host_status[(size_t)f] = P.scan_status;
    }
    if ((int64_t)dst_pitch < (int64_t)need_w * out_channels) return fail(ctx, DVO_EINVAL, "destination pitch too small");
    if (u && (out_channels != 1 || u->U.w != need_w || u->U.h != need_h))
        return fail(ctx, DVO_EINVAL, "undistort size != frame size");
    HIP_TRY(hipSetDevice(ctx->device));
    const bool on_host = entropy == DVO_JPEG_ENTROPY_HOST, split = entropy == DVO_JPEG_ENTROPY_DEVICE_SPLIT;
    // a segment of at least kSplitMinRuns runs of split_bytes goes to the split kernel, a shorter one keeps its lane
    const uint32_t split_from = split ? (uint32_t)j->split_bytes * kSplitMinRuns : 0;
    j->last_stream = st;
    HIP_TRY(hipMemsetAsync(j->d_status, 0, (size_t)n * sizeof(int32_t), st));
    if (split) HIP_TRY(hipMemsetAsync(j->d_split_info, 0, 3 * sizeof(int32_t), st));
    for (int f0 = 0; f0 < n;) {
        const int k = j->half;
        j->half ^= 1;
        if (j->ev_used[k]) HIP_TRY(hipEventSynchronize(j->ev[k]));
        // the group: up to `group` frames whose scans fit the staging half
        int nf = 0, nseg = 0, max_nblk = 0;
        uint32_t longest = 0;
        j->split_segs.clear();
        size_t bytes = 0;
        int64_t elems = 0;
        j->last_base.clear();
        j->last_count.clear();
        while (f0 + nf < n && nf < j->group) {
            jpeg::Parsed& P = j->parsed[(size_t)(f0 + nf)];
            const size_t sb = P.scan_end - P.scan_begin;
            if (bytes + align_up(sb, 16) > j->stage_cap || (size_t)elems + (size_t)P.plan.nblk * 64 > j->coef_cap ||
                (size_t)nseg + j->split_segs.size() + P.segs.size() > (size_t)0x7FFFFFFF)
                break;
            P.plan.base = elems;
            j->h_plans[k][nf] = P.plan;
            if (!on_host) {
                std::memcpy(j->h_bytes[k] + bytes, bufs[f0 + nf] + P.scan_begin, sb);
                for (const jpeg::Segment& sg : P.segs) {
                    const jpeg::Segment g{nf, (uint32_t)(bytes + (sg.offset - P.scan_begin)), sg.length, sg.mcu0, sg.nmcu};
                    if (split && sg.length >= split_from) {
                        j->split_segs.push_back(g);
                        longest = std::max(longest, sg.length);
                    } else {
                        j->h_segs[k][nseg++] = g;
                    }
                }
            }
            j->last_base.push_back(elems);
            j->last_count.push_back((int64_t)P.plan.nblk * 64);
            bytes += align_up(sb, 16);
            elems += (int64_t)P.plan.nblk * 64;
            max_nblk = std::max(max_nblk, P.plan.nblk);
            ++nf;
        }
        HIP_TRY(hipMemcpyAsync(j->d_plans, j->h_plans[k], (size_t)nf * sizeof(jpeg::FramePlan), hipMemcpyHostToDevice, st));
        if (on_host) {
            if (j->ev_coef_used) HIP_TRY(hipEventSynchronize(j->ev_coef));
            std::memset(j->h_coef, 0, (size_t)elems * sizeof(int16_t));
            for (int i = 0; i < nf; ++i) {
                const jpeg::Parsed& P = j->parsed[(size_t)(f0 + i)];
                if (entropy_host(P, bufs[f0 + i], j->h_coef + P.plan.base)) j->host_status[(size_t)(f0 + i)] = DVO_ECORRUPT;
            }
            HIP_TRY(hipMemcpyAsync(j->d_coef, j->h_coef, (size_t)elems * sizeof(int16_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipEventRecord(j->ev_coef, st));
            j->ev_coef_used = true;
        } else {
            HIP_TRY(hipMemsetAsync(j->d_coef, 0, (size_t)elems * sizeof(int16_t), st));
            if (bytes) HIP_TRY(hipMemcpyAsync(j->d_bytes, j->h_bytes[k], bytes, hipMemcpyHostToDevice, st));
            // one list: the one-lane segments, then the split ones
            const int nsplit = (int)j->split_segs.size();
            if (nsplit) std::memcpy(j->h_segs[k] + nseg, j->split_segs.data(), (size_t)nsplit * sizeof(jpeg::Segment));
            if (nseg + nsplit)
                HIP_TRY(hipMemcpyAsync(j->d_segs, j->h_segs[k], (size_t)(nseg + nsplit) * sizeof(jpeg::Segment),
                                       hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipEventRecord(j->ev[k], st));
        j->ev_used[k] = true;
        if (!on_host) {
            HIP_TRY(launch_jpeg_entropy(j->d_plans, j->d_segs, nseg, j->d_bytes, j->d_coef, j->d_status + f0, st));
            if (!j->split_segs.empty())
                HIP_TRY(launch_jpeg_entropy_split(j->d_plans, j->d_segs + nseg, (int)j->split_segs.size(), j->split_bytes,
                                                  (int)jpeg::split_count(longest, (uint32_t)j->split_bytes), j->d_bytes,
                                                  j->d_coef, j->d_status + f0, j->d_split_info, st));
        }
        HIP_TRY(launch_jpeg_idct(j->d_plans, nf, max_nblk, j->d_coef, j->d_planes, st));
        uint8_t* dst = d_dst + (int64_t)f0 * dst_fstride;
        if (u) {
            const int64_t gfs = (int64_t)j->gray_pitch * j->max_h;
            HIP_TRY(launch_jpeg_color(kGray14, j->d_plans, nf, need_w, need_h, j->d_planes, 1, j->d_gray, gfs,
                                      j->gray_pitch, st));
            HIP_TRY(launch_undistort_remap(u->U, u->d_xy, u->d_frac, j->d_gray, nf, gfs, j->gray_pitch, dst, dst_fstride,
                                           dst_pitch, st));
        } else {
            HIP_TRY(launch_jpeg_color(kGray14, j->d_plans, nf, need_w, need_h, j->d_planes, out_channels, dst,
                                      dst_fstride, dst_pitch, st));
        }
        f0 += nf;
    }
    HIP_TRY(hipMemcpyAsync(j->h_status, j->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return DVO_OK;
}

int check_stream_jpeg(dvo_stream* s, dvo_jpeg* j, const dvo_undistort* u, const uint8_t* const* bufs,
                      const int64_t* lens, int n, int n_min, const dvo_pair_record* d_records) {
    dvo_ctx* ctx = s->ctx;
    if (!j) return fail(ctx, DVO_EINVAL, "null decoder");
    if (j->ctx->device != ctx->device) return fail(ctx, DVO_EINVAL, "decoder and stream are on different devices");
    if (u && (u->U.w != s->cfg.width || u->U.h != s->cfg.height))
        return fail(ctx, DVO_EINVAL, "undistort size != stream size");
    if (n < n_min || n > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range");
    if (!bufs || !lens) return fail(ctx, DVO_EINVAL, "null buffer");
    if (n > 1 && !d_records) return fail(ctx, DVO_EINVAL, "null records");
    return DVO_OK;
}

int run_stream_jpeg(dvo_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs, const int64_t* lens, int n,
                    dvo_pair_record* d_records, bool drain) {
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = frame_pitch(s);
    const int64_t fs = (int64_t)pw * s->cfg.height;
    const int rc = jpeg_decode_impl(j, bufs, lens, n, 1, s->d_frames, fs, pw, j->stream_entropy, s->hs, u,
                                    s->cfg.width, s->cfg.height);
    if (rc) return fail(ctx, rc, j->ctx->err);
    return run_stream(s, s->d_frames, n, fs, pw, d_records, false, 1, drain);
}

}  // namespace

int dvo_jpeg_probe(const uint8_t* buf, int64_t len, int* w, int* h, int* components, int* sampling) {
    if (!buf || len < 0) return DVO_EINVAL;
    jpeg::Parsed P;
    const int rc = jpeg::parse(buf, (size_t)len, &P);
    if (rc) return rc;
    if (w) *w = P.plan.w;
    if (h) *h = P.plan.h;
    if (components) *components = P.plan.ncomp;
    if (sampling) *sampling = P.plan.hs << 4 | P.plan.vs;
    return DVO_OK;
}

int dvo_jpeg_entropy_host(const uint8_t* buf, int64_t len, dvo_jpeg_layout* layout, int16_t* coef, int64_t cap,
                          int* status) {
    if (!buf || len < 0 || !layout) return DVO_EINVAL;
    jpeg::Parsed P;
    const int rc = jpeg::parse(buf, (size_t)len, &P);
    if (rc) return rc;
    fill_layout(P, layout);
    if (!coef) return DVO_OK;
    if (cap < layout->coef_count) return DVO_ECAP;
    std::memset(coef, 0, (size_t)layout->coef_count * sizeof(int16_t));
    const int st = entropy_host(P, buf, coef);
    if (status) *status = st;
    return DVO_OK;
}

int dvo_jpeg_entropy_split_host(const uint8_t* buf, int64_t len, int split_bytes, int16_t* coef, int64_t cap, int* status,
                                int* passes) {
    if (!buf || len < 0 || !coef || !jpeg::split_bytes_ok(split_bytes)) return DVO_EINVAL;
    jpeg::Parsed P;
    const int rc = jpeg::parse(buf, (size_t)len, &P);
    if (rc) return rc;
    const int64_t count = (int64_t)P.plan.nblk * 64;
    if (cap < count) return DVO_ECAP;
    std::memset(coef, 0, (size_t)count * sizeof(int16_t));
    int st = P.scan_status, most = 0;
    for (const jpeg::Segment& sg : P.segs) {
        int np = 0;
        if (jpeg::decode_segment_split(P.plan, buf + sg.offset, sg.length, sg.mcu0, sg.nmcu, coef, (uint32_t)split_bytes, &np))
            st = jpeg::kCorrupt;
        most = std::max(most, np);
    }
    if (status) *status = st;
    if (passes) *passes = most;
    return DVO_OK;
}

int dvo_jpeg_create(dvo_ctx* ctx, int max_w, int max_h, int group_frames, dvo_jpeg** out) {
    if (!ctx || !out) return DVO_EINVAL;
    *out = nullptr;
    if (max_w < 1 || max_h < 1 || max_w > 65535 || max_h > 65535) return fail(ctx, DVO_EINVAL, "maximum size out of range");
    if (group_frames < 1 || group_frames > 65535) return fail(ctx, DVO_EINVAL, "group_frames out of range (1..65535)");
    auto j = std::make_unique<dvo_jpeg>();
    j->ctx = ctx;
    j->max_w = max_w, j->max_h = max_h, j->group = group_frames;
    const size_t pw = align_up((size_t)max_w, 16), ph = align_up((size_t)max_h, 16);
    j->frame_elems = 3 * pw * ph;
    // A group is sized for 4:2:2 frames (two thirds of 4:4:4's coefficients) of half a byte per pixel
    // of scan; frames that need more close their group early, and one frame of any kind fits.
    const size_t G = (size_t)group_frames;
    j->coef_cap = std::max(G * (j->frame_elems / 3 * 2), j->frame_elems);
    // (segment offsets into a group's bytes are 32-bit: a larger scan is refused with DVO_ECAP)
    j->stage_cap = align_up(std::max(G * ((size_t)max_w * max_h / 2 + 4096), 4 * (size_t)max_w * max_h + 65536), 256);
    j->stage_cap = std::min(j->stage_cap, (size_t)0xFFFFFF00u);
    j->seg_cap = (size_t)group_frames * (pw / 8) * (ph / 8);  // at most one segment per MCU
    j->gray_pitch = (int)pw;
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    auto dev = [&](auto** p, size_t bytes) {
        if (e == hipSuccess) e = j->mem.alloc(p, bytes + 256);
    };
    auto pinned = [&](auto** p, size_t bytes) {
        if (e == hipSuccess) e = j->pin.alloc(p, bytes + 256);
    };
    dev(&j->d_bytes, j->stage_cap);
    dev(&j->d_plans, G * sizeof(jpeg::FramePlan));
    dev(&j->d_segs, j->seg_cap * sizeof(jpeg::Segment));
    dev(&j->d_coef, j->coef_cap * sizeof(int16_t));
    dev(&j->d_planes, j->coef_cap);
    dev(&j->d_gray, G * pw * (size_t)max_h);
    dev(&j->d_status, (size_t)dvo_jpeg::kMaxCall * sizeof(int32_t));
    dev(&j->d_split_info, 3 * sizeof(int32_t));
    for (int k = 0; k < 2; ++k) {
        pinned(&j->h_bytes[k], j->stage_cap);
        pinned(&j->h_plans[k], G * sizeof(jpeg::FramePlan));
        pinned(&j->h_segs[k], j->seg_cap * sizeof(jpeg::Segment));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&j->ev[k], hipEventDisableTiming);
    }
    pinned(&j->h_status, (size_t)dvo_jpeg::kMaxCall * sizeof(int32_t));
    pinned(&j->h_coef, j->coef_cap * sizeof(int16_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&j->ev_coef, hipEventDisableTiming);
    if (e != hipSuccess) return fail(ctx, DVO_EHIP, std::string("JPEG decoder buffers: ") + hipGetErrorString(e));
    std::memset(j->h_status, 0, (size_t)dvo_jpeg::kMaxCall * sizeof(int32_t));
    HIP_TRY(hipMemset(j->d_split_info, 0, 3 * sizeof(int32_t)));
    *out = j.release();
    return DVO_OK;
}

void dvo_jpeg_destroy(dvo_jpeg* j) {
    if (!j) return;
    hipSetDevice(j->ctx->device);
    delete j;
}

int dvo_jpeg_decode(dvo_jpeg* j, const uint8_t* const* bufs, const int64_t* lens, int n, int out_channels,
                    uint8_t* d_dst, int64_t dst_frame_stride, int dst_pitch, int entropy, void* hip_stream) {
    if (!j) return DVO_EINVAL;
    return jpeg_decode_impl(j, bufs, lens, n, out_channels, d_dst, dst_frame_stride, dst_pitch, entropy,
                            hip_stream ? (hipStream_t)hip_stream : j->ctx->stream, nullptr, 0, 0);
}

int dvo_jpeg_set_split(dvo_jpeg* j, int split_bytes) {
    if (!j) return DVO_EINVAL;
    if (!jpeg::split_bytes_ok(split_bytes)) return fail(j->ctx, DVO_EINVAL, "split_bytes must be a power of two in 16..4096");
    j->split_bytes = split_bytes;
    return DVO_OK;
}

int dvo_jpeg_get_split(dvo_jpeg* j, int* split_bytes) {
    if (!j || !split_bytes) return DVO_EINVAL;
    *split_bytes = j->split_bytes;
    return DVO_OK;
}

int dvo_jpeg_set_stream_entropy(dvo_jpeg* j, int entropy) {
    if (!j) return DVO_EINVAL;
    if (entropy != DVO_JPEG_ENTROPY_DEVICE && entropy != DVO_JPEG_ENTROPY_DEVICE_SPLIT)
        return fail(j->ctx, DVO_EINVAL, "the stream decodes with DVO_JPEG_ENTROPY_DEVICE or _DEVICE_SPLIT");
    j->stream_entropy = entropy;
    return DVO_OK;
}

int dvo_jpeg_get_split_info(dvo_jpeg* j, int* max_passes, int* segments, int* fallbacks) {
    if (!j) return DVO_EINVAL;
    dvo_ctx* ctx = j->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (j->last_stream) HIP_TRY(hipStreamSynchronize(j->last_stream));
    int32_t v[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(v, j->d_split_info, sizeof(v), hipMemcpyDeviceToHost));
    if (max_passes) *max_passes = v[0];
    if (segments) *segments = v[1];
    if (fallbacks) *fallbacks = v[2];
    return DVO_OK;
}

int dvo_jpeg_status(dvo_jpeg* j, int* st, int n) {
    if (!j || n < 0 || (n > 0 && !st)) return DVO_EINVAL;
    if (n > (int)j->host_status.size()) return fail(j->ctx, DVO_EINVAL, "more frames than the last call decoded");
    for (int i = 0; i < n; ++i) st[i] = j->host_status[(size_t)i] || j->h_status[i] ? DVO_ECORRUPT : DVO_OK;
    return DVO_OK;
}

int dvo_jpeg_decode_image(dvo_jpeg* j, const uint8_t* buf, int64_t len, int out_channels, uint8_t* out,
                          int out_stride) {
    if (!j || !buf || !out) return DVO_EINVAL;
    dvo_ctx* ctx = j->ctx;
    int w = 0, h = 0;
    const int prc = dvo_jpeg_probe(buf, len, &w, &h, nullptr, nullptr);
    if (prc) return fail(ctx, prc, "not a decodable JPEG");
    if (out_channels != 1 && out_channels != 3 && out_channels != 4)
        return fail(ctx, DVO_EINVAL, "out_channels must be 1, 3 or 4");
    if ((int64_t)out_stride < (int64_t)w * out_channels) return fail(ctx, DVO_EINVAL, "bad stride");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pitch = (w * out_channels + 15) & ~15;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* ddst = mem.dev<uint8_t>((size_t)pitch * h);
    HIP_TRY(mem.error());
    const int64_t len64 = len;
    int rc = jpeg_decode_impl(j, &buf, &len64, 1, out_channels, ddst, 0, pitch, DVO_JPEG_ENTROPY_HOST, ctx->stream,
                              nullptr, 0, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, ddst, pitch, (size_t)w * out_channels, h, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int st = 0;
    rc = dvo_jpeg_status(j, &st, 1);
    if (rc) return rc;
    return st ? fail(ctx, DVO_ECORRUPT, "frame 0: corrupt entropy-coded data") : DVO_OK;
}

int dvo_undistort_image_jpeg(dvo_undistort* u, dvo_jpeg* j, const uint8_t* buf, int64_t len, uint8_t* out,
                             int out_stride) {
    if (!u || !j || !buf || !out) return DVO_EINVAL;
    dvo_ctx* ctx = j->ctx;
    if (u->ctx->device != ctx->device) return fail(ctx, DVO_EINVAL, "decoder and undistorter are on different devices");
    const int w = u->U.w, h = u->U.h;
    if (out_stride < w) return fail(ctx, DVO_EINVAL, "bad stride");
    HIP_TRY(hipSetDevice(ctx->device));
    const int pw = (w + 15) & ~15;
    CallMem mem(ctx->call, ctx->stream);
    uint8_t* ddst = mem.dev<uint8_t>((size_t)pw * h);
    HIP_TRY(mem.error());
    const int64_t len64 = len;
    int rc = jpeg_decode_impl(j, &buf, &len64, 1, 1, ddst, 0, pw, DVO_JPEG_ENTROPY_HOST, ctx->stream, u, w, h);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, out_stride, ddst, pw, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int st = 0;
    rc = dvo_jpeg_status(j, &st, 1);
    if (rc) return rc;
    return st ? fail(ctx, DVO_ECORRUPT, "frame 0: corrupt entropy-coded data") : DVO_OK;
}

int dvo_stream_process_jpeg(dvo_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                            const int64_t* lens, int n, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    const int rc = check_stream_jpeg(s, j, u, bufs, lens, n, 1, d_records);
    if (rc) return rc;
    return run_stream_jpeg(s, j, u, bufs, lens, n, d_records, true);
}

int dvo_stream_submit_jpeg(dvo_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                           const int64_t* lens, int n, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    const int rc = check_stream_jpeg(s, j, u, bufs, lens, n, 2, d_records);
    if (rc) return rc;
    return run_stream_jpeg(s, j, u, bufs, lens, n, d_records, false);
}

// ---------------------------------------------------------------------------
// Raw input for the k-NN stream: colour (v3:132), distorted (v3:133) and JPEG (v3:127) frames are
// brought to gray in the stream's own slab on its HIP stream, and detection runs on the slab.
// ---------------------------------------------------------------------------
namespace {

size_t knn_raw_pitch(int width) { return ((size_t)width + 15) & ~(size_t)15; }

// what check_stream_bgr and check_stream_jpeg refuse, for a dvo_knn_stream
int check_knn_raw_common(dvo_knn_stream* s, const dvo_undistort* u, int n, const dvo_pair_record* d_records,
                         bool records_needed, bool slab_needed) {
    dvo_ctx* ctx = s->ctx;
    if (u && (u->U.w != s->cfg.width || u->U.h != s->cfg.height))
        return fail(ctx, DVO_EINVAL, "undistort size != stream size");
    if (u && u->ctx->device != ctx->device)
        return fail(ctx, DVO_EINVAL, "undistorter and stream are on different devices");
    if (n < 1 || n > s->cfg.max_frames) return fail(ctx, DVO_EINVAL, "n_frames out of range (1..max_frames)");
    if (records_needed && n > 1 && !d_records) return fail(ctx, DVO_EINVAL, "null records");
    if (slab_needed && !s->raw)
        return fail(ctx, DVO_EINVAL, "raw input is not enabled: call dvo_knn_stream_set_raw_input(stream, 1) first");
    return DVO_OK;
}

int check_knn_raw(dvo_knn_stream* s, const dvo_undistort* u, const uint8_t* d_frames, int n, int stride, int channels,
                  const dvo_pair_record* d_records, bool records_needed) {
    dvo_ctx* ctx = s->ctx;
    if (channels != 1 && !channels_ok(channels)) return fail(ctx, DVO_EINVAL, "channels must be 1, 3 or 4");
    if (!d_frames || (int64_t)stride < (int64_t)s->cfg.width * channels)
        return fail(ctx, DVO_EINVAL, "bad frame buffer (null, or rows shorter than width * channels)");
    return check_knn_raw_common(s, u, n, d_records, records_needed, channels != 1 || u);
}

int check_knn_jpeg(dvo_knn_stream* s, dvo_jpeg* j, const dvo_undistort* u, const uint8_t* const* bufs, const int64_t* lens,
                   int n, const dvo_pair_record* d_records, bool records_needed) {
    dvo_ctx* ctx = s->ctx;
    if (!j) return fail(ctx, DVO_EINVAL, "null decoder");
    if (j->ctx->device != ctx->device) return fail(ctx, DVO_EINVAL, "decoder and stream are on different devices");
    if (!bufs || !lens) return fail(ctx, DVO_EINVAL, "null buffer");
    return check_knn_raw_common(s, u, n, d_records, records_needed, true);
}

// the event a profiled raw-input call begins at: recorded before the input launch (-1: not profiled)
int knn_raw_begin(dvo_knn_stream* s, int* ev_in) {
    dvo_ctx* ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    *ev_in = -1;
    if (!s->profiling) return DVO_OK;
    *ev_in = s->first_ev == 0 ? 1 : 0;
    HIP_TRY(hipEventRecord(s->ev_in[*ev_in], ctx->stream));
    return DVO_OK;
}

// checked arguments: one launch into the slab, then detection there
int knn_detect_raw(dvo_knn_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n, int64_t frame_stride, int stride,
                   int channels, uint64_t* d_draws) {
    dvo_ctx* ctx = s->ctx;
    if (channels == 1 && !u) return knn_stream_detect_gray(s, d_frames, n, frame_stride, stride, d_draws);
    int ev_in = -1;
    const int rc = knn_raw_begin(s, &ev_in);
    if (rc) return rc;
    const int w = s->cfg.width, h = s->cfg.height, pw = s->raw_pitch;
    const int64_t fs = (int64_t)pw * h;
    hipStream_t st = ctx->stream;
    if (channels == 1)
        HIP_TRY(launch_undistort_remap(u->U, u->d_xy, u->d_frac, d_frames, n, frame_stride, stride, s->raw, fs, pw, st));
    else if (u)
        HIP_TRY(launch_undistort_remap_bgr(u->U, u->d_xy, u->d_frac, kGray14, d_frames, n, frame_stride, stride, channels,
                                           s->raw, fs, pw, st));
    else
        HIP_TRY(launch_bgr2gray(kGray14, d_frames, n, frame_stride, stride, channels, w, h, s->raw, fs, pw, st));
    return knn_stream_detect_gray(s, s->raw, n, fs, pw, d_draws, ev_in);
}

// checked arguments: the decoder writes (and with u remaps) into the slab, then detection there.
// A header the parser refuses returns before anything is launched or the stream's state changes.
int knn_detect_jpeg(dvo_knn_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs, const int64_t* lens,
                    int n, uint64_t* d_draws) {
    dvo_ctx* ctx = s->ctx;
    int ev_in = -1;
    int rc = knn_raw_begin(s, &ev_in);
    if (rc) return rc;
    const int pw = s->raw_pitch;
    const int64_t fs = (int64_t)pw * s->cfg.height;
    rc = jpeg_decode_impl(j, bufs, lens, n, 1, s->raw, fs, pw, j->stream_entropy, ctx->stream, u, s->cfg.width,
                          s->cfg.height);
    if (rc) return j->ctx == ctx ? rc : fail(ctx, rc, j->ctx->err);
    return knn_stream_detect_gray(s, s->raw, n, fs, pw, d_draws, ev_in);
}

}  // namespace

size_t dvo_knn_stream_raw_input_bytes(int width, int height, int max_frames) {
    if (width < 1 || height < 1 || max_frames < 1) return 0;
    return (size_t)max_frames * knn_raw_pitch(width) * (size_t)height;
}

int dvo_knn_stream_set_raw_input(dvo_knn_stream* s, int enable) {
    if (!s) return DVO_EINVAL;
    dvo_ctx* ctx = s->ctx;
    if ((enable != 0) == (s->raw != nullptr)) return DVO_OK;
    s->pending = 0;  // a detection waiting for dvo_knn_stream_finish is dropped
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the old slab may be in use
    s->raw_mem.release();
    s->raw = nullptr;
    s->raw_pitch = 0;
    if (!enable) return DVO_OK;
    const hipError_t he =
        s->raw_mem.alloc(&s->raw, dvo_knn_stream_raw_input_bytes(s->cfg.width, s->cfg.height, s->cfg.max_frames));
    if (he != hipSuccess) s->raw = nullptr;
    HIP_TRY(he);
    s->raw_pitch = (int)knn_raw_pitch(s->cfg.width);
    return DVO_OK;
}

int dvo_knn_stream_detect_raw(dvo_knn_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                              int64_t frame_stride, int stride, int channels, uint64_t* d_draws) {
    if (!s) return DVO_EINVAL;
    const int rc = check_knn_raw(s, u, d_frames, n_frames, stride, channels, nullptr, false);
    return rc ? rc : knn_detect_raw(s, u, d_frames, n_frames, frame_stride, stride, channels, d_draws);
}

int dvo_knn_stream_process_raw(dvo_knn_stream* s, dvo_undistort* u, const uint8_t* d_frames, int n_frames,
                               int64_t frame_stride, int stride, int channels, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    int rc = check_knn_raw(s, u, d_frames, n_frames, stride, channels, d_records, true);
    if (!rc) rc = knn_detect_raw(s, u, d_frames, n_frames, frame_stride, stride, channels, nullptr);
    return rc ? rc : dvo_knn_stream_finish(s, d_records, nullptr, 1, 0);
}

int dvo_knn_stream_detect_jpeg(dvo_knn_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                               const int64_t* lens, int n, uint64_t* d_draws) {
    if (!s) return DVO_EINVAL;
    const int rc = check_knn_jpeg(s, j, u, bufs, lens, n, nullptr, false);
    return rc ? rc : knn_detect_jpeg(s, j, u, bufs, lens, n, d_draws);
}

int dvo_knn_stream_process_jpeg(dvo_knn_stream* s, dvo_jpeg* j, dvo_undistort* u, const uint8_t* const* bufs,
                                const int64_t* lens, int n, dvo_pair_record* d_records) {
    if (!s) return DVO_EINVAL;
    int rc = check_knn_jpeg(s, j, u, bufs, lens, n, d_records, true);
    if (!rc) rc = knn_detect_jpeg(s, j, u, bufs, lens, n, nullptr);
    return rc ? rc : dvo_knn_stream_finish(s, d_records, nullptr, 1, 0);
}

int dvo_jpeg_get_coefficients(dvo_jpeg* j, int frame, int16_t* out, int64_t cap, int64_t* n_out) {
    if (!j || !out || !n_out) return DVO_EINVAL;
    dvo_ctx* ctx = j->ctx;
    if (frame < 0 || frame >= (int)j->last_base.size()) return fail(ctx, DVO_EINVAL, "frame not in the last group");
    *n_out = j->last_count[(size_t)frame];
    if (cap < *n_out) return fail(ctx, DVO_ECAP, "caller capacity too small");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(j->last_stream));
    HIP_TRY(hipMemcpy(out, j->d_coef + j->last_base[(size_t)frame], (size_t)*n_out * sizeof(int16_t),
                      hipMemcpyDeviceToHost));
    return DVO_OK;
}
