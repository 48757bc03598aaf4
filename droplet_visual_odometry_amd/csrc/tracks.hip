// Tracks (dvo.h dvo_stream_set_tracks): the landmarks of consecutive pairs joined on the keypoint
// they share, and the ratio of the two baselines from the shared points.
//
// Frame j is detected once, so pair p - 1's trainIdx and pair p's queryIdx index one keypoint
// array.  The kernels run when a set retires, right after its landmark kernels, on the full
// lists those left in LandmarkScratch (tile by tile: a landmark's ordinal is the landmarks of
// the tiles before its own plus its place inside the tile), never on the caller's capped slots:
//   track_table_kernel   each landmark's ordinal at its trainIdx of the pair's table (atomicMin:
//                        the smallest ordinal wins where the ratio test kept a train index twice);
//   track_link_kernel    pair p's landmark looks its queryIdx up in pair p - 1's table, writes
//                        the link to the caller's slot and compacts its ratio, in ordinal
//                        order (wave ballots and mbcnt ranks, as landmark_tile_kernel), into the
//                        pair's ratio array from the tile's first ordinal on;
//   track_select_kernel  a workgroup per pair: the tiles' ratios moved together, then an exact
//                        radix select on their 64-bit patterns (positive doubles order as
//                        unsigned integers), most significant byte first, for the three ranks.
// With a refine binding (dvo.h dvo_stream_set_track_refine) the link kernel also writes every
// landmark's full link at its ordinal, and after the pose kernel:
//   track_id_kernel      list ranking by pointer jumping: launch 0 turns a link into (age, ordinal
//                        reached), launch r joins it with the state its ancestor had after launch
//                        r - 1 (ping-pong), so ages double; the last launch writes the caller's ids;
//   track_refine_kernel  per (tile, pair): thread 0 forms the pair's window cameras in LDS, then
//                        each landmark walks at most views - 2 links, gathers its observations
//                        into registers and runs the header's steps and final pass.
// With a pose binding (dvo.h dvo_stream_set_track_poses) the link kernel also writes each linked
// landmark's 3-D to 2-D correspondence beside its ratio, and a fourth kernel follows:
//   track_pose_kernel    a workgroup per pair: the tiles' correspondences moved together, then
//                        the header's Gauss-Newton steps from the record's R and ratio * t: 27
//                        sums per step (lane sums, shuffles inside a wave, the four wave totals
//                        through LDS), the 6 x 6 LDL^T solve and the Cayley update on lane 0, the
//                        new pose and a stop flag broadcast through LDS; then the final pass.
// With a bundle binding (dvo.h dvo_stream_set_track_bundle) the link kernel writes the full links
// too, and last of all:
//   track_bundle_kernel  a workgroup per pair: thread 0 forms the window cameras in LDS; per step
//                        the landmarks are linearised 32 at a time, lane per landmark, their blocks
//                        (W, Y = W V^-1, the U and h terms, g) left in LDS, and every entry of the
//                        reduced system S, r (up to 903 + 42, four per lane) adds the tile's
//                        landmarks in ordinal order onto the value it keeps in registers; then the
//                        LDL^T of S column by column across lanes, the two triangular solves on
//                        lane 0, the landmarks' back-substitution (lane per landmark, the blocks
//                        formed again) and the cameras' Cayley updates; the cost before and after,
//                        the guard, the gauge division and the final pass, lane per landmark with
//                        the pair's sums added in ordinal order by one lane each.
// With a PnP binding (dvo.h dvo_stream_set_track_pnp), after all of these:
//   track_pnp_corr_kernel  per (tile of raw matches, pair): the matches whose queryIdx pair p - 1's
//                        table holds, compacted in match order with their 3-D point and pixel;
//   track_pnp_kernel     a workgroup per pair: P3P (p3p.h) on seeded samples, a lane per sample,
//                        64 samples a round, their poses in LDS; a wave per sample's poses counts
//                        the supporters with ballots; the best (count, sample, solution) per wave,
//                        merged by the header's tie rule; then the pose kernel's step over the
//                        winner's supporters and its final pass over all correspondences.
// The arithmetic is the header's, one rounding per operation (-ffp-contract=off).
#include "dvo_internal.h"
#include "p3p.h"

namespace dvo {

namespace {

__device__ __forceinline__ const LandmarkTmp& track_entry(const TrackArgs& a, int p, int tile, int j) {
    return a.L.tmp[((int64_t)p * a.tiles + tile) * kLandmarkTile + j];
}

__global__ __launch_bounds__(kLandmarkTile) void track_table_kernel(TrackArgs a) {
    const int p = blockIdx.y, tile = blockIdx.x, j = threadIdx.x;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    if (j >= tc[tile]) return;
    int before = 0;
    for (int t = 0; t < tile; ++t) before += tc[t];
    const int i = track_entry(a, p, tile, j).match;
    const int t = a.mt[((int64_t)p * a.idx_stride + i) * a.idx_step];
    if ((unsigned)t < (unsigned)a.kp_cap) atomicMin(a.table + (int64_t)p * a.kp_cap + t, before + j);
}

__global__ __launch_bounds__(kLandmarkTile) void track_link_kernel(TrackArgs a) {
    __shared__ int wtot[kLandmarkTile / 64];
    const int p = blockIdx.y, tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    int first = 0;  // the tile's first ordinal
    for (int t = 0; t < tile; ++t) first += tc[t];
    bool linked = false;
    double ratio = 0;
    TrackCorr corr;
    if (tid < tc[tile]) {
        const LandmarkTmp b = track_entry(a, p, tile, tid);
        int lk = -1;
        if (p >= 1) {
            const int q = a.mq[((int64_t)p * a.idx_stride + b.match) * a.idx_step];
            if ((unsigned)q < (unsigned)a.kp_cap) {
                const int v = a.table[(int64_t)(p - 1) * a.kp_cap + q];
                if (v != kTrackEmpty) lk = v;
            }
        }
        if (lk >= 0) {
            // ordinal lk of pair p - 1: its tile and its place there (the table holds landmarks only)
            const int32_t* tp = tc - a.tiles;
            int t = 0, rem = lk;
            while (t < a.tiles - 1 && rem >= tp[t]) rem -= tp[t++];
            const LandmarkTmp e = track_entry(a, p - 1, t, min(rem, kLandmarkTile - 1));  // (never clamps: lk is an ordinal)
            const double* R = a.rec[p - 1].R;
            const double* tv = a.rec[p - 1].t;
            double y[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = ((R[3 * k] * e.X + R[3 * k + 1] * e.Y) + R[3 * k + 2] * e.Z) + tv[k];
            const double num = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
            const double den = sqrt((b.X * b.X + b.Y * b.Y) + b.Z * b.Z);
            ratio = num / den;
            linked = true;
            if (a.corr) {  // the pose kernel's correspondence: y and the landmark's x2, y2 as normalize_kernel has them
                const double ax = 1. / a.fx, ay = 1. / a.fy, bx = -a.cx * ax, by = -a.cy * ay;
                const float* px = a.pts_f + ((int64_t)p * a.pts_stride + b.match) * 4;
                const double x2 = px[2], y2 = px[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) corr.y[k] = y[k];
                corr.nu = x2 * ax + bx;
                corr.nv = y2 * ay + by;
            }
        }
        const int o = first + tid;
        if (a.link && o < a.cap) a.link[(int64_t)p * a.cap + o] = lk;
        if (a.flink) a.flink[(int64_t)p * a.pts_stride + o] = lk;  // o < the pair's landmarks <= pts_stride
    }
    const unsigned long long bal = __ballot(linked);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kLandmarkTile / 64; ++w) {
        const int c = wtot[w];
        before += w < wave ? c : 0;
        total += c;
    }
    // first + before + rank < first + tc[tile] <= the pair's landmarks <= pts_stride
    if (linked) a.ratio[(int64_t)p * a.pts_stride + first + before + rank] = ratio;
    if (linked && a.corr) a.corr[(int64_t)p * a.pts_stride + first + before + rank] = corr;
    if (tid == 0) a.lcnt[(int64_t)p * a.tiles + tile] = total;
}

constexpr int kSelNT = 256;  // one thread per radix bin

__global__ __launch_bounds__(kSelNT) void track_select_kernel(TrackArgs a) {
    __shared__ unsigned long long keys[kTrackLds];
    __shared__ int hist[3][kSelNT];
    __shared__ int wsum[3][kSelNT / 64];
    __shared__ int sel_bin[3], sel_before[3];
    const int p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    const int32_t* lc = a.lcnt + (int64_t)p * a.tiles;
    int n = 0, n_prev = 0;
    for (int t = 0; t < a.tiles; ++t) {
        n += lc[t];
        if (p >= 1) n_prev += tc[t - a.tiles];
    }
    // the tiles' ratios together, in ordinal order: in LDS when they fit, else moved down in
    // place (a tile's target ends at or before its source starts, and the sources of the tiles
    // after it begin past its own)
    unsigned long long* g = reinterpret_cast<unsigned long long*>(a.ratio + (int64_t)p * a.pts_stride);
    unsigned long long* key = n <= kTrackLds ? keys : g;
    for (int t = 0, off = 0, first = 0; t < a.tiles; first += tc[t], ++t) {
        const int c = lc[t];
        if (c == 0) continue;  // the same for every thread
        const unsigned long long v = tid < c ? g[first + tid] : 0;
        __syncthreads();
        if (tid < c) key[off + tid] = v;
        __syncthreads();
        off += c;
    }
    int k[3] = {(n - 1) / 2, (n - 1) / 4, 3 * (n - 1) / 4};
    unsigned long long prefix[3] = {0, 0, 0};
    for (int shift = 56; shift >= 0 && n >= 1; shift -= 8) {
#pragma unroll
        for (int r = 0; r < 3; ++r) hist[r][tid] = 0;
        __syncthreads();
        const unsigned long long high = shift == 56 ? 0ull : ~0ull << (shift + 8);  // the bytes already fixed
        for (int i = tid; i < n; i += kSelNT) {
            const unsigned long long v = key[i];
            const int bin = (int)(v >> shift) & 255;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if ((v & high) == prefix[r]) atomicAdd(&hist[r][bin], 1);
        }
        __syncthreads();
        int c[3], incl[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            int v = c[r] = hist[r][tid];
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d) v += o;
            }
            incl[r] = v;
            if (lane == 63) wsum[r][wave] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            int add = 0;
            for (int w = 0; w < wave; ++w) add += wsum[r][w];
            const int hi = incl[r] + add, lo = hi - c[r];
            if (lo <= k[r] && k[r] < hi) {  // exactly one bin: the counts sum to more than k[r]
                sel_bin[r] = tid;
                sel_before[r] = lo;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            k[r] -= sel_before[r];
            prefix[r] |= (unsigned long long)sel_bin[r] << shift;
        }
    }
    if (tid == 0) {
        dvo_track_scale o;
        o.ratio = __longlong_as_double((long long)prefix[0]);
        o.q1 = __longlong_as_double((long long)prefix[1]);
        o.q3 = __longlong_as_double((long long)prefix[2]);
        o.n_common = p >= 1 ? n : -1;
        o.n_prev = n_prev;
        a.scale[p] = o;
    }
}

// ---- track poses (dvo.h dvo_stream_set_track_poses) ----------------------------------------------
constexpr int kPoseNT = 256;    // the header's 256 lanes
constexpr int kPoseTerms = 27;  // 21 of H's upper triangle, 6 of g

// step 2 of the header's sum order: lane 0 ends with the wave's total (the lanes at and above s
// add what the tree never reads)
__device__ __forceinline__ double pose_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s);
    return v;
}

// H d = -g by the header's LDL^T, S the 27 sums; false: a pivot not > 0 or a non-finite d
__device__ bool pose_solve(const double* S, double* d) {
    double H[6][6], L[6][6], D[6], z[6];
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) H[i][j] = S[q++];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * D[k];
        if (!(dj > 0)) return false;
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double x = H[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) x = x - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = x / dj;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double x = -S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) x = x - L[i][k] * z[k];
        z[i] = x;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) z[i] = z[i] / D[i];
    bool finite = true;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double x = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) x = x - L[k][i] * d[k];
        d[i] = x;
        finite = finite && isfinite(x);
    }
    return finite;
}

// R <- C R, t <- C t + d[3..6) with C the Cayley map of d[0..3) / 2, into o[12] (R row by row, then t)
__device__ void pose_update(const double* R, const double* t, const double* d, double* o) {
    const double vx = d[0] * 0.5, vy = d[1] * 0.5, vz = d[2] * 0.5;
    const double vv = (vx * vx + vy * vy) + vz * vz, den = 1 + vv;
    const double C[3][3] = {
        {((1 - vv) + 2 * (vx * vx)) / den, (2 * (vx * vy) - 2 * vz) / den, (2 * (vx * vz) + 2 * vy) / den},
        {(2 * (vx * vy) + 2 * vz) / den, ((1 - vv) + 2 * (vy * vy)) / den, (2 * (vy * vz) - 2 * vx) / den},
        {(2 * (vx * vz) - 2 * vy) / den, (2 * (vy * vz) + 2 * vx) / den, ((1 - vv) + 2 * (vz * vz)) / den}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (C[i][0] * R[j] + C[i][1] * R[3 + j]) + C[i][2] * R[6 + j];
        o[9 + i] = ((C[i][0] * t[0] + C[i][1] * t[1]) + C[i][2] * t[2]) + d[3 + i];
    }
}

// Correspondence k of a pair: from the LDS copy (y0, y1, y2, nu, nv) where the pair's fit, else from
// global memory (G: TrackCorr, or the PnP kernel's PnpCorr).
template <class G>
__device__ __forceinline__ void pose_corr(const double (*cs)[kTrackPoseLds], const G* g, bool in_lds, int k, double& y0,
                                          double& y1, double& y2, double& nu, double& nv) {
    if (in_lds) {
        y0 = cs[0][k], y1 = cs[1][k], y2 = cs[2][k], nu = cs[3][k], nv = cs[4][k];
    } else {
        const G& v = g[k];
        y0 = v.y[0], y1 = v.y[1], y2 = v.y[2], nu = v.nu, nv = v.nv;
    }
}

// The header's "One step" (dvo.h, track poses) over n correspondences, by all 256 threads: 27 sums
// (lane sums, shuffles inside a wave, the four wave totals through wsum), the LDL^T solve and the
// Cayley update on lane 0, the new pose and the stop flag broadcast through next / stop.  With kSel
// the j-th correspondence is g[j].sel (the PnP kernel's polish set), else j itself.  True: R, tv
// hold the new pose; false: the step failed and they are what they were.  Two barriers, reached by
// all threads; the next write to *stop lies behind the caller's next barrier.
template <class G, bool kSel>
__device__ __forceinline__ bool pose_step(const double (*cs)[kTrackPoseLds], const G* g, bool in_lds, int n, double* R,
                                          double* tv, double kh, double kh2, double (*wsum)[kPoseTerms], double* next,
                                          int* stop) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[kPoseTerms];
#pragma unroll
    for (int q = 0; q < kPoseTerms; ++q) acc[q] = 0.0;
    for (int j = tid; j < n; j += kPoseNT) {
        int k = j;
        if constexpr (kSel) k = g[j].sel;
        double y0, y1, y2, nu, nv;
        pose_corr(cs, g, in_lds, k, y0, y1, y2, nu, nv);
        const double P0 = ((R[0] * y0 + R[1] * y1) + R[2] * y2) + tv[0];
        const double P1 = ((R[3] * y0 + R[4] * y1) + R[5] * y2) + tv[1];
        const double P2 = ((R[6] * y0 + R[7] * y1) + R[8] * y2) + tv[2];
        const bool ok = P2 > 0;
        const double ia = 1 / P2, u = P0 * ia, v = P1 * ia;
        const double ru = u - nu, rv = v - nv, e2 = ru * ru + rv * rv;
        const double w = e2 <= kh2 ? 1.0 : kh / sqrt(e2);
        const double b = -(u * ia), c = -(v * ia);
        const double Ju[6] = {b * P1, ia * P2 - b * P0, -(ia * P1), ia, 0.0, b};
        const double Jv[6] = {c * P1 - ia * P2, -(c * P0), ia * P0, 0.0, ia, c};
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int jj = i; jj < 6; ++jj, ++q) {
                const double term = w * (Ju[i] * Ju[jj] + Jv[i] * Jv[jj]);
                acc[q] = acc[q] + (ok ? term : 0.0);
            }
#pragma unroll
        for (int i = 0; i < 6; ++i, ++q) {
            const double term = w * (Ju[i] * ru + Jv[i] * rv);
            acc[q] = acc[q] + (ok ? term : 0.0);
        }
    }
#pragma unroll
    for (int q = 0; q < kPoseTerms; ++q) {
        const double v = pose_wave_sum(acc[q]);
        if (lane == 0) wsum[wave][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double S[kPoseTerms], d[6];
#pragma unroll
        for (int q = 0; q < kPoseTerms; ++q) S[q] = ((wsum[0][q] + wsum[1][q]) + wsum[2][q]) + wsum[3][q];
        const bool solved = pose_solve(S, d);
        if (solved) pose_update(R, tv, d, next);
        *stop = solved ? 0 : 1;
    }
    __syncthreads();
    if (*stop) return false;  // the same for every thread
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = next[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = next[9 + i];
    return true;
}

// The header's final pass over n correspondences on the pose R, tv, by all 256 threads; mask
// (PnP only, or null): 1 at the match index of every inlier below mask_cap.  One barrier; after
// it thread 0 holds the pair's sum of the inliers' e, n_used and n_inliers.  wsum was last read
// before the caller's last barrier.
template <class G, bool kMask>
__device__ __forceinline__ void pose_final(const TrackArgs& a, const double (*cs)[kTrackPoseLds], const G* g, bool in_lds,
                                           int n, const double* R, const double* tv, double inlier_px,
                                           double (*wsum)[kPoseTerms], int (*wcnt)[2], uint8_t* mask, int mask_cap,
                                           double* sum, int* n_used, int* n_inliers) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double se = 0.0;
    int used = 0, inl = 0;
    const double in2 = inlier_px * inlier_px;
    for (int k = tid; k < n; k += kPoseNT) {
        double y0, y1, y2, nu, nv;
        pose_corr(cs, g, in_lds, k, y0, y1, y2, nu, nv);
        const double P0 = ((R[0] * y0 + R[1] * y1) + R[2] * y2) + tv[0];
        const double P1 = ((R[3] * y0 + R[4] * y1) + R[5] * y2) + tv[1];
        const double P2 = ((R[6] * y0 + R[7] * y1) + R[8] * y2) + tv[2];
        const bool ok = P2 > 0;
        const double ia = 1 / P2, u = P0 * ia, v = P1 * ia;
        const double ex = a.fx * (u - nu), ey = a.fy * (v - nv);
        const double e = ex * ex + ey * ey;
        const bool in = ok && e <= in2;
        used += ok;
        inl += in;
        se = se + (in ? e : 0.0);
        if constexpr (kMask) {
            if (mask && in && g[k].match < mask_cap) mask[g[k].match] = 1;
        }
    }
    se = pose_wave_sum(se);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        used += __shfl_down(used, s);
        inl += __shfl_down(inl, s);
    }
    if (lane == 0) {
        wsum[wave][0] = se;
        wcnt[wave][0] = used;
        wcnt[wave][1] = inl;
    }
    __syncthreads();
    if (tid == 0) {
        *sum = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
        *n_used = ((wcnt[0][0] + wcnt[1][0]) + wcnt[2][0]) + wcnt[3][0];
        *n_inliers = ((wcnt[0][1] + wcnt[1][1]) + wcnt[2][1]) + wcnt[3][1];
    }
}

// A workgroup per pair.  Every barrier is reached by all 256 threads: a NONE pair leaves before
// the first as a whole, and the trip counts (the tiles' lcnt, iters, the stop flag read after a
// barrier) are the same for every thread.
__global__ __launch_bounds__(kPoseNT) void track_pose_kernel(TrackArgs a) {
    __shared__ double cs[5][kTrackPoseLds];  // y0, y1, y2, nu, nv of the correspondences that fit
    __shared__ double wsum[kPoseNT / 64][kPoseTerms];
    __shared__ int wcnt[kPoseNT / 64][2];
    __shared__ double next[12];
    __shared__ int stop;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    const int32_t* lc = a.lcnt + (int64_t)p * a.tiles;
    int n = 0;
    for (int t = 0; t < a.tiles; ++t) n += lc[t];
    double R[9], tv[3];
    {
        const bool has = p >= 1 && n >= 1;  // a ratio to start from (pair 0 links nothing: n is 0 there)
        const double ratio = has ? a.scale[p].ratio : 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = has ? a.rec[p].R[i] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) tv[i] = has ? ratio * a.rec[p].t[i] : 0.0;
    }
    dvo_track_pose o;
    o.rms = 0;
    o.n_used = o.n_inliers = o.iters = 0;
    if (p == 0 || n < a.pose_min_points) {
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) o.R[i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) o.t[i] = tv[i];
            o.scale = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
            o.status = DVO_TRACK_POSE_NONE;
            a.pose[p] = o;
        }
        return;
    }
    // the tiles' correspondences together, in ordinal order, as the select kernel moves the ratios:
    // into LDS when they fit, else down in place
    TrackCorr* g = a.corr + (int64_t)p * a.pts_stride;
    const bool in_lds = n <= kTrackPoseLds;
    for (int t = 0, off = 0, first = 0; t < a.tiles; first += tc[t], ++t) {
        const int c = lc[t];
        if (c == 0) continue;  // the same for every thread
        TrackCorr v;
        if (tid < c) v = g[first + tid];
        __syncthreads();
        if (tid < c) {
            if (in_lds) {
#pragma unroll
                for (int i = 0; i < 3; ++i) cs[i][off + tid] = v.y[i];
                cs[3][off + tid] = v.nu;
                cs[4][off + tid] = v.nv;
            } else {
                g[off + tid] = v;
            }
        }
        __syncthreads();
        off += c;
    }
    const double kh = a.huber_px / ((a.fx + a.fy) / 2), kh2 = kh * kh;
    int status = DVO_TRACK_POSE_OK, it = 0;
    for (; it < a.pose_iters; ++it)
        if (!pose_step<TrackCorr, false>(cs, g, in_lds, n, R, tv, kh, kh2, wsum, next, &stop)) {
            status = DVO_TRACK_POSE_DEGENERATE;
            break;
        }
    // the final pass on the last pose
    double sum;
    pose_final<TrackCorr, false>(a, cs, g, in_lds, n, R, tv, a.inlier_px, wsum, wcnt, nullptr, 0, &sum, &o.n_used,
                                 &o.n_inliers);
    if (tid == 0) {
        o.rms = o.n_inliers > 0 ? sqrt(sum / (double)o.n_inliers) : 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.R[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o.t[i] = tv[i];
        o.scale = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
        o.iters = it;
        o.status = status;
        a.pose[p] = o;
    }
}

// ---- track ids and refined landmarks (dvo.h dvo_stream_set_track_refine) --------------------------
// Launch `round` of the list ranking.  A landmark of age g has followed g links and stands at
// ordinal ord of pair p - g (g <= p: a link exists only from pair 1 on); joining it with that
// landmark's state of the launch before adds the links that one had followed.  After launch r
// every chain of up to 2^r links is ranked to its end and longer ones stand 2^r links back.
__global__ __launch_bounds__(kLandmarkTile) void track_id_kernel(TrackArgs a, int round, int last) {
    const int p = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    if (tid >= tc[tile]) return;
    int first = 0;
    for (int t = 0; t < tile; ++t) first += tc[t];
    const int o = first + tid;
    const int64_t at = (int64_t)p * a.pts_stride + o;
    TrackRank r;
    if (round == 0) {
        const int lk = a.flink[at];
        r.age = lk >= 0 ? 1 : 0;
        r.ord = lk >= 0 ? lk : o;
    } else {
        const TrackRank* src = a.rank + (int64_t)((round - 1) & 1) * a.rank_stride;
        r = src[at];
        if (r.age > 0) {
            const TrackRank b = src[(int64_t)(p - r.age) * a.pts_stride + r.ord];
            r.age += b.age;
            r.ord = b.ord;
        }
    }
    if (!last) {
        (a.rank + (int64_t)(round & 1) * a.rank_stride)[at] = r;
    } else if (o < a.cap) {
        dvo_track_id id;
        id.root_pair = p - r.age;
        id.root_ord = r.ord;
        id.age = r.age;
        id.reserved = 0;
        a.id[(int64_t)p * a.cap + o] = id;
    }
}

// the unit motion of pair q (R row by row, d, rho)
__device__ void refine_motion(const TrackArgs& a, int use_pose, int q, double* R, double* d, double* rho) {
    if (use_pose && a.pose[q].status == DVO_TRACK_POSE_OK) {
        const dvo_track_pose& s = a.pose[q];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = s.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = s.t[i] / s.scale;
        *rho = s.scale;
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = a.rec[q].R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = a.rec[q].t[i];
        *rho = a.scale[q].ratio;
    }
}

// The header's window cameras of pair p into cam (view v: A row by row, then b): view 0 the
// identity, view 1 the pair's unit motion, view k + 1 camera (A_k, b_k) for k = 1..W <= views - 2.
// Returns W; *rho_p: the pair's own rho.
__device__ int window_cameras(const TrackArgs& a, int p, int views, int use_pose, double (*cam)[12], double* rho_p) {
    double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, b[3] = {0, 0, 0}, sigma = 1, R[9], d[3], rho;
#pragma unroll
    for (int i = 0; i < 9; ++i) cam[0][i] = A[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cam[0][9 + i] = 0.0;
    refine_motion(a, use_pose, p, R, d, rho_p);
#pragma unroll
    for (int i = 0; i < 9; ++i) cam[1][i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cam[1][9 + i] = d[i];
    int W = 0;
    for (int k = 1; k <= views - 2; ++k) {  // camera k goes to view k + 1 <= views - 1
        const int q = p - k;
        if (q < 0) break;
        refine_motion(a, use_pose, q + 1, R, d, &rho);
        if (!(rho > 0)) break;  // also where pair q or q + 1 has no landmarks: pair q + 1 links nothing
        sigma = sigma / rho;
        if (!isfinite(sigma)) break;
        refine_motion(a, use_pose, q, R, d, &rho);
        double An[9], c[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) An[3 * i + j] = (R[i] * A[j] + R[3 + i] * A[3 + j]) + R[6 + i] * A[6 + j];
            c[i] = b[i] - sigma * d[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) b[i] = (R[i] * c[0] + R[3 + i] * c[1]) + R[6 + i] * c[2];
#pragma unroll
        for (int i = 0; i < 9; ++i) cam[k + 1][i] = A[i] = An[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) cam[k + 1][9 + i] = b[i];
        W = k;
    }
    return W;
}

// H d = -g by the header's LDL^T at size 3, S the 6 + 3 sums; false: a pivot not > 0 or a non-finite d
__device__ bool refine_solve(const double* S, double* d) {
    double H[3][3], L[3][3], D[3], z[3];
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) H[i][j] = S[q++];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double dj = H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * D[k];
        if (!(dj > 0)) return false;
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 3; ++i) {
            double x = H[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) x = x - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = x / dj;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double x = -S[6 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) x = x - L[i][k] * z[k];
        z[i] = x;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = z[i] / D[i];
    bool finite = true;
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double x = z[i];
#pragma unroll
        for (int k = i + 1; k < 3; ++k) x = x - L[k][i] * d[k];
        d[i] = x;
        finite = finite && isfinite(x);
    }
    return finite;
}

// Per (tile, pair).  The one barrier is reached by all 256 threads (an empty tile leaves before it
// as a whole); after it every thread runs alone, its trip counts from the links, views and iters.
__global__ __launch_bounds__(kLandmarkTile) void track_refine_kernel(TrackArgs a) {
    __shared__ double cam[kTrackRefineMaxViews][12];  // view v: A row by row, then b
    __shared__ int win;                               // the window's length W
    const int p = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    if (tc[tile] == 0) return;
    if (tid == 0) {
        double rho;
        win = window_cameras(a, p, a.rf_views, a.rf_use_pose, cam, &rho);
    }
    __syncthreads();
    if (tid >= tc[tile]) return;
    int first = 0;
    for (int t = 0; t < tile; ++t) first += tc[t];
    const int o = first + tid;
    if (o >= a.cap) return;  // nothing but the slot is written
    const LandmarkTmp e = track_entry(a, p, tile, tid);
    const double ax = 1. / a.fx, ay = 1. / a.fy, bx = -a.cx * ax, by = -a.cy * ay;
    double nu[kTrackRefineMaxViews], nv[kTrackRefineMaxViews];
#pragma unroll
    for (int v = 0; v < kTrackRefineMaxViews; ++v) nu[v] = nv[v] = 0.0;
    {
        const float* px = a.pts_f + ((int64_t)p * a.pts_stride + e.match) * 4;
        nu[0] = (double)px[0] * ax + bx, nv[0] = (double)px[1] * ay + by;
        nu[1] = (double)px[2] * ax + bx, nv[1] = (double)px[3] * ay + by;
    }
    int nviews = 2;
    {
        const int maxk = min(a.rf_views - 2, win);  // maxk <= p: the window stops at pair 0
        int cur = o;                                // c_{k-1}'s ordinal in pair p - k + 1, -1 past the chain's end
#pragma unroll
        for (int k = 1; k <= kTrackRefineMaxViews - 2; ++k) {
            if (k <= maxk && cur >= 0) {
                cur = a.flink[(int64_t)(p - k + 1) * a.pts_stride + cur];
                if (cur >= 0) {
                    // ordinal cur of pair p - k: its tile and its place there, as the link kernel finds them
                    const int32_t* tp = tc - (int64_t)k * a.tiles;
                    int t = 0, rem = cur;
                    while (t < a.tiles - 1 && rem >= tp[t]) rem -= tp[t++];
                    const int mi = track_entry(a, p - k, t, min(rem, kLandmarkTile - 1)).match;  // (never clamps)
                    const float* px = a.pts_f + ((int64_t)(p - k) * a.pts_stride + mi) * 4;
                    nu[k + 1] = (double)px[0] * ax + bx, nv[k + 1] = (double)px[1] * ay + by;
                    nviews = k + 2;
                }
            }
        }
    }
    dvo_landmark_refined out;
    out.rms = 0.0;
    out.n_used = out.n_inliers = out.iters = 0;
    out.reserved = 0;
    double X[3] = {e.X, e.Y, e.Z};
    if (nviews < 3) {
        out.views = 2;
        out.status = DVO_TRACK_REFINE_NONE;
    } else {
        const double kh = a.rf_huber_px / ((a.fx + a.fy) / 2), kh2 = kh * kh;
        int status = DVO_TRACK_REFINE_OK, it = 0;
        for (; it < a.rf_iters; ++it) {
            int z = 0;  // opaque zero: the cameras are read from LDS every step, not held in 96 registers across the loop
            asm volatile("" : "+v"(z));
            double S[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) S[q] = 0.0;
#pragma unroll
            for (int v = 0; v < kTrackRefineMaxViews; ++v) {
                if (v < nviews) {
                    const double* C = cam[v] + z;
                    const double P0 = ((C[0] * X[0] + C[1] * X[1]) + C[2] * X[2]) + C[9];
                    const double P1 = ((C[3] * X[0] + C[4] * X[1]) + C[5] * X[2]) + C[10];
                    const double P2 = ((C[6] * X[0] + C[7] * X[1]) + C[8] * X[2]) + C[11];
                    const bool ok = P2 > 0;
                    const double ia = 1 / P2, u = P0 * ia, w_ = P1 * ia;
                    const double ru = u - nu[v], rv = w_ - nv[v], e2 = ru * ru + rv * rv;
                    const double w = e2 <= kh2 ? 1.0 : kh / sqrt(e2);
                    double Ju[3], Jv[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        Ju[j] = ia * (C[j] - u * C[6 + j]);
                        Jv[j] = ia * (C[3 + j] - w_ * C[6 + j]);
                    }
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = i; j < 3; ++j, ++q) {
                            const double term = w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
                            S[q] = S[q] + (ok ? term : 0.0);
                        }
#pragma unroll
                    for (int i = 0; i < 3; ++i, ++q) {
                        const double term = w * (Ju[i] * ru + Jv[i] * rv);
                        S[q] = S[q] + (ok ? term : 0.0);
                    }
                }
            }
            double d[3];
            if (!refine_solve(S, d)) {
                status = DVO_TRACK_REFINE_DEGENERATE;
                break;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) X[i] = X[i] + d[i];
        }
        // the final pass on the last X
        double se = 0.0;
        int used = 0, inl = 0;
        const double in2 = a.rf_inlier_px * a.rf_inlier_px;
#pragma unroll
        for (int v = 0; v < kTrackRefineMaxViews; ++v) {
            if (v < nviews) {
                const double* C = cam[v];
                const double P0 = ((C[0] * X[0] + C[1] * X[1]) + C[2] * X[2]) + C[9];
                const double P1 = ((C[3] * X[0] + C[4] * X[1]) + C[5] * X[2]) + C[10];
                const double P2 = ((C[6] * X[0] + C[7] * X[1]) + C[8] * X[2]) + C[11];
                const bool ok = P2 > 0;
                const double ia = 1 / P2, u = P0 * ia, w_ = P1 * ia;
                const double ex = a.fx * (u - nu[v]), ey = a.fy * (w_ - nv[v]);
                const double er = ex * ex + ey * ey;
                const bool in = ok && er <= in2;
                used += ok;
                inl += in;
                se = se + (in ? er : 0.0);
            }
        }
        out.views = nviews;
        out.n_used = used;
        out.n_inliers = inl;
        out.rms = inl > 0 ? sqrt(se / (double)inl) : 0.0;
        out.iters = it;
        out.status = status;
    }
    out.X = X[0], out.Y = X[1], out.Z = X[2];
    a.refined[(int64_t)p * a.cap + o] = out;
}

// ---- track bundle (dvo.h dvo_stream_set_track_bundle) ---------------------------------------------
constexpr int kBundleNT = 256;
constexpr int kBundleTile = 32;                      // landmarks linearised per tile
constexpr int kBundleCamF = 63;                      // per camera c >= 1: W 18, Y 18, U terms 21, h terms 6
constexpr int kBundleG = 7 * kBundleCamF;            // then g 3
constexpr int kBundleF = kBundleG + 4;               // 445 doubles per landmark: odd, so a tile's lanes spread over the banks
constexpr int kBundleMaxN = 6 * (kTrackRefineMaxViews - 1);  // 42 unknowns
constexpr int kBundleLd = kBundleMaxN + 1;
constexpr int kBundleEnt = 4;                        // entries per lane: 903 + 42 <= 4 * 256
static_assert(kBundleMaxN * (kBundleMaxN + 1) / 2 + kBundleMaxN <= kBundleEnt * kBundleNT, "entries");
static_assert(2 * kBundleNT <= kBundleTile * kBundleF, "the evaluation's two columns lie in the tile's blocks");

// landmark o of pair p's full list
__device__ __forceinline__ const LandmarkTmp& track_ordinal(const TrackArgs& a, int p, int o) {
    const int32_t* tp = a.L.tcnt + (int64_t)p * a.tiles;
    int t = 0, rem = o;
    while (t < a.tiles - 1 && rem >= tp[t]) rem -= tp[t++];
    return track_entry(a, p, t, min(rem, kLandmarkTile - 1));  // (never clamps: o is an ordinal)
}

// The views of landmark o of pair p over V cameras, as track_refine_kernel gathers them; returns their number.
__device__ __forceinline__ int bundle_views(const TrackArgs& a, int p, int o, int match, int V, double* nu, double* nv) {
    const double ax = 1. / a.fx, ay = 1. / a.fy, bx = -a.cx * ax, by = -a.cy * ay;
#pragma unroll
    for (int v = 0; v < kTrackRefineMaxViews; ++v) nu[v] = nv[v] = 0.0;
    {
        const float* px = a.pts_f + ((int64_t)p * a.pts_stride + match) * 4;
        nu[0] = (double)px[0] * ax + bx, nv[0] = (double)px[1] * ay + by;
        nu[1] = (double)px[2] * ax + bx, nv[1] = (double)px[3] * ay + by;
    }
    int nviews = 2, cur = o;
#pragma unroll
    for (int k = 1; k <= kTrackRefineMaxViews - 2; ++k) {
        if (k <= V - 2 && cur >= 0) {  // V - 2 <= p: the window stops at pair 0
            cur = a.flink[(int64_t)(p - k + 1) * a.pts_stride + cur];
            if (cur >= 0) {
                const int mi = track_ordinal(a, p - k, cur).match;
                const float* px = a.pts_f + ((int64_t)(p - k) * a.pts_stride + mi) * 4;
                nu[k + 1] = (double)px[0] * ax + bx, nv[k + 1] = (double)px[1] * ay + by;
                nviews = k + 2;
            }
        }
    }
    return nviews;
}

struct BundleView {
    double P0, P1, P2, ia, u, v, ru, rv, e2, w;
    bool ok;
};

__device__ __forceinline__ BundleView bundle_view(const double* C, const double* X, double nu, double nv, double kh,
                                                  double kh2) {
    BundleView r;
    r.P0 = ((C[0] * X[0] + C[1] * X[1]) + C[2] * X[2]) + C[9];
    r.P1 = ((C[3] * X[0] + C[4] * X[1]) + C[5] * X[2]) + C[10];
    r.P2 = ((C[6] * X[0] + C[7] * X[1]) + C[8] * X[2]) + C[11];
    r.ok = r.P2 > 0;
    r.ia = 1 / r.P2, r.u = r.P0 * r.ia, r.v = r.P1 * r.ia;
    r.ru = r.u - nu, r.rv = r.v - nv, r.e2 = r.ru * r.ru + r.rv * r.rv;
    r.w = r.e2 <= kh2 ? 1.0 : kh / sqrt(r.e2);
    return r;
}

// the point and camera Jacobians of a view
__device__ __forceinline__ void bundle_jx(const double* C, const BundleView& q, double* Ju, double* Jv) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Ju[j] = q.ia * (C[j] - q.u * C[6 + j]);
        Jv[j] = q.ia * (C[3 + j] - q.v * C[6 + j]);
    }
}
__device__ __forceinline__ void bundle_jc(const BundleView& q, double* Ju, double* Jv) {
    const double b = -(q.u * q.ia), c = -(q.v * q.ia);
    Ju[0] = b * q.P1, Ju[1] = q.ia * q.P2 - b * q.P0, Ju[2] = -(q.ia * q.P1), Ju[3] = q.ia, Ju[4] = 0.0, Ju[5] = b;
    Jv[0] = c * q.P1 - q.ia * q.P2, Jv[1] = -(c * q.P0), Jv[2] = q.ia * q.P0, Jv[3] = 0.0, Jv[4] = q.ia, Jv[5] = c;
}

// the header's LDL^T at size 3 of the damped V (upper triangle row by row): L10, L20, L21, D; false: a pivot not > 0
struct BundleLdl3 {
    double L10, L20, L21, D0, D1, D2;
};
__device__ __forceinline__ bool bundle_factor3(const double* V, BundleLdl3* f) {
    f->D0 = V[0];
    f->L10 = V[1] / f->D0;
    f->L20 = V[2] / f->D0;
    f->D1 = V[3] - (f->L10 * f->L10) * f->D0;
    f->L21 = (V[4] - (f->L20 * f->L10) * f->D0) / f->D1;
    f->D2 = (V[5] - (f->L20 * f->L20) * f->D0) - (f->L21 * f->L21) * f->D1;
    return f->D0 > 0 && f->D1 > 0 && f->D2 > 0;
}
// V x = q by the factor's two triangular solves
__device__ __forceinline__ void bundle_apply3(const BundleLdl3& f, double q0, double q1, double q2, double* x) {
    const double z0 = q0, z1 = q1 - f.L10 * z0, z2 = (q2 - f.L20 * z0) - f.L21 * z1;
    const double y0 = z0 / f.D0, y1 = z1 / f.D1, y2 = z2 / f.D2;
    x[2] = y2;
    x[1] = y1 - f.L21 * x[2];
    x[0] = (y0 - f.L10 * x[1]) - f.L20 * x[2];
}

struct BundleShared {
    double blk[kBundleTile * kBundleF];        // a tile's blocks; the evaluation's two columns
    double S[kBundleMaxN * kBundleLd];         // the reduced system's upper triangle, L below it
    double D[kBundleMaxN], r[kBundleMaxN], y[kBundleMaxN], d[kBundleMaxN];
    double cam[kTrackRefineMaxViews][12], cam0[kTrackRefineMaxViews][12];
    double res[2], rho;
    int lnv[kBundleTile];  // a tile landmark's views, 0 where its factorisation failed
    int cnt[2], win, fail;
};

// The Huber cost and the final-pass sums of a state into sh.res (cost, the inliers' squared pixels)
// and sh.cnt (views, inliers): lane per landmark, 256 at a time, their values added in ordinal order
// by lane 0 and lane 64.  raw: the landmarks' own X, else bd_x.  write: also the caller's slots
// (kept: the steps and status of a kept fit).  Every barrier is reached by all threads.
__device__ void bundle_eval(const TrackArgs& a, BundleShared& sh, int p, int n, int V, double kh, double kh2, bool raw,
                            bool write, bool kept, int taken) {
    const int tid = threadIdx.x;
    double* evc = sh.blk;
    double* evs = sh.blk + kBundleNT;
    if (tid == 0) sh.cnt[0] = sh.cnt[1] = 0;
    __syncthreads();
    BundlePoint* bx = a.bd_x + (int64_t)p * a.pts_stride;
    const double in2 = a.bd_inlier_px * a.bd_inlier_px;
    double acc = 0.0;
    for (int base = 0; base < n; base += kBundleNT) {
        const int o = base + tid;
        if (o < n) {
            const LandmarkTmp e = track_ordinal(a, p, o);
            double X[3] = {e.X, e.Y, e.Z};
            int steps = 0;
            if (!raw) {
                const BundlePoint b = bx[o];
                X[0] = b.X[0], X[1] = b.X[1], X[2] = b.X[2];
                steps = b.steps;
            }
            double nu[kTrackRefineMaxViews], nv[kTrackRefineMaxViews];
            const int nviews = bundle_views(a, p, o, e.match, V, nu, nv);
            double ci = 0.0, se = 0.0;
            int used = 0, inl = 0;
#pragma unroll
            for (int v = 0; v < kTrackRefineMaxViews; ++v) {
                if (v < nviews) {
                    const BundleView q = bundle_view(sh.cam[v], X, nu[v], nv[v], kh, kh2);
                    const double rho = q.e2 <= kh2 ? q.e2 : (2 * kh) * sqrt(q.e2) - kh * kh;
                    ci = ci + (q.ok ? rho : 0.0);
                    const double ex = a.fx * q.ru, ey = a.fy * q.rv;
                    const double er = ex * ex + ey * ey;
                    const bool in = q.ok && er <= in2;
                    used += q.ok;
                    inl += in;
                    se = se + (in ? er : 0.0);
                }
            }
            evc[tid] = ci;
            evs[tid] = se;
            atomicAdd(&sh.cnt[0], nviews);
            atomicAdd(&sh.cnt[1], inl);
            if (write && a.bd_points && o < a.cap) {
                dvo_landmark_refined out;
                out.X = X[0], out.Y = X[1], out.Z = X[2];
                out.rms = inl > 0 ? sqrt(se / (double)inl) : 0.0;
                out.views = nviews;
                out.n_used = used;
                out.n_inliers = inl;
                out.iters = kept ? steps : 0;
                out.status = !kept ? DVO_TRACK_REFINE_NONE : steps == taken ? DVO_TRACK_REFINE_OK : DVO_TRACK_REFINE_DEGENERATE;
                out.reserved = 0;
                a.bd_points[(int64_t)p * a.cap + o] = out;
            }
        }
        __syncthreads();
        const int c = min(kBundleNT, n - base);
        if (tid == 0)
            for (int j = 0; j < c; ++j) acc = acc + evc[j];
        if (tid == 64)
            for (int j = 0; j < c; ++j) acc = acc + evs[j];
        __syncthreads();
    }
    if (tid == 0) sh.res[0] = acc;
    if (tid == 64) sh.res[1] = acc;
    __syncthreads();
}

// A workgroup per pair.  Every barrier is reached by all 256 threads: a NONE pair leaves before the
// first as a whole, and the trip counts come from the pair's count, V, iters and the failure flag
// read after a barrier.
__global__ __launch_bounds__(kBundleNT) void track_bundle_kernel(TrackArgs a) {
    __shared__ BundleShared sh;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int32_t* tc = a.L.tcnt + (int64_t)p * a.tiles;
    int n = 0;
    for (int t = 0; t < a.tiles; ++t) n += tc[t];
    if (n == 0 || n < a.bd_min_points) {
        if (tid == 0 && a.bundle) {
            dvo_track_bundle o;
            double rho;
            refine_motion(a, a.bd_use_pose, p, o.R, o.t, &rho);
            o.ratio = o.cost0 = o.cost = o.rms0 = o.rms = 0.0;
            o.n_points = o.n_obs = o.n_inliers = o.n_cams = o.iters = 0;
            o.status = DVO_TRACK_BUNDLE_NONE;
            a.bundle[p] = o;
        }
        if (a.bd_points)
            for (int o = tid; o < min(n, a.cap); o += kBundleNT) {
                const LandmarkTmp e = track_ordinal(a, p, o);
                dvo_landmark_refined out;
                out.X = e.X, out.Y = e.Y, out.Z = e.Z;
                out.rms = 0.0;
                out.views = 2;
                out.n_used = out.n_inliers = out.iters = 0;
                out.status = DVO_TRACK_REFINE_NONE;
                out.reserved = 0;
                a.bd_points[(int64_t)p * a.cap + o] = out;
            }
        return;
    }
    BundlePoint* bx = a.bd_x + (int64_t)p * a.pts_stride;
    if (tid == 0) {
        double rho;
        sh.win = window_cameras(a, p, a.bd_views, a.bd_use_pose, sh.cam, &rho);
        sh.rho = rho;
        for (int v = 0; v < kTrackRefineMaxViews; ++v)
            for (int i = 0; i < 12; ++i) sh.cam0[v][i] = v <= sh.win + 1 ? sh.cam[v][i] : 0.0;
    }
    for (int o = tid; o < n; o += kBundleNT) {
        const LandmarkTmp e = track_ordinal(a, p, o);
        BundlePoint b;
        b.X[0] = e.X, b.X[1] = e.Y, b.X[2] = e.Z;
        b.steps = b.pad = 0;
        bx[o] = b;
    }
    __syncthreads();
    const int V = sh.win + 2, n6 = 6 * (V - 1), nS = n6 * (n6 + 1) / 2;
    const double kh = a.bd_huber_px / ((a.fx + a.fy) / 2), kh2 = kh * kh, lam = a.bd_lambda;
    bundle_eval(a, sh, p, n, V, kh, kh2, true, false, false, 0);
    const double cost0 = sh.res[0], se0 = sh.res[1];
    const int inl0 = sh.cnt[1];
    // this lane's entries of S (upper triangle, row by row) and r: where Y's row, the second factor's
    // row, and the U / h term stand in a landmark's blocks
    int eY[kBundleEnt], eB[kBundleEnt], eU[kBundleEnt], eNeed[kBundleEnt], eKind[kBundleEnt], eDst[kBundleEnt];
#pragma unroll
    for (int q = 0; q < kBundleEnt; ++q) {
        const int e = tid + q * kBundleNT;
        eY[q] = eB[q] = eU[q] = eNeed[q] = eDst[q] = 0;
        eKind[q] = -1;
        if (e < nS) {
            int row = 0, rem = e;
            while (rem >= n6 - row) rem -= n6 - row, ++row;
            const int col = row + rem;
            const int c = row / 6, r = row % 6, c2 = col / 6, s = col % 6;  // cameras c + 1, c2 + 1
            eY[q] = c * kBundleCamF + 18 + r * 3;
            eB[q] = c2 * kBundleCamF + s * 3;
            eNeed[q] = c2 + 1;
            eDst[q] = row * kBundleLd + col;
            if (c == c2) {
                eU[q] = c * kBundleCamF + 36 + (r * 6 - r * (r - 1) / 2 + (s - r));
                eKind[q] = r == s ? 2 : 1;
            } else {
                eKind[q] = 0;
            }
        } else if (e < nS + n6) {
            const int row = e - nS, c = row / 6, r = row % 6;
            eY[q] = c * kBundleCamF + 18 + r * 3;
            eB[q] = kBundleG;
            eU[q] = c * kBundleCamF + 57 + r;
            eNeed[q] = c + 1;
            eDst[q] = row;
            eKind[q] = 3;
        }
    }
    int status = DVO_TRACK_BUNDLE_OK, it = 0;
    for (; it < a.bd_iters; ++it) {
        double accT[kBundleEnt], accU[kBundleEnt];
#pragma unroll
        for (int q = 0; q < kBundleEnt; ++q) accT[q] = accU[q] = 0.0;
        if (tid == 0) sh.fail = 0;
        for (int base = 0; base < n; base += kBundleTile) {
            const int cnt = min(kBundleTile, n - base);
            // 1. lane per landmark: linearise, factor V, form Y, leave the blocks in LDS
            if (tid < cnt) {
                const int o = base + tid;
                const LandmarkTmp e = track_ordinal(a, p, o);
                const BundlePoint bp = bx[o];
                const double X[3] = {bp.X[0], bp.X[1], bp.X[2]};
                double nu[kTrackRefineMaxViews], nv[kTrackRefineMaxViews];
                const int nviews = bundle_views(a, p, o, e.match, V, nu, nv);
                double* B = sh.blk + tid * kBundleF;
                double Vt[6], g[3];
#pragma unroll
                for (int i = 0; i < 6; ++i) Vt[i] = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) g[i] = 0.0;
#pragma unroll
                for (int v = 0; v < kTrackRefineMaxViews; ++v) {
                    if (v < nviews) {
                        const double* C = sh.cam[v];
                        const BundleView q = bundle_view(C, X, nu[v], nv[v], kh, kh2);
                        double Ju[3], Jv[3];
                        bundle_jx(C, q, Ju, Jv);
                        int k = 0;
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = i; j < 3; ++j, ++k) {
                                const double term = q.w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
                                Vt[k] = Vt[k] + (q.ok ? term : 0.0);
                            }
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const double term = q.w * (Ju[i] * q.ru + Jv[i] * q.rv);
                            g[i] = g[i] + (q.ok ? term : 0.0);
                        }
                        if (v >= 1) {
                            double Cu[6], Cv[6];
                            bundle_jc(q, Cu, Cv);
                            double* Bc = B + (v - 1) * kBundleCamF;
#pragma unroll
                            for (int r = 0; r < 6; ++r)
#pragma unroll
                                for (int j = 0; j < 3; ++j) {
                                    const double term = q.w * (Cu[r] * Ju[j] + Cv[r] * Jv[j]);
                                    Bc[r * 3 + j] = q.ok ? term : 0.0;
                                }
                            k = 36;
#pragma unroll
                            for (int r = 0; r < 6; ++r)
#pragma unroll
                                for (int s = r; s < 6; ++s, ++k) {
                                    const double term = q.w * (Cu[r] * Cu[s] + Cv[r] * Cv[s]);
                                    Bc[k] = q.ok ? term : 0.0;
                                }
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
                                const double term = q.w * (Cu[r] * q.ru + Cv[r] * q.rv);
                                Bc[57 + r] = q.ok ? term : 0.0;
                            }
                        }
                    }
                }
                Vt[0] = Vt[0] + lam * Vt[0];
                Vt[3] = Vt[3] + lam * Vt[3];
                Vt[5] = Vt[5] + lam * Vt[5];
                BundleLdl3 f;
                const bool good = bundle_factor3(Vt, &f);
                for (int v = 1; v < nviews; ++v) {
                    double* Bc = B + (v - 1) * kBundleCamF;
                    for (int r = 0; r < 6; ++r) {
                        double x[3];
                        bundle_apply3(f, Bc[r * 3], Bc[r * 3 + 1], Bc[r * 3 + 2], x);
                        Bc[18 + r * 3] = x[0], Bc[18 + r * 3 + 1] = x[1], Bc[18 + r * 3 + 2] = x[2];
                    }
                }
                B[kBundleG] = g[0], B[kBundleG + 1] = g[1], B[kBundleG + 2] = g[2];
                sh.lnv[tid] = good ? nviews : 0;
            }
            __syncthreads();
            // 2. lane per entry: the tile's landmarks in ascending ordinal onto the running value
            for (int l = 0; l < cnt; ++l) {
                const int nvl = sh.lnv[l];
                const double* B = sh.blk + l * kBundleF;
#pragma unroll
                for (int q = 0; q < kBundleEnt; ++q) {
                    if (eKind[q] >= 0 && nvl > eNeed[q]) {
                        const double* Y = B + eY[q];
                        const double* W = B + eB[q];
                        accT[q] = accT[q] + ((Y[0] * W[0] + Y[1] * W[1]) + Y[2] * W[2]);
                        if (eKind[q] != 0) accU[q] = accU[q] + B[eU[q]];
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < kBundleEnt; ++q) {
            if (eKind[q] == 0) sh.S[eDst[q]] = -accT[q];
            if (eKind[q] == 1) sh.S[eDst[q]] = accU[q] - accT[q];
            if (eKind[q] == 2) sh.S[eDst[q]] = (accU[q] + lam * accU[q]) - accT[q];
            if (eKind[q] == 3) sh.r[eDst[q]] = accU[q] - accT[q];
        }
        __syncthreads();
        // 3. the LDL^T of S: for column j, lane i - j runs row i's k loop in the header's order
        for (int j = 0; j < n6; ++j) {
            const int i = j + tid;
            double x = 0.0;
            if (i < n6) {
                x = sh.S[j * kBundleLd + i];
                for (int k = 0; k < j; ++k) x = x - (sh.S[i * kBundleLd + k] * sh.S[j * kBundleLd + k]) * sh.D[k];
                if (tid == 0) {
                    sh.D[j] = x;
                    if (!(x > 0)) sh.fail = 1;
                }
            }
            __syncthreads();
            if (i < n6 && tid > 0) sh.S[i * kBundleLd + j] = x / sh.D[j];
            __syncthreads();
        }
        if (tid == 0) {
            for (int i = 0; i < n6; ++i) {
                double x = -sh.r[i];
                for (int k = 0; k < i; ++k) x = x - sh.S[i * kBundleLd + k] * sh.y[k];
                sh.y[i] = x;
            }
            for (int i = 0; i < n6; ++i) sh.y[i] = sh.y[i] / sh.D[i];
            bool finite = true;
            for (int i = n6 - 1; i >= 0; --i) {
                double x = sh.y[i];
                for (int k = i + 1; k < n6; ++k) x = x - sh.S[k * kBundleLd + i] * sh.d[k];
                sh.d[i] = x;
                finite = finite && isfinite(x);
            }
            if (!finite) sh.fail = 1;
        }
        __syncthreads();
        if (sh.fail) {  // the same for every thread; the next write to it lies behind the next barrier
            status = DVO_TRACK_BUNDLE_DEGENERATE;
            break;
        }
        // the landmarks back-substitute on the step's cameras: lane per landmark, the blocks formed again
        for (int o = tid; o < n; o += kBundleNT) {
            const LandmarkTmp e = track_ordinal(a, p, o);
            BundlePoint bp = bx[o];
            const double X[3] = {bp.X[0], bp.X[1], bp.X[2]};
            double nu[kTrackRefineMaxViews], nv[kTrackRefineMaxViews];
            const int nviews = bundle_views(a, p, o, e.match, V, nu, nv);
            double Vt[6], g[3], tw[kTrackRefineMaxViews][3];
#pragma unroll
            for (int i = 0; i < 6; ++i) Vt[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = 0.0;
#pragma unroll
            for (int v = 0; v < kTrackRefineMaxViews; ++v) {
                tw[v][0] = tw[v][1] = tw[v][2] = 0.0;
                if (v < nviews) {
                    const double* C = sh.cam[v];
                    const BundleView q = bundle_view(C, X, nu[v], nv[v], kh, kh2);
                    double Ju[3], Jv[3];
                    bundle_jx(C, q, Ju, Jv);
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = i; j < 3; ++j, ++k) {
                            const double term = q.w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
                            Vt[k] = Vt[k] + (q.ok ? term : 0.0);
                        }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double term = q.w * (Ju[i] * q.ru + Jv[i] * q.rv);
                        g[i] = g[i] + (q.ok ? term : 0.0);
                    }
                    if (v >= 1) {
                        double Cu[6], Cv[6];
                        bundle_jc(q, Cu, Cv);
                        const double* dc = sh.d + 6 * (v - 1);
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            double t = 0.0;
#pragma unroll
                            for (int r = 0; r < 6; ++r) {
                                const double term = q.w * (Cu[r] * Ju[j] + Cv[r] * Jv[j]);
                                const double wd = (q.ok ? term : 0.0) * dc[r];
                                t = r == 0 ? wd : t + wd;
                            }
                            tw[v][j] = t;
                        }
                    }
                }
            }
            Vt[0] = Vt[0] + lam * Vt[0];
            Vt[3] = Vt[3] + lam * Vt[3];
            Vt[5] = Vt[5] + lam * Vt[5];
            BundleLdl3 f;
            if (bundle_factor3(Vt, &f)) {
                double qv[3] = {-g[0], -g[1], -g[2]}, x[3];
#pragma unroll
                for (int v = 1; v < kTrackRefineMaxViews; ++v)
                    if (v < nviews) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) qv[j] = qv[j] - tw[v][j];
                    }
                bundle_apply3(f, qv[0], qv[1], qv[2], x);
#pragma unroll
                for (int j = 0; j < 3; ++j) bp.X[j] = X[j] + x[j];
                ++bp.steps;
                bx[o] = bp;
            }
        }
        __syncthreads();
        if (tid >= 1 && tid < V) {
            double R[9], t[3], d[6], o[12];
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = sh.cam[tid][i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = sh.cam[tid][9 + i];
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = sh.d[6 * (tid - 1) + i];
            pose_update(R, t, d, o);
#pragma unroll
            for (int i = 0; i < 12; ++i) sh.cam[tid][i] = o[i];
        }
        __syncthreads();
    }
    // the guard and the gauge
    bundle_eval(a, sh, p, n, V, kh, kh2, false, false, false, it);
    const double cost = sh.res[0];
    const double b0 = sh.cam[1][9], b1 = sh.cam[1][10], b2 = sh.cam[1][11];
    const double s = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    const bool gauge = s > 0 && isfinite(1.0 / s);
    if (status == DVO_TRACK_BUNDLE_OK && !gauge)
        status = DVO_TRACK_BUNDLE_DEGENERATE;
    else if (status == DVO_TRACK_BUNDLE_OK && !(cost <= cost0))
        status = DVO_TRACK_BUNDLE_NOT_IMPROVED;
    const bool keep = it > 0 && gauge && cost <= cost0;
    __syncthreads();  // every thread has read cam[1] and res
    if (keep) {
        for (int o = tid; o < n; o += kBundleNT) {
            BundlePoint bp = bx[o];
#pragma unroll
            for (int j = 0; j < 3; ++j) bp.X[j] = bp.X[j] / s;
            bx[o] = bp;
        }
        if (tid >= 1 && tid < V) {
#pragma unroll
            for (int i = 0; i < 3; ++i) sh.cam[tid][9 + i] = sh.cam[tid][9 + i] / s;
        }
    } else if (tid < kTrackRefineMaxViews * 12) {
        sh.cam[tid / 12][tid % 12] = sh.cam0[tid / 12][tid % 12];
    }
    __syncthreads();
    bundle_eval(a, sh, p, n, V, kh, kh2, !keep, true, keep, it);
    if (tid == 0 && a.bundle) {
        dvo_track_bundle o;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.R[i] = sh.cam[1][i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o.t[i] = sh.cam[1][9 + i];
        if (V < 3) {
            o.ratio = 0.0;
        } else if (keep) {
            const double c0 = sh.cam[2][9], c1 = sh.cam[2][10], c2 = sh.cam[2][11];
            o.ratio = 1.0 / sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        } else {
            o.ratio = sh.rho;
        }
        o.cost0 = cost0;
        o.cost = cost;
        o.rms0 = inl0 > 0 ? sqrt(se0 / (double)inl0) : 0.0;
        o.rms = sh.cnt[1] > 0 ? sqrt(sh.res[1] / (double)sh.cnt[1]) : 0.0;
        o.n_points = n;
        o.n_obs = sh.cnt[0];
        o.n_inliers = sh.cnt[1];
        o.n_cams = V;
        o.iters = it;
        o.status = status;
        a.bundle[p] = o;
    }
}

// ---- track PnP (dvo.h dvo_stream_set_track_pnp) ----------------------------------------------------
// Per (tile of 256 raw matches, pair): match i is a correspondence iff pair p - 1's table holds a
// landmark at its queryIdx.  The hits of a tile go, in match order (wave ballots and mbcnt ranks, as
// the link kernel), to pnp_corr from slot tile * 256 on: hit r of the tile has r <= its place in the
// tile, so its slot is at most its match index < the pair's matches <= pts_stride.
__global__ __launch_bounds__(kLandmarkTile) void track_pnp_corr_kernel(TrackArgs a) {
    __shared__ int wtot[kLandmarkTile / 64];
    const int p = blockIdx.y, tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = tile * kLandmarkTile + tid;
    const int nm = p >= 1 ? (int)min((int64_t)max(a.rec[p].n_matches, 0), a.pts_stride) : 0;
    bool hit = false;
    PnpCorr c;
    if (i < nm) {
        const int q = a.mq[((int64_t)p * a.idx_stride + i) * a.idx_step];
        if ((unsigned)q < (unsigned)a.kp_cap) {
            const int v = a.table[(int64_t)(p - 1) * a.kp_cap + q];
            if (v != kTrackEmpty) {
                const LandmarkTmp e = track_ordinal(a, p - 1, v);
                const double* R = a.rec[p - 1].R;
                const double* tv = a.rec[p - 1].t;
#pragma unroll
                for (int k = 0; k < 3; ++k) c.y[k] = ((R[3 * k] * e.X + R[3 * k + 1] * e.Y) + R[3 * k + 2] * e.Z) + tv[k];
                const double ax = 1. / a.fx, ay = 1. / a.fy, bx = -a.cx * ax, by = -a.cy * ay;
                const float* px = a.pts_f + ((int64_t)p * a.pts_stride + i) * 4;
                const double x2 = px[2], y2 = px[3];
                c.nu = x2 * ax + bx;
                c.nv = y2 * ay + by;
                c.match = i;
                c.sel = 0;
                hit = true;
            }
        }
    }
    const unsigned long long bal = __ballot(hit);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kLandmarkTile / 64; ++w) {
        const int n = wtot[w];
        before += w < wave ? n : 0;
        total += n;
    }
    if (hit) a.pnp_corr[(int64_t)p * a.pts_stride + tile * kLandmarkTile + before + rank] = c;
    if (tid == 0) a.pnp_cnt[(int64_t)p * a.tiles + tile] = total;
}

// does correspondence (y, nu, nv) support the pose: the final pass's inlier test
__device__ __forceinline__ bool pnp_supports(const TrackArgs& a, const double* R, const double* tv, double in2, double y0,
                                             double y1, double y2, double nu, double nv) {
    const double P0 = ((R[0] * y0 + R[1] * y1) + R[2] * y2) + tv[0];
    const double P1 = ((R[3] * y0 + R[4] * y1) + R[5] * y2) + tv[1];
    const double P2 = ((R[6] * y0 + R[7] * y1) + R[8] * y2) + tv[2];
    const bool ok = P2 > 0;
    const double ia = 1 / P2, u = P0 * ia, v = P1 * ia;
    const double ex = a.fx * (u - nu), ey = a.fy * (v - nv);
    const double e = ex * ex + ey * ey;
    return ok && e <= in2;
}

// is (count, h, solution) a better hypothesis than (bc, bh, bs): more supporters, then the smaller h, then the smaller solution
__device__ __forceinline__ bool pnp_better(int count, int h, int sol, int bc, int bh, int bs) {
    return count > bc || (count == bc && (h < bh || (h == bh && sol < bs)));
}

// A workgroup per pair.  Every barrier is reached by all 256 threads: a NONE or NO_MODEL pair
// leaves as a whole, and the trip counts (the tiles' counts, hyps, the poses a sample left in LDS,
// iters, the stop flag read after a barrier) are the same for every thread of the workgroup or,
// inside the scoring loop where there is no barrier, of the wave.  Nothing is added in an order
// that lane scheduling could change: the scores are integer counts from ballots.
__global__ __launch_bounds__(kPoseNT) void track_pnp_kernel(TrackArgs a) {
    __shared__ double cs[5][kTrackPoseLds];  // y0, y1, y2, nu, nv of the correspondences that fit
    __shared__ double hyp[kPnpRound * 4][12];  // the round's poses: sample s of the round at hyp[4 s ..]
    __shared__ int hyp_n[kPnpRound];
    __shared__ double wpose[kPoseNT / 64][12];  // each wave's best pose
    __shared__ int wbest[kPoseNT / 64][3];      // its count, sample and solution
    __shared__ double wsum[kPoseNT / 64][kPoseTerms];
    __shared__ int wcnt[kPoseNT / 64][2];
    __shared__ double next[12];
    __shared__ int stop;
    const int p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* cc = a.pnp_cnt + (int64_t)p * a.tiles;
    int n = 0;
    for (int t = 0; t < a.tiles; ++t) n += cc[t];
    uint8_t* mask = a.pnp_mask ? a.pnp_mask + (int64_t)p * a.pnp_mask_cap : nullptr;
    if (mask) {  // 0 for every match in range; the final pass sets the inliers after the barriers below
        const int nm = (int)min((int64_t)max(a.rec[p].n_matches, 0), a.pts_stride);
        for (int i = tid; i < min(nm, a.pnp_mask_cap); i += kPoseNT) mask[i] = 0;
    }
    dvo_track_pnp o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = 0.0;
    o.scale = o.rms = 0.0;
    o.n_corr = n;
    o.n_best = o.n_used = o.n_inliers = o.sample = o.solution = o.iters = 0;
    if (p == 0 || n < a.pnp_min_points) {
        if (tid == 0) {
            o.status = DVO_TRACK_PNP_NONE;
            a.pnp[p] = o;
        }
        return;
    }
    // the tiles' correspondences together, in match order: moved down in place (a tile's target ends
    // at or before its source starts), and into LDS as well when they fit
    PnpCorr* g = a.pnp_corr + (int64_t)p * a.pts_stride;
    const bool in_lds = n <= kTrackPoseLds;
    for (int t = 0, off = 0; t < a.tiles; ++t) {
        const int c = cc[t];
        if (c == 0) continue;  // the same for every thread
        PnpCorr v;
        if (tid < c) v = g[t * kLandmarkTile + tid];
        __syncthreads();
        if (tid < c) {
            g[off + tid] = v;
            if (in_lds) {
#pragma unroll
                for (int i = 0; i < 3; ++i) cs[i][off + tid] = v.y[i];
                cs[3][off + tid] = v.nu;
                cs[4][off + tid] = v.nv;
            }
        }
        __syncthreads();
        off += c;
    }
    const double in2 = a.pnp_inlier_px * a.pnp_inlier_px;
    // the hypotheses, kPnpRound samples at a time: wave 0 solves a sample per lane, then wave w
    // scores the poses of the round's samples w, w + 4, ... in ascending (sample, solution)
    int bc = -1, bh = 0, bs = 0;  // the wave's best so far: the same in all its lanes
    double bR[9], bt[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) bR[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) bt[i] = 0.0;
    for (int base = 0; base < a.pnp_hyps; base += kPnpRound) {
        if (tid < kPnpRound) {
            int ns = 0, idx[3];
            if (base + tid < a.pnp_hyps && p3p_sample(a.pnp_seed, base + tid, n, idx)) {
                double Y[9], nunv[6], Rs[4][9], ts[4][3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    pose_corr(cs, g, in_lds, idx[j], Y[3 * j], Y[3 * j + 1], Y[3 * j + 2], nunv[2 * j], nunv[2 * j + 1]);
                ns = p3p_solve(Y, nunv, Rs, ts);
                for (int s = 0; s < ns; ++s) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) hyp[4 * tid + s][i] = Rs[s][i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) hyp[4 * tid + s][9 + i] = ts[s][i];
                }
            }
            hyp_n[tid] = ns;
        }
        __syncthreads();
        for (int s = wave; s < kPnpRound; s += kPoseNT / 64) {
            const int ns = hyp_n[s];  // 0 past hyps
            for (int sol = 0; sol < ns; ++sol) {
                double R[9], tv[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = hyp[4 * s + sol][i];
#pragma unroll
                for (int i = 0; i < 3; ++i) tv[i] = hyp[4 * s + sol][9 + i];
                int count = 0;
                for (int k0 = 0; k0 < n; k0 += 64) {  // the same trips for the wave's lanes: the ballot is whole
                    const int k = k0 + lane;
                    bool sup = false;
                    if (k < n) {
                        double y0, y1, y2, nu, nv;
                        pose_corr(cs, g, in_lds, k, y0, y1, y2, nu, nv);
                        sup = pnp_supports(a, R, tv, in2, y0, y1, y2, nu, nv);
                    }
                    count += __popcll(__ballot(sup));
                }
                if (pnp_better(count, base + s, sol, bc, bh, bs)) {
                    bc = count, bh = base + s, bs = sol;
#pragma unroll
                    for (int i = 0; i < 9; ++i) bR[i] = R[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) bt[i] = tv[i];
                }
            }
        }
        __syncthreads();  // the round's poses are read; the next round writes them
    }
    if (lane == 0) {
        wbest[wave][0] = bc, wbest[wave][1] = bh, wbest[wave][2] = bs;
#pragma unroll
        for (int i = 0; i < 9; ++i) wpose[wave][i] = bR[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) wpose[wave][9 + i] = bt[i];
    }
    __syncthreads();
    int win = 0;
    bc = wbest[0][0], bh = wbest[0][1], bs = wbest[0][2];
#pragma unroll
    for (int w = 1; w < kPoseNT / 64; ++w)
        if (pnp_better(wbest[w][0], wbest[w][1], wbest[w][2], bc, bh, bs)) bc = wbest[w][0], bh = wbest[w][1], bs = wbest[w][2], win = w;
    if (bc < a.pnp_min_points) {  // also no kept solution at all: bc is -1
        if (tid == 0) {
            o.n_best = bc < 0 ? 0 : bc;
            o.sample = bc < 0 ? -1 : bh;
            o.solution = bc < 0 ? -1 : bs;
            o.status = DVO_TRACK_PNP_NO_MODEL;
            a.pnp[p] = o;
        }
        return;
    }
    double R[9], tv[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = wpose[win][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = wpose[win][9 + i];
    // the polish set: the winner's supporters in ascending k, the j-th of them into g[j].sel
    // (j <= k, and sel is no correspondence's data); hyp_n is free now: the waves' totals
    int ns = 0;
    for (int k0 = 0; k0 < n; k0 += kPoseNT) {
        const int k = k0 + tid;
        bool sup = false;
        if (k < n) {
            double y0, y1, y2, nu, nv;
            pose_corr(cs, g, in_lds, k, y0, y1, y2, nu, nv);
            sup = pnp_supports(a, R, tv, in2, y0, y1, y2, nu, nv);
        }
        const unsigned long long bal = __ballot(sup);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) hyp_n[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kPoseNT / 64; ++w) {
            const int c = hyp_n[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (sup) g[ns + before + rank].sel = k;
        ns += total;
        __syncthreads();
    }
    const double kh = a.pnp_huber_px / ((a.fx + a.fy) / 2), kh2 = kh * kh;
    int status = DVO_TRACK_PNP_OK, it = 0;
    for (; it < a.pnp_iters; ++it)
        if (!pose_step<PnpCorr, true>(cs, g, in_lds, ns, R, tv, kh, kh2, wsum, next, &stop)) {
            status = DVO_TRACK_PNP_DEGENERATE;
            break;
        }
    double sum;
    pose_final<PnpCorr, true>(a, cs, g, in_lds, n, R, tv, a.pnp_inlier_px, wsum, wcnt, mask, a.pnp_mask_cap, &sum, &o.n_used,
                              &o.n_inliers);
    if (tid == 0) {
        o.rms = o.n_inliers > 0 ? sqrt(sum / (double)o.n_inliers) : 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.R[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o.t[i] = tv[i];
        o.scale = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
        o.n_best = bc;
        o.sample = bh;
        o.solution = bs;
        o.iters = it;
        o.status = status;
        a.pnp[p] = o;
    }
}

}  // namespace

hipError_t launch_tracks(const TrackArgs& a, int pairs, hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    if (!a.L.tmp || !a.L.tcnt || !a.mq || !a.mt || !a.rec || !a.table || !a.ratio || !a.lcnt || a.tiles < 1 ||
        a.kp_cap < 1 || a.idx_step < 1 || (!a.link && !a.scale) || (a.link && a.cap < 1))
        return hipErrorInvalidValue;
    if (a.pose ? !a.scale || !a.corr || !a.pts_f || a.pose_iters < 1 || a.pose_iters > kTrackPoseMaxIters ||
                     a.pose_min_points < 3 || !(a.huber_px > 0) || !(a.inlier_px > 0)
               : a.corr != nullptr)
        return hipErrorInvalidValue;
    const bool refine = a.id || a.refined;  // a refine binding; a bundle binding is bd_x
    if (a.flink ? !a.scale || !a.pts_f || a.cap < 1 || (!refine && !a.bd_x) : refine || a.bd_x != nullptr)
        return hipErrorInvalidValue;
    if (refine && ((a.id && (!a.rank || a.rank_stride < 1)) || a.rf_views < 3 || a.rf_views > kTrackRefineMaxViews ||
                   a.rf_iters < 1 || a.rf_iters > kTrackRefineMaxIters || !(a.rf_huber_px > 0) ||
                   !(a.rf_inlier_px > 0) || (a.rf_use_pose && !a.pose)))
        return hipErrorInvalidValue;
    if (a.bd_x && ((!a.bundle && !a.bd_points) || a.bd_views < 2 || a.bd_views > kTrackRefineMaxViews || a.bd_iters < 1 ||
                   a.bd_iters > kTrackBundleMaxIters || a.bd_min_points < 6 || !(a.bd_lambda > 0) ||
                   !(a.bd_huber_px > 0) || !(a.bd_inlier_px > 0) || (a.bd_use_pose && !a.pose)))
        return hipErrorInvalidValue;
    if (a.pnp ? !a.pnp_corr || !a.pnp_cnt || !a.pts_f || a.pnp_hyps < 1 || a.pnp_hyps > kPnpMaxHyps || a.pnp_iters < 1 ||
                    a.pnp_iters > kTrackPoseMaxIters || a.pnp_min_points < 4 || !(a.pnp_huber_px > 0) ||
                    !(a.pnp_inlier_px > 0) || (a.pnp_mask && a.pnp_mask_cap < 1)
              : a.pnp_corr != nullptr || a.pnp_mask != nullptr)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.table, 0x7f, (size_t)pairs * a.kp_cap * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)a.tiles, (unsigned)pairs);
    hipLaunchKernelGGL(track_table_kernel, grid, dim3(kLandmarkTile), 0, s, a);
    hipLaunchKernelGGL(track_link_kernel, grid, dim3(kLandmarkTile), 0, s, a);
    if (a.scale) hipLaunchKernelGGL(track_select_kernel, dim3((unsigned)pairs), dim3(kSelNT), 0, s, a);
    if (a.pose) hipLaunchKernelGGL(track_pose_kernel, dim3((unsigned)pairs), dim3(kPoseNT), 0, s, a);
    if (a.flink && a.id) {
        // the longest chain has pairs - 1 links: launch r ranks chains of up to 2^r
        int rounds = 0;
        while ((1 << rounds) < pairs - 1) ++rounds;
        for (int r = 0; r <= rounds; ++r)
            hipLaunchKernelGGL(track_id_kernel, grid, dim3(kLandmarkTile), 0, s, a, r, r == rounds ? 1 : 0);
    }
    if (a.flink && a.refined) hipLaunchKernelGGL(track_refine_kernel, grid, dim3(kLandmarkTile), 0, s, a);
    if (a.bd_x) hipLaunchKernelGGL(track_bundle_kernel, dim3((unsigned)pairs), dim3(kBundleNT), 0, s, a);
    if (a.pnp) {
        hipLaunchKernelGGL(track_pnp_corr_kernel, grid, dim3(kLandmarkTile), 0, s, a);
        hipLaunchKernelGGL(track_pnp_kernel, dim3((unsigned)pairs), dim3(kPoseNT), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dvo
