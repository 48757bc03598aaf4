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
// The arithmetic is the header's, one rounding per operation (-ffp-contract=off).
#include "dvo_internal.h"

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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    for (; it < a.pose_iters; ++it) {
        double acc[kPoseTerms];
#pragma unroll
        for (int q = 0; q < kPoseTerms; ++q) acc[q] = 0.0;
        for (int k = tid; k < n; k += kPoseNT) {
            double y0, y1, y2, nu, nv;
            if (in_lds) {
                y0 = cs[0][k], y1 = cs[1][k], y2 = cs[2][k], nu = cs[3][k], nv = cs[4][k];
            } else {
                const TrackCorr v = g[k];
                y0 = v.y[0], y1 = v.y[1], y2 = v.y[2], nu = v.nu, nv = v.nv;
            }
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
                for (int j = i; j < 6; ++j, ++q) {
                    const double term = w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
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
            stop = solved ? 0 : 1;
        }
        __syncthreads();
        if (stop) {  // the same for every thread; the next write to it lies behind the next barrier
            status = DVO_TRACK_POSE_DEGENERATE;
            break;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = next[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tv[i] = next[9 + i];
    }
    // the final pass on the last pose
    double se = 0.0;
    int used = 0, inl = 0;
    const double in2 = a.inlier_px * a.inlier_px;
    for (int k = tid; k < n; k += kPoseNT) {
        double y0, y1, y2, nu, nv;
        if (in_lds) {
            y0 = cs[0][k], y1 = cs[1][k], y2 = cs[2][k], nu = cs[3][k], nv = cs[4][k];
        } else {
            const TrackCorr v = g[k];
            y0 = v.y[0], y1 = v.y[1], y2 = v.y[2], nu = v.nu, nv = v.nv;
        }
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
    }
    se = pose_wave_sum(se);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        used += __shfl_down(used, s);
        inl += __shfl_down(inl, s);
    }
    if (lane == 0) {  // wsum was last read before the loop's final barrier
        wsum[wave][0] = se;
        wcnt[wave][0] = used;
        wcnt[wave][1] = inl;
    }
    __syncthreads();
    if (tid == 0) {
        const double sum = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
        o.n_used = ((wcnt[0][0] + wcnt[1][0]) + wcnt[2][0]) + wcnt[3][0];
        o.n_inliers = ((wcnt[0][1] + wcnt[1][1]) + wcnt[2][1]) + wcnt[3][1];
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
__device__ void refine_motion(const TrackArgs& a, int q, double* R, double* d, double* rho) {
    if (a.rf_use_pose && a.pose[q].status == DVO_TRACK_POSE_OK) {
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
        double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, b[3] = {0, 0, 0}, sigma = 1, R[9], d[3], rho;
#pragma unroll
        for (int i = 0; i < 9; ++i) cam[0][i] = A[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) cam[0][9 + i] = 0.0;
        refine_motion(a, p, R, d, &rho);
#pragma unroll
        for (int i = 0; i < 9; ++i) cam[1][i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) cam[1][9 + i] = d[i];
        int W = 0;
        for (int k = 1; k <= a.rf_views - 2; ++k) {  // camera k goes to view k + 1 <= views - 1
            const int q = p - k;
            if (q < 0) break;
            refine_motion(a, q + 1, R, d, &rho);
            if (!(rho > 0)) break;  // also where pair q or q + 1 has no landmarks: pair q + 1 links nothing
            sigma = sigma / rho;
            if (!isfinite(sigma)) break;
            refine_motion(a, q, R, d, &rho);
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
        win = W;
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
    if (a.flink && (!a.scale || !a.pts_f || a.cap < 1 || (!a.id && !a.refined) || (a.id && (!a.rank || a.rank_stride < 1)) ||
                    a.rf_views < 3 || a.rf_views > kTrackRefineMaxViews || a.rf_iters < 1 ||
                    a.rf_iters > kTrackRefineMaxIters || !(a.rf_huber_px > 0) || !(a.rf_inlier_px > 0) ||
                    (a.rf_use_pose && !a.pose)))
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
    return hipGetLastError();
}

}  // namespace dvo
