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
// The ratio's arithmetic is the header's, one rounding per operation (-ffp-contract=off).
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
        }
        const int o = first + tid;
        if (a.link && o < a.cap) a.link[(int64_t)p * a.cap + o] = lk;
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

}  // namespace

hipError_t launch_tracks(const TrackArgs& a, int pairs, hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    if (!a.L.tmp || !a.L.tcnt || !a.mq || !a.mt || !a.rec || !a.table || !a.ratio || !a.lcnt || a.tiles < 1 ||
        a.kp_cap < 1 || a.idx_step < 1 || (!a.link && !a.scale) || (a.link && a.cap < 1))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.table, 0x7f, (size_t)pairs * a.kp_cap * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)a.tiles, (unsigned)pairs);
    hipLaunchKernelGGL(track_table_kernel, grid, dim3(kLandmarkTile), 0, s, a);
    hipLaunchKernelGGL(track_link_kernel, grid, dim3(kLandmarkTile), 0, s, a);
    if (a.scale) hipLaunchKernelGGL(track_select_kernel, dim3((unsigned)pairs), dim3(kSelNT), 0, s, a);
    return hipGetLastError();
}

}  // namespace dvo
