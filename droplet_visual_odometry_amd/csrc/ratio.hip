// The k-NN modes' ratio test and keypoint gather on the device (visual_odometry_v3.py:223-238,
// KeyPoint_convert :355, :358), and the feature-slot copy of dvo_knn_pair_run.
//
// ratio_gather_kernel takes the matcher's k = 2 output (BFMatcher NORM_L1 distances, or FLANN's
// squared L2), applies Python's test `m.distance < 0.75 * n.distance` and writes the kept matches,
// in ascending queryIdx order, as the point quads the geometry kernels read (GeomArgs::pts_f), the
// DMatch list, the count and the pair's PairHeader.  The order is part of the result: RANSAC's
// subsets index into the point list, so the slots come from a ballot / prefix scan, never from
// atomics.
//
// ratio_gather_batch_kernel runs the same body for every pair of a dvo_knn_stream batch in one
// launch (a workgroup per pair, the counts read from the frame slots); knn_frame_state_kernel and
// knn_status_kernel are that path's bookkeeping: which frames overflow their slot, and the records
// of the pairs the reference raises on before findEssentialMat.
//
// hamming_ratio_stream_kernel runs the body on the ORB stream's packed Hamming 2-NN words
// (dvo_stream_set_ratio_test), and hamming_ratio_status_kernel marks the pairs the reference raises on.
#include "dvo_internal.h"

namespace dvo {

namespace {

constexpr int kRatioNT = 1024;  // one workgroup: 16 waves walk the queries 1024 at a time, in order

// Python's test on the float32 values DMatch.distance holds: the product and the compare are
// double (a float32 product 0.75f * d1 rounds and keeps a different set).  One workgroup of
// kRatioNT lanes runs one pair; h is the header it leaves.
// load(q, id, dd): the two train indices and distances of query q; store(slot, q, t, d0): the
// kept match of a slot.  The float matchers read a.idx / a.dist and write a.matches
// (ratio_gather_pair); the Hamming stream reads packed words and writes mq / mt / md.
template <class Load, class Store>
__device__ __forceinline__ void ratio_gather_body(const RatioArgs& a, const PairHeader h, Load load, Store store) {
    __shared__ int wtot[kRatioNT / 64];
    __shared__ int wmiss[kRatioNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;  // matches kept by the chunks before this one
    bool missing = false;
    for (int q0 = 0; q0 < a.nq; q0 += kRatioNT) {
        const int q = q0 + tid;
        bool keep = false;
        int t = -1;
        float d0 = 0.f;
        if (q < a.nq) {
            int2 id;
            float2 dd;
            load(q, id, dd);
            float d1 = dd.y;
            d0 = dd.x;
            if (a.squared) {  // FlannBasedMatcher::convertToDMatches: std::sqrt(float)
                d0 = sqrtf(d0);
                d1 = sqrtf(d1);
            }
            t = id.x;
            missing |= id.y < 0;
            keep = id.y >= 0 && t >= 0 && t < a.nkt && q < a.nkq && (double)d0 < a.ratio * (double)d1;
        }
        const unsigned long long bal = __ballot(keep);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kRatioNT / 64; ++w) {
            const int c = wtot[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int slot = base + before + rank;
            const dvo_keypoint& kq = a.kq[q];
            const dvo_keypoint& kt = a.kt[t];
            reinterpret_cast<float4*>(a.pts)[slot] = make_float4(kq.x, kq.y, kt.x, kt.y);
            store(slot, q, t, d0);
        }
        base += total;
        __syncthreads();  // wtot is rewritten by the next chunk
    }
    const unsigned long long mb = __ballot(missing);
    if (lane == 0) wmiss[wave] = mb != 0;
    __syncthreads();
    if (tid == 0) {
        int any = 0;
        for (int w = 0; w < kRatioNT / 64; ++w) any |= wmiss[w];
        *a.nmatch = base;
        if (a.hdr) *a.hdr = h;
        if (a.missing) *a.missing = any;
    }
}

__device__ __forceinline__ void ratio_gather_pair(const RatioArgs& a, const PairHeader h) {
    const int2* idx2 = reinterpret_cast<const int2*>(a.idx);
    const float2* dist2 = reinterpret_cast<const float2*>(a.dist);
    ratio_gather_body(
        a, h,
        [&](int q, int2& id, float2& dd) {
            id = idx2[q];
            dd = dist2[q];
        },
        [&](int slot, int q, int t, float d0) {
            reinterpret_cast<int4*>(a.matches)[slot] = make_int4(q, t, 0, __float_as_int(d0));
        });
}

// The ORB stream's ratio mode (launch_match_ratio): pair blockIdx.x's packed Hamming words
// (distance << 16 | trainIdx, -1 none; nearest in the forward half of P.buf.nn, second in the other)
// through the same body, the kept matches where crosscheck_stream_kernel leaves its own.
__global__ __launch_bounds__(kRatioNT) void hamming_ratio_stream_kernel(StreamParams P, double ratio) {
    const int p = blockIdx.x;
    const int cap = P.plan.kp_cap;
    const int fp = pair_frame(P, p);
    const int nq = min(P.buf.nkp[fp], cap), nt = min(P.buf.nkp[fp + 1], cap);
    const int32_t* w1 = P.buf.nn + (int64_t)p * cap;
    const int32_t* w2 = P.buf.nn + ((int64_t)P.nframes + p) * cap;
    int32_t* mq = P.buf.mq + (int64_t)p * cap;
    int32_t* mt = P.buf.mt + (int64_t)p * cap;
    float* md = P.buf.md + (int64_t)p * cap;
    const RatioArgs a{nullptr, nullptr, P.buf.kps + (int64_t)fp * cap, P.buf.kps + (int64_t)(fp + 1) * cap, nq, nq, nt,
                      ratio, 0, P.buf.pts + (int64_t)p * cap * 4, nullptr, P.buf.nmatch + p, nullptr, nullptr};
    ratio_gather_body(
        a, PairHeader{},
        [&](int q, int2& id, float2& dd) {
            const int a1 = w1[q], a2 = w2[q];
            id = make_int2(a1 < 0 ? -1 : a1 & 0xFFFF, a2 < 0 ? -1 : a2 & 0xFFFF);
            dd = make_float2((float)(a1 >> 16), (float)(a2 >> 16));
        },
        [&](int slot, int q, int t, float d0) {
            mq[slot] = q;
            mt[slot] = t;
            md[slot] = d0;
        });
}

__global__ __launch_bounds__(64) void hamming_ratio_status_kernel(const PairHeader* hdr, int pairs, dvo_pair_record* rec,
                                                                  int32_t* status) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= pairs) return;
    const PairHeader h = hdr[p];
    if (status) status[p] = h.flags ? DVO_ECAP : (h.nkp_prev == 0 || h.nkp_cur < 2) ? DVO_ENOFEAT : DVO_OK;
    if (!rec || h.flags || h.nkp_prev == 0 || h.nkp_cur >= 2) return;
    dvo_pair_record r{};
    r.n_kp_prev = h.nkp_prev;
    r.n_kp_cur = h.nkp_cur;
    r.status = DVO_ENOFEAT;
    rec[p] = r;
}

__global__ __launch_bounds__(kRatioNT) void ratio_gather_kernel(RatioArgs a) {
    ratio_gather_pair(a, PairHeader{a.nkq, a.nkt, 0, 0});
}

// The same for pair blockIdx.x of a batch of frame slots (dvo_knn_stream): the counts come from
// the slots, and every pair gets its count, flag and header, the empty ones too (RANSAC reads
// m_arr of all of them).  The header carries the detector's counts and whether a frame is marked.
__global__ __launch_bounds__(kRatioNT) void ratio_gather_batch_kernel(RatioBatchArgs b) {
    const int p = blockIdx.x;
    const int nq = b.fstate[2 * p], nt = b.fstate[2 * p + 2];
    const size_t o = (size_t)p * b.cap;
    const RatioArgs a{b.idx + o * 2, b.dist + o * 2, b.kps + o, b.kps + o + b.cap, nq, nq, nt, b.ratio, b.squared,
                      b.pts + o * 4, b.matches + o, b.nmatch + p, b.hdr + p, b.missing + p};
    ratio_gather_pair(a, PairHeader{b.n[2 * p], b.n[2 * p + 2], b.fstate[2 * p + 1] | b.fstate[2 * p + 3], 0});
}

// The first min(*cnt, kp_cap) keypoints and descriptors of a detection into a feature slot, the
// count and the detector's overflow flags beside them (the host reads both after one synchronisation).
__global__ __launch_bounds__(256) void feature_copy_kernel(const uint32_t* skps, const uint4* sdesc, const int32_t* cnt,
                                                           const int32_t* flags, int kp_cap, int dim, uint32_t* dkps,
                                                           uint4* ddesc, int32_t* dn) {
    const int n = min(max(*cnt, 0), kp_cap);
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    const int64_t kw = (int64_t)n * (int64_t)(sizeof(dvo_keypoint) / 4), dw = (int64_t)n * (dim / 4);
    for (int64_t i = i0; i < kw; i += step) dkps[i] = skps[i];
    for (int64_t i = i0; i < dw; i += step) ddesc[i] = sdesc[i];
    if (i0 == 0) {
        dn[0] = *cnt;
        dn[1] = *flags;
    }
}

// A frame whose detector count exceeds the slot or whose detector flagged an overflow is marked:
// it brings no feature to its pairs, and their records say DVO_ECAP.
__global__ __launch_bounds__(64) void knn_frame_state_kernel(const int32_t* n, int frames, int cap, int32_t* fstate) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= frames) return;
    const int c = n[2 * f];
    const int marked = n[2 * f + 1] != 0 || c > cap;
    fstate[2 * f] = marked ? 0 : max(c, 0);
    fstate[2 * f + 1] = marked;
}

__global__ __launch_bounds__(64) void knn_status_kernel(const int32_t* n, const int32_t* fstate, const int32_t* missing,
                                                        int pairs, dvo_pair_record* rec) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= pairs) return;
    if (fstate[2 * p + 1] | fstate[2 * p + 3]) return;  // DVO_ECAP stands
    if (fstate[2 * p] != 0 && fstate[2 * p + 2] >= 2 && missing[p] == 0) return;
    dvo_pair_record r{};
    r.n_kp_prev = n[2 * p];
    r.n_kp_cur = n[2 * p + 2];
    r.status = DVO_ENOFEAT;
    rec[p] = r;
}

}  // namespace

hipError_t launch_ratio_gather(const RatioArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(ratio_gather_kernel, dim3(1), dim3(kRatioNT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_hamming_ratio(const StreamParams& P, double ratio, hipStream_t s) {
    const int pairs = stream_pairs(P);
    if (pairs < 1) return hipSuccess;
    hipLaunchKernelGGL(hamming_ratio_stream_kernel, dim3(pairs), dim3(kRatioNT), 0, s, P, ratio);
    return hipGetLastError();
}

hipError_t launch_hamming_ratio_status(const PairHeader* hdr, int pairs, dvo_pair_record* records, int32_t* status,
                                       hipStream_t s) {
    if (pairs < 1) return hipSuccess;
    hipLaunchKernelGGL(hamming_ratio_status_kernel, dim3((pairs + 63) / 64), dim3(64), 0, s, hdr, pairs, records, status);
    return hipGetLastError();
}

hipError_t launch_feature_copy(const dvo_keypoint* skps, const float* sdesc, const int32_t* cnt, const int32_t* flags,
                               int kp_cap, int dim, dvo_keypoint* dkps, float* ddesc, int32_t* dn, hipStream_t s) {
    hipLaunchKernelGGL(feature_copy_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(skps),
                       reinterpret_cast<const uint4*>(sdesc), cnt, flags, kp_cap, dim, reinterpret_cast<uint32_t*>(dkps),
                       reinterpret_cast<uint4*>(ddesc), dn);
    return hipGetLastError();
}

hipError_t launch_ratio_gather_batch(const RatioBatchArgs& a, int pairs, hipStream_t s) {
    if (pairs < 1) return hipSuccess;
    hipLaunchKernelGGL(ratio_gather_batch_kernel, dim3(pairs), dim3(kRatioNT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_knn_frame_state(const int32_t* d_n, int frames, int cap, int32_t* d_fstate, hipStream_t s) {
    if (frames < 1) return hipSuccess;
    hipLaunchKernelGGL(knn_frame_state_kernel, dim3((frames + 63) / 64), dim3(64), 0, s, d_n, frames, cap, d_fstate);
    return hipGetLastError();
}

hipError_t launch_knn_status(const int32_t* d_n, const int32_t* d_fstate, const int32_t* d_missing, int pairs,
                             dvo_pair_record* records, hipStream_t s) {
    if (pairs < 1) return hipSuccess;
    hipLaunchKernelGGL(knn_status_kernel, dim3((pairs + 63) / 64), dim3(64), 0, s, d_n, d_fstate, d_missing, pairs,
                       records);
    return hipGetLastError();
}

}  // namespace dvo
