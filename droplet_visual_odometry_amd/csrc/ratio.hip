// The k-NN modes' ratio test and keypoint gather on the device (visual_odometry_v3.py:223-238,
// KeyPoint_convert :355, :358), and the feature-slot copy of dvo_knn_pair_run.
//
// ratio_gather_kernel takes the matcher's k = 2 output (BFMatcher NORM_L1 distances, or FLANN's
// squared L2), applies Python's test `m.distance < 0.75 * n.distance` and writes the kept matches,
// in ascending queryIdx order, as the point quads the geometry kernels read (GeomArgs::pts_f), the
// DMatch list, the count and the pair's PairHeader.  The order is part of the result: RANSAC's
// subsets index into the point list, so the slots come from a ballot / prefix scan, never from
// atomics.
#include "dvo_internal.h"

namespace dvo {

namespace {

constexpr int kRatioNT = 1024;  // one workgroup: 16 waves walk the queries 1024 at a time, in order

// Python's test on the float32 values DMatch.distance holds: the product and the compare are
// double (a float32 product 0.75f * d1 rounds and keeps a different set).
__global__ __launch_bounds__(kRatioNT) void ratio_gather_kernel(RatioArgs a) {
    __shared__ int wtot[kRatioNT / 64];
    __shared__ int wmiss[kRatioNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int2* idx2 = reinterpret_cast<const int2*>(a.idx);
    const float2* dist2 = reinterpret_cast<const float2*>(a.dist);
    int base = 0;  // matches kept by the chunks before this one
    bool missing = false;
    for (int q0 = 0; q0 < a.nq; q0 += kRatioNT) {
        const int q = q0 + tid;
        bool keep = false;
        int t = -1;
        float d0 = 0.f;
        if (q < a.nq) {
            const int2 id = idx2[q];
            const float2 dd = dist2[q];
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
            reinterpret_cast<int4*>(a.matches)[slot] = make_int4(q, t, 0, __float_as_int(d0));
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
        *a.hdr = PairHeader{a.nkq, a.nkt, 0, 0};
        *a.missing = any;
    }
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

}  // namespace

hipError_t launch_ratio_gather(const RatioArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(ratio_gather_kernel, dim3(1), dim3(kRatioNT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_feature_copy(const dvo_keypoint* skps, const float* sdesc, const int32_t* cnt, const int32_t* flags,
                               int kp_cap, int dim, dvo_keypoint* dkps, float* ddesc, int32_t* dn, hipStream_t s) {
    hipLaunchKernelGGL(feature_copy_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(skps),
                       reinterpret_cast<const uint4*>(sdesc), cnt, flags, kp_cap, dim, reinterpret_cast<uint32_t*>(dkps),
                       reinterpret_cast<uint4*>(ddesc), dn);
    return hipGetLastError();
}

}  // namespace dvo
