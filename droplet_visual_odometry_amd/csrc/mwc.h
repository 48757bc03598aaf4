// cv::RNG's multiply-with-carry generator and its jump-ahead, for the host and the device
// (geometry.hip: the RANSAC sample stream; flann.hip: the kd-forest's draws).
//
// The step is s' = (u32)s * A + (s >> 32), A = 4164903690.  With m = A * 2^32 - 1,
// s' * 2^32 = s + (u32)s * m, so s' = s * A (mod m) (A = 2^-32 mod m), and a state below m stays
// below m: from the second state of a stream on (the seed ~0 is the only state >= m it meets),
// s_{n+k} = s_n * A^k mod m exactly.  Products mod m are Montgomery products with R = 2^64.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace dvo {

constexpr uint64_t kMwcA = 4164903690ull;
constexpr uint64_t kMwcM = kMwcA * (1ull << 32) - 1;
constexpr uint64_t mwc_mprime() {  // -m^-1 mod 2^64 (Newton)
    uint64_t inv = kMwcM;
    for (int i = 0; i < 6; ++i) inv *= 2 - kMwcM * inv;
    return 0 - inv;
}
constexpr uint64_t kMwcMp = mwc_mprime();
static_assert(kMwcM % 2 == 1 && (uint64_t)(kMwcM * (0 - kMwcMp)) == 1, "Montgomery constants");
constexpr uint64_t kMwcAR = (uint64_t)((((unsigned __int128)kMwcA) << 64) % kMwcM);  // A * 2^64 mod m

__host__ __device__ __forceinline__ uint64_t mwc_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

__host__ __device__ __forceinline__ uint64_t mwc_mont(uint64_t a, uint64_t bR) {  // a * b mod m, a < m, bR = b * 2^64 mod m
    const uint64_t lo = a * bR, hi = mwc_mulhi(a, bR);
    const uint64_t u = lo * kMwcMp;
    const uint64_t uh = mwc_mulhi(u, kMwcM);
    uint64_t t = hi + uh;
    const bool c1 = t < hi;
    const uint64_t c = lo != 0;  // lo + u * m = 0 mod 2^64, with a carry unless lo == 0
    const uint64_t t2 = t + c;
    const bool c2 = t2 < t;
    return (c1 || c2 || t2 >= kMwcM) ? t2 - kMwcM : t2;
}

__host__ __device__ __forceinline__ uint64_t mwc_step(uint64_t s) { return (uint64_t)(uint32_t)s * kMwcA + (s >> 32); }

// The state k steps after s, for any k: s * A^k mod m by square-and-multiply.  A state at or
// above m takes one plain step first, which lands below 2 m; it is reduced once.
__host__ __device__ inline uint64_t mwc_jump_by(uint64_t s, uint64_t k) {
    if (k == 0) return s;
    if (s >= kMwcM) {
        s = mwc_step(s);
        --k;
    }
    uint64_t r = s >= kMwcM ? s - kMwcM : s;
    uint64_t bR = kMwcAR;  // A^(2^i) * 2^64 mod m
    for (; k; k >>= 1) {
        if (k & 1) r = mwc_mont(r, bR);
        bR = mwc_mont(bR, bR);
    }
    return r;
}

}  // namespace dvo
