// Colour frames on gfx950: the first step of the reference's frame path,
// cv.cvtColor(image_np, COLOR_BGR2GRAY) (scripts/visual_odometry_v3.py:132), alone and fused
// into the cv.undistort that follows it (v3:133).
//
// Gray is OpenCV's 8-bit fixed point of the pixel's bytes in B, G, R order,
//   Y = (B cb + G cg + R cr + (1 << (shift - 1))) >> shift,
// with the weights and the shift passed as an argument (GrayCoef); a fourth byte is ignored.
//
// bgr2gray_kernel<C>: one lane makes 4 consecutive gray pixels and stores them as one word (the
//   shape of undistort_remap_kernel).  Its 4 C source bytes are three dword loads (C = 3:
//   consecutive lanes read consecutive 12-byte runs) or one 16-byte load (C = 4) when the source
//   row allows it; rows at other addresses and the last w % 4 pixels of a row are read byte by
//   byte.  No lane reads past w C bytes of a source row or writes past w bytes of a destination row.
// undistort_remap_bgr_kernel<C>: undistort_remap_kernel over the gray image of a colour frame
//   without storing that image: each of the four taps is converted on its own and the same
//   weights, rounding and clamp follow, so the result is remap(gray) byte for byte.  A tap outside
//   the source is gray 0 and is not read.
// Source and destination must not overlap (both kernels read the source through __restrict__).
#include "dvo_internal.h"

namespace dvo {
namespace {

__device__ __forceinline__ int gray_of(const GrayCoef& c, int b, int g, int r) {
    return (b * c.cb + g * c.cg + r * c.cr + (1 << (c.shift - 1))) >> c.shift;
}

__device__ __forceinline__ int gray_at(const GrayCoef& c, const uint8_t* p) { return gray_of(c, p[0], p[1], p[2]); }

// byte k of a little-endian word run
__device__ __forceinline__ int byte_of(const uint32_t* v, int k) { return (int)((v[k >> 2] >> (8 * (k & 3))) & 255u); }

template <int C>
__global__ __launch_bounds__(256) void bgr2gray_kernel(GrayCoef coef, const uint8_t* __restrict__ src,
                                                       int64_t src_fstride, int src_pitch, int w, int h,
                                                       uint8_t* __restrict__ dst, int64_t dst_fstride,
                                                       int dst_pitch) {
    const int f = blockIdx.z;
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    const uint8_t* s = src + (int64_t)f * src_fstride + (int64_t)y * src_pitch;  // the row
    uint8_t* d = dst + (int64_t)f * dst_fstride + (int64_t)y * dst_pitch;
    const bool whole = x0 + 4 <= w;
    uint32_t word = 0;
    if (whole && ((uintptr_t)s & 3) == 0) {
        // x0 is a multiple of 4, so the lane's run starts 12 (C = 3) or 16 (C = 4) bytes apart
        uint32_t v[4];
        const uint8_t* p = s + (int64_t)x0 * C;
        if (C == 4 && ((uintptr_t)s & 15) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) v[k] = reinterpret_cast<const uint32_t*>(p)[k];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            word |= (uint32_t)gray_of(coef, byte_of(v, j * C), byte_of(v, j * C + 1), byte_of(v, j * C + 2)) << (8 * j);
    } else {
        for (int j = 0; j < 4 && x0 + j < w; ++j) word |= (uint32_t)gray_at(coef, s + (int64_t)(x0 + j) * C) << (8 * j);
    }
    if (whole && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d + x0) = word;
    } else {
        for (int j = 0; j < 4 && x0 + j < w; ++j) d[x0 + j] = (uint8_t)(word >> (8 * j));
    }
}

// remap_px of undistort.hip with every tap converted from C-byte pixels
template <int C>
__device__ __forceinline__ uint32_t remap_px_bgr(const GrayCoef& c, const uint8_t* src, int sw, int sh, int sp, int sx,
                                                 int sy, int a) {
    const int ty = a >> 5, tx = a & 31;
    const int w00 = (32 - ty) * (32 - tx) * 32, w01 = (32 - ty) * tx * 32, w10 = ty * (32 - tx) * 32, w11 = ty * tx * 32;
    int v00, v01, v10, v11;
    if ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1)) {
        // the two horizontal taps of a source row are 2 C contiguous bytes
        const uint8_t* S = src + (int64_t)sy * sp + (int64_t)sx * C;
        v00 = gray_at(c, S);
        v01 = gray_at(c, S + C);
        v10 = gray_at(c, S + sp);
        v11 = gray_at(c, S + sp + C);
    } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        return 0;
    } else {
        auto pix = [&](int x, int y) {
            return (x >= 0 && x < sw && y >= 0 && y < sh) ? gray_at(c, src + (int64_t)y * sp + (int64_t)x * C) : 0;
        };
        v00 = pix(sx, sy);
        v01 = pix(sx + 1, sy);
        v10 = pix(sx, sy + 1);
        v11 = pix(sx + 1, sy + 1);
    }
    const int r = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
    return (uint32_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

template <int C>
__global__ __launch_bounds__(256) void undistort_remap_bgr_kernel(UndistortGeom U, GrayCoef coef,
                                                                  const int16_t* __restrict__ xy,
                                                                  const uint16_t* __restrict__ frac,
                                                                  const uint8_t* __restrict__ src, int64_t src_fstride,
                                                                  int src_pitch, uint8_t* __restrict__ dst,
                                                                  int64_t dst_fstride, int dst_pitch) {
    const int f = blockIdx.z;
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= U.w || y >= U.h) return;
    const uint8_t* s = src + (int64_t)f * src_fstride;
    uint8_t* d = dst + (int64_t)f * dst_fstride + (int64_t)y * dst_pitch;
    const int16_t* m1 = xy + ((int64_t)y * U.w + x0) * 2;
    const uint16_t* m2 = frac + (int64_t)y * U.w + x0;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < U.w)
            word |= remap_px_bgr<C>(coef, s, U.w, U.h, src_pitch, m1[2 * j], m1[2 * j + 1], m2[j] & 1023) << (8 * j);
    if (x0 + 4 <= U.w && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d + x0) = word;
    } else {
        for (int j = 0; j < 4 && x0 + j < U.w; ++j) d[x0 + j] = (uint8_t)(word >> (8 * j));
    }
}

constexpr int kMaxGridZ = 65535;

}  // namespace

hipError_t launch_bgr2gray(const GrayCoef& c, const uint8_t* d_src, int n, int64_t src_fstride, int src_pitch,
                           int channels, int w, int h, uint8_t* d_dst, int64_t dst_fstride, int dst_pitch,
                           hipStream_t s) {
    if (channels != 3 && channels != 4) return hipErrorInvalidValue;
    for (int f0 = 0; f0 < n; f0 += kMaxGridZ) {
        dim3 grid((w + 255) / 256, (h + 3) / 4, std::min(n - f0, kMaxGridZ));
        const uint8_t* src = d_src + f0 * src_fstride;
        uint8_t* dst = d_dst + f0 * dst_fstride;
        if (channels == 3)
            hipLaunchKernelGGL(bgr2gray_kernel<3>, grid, dim3(256), 0, s, c, src, src_fstride, src_pitch, w, h, dst,
                               dst_fstride, dst_pitch);
        else
            hipLaunchKernelGGL(bgr2gray_kernel<4>, grid, dim3(256), 0, s, c, src, src_fstride, src_pitch, w, h, dst,
                               dst_fstride, dst_pitch);
    }
    return hipGetLastError();
}

hipError_t launch_undistort_remap_bgr(const UndistortGeom& U, const int16_t* d_xy, const uint16_t* d_frac,
                                      const GrayCoef& c, const uint8_t* d_src, int n, int64_t src_fstride,
                                      int src_pitch, int channels, uint8_t* d_dst, int64_t dst_fstride,
                                      int dst_pitch, hipStream_t s) {
    if (channels != 3 && channels != 4) return hipErrorInvalidValue;
    for (int f0 = 0; f0 < n; f0 += kMaxGridZ) {
        dim3 grid((U.w + 255) / 256, (U.h + 3) / 4, std::min(n - f0, kMaxGridZ));
        const uint8_t* src = d_src + f0 * src_fstride;
        uint8_t* dst = d_dst + f0 * dst_fstride;
        if (channels == 3)
            hipLaunchKernelGGL(undistort_remap_bgr_kernel<3>, grid, dim3(256), 0, s, U, c, d_xy, d_frac, src,
                               src_fstride, src_pitch, dst, dst_fstride, dst_pitch);
        else
            hipLaunchKernelGGL(undistort_remap_bgr_kernel<4>, grid, dim3(256), 0, s, U, c, d_xy, d_frac, src,
                               src_fstride, src_pitch, dst, dst_fstride, dst_pitch);
    }
    return hipGetLastError();
}

}  // namespace dvo
