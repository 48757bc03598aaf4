// Baseline JPEG frames on gfx950: cv.imdecode(np_arr, IMREAD_COLOR) (scripts/visual_odometry_v3.py:127)
// with libjpeg-turbo's default arithmetic (JDCT_ISLOW, fancy upsampling), byte for byte, and the
// cvtColor(BGR2GRAY) that follows it (v3:132) folded into the last kernel.
//
// jpeg_entropy_kernel: one lane decodes one entropy-coded segment (jpeg_entropy.h) of any frame of
//   the group into that frame's zeroed int16 coefficient blocks.  Segment i belongs to lane
//   i / nwaves of wave i % nwaves, so while there are no more segments than waves every segment
//   has a wave of its own and no lane waits for a neighbour's branches; a group with more segments
//   than the launch has lanes (64 x 16,384) is decoded in rounds.  A wave whose segments are
//   all of one frame decodes from a copy of that frame's plan (its Huffman tables) in LDS.
// jpeg_entropy_split_kernel: one workgroup of up to 1,024 lanes decodes one long segment by the
//   schedule of jpeg_split.h, lane i taking the i-th run of split_bytes bytes: guessed entry states,
//   synchronisation passes until no exit state changes, a scan of block counts and DC sums, a
//   write pass.  States and scan live in LDS; a segment of more runs than lanes is walked in chunks.
//   The workgroup (LANES: 64 .. 1,024) is the smallest that holds the longest segment of the launch:
//   what a workgroup keeps in LDS grows with it, and with it falls the number a CU runs at a time.
// jpeg_idct_kernel: 8 lanes per block.  Lane j fetches row j of the block as one 16-byte load and
//   dequantises it into LDS, reads back column j and runs pass 1 (jidctint.c, descale 11), writes
//   the column back, reads row j, runs pass 2 (descale 18), and stores 8 samples of the component's
//   u8 plane as one 8-byte word.
// jpeg_color_kernel<OUT>: one lane makes 4 pixels of a row: chroma upsampling (jdsample.c: h2v1 /
//   h2v2 "fancy" triangle filters over the real chroma width and height, replication when that
//   width is <= 2), YCbCr -> BGR (jdcolor.c's 16-bit fixed point), and a word store of 4 gray
//   bytes (OUT 1, no BGR is stored), 12 BGR bytes (OUT 3) or 16 BGRA bytes (OUT 4, A = 255).
// No kernel reads or writes outside the planes' whole-MCU extent or the w x h x OUT bytes of dst.
#include <cstddef>

#include "dvo_internal.h"
#include "jpeg_entropy.h"
#include "jpeg_split.h"

namespace dvo {
namespace {

using jpeg::FramePlan;
using jpeg::Segment;

static_assert(offsetof(FramePlan, qt) % 16 == 0 && sizeof(FramePlan) % 16 == 0, "qt rows are read as 16-byte words");

constexpr int kEntropyWaves = 16384;  // waves of one entropy launch

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const FramePlan* __restrict__ plans,
                                                          const Segment* __restrict__ segs, int nseg, int nwaves,
                                                          const uint8_t* __restrict__ bytes,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ FramePlan lp;
    // Round r gives the wave segments r 64 nwaves + blockIdx.x + lane nwaves; the launch has at most
    // kEntropyWaves waves, so a group with more than 64 of them per wave takes several rounds.  The
    // round's first segment is lane 0's, so the loop is the same for the whole wave.
    for (int64_t first = blockIdx.x; first < nseg; first += (int64_t)64 * nwaves) {
        const int64_t i = first + (int64_t)threadIdx.x * nwaves;
        const bool on = i < nseg;
        Segment sg{};
        if (on) sg = segs[i];
        // When the wave's segments belong to one frame (always, while every segment has its own wave)
        // its plan is copied to LDS: the decoder's table look-ups are a chain of dependent loads.
        const int f0 = __shfl(sg.frame, 0);
        const bool one = __all(!on || sg.frame == f0);
        if (one) {
            const uint4* src = reinterpret_cast<const uint4*>(plans + f0);
            uint4* dst = reinterpret_cast<uint4*>(&lp);
            for (int k = threadIdx.x; k < (int)(sizeof(FramePlan) / sizeof(uint4)); k += 64) dst[k] = src[k];
        }
        __syncthreads();
        if (on) {
            int bad;
            if (one)
                bad = jpeg::decode_segment(lp, bytes + sg.offset, sg.length, sg.mcu0, sg.nmcu, coef + lp.base);
            else
                bad = jpeg::decode_segment(plans[sg.frame], bytes + sg.offset, sg.length, sg.mcu0, sg.nmcu,
                                           coef + plans[sg.frame].base);
            if (bad) status[sg.frame] = jpeg::kCorrupt;
        }
        __syncthreads();  // before the next round's plan replaces this one
    }
}

// exclusive sum of v over the workgroup's lanes (whole waves); tot: one word per wave
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t* tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += tot[w];
    return before + inc - v;
}

// info: [0] most synchronisation passes of a segment, [1] segments decoded here, [2] of them by the one-lane fallback
template <int LANES>
__global__ __launch_bounds__(LANES) void jpeg_entropy_split_kernel(
    const FramePlan* __restrict__ plans, const Segment* __restrict__ segs, int nseg, uint32_t split_bytes,
    const uint8_t* __restrict__ bytes, int16_t* __restrict__ coef, int32_t* __restrict__ status,
    int32_t* __restrict__ info) {
    __shared__ FramePlan lp;
    static_assert(LANES % 64 == 0 && LANES <= jpeg::kSplitLanes, "whole waves, at most the model's chunk");
    __shared__ uint64_t s_exit[LANES];
    __shared__ uint32_t s_tot[4][LANES / 64];
    __shared__ uint64_t c_state, c_ord;
    __shared__ uint32_t c_dc[3];
    if ((int)blockIdx.x >= nseg) return;
    const Segment sg = segs[blockIdx.x];
    const int t = threadIdx.x, L = LANES;
    {
        const uint4* src = reinterpret_cast<const uint4*>(plans + sg.frame);
        uint4* dst = reinterpret_cast<uint4*>(&lp);
        for (int k = t; k < (int)(sizeof(FramePlan) / sizeof(uint4)); k += L) dst[k] = src[k];
    }
    if (t == 0) {
        c_state = jpeg::pack_state(0, 0, 0);
        c_ord = 0;
        c_dc[0] = c_dc[1] = c_dc[2] = 0;
    }
    __syncthreads();
    const uint8_t* data = bytes + sg.offset;
    const uint32_t len = sg.length, S = split_bytes;
    const uint32_t n = jpeg::split_count(len, S);
    int16_t* fcoef = coef + lp.base;
    // (the host sends segments of at least two runs; decode_segment refuses a bad MCU range itself)
    if (n < 2 || sg.mcu0 < 0 || sg.nmcu < 0 || (int64_t)sg.mcu0 + sg.nmcu > (int64_t)lp.mcux * lp.mcuy) {
        if (t == 0 && jpeg::decode_segment(lp, data, len, sg.mcu0, sg.nmcu, fcoef)) status[sg.frame] = jpeg::kCorrupt;
        return;
    }
    const uint64_t total = (uint64_t)sg.nmcu * (uint64_t)jpeg::blocks_per_mcu(lp);
    int bad = 0, np = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += (uint32_t)L) {
        const int nl = (int)min(n - c0, (uint32_t)L);
        const bool on = t < nl;
        const uint32_t g = c0 + (uint32_t)t;
        const uint64_t end_bit = on ? jpeg::split_end(len, S, g) : 0;
        uint64_t entry = jpeg::kDead;
        if (on) entry = t == 0 ? c_state : jpeg::split_guess(data, len, S, g);
        jpeg::LaneResult res{jpeg::kDead, 0, {0, 0, 0}, -1};
        // Pass 0 from the guesses, then passes while an exit state changed: lane i's entry is final
        // after pass i (jpeg_split.h), so pass nl - 1 is the last there can be, whatever the bytes.
        bool need = on;
        for (int pass = 0;; ++pass) {
            int changed = 0;
            if (need) {
                const jpeg::LaneResult r = jpeg::run(lp, data, len, entry, end_bit, nullptr);
                if (pass == 0 || r.exit != res.exit) {
                    changed = 1;
                    s_exit[t] = r.exit;
                }
                res = r;
            }
            const int any = __syncthreads_or(changed);  // the exits of this pass are written
            if (pass > 0) ++np;
            if ((pass > 0 && !any) || pass + 1 >= nl) break;
            const uint64_t e = on && t > 0 ? s_exit[t - 1] : entry;
            need = on && t > 0 && e != entry;
            entry = e;
            __syncthreads();  // ... and read, before the next pass writes
        }
        const uint32_t b0 = block_exclusive_sum(on ? res.blocks : 0u, s_tot[0]);
        const uint32_t d0 = block_exclusive_sum(on ? res.dc[0] : 0u, s_tot[1]);
        const uint32_t d1 = block_exclusive_sum(on ? res.dc[1] : 0u, s_tot[2]);
        const uint32_t d2 = block_exclusive_sum(on ? res.dc[2] : 0u, s_tot[3]);
        jpeg::CoefSink sink{fcoef, c_ord + b0, total, sg.mcu0, {c_dc[0] + d0, c_dc[1] + d1, c_dc[2] + d2}};
        const int err = on && res.err_block >= 0 && sink.first + (uint64_t)res.err_block < total;
        bad = __syncthreads_or(err);  // every lane has read the carried values
        if (bad) break;
        if (on) jpeg::run(lp, data, len, entry, end_bit, &sink);
        if (t == nl - 1) {
            c_state = res.exit;
            c_ord = sink.first + res.blocks;
            for (int c = 0; c < 3; ++c) c_dc[c] = sink.pred[c] + res.dc[c];
        }
        __syncthreads();
    }
    if (t != 0) return;
    if (!bad && c_ord < total) bad = 1;  // the data ended between two blocks
    // A corrupt segment is decode_segment's business: the blocks before the first bad one, that one
    // in part.  Chunks already written hold only what it writes to the same places.
    if (bad && jpeg::decode_segment(lp, data, len, sg.mcu0, sg.nmcu, fcoef)) status[sg.frame] = jpeg::kCorrupt;
    if (info) {
        atomicMax(&info[0], np);
        atomicAdd(&info[1], 1);
        if (bad) atomicAdd(&info[2], 1);
    }
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of jpeg_idct_islow over v[0..7], results descaled by n
__device__ __forceinline__ void idct8(int* v, int n) {
    int z1 = (v[2] + v[6]) * 4433;
    const int t2 = z1 - v[6] * 15137, t3 = z1 + v[2] * 6270;
    const int t0 = (v[0] + v[4]) * 8192, t1 = (v[0] - v[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a = v[7], b = v[5], c = v[3], d = v[1];
    z1 = a + d;
    int z2 = b + c, z3 = a + c, z4 = b + d;
    const int z5 = (z3 + z4) * 9633;
    a *= 2446, b *= 16819, c *= 25172, d *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    a += z1 + z3, b += z2 + z4, c += z2 + z3, d += z1 + z4;
    v[0] = descale(t10 + d, n), v[7] = descale(t10 - d, n);
    v[1] = descale(t11 + c, n), v[6] = descale(t11 - c, n);
    v[2] = descale(t12 + b, n), v[5] = descale(t12 - b, n);
    v[3] = descale(t13 + a, n), v[4] = descale(t13 - a, n);
}

__device__ __forceinline__ uint32_t clamp255(int x) { return (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

constexpr int kIdctBlocks = 32;  // 8 x 8 blocks per 256 lanes

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const FramePlan* __restrict__ plans,
                                                        const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes) {
    __shared__ int tile[kIdctBlocks][8][9];
    const FramePlan& P = plans[blockIdx.y];
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int b = blockIdx.x * kIdctBlocks + lb;  // block of the frame
    const bool on = b < P.nblk;
    const int c = on && P.ncomp > 1 && b >= P.blk0[1] ? (b >= P.blk0[2] ? 2 : 1) : 0;
    int v[8];
    if (on) {
        const uint4 q = *reinterpret_cast<const uint4*>(coef + P.base + (int64_t)b * 64 + j * 8);
        const uint4 t = *reinterpret_cast<const uint4*>(&P.qt[c][j * 8]);
        const uint32_t qw[4] = {q.x, q.y, q.z, q.w}, tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cf = (int16_t)(qw[i >> 1] >> (16 * (i & 1)));
            const int qv = (int)((tw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            tile[lb][j][i] = cf * qv;
        }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[lb][i][j];
        idct8(v, 11);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[lb][i][j] = v[i];
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[lb][j][i];
        idct8(v, 18);
        uint2 o;
        o.x = clamp255(v[0] + 128) | clamp255(v[1] + 128) << 8 | clamp255(v[2] + 128) << 16 | clamp255(v[3] + 128) << 24;
        o.y = clamp255(v[4] + 128) | clamp255(v[5] + 128) << 8 | clamp255(v[6] + 128) << 16 | clamp255(v[7] + 128) << 24;
        const int k = b - P.blk0[c], brow = k / P.bw[c], bcol = k - brow * P.bw[c];
        uint8_t* d = planes + P.base + (int64_t)P.blk0[c] * 64 + (int64_t)(brow * 8 + j) * (P.bw[c] * 8) + bcol * 8;
        *reinterpret_cast<uint2*>(d) = o;
    }
}

// 4 chroma samples for pixels x0 .. x0 + 3 of row y from a subsampled plane (pitch cp)
__device__ __forceinline__ void chroma4(const FramePlan& P, const uint8_t* __restrict__ plane, int cp, int x0, int y,
                                        int* out) {
    if (P.hs == 1) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(plane + (int64_t)y * cp + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (int)((w >> (8 * j)) & 255u);
        return;
    }
    const int cw = (P.w + 1) >> 1, chh = P.vs == 2 ? (P.h + 1) >> 1 : P.h;
    const int r0 = P.vs == 2 ? y >> 1 : y;
    const uint8_t* p0 = plane + (int64_t)r0 * cp;
    const int i0 = x0 >> 1;
    if (cw <= 2) {  // jdsample.c replicates when the chroma plane is at most 2 wide
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = p0[min(i0 + (j >> 1), cw - 1)];
        return;
    }
    int ix[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) ix[t] = min(max(i0 - 1 + t, 0), cw - 1);
    if (P.vs == 1) {
        int s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = p0[ix[t]];
        out[0] = (3 * s[1] + s[0] + 1) >> 2;
        out[1] = (3 * s[1] + s[2] + 2) >> 2;
        out[2] = (3 * s[2] + s[1] + 1) >> 2;
        out[3] = (3 * s[2] + s[3] + 2) >> 2;
    } else {
        const int r1 = (y & 1) ? min(r0 + 1, chh - 1) : max(r0 - 1, 0);
        const uint8_t* p1 = plane + (int64_t)r1 * cp;
        int s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = 3 * p0[ix[t]] + p1[ix[t]];
        out[0] = (3 * s[1] + s[0] + 8) >> 4;
        out[1] = (3 * s[1] + s[2] + 7) >> 4;
        out[2] = (3 * s[2] + s[1] + 8) >> 4;
        out[3] = (3 * s[2] + s[3] + 7) >> 4;
    }
}

template <int OUT>
__global__ __launch_bounds__(256) void jpeg_color_kernel(GrayCoef gc, const FramePlan* __restrict__ plans,
                                                         const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ dst, int64_t dst_fstride,
                                                         int dst_pitch) {
    const FramePlan& P = plans[blockIdx.z];
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= P.w || y >= P.h) return;
    const uint8_t* base = planes + P.base;
    const uint32_t yw = *reinterpret_cast<const uint32_t*>(base + (int64_t)y * (P.bw[0] * 8) + x0);
    uint32_t px[4];  // B | G << 8 | R << 16 | 255 << 24, or the gray byte
    if (P.ncomp == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t Y = (yw >> (8 * j)) & 255u;  // B = G = R = Y
            px[j] = OUT == 1 ? (uint32_t)(((int)Y * (gc.cb + gc.cg + gc.cr) + (1 << (gc.shift - 1))) >> gc.shift)
                             : Y * 0x010101u | 0xFF000000u;
        }
    } else {
        int cb[4], cr[4];
        const int cp = P.bw[1] * 8;
        chroma4(P, base + (int64_t)P.blk0[1] * 64, cp, x0, y, cb);
        chroma4(P, base + (int64_t)P.blk0[2] * 64, cp, x0, y, cr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int Y = (int)((yw >> (8 * j)) & 255u), u = cb[j] - 128, v = cr[j] - 128;
            const uint32_t R = clamp255(Y + ((91881 * v + 32768) >> 16));
            const uint32_t G = clamp255(Y + ((-22554 * u - 46802 * v + 32768) >> 16));
            const uint32_t B = clamp255(Y + ((116130 * u + 32768) >> 16));
            px[j] = OUT == 1 ? (uint32_t)(((int)B * gc.cb + (int)G * gc.cg + (int)R * gc.cr + (1 << (gc.shift - 1))) >> gc.shift)
                             : B | G << 8 | R << 16 | 0xFF000000u;
        }
    }
    uint8_t* d = dst + (int64_t)blockIdx.z * dst_fstride + (int64_t)y * dst_pitch + (int64_t)x0 * OUT;
    const bool whole = x0 + 4 <= P.w;
    if (OUT == 1) {
        if (whole && ((uintptr_t)d & 3) == 0) {
            *reinterpret_cast<uint32_t*>(d) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
        } else {
            for (int j = 0; j < 4 && x0 + j < P.w; ++j) d[j] = (uint8_t)px[j];
        }
    } else if (OUT == 3) {
        if (whole && ((uintptr_t)d & 3) == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(d);
            o[0] = (px[0] & 0xFFFFFFu) | px[1] << 24;
            o[1] = ((px[1] >> 8) & 0xFFFFu) | px[2] << 16;
            o[2] = ((px[2] >> 16) & 0xFFu) | px[3] << 8;
        } else {
            for (int j = 0; j < 4 && x0 + j < P.w; ++j)
                for (int k = 0; k < 3; ++k) d[3 * j + k] = (uint8_t)(px[j] >> (8 * k));
        }
    } else {
        if (whole && ((uintptr_t)d & 15) == 0) {
            *reinterpret_cast<uint4*>(d) = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
            for (int j = 0; j < 4 && x0 + j < P.w; ++j)
                for (int k = 0; k < 4; ++k) d[4 * j + k] = (uint8_t)(px[j] >> (8 * k));
        }
    }
}

}  // namespace

hipError_t launch_jpeg_entropy(const jpeg::FramePlan* d_plans, const jpeg::Segment* d_segs, int nseg,
                               const uint8_t* d_bytes, int16_t* d_coef, int32_t* d_status, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    const int nwaves = std::min(nseg, kEntropyWaves);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(nwaves), dim3(64), 0, s, d_plans, d_segs, nseg, nwaves, d_bytes, d_coef,
                       d_status);
    return hipGetLastError();
}

hipError_t launch_jpeg_entropy_split(const jpeg::FramePlan* d_plans, const jpeg::Segment* d_segs, int nseg, int split_bytes,
                                     int max_runs, const uint8_t* d_bytes, int16_t* d_coef, int32_t* d_status,
                                     int32_t* d_info, hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    if (!jpeg::split_bytes_ok(split_bytes)) return hipErrorInvalidValue;
#define DVO_SPLIT_LAUNCH(LANES)                                                                                  \
    hipLaunchKernelGGL(jpeg_entropy_split_kernel<LANES>, dim3(nseg), dim3(LANES), 0, s, d_plans, d_segs, nseg, \
                       (uint32_t)split_bytes, d_bytes, d_coef, d_status, d_info)
    if (max_runs <= 64)
        DVO_SPLIT_LAUNCH(64);
    else if (max_runs <= 128)
        DVO_SPLIT_LAUNCH(128);
    else if (max_runs <= 256)
        DVO_SPLIT_LAUNCH(256);
    else if (max_runs <= 512)
        DVO_SPLIT_LAUNCH(512);
    else
        DVO_SPLIT_LAUNCH(1024);
#undef DVO_SPLIT_LAUNCH
    return hipGetLastError();
}

hipError_t launch_jpeg_idct(const jpeg::FramePlan* d_plans, int nframes, int max_nblk, const int16_t* d_coef,
                            uint8_t* d_planes, hipStream_t s) {
    if (nframes <= 0 || max_nblk <= 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_nblk + kIdctBlocks - 1) / kIdctBlocks, nframes), dim3(256), 0, s,
                       d_plans, d_coef, d_planes);
    return hipGetLastError();
}

hipError_t launch_jpeg_color(const GrayCoef& c, const jpeg::FramePlan* d_plans, int nframes, int w, int h,
                             const uint8_t* d_planes, int out_channels, uint8_t* d_dst, int64_t dst_fstride,
                             int dst_pitch, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    const dim3 grid((w + 255) / 256, (h + 3) / 4, nframes);
    if (out_channels == 1)
        hipLaunchKernelGGL(jpeg_color_kernel<1>, grid, dim3(256), 0, s, c, d_plans, d_planes, d_dst, dst_fstride, dst_pitch);
    else if (out_channels == 3)
        hipLaunchKernelGGL(jpeg_color_kernel<3>, grid, dim3(256), 0, s, c, d_plans, d_planes, d_dst, dst_fstride, dst_pitch);
    else if (out_channels == 4)
        hipLaunchKernelGGL(jpeg_color_kernel<4>, grid, dim3(256), 0, s, c, d_plans, d_planes, d_dst, dst_fstride, dst_pitch);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace dvo
