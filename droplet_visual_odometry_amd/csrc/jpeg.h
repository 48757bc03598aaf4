// Baseline JPEG (SOF0, 8-bit, Huffman, one interleaved scan): what the host parser (jpeg_parse.cpp)
// hands to the entropy decoder (jpeg_entropy.h) and to the kernels of jpeg.hip.  No HIP runtime
// here: the parser and the entropy decoder also build as plain host code (tests/jpeg_entropy_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define DVO_HD __host__ __device__
#else
#define DVO_HD
#endif

namespace dvo {
namespace jpeg {

enum { kOk = 0, kUnsupported = -7, kCorrupt = -8 };  // DVO_OK, DVO_EUNSUPPORTED, DVO_ECORRUPT

// A derived Huffman table (libjpeg's d_derived_tbl): codes of at most 8 bits are found by the next
// 8 bits of the stream, longer ones by comparing the next l bits with the largest code of length l.
struct HuffTable {
    uint16_t look[256];   // length << 8 | value; 0: no code of <= 8 bits starts these 8 bits
    int32_t maxcode[17];  // [l], l = 1..16: largest code of length l, -1 if there is none
    int32_t valptr[17];   // [l]: code c of length l has value vals[valptr[l] + c]
    uint8_t vals[256];
};

// One entropy-coded segment: the bytes between two restart markers (or the whole scan).
struct Segment {
    int32_t frame;    // index of its frame in the group
    uint32_t offset;  // first byte, from the start of the file (parser) or of the group's bytes (decoder)
    uint32_t length;
    int32_t mcu0, nmcu;  // MCUs [mcu0, mcu0 + nmcu) of the frame
};

// One frame.  Coefficients: int16, per component [block row][block column][64] in natural order,
// padded to whole MCUs, the components one after the other from element `base` of the group's
// buffer.  The u8 component planes have the same layout with a block's 64 samples spread over 8
// rows of its plane (pitch 8 bw[c]), so a frame's planes start at byte `base` of their buffer.
struct FramePlan {
    int32_t w, h, ncomp;
    int32_t hs, vs;  // luma sampling: 1x1 (gray, 4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0)
    int32_t mcux, mcuy, restart;
    int32_t bw[3], bh[3];  // blocks per row and block rows of each component
    int32_t blk0[3];       // first block of each component within the frame
    int32_t nblk;          // blocks of the frame
    int64_t base;
    uint16_t qt[3][64];  // per component, natural order
    HuffTable dc[3], ac[3];  // per component
};

struct Parsed {
    FramePlan plan;
    std::vector<Segment> segs;   // offsets from the start of the file; frame = 0
    size_t scan_begin = 0, scan_end = 0;  // the bytes the segments lie in
    int scan_status = kOk;       // kCorrupt: restart markers missing or in excess
    std::string why;             // of a status other than kOk
};

// Markers -> plan and segment list.  kOk, kUnsupported or kCorrupt; reads only buf[0, len).
int parse(const uint8_t* buf, size_t len, Parsed* out);

}  // namespace jpeg
}  // namespace dvo
