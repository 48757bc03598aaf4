// Huffman decoding of one entropy-coded segment into coefficient blocks, written once for the host
// (dvo_jpeg_entropy_host, the host entropy path), the device (jpeg_entropy_kernel) and the
// sanitizer program (tests/jpeg_entropy_check.cpp).
//
// Every read is inside data[0, len).  Past the end, or from a marker on (FF not followed by 00),
// the bit reader feeds zero bytes and counts them; a block that has used bits of such a byte, a
// code that matches no table entry within 16 bits, a DC category above 15 and a coefficient index
// above 63 end the segment as corrupt.  Blocks not reached stay as they were (zero).
#pragma once

#include "jpeg.h"

namespace dvo {
namespace jpeg {

DVO_HD inline int zigzag(int k) {
    const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}

struct BitReader {
    const uint8_t* p;
    uint32_t len, pos;
    uint64_t acc;  // the low nbits bits are the unread ones
    int nbits;
    int fake;  // zero bytes fed after the end or a marker
    bool end;
};

// at least 32 unread bits
DVO_HD inline void refill(BitReader& r) {
    if (r.nbits > 32) return;
    if (!r.end && r.pos + 4 <= r.len) {
        uint32_t w;
        __builtin_memcpy(&w, r.p + r.pos, 4);
        const uint32_t t = ~w;  // a zero byte of t is an FF byte of w
        if (!((t - 0x01010101u) & ~t & 0x80808080u)) {
            r.acc = (r.acc << 32) | __builtin_bswap32(w);
            r.nbits += 32;
            r.pos += 4;
            return;
        }
    }
    while (r.nbits <= 56) {
        uint32_t b = 0;
        if (!r.end && r.pos < r.len) {
            b = r.p[r.pos];
            if (b != 0xFF) {
                r.pos += 1;
            } else if (r.pos + 1 < r.len && r.p[r.pos + 1] == 0) {
                r.pos += 2;  // FF 00 is the byte FF
            } else {
                r.end = true;
            }
        } else {
            r.end = true;
        }
        if (r.end) {
            b = 0;
            r.fake += 1;
        }
        r.acc = (r.acc << 8) | b;
        r.nbits += 8;
    }
}

// the next symbol, or -1 if no code matches (Reader: BitReader, or jpeg_split.h's SplitReader)
template <class Reader>
DVO_HD inline int huff_decode(Reader& r, const HuffTable& T) {
    refill(r);
    const uint32_t top = (uint32_t)(r.acc >> (r.nbits - 16)) & 0xFFFFu;
    const uint32_t e = T.look[top >> 8];
    if (e) {
        r.nbits -= (int)(e >> 8);
        return (int)(e & 255u);
    }
    for (int l = 9; l <= 16; ++l) {
        const int c = (int)(top >> (16 - l));
        if (c <= T.maxcode[l]) {
            const uint32_t idx = (uint32_t)(T.valptr[l] + c);
            if (idx >= 256u) return -1;
            r.nbits -= l;
            return T.vals[idx];
        }
    }
    return -1;
}

// s <= 15 bits as a signed value of category s
template <class Reader>
DVO_HD inline int receive_extend(Reader& r, int s) {
    if (s == 0) return 0;
    refill(r);
    const int v = (int)((r.acc >> (r.nbits - s)) & ((1u << s) - 1u));
    r.nbits -= s;
    return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

// MCUs [mcu0, mcu0 + nmcu) of the frame from data[0, len) into the frame's coefficients.
// 0, or 1 if the segment is corrupt.
DVO_HD inline int decode_segment(const FramePlan& P, const uint8_t* data, uint32_t len, int mcu0, int nmcu,
                                 int16_t* coef) {
    const int64_t total = (int64_t)P.mcux * P.mcuy;
    if (mcu0 < 0 || nmcu < 0 || (int64_t)mcu0 + nmcu > total) return 1;
    BitReader r{data, len, 0, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    for (int m = mcu0; m < mcu0 + nmcu; ++m) {
        const int my = m / P.mcux, mx = m - my * P.mcux;
        for (int c = 0; c < P.ncomp; ++c) {
            const int hc = c == 0 ? P.hs : 1, vc = c == 0 ? P.vs : 1;
            for (int by = 0; by < vc; ++by)
                for (int bx = 0; bx < hc; ++bx) {
                    const int64_t blk = P.blk0[c] + (int64_t)(my * vc + by) * P.bw[c] + (mx * hc + bx);
                    int16_t* o = coef + blk * 64;
                    int s = huff_decode(r, P.dc[c]);
                    if (s < 0 || s > 15) return 1;
                    pred[c] = (int)((uint32_t)pred[c] + (uint32_t)receive_extend(r, s));
                    o[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = huff_decode(r, P.ac[c]);
                        if (rs < 0) return 1;
                        s = rs & 15;
                        if (s == 0) {
                            if ((rs >> 4) != 15) break;
                            k += 16;
                            continue;
                        }
                        k += rs >> 4;
                        if (k > 63) return 1;
                        o[zigzag(k)] = (int16_t)receive_extend(r, s);
                        k += 1;
                    }
                    if (r.nbits < 8 * r.fake) return 1;  // the block used bits that the file does not have
                }
        }
    }
    return 0;
}

}  // namespace jpeg
}  // namespace dvo
