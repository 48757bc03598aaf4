// One entropy-coded segment decoded by many lanes: self-synchronising parallel Huffman decoding,
// written once for the host model (decode_segment_split: dvo_jpeg_entropy_split_host, the
// sanitizer program tests/jpeg_split_check.cpp) and the device (jpeg_entropy_split_kernel).  The
// result is decode_segment's (jpeg_entropy.h), coefficient for coefficient and status for status.
//
// The segment is cut into subsequences of split_bytes bytes, one lane each.  A lane's state is
// where its next symbol starts: the bit position in the raw segment, the block slot within the MCU
// (it selects the component, so the tables) and the zigzag index k (0: a DC code comes next).
//
// The position is canonical: byte index x 8 + bit, where the byte is the raw index of the data
// byte the bit lies in, never the 00 of an FF 00 pair (that byte belongs to its FF).  Two decoders
// that have consumed the same bits report the same value whatever they have prefetched.  The
// stuffing stays in the bytes and the reader reports the position exactly, for two reasons:
// removing it on the host would turn the copy into pinned staging from a memcpy into a byte loop
// on the one core that feeds the device, and segments below the split threshold go to the
// one-lane kernel in the same group, which reads stuffed bytes.  SplitReader is BitReader with one
// more shift register: bit j says that the j-th last byte fetched took two raw bytes, so the
// raw index of the first unread byte is pos - bytes held - stuffed pairs among them.
//
// Schedule, per chunk of at most `lanes` subsequences (the kernel's workgroup; the model uses
// kSplitLanes), with the last lane's exit state, block count and DC sums carried into the next:
//   pass 0   lane i decodes its subsequence from a guess (its first bit, slot 0, k 0) with no
//            sink; lane 0 starts from the true (carried) state.
//   pass p   lane i >= 1 whose left neighbour's exit state of pass p - 1 differs from the entry
//            it last ran with runs again from that state; a changed exit state is stored for pass
//            p + 1.  Repeat while any lane's exit changed.
//            Termination: lane 0's entry is true, so its exit is final after pass 0, so lane 1's
//            entry is final in pass 1, and so on: lane i's entry is final after pass i and the
//            loop ends after at most lanes - 1 passes, whatever the bytes are.  Every run walks
//            its subsequence plus at most one symbol (each symbol consumes at least one bit), so
//            adversarial bytes cost at most lanes x one lane's walk, today's one-lane decode.
//   scan     exclusive sums of (blocks completed, three DC sums) give each lane the ordinal of the
//            block it enters in and the DC predictors there.  The sums of DC differences wrap at
//            32 bits as decode_segment's pred does, and wrapping sums are associative, so scan +
//            local sum has the same low 16 bits that decode_segment stores.
//   write    every lane runs once more from its final entry with the coefficient sink.
// Errors are decode_segment's (no matching code, DC category above 15, k > 63, bits the file does
// not have).  A lane notes the first it meets and goes on with the next block: lanes that started
// from a guess meet errors all the time and still have to fall into step, and after the first
// error of a lane that started from the true state nothing counts any more (block ordinals only
// grow).  decode_segment looks for the last kind at a block's end; once a block has used such a
// bit it cannot end well, so here the symbol that uses one is the error, and as there is nothing
// left to decode the lane leaves the dead state: lanes entered dead do nothing.  An error counts
// only if its block ordinal
// lies inside the segment's nmcu x blocks-per-MCU: the last lanes run on into the padding bits and
// the zeros fed after the end, which decode_segment never looks at.  A segment with an error that
// counts, or with fewer blocks than it should have, is decoded again by decode_segment on one
// lane, before the chunk's write pass.  Earlier chunks have then written only what decode_segment
// writes to the same places (their lanes ran from true states and met no error), so nothing needs
// zeroing.
#pragma once

#include <vector>

#include "jpeg_entropy.h"

namespace dvo {
namespace jpeg {

constexpr int kSplitLanes = 1024;  // subsequences of one chunk: the lanes of the kernel's largest workgroup
constexpr int kSplitBytesMin = 16, kSplitBytesMax = 4096;  // a symbol is at most 31 bits: none jumps over a subsequence

DVO_HD inline bool split_bytes_ok(int s) { return s >= kSplitBytesMin && s <= kSplitBytesMax && (s & (s - 1)) == 0; }

// ---- lane state: pos (40 bits) | slot << 40 (4 bits) | k << 44 (6 bits); all ones: dead ----
constexpr uint64_t kDead = ~(uint64_t)0;
DVO_HD inline uint64_t pack_state(uint64_t pos, int slot, int k) {
    return (pos & (((uint64_t)1 << 40) - 1)) | (uint64_t)slot << 40 | (uint64_t)k << 44;
}
DVO_HD inline uint64_t state_pos(uint64_t s) { return s & (((uint64_t)1 << 40) - 1); }
DVO_HD inline int state_slot(uint64_t s) { return (int)(s >> 40) & 15; }
DVO_HD inline int state_k(uint64_t s) { return (int)(s >> 44) & 63; }

struct SplitReader {
    const uint8_t* p;
    uint32_t len;
    uint64_t pos;  // raw index of the next byte to fetch; counts on over the zero bytes fed after the end
    uint64_t acc;  // the low nbits bits are the unread ones
    int nbits;
    int fake;  // zero bytes fed after the end or a marker
    bool end;
    uint32_t stuffed;  // bit j: the j-th last byte fetched was the FF of an FF 00 pair
};

// at least 32 unread bits
DVO_HD inline void refill(SplitReader& r) {
    if (r.nbits > 32) return;
    if (!r.end && r.pos + 4 <= r.len) {
        uint32_t w;
        __builtin_memcpy(&w, r.p + r.pos, 4);
        const uint32_t t = ~w;  // a zero byte of t is an FF byte of w
        if (!((t - 0x01010101u) & ~t & 0x80808080u)) {
            r.acc = (r.acc << 32) | __builtin_bswap32(w);
            r.nbits += 32;
            r.pos += 4;
            r.stuffed <<= 4;
            return;
        }
    }
    while (r.nbits <= 56) {
        uint32_t b = 0, st = 0;
        if (!r.end && r.pos < r.len) {
            b = r.p[r.pos];
            if (b != 0xFF) {
                r.pos += 1;
            } else if (r.pos + 1 < r.len && r.p[r.pos + 1] == 0) {
                r.pos += 2;  // FF 00 is the byte FF
                st = 1;
            } else {
                r.end = true;
            }
        } else {
            r.end = true;
        }
        if (r.end) {
            b = 0;
            r.fake += 1;
            r.pos += 1;
        }
        r.acc = (r.acc << 8) | b;
        r.nbits += 8;
        r.stuffed = r.stuffed << 1 | st;
    }
}

// the canonical position of the next unread bit
DVO_HD inline uint64_t position(const SplitReader& r) {
    const int nb = (r.nbits + 7) >> 3;  // bytes held, the one partly read included: at most 8
    const int pairs = __builtin_popcount(r.stuffed & ((1u << nb) - 1u));
    return (r.pos - (uint64_t)nb - (uint64_t)pairs) * 8 + (uint64_t)(nb * 8 - r.nbits);
}

DVO_HD inline void open_reader(SplitReader& r, const uint8_t* data, uint32_t len, uint64_t bitpos) {
    r = SplitReader{data, len, bitpos >> 3, 0, 0, 0, false, 0};
    refill(r);
    r.nbits -= (int)(bitpos & 7);
}

DVO_HD inline int blocks_per_mcu(const FramePlan& P) { return P.ncomp == 1 ? 1 : P.hs * P.vs + 2; }
DVO_HD inline int slot_component(const FramePlan& P, int slot) {
    const int ny = P.ncomp == 1 ? 1 : P.hs * P.vs;
    return slot < ny ? 0 : (slot - ny + 1 > 2 ? 2 : slot - ny + 1);
}

// number of subsequences, the end (in bits) of subsequence g, and the guessed entry of g >= 1
DVO_HD inline uint32_t split_count(uint32_t len, uint32_t S) { return (uint32_t)(((uint64_t)len + S - 1) / S); }
DVO_HD inline uint64_t split_end(uint32_t len, uint32_t S, uint32_t g) {
    const uint64_t e = ((uint64_t)g + 1) * S;
    return (e < len ? e : (uint64_t)len) * 8;
}
DVO_HD inline uint64_t split_guess(const uint8_t* data, uint32_t len, uint32_t S, uint32_t g) {
    uint64_t s = (uint64_t)g * S;  // 1 <= s < len
    if (data[s - 1] == 0xFF && data[s] == 0) s += 1;  // the 00 of a pair is not data
    return pack_state(s * 8, 0, 0);
}

struct LaneResult {
    uint64_t exit;       // the state the next lane enters with
    uint32_t blocks;     // blocks completed
    uint32_t dc[3];      // per component, the wrapping sum of the DC differences
    int32_t err_block;   // lane-local index of the block the first error was met in, -1: none
};

struct CoefSink {
    int16_t* coef;   // the frame's coefficients
    uint64_t first;  // ordinal, within the segment, of the block the lane enters in
    uint64_t total;  // blocks of the segment: nmcu x blocks per MCU
    int32_t mcu0;
    uint32_t pred[3];  // DC predictors at the lane's entry
};

// block `ordinal` of the segment in the frame's coefficients; null outside the segment or the frame
DVO_HD inline int16_t* sink_block(const FramePlan& P, const CoefSink& K, uint64_t ordinal) {
    if (ordinal >= K.total) return nullptr;
    const uint32_t bpm = (uint32_t)blocks_per_mcu(P), o = (uint32_t)ordinal;  // total < 2^32: mcu0 + nmcu <= mcux mcuy
    const int m = K.mcu0 + (int)(o / bpm), slot = (int)(o % bpm);
    const int c = slot_component(P, slot);
    const int hc = c == 0 ? P.hs : 1, vc = c == 0 ? P.vs : 1;
    const int by = c == 0 ? slot / hc : 0, bx = c == 0 ? slot - by * hc : 0;
    const int my = m / P.mcux, mx = m - my * P.mcux;
    const int64_t blk = P.blk0[c] + (int64_t)(my * vc + by) * P.bw[c] + (mx * hc + bx);
    if (blk < 0 || blk >= P.nblk) return nullptr;
    return K.coef + blk * 64;
}

// Symbols from `entry` until the next one would start at or past end_bit.  Reads data[0, len)
// only; with a sink stores the coefficients of blocks inside the segment, without one nothing.
DVO_HD inline LaneResult run(const FramePlan& P, const uint8_t* data, uint32_t len, uint64_t entry, uint64_t end_bit,
                             const CoefSink* sink) {
    LaneResult R{entry, 0, {0, 0, 0}, -1};
    if (entry == kDead || state_pos(entry) >= end_bit) return R;
    const int bpm = blocks_per_mcu(P);
    int slot = state_slot(entry), k = state_k(entry);
    if (slot >= bpm) slot = 0;  // (no state made here has one)
    int c = slot_component(P, slot);
    SplitReader r;
    open_reader(r, data, len, state_pos(entry));
    int16_t* o = sink ? sink_block(P, *sink, sink->first) : nullptr;
    while (position(r) < end_bit) {  // one symbol per turn, each of at least one bit
        bool done = false, bad = false;
        if (k == 0) {
            const int s = huff_decode(r, P.dc[c]);
            if (s < 0) r.nbits -= 1;  // a code that matches nothing consumes nothing: every turn takes a bit
            if (s < 0 || s > 15) {
                bad = true;
            } else {
                R.dc[c] += (uint32_t)receive_extend(r, s);
                if (o) o[0] = (int16_t)(int)(sink->pred[c] + R.dc[c]);
                k = 1;
            }
        } else {
            const int rs = huff_decode(r, P.ac[c]);
            const int s = rs & 15;
            if (rs < 0) {
                r.nbits -= 1;
                bad = true;
            } else if (s == 0) {
                if ((rs >> 4) != 15) done = true;
                k += 16;
            } else {
                k += rs >> 4;
                if (k > 63) {
                    bad = true;
                } else {
                    const int v = receive_extend(r, s);
                    if (o) o[zigzag(k)] = (int16_t)v;
                    k += 1;
                }
            }
            if (k >= 64) done = true;
        }
        if (r.nbits < 8 * r.fake) {  // the symbol used bits that the file does not have: nothing to decode from here on
            if (R.err_block < 0) R.err_block = (int32_t)R.blocks;
            R.exit = kDead;
            return R;
        }
        if (bad) {
            // A lane that started from a guess meets errors all the time and has to go on to fall
            // into step; one that started from the true state has found the segment's first error,
            // and nothing after that counts.  Either way: note the first and take the block as ended.
            if (R.err_block < 0) R.err_block = (int32_t)R.blocks;
            done = true;
        }
        if (done) {
            R.blocks += 1;
            k = 0;
            slot = slot + 1 == bpm ? 0 : slot + 1;
            c = slot_component(P, slot);
            if (sink) o = sink_block(P, *sink, sink->first + R.blocks);
        }
    }
    R.exit = pack_state(position(r), slot, k);
    return R;
}

// The host model: decode_segment by the schedule above, the lanes taken one after the other.
// *passes (if not null) gets the synchronisation passes run, summed over the chunks.
inline int decode_segment_split(const FramePlan& P, const uint8_t* data, uint32_t len, int mcu0, int nmcu, int16_t* coef,
                                uint32_t S, int* passes, int lanes = kSplitLanes) {
    if (passes) *passes = 0;
    const uint32_t n = split_count(len, S);
    const int64_t frame_mcus = (int64_t)P.mcux * P.mcuy;
    if (n < 2 || mcu0 < 0 || nmcu < 0 || (int64_t)mcu0 + nmcu > frame_mcus)
        return decode_segment(P, data, len, mcu0, nmcu, coef);
    const uint64_t total = (uint64_t)nmcu * (uint64_t)blocks_per_mcu(P);
    uint64_t c_state = pack_state(0, 0, 0), c_ord = 0;
    uint32_t c_dc[3] = {0, 0, 0};
    std::vector<uint64_t> entry, exits;
    std::vector<LaneResult> res;
    bool bad = false;
    int np = 0;
    for (uint32_t c0 = 0; c0 < n && !bad; c0 += (uint32_t)lanes) {
        const int nl = (int)(n - c0 < (uint32_t)lanes ? n - c0 : (uint32_t)lanes);
        entry.assign((size_t)nl, kDead);
        exits.assign((size_t)nl, kDead);
        res.assign((size_t)nl, LaneResult{});
        for (int i = 0; i < nl; ++i) {
            entry[(size_t)i] = i == 0 ? c_state : split_guess(data, len, S, c0 + (uint32_t)i);
            res[(size_t)i] = run(P, data, len, entry[(size_t)i], split_end(len, S, c0 + (uint32_t)i), nullptr);
        }
        for (int pass = 1; pass < nl; ++pass) {
            for (int i = 0; i < nl; ++i) exits[(size_t)i] = res[(size_t)i].exit;  // reads are of the pass before
            bool any = false;
            for (int i = 1; i < nl; ++i) {
                if (exits[(size_t)i - 1] == entry[(size_t)i]) continue;
                entry[(size_t)i] = exits[(size_t)i - 1];
                res[(size_t)i] = run(P, data, len, entry[(size_t)i], split_end(len, S, c0 + (uint32_t)i), nullptr);
                if (res[(size_t)i].exit != exits[(size_t)i]) any = true;
            }
            ++np;
            if (!any) break;
        }
        std::vector<CoefSink> sinks((size_t)nl);
        uint64_t ord = c_ord;
        uint32_t dc[3] = {c_dc[0], c_dc[1], c_dc[2]};
        for (int i = 0; i < nl; ++i) {
            const LaneResult& r = res[(size_t)i];
            sinks[(size_t)i] = CoefSink{coef, ord, total, mcu0, {dc[0], dc[1], dc[2]}};
            if (r.err_block >= 0 && ord + (uint64_t)r.err_block < total) bad = true;
            ord += r.blocks;
            for (int c = 0; c < 3; ++c) dc[c] += r.dc[c];
        }
        if (bad) break;
        for (int i = 0; i < nl; ++i)
            run(P, data, len, entry[(size_t)i], split_end(len, S, c0 + (uint32_t)i), &sinks[(size_t)i]);
        c_state = res[(size_t)nl - 1].exit;
        c_ord = ord;
        for (int c = 0; c < 3; ++c) c_dc[c] = dc[c];
    }
    if (passes) *passes = np;
    if (bad || c_ord < total) return decode_segment(P, data, len, mcu0, nmcu, coef);
    return 0;
}

}  // namespace jpeg
}  // namespace dvo
