// JPEG markers -> a frame plan and the list of its entropy-coded segments (host only).
// Supported: SOF0, 8-bit, Huffman, one interleaved scan of 1 component, or of 3 components
// with Cb = Cr = 1x1 and Y 1x1, 2x1 or 2x2; 8-bit DQT, any DHT, any DRI.  Everything else that is a
// legal JPEG is kUnsupported, a malformed header kCorrupt.  No byte outside buf[0, len) is read.
#include <cstring>

#include "jpeg.h"
#include "jpeg_entropy.h"

namespace dvo {
namespace jpeg {
namespace {

int fail(Parsed* out, int code, const char* why) {
    out->why = why;
    return code;
}

unsigned be16(const uint8_t* p) { return (unsigned)p[0] << 8 | p[1]; }

// counts[1..16] codes per length and their values -> the derived table; false if the counts do
// not describe a prefix code
bool derive(const uint8_t* counts, const uint8_t* vals, int nvals, HuffTable* T) {
    std::memset(T, 0, sizeof(*T));
    std::memcpy(T->vals, vals, (size_t)nvals);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l];
        T->valptr[l] = p - code;
        T->maxcode[l] = -1;
        if (cnt) {
            if (code + cnt > (1 << l)) return false;
            T->maxcode[l] = code + cnt - 1;
            if (l <= 8)
                for (int c = code; c < code + cnt; ++c)
                    for (int i = 0; i < (1 << (8 - l)); ++i)
                        T->look[(c << (8 - l)) + i] = (uint16_t)(l << 8 | vals[p + (c - code)]);
        }
        p += cnt;
        code = (code + cnt) << 1;
    }
    T->maxcode[0] = -1;
    return true;
}

}  // namespace

int parse(const uint8_t* b, size_t n, Parsed* out) {
    *out = Parsed{};
    std::memset(&out->plan, 0, sizeof(out->plan));
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return fail(out, kCorrupt, "no SOI marker");
    if (n > 0x7FFFFFFFu) return fail(out, kCorrupt, "file of 2 GiB or more");
    uint16_t qt[4][64];
    bool qt_def[4] = {false, false, false, false};
    static_assert(sizeof(HuffTable) < 2048, "tables live on the stack here");
    HuffTable ht[2][4];
    bool ht_def[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool sof = false;
    int nc = 0, W = 0, H = 0, restart = 0, adobe = -1;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0}, ctd[3] = {0, 0, 0},
        cta[3] = {0, 0, 0};
    size_t pos = 2, scan_begin = 0;
    for (;;) {
        if (pos >= n) return fail(out, kCorrupt, "no SOS marker");
        if (b[pos] != 0xFF) return fail(out, kCorrupt, "marker expected");
        while (pos < n && b[pos] == 0xFF) ++pos;
        if (pos >= n) return fail(out, kCorrupt, "no SOS marker");
        const int m = b[pos++];
        if (m == 0) return fail(out, kCorrupt, "marker expected");
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return fail(out, kCorrupt, "EOI before SOS");
        if (pos + 2 > n) return fail(out, kCorrupt, "marker segment cut short");
        const size_t L = be16(b + pos);
        if (L < 2 || pos + L > n) return fail(out, kCorrupt, "marker segment cut short");
        const uint8_t* s = b + pos + 2;
        size_t sl = L - 2;
        pos += L;
        if (m == 0xC0) {
            if (sof) return fail(out, kCorrupt, "two SOF markers");
            if (sl < 6) return fail(out, kCorrupt, "SOF cut short");
            const int prec = s[0];
            H = (int)be16(s + 1);
            W = (int)be16(s + 3);
            nc = s[5];
            if (prec != 8) return fail(out, kUnsupported, "sample precision other than 8 bits");
            if (nc == 4) return fail(out, kUnsupported, "4 components");
            if (nc != 1 && nc != 3) return fail(out, kUnsupported, "component count other than 1 or 3");
            if (sl != (size_t)(6 + 3 * nc)) return fail(out, kCorrupt, "SOF length");
            if (W == 0) return fail(out, kCorrupt, "width 0");
            if (H == 0) return fail(out, kUnsupported, "height 0 (DNL)");
            for (int i = 0; i < nc; ++i) {
                cid[i] = s[6 + 3 * i];
                ch[i] = s[7 + 3 * i] >> 4;
                cv[i] = s[7 + 3 * i] & 15;
                ctq[i] = s[8 + 3 * i];
                if (ch[i] < 1 || ch[i] > 4 || cv[i] < 1 || cv[i] > 4 || ctq[i] > 3)
                    return fail(out, kCorrupt, "SOF component");
            }
            sof = true;
        } else if (m == 0xC4) {
            while (sl > 0) {
                if (sl < 17) return fail(out, kCorrupt, "DHT cut short");
                const int tc = s[0] >> 4, th = s[0] & 15;
                if (tc > 1 || th > 3) return fail(out, kCorrupt, "DHT table id");
                uint8_t counts[17] = {0};
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += (counts[l] = s[l]);
                if (total > 256 || sl < (size_t)(17 + total)) return fail(out, kCorrupt, "DHT cut short");
                if (!derive(counts, s + 17, total, &ht[tc][th])) return fail(out, kCorrupt, "DHT is no prefix code");
                ht_def[tc][th] = true;
                s += 17 + total;
                sl -= (size_t)(17 + total);
            }
        } else if (m == 0xDB) {
            while (sl > 0) {
                const int pq = s[0] >> 4, tq = s[0] & 15;
                if (tq > 3 || pq > 1) return fail(out, kCorrupt, "DQT table id");
                if (pq == 1) return fail(out, kUnsupported, "16-bit quantisation table");
                if (sl < 65) return fail(out, kCorrupt, "DQT cut short");
                for (int k = 0; k < 64; ++k) qt[tq][zigzag(k)] = s[1 + k];
                qt_def[tq] = true;
                s += 65;
                sl -= 65;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return fail(out, kCorrupt, "DRI length");
            restart = (int)be16(s);
        } else if (m == 0xEE) {
            if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) adobe = s[11];
        } else if (m == 0xC2) {
            return fail(out, kUnsupported, "progressive");
        } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
            return fail(out, kUnsupported, "arithmetic coding");
        } else if (m >= 0xC1 && m <= 0xC8) {
            return fail(out, kUnsupported, "SOF other than baseline");
        } else if (m == 0xDA) {
            if (!sof) return fail(out, kCorrupt, "SOS before SOF");
            if (sl < 1) return fail(out, kCorrupt, "SOS cut short");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != (size_t)(1 + 2 * ns + 3)) return fail(out, kCorrupt, "SOS length");
            if (ns != nc) return fail(out, kUnsupported, "more than one scan");
            for (int i = 0; i < nc; ++i) {
                if (s[1 + 2 * i] != cid[i]) return fail(out, kUnsupported, "scan components out of order");
                ctd[i] = s[2 + 2 * i] >> 4;
                cta[i] = s[2 + 2 * i] & 15;
                if (ctd[i] > 3 || cta[i] > 3 || !ht_def[0][ctd[i]] || !ht_def[1][cta[i]])
                    return fail(out, kCorrupt, "scan uses an undefined Huffman table");
            }
            const uint8_t* t = s + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return fail(out, kCorrupt, "spectral selection in a baseline scan");
            scan_begin = pos;
            break;
        }
        // every other marker segment is skipped
    }
    FramePlan& P = out->plan;
    if (nc == 3) {
        if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') return fail(out, kUnsupported, "RGB components");
        if (adobe == 0) return fail(out, kUnsupported, "Adobe transform 0 (RGB)");
        const bool y_ok = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
        if (!y_ok || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1)
            return fail(out, kUnsupported, "sampling other than 4:4:4, 4:2:2, 4:2:0");
        P.hs = ch[0];
        P.vs = cv[0];
    } else {
        P.hs = P.vs = 1;  // a one-component scan is not interleaved: its MCU is one block
    }
    P.w = W;
    P.h = H;
    P.ncomp = nc;
    P.restart = restart;
    P.mcux = (W + 8 * P.hs - 1) / (8 * P.hs);
    P.mcuy = (H + 8 * P.vs - 1) / (8 * P.vs);
    int blk = 0;
    for (int c = 0; c < nc; ++c) {
        if (!qt_def[ctq[c]]) return fail(out, kCorrupt, "component uses an undefined quantisation table");
        std::memcpy(P.qt[c], qt[ctq[c]], sizeof(P.qt[c]));
        P.dc[c] = ht[0][ctd[c]];
        P.ac[c] = ht[1][cta[c]];
        P.bw[c] = P.mcux * (c == 0 ? P.hs : 1);
        P.bh[c] = P.mcuy * (c == 0 ? P.vs : 1);
        P.blk0[c] = blk;
        blk += P.bw[c] * P.bh[c];
    }
    P.nblk = blk;

    // the scan: up to the first marker that is neither a stuffed FF 00 nor RSTn, split at RSTn
    const int total = P.mcux * P.mcuy;
    const int expected = restart ? (total + restart - 1) / restart : 1;
    int found = 0;
    size_t i = scan_begin, seg0 = scan_begin, scan_end = n;
    auto close = [&](size_t end) {
        if (found < expected) {
            const int m0 = restart ? found * restart : 0;
            const int nm = restart ? (total - m0 < restart ? total - m0 : restart) : total;
            out->segs.push_back(Segment{0, (uint32_t)seg0, (uint32_t)(end - seg0), m0, nm});
        }
        ++found;
    };
    int trailing = -1;
    while (i < n) {
        const uint8_t* f = static_cast<const uint8_t*>(std::memchr(b + i, 0xFF, n - i));
        if (!f) break;
        i = (size_t)(f - b);
        if (i + 1 >= n) break;  // a last FF belongs to the segment; the bit reader stops at it
        const int x = b[i + 1];
        if (x == 0) {
            i += 2;
        } else if (x == 0xFF) {
            i += 1;
        } else if (x >= 0xD0 && x <= 0xD7) {
            close(i);
            i += 2;
            seg0 = i;
        } else {
            scan_end = i;
            trailing = x;
            break;
        }
    }
    close(scan_end);
    if (trailing == 0xDA || trailing == 0xC4 || trailing == 0xDB || trailing == 0xDD) {
        out->segs.clear();
        return fail(out, kUnsupported, "more than one scan");
    }
    out->scan_begin = scan_begin;
    out->scan_end = scan_end;
    if (found != expected) {
        out->scan_status = kCorrupt;
        out->why = "restart markers missing or in excess";
    }
    return kOk;
}

}  // namespace jpeg
}  // namespace dvo
