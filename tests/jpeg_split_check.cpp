// Host check of the many-lane Huffman decoder (csrc/jpeg_split.h, the text the split entropy
// kernel compiles) against decode_segment under the address and undefined-behaviour sanitizers
// (tests/test_jpeg_split_host.py builds and runs it; no GPU).
//
//   jpeg_split_check CASES
//
// CASES: jpeg_entropy_check's format (u32 count, then per case i32 parse status, i32 entropy
// status, i32 mutate, u32 length and the file's bytes).  Every file, every segment and both
// coefficient arrays live in heap blocks of exactly their size.  Each file that parses is decoded
// segment by segment with decode_segment and with decode_segment_split at 16 and at 128 bytes per
// lane, and at 16 bytes in chunks of 3 lanes (the carried state); coefficients and status must be
// equal.  A case with `mutate` is also run cut at every length and with every byte changed in turn.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../droplet_visual_odometry_amd/csrc/jpeg_parse.cpp"
#include "../droplet_visual_odometry_amd/csrc/jpeg_split.h"

using namespace dvo::jpeg;

namespace {

long g_runs = 0, g_compared = 0, g_split = 0, g_corrupt = 0, g_bad = 0;
int g_max_passes = 0;

struct Config {
    uint32_t split_bytes;
    int lanes;
};
const Config kConfigs[] = {{16, kSplitLanes}, {128, kSplitLanes}, {16, 3}};

void run(const uint8_t* bytes, size_t n, const char* what, long at) {
    uint8_t* file = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    std::memcpy(file, bytes, n);
    Parsed P;
    ++g_runs;
    if (parse(file, n, &P) == kOk && P.plan.nblk <= 3 * 128 * 128) {
        const size_t elems = (size_t)P.plan.nblk * 64;
        int16_t* want = static_cast<int16_t*>(std::calloc(elems, sizeof(int16_t)));
        int want_status = 0;
        std::vector<uint8_t*> segs;
        for (const Segment& sg : P.segs) {
            uint8_t* seg = static_cast<uint8_t*>(std::malloc(sg.length ? sg.length : 1));
            std::memcpy(seg, file + sg.offset, sg.length);
            segs.push_back(seg);
            if (decode_segment(P.plan, seg, sg.length, sg.mcu0, sg.nmcu, want)) want_status = kCorrupt;
        }
        if (want_status) ++g_corrupt;
        for (const Config& cf : kConfigs) {
            int16_t* got = static_cast<int16_t*>(std::calloc(elems, sizeof(int16_t)));
            int got_status = 0;
            for (size_t i = 0; i < P.segs.size(); ++i) {
                const Segment& sg = P.segs[i];
                int passes = 0;
                if (decode_segment_split(P.plan, segs[i], sg.length, sg.mcu0, sg.nmcu, got, cf.split_bytes, &passes, cf.lanes))
                    got_status = kCorrupt;
                const uint32_t nsub = split_count(sg.length, cf.split_bytes);
                if (nsub >= 2) ++g_split;
                if (passes > (int)nsub) {
                    std::fprintf(stderr, "%s %ld: %d passes for %u subsequences\n", what, at, passes, nsub);
                    ++g_bad;
                }
                if (cf.lanes == kSplitLanes && passes > g_max_passes) g_max_passes = passes;
            }
            ++g_compared;
            if (got_status != want_status || std::memcmp(got, want, elems * sizeof(int16_t)) != 0) {
                if (g_bad < 20)
                    std::fprintf(stderr, "%s %ld: split %u x %d lanes: status %d (want %d), coefficients %s\n", what, at,
                                 cf.split_bytes, cf.lanes, got_status, want_status,
                                 std::memcmp(got, want, elems * sizeof(int16_t)) ? "differ" : "equal");
                ++g_bad;
            }
            std::free(got);
        }
        for (uint8_t* s : segs) std::free(s);
        std::free(want);
    }
    std::free(file);
}

uint32_t rd32(FILE* f) {
    uint32_t v = 0;
    if (std::fread(&v, 4, 1, f) != 1) {
        std::fprintf(stderr, "jpeg_split_check: case file cut short\n");
        std::exit(2);
    }
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    for (uint32_t i = 0; i < count; ++i) {
        rd32(f), rd32(f);
        const int mutate = (int)rd32(f);
        std::vector<uint8_t> b(rd32(f));
        if (!b.empty() && std::fread(b.data(), 1, b.size(), f) != b.size()) return 2;
        run(b.data(), b.size(), "case", (long)i);
        if (!mutate) continue;
        for (size_t n = 0; n < b.size(); ++n) run(b.data(), n, "cut", (long)n);
        for (size_t k = 0; k < b.size(); ++k) {
            std::vector<uint8_t> m = b;
            m[k] ^= (uint8_t)(1u << (k % 8));
            run(m.data(), m.size(), "bit", (long)k);
            m[k] = 0xFF;
            run(m.data(), m.size(), "ff", (long)k);
        }
    }
    std::fclose(f);
    if (g_bad) return 1;
    std::printf("ok %ld runs, %ld compared, %ld split, %ld corrupt, max passes %d\n", g_runs, g_compared, g_split,
                g_corrupt, g_max_passes);
    return 0;
}
