// Host check of the JPEG parser (csrc/jpeg_parse.cpp) and the Huffman decoder (csrc/jpeg_entropy.h,
// the text the entropy kernel compiles) under the address and undefined-behaviour sanitizers
// (tests/test_jpeg_entropy_host.py builds and runs it; no GPU).
//
//   jpeg_entropy_check CASES
//
// CASES: u32 count, then per case i32 parse status, i32 entropy status, i32 mutate, u32 length
// and the file's bytes.  Every file, every segment and every coefficient array lives in a heap
// block of exactly its size, so one byte read or written outside it stops the program.  A case
// must give its statuses; a case with `mutate` is also run cut at every length and with every
// byte changed in turn, where any status is right and only the bounds are checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../droplet_visual_odometry_amd/csrc/jpeg_parse.cpp"

using namespace dvo::jpeg;

namespace {

long g_runs = 0, g_decoded = 0;

struct Result {
    int parse, entropy;
};

// parse + decode of one file held in a block of exactly its size
Result run(const uint8_t* bytes, size_t n) {
    uint8_t* file = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    std::memcpy(file, bytes, n);
    Parsed P;
    Result r{parse(file, n, &P), kOk};
    ++g_runs;
    // a decoder is made for a largest frame: stay below 1024 x 1024 pixels here
    if (r.parse == kOk && P.plan.nblk <= 3 * 128 * 128) {
        const size_t elems = (size_t)P.plan.nblk * 64;
        int16_t* coef = static_cast<int16_t*>(std::calloc(elems, sizeof(int16_t)));
        r.entropy = P.scan_status;
        for (const Segment& sg : P.segs) {
            uint8_t* seg = static_cast<uint8_t*>(std::malloc(sg.length ? sg.length : 1));
            std::memcpy(seg, file + sg.offset, sg.length);
            if (decode_segment(P.plan, seg, sg.length, sg.mcu0, sg.nmcu, coef)) r.entropy = kCorrupt;
            std::free(seg);
        }
        std::free(coef);
        ++g_decoded;
    }
    std::free(file);
    return r;
}

uint32_t rd32(FILE* f) {
    uint32_t v = 0;
    if (std::fread(&v, 4, 1, f) != 1) {
        std::fprintf(stderr, "jpeg_entropy_check: case file cut short\n");
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
    int bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const int want_parse = (int)rd32(f), want_entropy = (int)rd32(f), mutate = (int)rd32(f);
        std::vector<uint8_t> b(rd32(f));
        if (!b.empty() && std::fread(b.data(), 1, b.size(), f) != b.size()) return 2;
        const Result r = run(b.data(), b.size());
        if (r.parse != want_parse || (r.parse == kOk && r.entropy != want_entropy)) {
            std::fprintf(stderr, "case %u: parse %d (want %d), entropy %d (want %d)\n", i, r.parse, want_parse,
                         r.entropy, want_entropy);
            ++bad;
        }
        if (!mutate) continue;
        for (size_t n = 0; n < b.size(); ++n) run(b.data(), n);
        for (size_t k = 0; k < b.size(); ++k) {
            std::vector<uint8_t> m = b;
            m[k] ^= (uint8_t)(1u << (k % 8));
            run(m.data(), m.size());
            m[k] = 0xFF;
            run(m.data(), m.size());
        }
    }
    std::fclose(f);
    if (bad) return 1;
    std::printf("ok %ld runs, %ld decoded\n", g_runs, g_decoded);
    return 0;
}
