// Host check of csrc/device_mem.h (tests/test_device_mem_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it; no GPU).  The HIP allocation calls the header uses
// are fake_hip.h's: a fake allocator that records sizes, can fail the n-th hipMalloc, and aborts
// when asked to free a pointer it does not hold.
#include "fake_hip.h"

#include "../droplet_visual_odometry_amd/csrc/device_mem.h"

using namespace dvo;

namespace {
constexpr int F = 3, CAP = 7;
constexpr size_t HC = 5;

// What a stream's pair sets must allocate (the sizes and their order are pinned),
// written out, not computed through PairSets::rows: bytes per pair of each array in allocation
// order (0: one of the three whole-launch offset arrays, 4 (sets F + 1) bytes), each + 256.
std::vector<size_t> expected_sizes(int sets) {
    const size_t per_pair[18] = {4,  16 * CAP, 32 * CAP, 720 * HC, 4 * HC, 40 * HC, 20 * HC, sizeof(RansacState),
                                 sizeof(PairHeader), 0, 0, 0, 720, 16, 96, 4, 576, 20};
    std::vector<size_t> v;
    for (size_t b : per_pair) v.push_back((b ? (size_t)sets * F * b : 4 * ((size_t)sets * F + 1)) + 256);
    return v;
}

// the 18 pointers of a PairArrays, in allocation order, as bytes
std::vector<const char*> pointers(const PairArrays& a) {
    const GeomArgs& g = a.g;
    const void* p[18] = {a.nmatch, a.pts, g.npts, g.models, g.nmod, g.cnt, g.subsets, g.rs, a.hdr,
                         g.dk_off, g.a_off, g.s_off, g.E, g.info, g.Rt, g.good, g.pose_P, g.pose_cnt};
    std::vector<const char*> v;
    for (const void* q : p) v.push_back(static_cast<const char*>(q));
    return v;
}

void check_sizes_and_views() {
    static_assert(sizeof(RansacState) == 48 && sizeof(PairHeader) == 16, "the size table below assumes these");
    PairSets ps;
    ps.shape(F, CAP, HC, 1, false);
    reset_log();
    CHECK(ps.ensure(1) == hipSuccess);
    CHECK(ps.nsets == 1 && g_mallocs == expected_sizes(1) && g_syncs == 0 && g_frees == 0);
    CHECK(ps.ensure(1) == hipSuccess && g_mallocs.size() == 18);  // enough already: no call
    reset_log();
    CHECK(ps.ensure(5) == hipSuccess);
    CHECK(ps.nsets == 5 && g_mallocs == expected_sizes(5));
    CHECK(g_syncs == 1 && g_frees == 18 && g_dev.size() == 18);  // waited, freed the old set first
    // bytes per pair of each per-set array (element size x elements per pair); 0: not offset
    const size_t stride[18] = {4,  16 * CAP, 32 * CAP, 720 * HC, 4 * HC, 40 * HC, 20 * HC, 48, 16,
                               0,  0,        0,        720,      16,     96,      4,       576, 20};
    const std::vector<const char*> base = pointers(ps.all);
    for (int i = 0; i < 18; ++i) CHECK(g_dev.count((void*)base[i]) == 1);
    for (int k = 0; k < 5; ++k) {
        const PairArrays v = ps.view(k);
        const std::vector<const char*> p = pointers(v);
        for (int i = 0; i < 18; ++i) CHECK(p[i] == base[i] + (size_t)k * F * stride[i]);
        CHECK(v.g.pts_f == v.pts && v.g.m_arr == v.nmatch);
    }
    ps.release();
    CHECK(g_dev.empty() && ps.nsets == 0);
}

void check_failed_grow() {
    for (int n = 0; n < 18; ++n) {
        PairSets ps;
        ps.shape(F, CAP, HC, 1, false);
        ps.all.g.fprec = reinterpret_cast<double*>(&ps);  // the stream's own members of g are not the sets'
        ps.all.g.hyp_cap = (int)HC;
        CHECK(ps.ensure(1) == hipSuccess);
        reset_log();
        g_fail_at = n;
        CHECK(ps.ensure(5) != hipSuccess);
        CHECK(ps.nsets == 0 && g_dev.empty() && (int)g_mallocs.size() == n + 1);
        for (const char* p : pointers(ps.all)) CHECK(p == nullptr);
        CHECK(ps.all.g.pts_f == nullptr && ps.all.g.m_arr == nullptr);
        CHECK(ps.all.g.fprec == reinterpret_cast<double*>(&ps) && ps.all.g.hyp_cap == (int)HC);
        reset_log();
        CHECK(ps.ensure(1) == hipSuccess);  // usable again: one set
        CHECK(ps.nsets == 1 && g_mallocs == expected_sizes(1) && g_dev.size() == 18);
    }
    CHECK(g_dev.empty());
}

void check_release() {
    reset_log();
    int *a = nullptr, *b = nullptr, *c = nullptr;
    {
        DeviceAllocs x;
        CHECK(x.alloc(&a, 40) == hipSuccess && x.alloc(&b, 0) == hipSuccess);
        CHECK(g_mallocs == (std::vector<size_t>{40, 0}));  // exactly the bytes asked for
        DeviceAllocs y(std::move(x));
        CHECK(x.empty() && g_dev.size() == 2);
        x.release();  // moved from: holds nothing
        CHECK(g_dev.size() == 2 && g_frees == 0);
        DeviceAllocs z;
        CHECK(z.alloc(&c, 8) == hipSuccess);
        z = std::move(y);  // frees z's own, takes y's
        CHECK(g_frees == 1 && g_dev.count(c) == 0 && g_dev.size() == 2 && y.empty());
        g_fail_at = (int)g_mallocs.size();
        CHECK(z.alloc(&c, 8) != hipSuccess);  // a failed call records nothing
        z.release();
        CHECK(g_frees == 3 && g_dev.empty());
        z.release();  // again: nothing left to free
        CHECK(z.alloc(&a, 16) == hipSuccess);
    }  // the destructors: z's one pointer once, x and y nothing (the fake aborts on a second free)
    CHECK(g_frees == 4 && g_dev.empty());
}

void check_ordinals() {
    reset_log();
    {
        CallSlots slots;
        void *a, *b, *c;
        {
            CallMem m(slots, nullptr);
            a = m.dev<double>(100);  // 800 bytes: the 4096 floor
            b = m.dev<uint8_t>(5000);
            c = m.dev<int32_t>(0);
            CHECK(a && b && c && m.error() == hipSuccess);
            CHECK(g_mallocs == (std::vector<size_t>{4096, 5000 + 5000 / 4, 4096}));
            uint8_t* h0 = m.host(10);
            uint8_t* h1 = m.host(6000);
            CHECK(h0 && h1 && g_pin.at(h0) == 4096 && g_pin.at(h1) == 7500);
        }
        {
            CallMem m(slots, nullptr);  // the next call: slots 0 and 1 again
            CHECK(m.dev<uint8_t>(4096) == a && m.dev<float>(1500) == b);  // both fit: nothing allocated
            CHECK(g_mallocs.size() == 3 && g_frees == 0);
            uint8_t* h0 = m.host(4096);
            CHECK(g_pin.size() == 2 && g_pin.at(h0) == 4096);
            const int src[3] = {1, 2, 3};
            int dst[3] = {0, 0, 0};
            uint8_t* back = nullptr;
            CHECK(m.put(dst, src, sizeof(src)) == hipSuccess && dst[2] == 3);  // pinned slot 1
            CHECK(m.get(dst, sizeof(dst), &back) == hipSuccess && std::memcmp(back, src, sizeof(src)) == 0);
            CHECK(g_pin.size() == 3);  // the third pinned request of a call is new
        }
        {
            CallMem m(slots, nullptr);
            void* a2 = m.dev<uint8_t>(4097);  // more than slot 0 holds: freed, then allocated with 25 % spare
            CHECK(a2 && g_frees == 1 && g_mallocs.size() == 4 && g_mallocs[3] == 4097 + 4097 / 4);
            CHECK(g_dev.count(b) == 1 && g_dev.count(c) == 1 && g_dev.size() == 3);
            g_fail_at = (int)g_mallocs.size();
            CHECK(m.dev<uint8_t>(1 << 20) == nullptr && m.error() == hipErrorOutOfMemory);  // slot 1 fails to grow
            CHECK(m.dev<uint8_t>(1) == c && m.error() == hipErrorOutOfMemory);  // the first failure is kept
        }
        {
            CallMem m(slots, nullptr);
            m.dev<uint8_t>(1);
            CHECK(m.dev<uint8_t>(1) != nullptr && m.error() == hipSuccess);  // the emptied slot 1 allocates again
        }
    }
    CHECK(g_dev.empty() && g_pin.empty());
}
}  // namespace

int main() {
    check_sizes_and_views();
    check_failed_grow();
    check_release();
    check_ordinals();
    std::puts("ok");
    return 0;
}
