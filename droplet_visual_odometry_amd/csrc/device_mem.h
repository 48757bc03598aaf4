// Host-side ownership of the library's device memory (api.cpp): DeviceAllocs frees what it
// allocated, PairSets owns a stream's per-pair arrays and the scratches of its pair outputs
// (pair_outputs.h) and describes them once.  Host code only.
#pragma once

#include <cstring>
#include <utility>
#include <vector>

#include "dvo_internal.h"

namespace dvo {

// Device allocations that are freed together.  alloc() asks hipMalloc for exactly the bytes it
// is given: padding is the caller's decision.
class DeviceAllocs {
  public:
    DeviceAllocs() = default;
    DeviceAllocs(DeviceAllocs&& o) noexcept : ptrs_(std::move(o.ptrs_)) { o.ptrs_.clear(); }  // so: no copies
    DeviceAllocs& operator=(DeviceAllocs&& o) noexcept {
        if (this != &o) {
            release();
            ptrs_ = std::move(o.ptrs_);
            o.ptrs_.clear();
        }
        return *this;
    }
    ~DeviceAllocs() { release(); }

    template <class T>
    hipError_t alloc(T** p, size_t bytes) {
        ptrs_.reserve(ptrs_.size() + 1);  // so that nothing can throw between hipMalloc and the record
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        ptrs_.push_back(q);
        *p = static_cast<T*>(q);
        return hipSuccess;
    }
    void release() {
        for (void* q : ptrs_) (void)hipFree(q);
        ptrs_.clear();
    }
    bool empty() const { return ptrs_.empty(); }

  private:
    std::vector<void*> ptrs_;
};

// Pinned host allocations (hipHostMalloc) that are freed together.
class PinnedAllocs {
  public:
    PinnedAllocs() = default;
    PinnedAllocs(const PinnedAllocs&) = delete;
    PinnedAllocs& operator=(const PinnedAllocs&) = delete;
    ~PinnedAllocs() { release(); }

    template <class T>
    hipError_t alloc(T** p, size_t bytes) {
        ptrs_.reserve(ptrs_.size() + 1);
        void* q = nullptr;
        const hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        ptrs_.push_back(q);
        *p = static_cast<T*>(q);
        return hipSuccess;
    }
    void release() {
        for (void* q : ptrs_) (void)hipHostFree(q);
        ptrs_.clear();
    }

  private:
    std::vector<void*> ptrs_;
};

// The per-pair arrays of a stream's pair sets: of all sets (pairs [0, nsets F)), or one set's view.
// g's configuration scalars and its round-local fprec / dk_ctl / dk_list belong to the stream and
// are the same in every view; g.pts_f and g.m_arr alias pts and nmatch.
struct PairArrays {
    GeomArgs g{};
    float* pts = nullptr;       // [pairs][kp_cap][4] (x1, y1, x2, y2) KeyPoint_convert pixel coords
    int32_t* nmatch = nullptr;  // [pairs]
    PairHeader* hdr = nullptr;  // [pairs]
};

// The per-pair geometry, one copy per pair set.  A stream starts with one set: the drained calls
// (dvo_stream_process, _process_pairs, _pair) run a batch's rounds back to back in it.  The first
// dvo_stream_submit / _submit_pairs grows it to kRansacRounds sets (the pipeline depth); no set is
// occupied then, since every drained call retires what it started.
// At 1280x720, N 2000, maxIters 1000 a set costs about 0.9 MB per pair (models 720 KB of it).
struct PairSets {
    PairArrays all;  // null pointers while nsets == 0
    int nsets = 0;   // sets allocated (0: none)
    // The stream's shape, stated once at its creation (shape()) and fixed for life: F pairs per set
    // of cap points and hc hypotheses each; the sets its track scratch covers (the most the stream
    // will ever hold) and whether a set keeps its own copy of the match indices there.
    int F = 0, cap = 0;
    size_t hc = 0;
    int tr_sets = 0;
    bool own_idx = false;
    hipStream_t stream = nullptr;  // the stream whose kernels use the arrays (ensure waits for it)
    DeviceAllocs mem;

    void shape(int F_, int cap_, size_t hc_, int track_sets, bool own_idx_) {
        F = F_, cap = cap_, hc = hc_, tr_sets = track_sets, own_idx = own_idx_;
    }
    // A set's slots in the scratches below: its pairs (one at least) of cap points.
    size_t scratch_pairs() const { return (size_t)(F > 0 ? F : 1); }
    size_t set_slots() const { return scratch_pairs() * cap; }

    // The one description of the arrays: f(pointer, elements per pair, whole-launch) per array, in
    // allocation order.  A whole-launch array has sets F + 1 elements and is not offset in a view.
    template <class Fn>
    static void rows(PairArrays& a, size_t cap, size_t hc, Fn&& f) {
        GeomArgs& g = a.g;
        f(a.nmatch, 1, false);
        f(a.pts, cap * 4, false);
        f(g.npts, cap * 4, false);
        f(g.models, hc * 90, false);
        f(g.nmod, hc, false);
        f(g.cnt, hc * 10, false);
        f(g.subsets, hc * 5, false);
        f(g.rs, 1, false);
        f(a.hdr, 1, false);
        f(g.dk_off, 1, true);
        f(g.a_off, 1, true);
        f(g.s_off, 1, true);
        f(g.E, 90, false);
        f(g.info, 4, false);
        f(g.Rt, 12, false);
        f(g.good, 1, false);
        f(g.pose_P, 72, false);
        f(g.pose_cnt, 5, false);
    }

    void release() {
        mem.release();
        rows(all, 0, 0, [](auto*& p, size_t, bool) { p = nullptr; });
        all.g.pts_f = nullptr;
        all.g.m_arr = nullptr;
        nsets = 0;
    }

    // At least `want` sets of the stream's shape.  Growing waits for the stream, frees the old
    // sets, then allocates the new ones (never both at once: batches are sized to fill the card),
    // each array n * sizeof(T) + 256 bytes.  On failure no set is left: nsets == 0 and every
    // pointer is null, and a later ensure() starts afresh.
    hipError_t ensure(int want) {
        if (nsets >= want) return hipSuccess;
        hipError_t e = hipSuccess;
        if (!mem.empty() && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        release();
        const size_t SF = (size_t)want * F;
        rows(all, cap, hc, [&](auto*& p, size_t per_pair, bool whole) {
            if (e == hipSuccess) e = mem.alloc(&p, (whole ? SF + 1 : SF * per_pair) * sizeof(*p) + 256);
        });
        if (e != hipSuccess) {
            release();
            return e;
        }
        all.g.pts_f = all.pts;
        all.g.m_arr = all.nmatch;
        nsets = want;
        return hipSuccess;
    }

    // The landmark kernels' scratch (launch_landmarks): empty until the stream's first binding
    // (PairOutputs::set_landmarks), then one copy for a set's pairs whatever the number of sets,
    // since it is live only between the two launches of one set's retire.  It does not depend on
    // the sets' arrays: ensure() and release() leave it alone, and because the shape is the
    // stream's for life it is allocated once and never regrown (nothing is freed, no pointer a
    // queued kernel holds goes stale).  A failure leaves it empty.
    LandmarkScratch lm;
    DeviceAllocs lm_mem;
    hipError_t ensure_landmarks() {
        if (lm.tmp) return hipSuccess;
        const size_t n = scratch_pairs() * landmark_tiles(cap);
        DeviceAllocs fresh;
        LandmarkScratch l;
        hipError_t e = fresh.alloc(&l.tmp, n * kLandmarkTile * sizeof(LandmarkTmp) + 256);
        if (e == hipSuccess) e = fresh.alloc(&l.tcnt, n * sizeof(int32_t) + 256);
        if (e != hipSuccess) return e;
        lm_mem = std::move(fresh);
        lm = l;
        return hipSuccess;
    }

    // The track kernels' scratch (launch_tracks): empty until the stream's first tracks binding
    // (PairOutputs::set_tracks), then tr_sets copies of a set's slots: like the landmark scratch it
    // is allocated once, whatever ensure() does later, and never regrown.  With own_idx, iq and it:
    // the ORB stream's per-set copy of its match indices.
    TrackScratch tr;
    DeviceAllocs tr_mem;
    hipError_t ensure_tracks() {
        if (tr.table) return hipSuccess;
        const size_t P = tr_sets * scratch_pairs(), n = tr_sets * set_slots();
        DeviceAllocs fresh;
        TrackScratch t;
        hipError_t e = fresh.alloc(&t.table, n * sizeof(int32_t) + 256);
        if (e == hipSuccess) e = fresh.alloc(&t.ratio, n * sizeof(double) + 256);
        if (e == hipSuccess) e = fresh.alloc(&t.lcnt, P * landmark_tiles(cap) * sizeof(int32_t) + 256);
        if (e == hipSuccess && own_idx) e = fresh.alloc(&t.iq, n * sizeof(int32_t) + 256);
        if (e == hipSuccess && own_idx) e = fresh.alloc(&t.it, n * sizeof(int32_t) + 256);
        if (e != hipSuccess) return e;
        tr_mem = std::move(fresh);
        tr = t;
        return hipSuccess;
    }
    // The pose kernel's correspondences (PairOutputs::set_track_poses): 40 B per slot beside the
    // ratios.  Allocated by the first pose binding (after the track scratch: a pose binding needs a
    // pending tracks binding) and never regrown.
    DeviceAllocs tp_mem;
    hipError_t ensure_track_poses() {
        if (tr.corr) return hipSuccess;
        if (!tr.table) return hipErrorInvalidValue;
        DeviceAllocs fresh;
        TrackCorr* c = nullptr;
        const hipError_t e = fresh.alloc(&c, tr_sets * set_slots() * sizeof(TrackCorr) + 256);
        if (e != hipSuccess) return e;
        tp_mem = std::move(fresh);
        tr.corr = c;
        return hipSuccess;
    }
    // The full links and the id kernel's two rank buffers (PairOutputs::set_track_refine): 4 B and
    // 16 B per slot.  Allocated by the first refine binding (after the track scratch: it needs a
    // pending tracks binding) and never regrown.
    DeviceAllocs rf_mem;
    hipError_t ensure_track_refine() {
        if (tr.flink) return hipSuccess;
        if (!tr.table) return hipErrorInvalidValue;
        const size_t n = tr_sets * set_slots();
        DeviceAllocs fresh;
        int32_t* l = nullptr;
        TrackRank* r = nullptr;
        hipError_t e = fresh.alloc(&l, n * sizeof(int32_t) + 256);
        if (e == hipSuccess) e = fresh.alloc(&r, 2 * n * sizeof(TrackRank) + 256);
        if (e != hipSuccess) return e;
        rf_mem = std::move(fresh);
        tr.flink = l;
        tr.rank = r;
        return hipSuccess;
    }
    // The bundle kernel's points and full links of its own (PairOutputs::set_track_bundle): 32 B and
    // 4 B per slot, one allocation, the links behind the points.  Allocated by the first bundle
    // binding (after the track scratch: it needs a pending tracks binding) and never regrown.  The
    // links are used where no refine binding has brought its own.
    DeviceAllocs bd_mem;
    hipError_t ensure_track_bundle() {
        if (tr.bx) return hipSuccess;
        if (!tr.table) return hipErrorInvalidValue;
        const size_t n = tr_sets * set_slots();
        DeviceAllocs fresh;
        BundlePoint* b = nullptr;
        const hipError_t e = fresh.alloc(&b, n * (sizeof(BundlePoint) + sizeof(int32_t)) + 256);
        if (e != hipSuccess) return e;
        bd_mem = std::move(fresh);
        tr.bx = b;
        tr.blink = reinterpret_cast<int32_t*>(b + n);
        return hipSuccess;
    }
    // The PnP kernels' correspondences and their per-tile counts (PairOutputs::set_track_pnp): 48 B
    // per slot and 4 B per tile, one allocation, the counts behind the correspondences.  Allocated
    // by the first PnP binding (after the track scratch: it needs a pending tracks binding) and
    // never regrown.
    DeviceAllocs pn_mem;
    hipError_t ensure_track_pnp() {
        if (tr.pc) return hipSuccess;
        if (!tr.table) return hipErrorInvalidValue;
        const size_t n = tr_sets * set_slots(), tiles = tr_sets * scratch_pairs() * landmark_tiles(cap);
        DeviceAllocs fresh;
        PnpCorr* c = nullptr;
        const hipError_t e = fresh.alloc(&c, n * sizeof(PnpCorr) + tiles * sizeof(int32_t) + 256);
        if (e != hipSuccess) return e;
        pn_mem = std::move(fresh);
        tr.pc = c;
        tr.pc_cnt = reinterpret_cast<int32_t*>(c + n);
        return hipSuccess;
    }
    // Set k's part of every scratch there is, as the track kernels' arguments: all of a TrackArgs
    // but the records and the caller's side (PairOutputs::fill in pair_outputs.h).  Set k's slots
    // start k set_slots() into each array, its two rank buffers at rank + 2 k set_slots(), one
    // set's slots apart; an own-index scratch is the set's index source; the full links are the
    // refine scratch's where there is one, else the bundle scratch's own.
    TrackArgs track_args(int k) const {
        const size_t n = k * set_slots();
        TrackArgs a{};
        a.L = lm;
        a.tiles = landmark_tiles(cap);
        a.table = tr.table + n;
        a.kp_cap = cap;
        a.ratio = tr.ratio + n;
        a.pts_stride = cap;
        a.lcnt = tr.lcnt + k * scratch_pairs() * a.tiles;
        if (tr.iq) a.mq = tr.iq + n, a.mt = tr.it + n, a.idx_stride = cap, a.idx_step = 1;
        if (tr.corr) a.corr = tr.corr + n;
        if (tr.flink) a.flink = tr.flink + n, a.rank = tr.rank + 2 * n, a.rank_stride = (int64_t)set_slots();
        if (tr.bx) a.bd_x = tr.bx + n;
        if (tr.bx && !a.flink) a.flink = tr.blink + n;
        if (tr.pc) a.pnp_corr = tr.pc + n, a.pnp_cnt = tr.pc_cnt + k * scratch_pairs() * a.tiles;
        return a;
    }

    // Set k's view: pairs [k F, (k + 1) F) of every per-set array.
    PairArrays view(int k) const {
        PairArrays v = all;
        if (k > 0)
            rows(v, cap, hc, [&](auto*& p, size_t per_pair, bool whole) {
                if (!whole) p += (size_t)k * F * per_pair;
            });
        v.g.pts_f = v.pts;
        v.g.m_arr = v.nmatch;
        return v;
    }
};

// Grow-only buffers of a context, device (hipMalloc) or pinned host (hipHostMalloc) memory: slot k
// holds at least what the largest k-th request so far asked for (4096 bytes at least, 25 % spare
// when it grows).
class Slots {
  public:
    explicit Slots(bool pinned) : pinned_(pinned) {}
    Slots(const Slots&) = delete;
    Slots& operator=(const Slots&) = delete;
    ~Slots() { release(); }

    hipError_t get(size_t k, size_t bytes, void** out) {
        if (slots_.size() <= k) slots_.resize(k + 1);
        Slot& e = slots_[k];
        if (!e.p || e.cap < bytes) {  // an empty request still gets a buffer: null means failure
            hipError_t err = e.p ? free_(e.p) : hipSuccess;
            e = Slot{};
            if (err != hipSuccess) return err;
            const size_t nb = bytes < 4096 ? 4096 : bytes + bytes / 4;
            err = pinned_ ? hipHostMalloc(&e.p, nb, hipHostMallocDefault) : hipMalloc(&e.p, nb);
            if (err != hipSuccess) return err;
            e.cap = nb;
        }
        *out = e.p;
        return hipSuccess;
    }
    void release() {
        for (Slot& e : slots_)
            if (e.p) (void)free_(e.p);
        slots_.clear();
    }

  private:
    struct Slot {
        void* p = nullptr;
        size_t cap = 0;
    };
    hipError_t free_(void* p) const { return pinned_ ? hipHostFree(p) : hipFree(p); }
    const bool pinned_;
    std::vector<Slot> slots_;
};

struct CallSlots {
    Slots dev{false}, pin{true};
};

// The memory of one synchronous per-call entry point: its k-th device request is the context's
// k-th device slot, its k-th pinned request the k-th pinned slot.  Entry points share the slots
// because each synchronises before it returns, so a call must not keep these pointers across a
// call into another entry point that makes its own CallMem.  A request that fails returns null and
// error() keeps the first failure: take every buffer, then check once.
// Host traffic goes through the pinned buffers: inputs are packed there and sent with asynchronous
// copies on the call's stream, outputs come back the same way, and the caller synchronises once
// (a pageable hipMemcpy is a blocking staged copy each: ~10-20 us apiece).
class CallMem {
  public:
    CallMem(CallSlots& slots, hipStream_t s) : slots_(slots), s_(s) {}

    template <class T>
    T* dev(size_t n) { return static_cast<T*>(take(slots_.dev, ndev_, n * sizeof(T))); }
    uint8_t* host(size_t bytes) { return static_cast<uint8_t*>(take(slots_.pin, npin_, bytes)); }
    hipError_t error() const { return err_; }

    hipError_t send(void* dev, const uint8_t* h, size_t n) {  // host -> device of pinned bytes
        return n ? hipMemcpyAsync(dev, h, n, hipMemcpyHostToDevice, s_) : hipSuccess;
    }
    hipError_t put(void* dev, const void* src, size_t n) {
        uint8_t* h = host(n);
        if (!h) return err_;
        if (n) std::memcpy(h, src, n);
        return send(dev, h, n);
    }
    hipError_t get(const void* dev, size_t n, uint8_t** h) {  // device -> host, valid after synchronising
        if (!(*h = host(n))) return err_;
        return n ? hipMemcpyAsync(*h, dev, n, hipMemcpyDeviceToHost, s_) : hipSuccess;
    }

  private:
    void* take(Slots& sl, size_t& k, size_t bytes) {
        void* p = nullptr;
        const hipError_t e = sl.get(k++, bytes, &p);
        if (err_ == hipSuccess) err_ = e;
        return p;
    }
    CallSlots& slots_;
    hipStream_t s_;
    size_t ndev_ = 0, npin_ = 0;
    hipError_t err_ = hipSuccess;
};

}  // namespace dvo
