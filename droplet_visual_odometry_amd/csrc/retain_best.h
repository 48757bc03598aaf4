// KeyPointsFilter::retainBest on one workgroup: retain_best_block and the block primitives it is
// built from, shared by the ORB selection kernels (orb.hip) and the SIFT retain stage (sift.hip).
// An accessor A names the list: val(i) the response, swap(i, j), and for the single-lane fallbacks
// Elem / get / put / ev.  Lpos and Rasc take n + 1 positions each, lds 64 ints.
#pragma once
#include <climits>

#include "dvo_internal.h"

namespace dvo {
namespace {

__device__ __forceinline__ void block_excl_scan2(int fa, int fb, int& pa, int& pb, int& ta, int& tb, int* lds) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned long long ma = __ballot(fa), mb = __ballot(fb);
    unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) {
        lds[wid] = __popcll(ma);
        lds[32 + wid] = __popcll(mb);
    }
    __syncthreads();
    int oa = 0, ob = 0, sa = 0, sb = 0;
    for (int w = 0; w < nw; ++w) {
        int ca = lds[w], cb = lds[32 + w];
        if (w < wid) {
            oa += ca;
            ob += cb;
        }
        sa += ca;
        sb += cb;
    }
    __syncthreads();
    pa = oa + __popcll(ma & lt);
    pb = ob + __popcll(mb & lt);
    ta = sa;
    tb = sb;
}

__device__ __forceinline__ int block_sum(int v, int* lds) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) lds[wid] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < nw; ++w) s += lds[w];
    __syncthreads();
    return s;
}

template <class A, class V>
__device__ int partition_step(const A& a, int first, int last, V p, int32_t* Lpos, int32_t* Rasc, int* lds) {
    int nL = 0, nR = 0;
    for (int base = first; base < last; base += blockDim.x) {
        const int i = base + threadIdx.x;
        const bool in = i < last;
        V v = in ? a.val(i) : p;
        int fl = in && i >= first + 1 && !(v > p);
        int fr = in && !(p > v);
        int pa, pb, ta, tb;
        block_excl_scan2(fl, fr, pa, pb, ta, tb, lds);
        if (fl) Lpos[nL + pa] = i;
        if (fr) Rasc[nR + pb] = i;
        nL += ta;
        nR += tb;
    }
    __syncthreads();
    const int K = min(nL, nR);
    int cnt = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) cnt += Lpos[k] < Rasc[nR - 1 - k];
    const int kstar = block_sum(cnt, lds);
    for (int k = threadIdx.x; k < kstar; k += blockDim.x) a.swap(Lpos[k], Rasc[nR - 1 - k]);
    const int cl = kstar < nL ? Lpos[kstar] : INT_MAX;
    const int cr = kstar > 0 ? Rasc[nR - kstar] : INT_MAX;
    __syncthreads();
    return min(cl, cr);
}

// libstdc++ heap primitives, single thread (rare depth-limit fallback).
template <class A>
__device__ void adjust_heap(const A& a, int first, int hole, int len, typename A::Elem value) {
    const int top = hole;
    int second = hole;
    while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (a.val(first + second) > a.val(first + second - 1)) second--;
        a.put(first + hole, a.get(first + second));
        hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
        second = 2 * (second + 1);
        a.put(first + hole, a.get(first + second - 1));
        hole = second - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && a.val(first + parent) > A::ev(value)) {
        a.put(first + hole, a.get(first + parent));
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a.put(first + hole, value);
}

template <class A>
__device__ void heap_select(const A& a, int first, int middle, int last) {
    const int len = middle - first;
    if (len >= 2) {
        int parent = (len - 2) / 2;
        while (true) {
            adjust_heap(a, first, parent, len, a.get(first + parent));
            if (parent == 0) break;
            parent--;
        }
    }
    for (int i = middle; i < last; ++i)
        if (a.val(i) > a.val(first)) {
            typename A::Elem v = a.get(i);
            a.put(i, a.get(first));
            adjust_heap(a, first, 0, len, v);
        }
}

template <class A>
__device__ void insertion_sort(const A& a, int first, int last) {
    if (first == last) return;
    for (int i = first + 1; i != last; ++i) {
        typename A::Elem v = a.get(i);
        if (A::ev(v) > a.val(first)) {
            for (int k = i; k > first; --k) a.put(k, a.get(k - 1));
            a.put(first, v);
        } else {
            int k = i;
            while (A::ev(v) > a.val(k - 1)) {
                a.put(k, a.get(k - 1));
                --k;
            }
            a.put(k, v);
        }
    }
}

template <class A>
__device__ void move_median_to_first(const A& a, int result, int x, int y, int z) {
    if (a.val(x) > a.val(y)) {
        if (a.val(y) > a.val(z)) a.swap(result, y);
        else if (a.val(x) > a.val(z)) a.swap(result, z);
        else a.swap(result, x);
    } else if (a.val(x) > a.val(z)) a.swap(result, x);
    else if (a.val(y) > a.val(z)) a.swap(result, z);
    else a.swap(result, y);
}

// Returns the retained size; the first `result` entries hold the kept
// elements in libstdc++ order.  Must be called by the whole block.
// semantics kOcv32: OpenCV 3.2's retainBest ran nth_element at begin + n (not
// n - 1) and still read the boundary response at n - 1 (oracle retain_best).
template <class A>
__device__ int retain_best_block(const A& a, int n, int npoints, int depth, int32_t* Lpos, int32_t* Rasc, int* lds,
                                 int semantics = kOcv4) {
    if (npoints < 0 || n <= npoints) return n;
    if (npoints == 0) return 0;
    const int nth = semantics == kOcv32 ? npoints : npoints - 1;
    int first = 0, last = n;
    if (depth < 0) depth = 2 * (31 - __clz(n));
    bool heap_done = false;
    while (last - first > 3) {
        if (depth == 0) {
            if (threadIdx.x == 0) {
                heap_select(a, first, nth + 1, last);
                a.swap(first, nth);
            }
            heap_done = true;
            break;
        }
        --depth;
        if (threadIdx.x == 0) move_median_to_first(a, first, first + 1, first + (last - first) / 2, last - 1);
        __syncthreads();
        auto p = a.val(first);
        const int cut = partition_step(a, first, last, p, Lpos, Rasc, lds);
        if (cut <= first || cut >= last) break;  // impossible for a correct emulation; never loop unbounded
        if (cut <= nth) first = cut;
        else last = cut;
    }
    if (!heap_done && threadIdx.x == 0) insertion_sort(a, first, last);
    __syncthreads();
    // std::partition(begin+npoints, end, response >= ambiguous) (bidirectional)
    auto amb = a.val(npoints - 1);
    int nL = 0, nR = 0;
    for (int base = npoints; base < n; base += blockDim.x) {
        const int i = base + threadIdx.x;
        const bool in = i < n;
        int fl = 0, fr = 0;
        if (in) {
            bool pr = a.val(i) >= amb;
            fl = !pr;
            fr = pr;
        }
        int pa, pb, ta, tb;
        block_excl_scan2(fl, fr, pa, pb, ta, tb, lds);
        if (fl) Lpos[nL + pa] = i;
        if (fr) Rasc[nR + pb] = i;
        nL += ta;
        nR += tb;
    }
    __syncthreads();
    const int K = min(nL, nR);
    int cnt = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) cnt += Lpos[k] < Rasc[nR - 1 - k];
    const int kstar = block_sum(cnt, lds);
    for (int k = threadIdx.x; k < kstar; k += blockDim.x) a.swap(Lpos[k], Rasc[nR - 1 - k]);
    __syncthreads();
    return npoints + nR;
}

}  // namespace
}  // namespace dvo
