// FLANN randomized kd-tree k-NN for gfx950: the MI355X replacement of
// cv::FlannBasedMatcher(dict(algorithm=FLANN_INDEX_KDTREE, trees=5),
// dict(checks=50)).knnMatch(previous, current, k=2), the matcher of the
// reference's 'flann' mode (scripts/visual_odometry_v3.py:206-212).  The
// algorithm is OpenCV 4.x's bundled FLANN, restated in oracle/flann.cpp (see
// its header for the call chain); every step below reproduces it exactly:
//
//   draws      cv::theRNG() outputs of one tree: n shuffle draws, then one per
//              internal node in preorder (the host jumps the multiply-with-
//              carry state to each chunk's start: s_k = s_0 A^k mod m);
//   shuffle    cv::randShuffle(ind): for i = 0..n-1 swap(ind[r_i % n], ind[i]).
//              Sequential as written; here every output position is traced
//              backwards through the transpositions that touch it (step i
//              touches positions i and r_i % n; the steps with r_i % n = v
//              are bucketed by v), O(n log n) work in parallel;
//   divideTree level by level, one workgroup per open node: mean / variance
//              per dimension in float over the node's first min(101, count)
//              points in ind order (one thread per dimension, the sum in point
//              order), selectDivision's top-5 by (variance desc, index asc)
//              and rand_int(num) from the node's preorder draw, then
//              planeSplit's two Hoare passes as parallel pairings (the k-th
//              misplaced point from the left swaps with the k-th from the
//              right), and the split-point rule; node ids are preorder ids, so
//              the child ids follow from the left child's count;
//   search     one wave per query (getNeighbors with eps 0): descend every
//              tree, then pop branches from a binary heap in LDS (libstdc++'s
//              push_heap / pop_heap sift order, so ties pop as in OpenCV)
//              while fewer than `checks` leaves were checked or the result is
//              not full; the checked set is a bitset in LDS; flann::L2's
//              grouped sum ((d0^2 + d1^2) + d2^2) + d3^2 per lane, the groups
//              added in order; a KNNUniqueResultSet of (distance, index).
//              A query whose heap outgrows LDS is flagged and redone with its
//              heap in global memory (the heap holds up to n entries).
//
// Every step is a __device__ body with two kernels around it: the single-pair kernel that
// dvo_flann_knn / dvo_knn_pair_run drive from the host, and a batch twin for dvo_knn_stream's
// FLANN mode (the second half of this file), which takes the pair from the grid and the counts
// from the frame slots, so the arithmetic of both paths is the same text.
#include <algorithm>
#include <cfloat>
#include <climits>

#include "dvo_internal.h"
#include "mwc.h"

namespace dvo {
namespace {

constexpr uint64_t kTheRngA = 4164903690ull;
constexpr int kFlNT = 256;         // build kernels
constexpr int kFlSample = 101;     // SAMPLE_MEAN + 1
constexpr int kFlHeapLds = 1024;   // heap entries per query wave in LDS

__device__ __forceinline__ void flann_draws_body(const uint64_t* chunk_state, int nchunk, int total, uint32_t* R, int c) {
    if (c >= nchunk) return;
    const int b = (int)((int64_t)total * c / nchunk), e = (int)((int64_t)total * (c + 1) / nchunk);
    uint64_t st = chunk_state[c];
    for (int i = b; i < e; ++i) {
        st = (uint64_t)(uint32_t)st * kTheRngA + (st >> 32);
        R[i] = (uint32_t)st;
    }
}

__global__ void flann_draws_kernel(const uint64_t* chunk_state, int nchunk, int total, uint32_t* R) {
    flann_draws_body(chunk_state, nchunk, total, R, blockIdx.x * blockDim.x + threadIdx.x);
}

__device__ __forceinline__ void flann_bucket_count_body(const uint32_t* R, int n, int* cnt, int s) {
    if (s < n) atomicAdd(&cnt[R[s] % (uint32_t)n], 1);
}

__global__ void flann_bucket_count_kernel(const uint32_t* R, int n, int* cnt) {
    flann_bucket_count_body(R, n, cnt, blockIdx.x * blockDim.x + threadIdx.x);
}

// exclusive scan of cnt[0..n) into off[0..n], one workgroup of 1024 (n <= 2^16)
__device__ __forceinline__ void flann_bucket_scan_body(const int* cnt, int n, int* off, int* fill) {
    __shared__ int part[1024];
    const int per = (n + 1023) / 1024, b = threadIdx.x * per, e = min(n, b + per);
    int s = 0;
    for (int i = b; i < e; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
        const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = b; i < e; ++i) {
        off[i] = run;
        fill[i] = 0;
        run += cnt[i];
    }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

__global__ __launch_bounds__(1024) void flann_bucket_scan_kernel(const int* cnt, int n, int* off, int* fill) {
    flann_bucket_scan_body(cnt, n, off, fill);
}

__device__ __forceinline__ void flann_bucket_fill_body(const uint32_t* R, int n, const int* off, int* fill, int* list,
                                                       int s) {
    if (s >= n) return;
    const int v = (int)(R[s] % (uint32_t)n);
    list[off[v] + atomicAdd(&fill[v], 1)] = s;  // bucket order is irrelevant: the trace takes a maximum
}

__global__ void flann_bucket_fill_kernel(const uint32_t* R, int n, const int* off, int* fill, int* list) {
    flann_bucket_fill_body(R, n, off, fill, list, blockIdx.x * blockDim.x + threadIdx.x);
}

// new_ind[p] = ind[pos], pos = the position whose value the n transpositions move into p
__device__ __forceinline__ void flann_shuffle_trace_body(const uint32_t* R, int n, const int* off, const int* list,
                                                         const int* ind, int* new_ind, int p) {
    if (p >= n) return;
    int pos = p, s = n - 1;
    while (s >= 0) {
        const int s1 = pos <= s ? pos : -1;
        int s2 = -1;
        for (int q = off[pos]; q < off[pos + 1]; ++q) {
            const int t = list[q];
            if (t <= s && t > s2) s2 = t;
        }
        const int st = max(s1, s2);
        if (st < 0) break;
        if (st == s1 && st == s2) {
        } else if (st == s1) {  // step st = pos: swap(ind[r % n], ind[pos]) brought ind[r % n] here
            pos = (int)(R[st] % (uint32_t)n);
        } else {  // step st put ind[st] at position r_st % n == pos
            pos = st;
        }
        s = st - 1;
    }
    new_ind[p] = ind[pos];
}

__global__ void flann_shuffle_trace_kernel(const uint32_t* R, int n, const int* off, const int* list,
                                           const int* ind, int* new_ind) {
    flann_shuffle_trace_body(R, n, off, list, ind, new_ind, blockIdx.x * blockDim.x + threadIdx.x);
}

struct FlannBuild {
    const float* data;
    int n, dim;
    int* ind;            // [n], permuted in place by the splits
    float* xv;           // [n] split values along ind (per-node segment scratch)
    int* sl;             // [n] left stops
    int* sr;             // [n] right stops
    const uint32_t* R;   // the tree's draws: [0, n) shuffle, [n, 2n - 1) internal nodes in preorder
    int4* nodes;         // the tree's 2n - 1 nodes {divfeat, divval bits, child1, child2} (ids tree-local)
    int4* open[2];       // open nodes {segment start, count, node id, preorder internal index}
    int* cnt;            // [levels] open nodes per level
};

// the open list of a level (a select, not an index: B may live in registers)
__device__ __forceinline__ int4* open_list(const FlannBuild& B, int level) { return (level & 1) ? B.open[1] : B.open[0]; }

__device__ __forceinline__ int block_scan_excl(int v, int& total, int* sh) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kFlNT / 64; ++w) {
        const int c = sh[w];
        off += w < wid ? c : 0;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

// One Hoare pass of planeSplit over [lo, hi) of the node segment: the points with !keep in
// [lo, mid) pair with the points with keep in [mid, hi), the k-th from the left with the k-th
// from the right (mid = lo + #keep in [lo, hi)).
template <class Keep>
__device__ void hoare_pass(const FlannBuild& B, int a, int lo, int mid, int hi, Keep keep, int* sh) {
    int nl = 0, nr = 0;
    for (int b0 = lo; b0 < hi; b0 += kFlNT) {
        const int i = b0 + threadIdx.x;
        const bool in = i < hi;
        const bool k = in && keep(B.xv[a + i]);
        const int fl = in && i < mid && !k, fr = in && i >= mid && k;
        int tl, tr;
        const int pl = block_scan_excl(fl, tl, sh);
        const int pr = block_scan_excl(fr, tr, sh + 8);
        if (fl) B.sl[a + lo + nl + pl] = i;
        if (fr) B.sr[a + lo + nr + pr] = i;
        nl += tl;
        nr += tr;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nl; q += kFlNT) {  // nl == nr
        const int i = B.sl[a + lo + q], j = B.sr[a + lo + nr - 1 - q];
        const int ti = B.ind[a + i];
        B.ind[a + i] = B.ind[a + j];
        B.ind[a + j] = ti;
        const float tx = B.xv[a + i];
        B.xv[a + i] = B.xv[a + j];
        B.xv[a + j] = tx;
    }
    __syncthreads();
}

__device__ __forceinline__ bool var_better(float va, int ia, float vb, int ib) {
    return va > vb || (va == vb && ia < ib);
}

// One open node e = {segment start, count, node id, preorder internal index} of `level`: one
// workgroup of kFlNT.  Its children go to the next level's open list, or become leaves.
__device__ __forceinline__ void flann_level_body(const FlannBuild& B, int level, const int4 e) {
    const int a = e.x, c = e.y, id = e.z, pre = e.w;
    __shared__ int s_ind[kFlSample];
    __shared__ float s_mean[256], s_var[256];
    __shared__ int sh[16];
    __shared__ int s_top[5], s_cnt[2];
    const int cnt = min(kFlSample, c);
    for (int j = threadIdx.x; j < cnt; j += kFlNT) s_ind[j] = B.ind[a + j];
    __syncthreads();
    const int k = threadIdx.x;
    if (k < B.dim) {  // meanSplit: float sums in point order, one thread per dimension
        float m = 0.f;
        for (int j = 0; j < cnt; ++j) m += B.data[(int64_t)s_ind[j] * B.dim + k];
        m /= (float)cnt;
        float v = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float d = B.data[(int64_t)s_ind[j] * B.dim + k] - m;
            v += d * d;
        }
        s_mean[k] = m;
        s_var[k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // selectDivision: the RAND_DIM = 5 largest variances, (var desc, index asc)
        const int lane = threadIdx.x;
        float v[4];
        int ix[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ix[q] = lane + 64 * q;
            v[q] = ix[q] < B.dim ? s_var[ix[q]] : -FLT_MAX;
            if (ix[q] >= B.dim) ix[q] = INT_MAX;
        }
        const int num = min(5, B.dim);
        for (int r = 0; r < num; ++r) {
            float bv = -FLT_MAX;
            int bi = INT_MAX;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ix[q] != INT_MAX && (bi == INT_MAX || var_better(v[q], ix[q], bv, bi))) {
                    bv = v[q];
                    bi = ix[q];
                }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (oi != INT_MAX && (bi == INT_MAX || var_better(ov, oi, bv, bi))) {
                    bv = ov;
                    bi = oi;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ix[q] == bi) ix[q] = INT_MAX;  // taken
            if (lane == 0) s_top[r] = bi;
        }
        if (lane == 0) {
            const int rv = (int)(B.R[B.n + pre] & 0x7FFFFFFFu);
            const int rnd = (int)((double)num * (rv / (2147483647.0 + 1.0)));
            s_cnt[0] = s_top[rnd];
        }
    }
    __syncthreads();
    const int cutfeat = s_cnt[0];
    const float cutval = s_mean[cutfeat];
    // planeSplit: split values along the segment, then the two passes (< cutval, then <= cutval)
    int lim1 = 0, lim2 = 0;
    for (int b0 = 0; b0 < c; b0 += kFlNT) {
        const int i = b0 + threadIdx.x;
        int l1 = 0, l2 = 0;
        if (i < c) {
            const float x = B.data[(int64_t)B.ind[a + i] * B.dim + cutfeat];
            B.xv[a + i] = x;
            l1 = x < cutval;
            l2 = x <= cutval;
        }
        int t1, t2;
        block_scan_excl(l1, t1, sh);
        block_scan_excl(l2, t2, sh + 8);
        lim1 += t1;
        lim2 += t2;
    }
    __syncthreads();
    hoare_pass(B, a, 0, lim1, c, [&](float x) { return x < cutval; }, sh);
    hoare_pass(B, a, lim1, lim2, c, [&](float x) { return x <= cutval; }, sh);
    int index;
    if (lim1 > c / 2) index = lim1;
    else if (lim2 < c / 2) index = lim2;
    else index = c / 2;
    if (lim1 == c || lim2 == 0) index = c / 2;
    if (threadIdx.x == 0) {
        const int l_id = id + 1, r_id = id + 2 * index;
        B.nodes[id] = make_int4(cutfeat, __float_as_int(cutval), l_id, r_id);
        const int ca[2] = {a, a + index}, cc[2] = {index, c - index}, ci[2] = {l_id, r_id}, cp[2] = {pre + 1, pre + index};
        for (int h = 0; h < 2; ++h) {
            if (cc[h] == 1) {
                B.nodes[ci[h]] = make_int4(B.ind[ca[h]], 0, -1, -1);
            } else {
                const int slot = atomicAdd(&B.cnt[level + 1], 1);
                open_list(B, level + 1)[slot] = make_int4(ca[h], cc[h], ci[h], cp[h]);
            }
        }
    }
}

__global__ __launch_bounds__(kFlNT) void flann_level_kernel(FlannBuild B, int level) {
    if ((int)blockIdx.x >= B.cnt[level]) return;
    flann_level_body(B, level, open_list(B, level)[blockIdx.x]);
}

__device__ __forceinline__ void flann_root_body(const FlannBuild& B) {
    if (threadIdx.x != 0) return;
    if (B.n == 1) {
        B.nodes[0] = make_int4(B.ind[0], 0, -1, -1);
        B.cnt[0] = 0;
    } else {
        B.open[0][0] = make_int4(0, B.n, 0, 0);
        B.cnt[0] = 1;
    }
}

__global__ void flann_root_kernel(FlannBuild B) { flann_root_body(B); }

// ---- search ------------------------------------------------------------------
struct FlannSearch {
    const float* q;        // [nq][dim]
    const float* t;        // [n][dim]
    const int4* nodes;     // [trees][2n - 1]
    int nq, n, dim, k, trees, checks, nodes_per_tree;
    int32_t* idx;          // [nq][k]
    float* dist;           // [nq][k]
    int32_t* flag;         // [nq]: heap outgrew LDS (redo with the global heap)
    const int32_t* redo;   // global-heap pass: the query of each workgroup
    float* gheap_d;        // global-heap pass: [workgroups][n]
    int32_t* gheap_n;
};

// Query qi of S, one wave: `checked` holds (S.n + 31) / 32 words of LDS, hd / hn a heap of hcap
// entries.  Writes the query's k results unless the heap outgrew hcap, which it returns.
__device__ __forceinline__ bool flann_search_body(const FlannSearch& S, int qi, uint32_t* checked, float* hd, int* hn,
                                                  int hcap) {
    const int lane = threadIdx.x;
    const int nwords = (S.n + 31) >> 5;
    for (int w = lane; w < nwords; w += 64) checked[w] = 0;
    const int ng = S.dim >> 2;  // groups of 4 (dim % 4 == 0)
    const float4 qv = lane < ng ? *reinterpret_cast<const float4*>(S.q + (int64_t)qi * S.dim + 4 * lane)
                                : make_float4(0.f, 0.f, 0.f, 0.f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // result set (KNNUniqueResultSet), wave-uniform
    float rd[4] = {FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX};
    int ri[4] = {-1, -1, -1, -1};
    int rsize = 0;
    bool full = false;
    float worst = FLT_MAX;
    int check_count = 0, hs = 0;
    bool overflow = false;
    auto qval = [&](int f) {  // q[f], f wave-uniform
        const int src = f >> 2, comp = f & 3;
        const float x = comp == 0 ? qv.x : comp == 1 ? qv.y : comp == 2 ? qv.z : qv.w;
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
    };
    auto add_point = [&](float d, int index) {
        if (d >= worst) return;
        int pos = rsize;  // (distance, index) order; an index is checked once, so no duplicates
        while (pos > 0 && (rd[pos - 1] > d || (rd[pos - 1] == d && ri[pos - 1] > index))) --pos;
        for (int j = 3; j > 0; --j)
            if (j > pos) {
                rd[j] = rd[j - 1];
                ri[j] = ri[j - 1];
            }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j == pos) {
                rd[j] = d;
                ri[j] = index;
            }
        if (rsize < S.k) ++rsize;
        if (rsize == S.k) {
            full = true;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j == S.k - 1) worst = rd[j];
        }
    };
    // std::push_heap / __adjust_heap with CompareT(a, b) = b.mindist < a.mindist (a min-heap)
    auto heap_push = [&](int node, float md) {
        if (hs == S.n) return;  // Heap::insert drops when full (count == length)
        if (hs == hcap) {
            overflow = true;
            return;
        }
        int hole = hs, parent = (hole - 1) / 2;
        while (hole > 0 && md < hd[parent]) {
            if (lane == 0) {
                hd[hole] = hd[parent];
                hn[hole] = hn[parent];
            }
            hole = parent;
            parent = (hole - 1) / 2;
        }
        if (lane == 0) {
            hd[hole] = md;
            hn[hole] = node;
        }
        ++hs;
    };
    auto heap_pop = [&](int& node, float& md) {
        node = hn[0];
        md = hd[0];
        const int len = hs - 1;
        if (len > 0) {
            const float vd = hd[len];
            const int vn = hn[len];
            int hole = 0, second = 0;
            while (second < (len - 1) / 2) {
                second = 2 * (second + 1);
                if (hd[second - 1] < hd[second]) second--;
                if (lane == 0) {
                    hd[hole] = hd[second];
                    hn[hole] = hn[second];
                }
                hole = second;
            }
            if ((len & 1) == 0 && second == (len - 2) / 2) {
                second = 2 * (second + 1);
                if (lane == 0) {
                    hd[hole] = hd[second - 1];
                    hn[hole] = hn[second - 1];
                }
                hole = second - 1;
            }
            int parent = (hole - 1) / 2;
            while (hole > 0 && vd < hd[parent]) {
                if (lane == 0) {
                    hd[hole] = hd[parent];
                    hn[hole] = hn[parent];
                }
                hole = parent;
                parent = (hole - 1) / 2;
            }
            if (lane == 0) {
                hd[hole] = vd;
                hn[hole] = vn;
            }
        }
        hs = len;
    };
    auto descend = [&](int tree, int node, float mindist) {
        const int4* nodes = S.nodes + (int64_t)tree * S.nodes_per_tree;
        while (!overflow) {
            if (worst < mindist) return;
            const int4 nd = nodes[__builtin_amdgcn_readfirstlane(node)];
            if (nd.z < 0 && nd.w < 0) {  // leaf: check it once
                const int index = nd.x;
                const uint32_t bit = 1u << (index & 31);
                if ((checked[index >> 5] & bit) || (check_count >= S.checks && full)) return;
                if (lane == 0) checked[index >> 5] |= bit;
                ++check_count;
                float g = 0.f;
                if (lane < ng) {
                    const float4 tv = *reinterpret_cast<const float4*>(S.t + (int64_t)index * S.dim + 4 * lane);
                    const float d0 = tv.x - qv.x, d1 = tv.y - qv.y, d2 = tv.z - qv.z, d3 = tv.w - qv.w;
                    g = d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
                }
                float d = 0.f;
                for (int j = 0; j < ng; ++j) d += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g), j));
                add_point(d, index);
                return;
            }
            const float val = qval(nd.x);
            const float divval = __int_as_float(nd.y);
            const float diff = val - divval;
            const int best = diff < 0 ? nd.z : nd.w, other = diff < 0 ? nd.w : nd.z;
            const float new_distsq = mindist + (val - divval) * (val - divval);
            if (new_distsq * 1.0f < worst || !full) heap_push(tree * S.nodes_per_tree + other, new_distsq);
            node = best;
        }
    };
    for (int tr = 0; tr < S.trees && !overflow; ++tr) {
        descend(tr, 0, 0.f);
        if (check_count >= S.checks && full) break;
    }
    while (hs > 0 && !overflow) {
        int gnode;
        float md;
        heap_pop(gnode, md);
        if (!(check_count < S.checks || !full)) break;
        const int tr = gnode / S.nodes_per_tree;
        descend(tr, gnode - tr * S.nodes_per_tree, md);
    }
    if (lane == 0 && !overflow)
        for (int j = 0; j < S.k; ++j) {
            S.idx[(int64_t)qi * S.k + j] = j < rsize ? ri[j] : -1;
            S.dist[(int64_t)qi * S.k + j] = j < rsize ? rd[j] : FLT_MAX;
        }
    return overflow;
}

template <bool kGlobalHeap>
__global__ __launch_bounds__(64) void flann_search_kernel(FlannSearch S) {
    extern __shared__ uint32_t smem[];
    const int qi = kGlobalHeap ? S.redo[blockIdx.x] : (int)blockIdx.x;
    if (qi >= S.nq) return;
    const int nwords = (S.n + 31) >> 5;
    float* hd = kGlobalHeap ? S.gheap_d + (int64_t)blockIdx.x * S.n : reinterpret_cast<float*>(smem + nwords);
    int* hn = kGlobalHeap ? S.gheap_n + (int64_t)blockIdx.x * S.n : reinterpret_cast<int*>(smem + nwords + kFlHeapLds);
    const bool overflow = flann_search_body(S, qi, smem, hd, hn, kGlobalHeap ? S.n : min(S.n, kFlHeapLds));
    if (!kGlobalHeap && threadIdx.x == 0) S.flag[qi] = overflow ? 1 : 0;
}

__global__ void flann_redo_list_kernel(const int32_t* flag, int nq, int32_t* list, int32_t* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq && flag[i]) list[atomicAdd(count, 1)] = i;
}


// ---- the batch twins (dvo_knn_stream's FLANN mode) -------------------------------------------
// The pair is a grid dimension and nq / nt come from fstate, so no count crosses to the host.  A
// workgroup of a pair that builds nothing (nq == 0 or nt < 2: an empty or marked frame, a single
// train) returns before its first descriptor load.  fstate counts never exceed cap
// (knn_frame_state_kernel), which bounds every index below: rows < nt <= cap, nodes < 2 nt - 1.

// the draws of a pair's forest: the theRNG state advances by them only when the forest is built
__host__ __device__ inline uint64_t flann_pair_draws(int nq, int nt, int trees) {
    return nq >= 1 && nt >= 2 ? (uint64_t)trees * (uint64_t)(2 * nt - 1) : 0;
}

__device__ __forceinline__ bool flann_pair(const FlannBatchArgs& a, int p, int& nq, int& nt) {
    nq = a.fstate[2 * p];
    nt = a.fstate[2 * p + 2];
    return nq >= 1 && nt >= 2;
}

// tree `tree` of pair p: it shuffles the order the tree before it left (ind and ind2 take turns)
__device__ __forceinline__ FlannBuild flann_pair_build(const FlannBatchArgs& a, int p, int nt, int tree) {
    const size_t C = (size_t)a.cap, o = (size_t)p * C;
    return FlannBuild{a.desc + (size_t)(p + 1) * C * a.dim, nt, a.dim, ((tree & 1) ? a.ind : a.ind2) + o, a.xv + o,
                      a.sl + o, a.sr + o, a.R + 2 * o, a.nodes + (size_t)p * a.trees * 2 * C + (size_t)tree * (2 * nt - 1),
                      {a.open + 2 * o, a.open + 2 * o + C}, a.lev + (size_t)p * (C + 2)};
}

__device__ __forceinline__ FlannSearch flann_pair_search(const FlannBatchArgs& a, int p, int nq, int nt) {
    const size_t C = (size_t)a.cap, o = (size_t)p * C;
    return FlannSearch{a.desc + o * a.dim, a.desc + (o + C) * a.dim, a.nodes + (size_t)p * a.trees * 2 * C,
                       nq, nt, a.dim, 2, a.trees, a.checks, 2 * nt - 1, a.idx + 2 * o, a.dist + 2 * o,
                       nullptr, nullptr, nullptr, nullptr};
}

// RNG plan, one workgroup: pair p's forest starts after the draws of the built pairs before it
// (an exclusive scan of their draw counts, then a jump by that count), every (pair, tree, chunk)
// start follows from the pair's, and the stream's state moves past the whole call.
//
// A sharded stream (FlannShard) runs the same plan on every rank over that rank's pairs of a
// window: `pre` are the draws of the ranks below it and `post` those of the ranks above it, so the
// plan starts from the state jumped by pre and leaves it jumped by pre + own + post, the state
// after the whole window on every rank.  mwc_jump_by composes (a jump by a, then one by b, is a
// jump by a + b), so each start equals the one a single plan over the whole window computes.
// Headroom of the 64-bit sums: a call's draws are at most 65,535 pairs x 64 trees x 131,071 draws
// (2 cap - 1 at cap = 65,536), about 5.5e11 < 2^40; 1024 ranks of them stay below 2^50.
__device__ __forceinline__ void flann_rng_plan_body(const FlannBatchArgs& a, int pairs, uint64_t pre, uint64_t post,
                                                    uint64_t* part /* LDS [1024] */) {
    const int tid = threadIdx.x;
    const int per = (pairs + 1023) / 1024, b = min(pairs, tid * per), e = min(pairs, b + per);
    uint64_t sum = 0;
    for (int p = b; p < e; ++p) sum += flann_pair_draws(a.fstate[2 * p], a.fstate[2 * p + 2], a.trees);
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
        const uint64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const uint64_t st0 = mwc_jump_by(*a.state, pre);
    uint64_t run = part[tid] - sum;
    for (int p = b; p < e; ++p) {
        a.starts[p] = mwc_jump_by(st0, run);
        run += flann_pair_draws(a.fstate[2 * p], a.fstate[2 * p + 2], a.trees);
    }
    __syncthreads();  // every thread has read the state, and the starts are written
    if (tid == 0) {
        *a.state = mwc_jump_by(st0, part[1023] + post);
        a.ctl[0] = 0;
        a.ctl[1] = 0;
    }
    const int per_pair = a.trees * kFlannChunks;
    for (int64_t i = tid; i < (int64_t)pairs * per_pair; i += 1024) {
        const int p = (int)(i / per_pair), r = (int)(i - (int64_t)p * per_pair), t = r / kFlannChunks, c = r % kFlannChunks;
        int nq, nt;
        if (!flann_pair(a, p, nq, nt)) continue;
        const int draws = 2 * nt - 1;
        a.cs[i] = mwc_jump_by(a.starts[p], (uint64_t)t * draws + (uint64_t)((int64_t)draws * c / kFlannChunks));
    }
}

__global__ __launch_bounds__(1024) void flann_rng_plan_kernel(FlannBatchArgs a, int pairs) {
    __shared__ uint64_t part[1024];
    flann_rng_plan_body(a, pairs, 0, 0, part);
}

// the workgroup's sum of v, to every thread; part is free again on return
__device__ __forceinline__ uint64_t flann_block_sum(uint64_t* part /* LDS [1024] */, uint64_t v) {
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    const uint64_t s = part[0];
    __syncthreads();
    return s;
}

// The sharded twin: one entry of the ranks' draw counts per lane (world <= 1024), summed below and
// above this rank; entry [rank] is not read.
__global__ __launch_bounds__(1024) void flann_rng_plan_shard_kernel(FlannBatchArgs a, int pairs, FlannShard sh) {
    __shared__ uint64_t part[1024];
    const int tid = threadIdx.x;
    const uint64_t v = tid < sh.world && tid != sh.rank ? sh.draws[tid] : 0;
    const uint64_t pre = flann_block_sum(part, tid < sh.rank ? v : 0);
    const uint64_t post = flann_block_sum(part, tid > sh.rank ? v : 0);
    flann_rng_plan_body(a, pairs, pre, post, part);
}

// The draws the call's pairs will consume (what the plan's scan ends at), for the ranks above
// this one: one workgroup, one plain 64-bit store.
__global__ __launch_bounds__(1024) void flann_shard_draws_kernel(const int32_t* fstate, int pairs, int trees,
                                                                 uint64_t* out) {
    __shared__ uint64_t part[1024];
    uint64_t sum = 0;
    for (int p = threadIdx.x; p < pairs; p += 1024) sum += flann_pair_draws(fstate[2 * p], fstate[2 * p + 2], trees);
    sum = flann_block_sum(part, sum);
    if (threadIdx.x == 0) *out = sum;
}

__global__ void flann_set_state_kernel(uint64_t* state, uint64_t value) { *state = value; }

// before tree `tree`: empty shuffle buckets and level counts; the first tree shuffles 0..nt-1
__global__ __launch_bounds__(256) void flann_prep_batch_kernel(FlannBatchArgs a, int tree) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const size_t C = (size_t)a.cap, o = (size_t)p * C;
    if (i < nt) {
        a.bcnt[o + i] = 0;
        if (tree == 0) a.ind[o + i] = i;
    }
    if (i < nt + 2) a.lev[(size_t)p * (C + 2) + i] = 0;
}

__global__ __launch_bounds__(kFlannChunks) void flann_draws_batch_kernel(FlannBatchArgs a, int tree) {
    const int p = blockIdx.y;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    flann_draws_body(a.cs + ((size_t)p * a.trees + tree) * kFlannChunks, kFlannChunks, 2 * nt - 1,
                     a.R + 2 * (size_t)p * a.cap, threadIdx.x);
}

__global__ __launch_bounds__(256) void flann_bucket_count_batch_kernel(FlannBatchArgs a) {
    const int p = blockIdx.y;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const size_t o = (size_t)p * a.cap;
    flann_bucket_count_body(a.R + 2 * o, nt, a.bcnt + o, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(1024) void flann_bucket_scan_batch_kernel(FlannBatchArgs a) {
    const int p = blockIdx.x;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const size_t o = (size_t)p * a.cap;
    flann_bucket_scan_body(a.bcnt + o, nt, a.boff + o + p, a.bfill + o);
}

__global__ __launch_bounds__(256) void flann_bucket_fill_batch_kernel(FlannBatchArgs a) {
    const int p = blockIdx.y;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const size_t o = (size_t)p * a.cap;
    flann_bucket_fill_body(a.R + 2 * o, nt, a.boff + o + p, a.bfill + o, a.blist + o, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void flann_shuffle_trace_batch_kernel(FlannBatchArgs a, int tree) {
    const int p = blockIdx.y;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const size_t o = (size_t)p * a.cap;
    flann_shuffle_trace_body(a.R + 2 * o, nt, a.boff + o + p, a.blist + o, ((tree & 1) ? a.ind2 : a.ind) + o,
                             ((tree & 1) ? a.ind : a.ind2) + o, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(64) void flann_root_batch_kernel(FlannBatchArgs a, int tree) {
    const int p = blockIdx.x;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    flann_root_body(flann_pair_build(a, p, nt, tree));
}

// Level `level` of every pair's tree: workgroup x takes open nodes x, x + gridDim.x, ... of its
// pair (the list is complete: the launch before filled it, this one fills the other).  A tree
// over nt points has no open node at level nt - 1 or below it (every split gives both children a point).
__global__ __launch_bounds__(kFlNT) void flann_level_batch_kernel(FlannBatchArgs a, int tree, int level) {
    const int p = blockIdx.y;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt) || level >= nt - 1) return;
    const FlannBuild B = flann_pair_build(a, p, nt, tree);
    const int c = B.cnt[level];
    if ((int)blockIdx.x >= c) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&a.ctl[1], level + 1);
    for (int slot = blockIdx.x; slot < c; slot += gridDim.x) {
        flann_level_body(B, level, open_list(B, level)[slot]);
        __syncthreads();  // the body's LDS is rewritten by the next node
    }
}

// The levels from level0 on, a workgroup per pair: it walks the open nodes of a level one after
// another with the level kernel's body, then the level they opened, until a level is empty.  A
// split leaves both children at least one point, so a node at level l holds at most nt - l
// points and no node is open at level nt - 1: the loop ends after at most nt - 1 - level0 levels.
__global__ __launch_bounds__(kFlNT) void flann_tail_batch_kernel(FlannBatchArgs a, int tree, int level0) {
    const int p = blockIdx.x;
    int nq, nt;
    if (!flann_pair(a, p, nq, nt)) return;
    const FlannBuild B = flann_pair_build(a, p, nt, tree);
    for (int level = level0; level < nt - 1; ++level) {
        // the count and the list were written by this workgroup's thread 0 (or a level launch before)
        const int c = __hip_atomic_load(&B.cnt[level], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) break;
        if (threadIdx.x == 0) atomicMax(&a.ctl[1], level + 1);
        for (int slot = 0; slot < c; ++slot) {
            flann_level_body(B, level, open_list(B, level)[slot]);
            __syncthreads();  // the body's LDS is rewritten by the next node; its stores are visible to the workgroup
        }
    }
}

__global__ __launch_bounds__(64) void flann_search_batch_kernel(FlannBatchArgs a) {
    extern __shared__ uint32_t smem[];
    const int p = blockIdx.y, qi = blockIdx.x;
    int nq, nt;
    const bool built = flann_pair(a, p, nq, nt);
    if (qi >= nq) return;
    if (!built) {  // a single train: no forest; the ratio test sees a query without neighbours
        if (threadIdx.x < 2) {
            const size_t o = ((size_t)p * a.cap + qi) * 2 + threadIdx.x;
            a.idx[o] = -1;
            a.dist[o] = FLT_MAX;
        }
        return;
    }
    const FlannSearch S = flann_pair_search(a, p, nq, nt);
    const int nwords = (nt + 31) >> 5;  // this pair's words only: the launch's LDS is sized for cap
    const bool overflow = flann_search_body(S, qi, smem, reinterpret_cast<float*>(smem + nwords),
                                            reinterpret_cast<int*>(smem + nwords + kFlHeapLds), min(nt, kFlHeapLds));
    if (overflow && threadIdx.x == 0) a.redo[atomicAdd(&a.ctl[0], 1)] = (uint32_t)p * (uint32_t)a.cap + (uint32_t)qi;
}

// The queries whose heap outgrew LDS, all pairs' in one list (its length is read here): a fixed
// pool of workgroups strides over it, each with a heap of cap entries in global memory.
__global__ __launch_bounds__(64) void flann_redo_batch_kernel(FlannBatchArgs a) {
    extern __shared__ uint32_t smem[];
    const int count = a.ctl[0];
    float* hd = a.gheap_d + (size_t)blockIdx.x * a.cap;
    int* hn = a.gheap_n + (size_t)blockIdx.x * a.cap;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t v = a.redo[i];
        const int p = (int)(v / (uint32_t)a.cap), qi = (int)(v % (uint32_t)a.cap);
        int nq, nt;
        if (!flann_pair(a, p, nq, nt) || qi >= nq) continue;
        flann_search_body(flann_pair_search(a, p, nq, nt), qi, smem, hd, hn, nt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace

size_t flann_search_lds(int n) { return ((size_t)(n + 31) / 32 + 2 * kFlHeapLds) * 4; }

hipError_t launch_flann_draws(const uint64_t* d_chunk_state, int nchunk, int total, uint32_t* d_R, hipStream_t s) {
    hipLaunchKernelGGL(flann_draws_kernel, dim3((nchunk + 63) / 64), dim3(64), 0, s, d_chunk_state, nchunk, total, d_R);
    return hipGetLastError();
}

hipError_t launch_flann_shuffle(const uint32_t* d_R, int n, int* d_cnt, int* d_off, int* d_fill, int* d_list,
                                const int* d_ind, int* d_new_ind, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(int) * n, s);
    if (e != hipSuccess) return e;
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(flann_bucket_count_kernel, dim3(g), dim3(256), 0, s, d_R, n, d_cnt);
    hipLaunchKernelGGL(flann_bucket_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, n, d_off, d_fill);
    hipLaunchKernelGGL(flann_bucket_fill_kernel, dim3(g), dim3(256), 0, s, d_R, n, d_off, d_fill, d_list);
    hipLaunchKernelGGL(flann_shuffle_trace_kernel, dim3(g), dim3(256), 0, s, d_R, n, d_off, d_list, d_ind, d_new_ind);
    return hipGetLastError();
}

hipError_t launch_flann_root(const FlannBuildArgs& a, hipStream_t s) {
    FlannBuild B{a.data, a.n, a.dim, a.ind, a.xv, a.sl, a.sr, a.R, a.nodes, {a.open0, a.open1}, a.cnt};
    hipLaunchKernelGGL(flann_root_kernel, dim3(1), dim3(64), 0, s, B);
    return hipGetLastError();
}

hipError_t launch_flann_level(const FlannBuildArgs& a, int level, int max_open, hipStream_t s) {
    FlannBuild B{a.data, a.n, a.dim, a.ind, a.xv, a.sl, a.sr, a.R, a.nodes, {a.open0, a.open1}, a.cnt};
    hipLaunchKernelGGL(flann_level_kernel, dim3(max_open), dim3(kFlNT), 0, s, B, level);
    return hipGetLastError();
}

hipError_t launch_flann_search(const FlannSearchArgs& a, hipStream_t s) {
    FlannSearch S{a.q, a.t, a.nodes, a.nq, a.n, a.dim, a.k, a.trees, a.checks, 2 * a.n - 1,
                  a.idx, a.dist, a.flag, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(flann_search_kernel<false>, dim3(a.nq), dim3(64), flann_search_lds(a.n), s, S);
    return hipGetLastError();
}

hipError_t launch_flann_redo_list(const int32_t* d_flag, int nq, int32_t* d_list, int32_t* d_count, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flann_redo_list_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, d_flag, nq, d_list, d_count);
    return hipGetLastError();
}

hipError_t launch_flann_search_global(const FlannSearchArgs& a, const int32_t* d_list, int count, float* d_heap_d,
                                      int32_t* d_heap_n, hipStream_t s) {
    FlannSearch S{a.q, a.t, a.nodes, a.nq, a.n, a.dim, a.k, a.trees, a.checks, 2 * a.n - 1,
                  a.idx, a.dist, a.flag, d_list, d_heap_d, d_heap_n};
    hipLaunchKernelGGL(flann_search_kernel<true>, dim3(count), dim3(64), ((size_t)(a.n + 31) / 32) * 4, s, S);
    return hipGetLastError();
}

size_t flann_batch_bytes(int pairs, int cap, int trees) {
    FlannBatchArgs a{};
    size_t total = 0;
    flann_batch_layout(a, pairs, cap, trees, [&](auto*&, size_t bytes) {
        total += bytes;
        return true;
    });
    return total;
}

hipError_t launch_flann_set_state(uint64_t* d_state, uint64_t value, hipStream_t s) {
    hipLaunchKernelGGL(flann_set_state_kernel, dim3(1), dim3(1), 0, s, d_state, value);
    return hipGetLastError();
}

void flann_rng_plan_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees, uint64_t* starts,
                         uint64_t* state_out) {
    auto brings = [&](int f) { return counts[f] > cap ? 0 : std::max(counts[f], 0); };  // knn_frame_state_kernel
    uint64_t run = 0;
    for (int p = 0; p + 1 < frames; ++p) {
        starts[p] = mwc_jump_by(state, run);
        run += flann_pair_draws(brings(p), brings(p + 1), trees);
    }
    *state_out = mwc_jump_by(state, run);
}

void flann_rng_shard_host(uint64_t state, const int32_t* counts, int frames, int cap, int trees,
                          const uint64_t* shard_draws, int world, int rank, uint64_t* starts, uint64_t* state_out,
                          uint64_t* own_draws) {
    auto brings = [&](int f) { return counts[f] > cap ? 0 : std::max(counts[f], 0); };  // knn_frame_state_kernel
    uint64_t pre = 0, post = 0;
    for (int i = 0; shard_draws && i < world; ++i)
        if (i != rank) (i < rank ? pre : post) += shard_draws[i];
    const uint64_t st0 = mwc_jump_by(state, pre);
    uint64_t run = 0;
    for (int p = 0; p + 1 < frames; ++p) {
        if (starts) starts[p] = mwc_jump_by(st0, run);
        run += flann_pair_draws(brings(p), brings(p + 1), trees);
    }
    if (state_out) *state_out = mwc_jump_by(st0, run + post);
    if (own_draws) *own_draws = run;
}

hipError_t launch_flann_shard_draws(const int32_t* d_fstate, int frames, int trees, uint64_t* d_draws, hipStream_t s) {
    hipLaunchKernelGGL(flann_shard_draws_kernel, dim3(1), dim3(1024), 0, s, d_fstate, std::max(frames - 1, 0), trees,
                       d_draws);
    return hipGetLastError();
}

hipError_t launch_flann_batch(const FlannBatchArgs& a, int frames, int levels, hipStream_t s, const FlannShard* shard) {
    const int P = frames - 1;
    if (P < 1) return hipSuccess;
    if (shard)
        hipLaunchKernelGGL(flann_rng_plan_shard_kernel, dim3(1), dim3(1024), 0, s, a, P, *shard);
    else
        hipLaunchKernelGGL(flann_rng_plan_kernel, dim3(1), dim3(1024), 0, s, a, P);
    const int L = levels > 0 ? levels : kFlannLevels, C = a.cap;
    const dim3 rows((C + 255) / 256, P);
    for (int t = 0; t < a.trees; ++t) {  // serial: tree t shuffles the order tree t - 1 left
        hipLaunchKernelGGL(flann_prep_batch_kernel, dim3((C + 2 + 255) / 256, P), dim3(256), 0, s, a, t);
        hipLaunchKernelGGL(flann_draws_batch_kernel, dim3(1, P), dim3(kFlannChunks), 0, s, a, t);
        hipLaunchKernelGGL(flann_bucket_count_batch_kernel, rows, dim3(256), 0, s, a);
        hipLaunchKernelGGL(flann_bucket_scan_batch_kernel, dim3(P), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(flann_bucket_fill_batch_kernel, rows, dim3(256), 0, s, a);
        hipLaunchKernelGGL(flann_shuffle_trace_batch_kernel, rows, dim3(256), 0, s, a, t);
        hipLaunchKernelGGL(flann_root_batch_kernel, dim3(P), dim3(64), 0, s, a, t);
        // a per-pair open list: level l has at most min(2^l, nt / 2) open nodes (each holds 2 points or
        // more); a pair gets at most `wide` workgroups, which stride over its list, so that the deep,
        // nearly empty levels do not pay for cap / 2 workgroups per pair that return at once
        const int wide = std::max(32, 8192 / P);
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(flann_level_batch_kernel,
                               dim3((int)std::min<int64_t>(std::min<int64_t>(int64_t(1) << std::min(l, 20), C / 2 + 1), wide), P),
                               dim3(kFlNT), 0, s, a, t, l);
        hipLaunchKernelGGL(flann_tail_batch_kernel, dim3(P), dim3(kFlNT), 0, s, a, t, L);
    }
    hipLaunchKernelGGL(flann_search_batch_kernel, dim3(C, P), dim3(64), flann_search_lds(C), s, a);
    hipLaunchKernelGGL(flann_redo_batch_kernel, dim3(kFlannRedoPool), dim3(64), ((size_t)(C + 31) / 32) * 4, s, a);
    return hipGetLastError();
}

}  // namespace dvo
