// Exhaustive neighbour joining (`-slow`: exhaustiveNJSearch, NJ.tcc:3648-3684) on a device-resident matrix of join distances.
//
// The reference evaluates setDistCriterion for every pair of active nodes at every join - O(N^3 L) profile arithmetic.  The
// join distance of two unchanged nodes does not change between joins (profileDist / seqDist minus the two diameters,
// NJ.tcc:1115-1124); only the out-distances in the criterion do.  So the distances are kept: an S x S matrix of numeric_t in
// SLOT space (S = nSeqs, rows `ld` apart: S rounded up to 64 elements), both triangles, symmetric, nodeOf[slot] = the node
// that owns the slot.  Live slots are always 0 .. nLive-1: a join hands the slot of one child to the new node and moves the
// node of the last live slot into the other child's slot (k_ex_move), so a search never meets a dead row or column.
//
//   fill        every leaf x leaf distance through the block kernels of vft_kernels_nj.h (k_pairs_block_tiled: seqDist's
//               counts for nucleotides; k_pairs_block: the generic pair path for matrix alphabets), written straight into
//               the matrix; k_ex_mirror then copies the upper triangle - profileDist(lower id, higher id), the order the
//               reference's loop calls it in - over the lower one.
//   row         after a join: the distances (active node, new node), the new node as profile2 (codeDist is taken from
//               profile2 only, NJ.tcc:1178-1180), by k_pairs_block with b = {new node} - a wavefront per pair: a block one
//               node wide leaves the lane-per-pair kernel one lane per workgroup - into the new node's row; k_ex_column
//               copies the row into its column.
//   search      k_ex_prepare gathers the out-distances per slot; k_ex_search makes one pass over the upper triangle of the
//               live slots - a wavefront per row, 64 lanes x 4 consecutive elements (16 bytes of float per lane, 1 KiB per
//               wave instruction, two in flight), rows r and nLive-2-r paired and split by chunks so that every wavefront
//               reads the same amount - forms the
//               criterion with vft_criterion's operations (double arithmetic on the numeric_t distance and the two
//               out-distances, one rounding to numeric_t; the library is built without contraction) and reduces the key
//               (criterion, lower node id, higher node id) to its lexicographic minimum: per lane, across the wavefront
//               with shuffles, across the workgroup through LDS, across workgroups through per-workgroup partials that
//               k_ex_finish reduces.  The key is a total order over pairs, so the result does not depend on which lane,
//               wavefront or workgroup saw a pair: it is the first (i, j) in the reference's one-thread loop order (i
//               ascending, j > i ascending, strict <) among the pairs that attain the minimum.  No float atomics.
#pragma once
#include "vft_kernels_tophits.h"

#define VFT_EX_WG 256
#define VFT_EX_MAX_PARTS 2048

template <typename REAL>
struct ExKey {
    REAL crit, dist;
    int32_t lo, hi;   // node ids, lo < hi
};

struct ExBestOut {   // the search's answer, host-mapped
    double dist, crit;
    int32_t i, j;
    int32_t stale, pad;   // stale != 0: an active node's out-distance did not carry the stamp nActive
};

template <typename REAL>
__device__ __forceinline__ bool vft_ex_better(const ExKey<REAL> &a, const ExKey<REAL> &b) {
    if (a.crit < b.crit) return true;
    if (!(a.crit == b.crit)) return false;
    return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi);
}

template <typename REAL>
__device__ __forceinline__ ExKey<REAL> vft_ex_none() {
    ExKey<REAL> k;
    k.crit = (REAL) INFINITY;
    k.dist = (REAL) 0;
    k.lo = k.hi = 0x7FFFFFFF;
    return k;
}

template <typename REAL>
__device__ __forceinline__ ExKey<REAL> vft_ex_wave_min(ExKey<REAL> k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ExKey<REAL> o;
        o.crit = __shfl_xor(k.crit, off, 64);
        o.dist = __shfl_xor(k.dist, off, 64);
        o.lo = __shfl_xor(k.lo, off, 64);
        o.hi = __shfl_xor(k.hi, off, 64);
        if (vft_ex_better<REAL>(o, k)) k = o;
    }
    return k;
}

// the workgroup's minimum, valid in thread 0
template <typename REAL>
__device__ __forceinline__ ExKey<REAL> vft_ex_block_min(ExKey<REAL> k) {
    __shared__ ExKey<REAL> sKey[VFT_EX_WG / 64];
    k = vft_ex_wave_min<REAL>(k);
    if ((threadIdx.x & 63) == 0) sKey[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < VFT_EX_WG / 64; w++)
            if (vft_ex_better<REAL>(sKey[w], k)) k = sKey[w];
    return k;
}

// lower triangle <- upper triangle (once, after the fill)
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_mirror(REAL *M, int64_t ld, int64_t n) {
    const int64_t c = (int64_t) blockIdx.x * VFT_EX_WG + threadIdx.x;
    for (int64_t r = blockIdx.y; r < n; r += gridDim.y)
        if (c < r) M[r * ld + c] = M[c * ld + r];
}

// The slot bookkeeping of one join: the new node takes slot sI; the node of the last live slot moves into slot sJ (row and
// column, from its row).  Entries against slot sI are rewritten by the row update that follows.
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_move(REAL *M, int64_t ld, int64_t *nodeOf, int64_t sI, int64_t sJ, int64_t last,
                                                       int64_t newnode) {
    const int64_t c = (int64_t) blockIdx.x * VFT_EX_WG + threadIdx.x;
    if (c == 0) {   // (no other thread of this launch reads nodeOf)
        nodeOf[sI] = newnode;
        if (sJ != last) nodeOf[sJ] = nodeOf[last];
        nodeOf[last] = -1;
    }
    if (sJ == last || c >= last || c == sJ) return;
    const REAL v = M[last * ld + c];
    M[sJ * ld + c] = v;
    M[c * ld + sJ] = v;
}

// column s <- row s
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_column(REAL *M, int64_t ld, int64_t s, int64_t n) {
    const int64_t c = (int64_t) blockIdx.x * VFT_EX_WG + threadIdx.x;
    if (c < n && c != s) M[c * ld + s] = M[s * ld + c];
}

// per-slot copies of what the criterion needs: the node id and its out-distance (which must be current)
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_prepare(Arena<REAL> A, const int64_t *nodeOf, int64_t n, int64_t nActive, REAL *slotOut,
                                                          int32_t *slotNode, unsigned int *stale) {
    const int64_t c = (int64_t) blockIdx.x * VFT_EX_WG + threadIdx.x;
    if (c >= n) return;
    const int64_t v = nodeOf[c];
    slotNode[c] = (int32_t) v;
    slotOut[c] = A.outDist[v];
    if ((int64_t) A.nOutActive[v] != nActive) atomicOr(stale, 1u);
}

template <typename REAL> struct ExVec4;
template <> struct ExVec4<float> { typedef float4 type; };
template <> struct ExVec4<double> { typedef double4 type; };

// the four pairs (r, c0 .. c0 + 3) of one lane: vft_criterion (setCriterion, NJ.tcc:1099-1107) with both stamps current
template <typename REAL>
__device__ __forceinline__ void vft_ex_eval(const typename ExVec4<REAL>::type &v, const typename ExVec4<REAL>::type &o, int64_t c0, int64_t r,
                                            int64_t n, double outR, int32_t nodeR, const int32_t *slotNode, double nm2, ExKey<REAL> &best) {
    const REAL d[4] = {v.x, v.y, v.z, v.w}, oc[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int64_t c = c0 + e;
        if (c <= r || c >= n) continue;
        const REAL crit = (REAL) ((double) d[e] - (outR + (double) oc[e]) / nm2);
        if (!(crit <= best.crit)) continue;
        const int32_t nodeC = slotNode[c];
        ExKey<REAL> k;
        k.crit = crit;
        k.dist = d[e];
        k.lo = nodeR < nodeC ? nodeR : nodeC;
        k.hi = nodeR < nodeC ? nodeC : nodeR;
        if (vft_ex_better<REAL>(k, best)) best = k;
    }
}

// Row r's columns beyond the diagonal in chunks of 256 (64 lanes x 4), of which this wavefront takes number `h` of every `H`, two
// chunks' loads in flight at a time.  (c0 and ld are multiples of 4: c0 < n implies c0 + 3 < ld.)
template <typename REAL>
__device__ __forceinline__ void vft_ex_row(const REAL *M, int64_t ld, int64_t n, int64_t r, int h, int H, const REAL *slotOut,
                                           const int32_t *slotNode, double nm2, ExKey<REAL> &best) {
    typedef typename ExVec4<REAL>::type V;
    const int lane = threadIdx.x & 63;
    const REAL *row = M + r * ld;
    const double outR = (double) slotOut[r];
    const int32_t nodeR = slotNode[r];
    const int64_t step = (int64_t) 256 * H;
    for (int64_t c0 = ((r + 1) & ~(int64_t) 255) + (int64_t) 256 * h + 4 * lane; c0 < n; c0 += 2 * step) {
        const int64_t c1 = c0 + step;
        const bool two = c1 < n;
        const V v0 = *(const V *) (row + c0), o0 = *(const V *) (slotOut + c0);
        const V v1 = *(const V *) (row + (two ? c1 : c0)), o1 = *(const V *) (slotOut + (two ? c1 : c0));
        vft_ex_eval<REAL>(v0, o0, c0, r, n, outR, nodeR, slotNode, nm2, best);
        if (two) vft_ex_eval<REAL>(v1, o1, c1, r, n, outR, nodeR, slotNode, nm2, best);
    }
}

// One pass over the upper triangle of the n live slots; part[blockIdx.x] = the workgroup's minimum.  Rows r and n-2-r are paired
// (together n columns, whatever r) and a pair is split H ways by chunks: item = pair * H + h, items dealt to the wavefronts in turn.
// Grid: at most VFT_EX_MAX_PARTS workgroups of four wavefronts.
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_search(const REAL *M, int64_t ld, int64_t n, int64_t nActive, int H, const REAL *slotOut,
                                                         const int32_t *slotNode, ExKey<REAL> *part) {
    const int64_t wave = (int64_t) blockIdx.x * (VFT_EX_WG / 64) + (threadIdx.x >> 6), nWaves = (int64_t) gridDim.x * (VFT_EX_WG / 64);
    const int64_t nItems = ((n - 2) / 2 + 1) * H;
    const double nm2 = (double) (nActive - 2);
    ExKey<REAL> best = vft_ex_none<REAL>();
    for (int64_t it = wave; it < nItems; it += nWaves) {
        const int64_t p = it / H;
        const int h = (int) (it % H);
        vft_ex_row<REAL>(M, ld, n, p, h, H, slotOut, slotNode, nm2, best);
        if (n - 2 - p != p) vft_ex_row<REAL>(M, ld, n, n - 2 - p, h, H, slotOut, slotNode, nm2, best);
    }
    best = vft_ex_block_min<REAL>(best);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

// the minimum of the partials -> the host-mapped record, then the completion flag; clears the stale word for the next search
template <typename REAL>
__global__ __launch_bounds__(VFT_EX_WG) void k_ex_finish(const ExKey<REAL> *part, int nPart, unsigned int *stale, ExBestOut *out,
                                                         unsigned long long *flag, unsigned long long seq) {
    ExKey<REAL> best = vft_ex_none<REAL>();
    for (int t = threadIdx.x; t < nPart; t += VFT_EX_WG)
        if (vft_ex_better<REAL>(part[t], best)) best = part[t];
    best = vft_ex_block_min<REAL>(best);
    if (threadIdx.x == 0) {
        out->dist = (double) best.dist;
        out->crit = (double) best.crit;
        out->i = best.lo == 0x7FFFFFFF ? -1 : best.lo;
        out->j = best.hi == 0x7FFFFFFF ? -1 : best.hi;
        out->stale = (int32_t) *stale;
        out->pad = 0;
        *stale = 0u;
    }
    vft_th_raise(flag, seq);
}
