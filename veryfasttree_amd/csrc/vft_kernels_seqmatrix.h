// `-makematrix`: the log-corrected distance of every ordered pair of input sequences (printDistances, NJ.tcc:274-288).
//
// For each pair (i, j), codes1 = i: seqDist on the leaf CODES (NJ.tcc:1601-1624; never profiles), the narrowing to numeric_t
// of Besthit::dist, logCorrect in double with libm's log (NJ.tcc:322-330) narrowed again, and the `dist <= 0 ? 0 : dist` of
// the print (NJ.tcc:284) - the value whose "%f" the reference writes.  n^2 x L column comparisons without joins, ordering
// or state.
//
// Decomposition (both kernels): grid (ceil(n / 64) column tiles, ceil((r1 - r0) / 64) row blocks), a workgroup of four
// wavefronts.  A lane owns ONE column sequence j = 64 * blockIdx.x + lane: its 16-byte chunks come from leafT (vft_layout.h),
// where the 64 lanes of a tile are contiguous - one coalesced 1 KiB load per chunk and wavefront.  A wavefront carries
// VFT_SM_ROWS row sequences i; their chunks have wave-uniform addresses and arrive as scalar loads (the shape of
// k_leaf_block, vft_kernels_nj.h), so 16 bytes of j per lane serve 16 pairs.  Rows beyond r1 are clamped to r0 and not
// stored; the lanes j >= n of the last tile read the tile's padding (allocated, "all gaps") and store nothing.
// out[(i - r0) * ld + j]: j runs along the lanes, so every store instruction writes one contiguous run of a row.
//
//   k_seqmatrix_nt   no distance matrix: integer nUse / nSame per pair from two AND + popcount groups per chunk
//                    (vft_seq_counts), order-free.  top = nUse - nSame.
//   k_seqmatrix_aa   distance matrix: the 20 x 20 `distances` table sits in LDS as numeric_t; the lane walks the columns IN
//                    ORDER and adds distances[c_i][c_j] into a double (seqDist's `top`, NJ.tcc:1614-1619).  c_i is
//                    wave-uniform (a scalar byte extract), so one
//                    lookup touches at most 20 addresses of one table row.  Raw codes are 0..19 and 127; the padding columns
//                    of the last chunk hold 127 on both sides.
//
// The epilogue runs in the lane.  The logarithm is glibc's, restated bit for bit (vft_glibc_log.h): its argument lies in
// (0.0133, 1] (Jukes-Cantor, dist < 0.74) or (0.01, 1] (scoredist, dist < 0.99) - positive and normal.
#pragma once
#include "vft_kernels_nj.h"
#include "vft_glibc_log.h"

#define VFT_SM_WG 256
#define VFT_SM_ROWS 16   // row sequences per wavefront; 4 wavefronts = 64 rows per workgroup

// steps 2-4 of a pair: top / nUse narrowed, log-corrected and narrowed, -0 and negatives to 0
template <typename REAL>
__device__ __forceinline__ REAL vft_sm_finish(double top, int nUse, bool logCorrect, bool scoredist) {
    REAL dist = (REAL) (nUse > 0 ? top / (double) nUse : 1.0);
    if (logCorrect) {   // NJ.tcc:322-330
        const double maxscore = 3.0;
        double d = (double) dist;
        if (!scoredist) d = d < 0.74 ? -0.75 * vft_glibc_log(1.0 - d * 4.0 / 3.0) : maxscore;
        else d = d < 0.99 ? -1.3 * vft_glibc_log(1.0 - d) : maxscore;
        dist = (REAL) (d < maxscore ? d : maxscore);
    }
    return dist <= (REAL) 0 ? (REAL) 0 : dist;
}

// the wave-uniform chunk `c` of leaf `i` (scalar load)
__device__ __forceinline__ uint4 vft_sm_row_chunk(const uint4 *rowT, int c) {
    typedef const __attribute__((address_space(4))) vft_u4_t *sp_t;
    const vft_u4_t q = *(sp_t) (rowT + (int64_t) c * VFT_TILE);
    uint4 v;
    v.x = q.x; v.y = q.y; v.z = q.z; v.w = q.w;
    return v;
}

template <typename REAL>
__global__ __launch_bounds__(VFT_SM_WG) void k_seqmatrix_nt(const uint4 *leafT, VftDims d, int64_t r0, int64_t r1, int32_t logCorrect,
                                                             REAL *out, int64_t ld) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int64_t j = (int64_t) blockIdx.x * 64 + lane;   // blockIdx.x < ceil(nSeqs / 64): the tile exists
    const int64_t i0 = r0 + (int64_t) blockIdx.y * 64 + (int64_t) wave * VFT_SM_ROWS;
    if (i0 >= r1) return;   // wave-uniform
    const uint4 *colT = leafT + vft_leaf_idx(d, (int64_t) blockIdx.x, 0, lane);
    const uint4 *rowT[VFT_SM_ROWS];
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) {
        const int64_t i = i0 + u < r1 ? i0 + u : r0;
        rowT[u] = leafT + vft_leaf_idx(d, i >> 6, 0, (int) (i & 63));
    }
    int nUse[VFT_SM_ROWS], nSame[VFT_SM_ROWS];
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) nUse[u] = nSame[u] = 0;
    const int nChunk = d.nChunk;
    for (int c = 0; c < nChunk; c++) {
        const uint4 vj = colT[(int64_t) c * VFT_TILE];
#pragma unroll
        for (int u = 0; u < VFT_SM_ROWS; u++) vft_seq_counts(vft_sm_row_chunk(rowT[u], c), vj, nUse[u], nSame[u]);
    }
    if (j >= d.nSeqs) return;
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) {
        if (i0 + u >= r1) break;
        out[(i0 + u - r0) * ld + j] = vft_sm_finish<REAL>((double) (nUse[u] - nSame[u]), nUse[u], logCorrect != 0, false);
    }
}

#define VFT_SM_LD 21   // row stride of the table in LDS: row and column 20 are zeros, where a gap (127) is sent

template <typename REAL>
__global__ __launch_bounds__(VFT_SM_WG) void k_seqmatrix_aa(const uint4 *leafT, VftDims d, const REAL *distances, int64_t r0, int64_t r1,
                                                             int32_t logCorrect, REAL *out, int64_t ld) {
    // distances[a][b] at a * 21 + b; a gap on either side reads +0.0, which leaves the running double as it is
    __shared__ REAL sDist[VFT_SM_LD * VFT_SM_LD];
    for (int t = threadIdx.x; t < VFT_SM_LD * VFT_SM_LD; t += VFT_SM_WG) {
        const int a = t / VFT_SM_LD, b = t % VFT_SM_LD;
        sDist[t] = a < 20 && b < 20 ? distances[a * 20 + b] : (REAL) 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int64_t j = (int64_t) blockIdx.x * 64 + lane;
    const int64_t i0 = r0 + (int64_t) blockIdx.y * 64 + (int64_t) wave * VFT_SM_ROWS;
    if (i0 >= r1) return;   // wave-uniform, after the only barrier
    const uint4 *colT = leafT + vft_leaf_idx(d, (int64_t) blockIdx.x, 0, lane);
    const uint4 *rowT[VFT_SM_ROWS];
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) {
        const int64_t i = i0 + u < r1 ? i0 + u : r0;
        rowT[u] = leafT + vft_leaf_idx(d, i >> 6, 0, (int) (i & 63));
    }
    double top[VFT_SM_ROWS];
    int nUse[VFT_SM_ROWS];
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) {
        top[u] = 0.0;
        nUse[u] = 0;
    }
    const int nChunk = d.nChunk;
    for (int c = 0; c < nChunk; c++) {
        const uint4 vj = colT[(int64_t) c * VFT_TILE];
        const uint32_t wj[4] = {vj.x, vj.y, vj.z, vj.w};
        uint32_t cj[VFT_CHUNK];   // the lane's 16 codes, a gap as 20
#pragma unroll
        for (int b = 0; b < VFT_CHUNK; b++) {
            const uint32_t x = (wj[b >> 2] >> ((b & 3) * 8)) & 0xFFu;
            cj[b] = x < 20u ? x : 20u;
        }
#pragma unroll
        for (int u = 0; u < VFT_SM_ROWS; u++) {
            const uint4 vi = vft_sm_row_chunk(rowT[u], c);   // wave-uniform
            const uint32_t wi[4] = {vi.x, vi.y, vi.z, vi.w};
            // codes are 0..19 or 127: bit 6 of a byte says "gap"
            nUse[u] += __popc(~(wi[0] | wj[0]) & 0x40404040u) + __popc(~(wi[1] | wj[1]) & 0x40404040u) +
                       __popc(~(wi[2] | wj[2]) & 0x40404040u) + __popc(~(wi[3] | wj[3]) & 0x40404040u);
#pragma unroll
            for (int b = 0; b < VFT_CHUNK; b++) {   // the columns of the chunk, in order
                const uint32_t x = (wi[b >> 2] >> ((b & 3) * 8)) & 0xFFu;
                const uint32_t ci = x < 20u ? x : 20u;
                top[u] += (double) sDist[ci * VFT_SM_LD + cj[b]];
            }
        }
    }
    if (j >= d.nSeqs) return;
#pragma unroll
    for (int u = 0; u < VFT_SM_ROWS; u++) {
        if (i0 + u >= r1) break;
        out[(i0 + u - r0) * ld + j] = vft_sm_finish<REAL>(top[u], nUse[u], logCorrect != 0, true);
    }
}
