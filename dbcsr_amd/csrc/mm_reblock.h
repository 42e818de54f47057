// mm_reblock.h -- a matrix under another block structure, without leaving the device and without leaving the block-sparse form:
// dbcsr_amd_bcsr_reblock_name_blocks (reblock_count_pieces, reblock_name_pieces) and dbcsr_amd_bcsr_reblock_gather (reblock_gather).  Part of the
// device-resident multiply engine: included by mm_engine.hip after mm_csr.h, whose search in running sums (csr_block_of) it takes over unchanged.
//
// The reference library has this capability in dbcsr_complete_redistribute (a copy between matrices of different blockings: CP2K goes from atomic to
// molecular or clustered blocks with it) and, for tensors, in dbcsr_t_split_blocks; their sources could not be consulted here, so the two rules below
// are the semantics of this library.
//
// A is a matrix without symmetry, (rs', cs') a second block structure with the same sums of sizes.
//   pattern  a new block (I, J) is stored iff its element rectangle intersects the rectangle of at least one block that A's index names.  Values play
//            no part: a stored block full of zeros counts, the holes of an unpacked data area are never read.
//   values   an element of a stored new block is the element of A at the same (row, column), bit for bit, where A's index names a block there
//            (-0.0, NaN, +-Inf included), and +0.0 elsewhere.
// Blocks are column by column on both sides: element (p, q) of an mb x nb block is blk[p + q mb].
//   name     a source block (R, C) covers the new block rows I0 ... I1 and the new block columns J0 ... J1, found by binary searches in the running sums
//            of the new sizes: it names (I1 - I0 + 1)(J1 - J0 + 1) pieces.  reblock_count_pieces leaves per source block the count, I0, J0 and the
//            column span; ONE exclusive scan in 64 bits gives every block the place of its first piece; reblock_name_pieces takes a piece per thread
//            (its block by a binary search in the scanned places) and stores (I, J) -- consecutive threads write consecutive entries.  The list holds a
//            new block once per source block that meets it: dbcsr_amd_bcsr_reserve_count takes duplicates.
//   gather   one workgroup per (new block, every T-th tile of at most 32 x 32 elements of it).  Per tile the workgroup first builds a lookup table in
//            LDS: every wave finds the source block row of each of the tile's rows and the source block column of each of its columns (lane l < 32
//            row l, lane 32 + l column l: 64 binary searches in the running sums of the source sizes, side by side), numbers the distinct ones with
//            a ballot (slots: at most 32 x 32, source blocks of one element), and the workgroup looks every (row slot, column slot) up in the source
//            index -- ONE binary search in that source row's col_i each -- for the block's data offset or "absent", and expands that once per tile
//            to where every column of the tile begins inside the source block of every row slot.  Then the move: both sides are column-major with
//            the same orientation, so nothing is staged and nothing transposed; lanes run along element rows, which are contiguous on both sides
//            as far as a source block reaches; the written side is walked by mm_block_walk.h (16-byte stores aligned on the new block, element-wise
//            heads and tails); a moving lane reads two entries of the table per element and never searches.  A new block of up to 32 rows is
//            written as whole runs of columns by the workgroup, a taller one column piece by column piece, as many lanes each as the piece has
//            16-byte packs.
// Every element of every block the new index names is written exactly once, nothing else.  No atomics, no scratch, no memset; elements are loaded and
// stored, never computed with; every offset into a data area is formed in 64 bits; the same bits on every call.
#ifndef DBCSR_AMD_MM_REBLOCK_H
#define DBCSR_AMD_MM_REBLOCK_H
#include "mm_csr.h"

namespace dbcsr_amd {

constexpr int kReblockTile = 32;   // rows and columns of a tile: the lookup table has kReblockTile^2 entries

// The lookup table of a tile, all of the kernel's LDS.  off: the data offset of the source block at (row slot, column slot) or -1 -- what the searches
// give.  base: per (row slot, column of the tile) the offset of that column's first element inside the source block there, or -1 -- off expanded once
// per tile so that the moving lanes add a row and nothing else.  Per row of the tile its slot and its place inside the source block (one 8-byte entry),
// per column the same, per slot the source block row / column, and per row slot the rows of its source blocks (their leading dimension)
struct ReblockTable {
  int64_t off[kReblockTile * kReblockTile];
  int64_t base[kReblockTile * kReblockTile];
  int2 row[kReblockTile], col[kReblockTile];   // (.x the slot, .y the place inside the source block)
  int slot_row[kReblockTile], slot_col[kReblockTile], slot_ld[kReblockTile];
};

// ---- the pieces of the source blocks --------------------------------------------------------------------------------------------------------------------
// cnt[b] = the pieces of source block b (saturated: the host refuses a total of 2^31 - 1 or more), first[3 b ...] = I0, J0 and the column span.  One wave
// per source block row: its span of new block rows is searched once per lane, a lane per block searches the span of new block columns.
__global__ void __launch_bounds__(256) reblock_count_pieces(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ roff,
                                                            const int64_t* __restrict__ coff, int nbr, int nbc, const int64_t* __restrict__ nroff,
                                                            const int64_t* __restrict__ ncoff, int nnbr, int nnbc, int64_t nblks,
                                                            int* __restrict__ cnt, int* __restrict__ first) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= nbr) return;
  const int R = (int)w;
  const int64_t r0 = roff[R], r1 = roff[R + 1];
  const int I0 = r1 > r0 ? csr_block_of(nroff, nnbr, r0) : -1, I1 = r1 > r0 ? csr_block_of(nroff, nnbr, r1 - 1) : -1;
  for (int64_t b = (int64_t)row_p[R] + lane; b < row_p[R + 1] && b < nblks; b += 64) {
    const int Cb = col_i[b];
    int J0 = -1, J1 = -1;
    if ((unsigned)Cb < (unsigned)nbc) {
      const int64_t c0 = coff[Cb], c1 = coff[Cb + 1];
      if (c1 > c0) J0 = csr_block_of(ncoff, nnbc, c0), J1 = csr_block_of(ncoff, nnbc, c1 - 1);
    }
    const bool some = I0 >= 0 && I1 >= I0 && J0 >= 0 && J1 >= J0;   // (a block of no element, or one outside the new structure: no piece)
    const int64_t n = some ? (int64_t)(I1 - I0 + 1) * (int64_t)(J1 - J0 + 1) : 0;
    cnt[b] = n > 0x7fffffff ? 0x7fffffff : (int)n;
    first[3 * b] = I0, first[3 * b + 1] = J0, first[3 * b + 2] = some ? J1 - J0 + 1 : 0;
  }
}

// rows[t], cols[t] <- the new block of piece t, t < min(pos[nblks], cap).  A thread per piece.
__global__ void __launch_bounds__(256) reblock_name_pieces(const int64_t* __restrict__ pos, const int* __restrict__ first, int64_t nblks, int64_t cap,
                                                           int32_t* __restrict__ rows, int32_t* __restrict__ cols) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cap || t >= pos[nblks]) return;
  int64_t lo = 0, hi = nblks;   // pos[lo] <= t < pos[hi]; blocks without a piece are passed over
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] <= t) lo = mid;
    else hi = mid;
  }
  const int span = first[3 * lo + 2];
  const int64_t k = t - pos[lo];
  const int i = span > 0 ? (int)(k / span) : 0;
  rows[t] = first[3 * lo] + i;
  cols[t] = first[3 * lo + 1] + (int)(k - (int64_t)i * span);
}

// ---- the move ---------------------------------------------------------------------------------------------------------------------------------------------
// the block row of block b: the last R with row_p[R] <= b (block rows without blocks are passed over)
__device__ __forceinline__ int reblock_row_of(const int* __restrict__ row_p, int nbr, int b) {
  int lo = 0, hi = nbr;   // row_p[lo] <= b < row_p[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (row_p[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// element (p, q) of the tile by the table: the source element, or +0.0 where the source stores no block
template <typename T>
__device__ __forceinline__ T reblock_at(const ReblockTable& tab, const T* __restrict__ src, int p, int q) {
  const int2 r = tab.row[p];
  const int64_t at = tab.base[r.x * kReblockTile + q];
  return at < 0 ? dense_zero<T>() : src[at + (int64_t)r.y];
}

// Every element of every block the new index (d_*) names <- the element of the source (s_*) at its (row, column), +0.0 where the source names no block;
// nothing else of the new data area is written.  One workgroup per (new block, every T-th tile of it).
template <typename T>
__global__ void __launch_bounds__(256) reblock_gather(const int* __restrict__ s_row_p, const int* __restrict__ s_col_i, const int64_t* __restrict__ s_blk_p,
                                                      const T* __restrict__ src, const int* __restrict__ s_rs, const int* __restrict__ s_cs,
                                                      const int64_t* __restrict__ s_roff, const int64_t* __restrict__ s_coff, int s_nbr, int s_nbc,
                                                      const int* __restrict__ d_row_p, const int* __restrict__ d_col_i, const int64_t* __restrict__ d_blk_p,
                                                      T* __restrict__ dst, const int* __restrict__ d_rs, const int* __restrict__ d_cs,
                                                      const int64_t* __restrict__ d_roff, const int64_t* __restrict__ d_coff, int d_nbr, int d_nbc,
                                                      int64_t d_nblks, int tiles_split, int vec_ok) {
  __shared__ ReblockTable tab;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t b = (int64_t)(blockIdx.x / (unsigned)tiles_split);
  const int sub = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles_split);
  if (b >= d_nblks || b >= d_row_p[d_nbr]) return;
  const int I = reblock_row_of(d_row_p, d_nbr, (int)b), J = d_col_i[b];
  if ((unsigned)J >= (unsigned)d_nbc) return;
  const int M = d_rs[I], N = d_cs[J];
  if (M <= 0 || N <= 0) return;
  const int64_t doff = d_blk_p[b], gr = d_roff[I], gc = d_coff[J];
  const int ntp = (M + kReblockTile - 1) / kReblockTile, ntq = (N + kReblockTile - 1) / kReblockTile;
  for (int t = sub; t < ntp * ntq; t += tiles_split) {
    const int tqi = t / ntp, tpi = t - tqi * ntp;
    const int p0 = tpi * kReblockTile, q0 = tqi * kReblockTile;
    const int tp = min(kReblockTile, M - p0), tq = min(kReblockTile, N - q0);
    // 1. the source block row of every row of the tile (lanes 0 ... 31) and the source block column of every column (lanes 32 ... 63), numbered by a
    //    ballot over the places where another one begins: every wave does the same, wave 0 writes the table
    const int l = lane & 31, side = lane >> 5;
    const bool in = l < (side ? tq : tp);
    const int64_t x = side ? gc + q0 + l : gr + p0 + l;
    const int blk = in ? csr_block_of(side ? s_coff : s_roff, side ? s_nbc : s_nbr, x) : -1;
    const int before = __shfl_up(blk, 1, 64);
    const bool begins = in && (l == 0 || before != blk);
    const unsigned long long all = __ballot(begins);
    const unsigned mine = side ? (unsigned)(all >> 32) : (unsigned)all;
    const int nR = __popc((unsigned)all), nC = __popc((unsigned)(all >> 32));
    const int slot = __popc(mine & (0xffffffffu >> (31 - l))) - 1;   // (the begins at or below l, less one)
    if (tid < 64 && in) {
      const int64_t x0 = blk >= 0 ? (side ? s_coff : s_roff)[blk] : x;
      if (side) {
        tab.col[l] = make_int2(slot, (int)(x - x0));
        if (begins) tab.slot_col[slot] = blk;
      } else {
        tab.row[l] = make_int2(slot, (int)(x - x0));
        if (begins) tab.slot_row[slot] = blk, tab.slot_ld[slot] = blk >= 0 ? s_rs[blk] : 0;
      }
    }
    __syncthreads();
    // 2. the data offset of the source block at every (row slot, column slot), or "absent": one binary search in the source row's col_i each
    for (int k = tid; k < nR * nC; k += 256) {
      const int sr = k / nC, sc = k - sr * nC;
      const int R = tab.slot_row[sr], Cb = tab.slot_col[sc];
      const int at = R >= 0 && Cb >= 0 ? dense_find(s_row_p, s_col_i, R, Cb) : -1;
      tab.off[sr * kReblockTile + sc] = at >= 0 ? s_blk_p[at] : -1;
    }
    __syncthreads();
    // ... expanded per column of the tile: where that column begins inside the source block of every row slot
    for (int k = tid; k < nR * tq; k += 256) {
      const int sr = k / tq, q = k - sr * tq;
      const int2 c = tab.col[q];
      const int64_t o = tab.off[sr * kReblockTile + c.x];
      tab.base[sr * kReblockTile + q] = o < 0 ? -1 : o + (int64_t)c.y * (int64_t)tab.slot_ld[sr];
    }
    __syncthreads();
    // 3. the move, along the written side's runs
    if (M <= kReblockTile) {   // (p0 = 0, tp = M: the tile's columns are one run of the new block)
      const int64_t run = (int64_t)q0 * M;
      T* out = dst + doff + run;
      walk_block<T>(
          doff + run, M * tq, tid, 256, vec_ok,
          [&](int e) {
            const int q = e / M;
            out[e] = reblock_at<T>(tab, src, e - q * M, q);
          },
          [&](int e) {
            Pack16<T> v;
            int q = e / M, p = e - q * M;   // (a pack may run on into the next column)
#pragma unroll
            for (int u = 0; u < Pack16<T>::V; ++u) {
              v.v[u] = reblock_at<T>(tab, src, p, q);
              if (++p == M) p = 0, ++q;
            }
            *reinterpret_cast<Pack16<T>*>(out + e) = v;
          });
    } else {   // a column piece of up to 32 rows per group of L lanes: as many lanes as the piece has packs
      constexpr int L = kReblockTile / Pack16<T>::V;
      for (int q = tid / L; q < tq; q += 256 / L) {
        const int64_t run = (int64_t)(q0 + q) * M + p0;
        T* out = dst + doff + run;
        walk_block<T>(
            doff + run, tp, tid % L, L, vec_ok, [&](int e) { out[e] = reblock_at<T>(tab, src, e, q); },
            [&](int e) {
              Pack16<T> v;
#pragma unroll
              for (int u = 0; u < Pack16<T>::V; ++u) v.v[u] = reblock_at<T>(tab, src, e + u, q);
              *reinterpret_cast<Pack16<T>*>(out + e) = v;
            });
      }
    }
    __syncthreads();
  }
}

}  // namespace dbcsr_amd
#endif
