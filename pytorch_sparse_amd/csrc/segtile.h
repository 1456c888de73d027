// Entry-balanced segmented kernels: the tiling shared by segreduce.hip, softmax.hip, spmm_heads.hip, attention.hip
// and spspmm_bw.hip (sddmm.hip only shares the host helpers of common.h).  Stated once, here.
//
//   tile      a workgroup owns kExpandTile = 2048 consecutive ENTRIES of a segmented order (ptr[nseg + 1]), whatever
//             the segment lengths.  It finds the segments [lo, lo + S) that meet the tile (expand.h: tile_span) and,
//             when S <= 2048, STAGES ptr[lo .. lo + S] in LDS; a lane then finds the segment of an entry by a binary
//             search in LDS, else (long runs of empty segments) in global memory: slice_entry, the same answer.
//   chunk     the run of entries one accumulator walks.  Scan kernels (segreduce, softmax, spspmm_bw): a wave's
//             kSegChunk = 512 entries, as kSegWindows = 8 WINDOWS of 64 (a lane per entry); the segmented window scan,
//             its carry and the head-record capture are written out in each of the three (segreduce.hip has the
//             commented original): as shared templates they did not compile to the same code
//             (profiles/segtile_codegen.md).  Group-walk kernels (spmm_heads, attention): a group of LPR lanes (LPR a
//             power of two, G = 64 / LPR groups per wave) walks L = 8 * LPR entries, as 8 windows of LPR entries read
//             a lane per entry and handed round the group.  spspmm_bw.hip links its four waves in LDS: its chunk is
//             the tile.
//   records   a segment that lies inside one chunk is finished by the tile kernel.  A segment cut by a chunk boundary
//             leaves pieces: the piece that ENDS in a chunk (the segment began before it) is the chunk's HEAD record,
//             the piece still open at the chunk's end its TAIL record; head_seg / tail_seg hold the segment id, -1
//             for no record.  A chunk has at most one of each.  The fix-up launch, one wave per chunk b with a head
//             record of segment s, folds the tail records of the chunks before b that lie in s -- [ptr[s] / L, b), or
//             a counted run where chunks are no fixed length of entries (spspmm_bw.hip) -- and then the head record.
//             softmax.hip leaves that total as the chunk's FINAL record for its third launch.
//   order     every combine takes the EARLIER piece as its first operand: the scan (lane - off before lane), the carry
//             (carry before window), the fix-up (tail records in chunk order, then the head record).  The ordered
//             min / max of segreduce.hip depends on it; the sums and the online softmax do not, they are written the
//             same way.  Nothing is atomic and every tree is fixed: two calls give the same bits.
//   zeroing   the tile kernel writes head_seg and tail_seg of EVERY chunk that has entries (-1 without a record), so
//             the workspace needs no clearing; value planes are read only where an id says so.  Outputs of segments
//             without entries are set by the entry point before the tile kernel (memset / fill launch).
//
// Online softmax: the state (m, l) of a piece is its maximum and the sum of exp(x - m).  Two pieces are rescaled to
// the larger maximum by soft_scale, with exp(-inf - x) taken as 0 also for x = -inf; the final l is soft_final_l.
// SmForward::combine (softmax.hip) keeps its two-armed `a.s + b.s * f` / `a.s * f + b.s`: the form l * fa + l2 * fb
// contracts to another fused multiply-add and rounds differently.  SmForward::finish keeps its own test `m == +inf`:
// under soft_final_l a NaN maximum would replace the NaN sum by the canonical NaN, other bits in the result.
#pragma once

#include "expand.h"

#include <initializer_list>

namespace tsamd {

constexpr int kSegWindows = 8;
constexpr int kSegChunk = kWave * kSegWindows;      // entries per wave
constexpr int kSegWaves = kExpandTile / kSegChunk;  // waves per workgroup (4)
static_assert(kSegWaves * kSegChunk == kExpandTile, "tile = waves x chunk");

// ---- slice ---------------------------------------------------------------------------------------------------------
struct SegSlice {
  int64_t lo, S;  // the segments [lo, lo + S) meet the tile
  bool staged;    // sp[0 .. S] = ptr[lo .. lo + S]
};

struct SegEntry {
  int64_t seg, start, end;  // the segment of an entry and its entries [start, end)
  int i;                    // seg - lo on a staged slice, else 0
};

// Block-wide: the slice of the tile [e0, e1).  `span` is 2 int64 of LDS; contains a __syncthreads().
__device__ __forceinline__ SegSlice slice_bounds(const int64_t *__restrict__ ptr, int64_t nseg, int64_t e0, int64_t e1,
                                                 int64_t *span) {
  int64_t lo, hi;
  tile_span(ptr, nseg, e0, e1, span, &lo, &hi);
  return {lo, hi - lo + 1, hi - lo + 1 <= kExpandTile};
}

// Block-wide: bounds, copy and the barrier behind it.  sp is kExpandTile + 1 int64 of LDS.  (spspmm_bw.hip fills two
// side arrays in its copy loop, before its one barrier, and takes slice_bounds alone.)
__device__ __forceinline__ SegSlice stage_slice(const int64_t *__restrict__ ptr, int64_t nseg, int64_t e0, int64_t e1,
                                                int64_t *sp, int64_t *span) {
  const SegSlice sl = slice_bounds(ptr, nseg, e0, e1, span);
  if (sl.staged) {
    for (int i = threadIdx.x; i <= (int)sl.S; i += blockDim.x) sp[i] = ptr[sl.lo + i];
    __syncthreads();
  }
  return sl;
}

__device__ __forceinline__ SegEntry slice_entry(const SegSlice &sl, const int64_t *__restrict__ ptr, const int64_t *sp,
                                                int64_t e) {
  SegEntry r;
  if (sl.staged) {
    r.i = segment_of_lds(sp, (int)sl.S, e);
    r.seg = sl.lo + r.i;
    r.start = sp[r.i];
    r.end = sp[r.i + 1];
  } else {
    r.i = 0;
    r.seg = sl.lo + segment_of(ptr + sl.lo, sl.S, e);
    r.start = ptr[r.seg];
    r.end = ptr[r.seg + 1];
  }
  return r;
}

// ---- group walk ----------------------------------------------------------------------------------------------------
constexpr int kSegValid = 1, kSegEnd = 2, kSegFresh = 4;  // an entry; the last of its segment; which began in the chunk

struct GroupGeom {
  int lg_lpr, lpr;  // lanes per group
  int g, gl;        // group of the wave, lane of the group
  int64_t L;        // entries per chunk
  int64_t chunk, c0, c1;  // the group's chunk and its entries; c0 >= e1: a group without a chunk (chunk >= nchunks)
};

__device__ __forceinline__ GroupGeom group_geom(int lg_lpr, int wave, int lane, int64_t e1) {
  GroupGeom q;
  q.lg_lpr = lg_lpr;
  q.lpr = 1 << lg_lpr;
  q.g = lane >> lg_lpr;
  q.gl = lane & (q.lpr - 1);
  q.L = (int64_t)kSegWindows << lg_lpr;
  q.chunk = (((int64_t)blockIdx.x * kSegWaves + wave) << (6 - lg_lpr)) + q.g;
  q.c0 = q.chunk * q.L;
  q.c1 = q.c0 + q.L < e1 ? q.c0 + q.L : e1;
  return q;
}

struct GroupEntry {
  int32_t fl, seg;  // kSeg* flags (0: no entry), segment
  uint32_t col;     // ind[e]
};

// the lane of this wave that read entry j of the group's window
__device__ __forceinline__ int group_src(const GroupGeom &q, int j) { return (q.g << q.lg_lpr) + (j < q.lpr ? j : 0); }

// entry j of the window, to every lane of the group; j >= LPR: no entry.  Wave-uniform j: every lane answers.
__device__ __forceinline__ GroupEntry group_broadcast(const GroupGeom &q, const GroupEntry &mine, int j) {
  const int src = group_src(q, j);
  GroupEntry r;
  r.fl = lane_read(mine.fl, src);
  if (j >= q.lpr) r.fl = 0;
  r.seg = lane_read(mine.seg, src);
  r.col = lane_read(mine.col, src);
  return r;
}

// after the last window: the ids of the chunk's records (the head id of a chunk with a head record was written
// where the segment ended)
__device__ __forceinline__ void group_record_ids(const GroupGeom &q, bool scribe, bool open, bool had_head,
                                                 int32_t cur, int64_t *__restrict__ head_seg,
                                                 int64_t *__restrict__ tail_seg) {
  if (scribe) {
    tail_seg[q.chunk] = open ? (int64_t)cur : -1;
    if (!had_head) head_seg[q.chunk] = -1;
  }
}

// ---- records -------------------------------------------------------------------------------------------------------
// The record workspace of a call: value planes of bytes_per_chunk x nchunks, each rounded up to 256 bytes, then the
// head and tail segment ids.  The size query and the launcher both read the layout from here.
struct SegRecords {
  static constexpr int kMaxPlanes = 4;
  size_t nchunks;
  int n;
  size_t off[kMaxPlanes + 3];  // value planes, head ids, tail ids, end

  SegRecords(int64_t entries, int64_t chunk, std::initializer_list<size_t> bytes_per_chunk) {
    nchunks = (size_t)ceil_div(entries > 0 ? entries : 1, chunk);
    n = 0;
    size_t at = 0;
    for (size_t b : bytes_per_chunk) {
      off[n++] = at;
      at += align_up(b * nchunks, 256);
    }
    off[n] = at;
    off[n + 1] = at + align_up(sizeof(int64_t) * nchunks, 256);
    off[n + 2] = at + 2 * align_up(sizeof(int64_t) * nchunks, 256);
  }
  size_t bytes() const { return off[n + 2]; }
  template <typename V>
  V *plane(void *workspace, int i) const {
    return reinterpret_cast<V *>(reinterpret_cast<char *>(workspace) + off[i]);
  }
  int64_t *head_seg(void *workspace) const { return plane<int64_t>(workspace, n); }
  int64_t *tail_seg(void *workspace) const { return plane<int64_t>(workspace, n + 1); }
};

// ---- online softmax ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float soft_exp(float x) { return __expf(x); }
__device__ __forceinline__ double soft_exp(double x) { return exp(x); }

template <typename A>
struct SoftScale {
  bool first;  // the state holds the larger maximum; false when either is NaN: f is NaN then, and so is every sum
  A mhi, f;    // the larger maximum, exp(smaller - larger)
  __device__ __forceinline__ A f_state() const { return first ? A(1) : f; }
  __device__ __forceinline__ A f_entry() const { return first ? f : A(1); }
};

// (m, .) (+) (m2, .): the common maximum and the weights of the two pieces
template <typename A>
__device__ __forceinline__ SoftScale<A> soft_scale(A m, A m2) {
  SoftScale<A> r;
  r.first = m >= m2;
  r.mhi = r.first ? m : m2;
  const A mlo = r.first ? m2 : m;
  r.f = mlo == -std::numeric_limits<A>::infinity() ? A(0) : soft_exp(mlo - r.mhi);
  return r;
}

// l of the final expression: m = +inf (torch's sum holds exp(inf - inf) = NaN) or NaN makes the row NaN
template <typename A>
__device__ __forceinline__ A soft_final_l(A m, A l) {
  return m < std::numeric_limits<A>::infinity() ? l : std::numeric_limits<A>::quiet_NaN();
}

}  // namespace tsamd
