// Value gradients of C = A * B (CSR x CSR -> CSR, sum): include/tsamd.h "SpSpMM value gradients".
//
//   gA[e] = sum over p in row k of B      of vB[p] * gC[pos(i, colB[p])]     e = (i, k) of A
//   gB[p] = sum over e in column k of A   of vA[e] * gC[pos(row(e), j)]      p = (k, j) of B
//
// Both are one computation: a SEGMENT (an entry of A | an entry of B) owns a LIST (row k of B | column k of A)
// and every list element contributes  w[t] * gC[find(row, col)]  with one of (row, col) fixed per segment and
// the other read from the list.  One kernel family, templated on the side and the value type.
//
// Balanced by PRODUCTS on the tiling of segtile.h: ptr[S + 1] = exclusive scan of the list lengths
// (tsamd_spspmm_bw_plan) is the segmented order.  Beside the slice of ptr a tile stages, per staged segment, the start
// of its list and its fixed index (one binary search over the row pointers per SEGMENT, not per product).  The list
// arrays are read coalesced: lanes with consecutive products of one segment read consecutive list elements.
//
//   tile kernel   a lane loads (index, weight) of its list element, finds the entry of C by a binary search over the
//                 sorted row of C (64-bit compares: column ids go up to 2^32 - 3) and forms the term; the lane that
//                 holds a segment's last product writes the sum.  Pieces of segments that cross a wave's chunk go to
//                 LDS, where one thread links the four waves in order; what crosses the TILE becomes the tile's HEAD
//                 and TAIL record: two records per tile.
//   fix-up        one wave per tile with a head record folds the tail records of the tiles before it (fixed
//                 strides and butterfly; fp32 pieces fold in fp64) and writes the segment.
//
// Deterministic (fixed combine tree), no atomics.  The output is zeroed inside the call: segments with an
// empty list get 0, every other segment is written exactly once.  Workspace: two records per tile -- nothing
// proportional to the number of products beyond that.
//
// Routes (tsamd_spspmm_bw_route): a tile that intersects more than kExpandTile segments (long runs of segments
// with empty lists) does not stage; its lanes search the global arrays instead.
#include "scan.h"
#include "segtile.h"

namespace tsamd {
namespace {

// List length of segment s (the row of entry s of a CSR pattern is the last r with rowptr[r] <= s:
// segment_of).  SIDE 0: the list is row colA[s] of B.  SIDE 1: column (row of s in B) of A.
template <int SIDE>
__global__ __launch_bounds__(256) void spspmm_bw_len_kernel(const int64_t *__restrict__ segptr, int64_t nrows,
                                                            const int64_t *__restrict__ segind,
                                                            const int64_t *__restrict__ listptr, int64_t nseg,
                                                            int64_t *__restrict__ len) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nseg) return;
  if (s == nseg) {  // the scan runs over nseg + 1 entries
    len[s] = 0;
    return;
  }
  const int64_t x = SIDE == 0 ? segind[s] : segment_of(segptr, nrows, s);
  len[s] = listptr[x + 1] - listptr[x];
}

// stats[0] = bytes of workspace tsamd_spspmm_value_bw needs, stats[1] = P
__global__ void spspmm_bw_stats_kernel(const int64_t *__restrict__ total, int64_t acc_bytes,
                                       int64_t *__restrict__ stats) {
  const int64_t P = *total;
  const int64_t ntiles = ((P > 0 ? P : 1) + kExpandTile - 1) / kExpandTile;  // as bw_records counts them
  const int64_t per = (ntiles * acc_bytes + 255) / 256 * 256 + (ntiles * 8 + 255) / 256 * 256;
  stats[0] = 2 * per;
  stats[1] = P;
}

// position of (row, col) in C, or -1 (an operand pair whose product pattern is not inside C)
__device__ __forceinline__ int64_t find_in_row(const int64_t *__restrict__ rowptrC, const int64_t *__restrict__ colC,
                                               int64_t row, int64_t col) {
  int64_t lo = rowptrC[row];
  const int64_t end = rowptrC[row + 1];
  int64_t hi = end;
  while (lo < hi) {  // lower bound
    const int64_t mid = (lo + hi) >> 1;
    if (colC[mid] < col) lo = mid + 1; else hi = mid;
  }
  return (lo < end && colC[lo] == col) ? lo : -1;
}

template <typename T, int SIDE>
__global__ __launch_bounds__(kSegWaves *kWave) void spspmm_bw_tile_kernel(
    const int64_t *__restrict__ ptr, int64_t nseg, int64_t P, const int64_t *__restrict__ segptr, int64_t nrows,
    const int64_t *__restrict__ segind, const int64_t *__restrict__ listptr, const int64_t *__restrict__ list_ind,
    const T *__restrict__ list_val, const int64_t *__restrict__ rowptrC, const int64_t *__restrict__ colC,
    const T *__restrict__ gC, T *__restrict__ out, T *__restrict__ head_val, T *__restrict__ tail_val,
    int64_t *__restrict__ head_seg, int64_t *__restrict__ tail_seg) {
  __shared__ int64_t sp[kExpandTile + 1];   // ptr[lo ..]
  __shared__ int64_t sl[kExpandTile];       // start of the segment's list
  __shared__ uint32_t sf[kExpandTile];      // its fixed index: row of C (SIDE 0, < 2^31) | column of C (SIDE 1, < 2^32)
  __shared__ int64_t span[2];
  __shared__ int64_t wh_seg[kSegWaves], wt_seg[kSegWaves];
  __shared__ int32_t wh_in[kSegWaves];       // the head segment of the wave began inside this tile
  __shared__ T wh_val[kSegWaves], wt_val[kSegWaves];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < P ? e0 + kExpandTile : P;
  const SegSlice slice = slice_bounds(ptr, nseg, e0, e1, span);
  if (slice.staged) {
    for (int i = threadIdx.x; i <= (int)slice.S; i += blockDim.x) {
      const int64_t s = slice.lo + i;
      sp[i] = ptr[s];
      if (i < (int)slice.S) {
        const int64_t r = segment_of(segptr, nrows, s), c = segind[s];
        sl[i] = listptr[SIDE == 0 ? c : r];
        sf[i] = (uint32_t)(SIDE == 0 ? r : c);
      }
    }
  }
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (lane == 0) {
    wh_seg[wave] = wt_seg[wave] = -1;
    wh_in[wave] = 0;
    wh_val[wave] = wt_val[wave] = T(0);
  }
  __syncthreads();
  const int64_t c0 = e0 + (int64_t)wave * kSegChunk;
  const int64_t c1 = c0 + kSegChunk < e1 ? c0 + kSegChunk : e1;

  int64_t cseg = -1;  // wave-uniform carry: the segment still open at the end of the last window
  T cval = T(0);
  int64_t hseg = -1;  // the segment that began before this chunk and ends in it (set by at most one lane)
  T hval = T(0);
  int32_t hin = 0;
  for (int w = 0; w < kSegWindows; ++w) {
    const int64_t base = c0 + (int64_t)w * kWave;
    if (base >= c1) break;
    const int64_t t = base + lane;
    const bool valid = t < c1;
    int64_t seg = -2 - lane, sstart = 0, send = 0;  // invalid lanes never match a neighbour
    T v = T(0);
    if (valid) {
      int64_t lstart, fixed;
      if (slice.staged) {
        const int i = segment_of_lds(sp, (int)slice.S, t);
        seg = slice.lo + i;
        sstart = sp[i];
        send = sp[i + 1];
        lstart = sl[i];
        fixed = (int64_t)sf[i];
      } else {
        seg = slice.lo + segment_of(ptr + slice.lo, slice.S, t);
        sstart = ptr[seg];
        send = ptr[seg + 1];
        const int64_t r = segment_of(segptr, nrows, seg), c = segind[seg];
        lstart = listptr[SIDE == 0 ? c : r];
        fixed = SIDE == 0 ? r : c;
      }
      const int64_t q = lstart + (t - sstart);
      const int64_t x = list_ind[q];
      const T wgt = list_val ? list_val[q] : T(1);
      const int64_t pos = find_in_row(rowptrC, colC, SIDE == 0 ? fixed : x, SIDE == 0 ? x : fixed);
      if (pos >= 0) v = wgt * gC[pos];
    }
    // segmented inclusive scan: segments are contiguous runs, so "lane - off has my segment" implies every
    // lane in between has it too
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int src = lane >= off ? lane - off : lane;
      const T ov = lane_read(v, src);
      const int64_t os = lane_read(seg, src);
      if (lane >= off && os == seg) v = ov + v;
    }
    if (valid && seg == cseg) v = cval + v;
    const bool is_end = valid && t + 1 == send;
    if (is_end) {
      if (sstart >= c0) {
        out[seg] = v;
      } else {  // began before this chunk: linked below
        hseg = seg;
        hval = v;
        hin = sstart >= e0 ? 1 : 0;
      }
    }
    const int last = (int)((c1 - base < kWave ? c1 - base : kWave) - 1);  // wave-uniform
    const bool last_end = lane_read((int32_t)is_end, last) != 0;
    cseg = last_end ? -1 : lane_read(seg, last);
    cval = lane_read(v, last);
  }
  if (hseg != -1) {  // at most one lane of the wave
    wh_seg[wave] = hseg;
    wh_val[wave] = hval;
    wh_in[wave] = hin;
  }
  if (lane == 0 && c0 < e1) {
    wt_seg[wave] = cseg;
    wt_val[wave] = cval;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // link the waves in product order
    int64_t oseg = -1, ths = -1;
    T oval = T(0), thv = T(0);
    for (int w = 0; w < kSegWaves; ++w) {
      if (wh_seg[w] != -1) {
        const T v = oseg == wh_seg[w] ? oval + wh_val[w] : wh_val[w];
        if (wh_in[w]) {
          out[wh_seg[w]] = v;
        } else {
          ths = wh_seg[w];
          thv = v;
        }
        oseg = -1;
      }
      if (wt_seg[w] != -1) {
        if (oseg == wt_seg[w]) {  // the whole chunk lies inside the open segment
          oval = oval + wt_val[w];
        } else {
          oseg = wt_seg[w];
          oval = wt_val[w];
        }
      } else if (w * kSegChunk < e1 - e0) {
        oseg = -1;
      }
    }
    head_seg[blockIdx.x] = ths;
    head_val[blockIdx.x] = thv;
    tail_seg[blockIdx.x] = oseg;
    tail_val[blockIdx.x] = oval;
  }
}

template <typename T>
__global__ __launch_bounds__(kSegWaves *kWave) void spspmm_bw_fixup_kernel(
    T *__restrict__ out, const T *__restrict__ head_val, const T *__restrict__ tail_val,
    const int64_t *__restrict__ head_seg, const int64_t *__restrict__ tail_seg, int64_t ntiles) {
  // fp32 pieces of a long segment fold in fp64 (as the SpMM and segment-reduce fix-ups do)
  using W = double;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (b >= ntiles) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  int64_t run = 0;  // tiles b-1, b-2, ... whose open segment is s
  for (;;) {
    const int64_t idx = b - 1 - run - lane;
    const bool ok = idx >= 0 && tail_seg[idx] == s;
    const unsigned long long m = __ballot(ok);
    const int c = m == ~0ull ? 64 : (int)__builtin_ctzll(~m);
    run += c;
    if (c < 64) break;
  }
  W acc = W(0);
  for (int64_t i = lane; i < run; i += kWave) acc += (W)tail_val[b - 1 - i];
  for (int off = 32; off > 0; off >>= 1) acc += lane_xor(acc, off);
  if (lane == 0) out[s] = (T)(acc + (W)head_val[b]);
}

// two records per tile
SegRecords bw_records(size_t elem, int64_t P) { return SegRecords(P, kExpandTile, {elem, elem}); }

template <typename T, int SIDE>
int launch_bw(const int64_t *ptr, int64_t nseg, int64_t P, const int64_t *segptr, int64_t nrows,
              const int64_t *segind, const int64_t *listptr, const int64_t *list_ind, const void *list_val,
              const int64_t *rowptrC, const int64_t *colC, const void *gC, void *out, void *workspace,
              hipStream_t stream) {
  const SegRecords rec = bw_records(sizeof(T), P);
  const int64_t ntiles = (int64_t)rec.nchunks;
  T *head_val = rec.plane<T>(workspace, 0), *tail_val = rec.plane<T>(workspace, 1);
  int64_t *head_seg = rec.head_seg(workspace), *tail_seg = rec.tail_seg(workspace);
  hipLaunchKernelGGL((spspmm_bw_tile_kernel<T, SIDE>), dim3((unsigned int)ntiles), dim3(kSegWaves * kWave), 0, stream,
                     ptr, nseg, P, segptr, nrows, segind, listptr, list_ind, reinterpret_cast<const T *>(list_val),
                     rowptrC, colC, reinterpret_cast<const T *>(gC), reinterpret_cast<T *>(out), head_val, tail_val,
                     head_seg, tail_seg);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((spspmm_bw_fixup_kernel<T>), dim3((unsigned int)ceil_div(ntiles, (int64_t)kSegWaves)),
                     dim3(kSegWaves * kWave), 0, stream, reinterpret_cast<T *>(out), (const T *)head_val,
                     (const T *)tail_val, (const int64_t *)head_seg, (const int64_t *)tail_seg, ntiles);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_spspmm_bw_route(int dtype, int64_t out[8]) {
  if (!out) return TSAMD_ERR_INVALID;
  if (dtype != TSAMD_F32 && dtype != TSAMD_F64) return TSAMD_ERR_UNSUPPORTED;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = kExpandTile;  // products per tile
  out[1] = kExpandTile;  // a tile that intersects more segments than this searches global memory
  out[2] = kSegChunk;     // products per wave (pieces are linked in LDS across the waves of a tile)
  out[3] = 2;            // carry records per tile
  return TSAMD_OK;
}

extern "C" size_t tsamd_spspmm_bw_plan_workspace_bytes(int64_t nseg) {
  return scan_workspace_bytes((nseg > 0 ? nseg : 0) + 1);
}

extern "C" size_t tsamd_spspmm_bw_workspace_bytes(int dtype, int64_t P) {
  return bw_records(dtype == TSAMD_F64 ? 8 : 4, P).bytes();
}

extern "C" int tsamd_spspmm_bw_plan(int dtype, int side, const int64_t *segptr, int64_t nrows,
                                    const int64_t *segind, int64_t nseg, const int64_t *listptr, int64_t *ptr,
                                    int64_t *stats, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (dtype != TSAMD_F32 && dtype != TSAMD_F64) return TSAMD_ERR_UNSUPPORTED;
  if (side != 0 && side != 1) return TSAMD_ERR_INVALID;
  if (nrows < 0 || nseg < 0 || !ptr || !stats) return TSAMD_ERR_INVALID;
  if (nseg > 0 && (!segptr || !segind || !listptr)) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_spspmm_bw_plan_workspace_bytes(nseg)) return TSAMD_ERR_WORKSPACE;
  const unsigned int grid = (unsigned int)ceil_div(nseg + 1, (int64_t)256);
  if (side == 0)
    hipLaunchKernelGGL(spspmm_bw_len_kernel<0>, dim3(grid), dim3(256), 0, stream, segptr, nrows, segind, listptr,
                       nseg, ptr);
  else
    hipLaunchKernelGGL(spspmm_bw_len_kernel<1>, dim3(grid), dim3(256), 0, stream, segptr, nrows, segind, listptr,
                       nseg, ptr);
  TSAMD_LAUNCH_CHECK();
  int64_t *total = stats + 1;  // overwritten with P by the stats kernel (same value)
  const int st = exclusive_scan_i64(ptr, ptr, nseg + 1, total, workspace, stream);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(spspmm_bw_stats_kernel, dim3(1), dim3(1), 0, stream, (const int64_t *)total,
                     (int64_t)(dtype == TSAMD_F64 ? 8 : 4), stats);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_spspmm_value_bw(int dtype, int side, const int64_t *ptr, int64_t P, const int64_t *segptr,
                                     int64_t nrows, const int64_t *segind, int64_t nseg, const int64_t *listptr,
                                     const int64_t *list_ind, const void *list_val, const int64_t *rowptrC,
                                     const int64_t *colC, const void *gC, void *grad, void *workspace,
                                     size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (dtype != TSAMD_F32 && dtype != TSAMD_F64) return TSAMD_ERR_UNSUPPORTED;
  if (side != 0 && side != 1) return TSAMD_ERR_INVALID;
  if (nrows < 0 || nseg < 0 || P < 0) return TSAMD_ERR_INVALID;
  if (nseg == 0) return TSAMD_OK;
  if (!grad) return TSAMD_ERR_INVALID;
  const size_t elem = dtype == TSAMD_F64 ? 8 : 4;
  TSAMD_HIP_TRY(hipMemsetAsync(grad, 0, elem * (size_t)nseg, stream));  // segments with an empty list
  if (P == 0) return TSAMD_OK;
  if (!ptr || !segptr || !segind || !listptr || !list_ind || !rowptrC || !colC || !gC) return TSAMD_ERR_INVALID;
  if (ceil_div(P, (int64_t)kExpandTile) >= ((int64_t)1 << 31)) return TSAMD_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < bw_records(elem, P).bytes()) return TSAMD_ERR_WORKSPACE;
  if (dtype == TSAMD_F32) {
    if (side == 0)
      return launch_bw<float, 0>(ptr, nseg, P, segptr, nrows, segind, listptr, list_ind, list_val, rowptrC, colC,
                                 gC, grad, workspace, stream);
    return launch_bw<float, 1>(ptr, nseg, P, segptr, nrows, segind, listptr, list_ind, list_val, rowptrC, colC, gC,
                               grad, workspace, stream);
  }
  if (side == 0)
    return launch_bw<double, 0>(ptr, nseg, P, segptr, nrows, segind, listptr, list_ind, list_val, rowptrC, colC, gC,
                                grad, workspace, stream);
  return launch_bw<double, 1>(ptr, nseg, P, segptr, nrows, segind, listptr, list_ind, list_val, rowptrC, colC, gC,
                              grad, workspace, stream);
}
