// Multi-head SpMM over [E, H] values: the aggregation of an attention layer,
//   out[s, h, :] = sum over i in [ptr[s], ptr[s+1]) of value[p(i), h] * x[ind[i], h, :],   p(i) = perm ? perm[i] : i,
// x is [nsrc, H, D], out is [nseg, H, D]; value == NULL means all ones.  Sum only.  A row of out is W = H * D wide.
//
// The group-walk kernel of segtile.h.  The lanes cover the columns: a group of LPR lanes holds one 16-byte packet of
// the row per lane, and a row wider than LPR packets takes several column blocks (blockIdx.y).  The gathers of four
// entries are issued before the first of them is added.  The loop is wave-uniform, the groups differ only in
// predicates.
//
//   tile kernel   acc += value * x for every entry of the chunk.  At the last entry of a segment that began inside the
//                 chunk the accumulator row is written to out.  A record is an accumulator row of W elements (fp32,
//                 fp64 for double): records[chunk * W + column].
//   fix-up        one wave per chunk with a head record, lanes over the columns: the tail records of the chunks
//                 [ptr[s] / L, b) are added in chunk order (fp32 records fold in fp64), then the head record, and the
//                 row is written.
//
//   packet route    D * itemsize a multiple of 16 and x, out on a 16-byte boundary: VEC = 16 / itemsize.
//   generic route   every other D >= 1 or operands off the boundary: VEC = 1, a lane holds one element.
//
// Workspace: nchunks = ceil(E / L) chunks,
//   2 * align256(acc_size * nchunks * H * D)  head and tail records
// + 2 * align256(8 * nchunks)                 head and tail segment ids (-1: no record)
// (tsamd_spmm_heads_workspace_bytes).  L = 8 * LPR, so a chunk of rows narrower than 64 packets carries one accumulator
// packet of records per eight entries: 4 bytes per fp32 entry up to 256 columns, W / 64 bytes above.
//
// out is zeroed first, so rows without entries are zeros and out is fully defined on return.  An entry adds to the
// accumulator of its own segment only and the accumulator is cleared where a segment ends, so a non-finite product
// reaches the row that holds the entry and no neighbour of the chunk or the record.  fp32 accumulation (fp64 for
// double), one rounding on the store.  Fixed combine tree: the entries of a chunk in order, the records in chunk
// order -- two calls give the same bits.  No atomics, no host sync, three launches (memset, tile, fix-up).
#include "segtile.h"

#include <type_traits>

namespace tsamd {
namespace {

constexpr int kShBatch = 4;  // gathers in flight per lane

struct ShPlan {
  int generic;
  int vec;
  int lg_lpr;       // lanes per row
  int64_t blocks;   // column blocks
  int64_t chunk;    // entries per group
};

// Lanes per row, from the PACKET count of an aligned row also on the generic route: a misaligned call then only takes
// more column blocks, and the chunk length -- hence the workspace, whose query cannot see the pointers -- is a
// function of (dtype, H, D) alone.
int sh_lg_lpr(int dtype, int64_t H, int64_t D) {
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const int64_t W = H * D;
  const int64_t packets = W > 0 ? ceil_div(W, vec) : 1;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < packets) ++lg;
  return lg;
}

// the one place the route is decided: the driver and tsamd_spmm_heads_route both plan through it
ShPlan sh_plan(int dtype, int64_t H, int64_t D, const void *x, const void *out) {
  ShPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const bool packets = D > 0 && D % vec == 0 && aligned16(x) && aligned16(out);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  p.lg_lpr = sh_lg_lpr(dtype, H, D);
  const int64_t W = H * D;
  p.blocks = W > 0 ? ceil_div(ceil_div(W, (int64_t)p.vec), (int64_t)1 << p.lg_lpr) : 1;
  p.chunk = (int64_t)kSegWindows << p.lg_lpr;
  return p;
}

// head and tail records: an accumulator row each
SegRecords sh_records(size_t acc, int64_t chunk, int64_t W, int64_t E) {
  const size_t row = acc * (size_t)(W > 0 ? W : 1);
  return SegRecords(E, chunk, {row, row});
}

template <typename T, int VEC>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_heads_tile_kernel(
    const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind, const int64_t *__restrict__ perm,
    const T *__restrict__ value, const T *__restrict__ x, T *__restrict__ out,
    typename Traits<T>::acc_t *__restrict__ head_val, typename Traits<T>::acc_t *__restrict__ tail_val,
    int64_t *__restrict__ head_seg, int64_t *__restrict__ tail_seg, int64_t nseg, int64_t E, int64_t H, int64_t D,
    int lg_lpr) {
  using A = typename Traits<T>::acc_t;
  using P = Pack<T, VEC>;
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  const SegSlice slice = stage_slice(ptr, nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = e0 + (int64_t)wave * kSegChunk;
  if (w0 >= e1) return;  // such a wave has no chunk

  const GroupGeom geo = group_geom(lg_lpr, wave, lane, e1);
  const int lpr = geo.lpr;
  const int64_t chunk = geo.chunk, c0 = geo.c0;
  const int64_t W = H * D;
  const int64_t col0 = ((int64_t)blockIdx.y * lpr + geo.gl) * VEC;
  const bool colok = col0 < W;  // the packet route has W % VEC == 0: a packet is inside the row or outside
  const int64_t h = colok ? col0 / D : 0;
  const bool scribe = geo.gl == 0 && blockIdx.y == 0;  // writes the segment ids of the chunk's records

  A acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = A(0);
  bool open = false, had_head = false;
  int32_t cur = -1;  // segment of the last entry taken

  for (int w = 0; w < kSegWindows; ++w) {
    // one entry of the window per lane of the group
    const int64_t e = c0 + (int64_t)w * lpr + geo.gl;
    GroupEntry mine = {0, 0, 0};
    int64_t p_l = 0;
    if (e < geo.c1) {
      const SegEntry en = slice_entry(slice, ptr, sp, e);
      mine.seg = (int32_t)en.seg;
      mine.col = (uint32_t)ind[e];
      p_l = perm ? perm[e] : e;
      mine.fl = kSegValid | (e + 1 == en.end ? kSegEnd : 0) | (en.start >= c0 ? kSegFresh : 0);
    }
    for (int j0 = 0; j0 < lpr; j0 += kShBatch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kShBatch], sg[kShBatch];
      P xv[kShBatch];
      A vv[kShBatch];
#pragma unroll
      for (int u = 0; u < kShBatch; ++u) {
        const int j = j0 + u;
        const GroupEntry en = group_broadcast(geo, mine, j);
        fl[u] = en.fl;
        sg[u] = en.seg;
        const uint32_t c = en.col;
        int64_t p = c0 + (int64_t)w * lpr + j;
        if (perm) p = lane_read(p_l, group_src(geo, j));
        xv[u] = P();
        vv[u] = A(1);
        if ((fl[u] & kSegValid) && colok) {
          xv[u] = *reinterpret_cast<const P *>(x + (uint64_t)c * (uint64_t)W + (uint64_t)col0);
          if (value) vv[u] = Traits<T>::to_acc(value[p * H + h]);
        }
      }
#pragma unroll
      for (int u = 0; u < kShBatch; ++u) {
        if (fl[u] & kSegValid) {  // an entry beyond the chunk adds nothing: no 0 * Inf
          cur = sg[u];
          open = true;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += vv[u] * Traits<T>::to_acc(xv[u].v[v]);
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            if (colok) {
              P o;
#pragma unroll
              for (int v = 0; v < VEC; ++v) o.v[v] = Traits<T>::from_acc(acc[v]);
              *reinterpret_cast<P *>(out + (uint64_t)sg[u] * (uint64_t)W + (uint64_t)col0) = o;
            }
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (colok) {
#pragma unroll
              for (int v = 0; v < VEC; ++v) head_val[(uint64_t)chunk * (uint64_t)W + (uint64_t)col0 + v] = acc[v];
            }
            if (scribe) head_seg[chunk] = sg[u];
          }
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = A(0);
          open = false;
        }
      }
    }
  }
  if (c0 < e1) {
    if (open && colok) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) tail_val[(uint64_t)chunk * (uint64_t)W + (uint64_t)col0 + v] = acc[v];
    }
    group_record_ids(geo, scribe, open, had_head, cur, head_seg, tail_seg);
  }
}

template <typename T>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_heads_fixup_kernel(
    const int64_t *__restrict__ ptr, T *__restrict__ out, const typename Traits<T>::acc_t *__restrict__ head_val,
    const typename Traits<T>::acc_t *__restrict__ tail_val, const int64_t *__restrict__ head_seg, int64_t W,
    int64_t L, int64_t nchunks) {
  using A = typename Traits<T>::acc_t;
  using F = typename std::conditional<std::is_same<A, float>::value, double, A>::type;  // fp32 records fold in fp64
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (b >= nchunks) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  const int64_t first = ptr[s] / L;  // every chunk in [first, b) ended inside s: its tail record is a piece of s
  for (int64_t col = lane; col < W; col += kWave) {
    F sum = F(0);
    for (int64_t i = first; i < b; ++i) sum += (F)tail_val[(uint64_t)i * (uint64_t)W + (uint64_t)col];
    sum += (F)head_val[(uint64_t)b * (uint64_t)W + (uint64_t)col];
    out[(uint64_t)s * (uint64_t)W + (uint64_t)col] = Traits<T>::from_acc((A)sum);
  }
}

template <typename T>
int launch_spmm_heads(const ShPlan &p, const int64_t *ptr, const int64_t *ind, const int64_t *perm,
                      const void *value, const void *x, void *out, int64_t nseg, int64_t H, int64_t D, int64_t E,
                      void *workspace, hipStream_t stream) {
  using A = typename Traits<T>::acc_t;
  constexpr int kVec = 16 / (int)sizeof(T);
  const int64_t W = H * D;
  const SegRecords rec = sh_records(sizeof(A), p.chunk, W, E);
  const int64_t nchunks = (int64_t)rec.nchunks;
  A *head_val = rec.plane<A>(workspace, 0), *tail_val = rec.plane<A>(workspace, 1);
  int64_t *head_seg = rec.head_seg(workspace), *tail_seg = rec.tail_seg(workspace);
  const dim3 block(kSegWaves * kWave);
  const dim3 tiles((unsigned int)ceil_div(E, (int64_t)kExpandTile), (unsigned int)p.blocks);
  const T *vv = reinterpret_cast<const T *>(value), *xx = reinterpret_cast<const T *>(x);
  T *oo = reinterpret_cast<T *>(out);
  if (p.generic)
    hipLaunchKernelGGL((spmm_heads_tile_kernel<T, 1>), tiles, block, 0, stream, ptr, ind, perm, vv, xx, oo, head_val,
                       tail_val, head_seg, tail_seg, nseg, E, H, D, p.lg_lpr);
  else
    hipLaunchKernelGGL((spmm_heads_tile_kernel<T, kVec>), tiles, block, 0, stream, ptr, ind, perm, vv, xx, oo,
                       head_val, tail_val, head_seg, tail_seg, nseg, E, H, D, p.lg_lpr);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((spmm_heads_fixup_kernel<T>), dim3((unsigned int)ceil_div(nchunks, (int64_t)kSegWaves)), block, 0,
                     stream, ptr, oo, (const A *)head_val, (const A *)tail_val, (const int64_t *)head_seg, W, p.chunk,
                     nchunks);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// sizes the 32-bit ids and the grid can carry
bool sh_indexable(int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E) {
  if (!heads_indexable(nseg, nsrc, H, D, E)) return false;
  if (H * D > 65535 * (int64_t)kWave) return false;  // column blocks are blockIdx.y
  return ceil_div(E, (int64_t)kExpandTile) <= 2147483647;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_spmm_heads_route(int dtype, int64_t H, int64_t D, const void *x, const void *out,
                                      int64_t out_route[8]) {
  if (!out_route || H < 0 || D < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out_route[i] = 0;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (H > 0 && D > 2147483647 / H) return TSAMD_ERR_UNSUPPORTED;
  const ShPlan p = sh_plan(dtype, H, D, x, out);
  out_route[0] = p.generic;
  out_route[1] = p.vec;
  out_route[2] = (int64_t)1 << p.lg_lpr;
  out_route[3] = (int64_t)64 >> p.lg_lpr;
  out_route[4] = p.chunk;
  out_route[5] = kExpandTile;
  out_route[6] = kExpandTile;  // a tile stages its pointer slice when it meets at most this many segments
  out_route[7] = p.blocks;
  return TSAMD_OK;
}

extern "C" size_t tsamd_spmm_heads_workspace_bytes(int dtype, int64_t nseg, int64_t H, int64_t D, int64_t E) {
  (void)nseg;
  if (!is_float_dtype(dtype) || H < 0 || D < 0 || E < 0) return 0;
  if (H > 0 && D > 2147483647 / H) return 0;
  const int64_t chunk = (int64_t)kSegWindows << sh_lg_lpr(dtype, H, D);
  return sh_records(acc_size(dtype), chunk, H * D, E).bytes();
}

extern "C" int tsamd_spmm_heads(int dtype, const int64_t *ptr, const int64_t *ind, const int64_t *perm,
                                const void *value, const void *x, void *out, int64_t nseg, int64_t nsrc, int64_t H,
                                int64_t D, int64_t E, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (nseg < 0 || nsrc < 0 || H < 0 || D < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (!sh_indexable(nseg, nsrc, H, D, E)) return TSAMD_ERR_UNSUPPORTED;
  if (nseg * H * D == 0) return TSAMD_OK;  // out has no element
  if (!out) return TSAMD_ERR_INVALID;
  const size_t out_bytes = dtype_size(dtype) * (size_t)(nseg * H * D);
  if (E == 0) {
    TSAMD_HIP_TRY(hipMemsetAsync(out, 0, out_bytes, stream));
    return TSAMD_OK;
  }
  if (nsrc == 0 || !ptr || !ind || !x) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_spmm_heads_workspace_bytes(dtype, nseg, H, D, E))
    return TSAMD_ERR_WORKSPACE;
  TSAMD_HIP_TRY(hipMemsetAsync(out, 0, out_bytes, stream));  // rows without entries
  const ShPlan p = sh_plan(dtype, H, D, x, out);
  return TSAMD_DISPATCH_FLOAT(dtype, [&]() -> int {
    return launch_spmm_heads<scalar_t>(p, ptr, ind, perm, value, x, out, nseg, H, D, E, workspace, stream);
  });
}
