// Multi-head SpMM over [E, H] values: the aggregation of an attention layer,
//   out[s, h, :] = sum over i in [ptr[s], ptr[s+1]) of value[p(i), h] * x[ind[i], h, :],   p(i) = perm ? perm[i] : i,
// x is [nsrc, H, D], out is [nseg, H, D]; value == NULL means all ones.  Sum only.  A row of out is W = H * D wide.
//
// The ENTRIES are split evenly, with the tiling of segreduce.hip / softmax.hip: a workgroup owns a tile of 2048
// consecutive entries and stages the pointer slice that meets them in LDS (expand.h), a wave owns 512 of them.  The
// lanes cover the columns: a group of LPR lanes (a power of two) holds one 16-byte packet of the row per lane, so a
// wave holds G = 64 / LPR groups, and a row wider than LPR packets takes several column blocks (blockIdx.y).  Each
// group walks a CHUNK of L = 512 / G = 8 * LPR consecutive entries of the wave, one after the other, in 8 windows of
// LPR entries: a window's ids, segments and flags are read once (a lane per entry) and handed round the group by
// lane reads; the gathers of four entries are issued before the first of them is added.  The loop is wave-uniform,
// the groups differ only in predicates.
//
//   tile kernel   acc += value * x for every entry of the chunk.  At the last entry of a segment the accumulator row
//                 is written to out -- unless the segment began before the chunk: that piece becomes the chunk's
//                 HEAD record.  A segment still open at the end of the chunk leaves the TAIL record.  A record is an
//                 accumulator row of W elements (fp32, fp64 for double): records[chunk * W + column].
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
#include "common.h"
#include "expand.h"

#include <type_traits>

namespace tsamd {
namespace {

constexpr int kShWaves = 4;
constexpr int kShWaveEntries = kExpandTile / kShWaves;  // 512
constexpr int kShWindows = 8;                           // windows of LPR entries per chunk
constexpr int kShBatch = 4;                             // gathers in flight per lane
static_assert(kShWaveEntries == kWave * kShWindows, "a chunk is 8 windows of the group's lanes");

constexpr int kShValid = 1, kShEnd = 2, kShFresh = 4;

struct ShPlan {
  int generic;
  int vec;
  int lg_lpr;       // lanes per row
  int64_t blocks;   // column blocks
  int64_t chunk;    // entries per group
};

bool sh_float_dtype(int dtype) {
  return dtype == TSAMD_F32 || dtype == TSAMD_F64 || dtype == TSAMD_F16 || dtype == TSAMD_BF16;
}

bool sh_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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
  const bool packets = D > 0 && D % vec == 0 && sh_aligned16(x) && sh_aligned16(out);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  p.lg_lpr = sh_lg_lpr(dtype, H, D);
  const int64_t W = H * D;
  p.blocks = W > 0 ? ceil_div(ceil_div(W, (int64_t)p.vec), (int64_t)1 << p.lg_lpr) : 1;
  p.chunk = (int64_t)kShWindows << p.lg_lpr;
  return p;
}

template <typename A>
size_t sh_workspace_bytes(int64_t chunk, int64_t W, int64_t E) {
  const size_t nchunks = (size_t)ceil_div(E > 0 ? E : 1, chunk);
  const size_t w = (size_t)(W > 0 ? W : 1);
  return 2 * align_up(sizeof(A) * nchunks * w, 256) + 2 * align_up(sizeof(int64_t) * nchunks, 256);
}

template <typename T, int VEC>
__global__ __launch_bounds__(kShWaves *kWave) void spmm_heads_tile_kernel(
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
  int64_t lo, hi;
  tile_span(ptr, nseg, e0, e1, span, &lo, &hi);
  const int64_t S = hi - lo + 1;
  const bool staged = S <= kExpandTile;
  if (staged) {
    for (int i = threadIdx.x; i <= (int)S; i += blockDim.x) sp[i] = ptr[lo + i];
    __syncthreads();
  }
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = e0 + (int64_t)wave * kShWaveEntries;
  if (w0 >= e1) return;  // such a wave has no chunk

  const int lpr = 1 << lg_lpr;
  const int lg_g = 6 - lg_lpr;
  const int g = lane >> lg_lpr;
  const int kl = lane & (lpr - 1);
  const int64_t L = (int64_t)kShWindows << lg_lpr;
  const int64_t chunk = (((int64_t)blockIdx.x * kShWaves + wave) << lg_g) + g;
  const int64_t c0 = chunk * L;
  const int64_t c1 = c0 + L < e1 ? c0 + L : e1;  // c0 >= e1: a group without a chunk (chunk >= nchunks)
  const int64_t W = H * D;
  const int64_t col0 = ((int64_t)blockIdx.y * lpr + kl) * VEC;
  const bool colok = col0 < W;  // the packet route has W % VEC == 0: a packet is inside the row or outside
  const int64_t h = colok ? col0 / D : 0;
  const bool scribe = kl == 0 && blockIdx.y == 0;  // writes the segment ids of the chunk's records

  A acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = A(0);
  bool open = false, had_head = false;
  int32_t cur = -1;  // segment of the last entry taken

  for (int w = 0; w < kShWindows; ++w) {
    // one entry of the window per lane of the group
    const int64_t e = c0 + (int64_t)w * lpr + kl;
    int32_t fl_l = 0, seg_l = 0;
    uint32_t c_l = 0;
    int64_t p_l = 0;
    if (e < c1) {
      int64_t seg, sstart, send;
      if (staged) {
        const int i = segment_of_lds(sp, (int)S, e);
        seg = lo + i;
        sstart = sp[i];
        send = sp[i + 1];
      } else {
        seg = lo + segment_of(ptr + lo, S, e);
        sstart = ptr[seg];
        send = ptr[seg + 1];
      }
      seg_l = (int32_t)seg;
      c_l = (uint32_t)ind[e];
      p_l = perm ? perm[e] : e;
      fl_l = kShValid | (e + 1 == send ? kShEnd : 0) | (sstart >= c0 ? kShFresh : 0);
    }
    for (int j0 = 0; j0 < lpr; j0 += kShBatch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kShBatch], sg[kShBatch];
      P xv[kShBatch];
      A vv[kShBatch];
#pragma unroll
      for (int u = 0; u < kShBatch; ++u) {
        const int j = j0 + u;
        const int src = (g << lg_lpr) + (j < lpr ? j : 0);
        fl[u] = lane_read(fl_l, src);
        if (j >= lpr) fl[u] = 0;
        sg[u] = lane_read(seg_l, src);
        const uint32_t c = lane_read(c_l, src);
        int64_t p = c0 + (int64_t)w * lpr + j;
        if (perm) p = lane_read(p_l, src);
        xv[u] = P();
        vv[u] = A(1);
        if ((fl[u] & kShValid) && colok) {
          xv[u] = *reinterpret_cast<const P *>(x + (uint64_t)c * (uint64_t)W + (uint64_t)col0);
          if (value) vv[u] = Traits<T>::to_acc(value[p * H + h]);
        }
      }
#pragma unroll
      for (int u = 0; u < kShBatch; ++u) {
        if (fl[u] & kShValid) {  // an entry beyond the chunk adds nothing: no 0 * Inf
          cur = sg[u];
          open = true;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += vv[u] * Traits<T>::to_acc(xv[u].v[v]);
        }
        if (fl[u] & kShEnd) {
          if (fl[u] & kShFresh) {
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
    if (scribe) {
      tail_seg[chunk] = open ? (int64_t)cur : -1;
      if (!had_head) head_seg[chunk] = -1;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kShWaves *kWave) void spmm_heads_fixup_kernel(
    const int64_t *__restrict__ ptr, T *__restrict__ out, const typename Traits<T>::acc_t *__restrict__ head_val,
    const typename Traits<T>::acc_t *__restrict__ tail_val, const int64_t *__restrict__ head_seg, int64_t W,
    int64_t L, int64_t nchunks) {
  using A = typename Traits<T>::acc_t;
  using F = typename std::conditional<std::is_same<A, float>::value, double, A>::type;  // fp32 records fold in fp64
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kShWaves + (threadIdx.x >> 6);
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
  const int64_t nchunks = ceil_div(E, p.chunk);
  const size_t rec = align_up(sizeof(A) * (size_t)(nchunks * W), 256);
  char *wp = reinterpret_cast<char *>(workspace);
  A *head_val = reinterpret_cast<A *>(wp);
  A *tail_val = reinterpret_cast<A *>(wp + rec);
  int64_t *head_seg = reinterpret_cast<int64_t *>(wp + 2 * rec);
  int64_t *tail_seg = head_seg + align_up(sizeof(int64_t) * (size_t)nchunks, 256) / sizeof(int64_t);
  const dim3 block(kShWaves * kWave);
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
  hipLaunchKernelGGL((spmm_heads_fixup_kernel<T>), dim3((unsigned int)ceil_div(nchunks, (int64_t)kShWaves)), block, 0,
                     stream, ptr, oo, (const A *)head_val, (const A *)tail_val, (const int64_t *)head_seg, W, p.chunk,
                     nchunks);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// sizes the 32-bit ids and the grid can carry
bool sh_indexable(int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E) {
  const int64_t lim = 2147483647;
  if (nseg > lim || nsrc > lim || H > lim || D > lim) return false;
  if (H > 0 && D > lim / H) return false;                                  // W = H * D
  if (H > 0 && E > (int64_t)9223372036854775807LL / 16 / H) return false;  // byte offsets into value
  if (H * D > 65535 * (int64_t)kWave) return false;                        // column blocks are blockIdx.y
  return ceil_div(E, (int64_t)kExpandTile) <= lim;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_spmm_heads_route(int dtype, int64_t H, int64_t D, const void *x, const void *out,
                                      int64_t out_route[8]) {
  if (!out_route || H < 0 || D < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out_route[i] = 0;
  if (!sh_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
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
  if (!sh_float_dtype(dtype) || H < 0 || D < 0 || E < 0) return 0;
  if (H > 0 && D > 2147483647 / H) return 0;
  const int64_t chunk = (int64_t)kShWindows << sh_lg_lpr(dtype, H, D);
  return dtype == TSAMD_F64 ? sh_workspace_bytes<double>(chunk, H * D, E) : sh_workspace_bytes<float>(chunk, H * D, E);
}

extern "C" int tsamd_spmm_heads(int dtype, const int64_t *ptr, const int64_t *ind, const int64_t *perm,
                                const void *value, const void *x, void *out, int64_t nseg, int64_t nsrc, int64_t H,
                                int64_t D, int64_t E, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (nseg < 0 || nsrc < 0 || H < 0 || D < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (!sh_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
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
  switch (dtype) {
    case TSAMD_F32:
      return launch_spmm_heads<float>(p, ptr, ind, perm, value, x, out, nseg, H, D, E, workspace, stream);
    case TSAMD_F64:
      return launch_spmm_heads<double>(p, ptr, ind, perm, value, x, out, nseg, H, D, E, workspace, stream);
    case TSAMD_F16:
      return launch_spmm_heads<f16_t>(p, ptr, ind, perm, value, x, out, nseg, H, D, E, workspace, stream);
    default:
      return launch_spmm_heads<bf16_t>(p, ptr, ind, perm, value, x, out, nseg, H, D, E, workspace, stream);
  }
}
