// Fused GATv2 attention over a sparse pattern.  For an entry e of row r with column c, and head h,
//   z[e, h, d] = x_dst[r, h, d] + x_src[c, h, d],    s[e, h] = sum_d att[h, d] * leaky_relu(z[e, h, d]),
//   out[r, h, :] = sum_e softmax_e(s(., h)) * x_src[c, h, :],    lse[r, h] = log sum_e exp(s[e, h]),
// x_dst [M, H, D], x_src [N, H, D], att [H, D], out [M, H, D], lse [M, H] (fp32).  The gathered row x_src[c] is the
// score operand AND the value: one gather per entry, and nothing of size E * D exists in either direction.
//
// Forward: the group-walk kernel of segtile.h with LPR = LPH * HPP lanes per group.
//   lanes   LPH lanes (a power of two) cover the D features of one head, VEC = 16 / itemsize adjacent features per
//           lane; HPP heads (a power of two) sit side by side in the group.  H > HPP takes ceil(H / HPP) column blocks
//           (blockIdx.y) of whole heads.  D <= 64 * VEC: a head never leaves its group of lanes.
//   regs    a lane holds its part of att[h, :] (loaded once per group) and of x_dst[row, h, :] (reloaded where the
//           segment changes), both as fp32.
//   score   the x_src packets of kGvBatch = 4 entries are issued before the first is used.  z is ONE fp32 add of the two
//           loaded elements, so its sign is the sign of the exact sum; the lane's part of the score is the sum of
//           att * leaky(z) over its VEC features, reduced by a xor butterfly whose masks stay below LPH.  Features
//           beyond D read as zero in all three operands and add an exact zero.
//   online  per group and head (m, l, acc[VEC]) through soft_scale / soft_final_l of segtile.h; the packet that gave
//           the score is the packet folded into acc.  There is no second gather.
//   rows    a segment that began inside the chunk is finished where it ends: acc / l to out, m + log(l) to lse.  A
//           segment cut by a chunk edge leaves head / tail records, (m, l) per head and the accumulator row; the fix-up
//           launch (a wave per chunk with a head record) folds the tail records of the chunks [rowptr[s] / L, b) in
//           chunk order, then the head record.
//   fill    out is zeroed and lse set to -inf first: rows without entries.
// Three launches, no atomics, no host sync, a fixed combine order: two calls give the same bits.  Non-finite scores
// follow the per-row, per-head rules at the top of attention.hip.
//
//   packet route    D * itemsize a multiple of 16 and every [., H, D] operand on a 16-byte boundary.
//   generic route   every other 1 <= D <= 64 * VEC or an operand off the boundary: the same lane map, element loads.
// att is always read by element loads.  Lane map, chunk and workspace are a function of (dtype, H, D) alone.
//
// Backward, entry kernel (tsamd_gatv2_attention_bw): a wave owns 64 consecutive entries, LPH lanes per head, heads and
// entries side by side.  It recomputes s from the two rows, forms dp = <g[r, h], x_src[c, h]> and delta = <g[r, h],
// out[r, h]> in the same butterfly and stores p = e(s - lse[r, h]) and ds = p * (dp - delta) as [E, H] fp32.  lse not
// finite: NaN both; s = -inf: 0 both.  delta is taken from the UNROUNDED out: the forward's out for float32, and for
// bfloat16 the fp32 copy out_acc that the forward writes beside out when asked to.  The bfloat16 rounding of out, times
// att, is larger than a gradient whose terms cancel (a row that one entry dominates).
//
// Backward, segment kernel (tsamd_gatv2_grad): the group walk again, over a segmented order (ptr, ind, perm) with u
// indexed by segment and w gathered by id:
//   out[s, h, :] = sum_e ds[perm(e), h] * att[h, :] * (u[s, h, :] + w[ind[e], h, :] > 0 ? 1 : slope).
// z is symmetric in its operands: (rowptr, col, none; u = x_dst, w = x_src) gives grad_x_dst, (colptr, row, csr2csc;
// u = x_src, w = x_dst) the score part of grad_x_src.  VALUE also gathers g[ind[e], h, :] and adds p[perm(e), h] * g:
// grad_x_src is complete after one walk.  ATT also sums ds * leaky(z) per lane over the whole chunk and writes one
// partial [H, D] row per chunk; a fold kernel adds the partials in chunk order (16 slices of consecutive chunks, then
// the slices in order) with fp32 accumulators.  Cut segments leave head / tail records of plain sums for one fix-up
// launch; segments without entries are zero-filled.  No atomics.
//
// Workspace: nchunks = ceil(E / L), W = H * D; the larger of
//   forward   2 * align256(4 * nchunks * W) + 2 * align256(8 * nchunks * H) + 2 * align256(8 * nchunks)
//   grad      3 * align256(4 * nchunks * W) + 2 * align256(8 * nchunks)
#include "segtile.h"

#include <cmath>

namespace tsamd {
namespace {

constexpr int kGvWaves = kSegWaves;
constexpr int kGvBatch = 4;      // entries whose gathers are in flight
constexpr int kGvBwHeads = 16;   // heads side by side in the entry kernel (H above takes passes)
constexpr int kGvFoldSlices = 16;
constexpr int kGvValue = 1, kGvAtt = 2;  // flags of tsamd_gatv2_grad

struct GvPlan {
  int generic;
  int vec;         // elements per load
  int lg_lph;      // lanes per head
  int lg_hpp;      // heads side by side
  int64_t blocks;  // column blocks = ceil(H / HPP)
  int64_t chunk;   // entries per group
  size_t workspace;
};

enum GvKind { kGvForward, kGvEntry, kGvSegment };

// one call: what the three entry points fill in
struct GvCall {
  int dtype, kind, flags;
  const int64_t *row, *ptr, *ind, *perm;  // row: entry kernel only, may be null; perm: segment kernel only, may be null
  const void *xa, *xb;                    // the operand of the segments and the gathered one: x_dst, x_src or u, w
  const void *att;
  double slope;
  void *out, *lse;  // lse: written by the forward, read by the entry kernel
  const void *grad_out;
  float *p, *ds;    // written by the entry kernel, read by the segment kernel
  float *out_acc;   // [nseg, H, D] fp32: the unrounded out; written by the forward (may be null), read by the entry kernel
  void *grad_att;
  int64_t nseg, nsrc, H, D, E;
  void *workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};
constexpr int kGvProceed = -1;

bool gv_dtype_ok(int dtype) { return dtype == TSAMD_F32 || dtype == TSAMD_BF16; }

SegRecords gv_fw_records(int64_t chunk, int64_t H, int64_t D, int64_t E) {
  const size_t h = (size_t)(H > 0 ? H : 1), w = h * (size_t)(D > 0 ? D : 1);
  return SegRecords(E, chunk, {4 * w, 4 * w, 8 * h, 8 * h});
}
SegRecords gv_grad_records(int64_t chunk, int64_t H, int64_t D, int64_t E) {
  const size_t w = (size_t)(H > 0 ? H : 1) * (size_t)(D > 0 ? D : 1);
  return SegRecords(E, chunk, {4 * w, 4 * w, 4 * w});
}

// the one place the plan is made; dtype is float32 or bfloat16 and 0 <= D <= 64 * vec
GvPlan gv_plan(int dtype, int64_t H, int64_t D, int64_t E, const void *a, const void *b, const void *c,
               const void *d = nullptr) {
  GvPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const bool packets = D > 0 && D % vec == 0 && aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  p.lg_lph = lg_ceil(D > 0 ? ceil_div(D, vec) : 1);
  p.lg_hpp = lg_ceil(H > 0 ? H : 1);
  if (p.lg_hpp > 6 - p.lg_lph) p.lg_hpp = 6 - p.lg_lph;
  p.blocks = ceil_div(H > 0 ? H : 1, (int64_t)1 << p.lg_hpp);
  p.chunk = (int64_t)kSegWindows << (p.lg_lph + p.lg_hpp);
  const size_t fw = gv_fw_records(p.chunk, H, D, E).bytes(), gr = gv_grad_records(p.chunk, H, D, E).bytes();
  p.workspace = fw > gr ? fw : gr;
  return p;
}

__device__ __forceinline__ float gv_leaky(float z, float slope) { return z > 0.f ? z : z * slope; }

// VEC adjacent features of a head row, from feature d0: one 16-byte load, or element loads that read zero beyond D
template <typename T, bool PACKED>
__device__ __forceinline__ Pack<T, 16 / (int)sizeof(T)> gv_load(const T *__restrict__ head_row, int64_t d0,
                                                                  int64_t D) {
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  if constexpr (PACKED) {
    return *reinterpret_cast<const P *>(head_row + d0);
  } else {
    P r = P();
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (d0 + v < D) r.v[v] = head_row[d0 + v];
    return r;
  }
}

template <typename T, bool PACKED>
__device__ __forceinline__ void gv_store(T *__restrict__ head_row, int64_t d0, int64_t D, const float *x) {
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  if constexpr (PACKED) {
    P o;
#pragma unroll
    for (int v = 0; v < VEC; ++v) o.v[v] = Traits<T>::from_acc(x[v]);
    *reinterpret_cast<P *>(head_row + d0) = o;
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (d0 + v < D) head_row[d0 + v] = Traits<T>::from_acc(x[v]);
  }
}

// out = 0 and, where lse is given, lse = -inf.  out is cleared in 16-byte units of its enclosing aligned range, the
// two ragged ends by bytes.
__global__ __launch_bounds__(256) void gatv2_fill_kernel(unsigned char *__restrict__ out, int64_t out_bytes,
                                                          float *__restrict__ lse, int64_t nlse) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uintptr_t begin = reinterpret_cast<uintptr_t>(out), end = begin + (uintptr_t)out_bytes;
  const uintptr_t unit = (begin & ~(uintptr_t)15) + (uintptr_t)i * 16;
  if (unit < end) {
    if (unit >= begin && unit + 16 <= end) {
      *reinterpret_cast<uint4 *>(unit) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (uintptr_t b = unit < begin ? begin : unit; b < unit + 16 && b < end; ++b)
        *reinterpret_cast<unsigned char *>(b) = 0;
    }
  }
  if (i < nlse) lse[i] = -std::numeric_limits<float>::infinity();
}

// what a lane knows of its place: the same in the forward and the segment kernel
struct GvLane {
  int lph, kl;
  int64_t h, d0, hoff;
  bool hok, colok, scribe, clerk;
};

__device__ __forceinline__ GvLane gv_lane(const GroupGeom &geo, int lg_lph, int lg_hpp, int64_t H, int64_t D,
                                          int vec) {
  GvLane q;
  q.lph = 1 << lg_lph;
  q.kl = geo.gl & (q.lph - 1);
  q.h = ((int64_t)blockIdx.y << lg_hpp) + (geo.gl >> lg_lph);
  q.hok = q.h < H;
  q.d0 = (int64_t)q.kl * vec;
  q.colok = q.hok && q.d0 < D;  // the packet route has D % VEC == 0: a packet is inside the head or outside
  q.hoff = q.hok ? q.h * D : 0;
  q.scribe = geo.gl == 0 && blockIdx.y == 0;  // writes the segment ids of the chunk's records
  q.clerk = q.hok && q.kl == 0;               // writes (m, l) and lse of its head
  return q;
}

// this lane's entry of window w
__device__ __forceinline__ GroupEntry gv_window(const GroupGeom &geo, const SegSlice &slice,
                                                const int64_t *__restrict__ ptr, const int64_t *sp,
                                                const int64_t *__restrict__ ind, int w, int64_t *e_out) {
  const int64_t e = geo.c0 + (int64_t)w * geo.lpr + geo.gl;
  GroupEntry mine = {0, 0, 0};
  if (e < geo.c1) {
    const SegEntry en = slice_entry(slice, ptr, sp, e);
    mine.seg = (int32_t)en.seg;
    mine.col = (uint32_t)ind[e];
    mine.fl = kSegValid | (e + 1 == en.end ? kSegEnd : 0) | (en.start >= geo.c0 ? kSegFresh : 0);
  }
  *e_out = e;
  return mine;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T, bool PACKED>
__global__ __launch_bounds__(kGvWaves *kWave) void gatv2_tile_kernel(
    const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind, const T *__restrict__ xd,
    const T *__restrict__ xs, const T *__restrict__ att, float slope, T *__restrict__ out, float *__restrict__ out_acc,
    float *__restrict__ lse, float *__restrict__ head_acc, float *__restrict__ tail_acc, float *__restrict__ head_ml,
    float *__restrict__ tail_ml, int64_t *__restrict__ head_seg, int64_t *__restrict__ tail_seg, int64_t nseg,
    int64_t E, int64_t H, int64_t D, int lg_lph, int lg_hpp) {
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  constexpr float kNegInf = -std::numeric_limits<float>::infinity();
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  const SegSlice slice = stage_slice(ptr, nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (e0 + (int64_t)wave * kSegChunk >= e1) return;  // such a wave has no chunk

  const GroupGeom geo = group_geom(lg_lph + lg_hpp, wave, lane, e1);
  const GvLane q = gv_lane(geo, lg_lph, lg_hpp, H, D, VEC);
  const int lpr = geo.lpr;
  const int64_t chunk = geo.chunk, W = H * D, d0 = q.d0, h = q.h;

  float m = kNegInf, l = 0.f;
  float acc[VEC], qa[VEC], aa[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    acc[v] = qa[v] = 0.f;
    aa[v] = q.colok && d0 + v < D ? Traits<T>::to_acc(att[q.hoff + d0 + v]) : 0.f;  // once per group
  }
  bool open = false, had_head = false;
  int32_t cur = -1;   // segment of the last entry taken
  int32_t qrow = -1;  // segment whose x_dst the lane holds

  for (int w = 0; w < kSegWindows; ++w) {
    int64_t e;
    const GroupEntry mine = gv_window(geo, slice, ptr, sp, ind, w, &e);
    for (int j0 = 0; j0 < lpr; j0 += kGvBatch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kGvBatch], sg[kGvBatch];
      P xv[kGvBatch];
#pragma unroll
      for (int u = 0; u < kGvBatch; ++u) {
        const GroupEntry en = group_broadcast(geo, mine, j0 + u);
        fl[u] = en.fl;
        sg[u] = en.seg;
        xv[u] = P();
        if ((fl[u] & kSegValid) && q.colok)
          xv[u] = gv_load<T, PACKED>(xs + ((uint64_t)en.col * (uint64_t)W + (uint64_t)q.hoff), d0, D);
      }
#pragma unroll
      for (int u = 0; u < kGvBatch; ++u) {
        const bool valid = (fl[u] & kSegValid) != 0;
        if (valid && sg[u] != qrow) {  // the segment changes: this lane's part of x_dst[row, h, :]
          qrow = sg[u];
          P a = P();
          if (q.colok) a = gv_load<T, PACKED>(xd + ((uint64_t)qrow * (uint64_t)W + (uint64_t)q.hoff), d0, D);
#pragma unroll
          for (int v = 0; v < VEC; ++v) qa[v] = Traits<T>::to_acc(a.v[v]);
        }
        float xf[VEC], part = 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          xf[v] = Traits<T>::to_acc(xv[u].v[v]);
          const float z = qa[v] + xf[v];  // one add: the sign of z is the sign of the exact sum
          part += aa[v] * gv_leaky(z, slope);
        }
        for (int off = q.lph >> 1; off > 0; off >>= 1) part += lane_xor(part, off);  // inside the head: off < lph
        if (valid) {  // an entry beyond the chunk adds nothing
          cur = sg[u];
          open = true;
          const SoftScale<float> sc = soft_scale(m, part);
          const float fa = sc.f_state(), fb = sc.f_entry();
          m = sc.mhi;
          l = l * fa + fb;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * fa + fb * xf[v];  // the packet that gave the score
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            const float lf = soft_final_l(m, l);
            if (q.colok) {
              float o[VEC];
#pragma unroll
              for (int v = 0; v < VEC; ++v) o[v] = acc[v] / lf;
              gv_store<T, PACKED>(out + ((uint64_t)sg[u] * (uint64_t)W + (uint64_t)q.hoff), d0, D, o);
              if (out_acc != nullptr) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                  if (d0 + v < D) out_acc[(uint64_t)sg[u] * (uint64_t)W + (uint64_t)(q.hoff + d0 + v)] = o[v];
              }
            }
            if (q.clerk) lse[(uint64_t)sg[u] * (uint64_t)H + (uint64_t)h] = m + logf(lf);
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (q.colok) {
#pragma unroll
              for (int v = 0; v < VEC; ++v)
                if (d0 + v < D) head_acc[(uint64_t)chunk * (uint64_t)W + (uint64_t)(q.hoff + d0 + v)] = acc[v];
            }
            if (q.clerk) {
              head_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2] = m;
              head_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2 + 1] = l;
            }
            if (q.scribe) head_seg[chunk] = sg[u];
          }
          m = kNegInf;
          l = 0.f;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
          open = false;
        }
      }
    }
  }
  if (geo.c0 < e1) {
    if (open && q.colok) {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (d0 + v < D) tail_acc[(uint64_t)chunk * (uint64_t)W + (uint64_t)(q.hoff + d0 + v)] = acc[v];
    }
    if (open && q.clerk) {
      tail_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2] = m;
      tail_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2 + 1] = l;
    }
    group_record_ids(geo, q.scribe, open, had_head, cur, head_seg, tail_seg);
  }
}

// (m, l, a) (+) (m2, l2, a2), every piece rescaled to the larger maximum
__device__ __forceinline__ void gv_combine(float &m, float &l, float &a, float m2, float l2, float a2) {
  const SoftScale<float> sc = soft_scale(m, m2);
  const float fa = sc.f_state(), fb = sc.f_entry();
  m = sc.mhi;
  l = l * fa + l2 * fb;
  a = a * fa + a2 * fb;
}

template <typename T>
__global__ __launch_bounds__(kGvWaves *kWave) void gatv2_fixup_kernel(
    const int64_t *__restrict__ ptr, T *__restrict__ out, float *__restrict__ out_acc, float *__restrict__ lse,
    const float *__restrict__ head_acc,
    const float *__restrict__ tail_acc, const float *__restrict__ head_ml, const float *__restrict__ tail_ml,
    const int64_t *__restrict__ head_seg, int64_t H, int64_t D, int64_t L, int64_t nchunks) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kGvWaves + (threadIdx.x >> 6);
  if (b >= nchunks) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  const int64_t W = H * D;
  const int64_t first = ptr[s] / L;  // every chunk in [first, b) ended inside s: its tail record is a piece of s
  for (int64_t col = lane; col < W; col += kWave) {
    const int64_t h = col / D;
    float m = -std::numeric_limits<float>::infinity(), l = 0.f, a = 0.f;
    for (int64_t i = first; i < b; ++i) {
      const uint64_t at = ((uint64_t)i * (uint64_t)H + (uint64_t)h) * 2;
      gv_combine(m, l, a, tail_ml[at], tail_ml[at + 1], tail_acc[(uint64_t)i * (uint64_t)W + (uint64_t)col]);
    }
    const uint64_t at = ((uint64_t)b * (uint64_t)H + (uint64_t)h) * 2;
    gv_combine(m, l, a, head_ml[at], head_ml[at + 1], head_acc[(uint64_t)b * (uint64_t)W + (uint64_t)col]);
    const float lf = soft_final_l(m, l);
    out[(uint64_t)s * (uint64_t)W + (uint64_t)col] = Traits<T>::from_acc(a / lf);
    if (out_acc != nullptr) out_acc[(uint64_t)s * (uint64_t)W + (uint64_t)col] = a / lf;
    if (col - h * D == 0) lse[(uint64_t)s * (uint64_t)H + (uint64_t)h] = m + logf(lf);
  }
}

int gv_fill(const GvCall &c, size_t itemsize, bool with_lse) {
  const int64_t bytes = (int64_t)itemsize * c.nseg * c.H * c.D, nlse = with_lse ? c.nseg * c.H : 0;
  const int64_t units = bytes / 16 + 2, n = units > nlse ? units : nlse;
  hipLaunchKernelGGL(gatv2_fill_kernel, dim3((unsigned int)ceil_div(n, (int64_t)256)), dim3(256), 0, c.stream,
                     reinterpret_cast<unsigned char *>(c.out), bytes, reinterpret_cast<float *>(c.lse), nlse);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

template <typename T>
int gv_launch_forward(const GvPlan &p, const GvCall &c) {
  const int st = gv_fill(c, sizeof(T), true);  // rows without entries: out = 0, lse = -inf
  if (st != TSAMD_OK || c.E == 0) return st;
  const SegRecords rec = gv_fw_records(p.chunk, c.H, c.D, c.E);
  const int64_t nchunks = (int64_t)rec.nchunks;
  float *head_acc = rec.plane<float>(c.workspace, 0), *tail_acc = rec.plane<float>(c.workspace, 1);
  float *head_ml = rec.plane<float>(c.workspace, 2), *tail_ml = rec.plane<float>(c.workspace, 3);
  int64_t *head_seg = rec.head_seg(c.workspace), *tail_seg = rec.tail_seg(c.workspace);
  const dim3 tiles((unsigned int)ceil_div(c.E, (int64_t)kExpandTile), (unsigned int)p.blocks), block(kGvWaves * kWave);
  T *oo = reinterpret_cast<T *>(c.out);
  float *ll = reinterpret_cast<float *>(c.lse);
#define TSAMD_GV_FW(PACKED)                                                                                           \
  hipLaunchKernelGGL((gatv2_tile_kernel<T, PACKED>), tiles, block, 0, c.stream, c.ptr, c.ind,                          \
                     reinterpret_cast<const T *>(c.xa), reinterpret_cast<const T *>(c.xb),                            \
                     reinterpret_cast<const T *>(c.att), (float)c.slope, oo, c.out_acc, ll, head_acc, tail_acc, head_ml, \
                     tail_ml, head_seg, tail_seg, c.nseg, c.E, c.H, c.D, p.lg_lph, p.lg_hpp)
  if (p.generic) TSAMD_GV_FW(false); else TSAMD_GV_FW(true);
#undef TSAMD_GV_FW
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((gatv2_fixup_kernel<T>), dim3((unsigned int)ceil_div(nchunks, (int64_t)kGvWaves)), block, 0,
                     c.stream, c.ptr, oo, c.out_acc, ll, (const float *)head_acc, (const float *)tail_acc,
                     (const float *)head_ml, (const float *)tail_ml, (const int64_t *)head_seg, c.H, c.D, p.chunk,
                     nchunks);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// ---- backward, entry kernel: p and ds per entry and head -------------------------------------------------------------
template <typename T, bool PACKED>
__global__ __launch_bounds__(kGvWaves *kWave) void gatv2_bw_kernel(
    const int64_t *__restrict__ row, const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind,
    const T *__restrict__ xd, const T *__restrict__ xs, const T *__restrict__ att, const float *__restrict__ o,
    const float *__restrict__ lse, const T *__restrict__ go, float slope, float *__restrict__ p_out,
    float *__restrict__ ds_out, int64_t nseg, int64_t H, int64_t D, int64_t E, int lg_lph, int lg_hpp) {
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  const int lane = (int)(threadIdx.x & 63);
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t base = ((int64_t)blockIdx.x * kGvWaves + wib) * kWave;
  if (base >= E) return;
  const int64_t rem = E - base;
  const int n = rem < kWave ? (int)rem : kWave;

  uint32_t c_l = 0, r_l = 0;  // this lane's entry
  if (lane < n) {
    const int64_t e = base + lane;
    c_l = (uint32_t)ind[e];
    r_l = (uint32_t)(row != nullptr ? row[e] : segment_of(ptr, nseg, e));
  }

  const int lg_lpr = lg_lph + lg_hpp;
  const int lph = 1 << lg_lph, hpp = 1 << lg_hpp;
  const int lg_g = 6 - lg_lpr;
  const int g = lane >> lg_lpr;                           // entry slot of the step
  const int hs = (lane & ((1 << lg_lpr) - 1)) >> lg_lph;  // head slot of the pass
  const int kl = lane & (lph - 1);                        // lane of the head
  const int64_t W = H * D, d0 = (int64_t)kl * VEC;
  const int nsteps = (n + (1 << lg_g) - 1) >> lg_g;

  for (int64_t h0 = 0; h0 < H; h0 += hpp) {
    const int64_t h = h0 + hs;
    const bool active = h < H && d0 < D;
    float aa[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) aa[v] = active && d0 + v < D ? Traits<T>::to_acc(att[h * D + d0 + v]) : 0.f;
    for (int s = 0; s < nsteps; ++s) {
      const int idx = (s << lg_g) + g;
      const int src = idx < n ? idx : n - 1;
      const uint32_t c = lane_read(c_l, src);
      const uint32_t r = lane_read(r_l, src);
      float ps = 0.f, pd = 0.f, pl = 0.f;
      if (active) {
        const uint64_t ar = (uint64_t)r * (uint64_t)W + (uint64_t)(h * D);
        const uint64_t ac = (uint64_t)c * (uint64_t)W + (uint64_t)(h * D);
        const P dv = gv_load<T, PACKED>(xd + ar, d0, D), sv = gv_load<T, PACKED>(xs + ac, d0, D);
        const P gv = gv_load<T, PACKED>(go + ar, d0, D);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float gj = Traits<T>::to_acc(gv.v[j]), xj = Traits<T>::to_acc(sv.v[j]);
          const float z = Traits<T>::to_acc(dv.v[j]) + xj;
          ps += aa[j] * gv_leaky(z, slope);
          pd += gj * xj;
          if (d0 + j < D) pl += gj * o[ar + (uint64_t)(d0 + j)];  // the unrounded out
        }
      }
      for (int off = lph >> 1; off > 0; off >>= 1) {  // inside the head: off < lph
        ps += lane_xor(ps, off);
        pd += lane_xor(pd, off);
        pl += lane_xor(pl, off);
      }
      if (h < H && kl == 0 && idx < n) {
        const int64_t e = base + idx;
        const float ls = lse[(uint64_t)r * (uint64_t)H + (uint64_t)h];
        float pv, dv;
        if (!(ls - ls == 0.f)) {  // -inf, +inf or NaN: the row is NaN in the forward
          pv = dv = std::numeric_limits<float>::quiet_NaN();
        } else if (ps == -std::numeric_limits<float>::infinity()) {
          pv = dv = 0.f;
        } else {
          pv = soft_exp(ps - ls);
          dv = pv * (pd - pl);
        }
        p_out[e * H + h] = pv;
        ds_out[e * H + h] = dv;
      }
    }
  }
}

template <typename T>
int gv_launch_entry(const GvPlan &p, const GvCall &c) {
  const int lg_hpp = p.lg_hpp < lg_ceil(kGvBwHeads) ? p.lg_hpp : lg_ceil(kGvBwHeads);
  const dim3 grid((unsigned int)ceil_div(c.E, (int64_t)kGvWaves * kWave)), block(kGvWaves * kWave);
#define TSAMD_GV_BW(PACKED)                                                                                          \
  hipLaunchKernelGGL((gatv2_bw_kernel<T, PACKED>), grid, block, 0, c.stream, c.row, c.ptr, c.ind,                    \
                     reinterpret_cast<const T *>(c.xa), reinterpret_cast<const T *>(c.xb),                           \
                     reinterpret_cast<const T *>(c.att), (const float *)c.out_acc,                                   \
                     reinterpret_cast<const float *>(c.lse), reinterpret_cast<const T *>(c.grad_out), (float)c.slope, \
                     c.p, c.ds, c.nseg, c.H, c.D, c.E, p.lg_lph, lg_hpp)
  if (p.generic) TSAMD_GV_BW(false); else TSAMD_GV_BW(true);
#undef TSAMD_GV_BW
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// ---- backward, segment kernel ----------------------------------------------------------------------------------------
template <typename T, bool PACKED, bool VALUE, bool ATT>
__global__ __launch_bounds__(kGvWaves *kWave) void gatv2_grad_kernel(
    const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind, const int64_t *__restrict__ perm,
    const T *__restrict__ xu, const T *__restrict__ xw, const T *__restrict__ att, float slope,
    const float *__restrict__ ds, const float *__restrict__ pp, const T *__restrict__ go, T *__restrict__ out,
    float *__restrict__ head_acc, float *__restrict__ tail_acc, float *__restrict__ att_part,
    int64_t *__restrict__ head_seg, int64_t *__restrict__ tail_seg, int64_t nseg, int64_t E, int64_t H, int64_t D,
    int lg_lph, int lg_hpp) {
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  const SegSlice slice = stage_slice(ptr, nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (e0 + (int64_t)wave * kSegChunk >= e1) return;  // such a wave has no chunk

  const GroupGeom geo = group_geom(lg_lph + lg_hpp, wave, lane, e1);
  const GvLane q = gv_lane(geo, lg_lph, lg_hpp, H, D, VEC);
  const int lpr = geo.lpr;
  const int64_t chunk = geo.chunk, W = H * D, d0 = q.d0, h = q.h;

  float acc[VEC], ua[VEC], aa[VEC], ga[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    acc[v] = ua[v] = ga[v] = 0.f;
    aa[v] = q.colok && d0 + v < D ? Traits<T>::to_acc(att[q.hoff + d0 + v]) : 0.f;
  }
  bool open = false, had_head = false;
  int32_t cur = -1, urow = -1;

  for (int w = 0; w < kSegWindows; ++w) {
    int64_t e;
    const GroupEntry mine = gv_window(geo, slice, ptr, sp, ind, w, &e);
    int64_t pe_l = 0;  // this lane's entry in the [E, H] arrays
    if (mine.fl & kSegValid) pe_l = perm != nullptr ? perm[e] : e;
    for (int j0 = 0; j0 < lpr; j0 += kGvBatch) {  // wave-uniform
      int32_t fl[kGvBatch], sg[kGvBatch];
      P wv[kGvBatch], gv[kGvBatch];
      float dsv[kGvBatch], pv[kGvBatch];
#pragma unroll
      for (int u = 0; u < kGvBatch; ++u) {
        const int j = j0 + u;
        const GroupEntry en = group_broadcast(geo, mine, j);
        const int64_t pe = lane_read(pe_l, group_src(geo, j));
        fl[u] = en.fl;
        sg[u] = en.seg;
        wv[u] = P();
        gv[u] = P();
        dsv[u] = pv[u] = 0.f;
        if ((fl[u] & kSegValid) && q.colok) {
          const uint64_t at = (uint64_t)en.col * (uint64_t)W + (uint64_t)q.hoff;
          wv[u] = gv_load<T, PACKED>(xw + at, d0, D);
          dsv[u] = ds[(uint64_t)pe * (uint64_t)H + (uint64_t)h];
          if constexpr (VALUE) {
            gv[u] = gv_load<T, PACKED>(go + at, d0, D);
            pv[u] = pp[(uint64_t)pe * (uint64_t)H + (uint64_t)h];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kGvBatch; ++u) {
        const bool valid = (fl[u] & kSegValid) != 0;
        if (valid && sg[u] != urow) {  // the segment changes: this lane's part of u[segment, h, :]
          urow = sg[u];
          P a = P();
          if (q.colok) a = gv_load<T, PACKED>(xu + ((uint64_t)urow * (uint64_t)W + (uint64_t)q.hoff), d0, D);
#pragma unroll
          for (int v = 0; v < VEC; ++v) ua[v] = Traits<T>::to_acc(a.v[v]);
        }
        if (valid) {
          cur = sg[u];
          open = true;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float z = ua[v] + Traits<T>::to_acc(wv[u].v[v]);  // the forward's add: the same branch
            acc[v] += (dsv[u] * aa[v]) * (z > 0.f ? 1.f : slope);
            if constexpr (VALUE) acc[v] += pv[u] * Traits<T>::to_acc(gv[u].v[v]);
            if constexpr (ATT) ga[v] += dsv[u] * gv_leaky(z, slope);
          }
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            if (q.colok) gv_store<T, PACKED>(out + ((uint64_t)sg[u] * (uint64_t)W + (uint64_t)q.hoff), d0, D, acc);
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (q.colok) {
#pragma unroll
              for (int v = 0; v < VEC; ++v)
                if (d0 + v < D) head_acc[(uint64_t)chunk * (uint64_t)W + (uint64_t)(q.hoff + d0 + v)] = acc[v];
            }
            if (q.scribe) head_seg[chunk] = sg[u];
          }
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
          open = false;
        }
      }
    }
  }
  if (geo.c0 < e1) {
    if (q.colok) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (d0 + v >= D) continue;
        const uint64_t at = (uint64_t)chunk * (uint64_t)W + (uint64_t)(q.hoff + d0 + v);
        if (open) tail_acc[at] = acc[v];
        if constexpr (ATT) att_part[at] = ga[v];  // every chunk with entries writes its whole partial row
      }
    }
    group_record_ids(geo, q.scribe, open, had_head, cur, head_seg, tail_seg);
  }
}

template <typename T>
__global__ __launch_bounds__(kGvWaves *kWave) void gatv2_grad_fixup_kernel(
    const int64_t *__restrict__ ptr, T *__restrict__ out, const float *__restrict__ head_acc,
    const float *__restrict__ tail_acc, const int64_t *__restrict__ head_seg, int64_t W, int64_t L, int64_t nchunks) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kGvWaves + (threadIdx.x >> 6);
  if (b >= nchunks) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  const int64_t first = ptr[s] / L;
  for (int64_t col = lane; col < W; col += kWave) {
    float a = 0.f;
    for (int64_t i = first; i < b; ++i) a += tail_acc[(uint64_t)i * (uint64_t)W + (uint64_t)col];
    a += head_acc[(uint64_t)b * (uint64_t)W + (uint64_t)col];
    out[(uint64_t)s * (uint64_t)W + (uint64_t)col] = Traits<T>::from_acc(a);
  }
}

// grad_att[col] = the partial rows of the chunks added in chunk order: kGvFoldSlices runs of consecutive chunks, a
// wave each, then the runs in order
template <typename T>
__global__ __launch_bounds__(kGvFoldSlices *kWave) void gatv2_att_fold_kernel(const float *__restrict__ part,
                                                                               int64_t nchunks, int64_t W,
                                                                               T *__restrict__ grad_att) {
  __shared__ float sh[kGvFoldSlices][kWave];
  const int lane = (int)(threadIdx.x & 63), slice = (int)(threadIdx.x >> 6);
  const int64_t col = (int64_t)blockIdx.x * kWave + lane;
  const int64_t per = (nchunks + kGvFoldSlices - 1) / kGvFoldSlices;
  const int64_t lo = slice * per, hi = lo + per < nchunks ? lo + per : nchunks;
  float a = 0.f;
  if (col < W)
    for (int64_t i = lo; i < hi; ++i) a += part[(uint64_t)i * (uint64_t)W + (uint64_t)col];
  sh[slice][lane] = a;
  __syncthreads();
  if (slice == 0 && col < W) {
    float t = 0.f;
    for (int j = 0; j < kGvFoldSlices; ++j) t += sh[j][lane];
    grad_att[col] = Traits<T>::from_acc(t);
  }
}

template <typename T>
int gv_launch_segment(const GvPlan &p, const GvCall &c) {
  const bool value = (c.flags & kGvValue) != 0, watt = (c.flags & kGvAtt) != 0;
  const int64_t W = c.H * c.D;
  const dim3 block(kGvWaves * kWave);
  const int st = gv_fill(c, sizeof(T), false);  // segments without entries
  if (st != TSAMD_OK) return st;
  if (c.E == 0) {
    if (watt) {  // an empty sum
      const int64_t bytes = (int64_t)sizeof(T) * W;
      hipLaunchKernelGGL(gatv2_fill_kernel, dim3((unsigned int)ceil_div(bytes / 16 + 2, (int64_t)256)), dim3(256), 0,
                         c.stream, reinterpret_cast<unsigned char *>(c.grad_att), bytes, (float *)nullptr, (int64_t)0);
      TSAMD_LAUNCH_CHECK();
    }
    return TSAMD_OK;
  }
  const SegRecords rec = gv_grad_records(p.chunk, c.H, c.D, c.E);
  const int64_t nchunks = (int64_t)rec.nchunks;
  float *head_acc = rec.plane<float>(c.workspace, 0), *tail_acc = rec.plane<float>(c.workspace, 1);
  float *part = rec.plane<float>(c.workspace, 2);
  int64_t *head_seg = rec.head_seg(c.workspace), *tail_seg = rec.tail_seg(c.workspace);
  const dim3 tiles((unsigned int)ceil_div(c.E, (int64_t)kExpandTile), (unsigned int)p.blocks);
  T *oo = reinterpret_cast<T *>(c.out);
#define TSAMD_GV_SEG(PACKED, VALUE, ATT)                                                                              \
  hipLaunchKernelGGL((gatv2_grad_kernel<T, PACKED, VALUE, ATT>), tiles, block, 0, c.stream, c.ptr, c.ind, c.perm,      \
                     reinterpret_cast<const T *>(c.xa), reinterpret_cast<const T *>(c.xb),                            \
                     reinterpret_cast<const T *>(c.att), (float)c.slope, (const float *)c.ds, (const float *)c.p,     \
                     reinterpret_cast<const T *>(c.grad_out), oo, head_acc, tail_acc, part, head_seg, tail_seg,       \
                     c.nseg, c.E, c.H, c.D, p.lg_lph, p.lg_hpp)
  if (value) {
    if (p.generic) TSAMD_GV_SEG(false, true, false); else TSAMD_GV_SEG(true, true, false);
  } else if (watt) {
    if (p.generic) TSAMD_GV_SEG(false, false, true); else TSAMD_GV_SEG(true, false, true);
  } else {
    if (p.generic) TSAMD_GV_SEG(false, false, false); else TSAMD_GV_SEG(true, false, false);
  }
#undef TSAMD_GV_SEG
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((gatv2_grad_fixup_kernel<T>), dim3((unsigned int)ceil_div(nchunks, (int64_t)kGvWaves)), block, 0,
                     c.stream, c.ptr, oo, (const float *)head_acc, (const float *)tail_acc, (const int64_t *)head_seg,
                     W, p.chunk, nchunks);
  TSAMD_LAUNCH_CHECK();
  if (watt) {
    hipLaunchKernelGGL((gatv2_att_fold_kernel<T>), dim3((unsigned int)ceil_div(W, (int64_t)kWave)),
                       dim3(kGvFoldSlices * kWave), 0, c.stream, (const float *)part, nchunks, W,
                       reinterpret_cast<T *>(c.grad_att));
    TSAMD_LAUNCH_CHECK();
  }
  return TSAMD_OK;
}

// ---- the driver ------------------------------------------------------------------------------------------------------
// the status of (dtype, H, D) alone, or kGvProceed: the route and workspace queries and every call start here
int gv_check_shape(int dtype, int64_t H, int64_t D) {
  if (H < 0 || D < 0) return TSAMD_ERR_INVALID;
  if (!gv_dtype_ok(dtype)) return TSAMD_ERR_UNSUPPORTED;  // float16 and float64 have no instantiation
  if (D > 64 * (16 / (int64_t)dtype_size(dtype))) return TSAMD_ERR_UNSUPPORTED;  // a head wider than its group of lanes
  if (H > 0 && D > 2147483647 / H) return TSAMD_ERR_UNSUPPORTED;
  return kGvProceed;
}

// the status of a call the host can decide, or kGvProceed.  include/tsamd.h lists the cases in this order
int gv_check(const GvCall &c) {
  const int64_t lim = 2147483647;
  if (c.nseg < 0 || c.nsrc < 0 || c.E < 0) return TSAMD_ERR_INVALID;
  const int st = gv_check_shape(c.dtype, c.H, c.D);
  if (st != kGvProceed) return st;
  if (!heads_indexable(c.nseg, c.nsrc, c.H, c.D, c.E)) return TSAMD_ERR_UNSUPPORTED;
  if (c.H > 0 && c.D > 0 && c.nseg > lim / 2 * 512 / (c.H * c.D)) return TSAMD_ERR_UNSUPPORTED;  // the fill's grid
  if (gv_plan(c.dtype, c.H, c.D, 0, nullptr, nullptr, nullptr).blocks > 65535)  // column blocks are blockIdx.y
    return TSAMD_ERR_UNSUPPORTED;
  if (ceil_div(c.E, (int64_t)kGvWaves * kWave) > lim) return TSAMD_ERR_UNSUPPORTED;
  const bool need_ws = c.kind != kGvEntry;
  if (c.kind == kGvEntry) {
    if (c.E == 0 || c.H == 0) return TSAMD_OK;  // p and ds have no element
    if (c.D == 0) return TSAMD_ERR_INVALID;     // the forward defines no lse for D = 0
    if (c.nseg == 0 || c.nsrc == 0 || !c.p || !c.ds || !c.ind || !c.xa || !c.xb || !c.att || !c.out_acc || !c.lse ||
        !c.grad_out || (!c.row && !c.ptr))
      return TSAMD_ERR_INVALID;
    return kGvProceed;
  }
  const bool watt = c.kind == kGvSegment && (c.flags & kGvAtt) != 0;
  if (c.kind == kGvSegment) {
    if (c.flags & ~(kGvValue | kGvAtt)) return TSAMD_ERR_INVALID;
    if ((c.flags & kGvValue) && (c.flags & kGvAtt)) return TSAMD_ERR_UNSUPPORTED;  // no such instantiation
  }
  if (c.nseg * c.H * c.D == 0 && !(watt && c.H * c.D > 0)) return TSAMD_OK;  // out has no element
  if ((c.nseg > 0 && !c.out) || (c.kind == kGvForward && !c.lse) || (watt && !c.grad_att)) return TSAMD_ERR_INVALID;
  if (c.E > 0) {
    if (c.nseg == 0 || c.nsrc == 0 || !c.ptr || !c.ind || !c.xa || !c.xb || !c.att) return TSAMD_ERR_INVALID;
    if (c.kind == kGvSegment && (!c.ds || ((c.flags & kGvValue) && (!c.p || !c.grad_out)))) return TSAMD_ERR_INVALID;
    if (need_ws && (!c.workspace || c.workspace_bytes < tsamd_gatv2_workspace_bytes(c.dtype, c.H, c.D, c.E)))
      return TSAMD_ERR_WORKSPACE;
  }
  return kGvProceed;
}

int gv_run(const GvCall &c) {
  const int st = gv_check(c);
  if (st != kGvProceed) return st;
  const void *third = c.kind == kGvEntry ? nullptr : c.out;
  const void *fourth = c.kind == kGvForward ? nullptr : c.grad_out;  // NULL counts as aligned
  const GvPlan p = gv_plan(c.dtype, c.H, c.D, c.E, c.xa, c.xb, third, fourth);
  if (c.dtype == TSAMD_F32)
    return c.kind == kGvForward ? gv_launch_forward<float>(p, c)
           : c.kind == kGvEntry ? gv_launch_entry<float>(p, c)
                                : gv_launch_segment<float>(p, c);
  return c.kind == kGvForward ? gv_launch_forward<bf16_t>(p, c)
         : c.kind == kGvEntry ? gv_launch_entry<bf16_t>(p, c)
                              : gv_launch_segment<bf16_t>(p, c);
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_gatv2_route(int dtype, int64_t H, int64_t D, int64_t E, const void *x_dst, const void *x_src,
                                 const void *out, int64_t out_route[7]) {
  if (!out_route || E < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 7; ++i) out_route[i] = 0;
  const int st = gv_check_shape(dtype, H, D);
  if (st != kGvProceed) return st;
  const GvPlan p = gv_plan(dtype, H, D, E, x_dst, x_src, out);
  out_route[0] = p.generic;
  out_route[1] = p.vec;
  out_route[2] = (int64_t)1 << p.lg_lph;
  out_route[3] = (int64_t)1 << p.lg_hpp;
  out_route[4] = p.blocks;
  out_route[5] = p.chunk;
  out_route[6] = (int64_t)p.workspace;
  return TSAMD_OK;
}

extern "C" size_t tsamd_gatv2_workspace_bytes(int dtype, int64_t H, int64_t D, int64_t E) {
  if (E < 0 || gv_check_shape(dtype, H, D) != kGvProceed) return 0;
  return gv_plan(dtype, H, D, E, nullptr, nullptr, nullptr).workspace;
}

extern "C" int tsamd_gatv2_attention(int dtype, const int64_t *rowptr, const int64_t *col, const void *x_dst,
                                     const void *x_src, const void *att, double negative_slope, void *out, float *out_acc,
                                     void *lse, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  GvCall c = {};
  c.dtype = dtype, c.kind = kGvForward, c.ptr = rowptr, c.ind = col, c.xa = x_dst, c.xb = x_src, c.att = att;
  c.slope = negative_slope, c.out = out, c.out_acc = out_acc, c.lse = lse, c.nseg = nseg, c.nsrc = nsrc, c.H = H, c.D = D, c.E = E;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = reinterpret_cast<hipStream_t>(stream);
  return gv_run(c);
}

// out_acc and lse are only read here
extern "C" int tsamd_gatv2_attention_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                        const void *x_dst, const void *x_src, const void *att, const float *out_acc,
                                        const void *lse, const void *grad_out, double negative_slope, float *p_out,
                                        float *ds_out, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *stream) {
  GvCall c = {};
  c.dtype = dtype, c.kind = kGvEntry, c.row = row, c.ptr = rowptr, c.ind = col, c.xa = x_dst, c.xb = x_src;
  c.att = att, c.slope = negative_slope, c.out_acc = const_cast<float *>(out_acc), c.lse = const_cast<void *>(lse);
  c.grad_out = grad_out, c.p = p_out, c.ds = ds_out, c.nseg = nseg, c.nsrc = nsrc, c.H = H, c.D = D, c.E = E;
  c.stream = reinterpret_cast<hipStream_t>(stream);
  return gv_run(c);
}

extern "C" int tsamd_gatv2_grad(int dtype, int flags, const int64_t *ptr, const int64_t *ind, const int64_t *perm,
                                const void *u, const void *w, const void *att, double negative_slope, const float *ds,
                                const float *p, const void *g, void *out, void *grad_att, int64_t nseg, int64_t nsrc,
                                int64_t H, int64_t D, int64_t E, void *workspace, size_t workspace_bytes,
                                void *stream) {
  GvCall c = {};
  c.dtype = dtype, c.kind = kGvSegment, c.flags = flags, c.ptr = ptr, c.ind = ind, c.perm = perm, c.xa = u, c.xb = w;
  c.att = att, c.slope = negative_slope, c.ds = const_cast<float *>(ds), c.p = const_cast<float *>(p);
  c.grad_out = (flags & kGvValue) ? g : nullptr, c.out = out, c.grad_att = grad_att;
  c.nseg = nseg, c.nsrc = nsrc, c.H = H, c.D = D, c.E = E;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = reinterpret_cast<hipStream_t>(stream);
  return gv_run(c);
}
