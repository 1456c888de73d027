// Fused attention over a sparse pattern: scores, softmax over the row and aggregation in one pass,
//   s(i, h)      = scale * <q[r, h, :], k[col[i], h, :]> (+ bias[i] or bias[i, h])     for i in [rowptr[r], rowptr[r+1]),
//   out[r, h, :] = sum_i softmax_i(s(., h)) * v[col[i], h, :],    lse[r, h] = log sum_i exp(s(i, h)),
// q [M, H, D], k and v [N, H, D], out [M, H, D], lse [M, H] (fp32, fp64 for double).  Nothing of size E is written.
//
// The group-walk kernel of segtile.h with LPR = LPH * HPP lanes per group; the gathers of four entries -- their k and v
// parts -- are issued before the first of them is used.
//
//   lanes   LPH lanes (a power of two) cover the D features of one head, VEC = 16 / itemsize adjacent features per
//           lane; HPP heads (a power of two) sit side by side in the group, so the lanes of a head are a block that
//           starts at a multiple of LPH.  H > HPP takes ceil(H / HPP) column blocks (blockIdx.y): whole heads only.
//           D > 64 * VEC (the WIDE instantiation) splits the features of a head over FB = ceil(D / (64 * VEC))
//           further blocks; each of them forms the whole score (a strided loop over q and k) and keeps its own
//           features of the accumulator, so a head's softmax state never crosses a block.
//   score   the lanes of head h hold their part of q[row, h, :], reloaded where the segment changes, gather the same
//           part of k[col, h, :] and reduce with a xor butterfly whose masks stay below LPH.  scale, then the bias.
//   online  per group and head (m, l, acc[VEC]); an entry of score s and value part x is folded as
//           m' = max(m, s), l = l * e(m - m') + e(s - m'), acc = acc * e(m - m') + e(s - m') * x (soft_scale of
//           segtile.h).  e is __expf for fp32 accumulators and exp for fp64 -- no exp2 with a folded scale.
//   rows    where a segment that began inside the chunk ends, acc / l goes to out and m + log(l) to lse.  A record is
//           (m, l) per head and the accumulator row.  The fix-up launch (a wave per chunk with a head record, lanes
//           over the H * D columns) folds the tail records of the chunks [rowptr[s] / L, b) in chunk order, then the
//           head record, every piece rescaled to the running maximum, and writes out and lse.
//   fill    out is zeroed and lse set to -inf first (one launch): rows without entries are zeros.
//
// Non-finite scores follow softmax.hip per row and head: a NaN or +inf score ends with m NaN / +inf, which the final
// expression turns into NaN for the whole row of that head (lse NaN); a row of -inf only ends with l = 0, 0 / 0 = NaN
// and lse = -inf; -inf beside finite scores weighs 0.  State is cleared where a segment ends, so nothing reaches a
// neighbour of the chunk or the record.
//
//   packet route    D * itemsize a multiple of 16 and q, k, v, out on a 16-byte boundary: 16-byte loads and stores.
//   generic route   every other D >= 1 or operands off the boundary: the same lane-to-feature map, one element per
//                   load (VEC = 1 loads), features beyond D read as zero.
// The lane map -- hence the chunk length and the workspace -- is a function of (dtype, H, D) alone.
//
// Workspace: nchunks = ceil(E / L),
//   2 * align256(acc * nchunks * H * D)   head and tail accumulator rows
// + 2 * align256(2 * acc * nchunks * H)   head and tail (m, l) pairs
// + 2 * align256(8 * nchunks)             head and tail segment ids (-1: no record)
// Fixed combine tree (the entries of a chunk in order, the records in chunk order): two calls give the same bits.  No
// atomics, no host sync, three launches (fill, tile, fix-up).
//
// Backward (tsamd_attention_heads_bw), on the layout of sddmm_heads_kernel: a wave owns 64 consecutive entries, LPH
// lanes per head, heads and entries side by side.  An entry's ids are read once; three dot products share the
// butterfly: s = scale * <q, k> + bias, dp = <grad_out[row], v[col]>, delta = <grad_out[row], out[row]>.  It stores
// p = e(s - lse[row]) and ds = p * (dp - delta) as [E, H]; lse not finite: NaN both; s = -inf: 0 both.  One launch.
//
// Additive (GAT) scores (tsamd_gat_attention_heads, MODE = kAtAdditive of the same two kernels): one scalar per node
// and head instead of a dot product,
//   z(i, h) = a_dst[r, h] + a_src[col[i], h] (+ bias inside the activation),   s = z > 0 ? z : negative_slope * z.
// The kernels take a_dst for q, a_src for k and the slope for scale.  No q / k packets and no butterfly: the LPH lanes
// of head h all load the element a_src[col * H + h], in the batch of kAtBatch gathers beside the v packets; a_dst[row
// * H + h] is reloaded where the segment changes (the qrow logic); every feature block of a WIDE head forms the score
// itself.  a_dst / a_src are element loads of any alignment: the packet route is decided by v, out and D.  Lane map,
// chunk, records, fix-up, fill and workspace are those above.  The backward keeps two dot products (dp, delta) in the
// butterfly and stores p and dz = ds * (z > 0 ? 1 : negative_slope).
//
// Dropout on the probabilities (tsamd_*_dropout, the DROP instantiations of the same two kernels): a mask that is a pure
// function of (seed, entry e in CSR storage order, head h) -- at_drop_keep below, which host and device both compile --
//   thr = floor(rate * 2^32),  r = philox(seed, e >> 2, h, 0xD20B),  keep = r[e & 3] >= thr,  c = 1 / (1 - rate).
// The softmax state (m, l) is folded as without dropout; only the accumulator row sees the mask: acc = acc * fa +
// (keep ? fb * c : 0) * x.  So lse, the records, the fix-up, the fill and the workspace are unchanged, and every
// feature block of a WIDE head forms the same mask.  One Philox call serves four consecutive entries of a head: a
// group of at least kAtBatch lanes starts its batches at multiples of four and calls once per batch and head, a
// narrower group calls per entry.  The backward recomputes the mask and stores pt = p * keep * c (what grad_v needs)
// and ds = p * (keep * c * dp - delta); nothing of size E is kept for the mask.  rate == 0 runs the plain kernels.
#include "philox.h"
#include "segtile.h"

#include <cmath>

#include <type_traits>

namespace tsamd {
namespace {

constexpr int kAtWaves = kSegWaves;
constexpr int kAtBatch = 4;     // entries whose gathers are in flight
constexpr int kAtFwHeads = 64;  // heads side by side at most: forward (a whole wave),
constexpr int kAtBwHeads = 16;  // backward (H above takes passes)
constexpr int kAtDot = 0;       // score modes: scale * <q, k> + bias,
constexpr int kAtAdditive = 1;  // leaky_relu(a_dst + a_src + bias)

struct AtPlan {
  int generic;
  int vec;          // elements per load
  int lg_lph;       // lanes per head
  int lg_hpp;       // heads side by side
  int fblocks;      // feature blocks of a head (1 unless D > 64 * (16 / itemsize))
  int64_t blocks;   // column blocks = ceil(H / HPP) * fblocks
  int64_t chunk;    // entries per group
};

// one call, forward or backward, in either score mode: what the four entry points fill in
struct AtCall {
  int dtype, mode;
  const int64_t *row, *rowptr, *col;  // row: backward only, may be null
  const void *bias;
  int64_t bias_heads;
  const void *sr, *sc;  // the score operands of the row and of the column: q, k (kAtDot) or a_dst, a_src (kAtAdditive)
  const void *v;
  double scalar;        // scale (kAtDot) or negative_slope (kAtAdditive)
  void *out, *lse;      // written by the forward, read by the backward
  const void *grad_out;
  void *p_out, *d_out;  // backward: p and ds (kAtDot) or dz (kAtAdditive)
  int64_t nseg, nsrc, H, D, E;
  void *workspace;
  size_t workspace_bytes;
  hipStream_t stream;
  double dropout;  // rate in [0, 1) of the dropout on the probabilities; 0: the plain kernels
  uint64_t seed;   // of its mask
};
constexpr int kAtProceed = -1;  // no status yet: the call has work and its arguments are in order

// ---- the dropout mask: one rule for the kernels and the host query --------------------------------------------------
constexpr uint32_t kAtDropTag = 0xD20B;  // c3 of the mask's Philox calls (docs/design/oracle_parity.md, the draw table)

// rate in [0, 1): not NaN, not negative, not 1 or above
inline bool at_rate_ok(double rate) { return rate >= 0.0 && rate < 1.0; }
// floor(rate * 2^32): the product is exact in a double and below 2^32
inline uint32_t at_drop_threshold(double rate) { return (uint32_t)std::floor(rate * 4294967296.0); }

// the four words of the batch of entries [e & ~3, (e & ~3) + 4) of head h
__host__ __device__ __forceinline__ U4 at_drop_words(uint64_t seed, int64_t e, int64_t h) {
  return philox(seed, (uint64_t)e >> 2, (uint32_t)h, kAtDropTag);
}
__host__ __device__ __forceinline__ bool at_drop_pick(const U4 &r, int at, uint32_t thr) {
  const uint32_t word = at == 0 ? r.x : at == 1 ? r.y : at == 2 ? r.z : r.w;
  return word >= thr;
}
// keep of entry e (CSR storage order) and head h
__host__ __device__ __forceinline__ bool at_drop_keep(uint64_t seed, uint32_t thr, int64_t e, int64_t h) {
  return at_drop_pick(at_drop_words(seed, e, h), (int)(e & 3), thr);
}

__device__ __forceinline__ float at_log(float x) { return logf(x); }
__device__ __forceinline__ double at_log(double x) { return log(x); }

// torch's leaky_relu: z > 0 ? z : z * slope, also at z == 0 and for NaN
template <typename A>
__device__ __forceinline__ A at_leaky(A z, A slope) {
  return z > A(0) ? z : z * slope;
}

// the lane map: a function of (dtype, H, D) alone
void at_lanes(int dtype, int64_t H, int64_t D, int max_heads, AtPlan *p) {
  const int max_lg_hpp = lg_ceil(max_heads);
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const int64_t slots = D > 0 ? ceil_div(D, vec) : 1;
  p->lg_lph = slots >= kWave ? 6 : lg_ceil(slots);
  p->lg_hpp = lg_ceil(H > 0 ? H : 1);
  if (p->lg_hpp > max_lg_hpp) p->lg_hpp = max_lg_hpp;
  if (p->lg_hpp > 6 - p->lg_lph) p->lg_hpp = 6 - p->lg_lph;
  p->fblocks = (int)ceil_div(slots, (int64_t)kWave);
  p->blocks = ceil_div(H > 0 ? H : 1, (int64_t)1 << p->lg_hpp) * p->fblocks;
  p->chunk = (int64_t)kSegWindows << (p->lg_lph + p->lg_hpp);
}

// the one place the route is decided: the driver and tsamd_attention_heads_route both plan through it
AtPlan at_plan(int dtype, int64_t H, int64_t D, int max_heads, const void *q, const void *k, const void *v,
               const void *out, const void *more = nullptr) {
  AtPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const bool packets = D > 0 && D % vec == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) &&
                       aligned16(more);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  at_lanes(dtype, H, D, max_heads, &p);
  return p;
}

// head and tail records: an accumulator row and (m, l) per head each
SegRecords at_records(size_t acc, int64_t chunk, int64_t H, int64_t D, int64_t E) {
  const size_t h = (size_t)(H > 0 ? H : 1), w = h * (size_t)(D > 0 ? D : 1);
  return SegRecords(E, chunk, {acc * w, acc * w, 2 * acc * h, 2 * acc * h});
}

// VEC adjacent features of a head row, from feature d0: one 16-byte load, or element loads that read zero beyond D
template <typename T, bool PACKED>
__device__ __forceinline__ Pack<T, 16 / (int)sizeof(T)> at_load(const T *__restrict__ head_row, int64_t d0,
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

template <typename T, bool PACKED, typename A>
__device__ __forceinline__ void at_store(T *__restrict__ head_row, int64_t d0, int64_t D, const A *x) {
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

// out = 0, lse = -inf.  out is cleared in 16-byte units of its enclosing aligned range, the two ragged ends by bytes.
template <typename A>
__global__ __launch_bounds__(256) void attention_fill_kernel(unsigned char *__restrict__ out, int64_t out_bytes,
                                                              A *__restrict__ lse, int64_t nlse) {
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
  if (i < nlse) lse[i] = -std::numeric_limits<A>::infinity();
}

template <typename T, bool PACKED, bool WIDE, int MODE, bool DROP>
__global__ __launch_bounds__(kAtWaves *kWave) void attention_tile_kernel(
    const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind, const T *__restrict__ bias, int64_t bias_heads,
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ x, typename Traits<T>::acc_t scale,
    T *__restrict__ out, typename Traits<T>::acc_t *__restrict__ lse, typename Traits<T>::acc_t *__restrict__ head_acc,
    typename Traits<T>::acc_t *__restrict__ tail_acc, typename Traits<T>::acc_t *__restrict__ head_ml,
    typename Traits<T>::acc_t *__restrict__ tail_ml, int64_t *__restrict__ head_seg, int64_t *__restrict__ tail_seg,
    int64_t nseg, int64_t E, int64_t H, int64_t D, int lg_lph, int lg_hpp, int fblocks, uint64_t seed, uint32_t thr,
    typename Traits<T>::acc_t keep_scale) {
  using A = typename Traits<T>::acc_t;
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  constexpr A kNegInf = -std::numeric_limits<A>::infinity();
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  const SegSlice slice = stage_slice(ptr, nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = e0 + (int64_t)wave * kSegChunk;
  if (w0 >= e1) return;  // such a wave has no chunk

  const GroupGeom geo = group_geom(lg_lph + lg_hpp, wave, lane, e1);
  const int lpr = geo.lpr, lph = 1 << lg_lph;
  const int hs = geo.gl >> lg_lph;      // head slot
  const int kl = geo.gl & (lph - 1);    // lane of the head
  const int64_t chunk = geo.chunk, c0 = geo.c0;
  const int64_t W = H * D;
  const int hb = (int)blockIdx.y / fblocks, fb = (int)blockIdx.y - hb * fblocks;
  const int64_t h = ((int64_t)hb << lg_hpp) + hs;
  const bool hok = h < H;
  const int64_t slots = (D + VEC - 1) / VEC;
  const int64_t slot = (int64_t)fb * kWave + kl;
  const bool colok = hok && slot < slots;  // the packet route has D % VEC == 0: a packet is inside the head or outside
  const int64_t d0 = slot * VEC;
  const int64_t hoff = hok ? h * D : 0;
  const bool scribe = geo.gl == 0 && blockIdx.y == 0;  // writes the segment ids of the chunk's records
  const bool clerk = hok && kl == 0 && fb == 0;    // writes (m, l) and lse of its head

  A m = kNegInf, l = A(0);
  A acc[VEC], qa[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = qa[v] = A(0);
  bool open = false, had_head = false;
  int32_t cur = -1;   // segment of the last entry taken
  int32_t qrow = -1;  // segment whose q the lane holds

  for (int w = 0; w < kSegWindows; ++w) {
    // one entry of the window per lane of the group
    const int64_t e = c0 + (int64_t)w * lpr + geo.gl;
    GroupEntry mine = {0, 0, 0};
    if (e < geo.c1) {
      const SegEntry en = slice_entry(slice, ptr, sp, e);
      mine.seg = (int32_t)en.seg;
      mine.col = (uint32_t)ind[e];
      mine.fl = kSegValid | (e + 1 == en.end ? kSegEnd : 0) | (en.start >= c0 ? kSegFresh : 0);
    }
    for (int j0 = 0; j0 < lpr; j0 += kAtBatch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kAtBatch], sg[kAtBatch];
      uint32_t cc[kAtBatch];
      P kx[kAtBatch], xv[kAtBatch];
      A bb[kAtBatch], sa[kAtBatch];
      bool kp[kAtBatch];
      if constexpr (DROP) {
        const int64_t p0 = c0 + (int64_t)w * lpr + j0;  // the batch's first entry
        if (lpr >= kAtBatch) {  // p0 is a multiple of four: one call for the batch
          const U4 r = at_drop_words(seed, p0, h);
#pragma unroll
          for (int u = 0; u < kAtBatch; ++u) kp[u] = at_drop_pick(r, u, thr);
        } else {
#pragma unroll
          for (int u = 0; u < kAtBatch; ++u) kp[u] = at_drop_keep(seed, thr, p0 + u, h);
        }
      }
#pragma unroll
      for (int u = 0; u < kAtBatch; ++u) {
        const int j = j0 + u;
        const GroupEntry en = group_broadcast(geo, mine, j);
        fl[u] = en.fl;
        sg[u] = en.seg;
        cc[u] = en.col;
        kx[u] = P();
        xv[u] = P();
        bb[u] = A(0);
        sa[u] = A(0);
        if ((fl[u] & kSegValid) && hok) {
          const uint64_t at = (uint64_t)cc[u] * (uint64_t)W + (uint64_t)hoff;
          if constexpr (MODE == kAtAdditive)  // a_src[col, h]: the lanes of the head read one address
            sa[u] = Traits<T>::to_acc(k[(uint64_t)cc[u] * (uint64_t)H + (uint64_t)h]);
          if (colok) {
            if constexpr (!WIDE && MODE == kAtDot) kx[u] = at_load<T, PACKED>(k + at, d0, D);
            xv[u] = at_load<T, PACKED>(x + at, d0, D);
          }
          if (bias) {
            const int64_t p = c0 + (int64_t)w * lpr + j;
            bb[u] = Traits<T>::to_acc(bias[bias_heads > 1 ? p * bias_heads + h : p]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kAtBatch; ++u) {
        const bool valid = (fl[u] & kSegValid) != 0;
        A part = A(0);
        if constexpr (MODE == kAtAdditive) {
          if (valid && sg[u] != qrow) {  // the segment changes: a_dst[row, h]
            qrow = sg[u];
            qa[0] = hok ? Traits<T>::to_acc(q[(uint64_t)qrow * (uint64_t)H + (uint64_t)h]) : A(0);
          }
          if (valid) part = qa[0] + sa[u];
        } else if constexpr (WIDE) {
          if (valid && hok) {
            const T *qr = q + (uint64_t)sg[u] * (uint64_t)W + (uint64_t)hoff;
            const T *kr = k + (uint64_t)cc[u] * (uint64_t)W + (uint64_t)hoff;
            for (int64_t sl = kl; sl < slots; sl += kWave) {
              const P a = at_load<T, PACKED>(qr, sl * VEC, D), b = at_load<T, PACKED>(kr, sl * VEC, D);
#pragma unroll
              for (int v = 0; v < VEC; ++v) part += Traits<T>::to_acc(a.v[v]) * Traits<T>::to_acc(b.v[v]);
            }
          }
        } else {
          if (valid && sg[u] != qrow) {  // the segment changes: this lane's part of q[row, h, :]
            qrow = sg[u];
            P a = P();
            if (colok) a = at_load<T, PACKED>(q + (uint64_t)qrow * (uint64_t)W + (uint64_t)hoff, d0, D);
#pragma unroll
            for (int v = 0; v < VEC; ++v) qa[v] = Traits<T>::to_acc(a.v[v]);
          }
          if (valid) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) part += qa[v] * Traits<T>::to_acc(kx[u].v[v]);
          }
        }
        if constexpr (MODE == kAtDot)
          for (int off = lph >> 1; off > 0; off >>= 1) part += lane_xor(part, off);  // inside the head: off < lph
        if (valid) {  // an entry beyond the chunk adds nothing
          A s;
          if constexpr (MODE == kAtAdditive) s = at_leaky(part + bb[u], scale);  // the bias inside the activation
          else s = part * scale + bb[u];
          cur = sg[u];
          open = true;
          const SoftScale<A> sc = soft_scale(m, s);
          const A fa = sc.f_state(), fb_ = sc.f_entry();
          m = sc.mhi;
          l = l * fa + fb_;
          if constexpr (DROP) {  // (m, l) above are the plain call's: only the accumulator row sees the mask
            const A fk = kp[u] ? fb_ * keep_scale : A(0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * fa + fk * Traits<T>::to_acc(xv[u].v[v]);
          } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * fa + fb_ * Traits<T>::to_acc(xv[u].v[v]);
          }
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            const A lf = soft_final_l(m, l);
            if (colok) {
              A o[VEC];
#pragma unroll
              for (int v = 0; v < VEC; ++v) o[v] = acc[v] / lf;
              at_store<T, PACKED>(out + (uint64_t)sg[u] * (uint64_t)W + (uint64_t)hoff, d0, D, o);
            }
            if (clerk) lse[(uint64_t)sg[u] * (uint64_t)H + (uint64_t)h] = m + at_log(lf);
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (colok) {
#pragma unroll
              for (int v = 0; v < VEC; ++v)
                if (d0 + v < D) head_acc[(uint64_t)chunk * (uint64_t)W + (uint64_t)(hoff + d0 + v)] = acc[v];
            }
            if (clerk) {
              head_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2] = m;
              head_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2 + 1] = l;
            }
            if (scribe) head_seg[chunk] = sg[u];
          }
          m = kNegInf;
          l = A(0);
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
      for (int v = 0; v < VEC; ++v)
        if (d0 + v < D) tail_acc[(uint64_t)chunk * (uint64_t)W + (uint64_t)(hoff + d0 + v)] = acc[v];
    }
    if (open && clerk) {
      tail_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2] = m;
      tail_ml[((uint64_t)chunk * (uint64_t)H + (uint64_t)h) * 2 + 1] = l;
    }
    group_record_ids(geo, scribe, open, had_head, cur, head_seg, tail_seg);
  }
}

// (m, l, a) (+) (m2, l2, a2), every piece rescaled to the larger maximum: a column of the accumulator row beside l
template <typename A>
__device__ __forceinline__ void at_combine(A &m, A &l, A &a, A m2, A l2, A a2) {
  const SoftScale<A> sc = soft_scale(m, m2);
  const A fa = sc.f_state(), fb = sc.f_entry();
  m = sc.mhi;
  l = l * fa + l2 * fb;
  a = a * fa + a2 * fb;
}

template <typename T>
__global__ __launch_bounds__(kAtWaves *kWave) void attention_fixup_kernel(
    const int64_t *__restrict__ ptr, T *__restrict__ out, typename Traits<T>::acc_t *__restrict__ lse,
    const typename Traits<T>::acc_t *__restrict__ head_acc, const typename Traits<T>::acc_t *__restrict__ tail_acc,
    const typename Traits<T>::acc_t *__restrict__ head_ml, const typename Traits<T>::acc_t *__restrict__ tail_ml,
    const int64_t *__restrict__ head_seg, int64_t H, int64_t D, int64_t L, int64_t nchunks) {
  using A = typename Traits<T>::acc_t;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kAtWaves + (threadIdx.x >> 6);
  if (b >= nchunks) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  const int64_t W = H * D;
  const int64_t first = ptr[s] / L;  // every chunk in [first, b) ended inside s: its tail record is a piece of s
  for (int64_t col = lane; col < W; col += kWave) {
    const int64_t h = col / D;
    A m = -std::numeric_limits<A>::infinity(), l = A(0), a = A(0);
    for (int64_t i = first; i < b; ++i) {
      const uint64_t at = ((uint64_t)i * (uint64_t)H + (uint64_t)h) * 2;
      at_combine(m, l, a, tail_ml[at], tail_ml[at + 1], tail_acc[(uint64_t)i * (uint64_t)W + (uint64_t)col]);
    }
    const uint64_t at = ((uint64_t)b * (uint64_t)H + (uint64_t)h) * 2;
    at_combine(m, l, a, head_ml[at], head_ml[at + 1], head_acc[(uint64_t)b * (uint64_t)W + (uint64_t)col]);
    const A lf = soft_final_l(m, l);
    out[(uint64_t)s * (uint64_t)W + (uint64_t)col] = Traits<T>::from_acc(a / lf);
    if (col - h * D == 0) lse[(uint64_t)s * (uint64_t)H + (uint64_t)h] = m + at_log(lf);
  }
}

template <typename T, int MODE, bool DROP>
int launch_attention(const AtPlan &p, const AtCall &c) {
  using A = typename Traits<T>::acc_t;
  const int64_t nseg = c.nseg, H = c.H, D = c.D, E = c.E, W = H * D;
  hipStream_t stream = c.stream;
  const dim3 block(kAtWaves * kWave);
  T *oo = reinterpret_cast<T *>(c.out);
  A *ll = reinterpret_cast<A *>(c.lse);
  {  // rows without entries: out = 0, lse = -inf
    const int64_t bytes = (int64_t)sizeof(T) * nseg * W;
    const int64_t units = bytes / 16 + 2, n = units > nseg * H ? units : nseg * H;
    hipLaunchKernelGGL((attention_fill_kernel<A>), dim3((unsigned int)ceil_div(n, (int64_t)256)), block, 0, stream,
                       reinterpret_cast<unsigned char *>(c.out), bytes, ll, nseg * H);
    TSAMD_LAUNCH_CHECK();
  }
  if (E == 0) return TSAMD_OK;
  const SegRecords rec = at_records(sizeof(A), p.chunk, H, D, E);
  const int64_t nchunks = (int64_t)rec.nchunks;
  A *head_acc = rec.plane<A>(c.workspace, 0), *tail_acc = rec.plane<A>(c.workspace, 1);
  A *head_ml = rec.plane<A>(c.workspace, 2), *tail_ml = rec.plane<A>(c.workspace, 3);
  int64_t *head_seg = rec.head_seg(c.workspace), *tail_seg = rec.tail_seg(c.workspace);
  const dim3 tiles((unsigned int)ceil_div(E, (int64_t)kExpandTile), (unsigned int)p.blocks);
  const T *bb = reinterpret_cast<const T *>(c.bias), *qq = reinterpret_cast<const T *>(c.sr),
          *kk = reinterpret_cast<const T *>(c.sc), *xx = reinterpret_cast<const T *>(c.v);
  const uint32_t thr = at_drop_threshold(c.dropout);
  const A keep_scale = (A)(1.0 / (1.0 - c.dropout));
#define TSAMD_AT_LAUNCH(PACKED, WIDE)                                                                               \
  hipLaunchKernelGGL((attention_tile_kernel<T, PACKED, WIDE, MODE, DROP>), tiles, block, 0, stream, c.rowptr, c.col, \
                     bb, c.bias_heads, qq, kk, xx, (A)c.scalar, oo, ll, head_acc, tail_acc, head_ml, tail_ml,        \
                     head_seg, tail_seg, nseg, E, H, D, p.lg_lph, p.lg_hpp, p.fblocks, c.seed, thr, keep_scale)
  if (p.fblocks > 1) {
    if (p.generic) TSAMD_AT_LAUNCH(false, true); else TSAMD_AT_LAUNCH(true, true);
  } else {
    if (p.generic) TSAMD_AT_LAUNCH(false, false); else TSAMD_AT_LAUNCH(true, false);
  }
#undef TSAMD_AT_LAUNCH
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((attention_fixup_kernel<T>), dim3((unsigned int)ceil_div(nchunks, (int64_t)kAtWaves)), block, 0,
                     stream, c.rowptr, oo, ll, (const A *)head_acc, (const A *)tail_acc, (const A *)head_ml,
                     (const A *)tail_ml, (const int64_t *)head_seg, H, D, p.chunk, nchunks);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// ---- backward: p and ds per entry and head ---------------------------------------------------------------------------
template <typename T, bool PACKED, int MODE, bool DROP>
__global__ __launch_bounds__(kAtWaves *kWave) void attention_bw_kernel(
    const int64_t *__restrict__ row, const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind,
    const T *__restrict__ bias, int64_t bias_heads, const T *__restrict__ q, const T *__restrict__ k,
    const T *__restrict__ x, const T *__restrict__ o, const typename Traits<T>::acc_t *__restrict__ lse,
    const T *__restrict__ go, typename Traits<T>::acc_t scale, T *__restrict__ p_out, T *__restrict__ ds_out,
    int64_t nseg, int64_t H, int64_t D, int64_t E, int lg_lph, int lg_hpp, uint64_t seed, uint32_t thr,
    typename Traits<T>::acc_t keep_scale) {
  using A = typename Traits<T>::acc_t;
  constexpr int VEC = 16 / (int)sizeof(T);
  using P = Pack<T, VEC>;
  const int lane = (int)(threadIdx.x & 63);
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t base = ((int64_t)blockIdx.x * kAtWaves + wib) * kWave;
  if (base >= E) return;
  const int64_t rem = E - base;
  const int n = rem < kWave ? (int)rem : kWave;

  // this lane's entry
  uint32_t c_l = 0, r_l = 0;
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
  const int64_t slots = (D + VEC - 1) / VEC;
  const int64_t W = H * D;
  const int nsteps = (n + (1 << lg_g) - 1) >> lg_g;

  for (int64_t h0 = 0; h0 < H; h0 += hpp) {
    const int64_t h = h0 + hs;
    const bool active = h < H;
    for (int s = 0; s < nsteps; ++s) {
      const int idx = (s << lg_g) + g;
      const int src = idx < n ? idx : n - 1;
      const uint32_t c = lane_read(c_l, src);
      const uint32_t r = lane_read(r_l, src);
      A ps = A(0), pd = A(0), pl = A(0);
      if (active) {
        const uint64_t ar = (uint64_t)r * (uint64_t)W + (uint64_t)(h * D);
        const uint64_t ac = (uint64_t)c * (uint64_t)W + (uint64_t)(h * D);
        for (int64_t sl = kl; sl < slots; sl += lph) {
          if constexpr (MODE == kAtDot) {
            const P qv = at_load<T, PACKED>(q + ar, sl * VEC, D), kv = at_load<T, PACKED>(k + ac, sl * VEC, D);
            const P xv = at_load<T, PACKED>(x + ac, sl * VEC, D), gv = at_load<T, PACKED>(go + ar, sl * VEC, D);
            const P ov = at_load<T, PACKED>(o + ar, sl * VEC, D);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const A gj = Traits<T>::to_acc(gv.v[j]);
              ps += Traits<T>::to_acc(qv.v[j]) * Traits<T>::to_acc(kv.v[j]);
              pd += gj * Traits<T>::to_acc(xv.v[j]);
              pl += gj * Traits<T>::to_acc(ov.v[j]);
            }
          } else {  // the score needs no features
            const P xv = at_load<T, PACKED>(x + ac, sl * VEC, D), gv = at_load<T, PACKED>(go + ar, sl * VEC, D);
            const P ov = at_load<T, PACKED>(o + ar, sl * VEC, D);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const A gj = Traits<T>::to_acc(gv.v[j]);
              pd += gj * Traits<T>::to_acc(xv.v[j]);
              pl += gj * Traits<T>::to_acc(ov.v[j]);
            }
          }
        }
      }
      for (int off = lph >> 1; off > 0; off >>= 1) {  // inside the head: off < lph
        if constexpr (MODE == kAtDot) ps += lane_xor(ps, off);
        pd += lane_xor(pd, off);
        pl += lane_xor(pl, off);
      }
      if (active && kl == 0 && idx < n) {
        const int64_t e = base + idx;
        A sc = ps * scale;
        if (bias) sc += Traits<T>::to_acc(bias[bias_heads > 1 ? e * bias_heads + h : e]);
        if constexpr (MODE == kAtAdditive) {  // ps is zero in this mode: sc holds the bias alone, ps takes d s / d z
          sc = (Traits<T>::to_acc(q[(uint64_t)r * (uint64_t)H + (uint64_t)h]) +
                Traits<T>::to_acc(k[(uint64_t)c * (uint64_t)H + (uint64_t)h])) + sc;  // z: the bias inside
          ps = sc > A(0) ? A(1) : scale;
          sc = at_leaky(sc, scale);
        }
        const A ls = lse[(uint64_t)r * (uint64_t)H + (uint64_t)h];
        A pv, dv;
        if (!(ls - ls == A(0))) {  // -inf, +inf or NaN: the row is NaN in the forward
          pv = dv = std::numeric_limits<A>::quiet_NaN();
        } else if (sc == -std::numeric_limits<A>::infinity()) {
          pv = dv = A(0);
        } else {
          pv = soft_exp(sc - ls);
          if constexpr (DROP) {  // pt = p * keep * c goes to p_out; ds = p * (keep * c * dp - delta)
            const A kc = at_drop_keep(seed, thr, e, h) ? keep_scale : A(0);
            dv = pv * (kc * pd - pl);
            pv *= kc;
          } else {
            dv = pv * (pd - pl);
          }
          if constexpr (MODE == kAtAdditive) dv *= ps;  // dz
        }
        p_out[e * H + h] = Traits<T>::from_acc(pv);
        ds_out[e * H + h] = Traits<T>::from_acc(dv);
      }
    }
  }
}

template <typename T, int MODE, bool DROP>
int launch_attention_bw(const AtPlan &p, const AtCall &c) {
  using A = typename Traits<T>::acc_t;
  const uint32_t thr = at_drop_threshold(c.dropout);
  const A keep_scale = (A)(1.0 / (1.0 - c.dropout));
  const dim3 grid((unsigned int)ceil_div(c.E, (int64_t)kAtWaves * kWave)), block(kAtWaves * kWave);
#define TSAMD_AT_BW(PACKED)                                                                                         \
  hipLaunchKernelGGL((attention_bw_kernel<T, PACKED, MODE, DROP>), grid, block, 0, c.stream, c.row, c.rowptr, c.col, \
                     reinterpret_cast<const T *>(c.bias), c.bias_heads, reinterpret_cast<const T *>(c.sr),          \
                     reinterpret_cast<const T *>(c.sc), reinterpret_cast<const T *>(c.v),                           \
                     reinterpret_cast<const T *>(c.out), reinterpret_cast<const A *>(c.lse),                        \
                     reinterpret_cast<const T *>(c.grad_out), (A)c.scalar, reinterpret_cast<T *>(c.p_out),          \
                     reinterpret_cast<T *>(c.d_out), c.nseg, c.H, c.D, c.E, p.lg_lph, p.lg_hpp, c.seed, thr, keep_scale)
  if (p.generic) TSAMD_AT_BW(false); else TSAMD_AT_BW(true);
#undef TSAMD_AT_BW
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// sizes the 32-bit ids and the grids can carry
bool at_indexable(int dtype, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E) {
  const int64_t lim = 2147483647;
  if (!heads_indexable(nseg, nsrc, H, D, E)) return false;
  if (H > 0 && D > 0 && nseg > lim / 2 * 512 / (H * D)) return false;  // the fill: 16-byte units of out / 256
  AtPlan p;
  at_lanes(dtype, H, D, kAtFwHeads, &p);
  if (p.blocks > 65535) return false;  // column blocks are blockIdx.y
  return ceil_div(E, (int64_t)kAtWaves * kWave) <= lim;
}

// the status of a call the host can decide, or kAtProceed.  include/tsamd.h lists the cases in this order
int at_check_sizes(const AtCall &c) {
  if (!at_rate_ok(c.dropout)) return TSAMD_ERR_INVALID;  // only the *_dropout entries can carry one
  if (c.nseg < 0 || c.nsrc < 0 || c.H < 0 || c.D < 0 || c.E < 0) return TSAMD_ERR_INVALID;
  if (!is_float_dtype(c.dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (!at_indexable(c.dtype, c.nseg, c.nsrc, c.H, c.D, c.E)) return TSAMD_ERR_UNSUPPORTED;
  if (c.bias && c.bias_heads != 1 && c.bias_heads != c.H) return TSAMD_ERR_INVALID;
  return kAtProceed;
}

int at_check_forward(const AtCall &c) {
  const int st = at_check_sizes(c);
  if (st != kAtProceed) return st;
  if (c.nseg * c.H * c.D == 0) return TSAMD_OK;  // out has no element
  if (!c.out || !c.lse) return TSAMD_ERR_INVALID;
  if (c.E > 0) {
    if (c.nsrc == 0 || !c.rowptr || !c.col || !c.sr || !c.sc || !c.v) return TSAMD_ERR_INVALID;
    if (!c.workspace || c.workspace_bytes < tsamd_attention_heads_workspace_bytes(c.dtype, c.H, c.D, c.E))
      return TSAMD_ERR_WORKSPACE;
  }
  return kAtProceed;
}

int at_check_backward(const AtCall &c) {
  const int st = at_check_sizes(c);
  if (st != kAtProceed) return st;
  if (c.E == 0 || c.H == 0) return TSAMD_OK;  // p and ds / dz have no element
  if (c.D == 0) return TSAMD_ERR_INVALID;     // the forward defines no lse for D = 0
  if (c.nseg == 0 || c.nsrc == 0 || !c.p_out || !c.d_out || !c.col || !c.sr || !c.sc || !c.v || !c.out || !c.lse ||
      !c.grad_out || (!c.row && !c.rowptr))
    return TSAMD_ERR_INVALID;
  return kAtProceed;
}

// a_dst / a_src are element loads of any alignment: in kAtAdditive the route is decided by v, out, grad_out and D
AtPlan at_call_plan(const AtCall &c, int max_heads) {
  const bool dot = c.mode == kAtDot;
  return at_plan(c.dtype, c.H, c.D, max_heads, dot ? c.sr : nullptr, dot ? c.sc : nullptr, c.v, c.out, c.grad_out);
}

int at_forward(const AtCall &c) {
  const int st = at_check_forward(c);
  if (st != kAtProceed) return st;
  const AtPlan p = at_call_plan(c, kAtFwHeads);
  const bool drop = c.dropout != 0.0;  // rate 0 keeps every entry at c = 1: the plain kernels, the plain call's bits
  return TSAMD_DISPATCH_FLOAT(c.dtype, [&]() -> int {
    if (c.mode == kAtDot)
      return drop ? launch_attention<scalar_t, kAtDot, true>(p, c) : launch_attention<scalar_t, kAtDot, false>(p, c);
    return drop ? launch_attention<scalar_t, kAtAdditive, true>(p, c)
                : launch_attention<scalar_t, kAtAdditive, false>(p, c);
  });
}

int at_backward(const AtCall &c) {
  const int st = at_check_backward(c);
  if (st != kAtProceed) return st;
  const AtPlan p = at_call_plan(c, kAtBwHeads);
  const bool drop = c.dropout != 0.0;
  return TSAMD_DISPATCH_FLOAT(c.dtype, [&]() -> int {
    if (c.mode == kAtDot)
      return drop ? launch_attention_bw<scalar_t, kAtDot, true>(p, c) : launch_attention_bw<scalar_t, kAtDot, false>(p, c);
    return drop ? launch_attention_bw<scalar_t, kAtAdditive, true>(p, c)
                : launch_attention_bw<scalar_t, kAtAdditive, false>(p, c);
  });
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_attention_heads_route(int dtype, int64_t H, int64_t D, const void *q, const void *k,
                                           const void *v, const void *out, int64_t out_route[8]) {
  if (!out_route || H < 0 || D < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out_route[i] = 0;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (H > 0 && D > 2147483647 / H) return TSAMD_ERR_UNSUPPORTED;
  const AtPlan p = at_plan(dtype, H, D, kAtFwHeads, q, k, v, out);
  out_route[0] = p.generic;
  out_route[1] = p.vec;
  out_route[2] = (int64_t)1 << p.lg_lph;
  out_route[3] = (int64_t)1 << p.lg_hpp;
  out_route[4] = p.blocks;
  out_route[5] = p.chunk;
  out_route[6] = kExpandTile;  // entries per tile; a tile stages its pointer slice when it meets at most this many segments
  out_route[7] = p.fblocks;
  return TSAMD_OK;
}

extern "C" size_t tsamd_attention_heads_workspace_bytes(int dtype, int64_t H, int64_t D, int64_t E) {
  if (!is_float_dtype(dtype) || H < 0 || D < 0 || E < 0) return 0;
  if (H > 0 && D > 2147483647 / H) return 0;
  AtPlan p;
  at_lanes(dtype, H, D, kAtFwHeads, &p);
  return at_records(acc_size(dtype), p.chunk, H, D, E).bytes();
}

// ---- the four calls: a descriptor each.  The additive (GAT) pair runs the same kernels in MODE = kAtAdditive, a_dst
// for the row operand, a_src for the column operand, the slope for the scalar -------------------------------------------
extern "C" int tsamd_attention_heads(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                                     int64_t bias_heads, const void *q, const void *k, const void *v, double scale,
                                     void *out, void *lse, int64_t nseg, int64_t nsrc, int64_t H, int64_t D,
                                     int64_t E, void *workspace, size_t workspace_bytes, void *stream) {
  return at_forward({dtype, kAtDot, nullptr, rowptr, col, bias, bias_heads, q, k, v, scale, out, lse, nullptr, nullptr,
                     nullptr, nseg, nsrc, H, D, E, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream)});
}

extern "C" int tsamd_gat_attention_heads(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                                         int64_t bias_heads, const void *a_dst, const void *a_src, const void *v,
                                         double negative_slope, void *out, void *lse, int64_t nseg, int64_t nsrc,
                                         int64_t H, int64_t D, int64_t E, void *workspace, size_t workspace_bytes,
                                         void *stream) {
  return at_forward({dtype, kAtAdditive, nullptr, rowptr, col, bias, bias_heads, a_dst, a_src, v, negative_slope, out,
                     lse, nullptr, nullptr, nullptr, nseg, nsrc, H, D, E, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream)});
}

// out and lse are only read here
extern "C" int tsamd_attention_heads_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                        const void *bias, int64_t bias_heads, const void *q, const void *k,
                                        const void *v, const void *out, const void *lse, const void *grad_out,
                                        double scale, void *p_out, void *ds_out, int64_t nseg, int64_t nsrc, int64_t H,
                                        int64_t D, int64_t E, void *stream) {
  return at_backward({dtype, kAtDot, row, rowptr, col, bias, bias_heads, q, k, v, scale, const_cast<void *>(out),
                      const_cast<void *>(lse), grad_out, p_out, ds_out, nseg, nsrc, H, D, E, nullptr, 0,
                      reinterpret_cast<hipStream_t>(stream)});
}

extern "C" int tsamd_gat_attention_heads_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                            const void *bias, int64_t bias_heads, const void *a_dst, const void *a_src,
                                            const void *v, const void *out, const void *lse, const void *grad_out,
                                            double negative_slope, void *p_out, void *dz_out, int64_t nseg,
                                            int64_t nsrc, int64_t H, int64_t D, int64_t E, void *stream) {
  return at_backward({dtype, kAtAdditive, row, rowptr, col, bias, bias_heads, a_dst, a_src, v, negative_slope,
                      const_cast<void *>(out), const_cast<void *>(lse), grad_out, p_out, dz_out, nseg, nsrc, H, D, E,
                      nullptr, 0, reinterpret_cast<hipStream_t>(stream)});
}

// ---- dropout on the probabilities: the four calls again, with the rate and the seed of the mask after the scalar -------
extern "C" int tsamd_attention_heads_dropout(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                                             int64_t bias_heads, const void *q, const void *k, const void *v,
                                             double scale, double dropout, uint64_t seed, void *out, void *lse,
                                             int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E,
                                             void *workspace, size_t workspace_bytes, void *stream) {
  return at_forward({dtype, kAtDot, nullptr, rowptr, col, bias, bias_heads, q, k, v, scale, out, lse, nullptr, nullptr,
                     nullptr, nseg, nsrc, H, D, E, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream),
                     dropout, seed});
}

extern "C" int tsamd_gat_attention_heads_dropout(int dtype, const int64_t *rowptr, const int64_t *col,
                                                 const void *bias, int64_t bias_heads, const void *a_dst,
                                                 const void *a_src, const void *v, double negative_slope,
                                                 double dropout, uint64_t seed, void *out, void *lse, int64_t nseg,
                                                 int64_t nsrc, int64_t H, int64_t D, int64_t E, void *workspace,
                                                 size_t workspace_bytes, void *stream) {
  return at_forward({dtype, kAtAdditive, nullptr, rowptr, col, bias, bias_heads, a_dst, a_src, v, negative_slope, out,
                     lse, nullptr, nullptr, nullptr, nseg, nsrc, H, D, E, workspace, workspace_bytes,
                     reinterpret_cast<hipStream_t>(stream), dropout, seed});
}

extern "C" int tsamd_attention_heads_dropout_bw(int dtype, const int64_t *row, const int64_t *rowptr,
                                                const int64_t *col, const void *bias, int64_t bias_heads, const void *q,
                                                const void *k, const void *v, const void *out, const void *lse,
                                                const void *grad_out, double scale, double dropout, uint64_t seed,
                                                void *p_out, void *ds_out, int64_t nseg, int64_t nsrc, int64_t H,
                                                int64_t D, int64_t E, void *stream) {
  return at_backward({dtype, kAtDot, row, rowptr, col, bias, bias_heads, q, k, v, scale, const_cast<void *>(out),
                      const_cast<void *>(lse), grad_out, p_out, ds_out, nseg, nsrc, H, D, E, nullptr, 0,
                      reinterpret_cast<hipStream_t>(stream), dropout, seed});
}

extern "C" int tsamd_gat_attention_heads_dropout_bw(int dtype, const int64_t *row, const int64_t *rowptr,
                                                    const int64_t *col, const void *bias, int64_t bias_heads,
                                                    const void *a_dst, const void *a_src, const void *v,
                                                    const void *out, const void *lse, const void *grad_out,
                                                    double negative_slope, double dropout, uint64_t seed, void *p_out,
                                                    void *dz_out, int64_t nseg, int64_t nsrc, int64_t H, int64_t D,
                                                    int64_t E, void *stream) {
  return at_backward({dtype, kAtAdditive, row, rowptr, col, bias, bias_heads, a_dst, a_src, v, negative_slope,
                      const_cast<void *>(out), const_cast<void *>(lse), grad_out, p_out, dz_out, nseg, nsrc, H, D, E,
                      nullptr, 0, reinterpret_cast<hipStream_t>(stream), dropout, seed});
}

// host arithmetic only, through the rule the kernels compile: keep[(e - e0) * H + h] of the entries [e0, e0 + n)
extern "C" int tsamd_attention_dropout_mask(uint64_t seed, double rate, int64_t e0, int64_t n, int64_t H,
                                            uint8_t *keep) {
  if (!keep || e0 < 0 || n < 0 || H < 0 || !at_rate_ok(rate)) return TSAMD_ERR_INVALID;
  const uint32_t thr = at_drop_threshold(rate);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t h = 0; h < H; ++h) keep[i * H + h] = at_drop_keep(seed, thr, e0 + i, h) ? 1 : 0;
  return TSAMD_OK;
}
