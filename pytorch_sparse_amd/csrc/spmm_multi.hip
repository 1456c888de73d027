// Fused multi-aggregation: up to six reductions of the products y_e = value[e] * x[col[e], :] of every row in ONE
// gather of x,
//   out[m, r, :] = reduce_r over e in [rowptr[m], rowptr[m+1]) of y_e,   reduce_r in sum, mean, min, max, var, std
// x is [N, F], out is [M, R, F] with R = the number of bits of `mask`, slots in bit order (tsamd_multi in tsamd.h);
// value == NULL means all ones.  var is the population variance, std its root; a row without entries gives 0 (and E
// in argmin / argmax).
//
// The group-walk kernel of segtile.h with the lane map of spmm_heads.hip: a group of LPR lanes holds one 16-byte
// packet of the row per lane, wider rows take column blocks (blockIdx.y), a group walks L = 8 * LPR entries and the
// gathers of four entries are issued before the first of them is used.  What a lane keeps per feature of its packet:
//
//   moments   S  = sum y                        (sum, mean: the plain running sum, one fma per entry)
//             K  = the first product of the piece, rounded once; any K is a valid shift
//             D1 = sum d, D2 = sum d^2,  d = fma(value, x, -K): the EXACT product minus K, rounded once
//             A piece of n entries is (n, mean, M2) = (n, K + D1 / n, D2 - D1^2 / n): no division per entry, and the
//             shift keeps D2 at the size of M2 + n (K - mean)^2 instead of n mean^2.
//   extrema   (min, argmin, max, argmax) with strict compares on the product rounded to the element type, started at
//             the largest / lowest finite value as tsamd_spmm does: the first occurrence wins a tie, a NaN product (and
//             a product beyond the finite range) never wins, a row of such products gives 0 and "no winner" = E.
//
// Three instantiations (moments, extrema, both), chosen from the mask: a ['mean', 'max'] call carries no variance
// sums and a ['sum', 'std'] call no winners.  The moment code is the same text in "moments" and "both", and the file
// is compiled without implicit contraction (every fma is written out), so a subset gives the bits of the full call.
//
//   tile kernel   walks the chunk; at the last entry of a row that began inside the chunk the row is finished in the
//                 accumulator type and written.  A row cut by a chunk boundary leaves records: per column the RAW
//                 sums (S, K, D1, D2) and (min, max, argmin, argmax) -- raw, because a piece mean rounded to fp32
//                 would put u * |mean| into the merge below.
//   fix-up        one wave per chunk with a head record, lanes over the columns: the tail records of the chunks
//                 [rowptr[s] / L, b) and then the head record are folded in chunk order in fp64.  A piece becomes
//                 (n, mean, M2) there (n from rowptr and the chunk bounds) and two pieces merge by
//                   M2 = M2a + M2b + delta^2 na nb / (na + nb),  mean = mean_a + delta nb / (na + nb)   (Chan et al.),
//                 the earlier piece first; the extrema fold with the same strict compares, so the first occurrence
//                 wins across pieces as well.
//   fill          rows without entries: zeros in every slot, E in the winners.
//
// Workspace: nchunks = ceil(E / L) chunks of [head | tail] records,
//   align256(8 * acc * F * nchunks)   moments (0 when the mask has none)
// + align256(4 * acc * F * nchunks)   extrema values, + align256(16 * F * nchunks) their entry ids (0 without)
// + 2 * align256(8 * nchunks)         head and tail row ids (-1: no record)
// No atomics, no host sync, three launches (fill, tile, fix-up), fixed combine tree: two calls give the same bits.
#include "segtile.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace tsamd {
namespace {

constexpr int kSmBatch = 4;  // gathers in flight per lane
constexpr int kSmMoments = 1, kSmExtrema = 2;
constexpr int kSmMomentBits = TSAMD_MULTI_SUM | TSAMD_MULTI_MEAN | TSAMD_MULTI_VAR | TSAMD_MULTI_STD;
constexpr int kSmExtremaBits = TSAMD_MULTI_MIN | TSAMD_MULTI_MAX;
constexpr int kSmAllBits = kSmMomentBits | kSmExtremaBits;

__device__ __forceinline__ float sm_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double sm_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sm_sqrt(float a) { return __fsqrt_rn(a); }
__device__ __forceinline__ double sm_sqrt(double a) { return __dsqrt_rn(a); }

int sm_set(int mask) { return ((mask & kSmMomentBits) ? kSmMoments : 0) | ((mask & kSmExtremaBits) ? kSmExtrema : 0); }

struct SmPlan {
  int generic, vec, lg_lpr, set;
  int64_t blocks, chunk;
};

// lanes per row from the packet count of an aligned row, also on the generic route (spmm_heads.hip: sh_lg_lpr)
int sm_lg_lpr(int dtype, int64_t F) {
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const int64_t packets = F > 0 ? ceil_div(F, vec) : 1;
  int lg = 0;
  while (lg < 6 && ((int64_t)1 << lg) < packets) ++lg;
  return lg;
}

// the one place the route is decided: the driver and tsamd_spmm_multi_route both plan through it
SmPlan sm_plan(int dtype, int mask, int64_t F, const void *x, const void *out, int64_t stride_m, int64_t stride_r) {
  SmPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const bool packets =
      F > 0 && F % vec == 0 && stride_m % vec == 0 && stride_r % vec == 0 && aligned16(x) && aligned16(out);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  p.lg_lpr = sm_lg_lpr(dtype, F);
  p.set = sm_set(mask);
  p.blocks = F > 0 ? ceil_div(ceil_div(F, (int64_t)p.vec), (int64_t)1 << p.lg_lpr) : 1;
  p.chunk = (int64_t)kSegWindows << p.lg_lpr;
  return p;
}

// planes: moments [chunk][head | tail][S, K, D1, D2][F], extrema values [chunk][head | tail][min, max][F], their
// entry ids the same shape in uint32
SegRecords sm_records(size_t acc, int set, int64_t chunk, int64_t F, int64_t E) {
  const size_t f = (size_t)(F > 0 ? F : 1);
  return SegRecords(E, chunk,
                    {(set & kSmMoments) ? 8 * acc * f : 0, (set & kSmExtrema) ? 4 * acc * f : 0,
                     (set & kSmExtrema) ? 16 * f : 0});
}

// slot of every reduction in out[m, :, f] (bit order), -1: not asked for
struct SmSlots {
  int sum, mean, min, max, var, std;
};
SmSlots sm_slots(int mask) {
  int r = 0;
  SmSlots s;
  s.sum = (mask & TSAMD_MULTI_SUM) ? r++ : -1;
  s.mean = (mask & TSAMD_MULTI_MEAN) ? r++ : -1;
  s.min = (mask & TSAMD_MULTI_MIN) ? r++ : -1;
  s.max = (mask & TSAMD_MULTI_MAX) ? r++ : -1;
  s.var = (mask & TSAMD_MULTI_VAR) ? r++ : -1;
  s.std = (mask & TSAMD_MULTI_STD) ? r++ : -1;
  return s;
}

template <typename T>
struct SmArgs {
  using A = typename Traits<T>::acc_t;
  const int64_t *ptr, *ind;
  const T *value, *x;
  T *out;
  int64_t *argmin, *argmax;
  A *mom, *ext;     // record planes
  uint32_t *ids;
  int64_t *head_seg, *tail_seg;
  int64_t nseg, E, F, sm, sr, L, nchunks;
  SmSlots slot;
  int lg_lpr;
};

// VEC consecutive elements of one slot of a row
template <typename T, int VEC>
__device__ __forceinline__ void sm_store(T *__restrict__ at, const typename Traits<T>::acc_t (&a)[VEC]) {
  Pack<T, VEC> o;
#pragma unroll
  for (int v = 0; v < VEC; ++v) o.v[v] = Traits<T>::from_acc(a[v]);
  *reinterpret_cast<Pack<T, VEC> *>(at) = o;
}

template <typename T, int VEC, int SET>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_multi_tile_kernel(const SmArgs<T> a) {
  using A = typename Traits<T>::acc_t;
  using P = Pack<T, VEC>;
  constexpr bool kMom = (SET & kSmMoments) != 0, kExt = (SET & kSmExtrema) != 0;
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < a.E ? e0 + kExpandTile : a.E;
  const SegSlice slice = stage_slice(a.ptr, a.nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = e0 + (int64_t)wave * kSegChunk;
  if (w0 >= e1) return;  // such a wave has no chunk

  const GroupGeom geo = group_geom(a.lg_lpr, wave, lane, e1);
  const int lpr = geo.lpr;
  const int64_t chunk = geo.chunk, c0 = geo.c0;
  const uint64_t F = (uint64_t)a.F;
  const int64_t col0 = ((int64_t)blockIdx.y * lpr + geo.gl) * VEC;
  const bool colok = col0 < a.F;  // the packet route has F % VEC == 0: a packet is inside the row or outside
  const bool scribe = geo.gl == 0 && blockIdx.y == 0;  // writes the row ids of the chunk's records
  const uint32_t none = (uint32_t)a.E;
  const bool has_value = a.value != nullptr;

  A S[VEC], K[VEC], D1[VEC], D2[VEC], mn[VEC], mx[VEC];
  uint32_t amn[VEC], amx[VEC];
  int32_t cnt = 0;  // entries of the open piece
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      S[v] = K[v] = D1[v] = D2[v] = A(0);
      mn[v] = Traits<T>::max_init();
      mx[v] = Traits<T>::lowest_init();
      amn[v] = amx[v] = none;
    }
    cnt = 0;
  };
  clear();
  bool open = false, had_head = false;
  int32_t cur = -1;  // row of the last entry taken

  // the raw sums and winners of the open piece -> the chunk's head (which = 0) or tail (1) record
  auto record = [&](int which) __attribute__((always_inline)) {
    const uint64_t at = (uint64_t)chunk * 2 + (uint64_t)which;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if constexpr (kMom) {
        A *m = a.mom + at * 4 * F + (uint64_t)col0 + v;
        m[0] = S[v], m[F] = K[v], m[2 * F] = D1[v], m[3 * F] = D2[v];
      }
      if constexpr (kExt) {
        A *x2 = a.ext + at * 2 * F + (uint64_t)col0 + v;
        uint32_t *i2 = a.ids + at * 2 * F + (uint64_t)col0 + v;
        x2[0] = mn[v], x2[F] = mx[v], i2[0] = amn[v], i2[F] = amx[v];
      }
    }
  };

  // a row that lies inside the chunk: finished in the accumulator type
  auto finish = [&](int32_t row) __attribute__((always_inline)) {
    T *o = a.out + (uint64_t)row * (uint64_t)a.sm + (uint64_t)col0;
    if constexpr (kMom) {
      const A n = (A)cnt;
      A r[VEC];
      if (a.slot.sum >= 0) sm_store<T, VEC>(o + a.slot.sum * a.sr, S);
      if (a.slot.mean >= 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) r[v] = S[v] / n;
        sm_store<T, VEC>(o + a.slot.mean * a.sr, r);
      }
      if (a.slot.var >= 0 || a.slot.std >= 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const A m2 = D2[v] - D1[v] * D1[v] / n;
          r[v] = (m2 > A(0) ? m2 : A(0)) / n;
        }
        if (a.slot.var >= 0) sm_store<T, VEC>(o + a.slot.var * a.sr, r);
        if (a.slot.std >= 0) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) r[v] = sm_sqrt(r[v]);
          sm_store<T, VEC>(o + a.slot.std * a.sr, r);
        }
      }
    }
    if constexpr (kExt) {
      A r[VEC];
      if (a.slot.min >= 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) r[v] = amn[v] == none ? A(0) : mn[v];
        sm_store<T, VEC>(o + a.slot.min * a.sr, r);
        if (a.argmin) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) a.argmin[(uint64_t)row * F + (uint64_t)col0 + v] = (int64_t)amn[v];
        }
      }
      if (a.slot.max >= 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) r[v] = amx[v] == none ? A(0) : mx[v];
        sm_store<T, VEC>(o + a.slot.max * a.sr, r);
        if (a.argmax) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) a.argmax[(uint64_t)row * F + (uint64_t)col0 + v] = (int64_t)amx[v];
        }
      }
    }
  };

  for (int w = 0; w < kSegWindows; ++w) {
    // one entry of the window per lane of the group
    const int64_t e = c0 + (int64_t)w * lpr + geo.gl;
    GroupEntry mine = {0, 0, 0};
    A val_l = A(1);
    if (e < geo.c1) {
      const SegEntry en = slice_entry(slice, a.ptr, sp, e);
      mine.seg = (int32_t)en.seg;
      mine.col = (uint32_t)a.ind[e];
      if (has_value) val_l = Traits<T>::to_acc(a.value[e]);
      mine.fl = kSegValid | (e + 1 == en.end ? kSegEnd : 0) | (en.start >= c0 ? kSegFresh : 0);
    }
    for (int j0 = 0; j0 < lpr; j0 += kSmBatch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kSmBatch], sg[kSmBatch];
      P xv[kSmBatch];
      A vv[kSmBatch];
#pragma unroll
      for (int u = 0; u < kSmBatch; ++u) {
        const int j = j0 + u;
        const GroupEntry en = group_broadcast(geo, mine, j);
        fl[u] = en.fl;
        sg[u] = en.seg;
        vv[u] = lane_read(val_l, group_src(geo, j));
        xv[u] = P();
        if ((fl[u] & kSegValid) && colok)
          xv[u] = *reinterpret_cast<const P *>(a.x + (uint64_t)en.col * F + (uint64_t)col0);
      }
#pragma unroll
      for (int u = 0; u < kSmBatch; ++u) {
        if (fl[u] & kSegValid) {  // an entry beyond the chunk takes no part
          cur = sg[u];
          open = true;
          const bool first = cnt == 0;
          const uint32_t id = (uint32_t)(c0 + (int64_t)w * lpr + j0 + u);
          ++cnt;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const A xa = Traits<T>::to_acc(xv[u].v[v]);
            const A y = vv[u] * xa;
            if constexpr (kMom) {
              S[v] = sm_fma(vv[u], xa, S[v]);
              K[v] = first ? y : K[v];
              const A d = sm_fma(vv[u], xa, -K[v]);
              D1[v] = D1[v] + d;
              D2[v] = sm_fma(d, d, D2[v]);
            }
            if constexpr (kExt) {
              const A p = has_value ? Traits<T>::round_acc(y) : xa;
              const bool lt = p < mn[v], gt = p > mx[v];
              mn[v] = lt ? p : mn[v];
              amn[v] = lt ? id : amn[v];
              mx[v] = gt ? p : mx[v];
              amx[v] = gt ? id : amx[v];
            }
          }
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            if (colok) finish(sg[u]);
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (colok) record(0);
            if (scribe) a.head_seg[chunk] = sg[u];
          }
          clear();
          open = false;
        }
      }
    }
  }
  if (c0 < e1) {
    if (open && colok) record(1);
    group_record_ids(geo, scribe, open, had_head, cur, a.head_seg, a.tail_seg);
  }
}

template <typename T, int SET>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_multi_fixup_kernel(const SmArgs<T> a) {
  using A = typename Traits<T>::acc_t;
  constexpr bool kMom = (SET & kSmMoments) != 0, kExt = (SET & kSmExtrema) != 0;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (b >= a.nchunks) return;
  const int64_t s = a.head_seg[b];
  if (s < 0) return;
  const uint64_t F = (uint64_t)a.F;
  const int64_t r0 = a.ptr[s], r1 = a.ptr[s + 1];
  const int64_t first = r0 / a.L;  // every chunk in [first, b) ended inside s: its tail record is a piece of s
  const uint32_t none = (uint32_t)a.E;
  for (int64_t col = lane; col < a.F; col += kWave) {
    T *o = a.out + (uint64_t)s * (uint64_t)a.sm + (uint64_t)col;
    if constexpr (kMom) {
      double S = 0, na = 0, mean = 0, M2 = 0;
      for (int64_t i = first; i <= b; ++i) {
        const A *m = a.mom + ((uint64_t)i * 2 + (i < b ? 1u : 0u)) * 4 * F + (uint64_t)col;
        const int64_t lo = i * a.L > r0 ? i * a.L : r0;
        const double nb = (double)((i < b ? (i + 1) * a.L : r1) - lo);  // the piece's entries
        const double d1 = (double)m[2 * F], d2 = (double)m[3 * F];
        const double mean_b = (double)m[F] + d1 / nb;
        double m2_b = d2 - d1 * d1 / nb;
        m2_b = m2_b > 0 ? m2_b : 0;
        S += (double)m[0];
        const double nab = na + nb, delta = mean_b - mean;
        M2 = M2 + m2_b + delta * delta * (na * nb / nab);  // the first piece: na = 0, delta^2 * 0
        mean = mean + delta * (nb / nab);
        na = nab;
      }
      const double var = M2 / na;
      if (a.slot.sum >= 0) o[a.slot.sum * a.sr] = Traits<T>::from_acc((A)S);
      if (a.slot.mean >= 0) o[a.slot.mean * a.sr] = Traits<T>::from_acc((A)S / (A)na);
      if (a.slot.var >= 0) o[a.slot.var * a.sr] = Traits<T>::from_acc((A)var);
      if (a.slot.std >= 0) o[a.slot.std * a.sr] = Traits<T>::from_acc((A)__dsqrt_rn(var));
    }
    if constexpr (kExt) {
      A mn = Traits<T>::max_init(), mx = Traits<T>::lowest_init();
      uint32_t amn = none, amx = none;
      for (int64_t i = first; i <= b; ++i) {
        const uint64_t at = ((uint64_t)i * 2 + (i < b ? 1u : 0u)) * 2 * F + (uint64_t)col;
        const A pmn = a.ext[at], pmx = a.ext[at + F];
        const bool lt = pmn < mn, gt = pmx > mx;  // strict: the earlier piece keeps a tie
        mn = lt ? pmn : mn;
        amn = lt ? a.ids[at] : amn;
        mx = gt ? pmx : mx;
        amx = gt ? a.ids[at + F] : amx;
      }
      if (a.slot.min >= 0) {
        o[a.slot.min * a.sr] = Traits<T>::from_acc(amn == none ? A(0) : mn);
        if (a.argmin) a.argmin[(uint64_t)s * F + (uint64_t)col] = (int64_t)amn;
      }
      if (a.slot.max >= 0) {
        o[a.slot.max * a.sr] = Traits<T>::from_acc(amx == none ? A(0) : mx);
        if (a.argmax) a.argmax[(uint64_t)s * F + (uint64_t)col] = (int64_t)amx;
      }
    }
  }
}

// rows without entries: zeros in all R slots, E in the winners
template <typename T>
__global__ __launch_bounds__(256) void spmm_multi_fill_kernel(const int64_t *__restrict__ ptr, T *__restrict__ out,
                                                              int64_t *__restrict__ argmin,
                                                              int64_t *__restrict__ argmax, int64_t nseg, int64_t F,
                                                              int64_t sm, int64_t sr, int R, int64_t E) {
  const int64_t total = nseg * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / F, col = i - row * F;
    if (ptr && ptr[row] != ptr[row + 1]) continue;
    for (int r = 0; r < R; ++r) out[(uint64_t)row * (uint64_t)sm + (uint64_t)r * (uint64_t)sr + (uint64_t)col] = T{};
    if (argmin) argmin[i] = E;
    if (argmax) argmax[i] = E;
  }
}

template <typename T, int SET>
int launch_spmm_multi_set(const SmPlan &p, const SmArgs<T> &a, hipStream_t stream) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const dim3 block(kSegWaves * kWave);
  const dim3 tiles((unsigned int)ceil_div(a.E, (int64_t)kExpandTile), (unsigned int)p.blocks);
  if (p.generic)
    hipLaunchKernelGGL((spmm_multi_tile_kernel<T, 1, SET>), tiles, block, 0, stream, a);
  else
    hipLaunchKernelGGL((spmm_multi_tile_kernel<T, kVec, SET>), tiles, block, 0, stream, a);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((spmm_multi_fixup_kernel<T, SET>), dim3((unsigned int)ceil_div(a.nchunks, (int64_t)kSegWaves)),
                     block, 0, stream, a);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

template <typename T>
int launch_fill(const int64_t *ptr, void *out, int64_t *argmin, int64_t *argmax, int64_t M, int64_t F, int64_t sm,
                int64_t sr, int mask, int64_t E, hipStream_t stream) {
  const int64_t blocks = ceil_div(M * F, (int64_t)256);
  hipLaunchKernelGGL((spmm_multi_fill_kernel<T>), dim3((unsigned int)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     stream, ptr, reinterpret_cast<T *>(out), (mask & TSAMD_MULTI_MIN) ? argmin : nullptr,
                     (mask & TSAMD_MULTI_MAX) ? argmax : nullptr, M, F, sm, sr, __builtin_popcount(mask), E);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

template <typename T>
int launch_spmm_multi(const SmPlan &p, int mask, const int64_t *ptr, const int64_t *ind, const void *value,
                      const void *x, void *out, int64_t sm, int64_t sr, int64_t *argmin, int64_t *argmax, int64_t M,
                      int64_t F, int64_t E, void *workspace, hipStream_t stream) {
  using A = typename Traits<T>::acc_t;
  const SegRecords rec = sm_records(sizeof(A), p.set, p.chunk, F, E);
  SmArgs<T> a;
  a.ptr = ptr, a.ind = ind;
  a.value = reinterpret_cast<const T *>(value), a.x = reinterpret_cast<const T *>(x);
  a.out = reinterpret_cast<T *>(out);
  a.argmin = (mask & TSAMD_MULTI_MIN) ? argmin : nullptr;
  a.argmax = (mask & TSAMD_MULTI_MAX) ? argmax : nullptr;
  a.mom = rec.plane<A>(workspace, 0), a.ext = rec.plane<A>(workspace, 1), a.ids = rec.plane<uint32_t>(workspace, 2);
  a.head_seg = rec.head_seg(workspace), a.tail_seg = rec.tail_seg(workspace);
  a.nseg = M, a.E = E, a.F = F, a.sm = sm, a.sr = sr, a.L = p.chunk, a.nchunks = (int64_t)rec.nchunks;
  a.slot = sm_slots(mask);
  a.lg_lpr = p.lg_lpr;
  const int st = launch_fill<T>(ptr, out, argmin, argmax, M, F, sm, sr, mask, E, stream);
  if (st != TSAMD_OK) return st;
  switch (p.set) {
    case kSmMoments: return launch_spmm_multi_set<T, kSmMoments>(p, a, stream);
    case kSmExtrema: return launch_spmm_multi_set<T, kSmExtrema>(p, a, stream);
    default: return launch_spmm_multi_set<T, kSmMoments | kSmExtrema>(p, a, stream);
  }
}

bool sm_mask_ok(int mask) { return mask > 0 && (mask & ~kSmAllBits) == 0; }

// sizes the 32-bit ids and the grid can carry
bool sm_indexable(int64_t M, int64_t N, int64_t F, int64_t E) {
  const int64_t lim = (int64_t)1 << 32;
  if (M >= lim / 2 || N >= lim || F >= lim / 2 || E >= lim) return false;
  return F <= 65535 * (int64_t)kWave;  // column blocks are blockIdx.y
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_spmm_multi_route(int dtype, int mask, int64_t F, const void *x, const void *out,
                                      int64_t stride_m, int64_t stride_r, int64_t out_route[8]) {
  if (!out_route || F < 0 || !sm_mask_ok(mask)) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out_route[i] = 0;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (!sm_indexable(0, 0, F, 0)) return TSAMD_ERR_UNSUPPORTED;
  const SmPlan p = sm_plan(dtype, mask, F, x, out, stride_m, stride_r);
  out_route[0] = p.generic;
  out_route[1] = p.vec;
  out_route[2] = (int64_t)1 << p.lg_lpr;
  out_route[3] = (int64_t)64 >> p.lg_lpr;
  out_route[4] = p.chunk;
  out_route[5] = kExpandTile;
  out_route[6] = p.set;
  out_route[7] = p.blocks;
  return TSAMD_OK;
}

extern "C" size_t tsamd_spmm_multi_workspace_bytes(int dtype, int mask, int64_t M, int64_t F, int64_t E) {
  if (!is_float_dtype(dtype) || !sm_mask_ok(mask) || M < 0 || F < 0 || E < 0) return 0;
  if (!sm_indexable(M, 0, F, E)) return 0;
  return sm_records(acc_size(dtype), sm_set(mask), (int64_t)kSegWindows << sm_lg_lpr(dtype, F), F, E).bytes();
}

extern "C" int tsamd_spmm_multi(int dtype, int mask, const int64_t *rowptr, const int64_t *col, const void *value,
                                const void *x, void *out, int64_t stride_m, int64_t stride_r, int64_t *argmin,
                                int64_t *argmax, int64_t M, int64_t N, int64_t F, int64_t E, void *workspace,
                                size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (M < 0 || N < 0 || F < 0 || E < 0 || stride_m < 0 || stride_r < 0 || !sm_mask_ok(mask)) return TSAMD_ERR_INVALID;
  if (!is_float_dtype(dtype) || !sm_indexable(M, N, F, E)) return TSAMD_ERR_UNSUPPORTED;
  if (M * F == 0) return TSAMD_OK;  // out has no element
  if (!out) return TSAMD_ERR_INVALID;
  if (E == 0)  // every row is empty
    return TSAMD_DISPATCH_FLOAT(dtype, [&]() -> int {
      return launch_fill<scalar_t>(nullptr, out, argmin, argmax, M, F, stride_m, stride_r, mask, E, stream);
    });
  if (N == 0 || !rowptr || !col || !x) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_spmm_multi_workspace_bytes(dtype, mask, M, F, E) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255u) != 0)
    return TSAMD_ERR_WORKSPACE;
  const SmPlan p = sm_plan(dtype, mask, F, x, out, stride_m, stride_r);
  return TSAMD_DISPATCH_FLOAT(dtype, [&]() -> int {
    return launch_spmm_multi<scalar_t>(p, mask, rowptr, col, value, x, out, stride_m, stride_r, argmin, argmax, M, F, E,
                                       workspace, stream);
  });
}
