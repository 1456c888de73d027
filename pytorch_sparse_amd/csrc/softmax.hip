// Entry-balanced segmented softmax and its backward:
//   forward    y[p(i)] = exp(v[p(i)] - m_j) / s_j   for i in [ptr[j], ptr[j+1]),  p(i) = perm ? perm[i] : i,
//              m_j = max, s_j = sum of exp(v - m_j) over the segment (SparseTensor.softmax(dim): the rows through
//              rowptr, the columns through csr2csc / colptr);
//   backward   gv[p(i)] = y[p(i)] * (g[p(i)] - dot_j),  dot_j = sum of g * y over the segment.
//
// Both are a segmented reduction followed by a per-entry normalisation, on the tiling of segtile.h with the scan of
// segreduce.hip; they differ only in the MODE below: what a lane keeps of its entry, the scanned quantity and its
// combine, and the final expression.
//
//   tile kernel   segmented inclusive scan of every window, wave-uniform carry between the windows of a chunk.  The
//                 lane that holds the LAST entry of a segment that began inside the chunk leaves the segment's
//                 total in the wave's LDS slot of that entry; after the last window every lane fetches the total of its
//                 segment from there and writes its result -- the inputs are read once.  A segment cut by a chunk
//                 boundary writes nothing here; its records hold totals.
//   fix-up        one wave per chunk with a head record: the tail records of the chunks [ptr[s] / 512, b) are folded
//                 64 per round (lane l takes records l, l + 64, ... in entry order, then a xor butterfly), combined
//                 with the head record and left as the chunk's FINAL record.
//   finish        one wave per chunk that holds a piece of a cut segment (the others exit at once): re-reads the
//                 entries of the head piece [c0, ptr[hs + 1]) and of the tail piece [max(ptr[ts], c0), c1), takes the
//                 final record of the chunk where the segment ends and writes the result.
//
// The forward scans the pair (m, s) with the online-softmax combine (segtile.h)
//   (m1, s1) (+) (m2, s2) = (max, s_hi + s_lo * exp(m_lo - m_hi)),
// which is bitwise commutative, so the butterfly leaves the same bits in every lane.  An entry is (v, 1).  Non-finite
// inputs follow torch.softmax of the segment alone: a NaN entry makes s NaN (exp(NaN)) and a NaN s stays NaN through
// every later combine, so the whole segment is NaN; a segment that holds +inf ends with m = +inf, which the final
// expression turns into NaN for every entry; a segment of -inf only ends with m = -inf and exp(-inf - -inf) = NaN in
// the final expression; -inf beside finite entries gives exp(-inf) = 0.
// Accumulation is fp32 (fp64 for double); the result is rounded to the element type once, on the store.
// Deterministic (fixed combine tree), no atomics, no host sync.  Heads (D > 1) are blockIdx.y.
#include "segtile.h"

#include <type_traits>

namespace tsamd {
namespace {

constexpr int kSmFold = kWave;  // tail records one fix-up round folds

template <typename T>
struct SmForward {
  using A = typename Traits<T>::acc_t;
  struct Acc {
    A m, s;
  };
  struct In {
    A v;
  };
  __device__ static __forceinline__ Acc identity() { return {-std::numeric_limits<A>::infinity(), A(0)}; }
  __device__ static __forceinline__ In load(const T *__restrict__ value, const T *__restrict__, int64_t i) {
    return {Traits<T>::to_acc(value[i])};
  }
  __device__ static __forceinline__ Acc lift(In in) { return {in.v, A(1)}; }
  __device__ static __forceinline__ Acc combine(Acc a, Acc b) {
    const SoftScale<A> c = soft_scale(a.m, b.m);
    return {c.mhi, c.first ? a.s + b.s * c.f : a.s * c.f + b.s};  // not s * f_state + s2 * f_entry: segtile.h
  }
  __device__ static __forceinline__ Acc read(Acc a, int src) { return {lane_read(a.m, src), lane_read(a.s, src)}; }
  __device__ static __forceinline__ A finish(In in, Acc t) {
    // m = +inf: torch's sum holds exp(inf - inf) = NaN, so the finite entries are 0 / NaN, not 0 / s.  Not
    // soft_final_l: a NaN maximum keeps s here (NaN already, with its own sign and payload)
    const A s = t.m == std::numeric_limits<A>::infinity() ? std::numeric_limits<A>::quiet_NaN() : t.s;
    return soft_exp(in.v - t.m) / s;
  }
};

template <typename T>
struct SmBackward {
  using A = typename Traits<T>::acc_t;
  struct Acc {
    A s;
  };
  struct In {
    A y, g;
  };
  __device__ static __forceinline__ Acc identity() { return {A(0)}; }
  __device__ static __forceinline__ In load(const T *__restrict__ y, const T *__restrict__ grad, int64_t i) {
    return {Traits<T>::to_acc(y[i]), Traits<T>::to_acc(grad[i])};
  }
  __device__ static __forceinline__ Acc lift(In in) { return {in.g * in.y}; }
  __device__ static __forceinline__ Acc combine(Acc a, Acc b) { return {a.s + b.s}; }
  __device__ static __forceinline__ Acc read(Acc a, int src) { return {lane_read(a.s, src)}; }
  __device__ static __forceinline__ A finish(In in, Acc t) { return in.y * (in.g - t.s); }
};

// a, b: (value, unused) forward, (y, grad) backward
template <typename T, typename M>
__global__ __launch_bounds__(kSegWaves *kWave) void softmax_tile_kernel(
    const T *__restrict__ a, const T *__restrict__ b, const int64_t *__restrict__ perm,
    const int64_t *__restrict__ ptr, int64_t nseg, int64_t E, int64_t D, T *__restrict__ out,
    typename M::Acc *__restrict__ head_val, typename M::Acc *__restrict__ tail_val, int64_t *__restrict__ head_seg,
    int64_t *__restrict__ tail_seg, int64_t nchunks) {
  using Acc = typename M::Acc;
  using In = typename M::In;
  __shared__ int64_t sp[kExpandTile + 1];
  __shared__ int64_t span[2];
  __shared__ Acc totals[kExpandTile];  // slot of an entry: the total of the segment that ends there
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  const int64_t d = blockIdx.y;
  const SegSlice slice = stage_slice(ptr, nseg, e0, e1, sp, span);
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t chunk = (int64_t)blockIdx.x * kSegWaves + wave;
  const int64_t c0 = e0 + (int64_t)wave * kSegChunk;
  const int64_t c1 = c0 + kSegChunk < e1 ? c0 + kSegChunk : e1;
  if (c0 >= e1) return;  // such a wave has no chunk: chunk >= nchunks
  Acc *mine = totals + wave * kSegChunk;

  int64_t cseg = -1;  // wave-uniform carry: the segment still open at the end of the last window
  Acc cval = M::identity();
  int64_t hseg = -1;  // head record of this chunk (set by at most one lane)
  Acc hval = M::identity();
  In in[kSegWindows];
  int64_t at[kSegWindows];  // element index of the lane's entry in window w
  int endl[kSegWindows];    // chunk-local slot of its segment's last entry; -1: not finished here
#pragma unroll
  for (int w = 0; w < kSegWindows; ++w) {
    const int64_t base = c0 + (int64_t)w * kWave;
    endl[w] = -1;
    at[w] = 0;
    in[w] = In();
    if (base < c1) {
      const int64_t e = base + lane;
      const bool valid = e < c1;
      int64_t seg = -2 - lane, sstart = 0, send = 0;  // invalid lanes never match a neighbour
      Acc x = M::identity();
      if (valid) {
        const SegEntry en = slice_entry(slice, ptr, sp, e);
        seg = en.seg;
        sstart = en.start;
        send = en.end;
        at[w] = (perm ? perm[e] : e) * D + d;
        in[w] = M::load(a, b, at[w]);
        x = M::lift(in[w]);
      }
      // segmented inclusive scan: segments are contiguous runs, so "lane - off has my segment"
      // implies every lane in between has it too
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int src = lane >= off ? lane - off : lane;
        const Acc ox = M::read(x, src);
        const int64_t os = lane_read(seg, src);
        if (lane >= off && os == seg) x = M::combine(ox, x);
      }
      if (valid && seg == cseg) x = M::combine(cval, x);
      const bool is_end = valid && e + 1 == send;
      if (valid && sstart >= c0 && send <= c1) endl[w] = (int)(send - 1 - c0);
      if (is_end) {
        if (sstart >= c0) {
          mine[e - c0] = x;
        } else {  // began before this chunk: the fix-up kernel finishes it
          hseg = seg;
          hval = x;
        }
      }
      const int last = (int)((c1 - base < kWave ? c1 - base : kWave) - 1);  // wave-uniform
      const bool last_end = lane_read((int32_t)is_end, last) != 0;
      cseg = last_end ? -1 : lane_read(seg, last);
      cval = M::read(x, last);
    }
  }
  const unsigned long long hm = __ballot(hseg != -1);
  const int hl = hm ? (int)__builtin_ctzll(hm) : 0;
  const int64_t hs = lane_read(hseg, hl);
  const Acc hv = M::read(hval, hl);
  if (lane == 0) {
    head_seg[chunk] = hm ? hs : -1;
    tail_seg[chunk] = cseg;
    head_val[d * nchunks + chunk] = hv;
    tail_val[d * nchunks + chunk] = cval;
  }
  // the totals were written by other lanes of this wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int w = 0; w < kSegWindows; ++w) {
    if (endl[w] >= 0) out[at[w]] = Traits<T>::from_acc(M::finish(in[w], mine[endl[w]]));
  }
}

template <typename T, typename M>
__global__ __launch_bounds__(kSegWaves *kWave) void softmax_fixup_kernel(
    const int64_t *__restrict__ ptr, const typename M::Acc *__restrict__ head_val,
    const typename M::Acc *__restrict__ tail_val, const int64_t *__restrict__ head_seg,
    typename M::Acc *__restrict__ final_val, int64_t nchunks) {
  using Acc = typename M::Acc;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (b >= nchunks) return;
  const int64_t s = head_seg[b];
  if (s < 0) return;
  const int64_t d = blockIdx.y;
  const int64_t first = ptr[s] / kSegChunk;  // every chunk in [first, b) ended inside s: its tail record is a piece
  const Acc *tv = tail_val + d * nchunks;
  Acc acc = M::identity();
  for (int64_t i = first + lane; i < b; i += kSmFold) acc = M::combine(acc, tv[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = M::combine(acc, M::read(acc, lane ^ off));
  if (lane == 0) final_val[d * nchunks + b] = M::combine(acc, head_val[d * nchunks + b]);
}

template <typename T, typename M>
__global__ __launch_bounds__(kSegWaves *kWave) void softmax_finish_kernel(
    const T *__restrict__ a, const T *__restrict__ b, const int64_t *__restrict__ perm,
    const int64_t *__restrict__ ptr, int64_t E, int64_t D, T *__restrict__ out,
    const typename M::Acc *__restrict__ final_val, const int64_t *__restrict__ head_seg,
    const int64_t *__restrict__ tail_seg, int64_t nchunks) {
  using Acc = typename M::Acc;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t c = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const int64_t hs = head_seg[c], ts = tail_seg[c];
  if (hs < 0 && ts < 0) return;  // every segment of this chunk was finished by the tile kernel
  const int64_t d = blockIdx.y;
  const int64_t c0 = c * kSegChunk;
  const int64_t c1 = c0 + kSegChunk < E ? c0 + kSegChunk : E;
  int64_t hend = c0, tbeg = c1;  // head piece [c0, hend), tail piece [tbeg, c1)
  Acc ht = M::identity(), tt = M::identity();
  if (hs >= 0) {
    hend = ptr[hs + 1];
    ht = final_val[d * nchunks + c];
  }
  if (ts >= 0) {
    const int64_t ps = ptr[ts];
    tbeg = ps > c0 ? ps : c0;
    tt = final_val[d * nchunks + (ptr[ts + 1] - 1) / kSegChunk];  // the chunk where ts ends
  }
  for (int64_t e = c0 + lane; e < c1; e += kWave) {
    const bool head = e < hend;
    if (head || e >= tbeg) {
      const int64_t i = (perm ? perm[e] : e) * D + d;
      out[i] = Traits<T>::from_acc(M::finish(M::load(a, b, i), head ? ht : tt));
    }
  }
}

// head, tail and final records: at most the pair (m, s) each
SegRecords sm_records(size_t acc, int64_t E, int64_t D) {
  const size_t plane = 2 * acc * (size_t)(D > 0 ? D : 1);
  return SegRecords(E, kSegChunk, {plane, plane, plane});
}

template <typename T, typename M>
int launch_softmax(const T *a, const T *b, const int64_t *perm, const int64_t *ptr, int64_t nseg, int64_t E,
                   int64_t D, T *out, void *workspace, hipStream_t stream) {
  using A = typename Traits<T>::acc_t;
  using Acc = typename M::Acc;
  static_assert(sizeof(Acc) <= 2 * sizeof(A), "a record is at most the pair (m, s)");
  const SegRecords rec = sm_records(sizeof(A), E, D);
  const int64_t nchunks = (int64_t)rec.nchunks;
  Acc *head_val = rec.plane<Acc>(workspace, 0), *tail_val = rec.plane<Acc>(workspace, 1);
  Acc *final_val = rec.plane<Acc>(workspace, 2);
  int64_t *head_seg = rec.head_seg(workspace), *tail_seg = rec.tail_seg(workspace);
  const dim3 block(kSegWaves * kWave);
  const dim3 tiles((unsigned int)ceil_div(E, (int64_t)kExpandTile), (unsigned int)D);
  const dim3 chunks((unsigned int)ceil_div(nchunks, (int64_t)kSegWaves), (unsigned int)D);
  hipLaunchKernelGGL((softmax_tile_kernel<T, M>), tiles, block, 0, stream, a, b, perm, ptr, nseg, E, D, out, head_val,
                     tail_val, head_seg, tail_seg, nchunks);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((softmax_fixup_kernel<T, M>), chunks, block, 0, stream, ptr, (const Acc *)head_val,
                     (const Acc *)tail_val, (const int64_t *)head_seg, final_val, nchunks);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((softmax_finish_kernel<T, M>), chunks, block, 0, stream, a, b, perm, ptr, E, D, out,
                     (const Acc *)final_val, (const int64_t *)head_seg, (const int64_t *)tail_seg, nchunks);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// a, b: (value, NULL) forward, (y, grad) backward
template <bool BW>
int sm_entry(int dtype, const void *a, const void *b, const int64_t *perm, const int64_t *seg_ptr, int64_t nseg,
             int64_t E, int64_t D, void *out, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  if (nseg < 0 || E < 0 || D < 0) return TSAMD_ERR_INVALID;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (D > 65535) return TSAMD_ERR_UNSUPPORTED;
  if (E == 0 || D == 0) return TSAMD_OK;
  if (nseg == 0 || !out || !seg_ptr || !a || (BW && !b)) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_segment_softmax_workspace_bytes(dtype, E, D)) return TSAMD_ERR_WORKSPACE;
  return TSAMD_DISPATCH_FLOAT(dtype, [&]() -> int {
    using M = typename std::conditional<BW, SmBackward<scalar_t>, SmForward<scalar_t>>::type;
    return launch_softmax<scalar_t, M>(reinterpret_cast<const scalar_t *>(a), reinterpret_cast<const scalar_t *>(b),
                                       perm, seg_ptr, nseg, E, D, reinterpret_cast<scalar_t *>(out), workspace, stream);
  });
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_segment_softmax_route(int64_t out[8]) {
  if (!out) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = kSegChunk;
  out[1] = kExpandTile;
  out[2] = kExpandTile;  // a tile stages its pointer slice when it meets at most this many segments
  out[3] = kSmFold;
  return TSAMD_OK;
}

extern "C" size_t tsamd_segment_softmax_workspace_bytes(int dtype, int64_t E, int64_t D) {
  if (!is_float_dtype(dtype)) return 0;
  return sm_records(acc_size(dtype), E, D).bytes();
}

extern "C" int tsamd_segment_softmax(int dtype, const void *value, const int64_t *perm, const int64_t *seg_ptr,
                                     int64_t nseg, int64_t E, int64_t D, void *out, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  return sm_entry<false>(dtype, value, nullptr, perm, seg_ptr, nseg, E, D, out, workspace, workspace_bytes,
                         reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tsamd_segment_softmax_bw(int dtype, const void *y, const void *grad, const int64_t *perm,
                                        const int64_t *seg_ptr, int64_t nseg, int64_t E, int64_t D, void *grad_value,
                                        void *workspace, size_t workspace_bytes, void *stream) {
  return sm_entry<true>(dtype, y, grad, perm, seg_ptr, nseg, E, D, grad_value, workspace, workspace_bytes,
                        reinterpret_cast<hipStream_t>(stream));
}
