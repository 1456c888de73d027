// Multi-head SDDMM over a sparse pattern: the scores of an attention layer,
//   out[p(i), h] = scale * sum_d q[r(i), h, d] * k[ind[i], h, d],   p(i) = perm ? perm[i] : i,
// for the entries i of a segmented order (ptr, ind): CSR as it stands, CSC through (colptr, row, csr2csc).  r(i) is
// row[i] when the caller has the ids, else the last r with ptr[r] <= i.  q is [nseg, H, D], k is [nsrc, H, D], out is
// [E, H] with the H scores of an entry adjacent.
//
// The work is split by ENTRIES, as spmm_value_bw_kernel does: a wave owns 64 consecutive entries whatever the degrees
// and reads their ids once, coalesced.  A group of LPR = LPH * HPP lanes takes one entry per step: LPH lanes (a power
// of two) cover the D features of one head, HPP heads sit side by side in the group (at most kSdHeads), G = 64 / LPR
// entries side by side in the wave.  H > HPP takes ceil(H / HPP) passes over the wave's entries; every pass reads
// other heads of q and k, so nothing is gathered twice.  The reduction is a xor butterfly over the LPH lanes of a head
// only -- the masks stay below LPH and a head starts at a multiple of LPH, so no sum crosses into the next head.
//
//   packet route    D * itemsize a multiple of 16, D / VEC a power of two (VEC = 16 / itemsize) and q, k on a 16-byte
//                   boundary: a lane takes 16-byte packets kl, kl + LPH, ... of its head.
//   generic route   every other D >= 1 and operands off the boundary: the same kernel with VEC = 1, a lane takes
//                   features kl, kl + LPH, ...; lanes beyond D add zero to the butterfly.
//
// The scores of a pass are staged in the wave's LDS slice ([64 entries][heads of the pass]) and written by consecutive
// lanes to consecutive addresses: with H <= HPP and no perm a window is one run of 64 * H elements.
// f32 / f16 / bf16 accumulate in fp32, f64 in fp64; `scale` is applied to the accumulator and the product is rounded
// to the element type once, on the store.  Deterministic, no atomics, no workspace, no host sync, one launch.
#include "expand.h"

namespace tsamd {
namespace {

constexpr int kSdWaves = 4;    // waves per workgroup
constexpr int kSdHeads = 16;   // heads a group holds side by side at most (LDS: 64 * 16 accumulators per wave)

struct SdPlan {
  int generic;  // 0 packet route, 1 generic route
  int vec;      // elements per load
  int lg_lph;   // lanes per head
  int lg_lpr;   // lanes per entry = lanes per head * heads side by side
};

// the one place the route is decided: the driver and tsamd_sddmm_heads_route both plan through it
SdPlan sd_plan(int dtype, int64_t H, int64_t D, const void *q, const void *k) {
  SdPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  const bool packets = D > 0 && D % vec == 0 && ((D / vec) & (D / vec - 1)) == 0 && aligned16(q) && aligned16(k);
  p.generic = packets ? 0 : 1;
  p.vec = packets ? (int)vec : 1;
  const int64_t per_head = packets ? D / vec : (D > 0 ? D : 1);
  p.lg_lph = per_head >= kWave ? 6 : lg_ceil(per_head);
  int lg_hpp = H >= kSdHeads ? 4 : lg_ceil(H > 0 ? H : 1);
  if (lg_hpp > 6 - p.lg_lph) lg_hpp = 6 - p.lg_lph;
  p.lg_lpr = p.lg_lph + lg_hpp;
  return p;
}

template <typename T, int VEC>
__global__ __launch_bounds__(kSdWaves *kWave) void sddmm_heads_kernel(
    const int64_t *__restrict__ row, const int64_t *__restrict__ ptr, const int64_t *__restrict__ ind,
    const int64_t *__restrict__ perm, const T *__restrict__ q, const T *__restrict__ k,
    typename Traits<T>::acc_t scale, T *__restrict__ out, int64_t nseg, int64_t H, int64_t D, int64_t E, int lg_lph,
    int lg_lpr) {
  using A = typename Traits<T>::acc_t;
  using P = Pack<T, VEC>;
  __shared__ A stage[kSdWaves][kWave * kSdHeads];
  const int lane = (int)(threadIdx.x & 63);
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t base = ((int64_t)blockIdx.x * kSdWaves + wib) * kWave;
  if (base >= E) return;
  const int64_t rem = E - base;
  const int n = rem < kWave ? (int)rem : kWave;

  // this lane's entry
  uint32_t c_l = 0, r_l = 0;
  int64_t p_l = 0;
  if (lane < n) {
    const int64_t e = base + lane;
    c_l = (uint32_t)ind[e];
    r_l = (uint32_t)(row != nullptr ? row[e] : segment_of(ptr, nseg, e));
    p_l = perm ? perm[e] : e;
  }

  const int lph = 1 << lg_lph;
  const int lg_g = 6 - lg_lpr;
  const int hpp = 1 << (lg_lpr - lg_lph);
  const int g = lane >> lg_lpr;                        // entry slot of the step
  const int hs = (lane & ((1 << lg_lpr) - 1)) >> lg_lph;  // head slot of the pass
  const int kl = lane & (lph - 1);                     // lane of the head
  const int64_t slots = D / VEC;                       // packets (features on the generic route) per head
  const int nsteps = (n + (1 << lg_g) - 1) >> lg_g;
  A *mine = stage[wib];

  for (int64_t h0 = 0; h0 < H; h0 += hpp) {
    const int hc = H - h0 < hpp ? (int)(H - h0) : hpp;  // heads of this pass
    const bool active = hs < hc;
    const int64_t h = h0 + hs;
    for (int s = 0; s < nsteps; ++s) {
      const int idx = (s << lg_g) + g;
      const int src = idx < n ? idx : n - 1;
      const uint32_t c = lane_read(c_l, src);
      const uint32_t r = lane_read(r_l, src);
      A acc = A(0);
      if (active) {
        const T *qr = q + ((uint64_t)r * (uint64_t)H + (uint64_t)h) * (uint64_t)D;
        const T *kr = k + ((uint64_t)c * (uint64_t)H + (uint64_t)h) * (uint64_t)D;
        for (int64_t sl = kl; sl < slots; sl += lph) {
          const P x = *reinterpret_cast<const P *>(qr + sl * VEC);
          const P y = *reinterpret_cast<const P *>(kr + sl * VEC);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc += Traits<T>::to_acc(x.v[j]) * Traits<T>::to_acc(y.v[j]);
        }
      }
      for (int off = lph >> 1; off > 0; off >>= 1) acc += lane_xor(acc, off);  // inside the head: off < lph
      if (active && kl == 0 && idx < n) mine[idx * hc + hs] = acc * scale;
    }
    // the scores were staged by other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int total = n * hc;
    for (int t0 = 0; t0 < total; t0 += kWave) {  // wave-uniform trip count: every lane answers the lane_read
      const int t = t0 + lane;
      const bool ok = t < total;
      const int j = ok ? t / hc : 0;
      const int64_t pj = lane_read(p_l, j);
      if (ok) out[pj * H + h0 + (t - j * hc)] = Traits<T>::from_acc(mine[t]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the next pass overwrites the slice
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

template <typename T>
int launch_sddmm_heads(const SdPlan &p, const int64_t *row, const int64_t *ptr, const int64_t *ind,
                       const int64_t *perm, const void *q, const void *k, double scale, void *out, int64_t nseg,
                       int64_t H, int64_t D, int64_t E, hipStream_t stream) {
  using A = typename Traits<T>::acc_t;
  constexpr int kVec = 16 / (int)sizeof(T);
  const dim3 grid((unsigned int)ceil_div(E, (int64_t)kSdWaves * kWave)), block(kSdWaves * kWave);
  const T *qq = reinterpret_cast<const T *>(q), *kk = reinterpret_cast<const T *>(k);
  T *oo = reinterpret_cast<T *>(out);
  if (p.generic)
    hipLaunchKernelGGL((sddmm_heads_kernel<T, 1>), grid, block, 0, stream, row, ptr, ind, perm, qq, kk, (A)scale, oo,
                       nseg, H, D, E, p.lg_lph, p.lg_lpr);
  else
    hipLaunchKernelGGL((sddmm_heads_kernel<T, kVec>), grid, block, 0, stream, row, ptr, ind, perm, qq, kk, (A)scale,
                       oo, nseg, H, D, E, p.lg_lph, p.lg_lpr);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// sizes the 32-bit ids and the grid can carry
bool sd_indexable(int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E) {
  return heads_indexable(nseg, nsrc, H, D, E) && ceil_div(E, (int64_t)kSdWaves * kWave) <= 2147483647;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_sddmm_heads_route(int dtype, int64_t H, int64_t D, const void *q, const void *k,
                                       int64_t out[8]) {
  if (!out || H < 0 || D < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  const SdPlan p = sd_plan(dtype, H, D, q, k);
  out[0] = p.generic;
  out[1] = p.vec;
  out[2] = (int64_t)1 << p.lg_lph;
  out[3] = (int64_t)64 >> p.lg_lpr;
  out[4] = (int64_t)1 << (p.lg_lpr - p.lg_lph);
  out[5] = kWave;
  out[6] = kSdWaves * kWave;
  out[7] = kSdHeads;
  return TSAMD_OK;
}

extern "C" int tsamd_sddmm_heads(int dtype, const int64_t *row, const int64_t *ptr, const int64_t *ind,
                                 const int64_t *perm, const void *q, const void *k, double scale, void *out,
                                 int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (nseg < 0 || nsrc < 0 || H < 0 || D < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (!is_float_dtype(dtype)) return TSAMD_ERR_UNSUPPORTED;
  if (!sd_indexable(nseg, nsrc, H, D, E)) return TSAMD_ERR_UNSUPPORTED;
  if (E == 0 || H == 0 || D == 0) return TSAMD_OK;
  if (nseg == 0 || nsrc == 0 || !out || !ind || !q || !k || (!row && !ptr)) return TSAMD_ERR_INVALID;
  const SdPlan p = sd_plan(dtype, H, D, q, k);
  return TSAMD_DISPATCH_FLOAT(dtype, [&]() -> int {
    return launch_sddmm_heads<scalar_t>(p, row, ptr, ind, perm, q, k, scale, out, nseg, H, D, E, stream);
  });
}
