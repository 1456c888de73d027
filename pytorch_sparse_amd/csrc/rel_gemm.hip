// Relational SpMM, the dense half: two matrix-instruction kernels over relation groups (docs/design/widening.md,
// "Relational SpMM"; C-ABI in include/tsamd.h).
//
//   rel_gemm    out[dst[t], :] = src[sidx[t], :] @ W[g]  (or W[g]^T)  for the items t of group g = [relptr[g], relptr[g+1])
//   rel_wgrad   grad_W[g] = sum over the items t of group g of  h[hidx[t], :]^T (outer) go[gidx[t], :]
//
// Both walk a table of units -- tiles of 64 items for rel_gemm, chunks of CK items for rel_wgrad -- that never straddle
// a group.  The table is built on the device from relptr: per-group unit counts, the exclusive scan of scan.h, one
// binary search per slot of the host-side bound ceil(P / unit) + R.  Slots past the last unit carry g = -1 and their
// workgroup returns.
//
// Operands.  float32 contracts with v_mfma_f32_32x32x2_f32, bfloat16 with v_mfma_f32_32x32x16_bf16; both accumulate in
// fp32.  A lane of these instructions supplies row (lane % 32) of each operand and, of the K step, the half
// (lane / 32).  Which k of the step a register element stands for is free as long as both operands agree, so a lane
// takes ONE 16-byte packet of its row per operand and 32-byte chunk of K: 8 bf16 = its half of one 32x32x16 step, or
// 4 floats = its halves of four 32x32x2 steps (step e contracts k = chunk * 8 + e and chunk * 8 + 4 + e).
//
// rel_gemm.  256 threads, a tile of 64 items x TN = 64 or 128 outputs.  K is cut into slices of 128 bytes (32 floats,
// 64 bf16).  A slice of the 64 gathered rows and of the TN weight rows is fetched in 16-byte packets into registers
// while the slice before it is contracted, then written to LDS rows of 144 bytes: 128 + 16 of padding, so that 8
// consecutive rows start 4 banks apart and every group of 8 lanes of a ds_read_b128 covers the 32 banks once (no bank
// conflict on the operand reads; the packet writes of 8 consecutive lanes fill one row, conflict-free as well).  The
// weights are repacked once per call to [R, N, Kp] with the contraction index contiguous and zero-padded to the packet
// (Kp), so both operands are staged and read the same way and the weight fetch needs no bounds test inside K.  Padding:
// a row past the tile's tail, a k past K and an output column past N are ZERO packets, so they add exact zeros.  The
// weight is the "A" operand (rows = output columns) and the items are the "B" operand: a lane then holds, for its item,
// 4 consecutive output columns per register quad and writes them with one 16-byte store into row dst[t].
//
// rel_wgrad.  256 threads, one chunk x a block of 64 x (64 or 128) of [F, Fo].  The items are the contraction index:
// slices of 32 gathered rows of h and go lie item-major in LDS, and the operands are read down the columns
// (float32: one ds_read_b32 per step, lanes on consecutive floats; bfloat16: 8 16-bit reads packed into the step's
// operand).  The block goes to wpart[chunk, F, Fo]; tsamd_segment_reduce folds a group's chunks in ascending order.
#include "rel_common.h"

namespace tsamd {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// weights -> [R, N, Kp], contraction index contiguous, zeros from K to Kp
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void rel_pack_weight(const T *__restrict__ w, T *__restrict__ wp, int64_t total, int64_t K, int64_t N,
                                int64_t Kp, int transposed) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int64_t k = o % Kp, gn = o / Kp, n = gn % N, g = gn / N;
  T v{};
  if (k < K) v = transposed ? w[(g * N + n) * K + k] : w[(g * K + k) * N + n];
  wp[o] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernel 1: gather - GEMM - scatter
// ---------------------------------------------------------------------------------------------------------------------
// Wave w: items (w & 1) * 32 .. + 32, output blocks of 32 columns (w >> 1) * NB .. + NB.  Accumulator register r of a lane
// is output column 8 * (r / 4) + 4 * (lane / 32) + r % 4 of the block, for item lane % 32.
template <typename T, int NB>
__global__ __launch_bounds__(kRelThreads) void rel_gemm_kernel(
    const T *__restrict__ src, int64_t n_src, bool vec_src, const int64_t *__restrict__ src_idx,
    const int64_t *__restrict__ dst_idx, const RelUnit *__restrict__ table, const T *__restrict__ wp, int64_t Kp,
    const float *__restrict__ dst_scale, float *__restrict__ out, int64_t n_dst, bool vec_out, int64_t K, int64_t N) {
  constexpr int TN = 64 * NB;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int KS = kRelSliceBytes / sizeof(T);
  constexpr int BPT = TN / 32;  // weight packets per thread and slice
  __shared__ __attribute__((aligned(16))) unsigned char lds_a[kRelTM * kRelLdsRow];
  __shared__ __attribute__((aligned(16))) unsigned char lds_b[TN * kRelLdsRow];

  const RelUnit u = table[blockIdx.x];
  if (u.g < 0) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
  const int64_t n0 = (int64_t)blockIdx.y * TN;

  // the packets this thread stages: row prow (+ 32 s) of either operand, packet pk of the slice
  const int prow = tid >> 3, pk = tid & 7;
  const T *arow[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int r = prow + 32 * s;
    arow[s] = nullptr;
    if (r < u.n) {
      const int64_t i = src_idx[u.start + r];
      if (i >= 0 && i < n_src) arow[s] = src + i * K;
    }
  }
  const T *brow[BPT];
#pragma unroll
  for (int s = 0; s < BPT; ++s) {
    const int64_t n = n0 + prow + 32 * s;
    brow[s] = n < N ? wp + ((int64_t)u.g * N + n) * Kp : nullptr;
  }
  uint4 ra[2], rb[BPT];
  auto fetch = [&](int64_t k0) {
    const int64_t k = k0 + (int64_t)pk * VEC;
#pragma unroll
    for (int s = 0; s < 2; ++s) ra[s] = rel_load_packet(arow[s], k, K, vec_src);
#pragma unroll
    for (int s = 0; s < BPT; ++s) rb[s] = rel_load_packet(brow[s], k, Kp, true);
  };

  f32x16 acc[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;

  const int ib = wave & 1, nb0 = (wave >> 1) * NB;
  fetch(0);
  for (int64_t k0 = 0; k0 < K; k0 += KS) {
#pragma unroll
    for (int s = 0; s < 2; ++s) *reinterpret_cast<uint4 *>(&lds_a[(prow + 32 * s) * kRelLdsRow + pk * 16]) = ra[s];
#pragma unroll
    for (int s = 0; s < BPT; ++s) *reinterpret_cast<uint4 *>(&lds_b[(prow + 32 * s) * kRelLdsRow + pk * 16]) = rb[s];
    __syncthreads();
    if (k0 + KS < K) fetch(k0 + KS);
#pragma unroll
    for (int c = 0; c < kRelSliceBytes / 32; ++c) {
      const int off = c * 32 + kh * 16;
      const uint4 item = *reinterpret_cast<const uint4 *>(&lds_a[(ib * 32 + li) * kRelLdsRow + off]);
#pragma unroll
      for (int x = 0; x < NB; ++x) {
        const uint4 w = *reinterpret_cast<const uint4 *>(&lds_b[((nb0 + x) * 32 + li) * kRelLdsRow + off]);
        RelMma<T>::packet(w, item, acc[x]);
      }
    }
    __syncthreads();
  }

  const int j = ib * 32 + li;
  if (j >= u.n) return;
  const int64_t d = dst_idx[u.start + j];
  if (d < 0 || d >= n_dst) return;
  const float scale = dst_scale ? dst_scale[d] : 1.f;
  float *orow = out + d * N;
#pragma unroll
  for (int x = 0; x < NB; ++x) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int64_t n = n0 + (nb0 + x) * 32 + 8 * rq + 4 * kh;
      const float4 v = float4{acc[x][4 * rq] * scale, acc[x][4 * rq + 1] * scale, acc[x][4 * rq + 2] * scale,
                              acc[x][4 * rq + 3] * scale};
      if (vec_out) {
        if (n < N) *reinterpret_cast<float4 *>(orow + n) = v;
      } else {
        if (n < N) orow[n] = v.x;
        if (n + 1 < N) orow[n + 1] = v.y;
        if (n + 2 < N) orow[n + 2] = v.z;
        if (n + 3 < N) orow[n + 3] = v.w;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// kernel 2: per-group weight gradient
// ---------------------------------------------------------------------------------------------------------------------
// 8 bf16 of column c, rows it .. it + 7 of an item-major LDS slice
__device__ inline uint4 rel_column8(const unsigned char *base, int row_bytes, int it, int c) {
  const unsigned char *p = base + it * row_bytes + c * 2;
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t lo = *reinterpret_cast<const uint16_t *>(p + (2 * e) * row_bytes);
    const uint32_t hi = *reinterpret_cast<const uint16_t *>(p + (2 * e + 1) * row_bytes);
    w[e] = lo | (hi << 16);
  }
  return uint4{w[0], w[1], w[2], w[3]};
}

// Wave w: rows (w & 1) * 32 .. + 32 of the block, column blocks of 32 (w >> 1) * NB .. + NB.  Accumulator register r of a
// lane is row 8 * (r / 4) + 4 * (lane / 32) + r % 4, column lane % 32.
template <typename T, int NB>
__global__ __launch_bounds__(kRelThreads) void rel_wgrad_kernel(
    const T *__restrict__ h, int64_t n_h, bool vec_h, const int64_t *__restrict__ h_idx, const T *__restrict__ go,
    int64_t n_go, bool vec_go, const int64_t *__restrict__ go_idx, const RelUnit *__restrict__ table,
    float *__restrict__ wpart, int64_t F, int64_t Fo, int fo_tiles) {
  constexpr int TFO = 64 * NB;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int HPR = kRelTF / VEC, GPR = TFO / VEC;  // packets per staged row
  constexpr int HROW = kRelTF * (int)sizeof(T) + 16, GROW = TFO * (int)sizeof(T) + 16;
  constexpr int HPT = kRelKI * HPR / kRelThreads, GPT = kRelKI * GPR / kRelThreads;
  static_assert(HPT >= 1 && GPT >= 1, "every thread stages at least one packet of each operand");
  __shared__ __attribute__((aligned(16))) unsigned char lds_h[kRelKI * HROW];
  __shared__ __attribute__((aligned(16))) unsigned char lds_g[kRelKI * GROW];

  const RelUnit u = table[blockIdx.x];
  if (u.g < 0) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
  const int64_t f0 = (int64_t)((int)blockIdx.y / fo_tiles) * kRelTF, fo0 = (int64_t)((int)blockIdx.y % fo_tiles) * TFO;

  uint4 rh[HPT], rg[GPT];
  auto fetch = [&](int it0) {
#pragma unroll
    for (int s = 0; s < HPT; ++s) {
      const int p = tid + kRelThreads * s, item = it0 + p / HPR;
      const T *row = nullptr;
      if (item < u.n) {
        const int64_t i = h_idx[u.start + item];
        if (i >= 0 && i < n_h) row = h + i * F;
      }
      rh[s] = rel_load_packet(row, f0 + (int64_t)(p % HPR) * VEC, F, vec_h);
    }
#pragma unroll
    for (int s = 0; s < GPT; ++s) {
      const int p = tid + kRelThreads * s, item = it0 + p / GPR;
      const T *row = nullptr;
      if (item < u.n) {
        const int64_t i = go_idx[u.start + item];
        if (i >= 0 && i < n_go) row = go + i * Fo;
      }
      rg[s] = rel_load_packet(row, fo0 + (int64_t)(p % GPR) * VEC, Fo, vec_go);
    }
  };

  f32x16 acc[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;

  const int fb = wave & 1, nb0 = (wave >> 1) * NB;
  fetch(0);
  for (int it0 = 0; it0 < u.n; it0 += kRelKI) {
#pragma unroll
    for (int s = 0; s < HPT; ++s) {
      const int p = tid + kRelThreads * s;
      *reinterpret_cast<uint4 *>(&lds_h[(p / HPR) * HROW + (p % HPR) * 16]) = rh[s];
    }
#pragma unroll
    for (int s = 0; s < GPT; ++s) {
      const int p = tid + kRelThreads * s;
      *reinterpret_cast<uint4 *>(&lds_g[(p / GPR) * GROW + (p % GPR) * 16]) = rg[s];
    }
    __syncthreads();
    if (it0 + kRelKI < u.n) fetch(it0 + kRelKI);
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
      for (int kk = 0; kk < kRelKI / 2; ++kk) {
        const int it = kk * 2 + kh;
        const float a = *reinterpret_cast<const float *>(&lds_h[it * HROW + (fb * 32 + li) * 4]);
#pragma unroll
        for (int x = 0; x < NB; ++x) {
          const float b = *reinterpret_cast<const float *>(&lds_g[it * GROW + ((nb0 + x) * 32 + li) * 4]);
          acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[x], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < kRelKI / 16; ++ks) {
        const int it = ks * 16 + kh * 8;
        const uint4 a = rel_column8(lds_h, HROW, it, fb * 32 + li);
#pragma unroll
        for (int x = 0; x < NB; ++x) {
          const uint4 b = rel_column8(lds_g, GROW, it, (nb0 + x) * 32 + li);
          RelMma<T>::packet(a, b, acc[x]);
        }
      }
    }
    __syncthreads();
  }

  float *block = wpart + (int64_t)blockIdx.x * F * Fo;
#pragma unroll
  for (int x = 0; x < NB; ++x) {
    const int64_t fo = fo0 + (nb0 + x) * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t f = f0 + fb * 32 + 8 * (r / 4) + 4 * kh + r % 4;
      if (f < F && fo < Fo) block[f * Fo + fo] = acc[x][r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------------------------------
struct RelGemmPlan {
  RelTablePlan t;
  size_t wp, bytes;
  int64_t Kp;
};
RelGemmPlan rel_gemm_plan(int dtype, int64_t P, int64_t R, int64_t K, int64_t N) {
  RelGemmPlan p;
  const int64_t vec = 16 / (int64_t)dtype_size(dtype);
  p.Kp = ceil_div(K, vec) * vec;
  p.t = rel_table_plan(P, R, kRelTM, 0);
  p.wp = p.t.end;
  p.bytes = p.wp + align_up(dtype_size(dtype) * (size_t)(R * N * p.Kp), 256);
  return p;
}

struct RelWgradPlan {
  RelTablePlan t;
  size_t wpart, sum, bytes;
  int64_t CK;
};
RelWgradPlan rel_wgrad_plan(int dtype, int64_t P, int64_t R, int64_t F, int64_t Fo) {
  RelWgradPlan p;
  p.CK = rel_chunk(P);
  p.t = rel_table_plan(P, R, p.CK, 0);
  p.wpart = p.t.end;
  p.sum = p.wpart + align_up(sizeof(float) * (size_t)(p.t.bound * F * Fo), 256);
  // fp32 sums of the chunks before the cast (float32 sums straight into the result)
  p.bytes = p.sum + (dtype == TSAMD_F32 ? 0 : align_up(sizeof(float) * (size_t)(R * F * Fo), 256));
  return p;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_rel_gemm_route(int dtype, int64_t P, int64_t R, int64_t F, int64_t Fo, int64_t out[16]) {
  if (!out || P < 0 || R < 0 || F < 0 || Fo < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_sizes(P, R, F, Fo)) return TSAMD_ERR_UNSUPPORTED;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  const RelGemmPlan g = rel_gemm_plan(dtype, P, R, F, Fo);
  const RelWgradPlan w = rel_wgrad_plan(dtype, P, R, F, Fo);
  out[0] = kRelTM;
  out[1] = rel_tn(Fo);
  out[2] = kRelSliceBytes / (int64_t)dtype_size(dtype);
  out[3] = g.t.bound;
  out[4] = 32;
  out[5] = 32;
  out[6] = dtype == TSAMD_F32 ? 2 : 16;
  out[7] = w.CK;
  out[8] = w.t.bound;
  out[9] = kRelKI;
  out[10] = kRelTF;
  out[11] = rel_tn(Fo);
  out[12] = (int64_t)g.bytes;
  out[13] = (int64_t)w.bytes;
  return TSAMD_OK;
}

extern "C" size_t tsamd_rel_gemm_workspace_bytes(int dtype, int64_t P, int64_t R, int64_t K, int64_t N) {
  if (!rel_dtype(dtype) || P < 0 || R < 0 || !rel_sizes(P, R, K, N)) return 0;
  return rel_gemm_plan(dtype, P, R, K, N).bytes;
}

extern "C" int tsamd_rel_gemm(int dtype, int transposed, const void *src, int64_t n_src, const int64_t *src_idx,
                              const int64_t *dst_idx, const int64_t *relptr, const void *weight, const float *dst_scale,
                              float *out, int64_t n_dst, int64_t P, int64_t R, int64_t K, int64_t N, void *workspace,
                              size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (P < 0 || R < 0 || K < 0 || N < 0 || n_src < 0 || n_dst < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_sizes(P, R, K, N)) return TSAMD_ERR_UNSUPPORTED;
  if (P == 0 || R == 0) return TSAMD_OK;
  if (!src || !src_idx || !dst_idx || !relptr || !weight || !out) return TSAMD_ERR_INVALID;
  const RelGemmPlan p = rel_gemm_plan(dtype, P, R, K, N);
  if (!workspace || workspace_bytes < p.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return TSAMD_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  const int st = rel_table_build(p.t, relptr, P, R, kRelTM, ws, stream);
  if (st != TSAMD_OK) return st;
  const bool vec_src = aligned16(src) && (K * (int64_t)dtype_size(dtype)) % 16 == 0;
  const bool vec_out = aligned16(out) && N % 4 == 0;
  const RelUnit *table = reinterpret_cast<const RelUnit *>(ws + p.t.table);
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    T *wp = reinterpret_cast<T *>(ws + p.wp);
    const int64_t total = R * N * p.Kp;
    hipLaunchKernelGGL((rel_pack_weight<T>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const T *>(weight), wp, total, K, N, p.Kp, transposed ? 1 : 0);
    TSAMD_LAUNCH_CHECK();
    const int tn = rel_tn(N);
    const dim3 grid((unsigned)p.t.bound, (unsigned)ceil_div(N, tn));
    if (tn == 64)
      hipLaunchKernelGGL((rel_gemm_kernel<T, 1>), grid, dim3(kRelThreads), 0, stream, reinterpret_cast<const T *>(src),
                         n_src, vec_src, src_idx, dst_idx, table, wp, p.Kp, dst_scale, out, n_dst, vec_out, K, N);
    else
      hipLaunchKernelGGL((rel_gemm_kernel<T, 2>), grid, dim3(kRelThreads), 0, stream, reinterpret_cast<const T *>(src),
                         n_src, vec_src, src_idx, dst_idx, table, wp, p.Kp, dst_scale, out, n_dst, vec_out, K, N);
    TSAMD_LAUNCH_CHECK();
    return TSAMD_OK;
  };
  return dtype == TSAMD_F32 ? run(float{}) : run(bf16_t{});
}

extern "C" size_t tsamd_rel_wgrad_workspace_bytes(int dtype, int64_t P, int64_t R, int64_t F, int64_t Fo) {
  if (!rel_dtype(dtype) || P < 0 || R < 0 || !rel_sizes(P, R, F, Fo)) return 0;
  return rel_wgrad_plan(dtype, P, R, F, Fo).bytes;
}

extern "C" int tsamd_rel_wgrad(int dtype, const void *h, int64_t n_h, const int64_t *h_idx, const void *go, int64_t n_go,
                               const int64_t *go_idx, const int64_t *relptr, void *grad_weight, int64_t P, int64_t R,
                               int64_t F, int64_t Fo, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (P < 0 || R < 0 || F < 0 || Fo < 0 || n_h < 0 || n_go < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_sizes(P, R, F, Fo)) return TSAMD_ERR_UNSUPPORTED;
  if (R == 0) return TSAMD_OK;
  if (!relptr || !grad_weight || (P > 0 && (!h || !h_idx || !go || !go_idx))) return TSAMD_ERR_INVALID;
  const RelWgradPlan p = rel_wgrad_plan(dtype, P, R, F, Fo);
  if (!workspace || workspace_bytes < p.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return TSAMD_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  int st = rel_table_build(p.t, relptr, P, R, p.CK, ws, stream);
  if (st != TSAMD_OK) return st;
  const RelUnit *table = reinterpret_cast<const RelUnit *>(ws + p.t.table);
  float *wpart = reinterpret_cast<float *>(ws + p.wpart);
  const int64_t esize = (int64_t)dtype_size(dtype);
  const bool vec_h = aligned16(h) && (F * esize) % 16 == 0, vec_go = aligned16(go) && (Fo * esize) % 16 == 0;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    if (P > 0) {
      const int tfo = rel_tn(Fo), fo_tiles = (int)ceil_div(Fo, tfo);
      const dim3 grid((unsigned)p.t.bound, (unsigned)(ceil_div(F, kRelTF) * fo_tiles));
      if (tfo == 64)
        hipLaunchKernelGGL((rel_wgrad_kernel<T, 1>), grid, dim3(kRelThreads), 0, stream, reinterpret_cast<const T *>(h), n_h,
                           vec_h, h_idx, reinterpret_cast<const T *>(go), n_go, vec_go, go_idx, table, wpart, F, Fo,
                           fo_tiles);
      else
        hipLaunchKernelGGL((rel_wgrad_kernel<T, 2>), grid, dim3(kRelThreads), 0, stream, reinterpret_cast<const T *>(h), n_h,
                           vec_h, h_idx, reinterpret_cast<const T *>(go), n_go, vec_go, go_idx, table, wpart, F, Fo,
                           fo_tiles);
      TSAMD_LAUNCH_CHECK();
    }
    // a group's chunks in ascending order; a group without items is an empty segment: zeros
    const bool direct = std::is_same<T, float>::value;
    float *sum = direct ? static_cast<float *>(grad_weight) : reinterpret_cast<float *>(ws + p.sum);
    st = tsamd_segment_reduce(TSAMD_F32, TSAMD_SUM, wpart, nullptr, reinterpret_cast<const int64_t *>(ws + p.t.uptr), R,
                              F * Fo, sum, stream_);
    if (st != TSAMD_OK) return st;
    if (!direct) {
      const int64_t n = R * F * Fo;
      hipLaunchKernelGGL((rel_cast_from_f32<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, stream, sum,
                         static_cast<T *>(grad_weight), n);
      TSAMD_LAUNCH_CHECK();
    }
    return TSAMD_OK;
  };
  return dtype == TSAMD_F32 ? run(float{}) : run(bf16_t{});
}
