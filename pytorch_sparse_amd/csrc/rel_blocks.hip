// Relational SpMM with block-diagonal weights W[g] = diag(Q[g, 0] .. Q[g, B - 1]), Q[g, b] of [ci, co]
// (docs/design/widening.md, "Block-diagonal relational SpMM"; C-ABI in include/tsamd.h).  Tiles, unit table, packets
// and matrix instructions are those of rel_gemm.hip (rel_common.h); what differs is how much of K a tile contracts.
//
//   rel_gemm_blocks    out[dst[t], b co + n] = sum_k src[sidx[t], b ci + k] Q[g, b][k, n]      (kb, nb) = (ci, co);
//                      transposed: the weight is [R, B, co, ci] and every block is read as its transpose
//   rel_wgrad_blocks   grad_Q[g, b] = sum over the items t of group g of  h[hidx[t], b-slice]^T (outer) go[gidx[t], b-slice]
//
// The window.  Output columns [n0, n1) only meet the diagonal blocks n0 / nb .. (n1 - 1) / nb, and these are
// consecutive, so the inputs they need are ONE range of K: [kb (n0 / nb), kb ((n1 - 1) / nb + 1)).  A workgroup runs its
// K loop over the window of its 64- or 128-column tile only (its start rounded down to the 16-byte packet), and inside a
// 128-byte slice a wave issues the matrix instruction for one of its 32-column blocks only in the 32-byte chunks of K
// that meet the block's OWN window; both tests are wave-uniform.  The weights are repacked once per call to
// [R, N, Kw]: row n holds, K-contiguous from its tile's window start, Q[g, n / nb][k - kb (n / nb), n % nb] where k lies
// in block n / nb and exact zeros elsewhere; Kw is the longest tile window, padded to the packet.  A 32-column block
// that straddles diagonal blocks multiplies the zeros between them: exact, and window / kb times the work it needs.
//
// rel_wgrad_blocks.  Chunks of CK items as in rel_wgrad, but only the 64 x (64 | 128) tiles of [F, Fo] that meet the
// diagonal: the rows a column tile needs are one range as well, so gridDim.y = column tiles x the longest such range in
// row tiles and a workgroup past its own range returns before its first load.  Inside a tile only the 32 x 32 blocks that
// meet the diagonal are contracted, dealt to the four waves in turn, and the store keeps the elements with
// f / ci == fo / co, compact: wpart[chunk, B, ci, co].
#include "rel_common.h"

namespace tsamd {
namespace {

// first element of K that the output columns from n0 on need, rounded down to the packet
__host__ __device__ inline int rel_window_lo(int n0, int kb, int nb, int vec) { return kb * (n0 / nb) / vec * vec; }
// one past the last element of K that the output columns below n1 need
__host__ __device__ inline int rel_window_hi(int n1, int kb, int nb) { return kb * ((n1 - 1) / nb + 1); }

static inline bool rel_blocks_sizes(int64_t P, int64_t R, int64_t B, int64_t ci, int64_t co) {
  return B >= 1 && ci >= 1 && co >= 1 && B <= kRelMaxWidth && ci <= kRelMaxWidth && co <= kRelMaxWidth &&
         rel_sizes(P, R, B * ci, B * co);
}

// ---------------------------------------------------------------------------------------------------------------------
// weights -> [R, N, Kw]: the window of every row's tile, zeros off the row's diagonal block
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void rel_pack_blocks_weight(const T *__restrict__ w, T *__restrict__ wp, int64_t total, int B, int kb, int nb,
                                       int TN, int Kw, int transposed) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int N = B * nb;
  const int j = (int)(o % Kw), n = (int)(o / Kw % N), b = n / nb;
  const int64_t g = o / Kw / N;
  const int kk = rel_window_lo(n / TN * TN, kb, nb, VEC) + j - b * kb;  // index inside block b
  T v{};
  if (kk >= 0 && kk < kb) {
    const int64_t q = (g * B + b) * kb * nb;
    v = transposed ? w[q + (int64_t)(n - b * nb) * kb + kk] : w[q + (int64_t)kk * nb + (n - b * nb)];
  }
  wp[o] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernel 1: gather - windowed GEMM - scatter
// ---------------------------------------------------------------------------------------------------------------------
// Wave w: items (w & 1) * 32 .. + 32, output blocks of 32 columns (w >> 1) * NB .. + NB.  Accumulator register r of a lane
// is output column 8 * (r / 4) + 4 * (lane / 32) + r % 4 of the block, for item lane % 32.
template <typename T, int NB>
__global__ __launch_bounds__(kRelThreads) void rel_blocks_gemm_kernel(
    const T *__restrict__ src, int64_t n_src, bool vec_src, const int64_t *__restrict__ src_idx,
    const int64_t *__restrict__ dst_idx, const RelUnit *__restrict__ table, const T *__restrict__ wp, int Kw,
    const float *__restrict__ dst_scale, float *__restrict__ out, int64_t n_dst, bool vec_out, int K, int N, int kb,
    int nb) {
  constexpr int TN = 64 * NB;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int KS = kRelSliceBytes / sizeof(T);
  constexpr int CH = 32 / sizeof(T);  // elements of K per matrix-instruction packet pair
  constexpr int BPT = TN / 32;        // weight packets per thread and slice
  __shared__ __attribute__((aligned(16))) unsigned char lds_a[kRelTM * kRelLdsRow];
  __shared__ __attribute__((aligned(16))) unsigned char lds_b[TN * kRelLdsRow];

  const RelUnit u = table[blockIdx.x];
  if (u.g < 0) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
  const int n0 = (int)blockIdx.y * TN, n1 = n0 + TN < N ? n0 + TN : N;
  const int kw0 = rel_window_lo(n0, kb, nb, VEC), kw1 = rel_window_hi(n1, kb, nb), len = kw1 - kw0;

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
    const int n = n0 + prow + 32 * s;
    brow[s] = n < N ? wp + ((int64_t)u.g * N + n) * Kw : nullptr;
  }
  uint4 ra[2], rb[BPT];
  auto fetch = [&](int j0) {
    const int j = j0 + pk * VEC;
#pragma unroll
    for (int s = 0; s < 2; ++s) ra[s] = rel_load_packet(arow[s], kw0 + j, kw1, vec_src);
#pragma unroll
    for (int s = 0; s < BPT; ++s) rb[s] = rel_load_packet(brow[s], j, Kw, true);
  };

  // the windows of this wave's own column blocks, relative to kw0; an empty one for a block past N
  const int ib = wave & 1, nb0 = (wave >> 1) * NB;
  int wlo[NB], whi[NB];
  f32x16 acc[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x) {
    const int c0 = n0 + (nb0 + x) * 32, c1 = c0 + 32 < N ? c0 + 32 : N;
    wlo[x] = whi[x] = 0;
    if (c0 < N) {
      wlo[x] = kb * (c0 / nb) - kw0;
      whi[x] = rel_window_hi(c1, kb, nb) - kw0;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
  }

  fetch(0);
  for (int j0 = 0; j0 < len; j0 += KS) {
#pragma unroll
    for (int s = 0; s < 2; ++s) *reinterpret_cast<uint4 *>(&lds_a[(prow + 32 * s) * kRelLdsRow + pk * 16]) = ra[s];
#pragma unroll
    for (int s = 0; s < BPT; ++s) *reinterpret_cast<uint4 *>(&lds_b[(prow + 32 * s) * kRelLdsRow + pk * 16]) = rb[s];
    __syncthreads();
    if (j0 + KS < len) fetch(j0 + KS);
#pragma unroll
    for (int x = 0; x < NB; ++x) {
      // the chunks of this slice that meet the block's window: a range, the same for every lane of the wave
      const int lo = wlo[x] - j0, hi = whi[x] - j0;
      const int ca = lo > 0 ? lo / CH : 0, cb = hi < KS ? (hi + CH - 1) / CH : KS / CH;
#pragma unroll 1
      for (int c = ca; c < cb; ++c) {
        const int off = c * 32 + kh * 16;
        const uint4 item = *reinterpret_cast<const uint4 *>(&lds_a[(ib * 32 + li) * kRelLdsRow + off]);
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
      const int n = n0 + (nb0 + x) * 32 + 8 * rq + 4 * kh;
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
// kernel 2: per-group weight gradient, the tiles on the diagonal
// ---------------------------------------------------------------------------------------------------------------------
// 8 bf16 of column c, rows it .. it + 7 of an item-major LDS slice
__device__ inline uint4 rel_blocks_column8(const unsigned char *base, int row_bytes, int it, int c) {
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

// row tiles of [F, Fo] that the column tile from fo0 on can need: the longest range over the column tiles
static inline int rel_blocks_span(int Fo, int tfo, int ci, int co) {
  int span = 1;
  for (int fo0 = 0; fo0 < Fo; fo0 += tfo) {
    const int fo1 = fo0 + tfo < Fo ? fo0 + tfo : Fo;
    const int s = (rel_window_hi(fo1, ci, co) - 1) / kRelTF - ci * (fo0 / co) / kRelTF + 1;
    if (s > span) span = s;
  }
  return span;
}

// A wave owns up to NB of the tile's 32 x 32 blocks on the diagonal.  Accumulator register r of a lane is row
// 8 * (r / 4) + 4 * (lane / 32) + r % 4, column lane % 32 of its block.
template <typename T, int NB>
__global__ __launch_bounds__(kRelThreads) void rel_blocks_wgrad_kernel(
    const T *__restrict__ h, int64_t n_h, bool vec_h, const int64_t *__restrict__ h_idx, const T *__restrict__ go,
    int64_t n_go, bool vec_go, const int64_t *__restrict__ go_idx, const RelUnit *__restrict__ table,
    float *__restrict__ wpart, int F, int Fo, int ci, int co, int span) {
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
  // the column tile, and the row tile number blockIdx.y % span of the rows its diagonal blocks cover
  const int fo0 = (int)blockIdx.y / span * TFO, fo1 = fo0 + TFO < Fo ? fo0 + TFO : Fo;
  const int f0 = (ci * (fo0 / co) / kRelTF + (int)blockIdx.y % span) * kRelTF;
  if (f0 >= rel_window_hi(fo1, ci, co)) return;

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

  // The 32 x 32 blocks of the tile that hold an element of the diagonal, in the order s = 2 * column block + row
  // half, are dealt to the four waves in turn: a wave with a fixed block would idle wherever its block is off the
  // diagonal.  sub[x]: the x-th block of this wave, -1 for none.
  const int me = __builtin_amdgcn_readfirstlane(wave);
  int sub[NB];
  f32x16 acc[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x) {
    sub[x] = -1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
  }
  int rank = 0;
#pragma unroll
  for (int s = 0; s < 4 * NB; ++s) {
    const int ra = f0 + (s & 1) * 32, rb = ra + 32 < F ? ra + 32 : F;
    const int ca = fo0 + (s >> 1) * 32, cb = ca + 32 < Fo ? ca + 32 : Fo;
    if (ra >= F || ca >= Fo) continue;
    const int lo = ra / ci > ca / co ? ra / ci : ca / co, hi = (rb - 1) / ci < (cb - 1) / co ? (rb - 1) / ci : (cb - 1) / co;
    if (lo > hi) continue;
#pragma unroll
    for (int x = 0; x < NB; ++x)
      if (rank == 4 * x + me) sub[x] = s;
    ++rank;
  }

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
#pragma unroll
    for (int x = 0; x < NB; ++x) {
      if (sub[x] < 0) continue;
      const int hc = (sub[x] & 1) * 32 + li, gc = (sub[x] >> 1) * 32 + li;  // this lane's column of either slice
      if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int kk = 0; kk < kRelKI / 2; ++kk) {
          const int it = kk * 2 + kh;
          const float a = *reinterpret_cast<const float *>(&lds_h[it * HROW + hc * 4]);
          const float b = *reinterpret_cast<const float *>(&lds_g[it * GROW + gc * 4]);
          acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[x], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < kRelKI / 16; ++ks) {
          const int it = ks * 16 + kh * 8;
          const uint4 a = rel_blocks_column8(lds_h, HROW, it, hc);
          const uint4 b = rel_blocks_column8(lds_g, GROW, it, gc);
          RelMma<T>::packet(a, b, acc[x]);
        }
      }
    }
    __syncthreads();
  }

  // element (f, fo) of diagonal block b = f / ci = fo / co is word f co + (fo - b co) of the compact [B, ci, co]
  float *block = wpart + (int64_t)blockIdx.x * F * co;
#pragma unroll
  for (int x = 0; x < NB; ++x) {
    if (sub[x] < 0) continue;
    const int fo = fo0 + (sub[x] >> 1) * 32 + li, ra = f0 + (sub[x] & 1) * 32;
    if (fo >= Fo) continue;
    const int b = fo / co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = ra + 8 * (r / 4) + 4 * kh + r % 4;
      if (f >= b * ci && f < (b + 1) * ci) block[(int64_t)f * co + (fo - b * co)] = acc[x][r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------------------------------
struct RelBlocksGemmPlan {
  RelTablePlan t;
  size_t wp, bytes;
  int kb, nb, tn, Kw;
};
RelBlocksGemmPlan rel_blocks_gemm_plan(int dtype, int64_t P, int64_t R, int64_t B, int64_t ci, int64_t co) {
  RelBlocksGemmPlan p;
  const int vec = 16 / (int)dtype_size(dtype);
  p.kb = (int)ci;
  p.nb = (int)co;
  const int N = (int)B * p.nb;
  p.tn = rel_tn(N);
  p.Kw = vec;
  for (int n0 = 0; n0 < N; n0 += p.tn) {
    const int n1 = n0 + p.tn < N ? n0 + p.tn : N;
    const int len = (int)ceil_div(rel_window_hi(n1, p.kb, p.nb) - rel_window_lo(n0, p.kb, p.nb, vec), vec) * vec;
    if (len > p.Kw) p.Kw = len;
  }
  p.t = rel_table_plan(P, R, kRelTM, 0);
  p.wp = p.t.end;
  p.bytes = p.wp + align_up(dtype_size(dtype) * (size_t)(R * N * p.Kw), 256);
  return p;
}

struct RelBlocksWgradPlan {
  RelTablePlan t;
  size_t wpart, sum, bytes;
  int64_t CK;
  int tfo, span;
};
RelBlocksWgradPlan rel_blocks_wgrad_plan(int dtype, int64_t P, int64_t R, int64_t B, int64_t ci, int64_t co) {
  RelBlocksWgradPlan p;
  p.CK = rel_chunk(P);
  p.tfo = rel_tn(B * co);
  p.span = rel_blocks_span((int)(B * co), p.tfo, (int)ci, (int)co);
  p.t = rel_table_plan(P, R, p.CK, 0);
  p.wpart = p.t.end;
  p.sum = p.wpart + align_up(sizeof(float) * (size_t)(p.t.bound * B * ci * co), 256);
  // fp32 sums of the chunks before the cast (float32 sums straight into the result)
  p.bytes = p.sum + (dtype == TSAMD_F32 ? 0 : align_up(sizeof(float) * (size_t)(R * B * ci * co), 256));
  return p;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_rel_blocks_route(int dtype, int64_t P, int64_t R, int64_t B, int64_t ci, int64_t co,
                                      int64_t out[16]) {
  if (!out || P < 0 || R < 0 || B < 0 || ci < 0 || co < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_blocks_sizes(P, R, B, ci, co)) return TSAMD_ERR_UNSUPPORTED;
  const RelBlocksGemmPlan g = rel_blocks_gemm_plan(dtype, P, R, B, ci, co);
  const RelBlocksWgradPlan w = rel_blocks_wgrad_plan(dtype, P, R, B, ci, co);
  out[0] = kRelTM;
  out[1] = g.tn;
  out[2] = kRelSliceBytes / (int64_t)dtype_size(dtype);
  out[3] = g.t.bound;
  out[4] = 32;
  out[5] = 32;
  out[6] = dtype == TSAMD_F32 ? 2 : 16;
  out[7] = w.CK;
  out[8] = w.t.bound;
  out[9] = g.Kw;
  out[10] = ceil_div(B * co, w.tfo) * w.span;
  out[11] = w.tfo;
  out[12] = (int64_t)g.bytes;
  out[13] = (int64_t)w.bytes;
  out[14] = out[15] = 0;
  return TSAMD_OK;
}

extern "C" size_t tsamd_rel_gemm_blocks_workspace_bytes(int dtype, int64_t P, int64_t R, int64_t B, int64_t ci,
                                                        int64_t co) {
  if (!rel_dtype(dtype) || P < 0 || R < 0 || !rel_blocks_sizes(P, R, B, ci, co)) return 0;
  return rel_blocks_gemm_plan(dtype, P, R, B, ci, co).bytes;
}

extern "C" int tsamd_rel_gemm_blocks(int dtype, int transposed, const void *src, int64_t n_src, const int64_t *src_idx,
                                     const int64_t *dst_idx, const int64_t *relptr, const void *weight,
                                     const float *dst_scale, float *out, int64_t n_dst, int64_t P, int64_t R, int64_t B,
                                     int64_t ci, int64_t co, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (P < 0 || R < 0 || B < 0 || ci < 0 || co < 0 || n_src < 0 || n_dst < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_blocks_sizes(P, R, B, ci, co)) return TSAMD_ERR_UNSUPPORTED;
  if (P == 0 || R == 0) return TSAMD_OK;
  if (!src || !src_idx || !dst_idx || !relptr || !weight || !out) return TSAMD_ERR_INVALID;
  const RelBlocksGemmPlan p = rel_blocks_gemm_plan(dtype, P, R, B, ci, co);
  if (!workspace || workspace_bytes < p.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return TSAMD_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  const int st = rel_table_build(p.t, relptr, P, R, kRelTM, ws, stream);
  if (st != TSAMD_OK) return st;
  const int K = (int)B * p.kb, N = (int)B * p.nb;
  const bool vec_src = aligned16(src) && (K * (int64_t)dtype_size(dtype)) % 16 == 0;
  const bool vec_out = aligned16(out) && N % 4 == 0;
  const RelUnit *table = reinterpret_cast<const RelUnit *>(ws + p.t.table);
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    T *wp = reinterpret_cast<T *>(ws + p.wp);
    const int64_t total = R * N * p.Kw;
    hipLaunchKernelGGL((rel_pack_blocks_weight<T>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const T *>(weight), wp, total, (int)B, p.kb, p.nb, p.tn, p.Kw, transposed ? 1 : 0);
    TSAMD_LAUNCH_CHECK();
    const dim3 grid((unsigned)p.t.bound, (unsigned)ceil_div(N, p.tn));
    if (p.tn == 64)
      hipLaunchKernelGGL((rel_blocks_gemm_kernel<T, 1>), grid, dim3(kRelThreads), 0, stream,
                         reinterpret_cast<const T *>(src), n_src, vec_src, src_idx, dst_idx, table, wp, p.Kw, dst_scale, out,
                         n_dst, vec_out, K, N, p.kb, p.nb);
    else
      hipLaunchKernelGGL((rel_blocks_gemm_kernel<T, 2>), grid, dim3(kRelThreads), 0, stream,
                         reinterpret_cast<const T *>(src), n_src, vec_src, src_idx, dst_idx, table, wp, p.Kw, dst_scale, out,
                         n_dst, vec_out, K, N, p.kb, p.nb);
    TSAMD_LAUNCH_CHECK();
    return TSAMD_OK;
  };
  return dtype == TSAMD_F32 ? run(float{}) : run(bf16_t{});
}

extern "C" size_t tsamd_rel_wgrad_blocks_workspace_bytes(int dtype, int64_t P, int64_t R, int64_t B, int64_t ci,
                                                         int64_t co) {
  if (!rel_dtype(dtype) || P < 0 || R < 0 || !rel_blocks_sizes(P, R, B, ci, co)) return 0;
  return rel_blocks_wgrad_plan(dtype, P, R, B, ci, co).bytes;
}

extern "C" int tsamd_rel_wgrad_blocks(int dtype, const void *h, int64_t n_h, const int64_t *h_idx, const void *go,
                                      int64_t n_go, const int64_t *go_idx, const int64_t *relptr, void *grad_weight,
                                      int64_t P, int64_t R, int64_t B, int64_t ci, int64_t co, void *workspace,
                                      size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (P < 0 || R < 0 || B < 0 || ci < 0 || co < 0 || n_h < 0 || n_go < 0) return TSAMD_ERR_INVALID;
  if (!rel_dtype(dtype) || !rel_blocks_sizes(P, R, B, ci, co)) return TSAMD_ERR_UNSUPPORTED;
  if (R == 0) return TSAMD_OK;
  if (!relptr || !grad_weight || (P > 0 && (!h || !h_idx || !go || !go_idx))) return TSAMD_ERR_INVALID;
  const RelBlocksWgradPlan p = rel_blocks_wgrad_plan(dtype, P, R, B, ci, co);
  if (!workspace || workspace_bytes < p.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return TSAMD_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  int st = rel_table_build(p.t, relptr, P, R, p.CK, ws, stream);
  if (st != TSAMD_OK) return st;
  const RelUnit *table = reinterpret_cast<const RelUnit *>(ws + p.t.table);
  float *wpart = reinterpret_cast<float *>(ws + p.wpart);
  const int F = (int)(B * ci), Fo = (int)(B * co);
  const int64_t esize = (int64_t)dtype_size(dtype);
  const bool vec_h = aligned16(h) && (F * esize) % 16 == 0, vec_go = aligned16(go) && (Fo * esize) % 16 == 0;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    if (P > 0) {
      const dim3 grid((unsigned)p.t.bound, (unsigned)(ceil_div(Fo, p.tfo) * p.span));
      if (p.tfo == 64)
        hipLaunchKernelGGL((rel_blocks_wgrad_kernel<T, 1>), grid, dim3(kRelThreads), 0, stream,
                           reinterpret_cast<const T *>(h), n_h, vec_h, h_idx, reinterpret_cast<const T *>(go), n_go, vec_go,
                           go_idx, table, wpart, F, Fo, (int)ci, (int)co, p.span);
      else
        hipLaunchKernelGGL((rel_blocks_wgrad_kernel<T, 2>), grid, dim3(kRelThreads), 0, stream,
                           reinterpret_cast<const T *>(h), n_h, vec_h, h_idx, reinterpret_cast<const T *>(go), n_go, vec_go,
                           go_idx, table, wpart, F, Fo, (int)ci, (int)co, p.span);
      TSAMD_LAUNCH_CHECK();
    }
    // a group's chunks in ascending order; a group without items is an empty segment: zeros
    const bool direct = std::is_same<T, float>::value;
    float *sum = direct ? static_cast<float *>(grad_weight) : reinterpret_cast<float *>(ws + p.sum);
    st = tsamd_segment_reduce(TSAMD_F32, TSAMD_SUM, wpart, nullptr, reinterpret_cast<const int64_t *>(ws + p.t.uptr), R,
                              B * ci * co, sum, stream_);
    if (st != TSAMD_OK) return st;
    if (!direct) {
      const int64_t n = R * B * ci * co;
      hipLaunchKernelGGL((rel_cast_from_f32<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, stream, sum,
                         static_cast<T *>(grad_weight), n);
      TSAMD_LAUNCH_CHECK();
    }
    return TSAMD_OK;
  };
  return dtype == TSAMD_F32 ? run(float{}) : run(bf16_t{});
}
