// What the two relational units share (rel_gemm.hip: dense weight blocks, rel_blocks.hip: block-diagonal ones): the
// tile constants, the unit table over relation groups, the 16-byte operand packets and the matrix instructions
// (docs/design/widening.md, "Relational SpMM").  Everything sits in an anonymous namespace: each unit gets its own copy.
#pragma once
#include "common.h"
#include "scan.h"

namespace tsamd {
namespace {

constexpr int kRelThreads = 256;
constexpr int kRelTM = 64;         // items per tile of rel_gemm
constexpr int kRelSliceBytes = 128;  // bytes of K per staged slice
constexpr int kRelLdsRow = kRelSliceBytes + 16;
constexpr int kRelKI = 32;         // items per LDS slice of rel_wgrad
constexpr int kRelTF = 64;         // rows of [F, Fo] per block of rel_wgrad
constexpr int64_t kRelMaxWidth = 512;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct RelUnit {
  int64_t start;  // first item
  int32_t g;      // group, -1: no unit in this slot
  int32_t n;      // items, 1 .. unit
};

static inline int rel_tn(int64_t N) { return N <= 64 ? 64 : 128; }
static inline int64_t rel_chunk(int64_t P) {
  const int64_t ck = ceil_div(P, 1024) > 256 ? ceil_div(P, 1024) : 256;
  return ceil_div(ck, kRelKI) * kRelKI;
}
static inline bool rel_dtype(int dtype) { return dtype == TSAMD_F32 || dtype == TSAMD_BF16; }
static inline bool rel_sizes(int64_t P, int64_t R, int64_t K, int64_t N) {
  const int64_t lim = 2147483647;
  return K >= 1 && K <= kRelMaxWidth && N >= 1 && N <= kRelMaxWidth && P < lim && R < lim && P / kRelTM + R + 1 < lim;
}

// ---------------------------------------------------------------------------------------------------------------------
// the unit table
// ---------------------------------------------------------------------------------------------------------------------
__global__ void rel_unit_counts(const int64_t *__restrict__ relptr, int64_t R, int64_t unit, int64_t *__restrict__ cnt) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > R) return;
  int64_t n = 0;
  if (g < R) n = relptr[g + 1] - relptr[g];
  cnt[g] = n > 0 ? (n + unit - 1) / unit : 0;
}

__global__ void rel_unit_table(const int64_t *__restrict__ relptr, const int64_t *__restrict__ uptr, int64_t R,
                               int64_t P, int64_t unit, int64_t bound, RelUnit *__restrict__ table) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= bound) return;
  RelUnit u{0, -1, 0};
  if (b < uptr[R]) {
    int64_t lo = 0, hi = R;  // the group with uptr[g] <= b < uptr[g + 1]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (uptr[mid] <= b) lo = mid; else hi = mid;
    }
    const int64_t start = relptr[lo] + (b - uptr[lo]) * unit;
    int64_t n = relptr[lo + 1] - start;
    if (n > unit) n = unit;
    if (start >= 0 && n > 0 && start + n <= P) u = RelUnit{start, (int32_t)lo, (int32_t)n};
  }
  table[b] = u;
}

// cnt / uptr [R + 1] (scanned in place) | scan scratch | table [bound]
struct RelTablePlan {
  size_t uptr, scan, table, end;
  int64_t bound;
};
RelTablePlan rel_table_plan(int64_t P, int64_t R, int64_t unit, size_t off) {
  RelTablePlan p;
  p.bound = ceil_div(P, unit) + R;
  p.uptr = off;
  p.scan = p.uptr + align_up(sizeof(int64_t) * (size_t)(R + 1), 256);
  p.table = p.scan + align_up(scan_workspace_bytes(R + 1), 256);
  p.end = p.table + align_up(sizeof(RelUnit) * (size_t)p.bound, 256);
  return p;
}
int rel_table_build(const RelTablePlan &p, const int64_t *relptr, int64_t P, int64_t R, int64_t unit, char *ws,
                    hipStream_t stream) {
  int64_t *uptr = reinterpret_cast<int64_t *>(ws + p.uptr);
  hipLaunchKernelGGL(rel_unit_counts, dim3((unsigned)ceil_div(R + 1, 256)), dim3(256), 0, stream, relptr, R, unit, uptr);
  TSAMD_LAUNCH_CHECK();
  const int st = exclusive_scan_i64(uptr, uptr, R + 1, nullptr, ws + p.scan, stream);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(rel_unit_table, dim3((unsigned)ceil_div(p.bound, 256)), dim3(256), 0, stream, relptr, uptr, R, P,
                     unit, p.bound, reinterpret_cast<RelUnit *>(ws + p.table));
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// staging and the matrix instructions
// ---------------------------------------------------------------------------------------------------------------------
// 16 bytes of `row` from element k on; elements from K on, and a null row, are zeros.  vec: row + k is 16-byte aligned
// and K a multiple of the packet.
template <typename T>
__device__ inline uint4 rel_load_packet(const T *row, int64_t k, int64_t K, bool vec) {
  constexpr int VEC = 16 / sizeof(T);
  if (row == nullptr || k >= K) return uint4{0u, 0u, 0u, 0u};
  if (vec) return *reinterpret_cast<const uint4 *>(row + k);
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    uint32_t bits = 0;
    if (k + e < K) {
      if constexpr (sizeof(T) == 4) {
        bits = __float_as_uint(row[k + e]);
      } else {
        bits = (uint32_t)row[k + e].bits << (16 * (e & 1));
      }
    }
    const int word = e * (int)sizeof(T) / 4;
    if (word == 0) w0 |= bits;
    if (word == 1) w1 |= bits;
    if (word == 2) w2 |= bits;
    if (word == 3) w3 |= bits;
  }
  return uint4{w0, w1, w2, w3};
}

template <typename T>
struct RelMma;
template <>
struct RelMma<float> {
  // a, b: the lane's packet of the row-operand and of the column-operand; four steps
  __device__ static inline void packet(const uint4 &a, const uint4 &b, f32x16 &c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
  }
};
template <>
struct RelMma<bf16_t> {
  __device__ static inline void packet(const uint4 &a, const uint4 &b, f32x16 &c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

template <typename T>
__global__ void rel_cast_from_f32(const float *__restrict__ in, T *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = Traits<T>::from_acc(in[i]);
}

}  // namespace
}  // namespace tsamd
