// HGT budget sampling on gfx950 (hgt_sample; the reference has it on the CPU only, csrc/cpu/hgt_sample_cpu.cpp:
// one hash map id -> float per node type, torch::multinomial for the draw).
// State of a node type, alive for the whole call: ONE 64-bit word per id of the type's id space
//     0            untouched
//     all-ones     seen (listed in the output)
//     otherwise    the budget in fixed point, units of 2^-32
// and a list of the ids whose word ever left 0 (the candidates), its length in a device counter.
//   * budget update: one lane per draw of a tsamd_sample_plan / _draw pair with k = 50 (the whole column in stored order
//     when it has at most 50 entries, else 50 distinct uniform entries): an unseen source receives floor(2^32 / c), c =
//     number of draws of the column, with ONE returning 64-bit integer atomic; the lane that finds 0 appends the id to
//     the candidate list.  Integer sums do not depend on the order of arrival, so the budgets -- and with them every
//     later draw -- are a pure function of the seed (a float atomic sum is not).
//   * selection: sequential draws without replacement with probability proportional to budget^2 have the law of an
//     EXPONENTIAL RACE: candidate v gets key = -log(u_v) / budget_v^2 with u_v uniform in (0, 1], the k smallest keys
//     win, in ascending order.  u_v = Philox(seed, v, hop, type tag) depends on the id and not on the position in the
//     (arbitrarily ordered) candidate list; keys are rounded to float32, whose bits order like the numbers, and equal
//     keys are ordered by id: (key bits, id) goes through the stable radix sort as (row, col).  Candidates drawn in an
//     earlier hop stay in the list as dead entries (word = seen) and sort behind every live one.  The type tag rides on
//     top of the key bits, so the candidates of ALL types of a hop can share one sort (the sort is bound by its
//     launches at mini-batch sizes): type t's winners are then the first k_t entries of its segment.
#include "common.h"
#include "philox.h"

namespace tsamd {
namespace {

constexpr uint64_t kSeen = ~0ull;
constexpr uint32_t kDeadKey = 0xFFFFFFFFu;  // above the bits of every finite float

__global__ void hgt_seen_kernel(const int64_t *__restrict__ ids, int64_t n, int64_t M, uint64_t *__restrict__ word,
                                unsigned long long *err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = ids[i];
  if (v < 0 || v >= M) {
    atomicAdd(err, 1ull);
    return;
  }
  word[v] = kSeen;
}

// ids outside [0, M) are counted and replaced by 0, so that what follows reads in bounds
__global__ void hgt_check_ids_kernel(int64_t *__restrict__ ids, int64_t n, int64_t M, unsigned long long *err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = ids[i];
  if (v < 0 || v >= M) {
    atomicAdd(err, 1ull);
    ids[i] = 0;
  }
}

// one lane per (frontier node i, draw j), j < TSAMD_HGT_MAX_NEIGHBORS; state = (length of the candidate list, #errors)
__global__ void hgt_budget_add_kernel(const int64_t *__restrict__ out_ptr, int64_t F, const int64_t *__restrict__ nbr,
                                      int64_t M, uint64_t *__restrict__ word, int64_t *__restrict__ cand,
                                      int64_t capacity, unsigned long long *state) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= F * TSAMD_HGT_MAX_NEIGHBORS) return;
  const int64_t i = t / TSAMD_HGT_MAX_NEIGHBORS, j = t - i * TSAMD_HGT_MAX_NEIGHBORS;
  const int64_t o = out_ptr[i], c = out_ptr[i + 1] - o;
  if (j >= c || c > TSAMD_HGT_MAX_NEIGHBORS) return;
  const int64_t v = nbr[o + j];
  if (v < 0 || v >= M) {
    atomicAdd(state + 1, 1ull);
    return;
  }
  if (word[v] == kSeen) return;  // (nothing turns seen while this kernel runs)
  const unsigned long long add = (1ull << 32) / (unsigned long long)c;
  const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long *>(&word[v]), add);
  if (old == 0) {
    const unsigned long long p = atomicAdd(state, 1ull);
    if ((int64_t)p < capacity) cand[p] = v;
    else atomicAdd(state + 1, 1ull);
  }
}

__global__ void hgt_keys_kernel(const int64_t *__restrict__ cand, int64_t C, const uint64_t *__restrict__ word, int64_t M,
                                uint64_t seed, uint32_t hop, uint32_t tag, int64_t *__restrict__ key,
                                int64_t *__restrict__ id) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= C) return;
  const int64_t v = cand[p];
  uint32_t bits = kDeadKey;
  if (v >= 0 && v < M) {
    const uint64_t w = word[v];
    if (w != kSeen && w != 0) {
      const U4 r = philox(seed, (uint64_t)v, hop, 0x4847u ^ (tag << 16));
      const double u = (double)((u64(r.x, r.y) >> 11) + 1ull) * 0x1.0p-53;  // (0, 1]
      const double b = (double)w * 0x1.0p-32;
      bits = __float_as_uint((float)(-log(u) / (b * b)));  // >= +0: the bits order like the numbers
    }
  }
  key[p] = (int64_t)(((uint64_t)tag << 32) | bits);  // the type tag on top: several types can share one sort
  id[p] = (v >= 0 && v < M) ? v : 0;
}

// the k first entries of the sorted (key, id) list are the winners, in draw order
__global__ void hgt_commit_kernel(const int64_t *__restrict__ key_s, const int64_t *__restrict__ id_s, int64_t k,
                                  uint64_t *__restrict__ word, int64_t M, int64_t tag, int64_t *__restrict__ out,
                                  unsigned long long *err) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= k) return;
  const int64_t v = id_s[p];
  // the caller asked for more than the live candidates, or points at another type's segment
  if ((uint32_t)key_s[p] == kDeadKey || (key_s[p] >> 32) != tag || v < 0 || v >= M) {
    atomicAdd(err, 1ull);
    out[p] = -1;
    return;
  }
  out[p] = v;
  word[v] = kSeen;
}

struct SelectCarve {
  int64_t *key, *id, *key_s, *id_s, *perm;
  void *sort_ws;
  size_t sort_bytes, total;
};

SelectCarve select_carve(void *workspace, int64_t C) {
  SelectCarve c;
  char *p = reinterpret_cast<char *>(workspace);
  const size_t arr = align_up(sizeof(int64_t) * (size_t)(C > 0 ? C : 1), 256);
  c.key = reinterpret_cast<int64_t *>(p);
  c.id = reinterpret_cast<int64_t *>(p + arr);
  c.key_s = reinterpret_cast<int64_t *>(p + 2 * arr);
  c.id_s = reinterpret_cast<int64_t *>(p + 3 * arr);
  c.perm = reinterpret_cast<int64_t *>(p + 4 * arr);
  c.sort_ws = p + 5 * arr;
  c.sort_bytes = tsamd_sort_coo_workspace_bytes(C);
  c.total = 5 * arr + c.sort_bytes;
  return c;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_hgt_seen(const int64_t *ids, int64_t n, int64_t M, uint64_t *word, int64_t *err, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (n < 0 || M < 0 || !err || (n > 0 && !ids) || (M > 0 && !word)) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  hipLaunchKernelGGL(hgt_seen_kernel, dim3((unsigned int)ceil_div(n, 256)), dim3(256), 0, stream, ids, n, M, word,
                     reinterpret_cast<unsigned long long *>(err));
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_hgt_check_ids(int64_t *ids, int64_t n, int64_t M, int64_t *err, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (n < 0 || M < 0 || !err || (n > 0 && !ids)) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  hipLaunchKernelGGL(hgt_check_ids_kernel, dim3((unsigned int)ceil_div(n, 256)), dim3(256), 0, stream, ids, n, M,
                     reinterpret_cast<unsigned long long *>(err));
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_hgt_budget_add(const int64_t *out_ptr, int64_t F, const int64_t *nbr, int64_t M, uint64_t *word,
                                    int64_t *cand, int64_t capacity, int64_t *state, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (F < 0 || M < 0 || capacity < 0 || !state) return TSAMD_ERR_INVALID;
  if (F == 0) return TSAMD_OK;
  if (!out_ptr || !nbr || (M > 0 && !word) || (capacity > 0 && !cand)) return TSAMD_ERR_INVALID;
  const int64_t lanes = F * TSAMD_HGT_MAX_NEIGHBORS;
  hipLaunchKernelGGL(hgt_budget_add_kernel, dim3((unsigned int)ceil_div(lanes, 256)), dim3(256), 0, stream, out_ptr, F,
                     nbr, M, word, cand, capacity, reinterpret_cast<unsigned long long *>(state));
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_hgt_keys(const int64_t *cand, int64_t C, const uint64_t *word, int64_t M, uint64_t seed, int64_t hop,
                              int64_t type_tag, int64_t *key, int64_t *id, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (C < 0 || M < 0 || type_tag < 0 || type_tag >= ((int64_t)1 << 16)) return TSAMD_ERR_INVALID;
  if (C == 0) return TSAMD_OK;
  if (!cand || !word || !key || !id) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(hgt_keys_kernel, dim3((unsigned int)ceil_div(C, 256)), dim3(256), 0, stream, cand, C, word, M, seed,
                     (uint32_t)hop, (uint32_t)type_tag, key, id);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_hgt_commit(const int64_t *key_sorted, const int64_t *id_sorted, int64_t k, uint64_t *word, int64_t M,
                                int64_t type_tag, int64_t *out, int64_t *err, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (k < 0 || M < 0 || !err) return TSAMD_ERR_INVALID;
  if (k == 0) return TSAMD_OK;
  if (!key_sorted || !id_sorted || !word || !out) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(hgt_commit_kernel, dim3((unsigned int)ceil_div(k, 256)), dim3(256), 0, stream, key_sorted, id_sorted, k,
                     word, M, type_tag, out, reinterpret_cast<unsigned long long *>(err));
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_hgt_select_workspace_bytes(int64_t C) { return select_carve(nullptr, C).total + 256; }

extern "C" int tsamd_hgt_select(const int64_t *cand, int64_t C, uint64_t *word, int64_t M, int64_t k, uint64_t seed,
                                int64_t hop, int64_t type_tag, int64_t *out, int64_t *err, void *workspace,
                                size_t workspace_bytes, void *stream_) {
  if (C < 0 || M < 0 || k < 0 || k > C || !err) return TSAMD_ERR_INVALID;
  if (k == 0) return TSAMD_OK;
  if (!cand || !word || !out) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_hgt_select_workspace_bytes(C)) return TSAMD_ERR_WORKSPACE;
  const SelectCarve c = select_carve(workspace, C);
  int st = tsamd_hgt_keys(cand, C, word, M, seed, hop, type_tag, c.key, c.id, stream_);
  if (st != TSAMD_OK) return st;
  st = tsamd_sort_coo(c.key, c.id, C, (type_tag + 1) << 32, M, c.key_s, c.id_s, c.perm, c.sort_ws, c.sort_bytes, stream_);
  if (st != TSAMD_OK) return st;
  return tsamd_hgt_commit(c.key_s, c.id_s, k, word, M, type_tag, out, err, stream_);
}
