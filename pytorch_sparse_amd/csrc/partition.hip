// Multilevel k-way graph partitioning on gfx950 (partition / partition2 / mt_partition; the reference hands these to
// METIS on the CPU, csrc/cpu/metis_cpu.cpp, and refuses device tensors, csrc/metis.cpp:21-26).  This unit holds the
// kernels of the four phases; the level loop that strings them together (and owns every allocation and read-back) is
// the host driver in ops_partition.cpp, docs/design/partition.md has the scheme.
//   working graph   symmetric CSR (rowptr, row, col, w) with int64 edge weights, no self-loops, no duplicates, and
//                   int64 vertex weights vw
//   matching        handshake rounds: every unmatched vertex proposes to its heaviest unmatched neighbour under the
//                   weight cap -- ties by hash(round, neighbour id), then by the smaller id -- mutual proposals match
//   contraction     (cmap[r], cmap[c], w) with r == c parked on a sentinel key, then the existing sort + coalesce and
//                   an int64 segment sum
//   initial         level-synchronous pull BFS (one packed (component, level) word per vertex), sort by (component,
//                   level, id), scan of the vertex weights, part = floor((prefix + w / 2) k / W)
//   refinement      synchronous rounds: connectivity of every vertex to its adjacent parts -- those of positive
//                   connectivity; zero-weight edges alone do not make a part adjacent -- (short rows: a lane and a
//                   short loop; longer rows: a wave and a 128-slot LDS hash; rows that overflow it: a dense per-workgroup
//                   table of k counters in global scratch), a recount of the gain against the neighbours that move first,
//                   and a commit by sort + segmented prefix sum -- no cursor atomics
// Every atomic in this file is an integer add / min / a flag store whose result does not depend on the order of
// arrival, so a call is reproducible bit for bit.
#include "common.h"

namespace tsamd {
namespace {

constexpr int kLaneRow = 32;           // rows up to this length: one lane per row
constexpr int kSlots = 128;            // LDS hash slots of a wave-per-row vertex
constexpr int kSlotBits = 7;
constexpr int kSpillBlocks = 64;       // workgroups (and dense tables) of the spill kernel
constexpr int64_t kGainClamp = (int64_t)1 << 40;
constexpr int64_t kIdBits = 31;

__device__ inline int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline dim3 grid_for(int64_t n, int block = 256) { return dim3((unsigned int)ceil_div(n > 0 ? n : 1, block)); }

__device__ inline void add_i64(int64_t *p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
__device__ inline void min_i64(int64_t *p, int64_t v) { atomicMin(reinterpret_cast<long long *>(p), (long long)v); }

__device__ inline uint32_t tie_hash(uint32_t round, uint32_t id) {
  uint32_t x = round * 0x9E3779B1u + id * 0x85EBCA77u;
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  x *= 0x297A2D39u;
  x ^= x >> 15;
  return x;
}

__global__ void fill_kernel(int64_t *p, int64_t n, int64_t v) {
  const int64_t i = gid();
  if (i < n) p[i] = v;
}

// ---- working graph / contraction ------------------------------------------------------------------------------------
// entry e of (row, col, w) -> slot e (and, mirror, its transpose -> slot E + e) of the relabelled list; a self-loop goes
// to the sentinel key (n_key, 0) with weight 0.  info[0..1] += low / high 32 bits of the kept weights, info[2] +=
// negative weights, info[3] += parked entries.
__global__ void edges_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                             const int64_t *__restrict__ w, const int64_t *__restrict__ cmap, int64_t E, int64_t n,
                             int64_t n_key, int mirror, int64_t *__restrict__ r_out, int64_t *__restrict__ c_out,
                             int64_t *__restrict__ w_out, int64_t *__restrict__ info) {
  const int64_t e = gid();
  if (e >= E) return;
  int64_t r = row[e], c = col[e];
  int64_t x = w ? w[e] : 1;
  const bool bad = r < 0 || r >= n || c < 0 || c >= n || x < 0;
  if (bad) add_i64(info + 2, 1);
  if (!bad && cmap) {
    r = cmap[r];
    c = cmap[c];
  }
  const bool park = bad || r == c;
  if (park) {
    r = n_key;
    c = 0;
    x = 0;
    add_i64(info + 3, mirror ? 2 : 1);
  } else {
    const uint64_t u = (uint64_t)x;
    add_i64(info + 0, (int64_t)((u & 0xFFFFFFFFull) * (mirror ? 2 : 1)));
    add_i64(info + 1, (int64_t)((u >> 32) * (mirror ? 2 : 1)));
  }
  r_out[e] = r;
  c_out[e] = c;
  w_out[e] = x;
  if (mirror) {
    r_out[E + e] = park ? r : c;
    c_out[E + e] = park ? c : r;
    w_out[E + e] = x;
  }
}

__global__ void vertex_weights_kernel(const int64_t *__restrict__ vw, const int64_t *__restrict__ cmap, int64_t n,
                                      int64_t n_c, int64_t *__restrict__ vw_c) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t c = cmap[v];
  if (c >= 0 && c < n_c) add_i64(vw_c + c, vw[v]);
}

// ---- matching -------------------------------------------------------------------------------------------------------
struct Prop {
  int64_t w;
  uint32_t h;
  int64_t id;  // -1: none
};
__device__ inline bool prop_better(const Prop &a, const Prop &b) {  // a beats b
  if (a.id < 0) return false;
  if (b.id < 0) return true;
  if (a.w != b.w) return a.w > b.w;
  if (a.h != b.h) return a.h > b.h;
  return a.id < b.id;
}
__device__ inline void prop_edge(Prop &best, int64_t v, int64_t u, int64_t x, const int64_t *match, const int64_t *vw,
                                 int64_t vwv, int64_t capw, uint32_t round, int64_t n) {
  if (u == v || u < 0 || u >= n || match[u] >= 0 || vwv + vw[u] > capw) return;
  Prop p{x, tie_hash(round, (uint32_t)u), u};
  if (prop_better(p, best)) best = p;
}

__global__ void propose_lane_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col,
                                    const int64_t *__restrict__ w, const int64_t *__restrict__ vw,
                                    const int64_t *__restrict__ match, int64_t n, int64_t capw, uint32_t round,
                                    int64_t *__restrict__ prop) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (e - b > kLaneRow) return;  // the wave kernel's row
  Prop best{0, 0, -1};
  if (match[v] < 0) {
    const int64_t vwv = vw[v];
    for (int64_t j = b; j < e; ++j) prop_edge(best, v, col[j], w[j], match, vw, vwv, capw, round, n);
  }
  prop[v] = best.id;
}

// one wave (= one workgroup of 64) per row longer than kLaneRow
__global__ void __launch_bounds__(64) propose_wave_kernel(const int64_t *__restrict__ rowptr,
                                                           const int64_t *__restrict__ col,
                                                           const int64_t *__restrict__ w,
                                                           const int64_t *__restrict__ vw,
                                                           const int64_t *__restrict__ match, int64_t n, int64_t capw,
                                                           uint32_t round, int64_t *__restrict__ prop) {
  const int64_t v = blockIdx.x;
  if (v >= n) return;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (e - b <= kLaneRow) return;
  Prop best{0, 0, -1};
  if (match[v] < 0) {
    const int64_t vwv = vw[v];
    for (int64_t j = b + threadIdx.x; j < e; j += 64) prop_edge(best, v, col[j], w[j], match, vw, vwv, capw, round, n);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    Prop o;
    o.w = __shfl_xor((long long)best.w, off);
    o.h = (uint32_t)__shfl_xor((int)best.h, off);
    o.id = __shfl_xor((long long)best.id, off);
    if (prop_better(o, best)) best = o;
  }
  if (threadIdx.x == 0) prop[v] = best.id;
}

__global__ void handshake_kernel(const int64_t *__restrict__ prop, int64_t n, int64_t *__restrict__ match) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t u = prop[v];
  if (u >= 0 && match[v] < 0 && prop[u] == v) match[v] = u;  // (match[v] is written by lane v alone)
}

__global__ void leader_kernel(const int64_t *__restrict__ match, int64_t n, int64_t *__restrict__ flag) {
  const int64_t v = gid();
  if (v < n) flag[v] = (match[v] < 0 || v < match[v]) ? 1 : 0;
}
__global__ void cmap_kernel(const int64_t *__restrict__ match, const int64_t *__restrict__ rank, int64_t n,
                            int64_t *__restrict__ cmap) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t u = match[v];
  cmap[v] = (u < 0 || v < u) ? rank[v] : rank[u];
}

// ---- initial partition ----------------------------------------------------------------------------------------------
// cl[v] = component << 31 | level once visited, -1 before.  state: [0] min (degree << 31 | id) over the vertices with
// edges, [1] smallest unvisited id, [2] 1 = the seed kernel found a start, [3] 1 = the last step added a vertex.
constexpr int64_t kNone = 0x7FFFFFFFFFFFFFFFll;

__global__ void bfs_init_kernel(const int64_t *__restrict__ rowptr, int64_t n, int64_t *__restrict__ cl,
                                int64_t *__restrict__ state) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t d = rowptr[v + 1] - rowptr[v];
  if (d == 0) {
    cl[v] = n << kIdBits;  // isolated vertices: one last "component", nothing to search
  } else {
    cl[v] = -1;
    min_i64(state + 0, (d << kIdBits) | v);
  }
}
__global__ void bfs_unvisited_kernel(const int64_t *__restrict__ cl, int64_t n, int64_t *__restrict__ state) {
  const int64_t v = gid();
  if (v < n && cl[v] < 0) min_i64(state + 1, v);
}
__global__ void bfs_seed_kernel(int64_t *__restrict__ cl, int64_t n, int64_t comp, int first,
                                int64_t *__restrict__ state) {
  if (gid() != 0) return;
  const int64_t key = first ? state[0] : state[1];
  const int64_t s = key == kNone ? -1 : (first ? (key & (((int64_t)1 << kIdBits) - 1)) : key);
  if (s >= 0 && s < n) {
    cl[s] = comp << kIdBits;
    state[2] = 1;
  } else {
    state[2] = 0;
  }
  state[1] = kNone;
  state[3] = 0;
}
// pull step: an unvisited vertex with a neighbour at (comp, level) joins at level + 1.  The packed word makes the test
// and the update one 64-bit access each, so a vertex that joins in this launch is never mistaken for a frontier vertex.
__global__ void bfs_step_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col, int64_t n,
                                int64_t *cl, int64_t comp, int64_t level, int64_t *__restrict__ state) {
  const int64_t v = gid();
  if (v >= n) return;
  if (__hip_atomic_load(cl + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) return;
  const int64_t want = (comp << kIdBits) | level;
  for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) {
    const int64_t u = col[j];
    if (u < 0 || u >= n) continue;
    if (__hip_atomic_load(cl + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want) {
      __hip_atomic_store(cl + v, want + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      state[3] = 1;
      return;
    }
  }
}
__global__ void bfs_keys_kernel(const int64_t *__restrict__ cl, int64_t n, int64_t *__restrict__ comp,
                                int64_t *__restrict__ level) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t x = cl[v] < 0 ? (n << kIdBits) : cl[v];
  comp[v] = x >> kIdBits;
  level[v] = x & (((int64_t)1 << kIdBits) - 1);
}
// position i of the (component, level, id) order: part = min(k - 1, floor((2 prefix + w) k / (2 W)))
__global__ void assign_kernel(const int64_t *__restrict__ perm, const int64_t *__restrict__ w_sorted,
                              const int64_t *__restrict__ prefix, const int64_t *__restrict__ total, int64_t n,
                              int64_t k, int64_t *__restrict__ part) {
  const int64_t i = gid();
  if (i >= n) return;
  const int64_t W = *total;
  int64_t p = W > 0 ? ((2 * prefix[i] + w_sorted[i]) * k) / (2 * W) : (i * k) / n;
  if (p > k - 1) p = k - 1;
  if (p < 0) p = 0;
  const int64_t v = perm[i];
  if (v >= 0 && v < n) part[v] = p;
}

// ---- refinement -----------------------------------------------------------------------------------------------------
__global__ void part_weights_kernel(const int64_t *__restrict__ part, const int64_t *__restrict__ vw, int64_t n,
                                    int64_t k, int64_t *__restrict__ pw) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t p = part[v];
  if (p >= 0 && p < k) add_i64(pw + p, vw[v]);
}

// mode 0: destinations above the own part, 1: below, 2: any (rebalance)
__device__ inline bool eligible(int64_t p, int64_t own, int mode, const int64_t *pw, int64_t vwv, int64_t cap) {
  if (p == own) return false;
  if (mode == 0 && p < own) return false;
  if (mode == 1 && p > own) return false;
  return pw[p] + vwv <= cap;
}
// what a vertex reports: (destination or -1, gain = connectivity to it - connectivity to the own part)
__device__ inline void report(int64_t v, int64_t own, int64_t c_own, int64_t best, int64_t c_best, int mode,
                              const int64_t *pw, int64_t vwv, int64_t cap, const int64_t *lightest,
                              int64_t *dest, int64_t *gain) {
  int64_t d = best, g = best >= 0 ? c_best - c_own : 0;
  if (mode == 2) {
    if (pw[own] <= cap) {
      d = -1;
    } else if (d < 0 && lightest) {  // no adjacent part with room: the globally lightest part
      const int64_t l = *lightest;
      if (l != own && pw[l] + vwv <= cap) {
        d = l;
        g = -c_own;
      }
    }
  } else if (d >= 0 && !(g > 0 || pw[own] > cap)) {
    d = -1;
  }
  dest[v] = d;
  gain[v] = d >= 0 ? g : 0;
}
__device__ inline void better_part(int64_t &best, int64_t &c_best, int64_t p, int64_t c) {
  if (p >= 0 && (best < 0 || c > c_best || (c == c_best && p < best))) {
    best = p;
    c_best = c;
  }
}

__global__ void conn_lane_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col,
                                 const int64_t *__restrict__ w, const int64_t *__restrict__ vw,
                                 const int64_t *__restrict__ part, const int64_t *__restrict__ pw, int64_t n, int64_t k,
                                 int64_t cap, int mode, const int64_t *__restrict__ lightest,
                                 int64_t *__restrict__ dest, int64_t *__restrict__ gain) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (e - b > kLaneRow) return;
  const int64_t own = part[v], vwv = vw[v];
  int64_t c_own = 0, best = -1, c_best = 0;
  for (int64_t j = b; j < e; ++j) {
    const int64_t p = part[col[j]];
    if (p == own) {
      c_own += w[j];
      continue;
    }
    bool first = true;
    for (int64_t i = b; i < j; ++i) first = first && part[col[i]] != p;
    if (!first || !eligible(p, own, mode, pw, vwv, cap)) continue;
    int64_t c = 0;
    for (int64_t i = j; i < e; ++i) c += part[col[i]] == p ? w[i] : 0;
    if (c != 0) better_part(best, c_best, p, c);  // zero-weight edges alone make no adjacent part (as in every route)
  }
  report(v, own, c_own, best, c_best, mode, pw, vwv, cap, lightest, dest, gain);
}

__device__ inline void wave_best(int64_t &best, int64_t &c_best) {
  for (int off = 32; off >= 1; off >>= 1) {
    const int64_t ob = __shfl_xor((long long)best, off), oc = __shfl_xor((long long)c_best, off);
    better_part(best, c_best, ob, oc);
  }
}

// one wave (= one workgroup of 64) per row longer than kLaneRow: part id -> summed weight in a 128-slot LDS hash
// (ds_cmpst claims a slot, a 64-bit ds_add sums -- integer adds, any order).  A row that touches more parts than fit
// is appended to `spill` (spill_count += 1) and left to conn_spill_kernel.
__global__ void __launch_bounds__(64) conn_wave_kernel(const int64_t *__restrict__ rowptr,
                                                        const int64_t *__restrict__ col, const int64_t *__restrict__ w,
                                                        const int64_t *__restrict__ vw,
                                                        const int64_t *__restrict__ part,
                                                        const int64_t *__restrict__ pw, int64_t n, int64_t k, int64_t cap,
                                                        int mode, const int64_t *__restrict__ lightest,
                                                        int64_t *__restrict__ dest, int64_t *__restrict__ gain,
                                                        int64_t *__restrict__ spill, int64_t *__restrict__ spill_count) {
  __shared__ int key[kSlots];
  __shared__ unsigned long long val[kSlots];
  __shared__ int overflow;
  const int64_t v = blockIdx.x;
  if (v >= n) return;
  const int64_t b = rowptr[v], e = rowptr[v + 1];
  if (e - b <= kLaneRow) return;
  const int lane = threadIdx.x;
  for (int s = lane; s < kSlots; s += 64) {
    key[s] = -1;
    val[s] = 0;
  }
  if (lane == 0) overflow = 0;
  __syncthreads();
  for (int64_t j = b + lane; j < e; j += 64) {
    const int p = (int)part[col[j]];
    uint32_t h = ((uint32_t)p * 0x9E3779B1u) >> (32 - kSlotBits);
    int tries = 0;
    for (; tries < kSlots; ++tries) {
      const int old = atomicCAS(&key[h], -1, p);
      if (old == -1 || old == p) {
        atomicAdd(&val[h], (unsigned long long)w[j]);
        break;
      }
      h = (h + 1) & (kSlots - 1);
    }
    if (tries == kSlots) overflow = 1;
  }
  __syncthreads();
  if (overflow) {
    if (lane == 0) {
      const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long *>(spill_count), 1ull);
      if ((int64_t)at < n) spill[at] = v;
    }
    return;
  }
  const int64_t own = part[v], vwv = vw[v];
  int64_t c_own = 0, best = -1, c_best = 0;
  for (int s = lane; s < kSlots; s += 64) {
    const int64_t p = key[s];
    if (p < 0) continue;
    if (p == own) c_own = (int64_t)val[s];
    else if (val[s] != 0 && eligible(p, own, mode, pw, vwv, cap)) better_part(best, c_best, p, (int64_t)val[s]);
  }
  for (int off = 32; off >= 1; off >>= 1) c_own += __shfl_xor((long long)c_own, off);
  wave_best(best, c_best);
  if (lane == 0) report(v, own, c_own, best, c_best, mode, pw, vwv, cap, lightest, dest, gain);
}

// the spilled rows: workgroup g owns table[g * k .. (g + 1) * k), one counter per part, in global scratch
__global__ void __launch_bounds__(256) conn_spill_kernel(const int64_t *__restrict__ rowptr,
                                                          const int64_t *__restrict__ col,
                                                          const int64_t *__restrict__ w, const int64_t *__restrict__ vw,
                                                          const int64_t *__restrict__ part,
                                                          const int64_t *__restrict__ pw, int64_t n, int64_t k, int64_t cap,
                                                          int mode, const int64_t *__restrict__ lightest,
                                                          int64_t *__restrict__ dest, int64_t *__restrict__ gain,
                                                          const int64_t *__restrict__ spill,
                                                          const int64_t *__restrict__ spill_count, int64_t *table) {
  __shared__ int64_t s_best[4], s_cbest[4];
  int64_t count = *spill_count;
  if (count > n) count = n;
  int64_t *tab = table + (int64_t)blockIdx.x * k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = blockIdx.x; r < count; r += gridDim.x) {
    const int64_t v = spill[r];
    for (int64_t p = threadIdx.x; p < k; p += blockDim.x) __hip_atomic_store(tab + p, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int64_t b = rowptr[v], e = rowptr[v + 1];
    for (int64_t j = b + threadIdx.x; j < e; j += blockDim.x) {
      const int64_t p = part[col[j]];
      if (p >= 0 && p < k) add_i64(tab + p, w[j]);
    }
    __syncthreads();
    const int64_t own = part[v], vwv = vw[v];
    int64_t best = -1, c_best = 0;
    for (int64_t p = threadIdx.x; p < k; p += blockDim.x) {
      const int64_t c = __hip_atomic_load(tab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (c != 0 && eligible(p, own, mode, pw, vwv, cap)) better_part(best, c_best, p, c);
    }
    wave_best(best, c_best);
    if (lane == 0) {
      s_best[wave] = best;
      s_cbest[wave] = c_best;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      best = -1;
      c_best = 0;
      for (int i = 0; i < 4; ++i) better_part(best, c_best, s_best[i], s_cbest[i]);
      const int64_t c_own = __hip_atomic_load(tab + own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      report(v, own, c_own, best, c_best, mode, pw, vwv, cap, lightest, dest, gain);
    }
    __syncthreads();
  }
}

// The gain of candidate r recounted with every neighbour that moves FIRST -- a candidate of higher gain, or of equal
// gain and smaller id -- already at its destination: one lane per edge, acc[r] += w * ([c at dest r] - [c at part r]).
__global__ void recount_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                               const int64_t *__restrict__ w, const int64_t *__restrict__ part,
                               const int64_t *__restrict__ dest, const int64_t *__restrict__ gain, int64_t E,
                               int64_t *__restrict__ acc) {
  const int64_t e = gid();
  if (e >= E) return;
  const int64_t r = row[e], c = col[e];
  const int64_t dr = dest[r];
  if (dr < 0) return;
  const int64_t dc = dest[c];
  const bool first = dc >= 0 && (gain[c] > gain[r] || (gain[c] == gain[r] && c < r));
  const int64_t pc = first ? dc : part[c];
  const int64_t x = (pc == dr ? w[e] : 0) - (pc == part[r] ? w[e] : 0);
  if (x != 0) add_i64(acc + r, x);
}
__global__ void recount_filter_kernel(const int64_t *__restrict__ acc, const int64_t *__restrict__ part,
                                      const int64_t *__restrict__ pw, int64_t cap, int64_t n,
                                      int64_t *__restrict__ dest) {
  const int64_t v = gid();
  if (v >= n || dest[v] < 0) return;
  if (!(acc[v] > 0 || pw[part[v]] > cap)) dest[v] = -1;
}

// sort keys of a commit: (group or the sentinel group k, kGainClamp - gain): the best gains first, ids ascending behind
// them through the stability of the sort.  select = 0: group = destination; 1: group = own part if it is over capacity.
__global__ void commit_keys_kernel(const int64_t *__restrict__ dest, const int64_t *__restrict__ gain,
                                   const int64_t *__restrict__ part, const int64_t *__restrict__ pw, int64_t cap,
                                   int64_t n, int64_t k, int select, int64_t *__restrict__ key_row,
                                   int64_t *__restrict__ key_col) {
  const int64_t v = gid();
  if (v >= n) return;
  int64_t g = dest[v];
  if (select && g >= 0) g = pw[part[v]] > cap ? part[v] : -1;
  int64_t x = gain[v];
  x = x > kGainClamp - 1 ? kGainClamp - 1 : (x < 1 - kGainClamp ? 1 - kGainClamp : x);
  key_row[v] = g < 0 ? k : g;
  key_col[v] = g < 0 ? 0 : kGainClamp - x;
}
// position i of the sorted order: weight before it inside its group = prefix[i] - prefix[ptr[group]].
// select = 0: accepted while the group's (destination's) remaining room holds it; 1: chosen while the group's (over-weight
// part's) excess is not yet covered.  Rejected vertices lose their destination.
__global__ void accept_kernel(const int64_t *__restrict__ group_sorted, const int64_t *__restrict__ perm,
                              const int64_t *__restrict__ w_sorted, const int64_t *__restrict__ prefix,
                              const int64_t *__restrict__ ptr, const int64_t *__restrict__ pw, int64_t cap, int64_t n,
                              int64_t k, int select, int64_t *__restrict__ dest) {
  const int64_t i = gid();
  if (i >= n) return;
  const int64_t g = group_sorted[i];
  if (g < 0 || g >= k) return;
  const int64_t before = prefix[i] - prefix[ptr[g]];
  const bool ok = select ? before < pw[g] - cap : before + w_sorted[i] <= cap - pw[g];
  if (!ok) dest[perm[i]] = -1;
}
__global__ void apply_kernel(const int64_t *__restrict__ dest, const int64_t *__restrict__ vw, int64_t n, int64_t k,
                             int64_t *__restrict__ part, int64_t *__restrict__ pw, int64_t *__restrict__ moved) {
  const int64_t v = gid();
  if (v >= n) return;
  const int64_t d = dest[v];
  if (d < 0 || d >= k || d == part[v]) return;
  add_i64(pw + part[v], -vw[v]);
  add_i64(pw + d, vw[v]);
  part[v] = d;
  add_i64(moved, 1);
}
// every edge is stored twice, so *cut ends at twice the cut weight
__global__ void cut_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                           const int64_t *__restrict__ w, const int64_t *__restrict__ part, int64_t E,
                           int64_t *__restrict__ cut) {
  const int64_t e = gid();
  int64_t x = 0;
  if (e < E && part[row[e]] != part[col[e]]) x = w[e];
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor((long long)x, off);
  if ((threadIdx.x & 63) == 0 && x != 0) add_i64(cut, x);
}
// cuts = (before, after) of a round that started within capacity (over == 0): a round that raised the cut is undone
__global__ void keep_better_kernel(const int64_t *__restrict__ cuts, const int64_t *__restrict__ over,
                                   const int64_t *__restrict__ part_old, const int64_t *__restrict__ pw_old, int64_t n,
                                   int64_t k, int64_t *__restrict__ part, int64_t *__restrict__ pw) {
  if (!(cuts[1] > cuts[0] && *over == 0)) return;
  const int64_t i = gid();
  if (i < n) part[i] = part_old[i];
  if (i < k) pw[i] = pw_old[i];
}
__global__ void keep_better_cut_kernel(int64_t *__restrict__ cuts, const int64_t *__restrict__ over) {
  if (gid() != 0) return;
  if (!(cuts[1] > cuts[0] && *over == 0)) cuts[0] = cuts[1];
  cuts[1] = 0;
}
// balance[0] = parts over capacity, [1] = smallest part weight, [2] = smallest id of a part of that weight
__global__ void balance_kernel(const int64_t *__restrict__ pw, int64_t k, int64_t cap, int64_t *__restrict__ balance) {
  const int64_t p = gid();
  if (p >= k) return;
  if (pw[p] > cap) add_i64(balance, 1);
  min_i64(balance + 1, pw[p]);
}
__global__ void lightest_kernel(const int64_t *__restrict__ pw, int64_t k, int64_t *__restrict__ balance) {
  const int64_t p = gid();
  if (p < k && pw[p] == balance[1]) min_i64(balance + 2, p);
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

#define PART_STREAM hipStream_t stream = reinterpret_cast<hipStream_t>(stream_)

extern "C" int tsamd_partition_edges(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *cmap,
                                     int64_t E, int64_t n, int64_t n_key, int mirror, int64_t *row_out, int64_t *col_out,
                                     int64_t *weight_out, int64_t *info, void *stream_) {
  PART_STREAM;
  if (E < 0 || n < 0 || n_key < 0 || !info) return TSAMD_ERR_INVALID;
  if (E == 0) return TSAMD_OK;
  if (!row || !col || !row_out || !col_out || !weight_out) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(edges_kernel, grid_for(E), dim3(256), 0, stream, row, col, weight, cmap, E, n, n_key, mirror, row_out,
                     col_out, weight_out, info);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_vertex_weights(const int64_t *vweight, const int64_t *cmap, int64_t n, int64_t n_c,
                                              int64_t *vweight_c, void *stream_) {
  PART_STREAM;
  if (n < 0 || n_c < 0) return TSAMD_ERR_INVALID;
  if (n_c == 0) return TSAMD_OK;
  if (!vweight_c || (n > 0 && (!vweight || !cmap))) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(vweight_c, 0, sizeof(int64_t) * (size_t)n_c, stream));
  if (n == 0) return TSAMD_OK;
  hipLaunchKernelGGL(vertex_weights_kernel, grid_for(n), dim3(256), 0, stream, vweight, cmap, n, n_c, vweight_c);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_partition_match_workspace_bytes(int64_t n) {
  const size_t arr = align_up(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), 256);
  return 2 * arr + tsamd_exclusive_scan_workspace_bytes(n) + 256;
}

extern "C" int tsamd_partition_match(const int64_t *rowptr, const int64_t *col, const int64_t *weight,
                                     const int64_t *vweight, int64_t n, int64_t cap, int64_t rounds, int64_t *match,
                                     int64_t *cmap, int64_t *n_coarse, void *workspace, size_t workspace_bytes,
                                     void *stream_) {
  PART_STREAM;
  if (n < 0 || rounds < 0 || !n_coarse) return TSAMD_ERR_INVALID;
  if (n >= ((int64_t)1 << kIdBits)) return TSAMD_ERR_UNSUPPORTED;
  if (n == 0) {
    TSAMD_HIP_TRY(hipMemsetAsync(n_coarse, 0, sizeof(int64_t), stream));
    return TSAMD_OK;
  }
  if (!rowptr || !vweight || !match || !cmap) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_partition_match_workspace_bytes(n)) return TSAMD_ERR_WORKSPACE;
  const size_t arr = align_up(sizeof(int64_t) * (size_t)n, 256);
  char *p = reinterpret_cast<char *>(workspace);
  int64_t *prop = reinterpret_cast<int64_t *>(p), *rank = reinterpret_cast<int64_t *>(p + arr);
  void *scan_ws = p + 2 * arr;
  TSAMD_HIP_TRY(hipMemsetAsync(match, 0xFF, sizeof(int64_t) * (size_t)n, stream));  // -1
  for (int64_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(propose_lane_kernel, grid_for(n), dim3(256), 0, stream, rowptr, col, weight, vweight, match, n, cap,
                       (uint32_t)r, prop);
    TSAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(propose_wave_kernel, dim3((unsigned int)n), dim3(64), 0, stream, rowptr, col, weight, vweight, match,
                       n, cap, (uint32_t)r, prop);
    TSAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(handshake_kernel, grid_for(n), dim3(256), 0, stream, prop, n, match);
    TSAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(leader_kernel, grid_for(n), dim3(256), 0, stream, match, n, rank);
  TSAMD_LAUNCH_CHECK();
  const int st = tsamd_exclusive_scan_i64(rank, rank, n, n_coarse, scan_ws, tsamd_exclusive_scan_workspace_bytes(n), stream_);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(cmap_kernel, grid_for(n), dim3(256), 0, stream, match, rank, n, cmap);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_bfs_init(const int64_t *rowptr, int64_t n, int64_t *cl, int64_t *state, void *stream_) {
  PART_STREAM;
  if (n < 0 || !state) return TSAMD_ERR_INVALID;
  if (n >= ((int64_t)1 << kIdBits)) return TSAMD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(64), 0, stream, state, (int64_t)4, kNone);
  TSAMD_LAUNCH_CHECK();
  if (n == 0) return TSAMD_OK;
  if (!rowptr || !cl) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(bfs_init_kernel, grid_for(n), dim3(256), 0, stream, rowptr, n, cl, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_bfs_seed(int64_t *cl, int64_t n, int64_t component, int first, int64_t *state,
                                        void *stream_) {
  PART_STREAM;
  if (n < 0 || component < 0 || !state || (n > 0 && !cl)) return TSAMD_ERR_INVALID;
  if (!first && n > 0) {
    hipLaunchKernelGGL(bfs_unvisited_kernel, grid_for(n), dim3(256), 0, stream, cl, n, state);
    TSAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bfs_seed_kernel, dim3(1), dim3(64), 0, stream, cl, n, component, first, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_bfs_step(const int64_t *rowptr, const int64_t *col, int64_t n, int64_t *cl,
                                        int64_t component, int64_t level, int64_t *state, void *stream_) {
  PART_STREAM;
  if (n < 0 || component < 0 || level < 0 || !state) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(state + 3, 0, sizeof(int64_t), stream));
  if (n == 0) return TSAMD_OK;
  if (!rowptr || !cl) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(bfs_step_kernel, grid_for(n), dim3(256), 0, stream, rowptr, col, n, cl, component, level, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_partition_assign_workspace_bytes(int64_t n) {
  const size_t arr = align_up(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), 256);
  return 5 * arr + 256 + align_up(tsamd_sort_coo_workspace_bytes(n), 256) + tsamd_exclusive_scan_workspace_bytes(n) + 256;
}

extern "C" int tsamd_partition_assign(const int64_t *cl, const int64_t *vweight, int64_t n, int64_t k, int64_t *part,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!cl || !vweight || !part) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_partition_assign_workspace_bytes(n)) return TSAMD_ERR_WORKSPACE;
  const size_t arr = align_up(sizeof(int64_t) * (size_t)n, 256);
  char *p = reinterpret_cast<char *>(workspace);
  int64_t *comp = reinterpret_cast<int64_t *>(p), *level = reinterpret_cast<int64_t *>(p + arr);
  int64_t *perm = reinterpret_cast<int64_t *>(p + 2 * arr), *w_s = reinterpret_cast<int64_t *>(p + 3 * arr);
  int64_t *prefix = reinterpret_cast<int64_t *>(p + 4 * arr), *total = reinterpret_cast<int64_t *>(p + 5 * arr);
  const size_t sort_bytes = tsamd_sort_coo_workspace_bytes(n);
  void *sort_ws = p + 5 * arr + 256, *scan_ws = p + 5 * arr + 256 + align_up(sort_bytes, 256);
  hipLaunchKernelGGL(bfs_keys_kernel, grid_for(n), dim3(256), 0, stream, cl, n, comp, level);
  TSAMD_LAUNCH_CHECK();
  int st = tsamd_sort_coo_values(0, comp, level, n, n + 1, n + 1, nullptr, nullptr, perm, nullptr, vweight, w_s, 8, sort_ws,
                                 sort_bytes, stream_);
  if (st != TSAMD_OK) return st;
  st = tsamd_exclusive_scan_i64(w_s, prefix, n, total, scan_ws, tsamd_exclusive_scan_workspace_bytes(n), stream_);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(assign_kernel, grid_for(n), dim3(256), 0, stream, perm, w_s, prefix, total, n, k, part);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_part_weights(const int64_t *part, const int64_t *vweight, int64_t n, int64_t k,
                                            int64_t *pweight, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1 || !pweight) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(pweight, 0, sizeof(int64_t) * (size_t)k, stream));
  if (n == 0) return TSAMD_OK;
  if (!part || !vweight) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(part_weights_kernel, grid_for(n), dim3(256), 0, stream, part, vweight, n, k, pweight);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_partition_conn_workspace_bytes(int64_t n, int64_t k) {
  return align_up(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), 256) + 256 +
         sizeof(int64_t) * (size_t)kSpillBlocks * (size_t)(k > 0 ? k : 1) + 256;
}

extern "C" int tsamd_partition_conn(const int64_t *rowptr, const int64_t *col, const int64_t *weight,
                                    const int64_t *vweight, const int64_t *part, const int64_t *pweight, int64_t n,
                                    int64_t k, int64_t cap, int mode, const int64_t *lightest, int64_t *dest,
                                    int64_t *gain, void *workspace, size_t workspace_bytes, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1 || mode < 0 || mode > 2) return TSAMD_ERR_INVALID;
  if (k >= ((int64_t)1 << kIdBits)) return TSAMD_ERR_UNSUPPORTED;
  if (n == 0) return TSAMD_OK;
  if (!rowptr || !vweight || !part || !pweight || !dest || !gain) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_partition_conn_workspace_bytes(n, k)) return TSAMD_ERR_WORKSPACE;
  const size_t arr = align_up(sizeof(int64_t) * (size_t)n, 256);
  char *p = reinterpret_cast<char *>(workspace);
  int64_t *spill = reinterpret_cast<int64_t *>(p), *spill_count = reinterpret_cast<int64_t *>(p + arr);
  int64_t *table = reinterpret_cast<int64_t *>(p + arr + 256);
  TSAMD_HIP_TRY(hipMemsetAsync(spill_count, 0, sizeof(int64_t), stream));
  hipLaunchKernelGGL(conn_lane_kernel, grid_for(n), dim3(256), 0, stream, rowptr, col, weight, vweight, part, pweight, n, k,
                     cap, mode, lightest, dest, gain);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(conn_wave_kernel, dim3((unsigned int)n), dim3(64), 0, stream, rowptr, col, weight, vweight, part,
                     pweight, n, k, cap, mode, lightest, dest, gain, spill, spill_count);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(conn_spill_kernel, dim3(kSpillBlocks), dim3(256), 0, stream, rowptr, col, weight, vweight, part,
                     pweight, n, k, cap, mode, lightest, dest, gain, spill, spill_count, table);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_recount(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *part,
                                       const int64_t *pweight, const int64_t *gain, int64_t n, int64_t E, int64_t cap,
                                       int64_t *dest, int64_t *acc, void *stream_) {
  PART_STREAM;
  if (n < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!part || !pweight || !gain || !dest || !acc || (E > 0 && (!row || !col || !weight))) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(acc, 0, sizeof(int64_t) * (size_t)n, stream));
  if (E > 0) {
    hipLaunchKernelGGL(recount_kernel, grid_for(E), dim3(256), 0, stream, row, col, weight, part, dest, gain, E, acc);
    TSAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(recount_filter_kernel, grid_for(n), dim3(256), 0, stream, acc, part, pweight, cap, n, dest);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_partition_commit_workspace_bytes(int64_t n, int64_t k) {
  const size_t arr = align_up(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), 256);
  return 7 * arr + align_up(sizeof(int64_t) * (size_t)(k + 2), 256) + align_up(tsamd_sort_coo_workspace_bytes(n), 256) +
         tsamd_exclusive_scan_workspace_bytes(n) + 256;
}

extern "C" int tsamd_partition_commit(int64_t *dest, const int64_t *gain, const int64_t *vweight, const int64_t *part,
                                      const int64_t *pweight, int64_t n, int64_t k, int64_t cap, int select,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!dest || !gain || !vweight || !part || !pweight) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_partition_commit_workspace_bytes(n, k)) return TSAMD_ERR_WORKSPACE;
  const size_t arr = align_up(sizeof(int64_t) * (size_t)n, 256);
  char *p = reinterpret_cast<char *>(workspace);
  int64_t *key_row = reinterpret_cast<int64_t *>(p), *key_col = reinterpret_cast<int64_t *>(p + arr);
  int64_t *row_s = reinterpret_cast<int64_t *>(p + 2 * arr), *perm = reinterpret_cast<int64_t *>(p + 3 * arr);
  int64_t *w_s = reinterpret_cast<int64_t *>(p + 4 * arr), *prefix = reinterpret_cast<int64_t *>(p + 5 * arr);
  int64_t *col_s = reinterpret_cast<int64_t *>(p + 6 * arr);
  int64_t *ptr = reinterpret_cast<int64_t *>(p + 7 * arr);
  const size_t ptr_bytes = align_up(sizeof(int64_t) * (size_t)(k + 2), 256), sort_bytes = tsamd_sort_coo_workspace_bytes(n);
  void *sort_ws = p + 7 * arr + ptr_bytes, *scan_ws = p + 7 * arr + ptr_bytes + align_up(sort_bytes, 256);
  hipLaunchKernelGGL(commit_keys_kernel, grid_for(n), dim3(256), 0, stream, dest, gain, part, pweight, cap, n, k, select,
                     key_row, key_col);
  TSAMD_LAUNCH_CHECK();
  int st = tsamd_sort_coo_values(0, key_row, key_col, n, k + 1, 2 * kGainClamp, row_s, col_s, perm, nullptr, vweight, w_s, 8,
                                 sort_ws, sort_bytes, stream_);
  if (st != TSAMD_OK) return st;
  st = tsamd_exclusive_scan_i64(w_s, prefix, n, nullptr, scan_ws, tsamd_exclusive_scan_workspace_bytes(n), stream_);
  if (st != TSAMD_OK) return st;
  st = tsamd_ind2ptr(row_s, k + 1, n, ptr, stream_);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(accept_kernel, grid_for(n), dim3(256), 0, stream, row_s, perm, w_s, prefix, ptr, pweight, cap, n, k,
                     select, dest);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_apply(const int64_t *dest, const int64_t *vweight, int64_t n, int64_t k, int64_t *part,
                                     int64_t *pweight, int64_t *moved, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1 || !moved) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!dest || !vweight || !part || !pweight) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(apply_kernel, grid_for(n), dim3(256), 0, stream, dest, vweight, n, k, part, pweight, moved);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_cut(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *part,
                                   int64_t E, int64_t *cut, void *stream_) {
  PART_STREAM;
  if (E < 0 || !cut) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(cut, 0, sizeof(int64_t), stream));
  if (E == 0) return TSAMD_OK;
  if (!row || !col || !weight || !part) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(cut_kernel, grid_for(E), dim3(256), 0, stream, row, col, weight, part, E, cut);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_keep_better(int64_t *cuts, const int64_t *over, const int64_t *part_old,
                                           const int64_t *pweight_old, int64_t n, int64_t k, int64_t *part,
                                           int64_t *pweight, void *stream_) {
  PART_STREAM;
  if (n < 0 || k < 1 || !cuts || !over || !pweight_old || !pweight) return TSAMD_ERR_INVALID;
  if (n > 0 && (!part_old || !part)) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(keep_better_kernel, grid_for(n > k ? n : k), dim3(256), 0, stream, cuts, over, part_old, pweight_old,
                     n, k, part, pweight);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(keep_better_cut_kernel, dim3(1), dim3(64), 0, stream, cuts, over);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_partition_balance(const int64_t *pweight, int64_t k, int64_t cap, int64_t *balance, void *stream_) {
  PART_STREAM;
  if (k < 1 || !pweight || !balance) return TSAMD_ERR_INVALID;
  TSAMD_HIP_TRY(hipMemsetAsync(balance, 0, sizeof(int64_t), stream));
  hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(64), 0, stream, balance + 1, (int64_t)2, kNone);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(balance_kernel, grid_for(k), dim3(256), 0, stream, pweight, k, cap, balance);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(lightest_kernel, grid_for(k), dim3(256), 0, stream, pweight, k, balance);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}
