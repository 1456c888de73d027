// Reverse Cuthill-McKee ordering on gfx950 (reverse_cuthill_mckee; the reference hands the matrix to scipy on the CPU,
// torch_sparse/bandwidth.py:8-20).  scipy's serial search restated as a level-synchronous one that gives the same
// permutation bit for bit; docs/design/rcm.md has the restatement, tests/rcm_oracle.py its numpy form.  This unit holds
// the kernels; the prologue (rank by (degree, id) and the relabelled, re-sorted graph through the existing sort) and the
// loop that alternates the two routes below are the host driver in ops_rcm.cpp.
//   working graph   CSR of the graph relabelled by rank in stable (degree, id) order, rows sorted by the new ids: the
//                   entries of a row then stand in the order in which scipy appends a node's children
//   a level         frontier = order[lo, hi).  claim: min of the frontier position into owner[j] for every unvisited
//                   neighbour j; flag: the entry whose position won; scan of the flags in (position, adjacency) order;
//                   write: pos[j] = hi + offset, order[hi + offset] = j.  A repeated entry of a row counts once.
//   big route       one level per group of launches, one lane per frontier ENTRY (tile_span / segment_of over the scan
//                   of the frontier's row lengths), so a hub row is spread over as many workgroups as it has tiles
//   small route     ONE workgroup runs whole levels, finds the next component's seed and batches isolated seeds, until
//                   a frontier outgrows kRcmNodes nodes / kRcmEdges entries, everything is ordered or the level budget
//                   of the launch is spent; the host reads one state record and relaunches
// No workgroup waits for another one anywhere: the small route is one workgroup, the big route's phases are launches.
// Every atomic is an integer min or max whose result does not depend on the order of arrival.
#include "common.h"
#include "expand.h"
#include "scan.h"

namespace tsamd {
namespace {

constexpr int kRcmThreads = 1024;            // the small route's workgroup
constexpr int kRcmNodes = kRcmThreads;       // its frontier: one node per thread
constexpr int kRcmItems = 8;                 // frontier entries per thread
constexpr int kRcmEdges = kRcmThreads * kRcmItems;
constexpr int kRcmSeedChunks = 4096;         // chunks of kRcmThreads seeds one launch may search
constexpr int64_t kUnowned = 0x7fffffffffffffffLL;

// the state record, int64[kRcmStateWords]
enum { kLo = 0, kHi, kCursor, kReason, kLevels, kComponents, kEntries, kError, kRcmStateWords };

__device__ inline int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline dim3 grid_for(int64_t n, int block = 256) { return dim3((unsigned int)ceil_div(n > 0 ? n : 1, block)); }

__device__ inline void min_i64(int64_t *p, int64_t v) { atomicMin(reinterpret_cast<long long *>(p), (long long)v); }
__device__ inline void max_i64(int64_t *p, int64_t v) { atomicMax(reinterpret_cast<long long *>(p), (long long)v); }
// pos / owner / order are written and read by different lanes of one launch (small route): device-scope accesses, so
// that no read is served from a stale line of the vector cache
__device__ inline int64_t ld(const int64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st(int64_t *p, int64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- degree, prologue, epilogue -------------------------------------------------------------------------------------
__global__ void row_length_kernel(const int64_t *__restrict__ rowptr, int64_t n, int64_t *__restrict__ deg) {
  const int64_t i = gid();
  if (i < n) deg[i] = rowptr[i + 1] - rowptr[i];
}

// one lane per ENTRY: a row that holds its own diagonal gets length + 1 (a max, so a repeated diagonal counts once)
__global__ void __launch_bounds__(256) diagonal_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col,
                                                       int64_t n, int64_t E, int64_t *__restrict__ deg) {
  __shared__ int64_t span[2];
  const int64_t e0 = (int64_t)blockIdx.x * kExpandTile, e1 = e0 + kExpandTile < E ? e0 + kExpandTile : E;
  int64_t slo, shi;
  tile_span(rowptr, n, e0, e1, span, &slo, &shi);
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const int64_t r = slo + segment_of(rowptr + slo, shi - slo + 1, e);
    if (col[e] == r) max_i64(deg + r, rowptr[r + 1] - rowptr[r] + 1);
  }
}

// out[i] = table[idx[i]]; an id outside [0, n) gives 0 and raises state[kError]
__global__ void relabel_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ table, int64_t count, int64_t n,
                               int64_t *__restrict__ out, int64_t *__restrict__ state) {
  const int64_t i = gid();
  if (i >= count) return;
  const int64_t v = idx[i];
  const bool ok = v >= 0 && v < n;
  if (!ok) max_i64(state + kError, 1);
  out[i] = ok ? table[v] : 0;
}

// rank[by_rank[r]] = r
__global__ void invert_kernel(const int64_t *__restrict__ by_rank, int64_t n, int64_t *__restrict__ rank) {
  const int64_t r = gid();
  if (r < n) rank[by_rank[r]] = r;
}

// seeds_r[i] = rank[seeds[i]] (-1 for an id out of range); seen[s] = the largest i with seeds[i] == s, so a repeated id
// is found by the check below
__global__ void seeds_kernel(const int64_t *__restrict__ seeds, const int64_t *__restrict__ rank, int64_t n,
                             int64_t *__restrict__ seeds_r, int64_t *__restrict__ seen, int64_t *__restrict__ state) {
  const int64_t i = gid();
  if (i >= n) return;
  const int64_t s = seeds[i];
  const bool ok = s >= 0 && s < n;
  if (!ok) max_i64(state + kError, 2);
  seeds_r[i] = ok ? rank[s] : -1;
  if (ok) max_i64(seen + s, i);
}
__global__ void seeds_check_kernel(const int64_t *__restrict__ seeds, const int64_t *__restrict__ seen, int64_t n,
                                   int64_t *__restrict__ state) {
  const int64_t i = gid();
  if (i >= n) return;
  const int64_t s = seeds[i];
  if (s >= 0 && s < n && seen[s] != i) max_i64(state + kError, 2);
}

__global__ void init_kernel(int64_t n, int64_t *__restrict__ pos, int64_t *__restrict__ owner, int64_t *__restrict__ seen) {
  const int64_t i = gid();
  if (i >= n) return;
  pos[i] = -1;
  owner[i] = kUnowned;
  seen[i] = -1;
}

// perm[i] = by_rank[order[n - 1 - i]]
__global__ void finish_kernel(const int64_t *__restrict__ order, const int64_t *__restrict__ by_rank, int64_t n,
                              int64_t *__restrict__ perm) {
  const int64_t i = gid();
  if (i < n) perm[i] = by_rank[order[n - 1 - i]];
}

// ---- big route ------------------------------------------------------------------------------------------------------
// fdeg[p] = row length of the p-th frontier node
__global__ void frontier_length_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ order,
                                       const int64_t *__restrict__ state, int64_t *__restrict__ fdeg) {
  const int64_t lo = state[kLo], nf = state[kHi] - lo, p = gid();
  if (p >= nf) return;
  const int64_t u = order[lo + p];
  fdeg[p] = rowptr[u + 1] - rowptr[u];
}

// one lane per frontier entry t in [0, T): fptr = exclusive scan of fdeg (fptr[nf] = T).  ej[t] = the neighbour if it is
// unvisited and not a repeat of the entry before it, else -1; ep[t] = the position of the frontier node.
__global__ void __launch_bounds__(256)
claim_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col, const int64_t *__restrict__ order,
             const int64_t *__restrict__ fptr, const int64_t *__restrict__ state, int64_t T,
             const int64_t *__restrict__ pos, int64_t *__restrict__ owner, int64_t *__restrict__ ej,
             int64_t *__restrict__ ep) {
  __shared__ int64_t span[2];
  const int64_t lo = state[kLo], nf = state[kHi] - lo;
  const int64_t t0 = (int64_t)blockIdx.x * kExpandTile, t1 = t0 + kExpandTile < T ? t0 + kExpandTile : T;
  int64_t slo, shi;
  tile_span(fptr, nf, t0, t1, span, &slo, &shi);
  for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
    const int64_t p = slo + segment_of(fptr + slo, shi - slo + 1, t);
    const int64_t k = rowptr[order[lo + p]] + (t - fptr[p]);
    const int64_t j = col[k];
    const bool cand = pos[j] < 0 && !(t > fptr[p] && col[k - 1] == j);
    if (cand) min_i64(owner + j, lo + p);
    ej[t] = cand ? j : -1;
    ep[t] = lo + p;
  }
}

__global__ void flag_kernel(const int64_t *__restrict__ ej, const int64_t *__restrict__ ep,
                            const int64_t *__restrict__ owner, int64_t T, int64_t *__restrict__ off) {
  const int64_t t = gid();
  if (t >= T) return;
  const int64_t j = ej[t];
  off[t] = (j >= 0 && owner[j] == ep[t]) ? 1 : 0;
}

// off = exclusive scan of the flags
__global__ void write_kernel(const int64_t *__restrict__ ej, const int64_t *__restrict__ ep,
                             const int64_t *__restrict__ owner, const int64_t *__restrict__ off,
                             const int64_t *__restrict__ state, int64_t T, int64_t n, int64_t *__restrict__ pos,
                             int64_t *__restrict__ order) {
  const int64_t t = gid();
  if (t >= T) return;
  const int64_t j = ej[t];
  if (j < 0 || owner[j] != ep[t]) return;
  const int64_t q = state[kHi] + off[t];
  if (q >= n) return;  // cannot happen on a state record the one-workgroup route left behind
  pos[j] = q;
  order[q] = j;
}

// the frontier becomes the nodes just written; children (device, nullable = none)
__global__ void advance_kernel(const int64_t *__restrict__ children, int64_t *__restrict__ state) {
  if (gid() != 0) return;
  const int64_t c = children ? children[0] : 0, hi = state[kHi];
  state[kLo] = hi;
  state[kHi] = hi + c;
  if (c > 0) state[kLevels] += 1;
}

// ---- small route ----------------------------------------------------------------------------------------------------
// exclusive scan of one int per thread over the 1024-thread workgroup; sm: 17 ints.  BEGINS with a barrier (sm may still
// be read from the call before) and ends with reads of sm, not with a barrier.
__device__ inline int block_scan_1024(int v, int *sm, int *total) {
  const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
  const int inc = (int)wave_inclusive_scan_u32((uint32_t)v);
  __syncthreads();
  if (lane == 63) sm[wid] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kRcmThreads / 64; ++w) {
    const int s = sm[w];
    if (w < wid) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

enum { kDone = 0, kOver = 1, kBudget = 2, kSeedBudget = 3 };

__global__ void __launch_bounds__(kRcmThreads)
small_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col, const int64_t *__restrict__ seeds_r,
             int64_t n, int cap_nodes, int budget, int64_t *pos, int64_t *owner, int64_t *order, int64_t *state) {
  __shared__ int s_fptr[kRcmNodes + 1];   // scan of the frontier's row lengths
  __shared__ int64_t s_row[kRcmNodes];    // first entry of the frontier node's row
  __shared__ int s_ej[kRcmEdges];         // the candidate of every frontier entry, or -1
  __shared__ int s_scan[kRcmThreads / 64 + 1];
  __shared__ int s_first;
  const int tid = (int)threadIdx.x;
  // bad input (tsamd_rcm_begin / _relabel raised the flag): nothing runs on it.  A seed order that repeats a node would
  // hand out more positions than there are nodes.
  if (state[kError] != 0) {
    if (tid == 0) state[kReason] = kDone;
    return;
  }
  int64_t lo = state[kLo], hi = state[kHi], cursor = state[kCursor];
  int64_t levels = state[kLevels], components = state[kComponents], entries = 0;
  int reason = kBudget, chunks = 0;

  for (int it = 0; it < budget; ++it) {
    if (hi == lo) {  // the component is complete: the next unvisited seed starts one
      if (hi >= n || cursor >= n) { reason = kDone; break; }
      bool found = false;
      while (!found && cursor < n) {
        if (chunks == kRcmSeedChunks) break;
        ++chunks;
        if (tid == 0) s_first = kRcmThreads;
        const int64_t i = cursor + tid;
        const int64_t s = i < n ? seeds_r[i] : -1;
        const bool fresh = s >= 0 && ld(pos + s) < 0;
        const bool isolated = fresh && rowptr[s + 1] == rowptr[s];
        __syncthreads();
        if (fresh && !isolated) atomicMin(&s_first, tid);
        __syncthreads();
        const int first = s_first;
        // the isolated seeds in front of it are components of one level each, in seed order
        const bool emit = isolated && tid < first;
        int iso;
        const int at = block_scan_1024(emit ? 1 : 0, s_scan, &iso);
        if (emit && hi + at < n) {  // positions stay below n whatever the seeds hold
          st(pos + s, hi + at);
          st(order + hi + at, s);
        }
        hi += iso;
        lo = hi;
        levels += iso;
        components += iso;
        if (first < kRcmThreads) {
          if (tid == first && hi < n) {
            st(pos + s, hi);
            st(order + hi, s);
          }
          hi += 1;
          levels += 1;
          components += 1;
          cursor += first + 1;
          found = true;
        } else {
          cursor += kRcmThreads;
        }
        __threadfence();
        __syncthreads();  // pos / order are read next; s_first is rewritten by the next chunk
      }
      if (!found) {
        reason = (hi >= n || cursor >= n) ? kDone : kSeedBudget;
        break;
      }
    }
    const int64_t nf = hi - lo;
    if (nf > cap_nodes) { reason = kOver; break; }
    // the frontier's row lengths and their scan
    int64_t u = 0, start = 0, len = 0;
    if (tid < nf) {
      u = ld(order + lo + tid);
      start = rowptr[u];
      len = rowptr[u + 1] - start;
    }
    const bool wide = __syncthreads_or(len > kRcmEdges);
    if (wide) { reason = kOver; break; }
    int T;
    const int at = block_scan_1024((int)len, s_scan, &T);
    if (T > kRcmEdges) { reason = kOver; break; }
    if (tid < nf) {
      s_fptr[tid] = at;
      s_row[tid] = start;
    }
    if (tid == 0) s_fptr[nf] = T;
    __syncthreads();
    entries = T;
    // claim: thread t takes the entries [t * ipt, (t + 1) * ipt)
    const int ipt = (T + kRcmThreads - 1) / kRcmThreads;
    const int t0 = tid * ipt, t1 = t0 + ipt < T ? t0 + ipt : T;
    int p0 = 0;
    if (t0 < t1) {
      int a = 0, b = (int)nf;  // last p with s_fptr[p] <= t0
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (s_fptr[mid] <= t0) a = mid; else b = mid;
      }
      p0 = a;
    }
    int p = p0;
    for (int t = t0; t < t1; ++t) {
      while (s_fptr[p + 1] <= t) ++p;
      const int64_t k = s_row[p] + (t - s_fptr[p]);
      const int64_t j = col[k];
      const bool cand = ld(pos + j) < 0 && !(t > s_fptr[p] && col[k - 1] == j);
      if (cand) min_i64(owner + j, lo + p);
      s_ej[t] = cand ? (int)j : -1;
    }
    __threadfence();  // every claim has reached the owner array before a winner is read
    __syncthreads();
    // flag, scan, write
    uint32_t mine = 0;
    p = p0;
    for (int t = t0; t < t1; ++t) {
      while (s_fptr[p + 1] <= t) ++p;
      const int j = s_ej[t];
      if (j >= 0 && ld(owner + j) == lo + p) mine |= 1u << (t - t0);
    }
    int children;
    int q = block_scan_1024(__popc(mine), s_scan, &children);
    for (int t = t0; t < t1; ++t) {
      if (mine >> (t - t0) & 1u) {
        const int j = s_ej[t];
        if (hi + q < n) {
          st(pos + j, hi + q);
          st(order + hi + q, (int64_t)j);
        }
        ++q;
      }
    }
    __threadfence();
    __syncthreads();  // the next level reads pos / order, and rewrites the LDS arrays
    lo = hi;
    hi += children;
    if (children > 0) levels += 1;
  }
  if (tid == 0) {
    if (hi > n) state[kError] = 2;  // more positions than nodes: only a seed order that repeats a node gets here
    state[kLo] = lo;
    state[kHi] = hi;
    state[kCursor] = cursor;
    state[kReason] = reason;
    state[kLevels] = levels;
    state[kComponents] = components;
    state[kEntries] = entries;
  }
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

#define RCM_STREAM hipStream_t stream = (hipStream_t)stream_

extern "C" int tsamd_rcm_limits(int64_t out[3]) {
  if (!out) return TSAMD_ERR_INVALID;
  out[0] = kRcmNodes;
  out[1] = kRcmEdges;
  out[2] = 256;  // levels per launch of the small route: what tsamd::rcm passes as `budget`
  return TSAMD_OK;
}

extern "C" int tsamd_rcm_degree(const int64_t *rowptr, const int64_t *col, int64_t n, int64_t E, int64_t *deg,
                                void *stream_) {
  RCM_STREAM;
  if (n < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!rowptr || !deg || (E > 0 && !col)) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(row_length_kernel, grid_for(n), dim3(256), 0, stream, rowptr, n, deg);
  TSAMD_LAUNCH_CHECK();
  if (E == 0) return TSAMD_OK;
  hipLaunchKernelGGL(diagonal_kernel, grid_for(E, kExpandTile), dim3(256), 0, stream, rowptr, col, n, E, deg);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_rcm_relabel(const int64_t *idx, const int64_t *table, int64_t count, int64_t n, int64_t *out,
                                 int64_t *state, void *stream_) {
  RCM_STREAM;
  if (count < 0 || n < 0 || !state) return TSAMD_ERR_INVALID;
  if (count == 0) return TSAMD_OK;
  if (!idx || !table || !out) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(relabel_kernel, grid_for(count), dim3(256), 0, stream, idx, table, count, n, out, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_rcm_begin(const int64_t *by_rank, const int64_t *seeds, int64_t n, int64_t *rank, int64_t *seeds_r,
                               int64_t *pos, int64_t *owner, int64_t *scratch, int64_t *state, void *stream_) {
  RCM_STREAM;
  if (n < 0 || !state) return TSAMD_ERR_INVALID;
  if (n >= ((int64_t)1 << 31)) return TSAMD_ERR_UNSUPPORTED;
  if (n == 0) return TSAMD_OK;
  if (!by_rank || !seeds || !rank || !seeds_r || !pos || !owner || !scratch) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(init_kernel, grid_for(n), dim3(256), 0, stream, n, pos, owner, scratch);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(invert_kernel, grid_for(n), dim3(256), 0, stream, by_rank, n, rank);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(seeds_kernel, grid_for(n), dim3(256), 0, stream, seeds, rank, n, seeds_r, scratch, state);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(seeds_check_kernel, grid_for(n), dim3(256), 0, stream, seeds, scratch, n, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_rcm_small(const int64_t *rowptr, const int64_t *col, const int64_t *seeds_r, int64_t n,
                               int64_t cap_nodes, int64_t budget, int64_t *pos, int64_t *owner, int64_t *order,
                               int64_t *state, void *stream_) {
  RCM_STREAM;
  if (n <= 0 || cap_nodes < 0 || budget < 1 || budget > ((int64_t)1 << 20)) return TSAMD_ERR_INVALID;
  if (n >= ((int64_t)1 << 31)) return TSAMD_ERR_UNSUPPORTED;
  if (!rowptr || !seeds_r || !pos || !owner || !order || !state) return TSAMD_ERR_INVALID;
  const int cap = (int)(cap_nodes < kRcmNodes ? cap_nodes : kRcmNodes);
  hipLaunchKernelGGL(small_kernel, dim3(1), dim3(kRcmThreads), 0, stream, rowptr, col, seeds_r, n, cap, (int)budget, pos,
                     owner, order, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_rcm_level_workspace_bytes(int64_t nf) {
  return tsamd_exclusive_scan_workspace_bytes(nf + 1) + 256;
}

extern "C" int tsamd_rcm_level_plan(const int64_t *rowptr, const int64_t *order, int64_t nf, int64_t *fptr,
                                    int64_t *state, void *workspace, size_t workspace_bytes, void *stream_) {
  RCM_STREAM;
  if (nf <= 0) return TSAMD_ERR_INVALID;
  if (!rowptr || !order || !fptr || !state) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_rcm_level_workspace_bytes(nf)) return TSAMD_ERR_WORKSPACE;
  hipLaunchKernelGGL(frontier_length_kernel, grid_for(nf), dim3(256), 0, stream, rowptr, order, state, fptr);
  TSAMD_LAUNCH_CHECK();
  TSAMD_HIP_TRY(hipMemsetAsync(fptr + nf, 0, sizeof(int64_t), stream));
  return tsamd_exclusive_scan_i64(fptr, fptr, nf + 1, state + kEntries, workspace, workspace_bytes, stream_);
}

extern "C" int tsamd_rcm_level_run(const int64_t *rowptr, const int64_t *col, const int64_t *fptr, int64_t T, int64_t n,
                                   int64_t *pos, int64_t *owner, int64_t *order, int64_t *ej, int64_t *ep, int64_t *off,
                                   int64_t *state, void *workspace, size_t workspace_bytes, void *stream_) {
  RCM_STREAM;
  if (T < 0 || n < 0 || !state) return TSAMD_ERR_INVALID;
  if (T == 0) {
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, stream, (const int64_t *)nullptr, state);
    TSAMD_LAUNCH_CHECK();
    return TSAMD_OK;
  }
  if (!rowptr || !col || !fptr || !pos || !owner || !order || !ej || !ep || !off) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_rcm_level_workspace_bytes(T)) return TSAMD_ERR_WORKSPACE;
  int64_t *children = reinterpret_cast<int64_t *>(workspace);
  void *scan_ws = reinterpret_cast<char *>(workspace) + 256;
  hipLaunchKernelGGL(claim_kernel, grid_for(T, kExpandTile), dim3(256), 0, stream, rowptr, col, order, fptr, state, T, pos,
                     owner, ej, ep);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(flag_kernel, grid_for(T), dim3(256), 0, stream, ej, ep, owner, T, off);
  TSAMD_LAUNCH_CHECK();
  const int st = tsamd_exclusive_scan_i64(off, off, T, children, scan_ws, workspace_bytes - 256, stream_);
  if (st != TSAMD_OK) return st;
  hipLaunchKernelGGL(write_kernel, grid_for(T), dim3(256), 0, stream, ej, ep, owner, off, state, T, n, pos, order);
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, stream, (const int64_t *)children, state);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" int tsamd_rcm_finish(const int64_t *order, const int64_t *by_rank, int64_t n, int64_t *perm, void *stream_) {
  RCM_STREAM;
  if (n < 0) return TSAMD_ERR_INVALID;
  if (n == 0) return TSAMD_OK;
  if (!order || !by_rank || !perm) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(finish_kernel, grid_for(n), dim3(256), 0, stream, order, by_rank, n, perm);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}
