// The state of the SpMM operator glue: everything that outlives a call of ops_spmm.cpp.  Three caches -- the operand
// cache (opt-in: a result can depend on it), the transposed-pattern cache (owned arrays only) and the pattern hints
// (advisory) -- over one entry record, each behind its own lock, and the four operators that switch and read them.
#include "ops_spmm_state.h"

#include <array>
#include <atomic>

#include <c10/util/SmallVector.h>

namespace tsamd_ops {

bool stream_is_capturing(void *stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(reinterpret_cast<hipStream_t>(stream), &cs) != hipSuccess ||
         cs != hipStreamCaptureStatusNone;
}

namespace {

// "The same tensor contents as last time", as far as torch can tell: the same storage object (held weakly: while it is
// alive its address cannot be handed to another tensor), the same data pointer and the same version counter.
// Inference tensors have no version counter: no cache below ever keeps or matches one (may_remember turns them away).
struct TensorIdentity {
  c10::weak_intrusive_ptr<c10::StorageImpl> storage{c10::weak_intrusive_ptr<c10::StorageImpl>(
      c10::make_intrusive<c10::StorageImpl>(c10::StorageImpl::use_byte_size_t(), 0, c10::DataPtr(), nullptr, false))};
  const void *ptr = nullptr;
  uint32_t version = 0;

  static uint32_t version_of(const Tensor &t) { return t.unsafeGetTensorImpl()->version_counter().current_version(); }
  bool matches(const Tensor &t) const {
    if (ptr != t.data_ptr() || version != version_of(t)) return false;
    auto alive = storage.lock();
    return alive && alive.get() == t.storage().unsafeGetStorageImpl();
  }
  void rearm(const Tensor &t) {
    storage = c10::weak_intrusive_ptr<c10::StorageImpl>(
        c10::intrusive_ptr<c10::StorageImpl>::reclaim_copy(t.storage().unsafeGetStorageImpl()));
    ptr = t.data_ptr();
    version = version_of(t);
  }
  void forget() { ptr = nullptr; }
};

// Who an entry may identify: a tensor on the GPU, contiguous, with a version counter.
bool may_remember(const Tensor &t) {
  return t.defined() && t.device().is_cuda() && t.is_contiguous() && !t.is_inference();
}

// What every cache below keeps per entry: the identities of one or two tensors, the scalars of the key, the stream the
// kept tensor is produced and consumed on (no cross-stream events: another stream never matches), and the kept tensor.
using Key = c10::SmallVector<int64_t, 12>;
struct Entry {
  TensorIdentity first, second;  // (second: entries over two tensors)
  Key key;
  void *stream = nullptr;
  Tensor kept;

  bool keyed(const Key &k, void *s) const { return key == k && stream == s; }
  bool matches(const Key &k, void *s, const Tensor &a, const Tensor *b = nullptr) const {
    return keyed(k, s) && first.matches(a) && (b == nullptr || second.matches(*b));
  }
  // (leaves `kept` alone: whether it is reused, replaced or dropped is the cache's policy)
  void rearm(const Key &k, void *s, const Tensor &a, const Tensor *b = nullptr) {
    key = k;
    stream = s;
    first.rearm(a);
    if (b != nullptr) second.rearm(*b);
  }
  void drop() {
    kept = Tensor();
    first.forget();
    second.forget();
  }
};

// NAME=1 turns a switch that is off by default on, NAME=0 one that is on by default off
bool env_switch(const char *name, bool dflt) {
  const char *env = getenv(name);
  if (env == nullptr) return dflt;
  return dflt ? env[0] != '0' : env[0] == '1';
}

// each cache's state: made at its first use (its environment switch is read then)
template <class Cache>
Cache &state() {
  static Cache c;
  return c;
}

int64_t minmax_class(int red) { return (red == TSAMD_MIN || red == TSAMD_MAX) ? 1 : 0; }

// ---- operand cache (include/tsamd.h: tsamd_spmm_cached) ------------------------------------------------
// One entry: the relabelled copy of the last dense operand that needed one.  A call may reuse it when the
// operand is provably the same tensor contents as far as torch can tell (TensorIdentity), with the same shape /
// dtype / device / stream, same sparse pattern (col pointer, version and length) and reduction class -- and the
// kernel side re-checks a sampled fingerprint on the device.
//
// OPT-IN (off by default): the reference boundary keeps no state between calls (csrc/cuda/spmm_cuda.cu:102,134
// allocate fresh outputs, nothing else survives), and neither the version counter nor a SAMPLED fingerprint can
// see a sparse write that bypasses autograd's bookkeeping (`x.data[i] = ...`, a DLPack / raw-pointer writer, a
// collective landing in a persistent buffer): with the cache on such a write returns a stale product.  A caller
// that knows its operand is only ever updated through torch (or densely) turns it on with
// torch.ops.tsamd.operand_cache(True) or TSAMD_OPERAND_CACHE=1; inference tensors (no version counter) never use it.
struct OperandCache {
  std::mutex mu;
  std::atomic<bool> enabled{env_switch("TSAMD_OPERAND_CACHE", false)};  // written under mu, read without
  // first: mat.  key: dtype, reduction class, device, col pointer / version / length, sizes of mat
  Entry entry;
  int64_t hits = 0, fills = 0;
};

// torch.ops.tsamd.operand_cache(enable) -> [was enabled, hits, fills]; drops the cached copy
std::vector<int64_t> operand_cache_ctl(bool enable) {
  OperandCache &c = state<OperandCache>();
  std::lock_guard<std::mutex> lock(c.mu);
  std::vector<int64_t> r = {c.enabled ? 1 : 0, c.hits, c.fills};
  c.enabled = enable;
  c.entry.drop();
  return r;
}

// ---- transposed-pattern cache ------------------------------------------------------------------------------
// grad_mat = A^T * grad_out multiplies by the CSC view (colptr, row[csr2csc], value[csr2csc]).  The reference
// gathers row[csr2csc] and value[csr2csc] anew in every backward (spmm.cpp:104-106).  The row ids of the CSC
// order only depend on the PATTERN, which a training loop does not change: they are gathered once and kept
// (one entry; key = the identities of `row` and `csr2csc`), so that every
// later backward reads them sequentially; the stream is part of the key (a backward on another stream starts a
// new entry instead of reading arrays whose producer it is not ordered after).  TSAMD_PATTERN_CACHE=0 turns it off (then, and for a pattern seen
// for the first time in a no-reuse setting, the kernel reads (row, value) through csr2csc -- tsamd_spmm_permuted).
//
// Only the `tsamd::spmm_sum_owned` / `tsamd::spmm_mean_owned` ops consult it -- the ones SparseTensor.matmul
// calls with arrays that its SparseStorage owns (immutable by the storage's contract, exactly like the
// reference's own storage-level caches rowcount / colptr / csr2csc).  The bare reference ops
// `torch_sparse::spmm_sum / spmm_mean` keep no state THAT A RESULT CAN DEPEND ON between calls: not this cache, not the
// operand cache unless the caller opts in.  (They do keep pattern hints, below: advisory state, which moves addresses and
// the order of execution and which no value can depend on -- a stale hint is at worst a slower call.)
struct PatternCache {
  std::mutex mu;
  bool enabled = env_switch("TSAMD_PATTERN_CACHE", true);
  // first: row, second: csr2csc.  key: E.  kept: row[csr2csc], gathered at the second sighting
  Entry pattern;
  // value[csr2csc] of FIXED edge weights (a value tensor that does not require grad, e.g. GCN's normalised
  // adjacency): valid while the pattern entry is and the value tensor keeps its identity.  key: dtype, length
  Entry values;
  // what the backwards did with the entry (torch.ops.tsamd.pattern_cache_stats; read by the tests only)
  int64_t row_hits = 0, value_hits = 0, value_fills = 0;
};

// torch.ops.tsamd.pattern_cache(enable) -> was enabled; drops the cached row ids
bool pattern_cache_ctl(bool enable) {
  PatternCache &c = state<PatternCache>();
  std::lock_guard<std::mutex> lock(c.mu);
  const bool was = c.enabled;
  c.enabled = enable;
  c.pattern.drop();
  c.values.drop();
  return was;
}

// torch.ops.tsamd.pattern_cache_stats() -> [enabled, backwards served from the kept row ids, backwards served from the
// kept value[csr2csc], gathers of value[csr2csc] into the entry]; the counters only grow
std::vector<int64_t> pattern_cache_stats() {
  PatternCache &c = state<PatternCache>();
  std::lock_guard<std::mutex> lock(c.mu);
  return {c.enabled ? 1 : 0, c.row_hits, c.value_hits, c.value_fills};
}

// ---- pattern hints (include/tsamd.h: tsamd_spmm_hinted) ---------------------------------------------------
// What the forward works out from (rowptr, col) alone -- the camping probe's verdict, the hot 64-id blocks and their
// ranks, the slot -> partition map of the column order -- is kept per pattern and reused by the later calls with the
// same pattern: the same tensors in every layer and every epoch.  ON by default and without a switch, for the bare
// reference ops too, because the ops keep no state THAT A RESULT CAN DEPEND ON: the hints are advisory (they choose
// addresses and the order of execution, never a value), a call with stale hints -- `col.data` overwritten in place,
// which no version counter sees -- returns the bits of a call without any, only more slowly.  That is the difference to
// the operand cache above, which keeps a copy of X: there a stale entry is a wrong result, hence opt-in.
// Four entries, least recently used out (forward and transposed pattern of a training step, times two graphs).  Key:
// the identities of rowptr and col plus every size the buffer's layout depends on (M, N, E, row bytes, dtype, reduction
// class, B), the device, the stream (the entry's buffer is allocated, written and read on that stream only, so
// replacing an entry is stream-ordered) and the column-order setting in force.  Inference tensors (no version counter),
// non-contiguous inputs, capturing streams and the verification mode go without.
struct PatternHints {
  // first: rowptr, second: col.  kept: the hints buffer; undefined: the slot is free
  struct Slot : Entry {
    uint64_t used = 0;
  };
  std::mutex mu;
  std::array<Slot, 4> slots;
  uint64_t clock = 0;
  int64_t builds = 0, reuses = 0;
};

// torch.ops.tsamd.pattern_hints() -> [entries, calls that built hints, calls that reused them]; drops every entry
// (tests only: the counters only grow)
std::vector<int64_t> pattern_hints_ctl() {
  PatternHints &h = state<PatternHints>();
  std::lock_guard<std::mutex> lock(h.mu);
  int64_t n = 0;
  for (auto &e : h.slots) {
    n += e.kept.defined() ? 1 : 0;
    e.drop();
  }
  return {n, h.builds, h.reuses};
}

}  // namespace

bool operand_cache_enabled() { return state<OperandCache>().enabled; }

OperandCopy operand_cache_copy(const Tensor &col, const Tensor &mat, int dt, int red, int64_t E, size_t bytes) {
  OperandCache &oc = state<OperandCache>();
  OperandCopy r;
  if (!oc.enabled || !may_remember(mat)) return r;
  void *stream = current_stream(mat);
  if (stream_is_capturing(stream)) return r;
  const uint32_t col_version = col.is_inference() ? 0u : TensorIdentity::version_of(col);
  Key key = {dt, minmax_class(red), (int64_t)mat.get_device(), (int64_t) reinterpret_cast<intptr_t>(col.data_ptr()),
             (int64_t)col_version, E};
  key.append(mat.sizes().begin(), mat.sizes().end());

  r.held = std::unique_lock<std::mutex>(oc.mu);
  Entry &e = oc.entry;
  r.valid = e.kept.defined() && (size_t)e.kept.numel() >= bytes && e.matches(key, stream, mat);
  if (!r.valid) {
    // a buffer is only ever touched on the stream it was allocated under (the caching allocator's reuse is
    // stream-ordered on that stream): another stream gets a fresh one instead of racing with pending work
    if (!e.kept.defined() || (size_t)e.kept.numel() < bytes || e.kept.get_device() != mat.get_device() ||
        e.stream != stream) {
      e.kept = Tensor();  // release before the new allocation
      e.kept = workspace(bytes, mat);
    }
    e.rearm(key, stream, mat);
  }
  ++(r.valid ? oc.hits : oc.fills);
  r.buf = e.kept;
  return r;
}

CscView pattern_cache_csc_view(const Tensor &row, const Tensor &csr2csc, const OptTensor &value, bool want_values) {
  CscView view;
  if (!may_remember(row) || !may_remember(csr2csc)) return view;
  void *stream = current_stream(row);
  if (stream_is_capturing(stream)) return view;
  Tensor v = want_values ? value.value().detach() : Tensor();
  const bool keep_values = want_values && !needs_grad(value.value()) && may_remember(v);
  {
    PatternCache &pc = state<PatternCache>();
    std::lock_guard<std::mutex> lock(pc.mu);
    if (!pc.enabled) return view;
    const Key key = {row.numel()};
    if (!pc.pattern.matches(key, stream, row, &csr2csc)) {
      // the FIRST backward with this pattern: the gather only pays off when the pattern comes back, so it is made on
      // the second sighting
      pc.pattern.rearm(key, stream, row, &csr2csc);
      pc.pattern.kept = Tensor();
      pc.values.drop();
      return view;
    }
    ++pc.row_hits;
    if (!pc.pattern.kept.defined()) pc.pattern.kept = row.index_select(0, csr2csc);
    view.row_t = pc.pattern.kept;
    if (keep_values) {
      // (matched against the pattern entry that this very call confirmed, under the same lock)
      const Key vkey = {(int64_t)v.scalar_type(), v.numel()};
      if (pc.values.kept.defined() && pc.values.matches(vkey, stream, v)) {
        ++pc.value_hits;
      } else {
        pc.values.kept = v.index_select(0, csr2csc);
        pc.values.rearm(vkey, stream, v);
        ++pc.value_fills;
      }
      view.value_t = pc.values.kept;
    }
  }
  if (want_values && !view.value_t.defined()) view.value_t = v.index_select(0, csr2csc);
  return view;
}

std::pair<Tensor, int> pattern_hints_for(const Tensor &rowptr, const Tensor &col, int dt, int red, int64_t B, int64_t M,
                                         int64_t N, int64_t K, int64_t E, const Tensor &like, void *stream) {
  const size_t bytes = tsamd_spmm_hints_bytes(dt, red, B, M, N, K, E);
  if (bytes == 0 || !may_remember(rowptr) || !may_remember(col) || tsamd_spmm_reference_order(-1) != 0 ||
      stream_is_capturing(stream))
    return {Tensor(), 0};
  const Key key = {M, N, E, K * (int64_t)like.element_size(), dt, minmax_class(red), B, (int64_t)like.get_device(),
                   (int64_t)tsamd_spmm_column_order(-1)};
  PatternHints &h = state<PatternHints>();
  std::lock_guard<std::mutex> lock(h.mu);
  PatternHints::Slot *same = nullptr, *victim = &h.slots[0];
  for (auto &e : h.slots) {
    if (e.kept.defined() && e.keyed(key, stream) && (size_t)e.kept.numel() >= bytes) {
      if (e.first.matches(rowptr) && e.second.matches(col)) {
        e.used = ++h.clock;
        ++h.reuses;
        return {e.kept, 2};
      }
      // the same arrays after a recorded write: the entry is built anew in place
      if (e.first.ptr == rowptr.data_ptr() && e.second.ptr == col.data_ptr()) same = &e;
    }
    if (victim->kept.defined() && (!e.kept.defined() || e.used < victim->used)) victim = &e;
  }
  PatternHints::Slot &e = same != nullptr ? *same : *victim;
  if (same == nullptr) {
    e.kept = Tensor();  // release before the new allocation
    e.kept = workspace(bytes, like);
  }
  e.rearm(key, stream, rowptr, &col);
  e.used = ++h.clock;
  ++h.builds;
  return {e.kept, 1};
}

void pattern_hints_drop(const Tensor &buf) {
  PatternHints &h = state<PatternHints>();
  std::lock_guard<std::mutex> lock(h.mu);
  for (auto &e : h.slots)
    if (e.kept.defined() && e.kept.data_ptr() == buf.data_ptr()) e.drop();
}

}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_spmm_state = torch::RegisterOperators()
                                      .op("tsamd::operand_cache", &operand_cache_ctl)
                                      .op("tsamd::pattern_cache", &pattern_cache_ctl)
                                      .op("tsamd::pattern_cache_stats", &pattern_cache_stats)
                                      .op("tsamd::pattern_hints", &pattern_hints_ctl);
