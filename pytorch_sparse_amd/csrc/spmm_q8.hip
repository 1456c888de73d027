// SpMM over quantised features: x is held as OCP fp8 (e4m3fn) codes xq [N, F], one byte per element, with one float32
// scale per row,
//   out[m, :] = reduce over e in [rowptr[m], rowptr[m+1]) of value[e] * scale[col[e]] * decode(xq[col[e], :])
// reduce is sum or mean, value and scale are float32 or NULL (ones), out is float32 or bfloat16, accumulation float32.
// The gather of a 128-wide row is 128 bytes -- one cache line -- where bfloat16 moves 256 and float32 512.
// tsamd_quantize_rows makes (xq, scale) from float32 / bfloat16 / float16 rows.
//
// The group-walk kernel of segtile.h.  A lane holds one PACKET of PW codes of the row (PW consecutive features) and
// PW float32 accumulators; a group of LPR lanes covers LPR packets, a row with more packets than 64 lanes takes column
// blocks (blockIdx.y).  A group walks L = 8 * LPR entries as 8 windows of LPR entries: a lane reads col[e], value[e]
// and scale[col[e]] of ONE entry of the window, forms w = value * scale once and the pair (col, w) is handed round the
// group; the gathers of four entries are issued before the first of them is decoded.  A 128-wide row is 8 lanes of 16
// bytes, so a wave has 8 rows x 4 entries = 32 cache lines in flight.
//
//   packet ladder   rows of xq are F bytes apart, so PW is the largest of 16 / 8 / 4 / 1 bytes that divides F and the
//                   address of xq: every packet of every row is then aligned and inside its row -- there is no ragged
//                   packet and no byte beyond xq + N * F is read.  LPR and L come from the ladder step of F ALONE
//                   (the workspace query cannot see pointers): a base off the boundary only takes more column blocks.
//   decode          v_cvt_pk_f32_fp8 on the low and on the high word of every dword of the packet (the OCP format of
//                   gfx950: 0x7f / 0xff are NaN, there is no infinity), then one fma per feature into the accumulator.
//   identity        accumulators start at -0.0f, the identity of IEEE addition: a row of one entry is w * decode(code)
//                   bit for bit, the sign of a zero included.
//   tile kernel     at the last entry of a row that began inside the chunk the accumulators are divided by the row
//                   length (mean), rounded to the output type and stored, as 16-byte packets where out allows.  A row
//                   cut by a chunk boundary leaves records of F float32 partial sums (records[chunk * F + column]).
//   fix-up          one wave per chunk with a head record, lanes over the columns: the tail records of the chunks
//                   [rowptr[s] / L, b) and then the head record are added in chunk order in fp64, rounded once.
//   fill            rows without entries are set to zero; the rest of out is written by the two kernels above.
//
// Workspace: nchunks = ceil(E / L),  2 * align256(4 * F * nchunks) [head, tail records] + 2 * align256(8 * nchunks)
// [their row ids, -1: no record].  No atomics, no host sync, three launches (fill, tile, fix-up), fixed combine tree:
// two calls give the same bits.
#include "segtile.h"

namespace tsamd {
namespace {

constexpr int kQ8Batch = 4;      // gathers in flight per lane
constexpr int64_t kQ8MaxF = 1024;

// ---- plan ------------------------------------------------------------------------------------------------------------
// largest ladder step that divides both F and the address
int q8_packet(int64_t F, const void *base) {
  const uint64_t a = (uint64_t)F | (uint64_t)reinterpret_cast<uintptr_t>(base);
  return (a & 15u) == 0 ? 16 : (a & 7u) == 0 ? 8 : (a & 3u) == 0 ? 4 : 1;
}

// lanes per row: from the packets of an aligned row
int q8_lg_lpr(int64_t F) {
  const int64_t packets = F > 0 ? F / q8_packet(F, nullptr) : 1;
  const int lg = lg_ceil(packets);
  return lg < 6 ? lg : 6;
}

struct Q8Plan {
  int pw, lg_lpr, ovec;
  int64_t blocks, chunk;
};

// the one place the route is decided: the driver and tsamd_spmm_q8_route both plan through it
Q8Plan q8_plan(int64_t F, const void *xq, const void *out) {
  Q8Plan p;
  p.pw = q8_packet(F, xq);
  p.lg_lpr = q8_lg_lpr(F);
  p.ovec = p.pw >= 4 && aligned16(out) ? 1 : 0;  // F is a multiple of 4 then: every row of out starts a packet
  p.blocks = F > 0 ? ceil_div(F / p.pw, (int64_t)1 << p.lg_lpr) : 1;
  p.chunk = (int64_t)kSegWindows << p.lg_lpr;
  return p;
}

// head and tail records: a row of F float32 partial sums each
SegRecords q8_records(int64_t chunk, int64_t F, int64_t E) {
  const size_t row = sizeof(float) * (size_t)(F > 0 ? F : 1);
  return SegRecords(E, chunk, {row, row});
}

bool q8_out_dtype(int dtype) { return dtype == TSAMD_F32 || dtype == TSAMD_BF16; }

// sizes the 32-bit ids and the grid can carry
bool q8_indexable(int64_t M, int64_t N, int64_t E) {
  const int64_t lim = (int64_t)1 << 32;
  return M < lim / 2 && N < lim && E < lim;
}

// ---- packets ---------------------------------------------------------------------------------------------------------
template <int PW>
struct Q8Codes {
  uint32_t d[PW >= 4 ? PW / 4 : 1];
};

template <int PW>
__device__ __forceinline__ Q8Codes<PW> q8_load(const uint8_t *__restrict__ p) {
  Q8Codes<PW> c;
  if constexpr (PW == 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    c.d[0] = v.x, c.d[1] = v.y, c.d[2] = v.z, c.d[3] = v.w;
  } else if constexpr (PW == 8) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    c.d[0] = v.x, c.d[1] = v.y;
  } else if constexpr (PW == 4) {
    c.d[0] = *reinterpret_cast<const uint32_t *>(p);
  } else {
    c.d[0] = *p;
  }
  return c;
}

// acc[f] = fma(w, decode(code f), acc[f]): two v_cvt_pk_f32_fp8 per dword
template <int PW>
__device__ __forceinline__ void q8_fma(float w, const Q8Codes<PW> &c, float (&acc)[PW]) {
  if constexpr (PW == 1) {
    acc[0] = __builtin_fmaf(w, __builtin_amdgcn_cvt_pk_f32_fp8((int)c.d[0], false)[0], acc[0]);
  } else {
#pragma unroll
    for (int i = 0; i < PW / 4; ++i) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.d[i], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.d[i], true);
      acc[4 * i + 0] = __builtin_fmaf(w, lo[0], acc[4 * i + 0]);
      acc[4 * i + 1] = __builtin_fmaf(w, lo[1], acc[4 * i + 1]);
      acc[4 * i + 2] = __builtin_fmaf(w, hi[0], acc[4 * i + 2]);
      acc[4 * i + 3] = __builtin_fmaf(w, hi[1], acc[4 * i + 3]);
    }
  }
}

// a finished packet of a row: mean, the rounding to O, packets of 16 bytes (8 for four bfloat16) where `vec`
template <typename O, int PW>
__device__ __forceinline__ void q8_store(O *__restrict__ p, const float (&acc)[PW], bool mean, float n, bool vec) {
  constexpr int kStep = PW < 16 / (int)sizeof(O) ? PW : 16 / (int)sizeof(O);
  O o[PW];
#pragma unroll
  for (int v = 0; v < PW; ++v) o[v] = Traits<O>::from_acc(mean ? acc[v] / n : acc[v]);
  if (vec) {
#pragma unroll
    for (int v = 0; v < PW; v += kStep) {
      Pack<O, kStep> pk;
#pragma unroll
      for (int u = 0; u < kStep; ++u) pk.v[u] = o[v + u];
      *reinterpret_cast<Pack<O, kStep> *>(p + v) = pk;
    }
  } else {
#pragma unroll
    for (int v = 0; v < PW; ++v) p[v] = o[v];
  }
}

struct Q8Args {
  const int64_t *ptr, *ind;
  const float *value, *scale;
  const uint8_t *xq;
  void *out;
  float *head_val, *tail_val;
  int64_t *head_seg, *tail_seg;
  int64_t nseg, E, F, L, nchunks;
  int lg_lpr, mean, ovec;
};

// ---- tile kernel -----------------------------------------------------------------------------------------------------
template <typename O, int PW>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_q8_tile_kernel(const Q8Args a) {
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
  const int64_t chunk = geo.chunk, c0 = geo.c0, F = a.F;
  const int64_t col0 = ((int64_t)blockIdx.y * lpr + geo.gl) * PW;
  const bool colok = col0 < F;  // PW divides F: a packet is inside the row or outside
  const bool scribe = geo.gl == 0 && blockIdx.y == 0;  // writes the row ids of the chunk's records
  const bool mean = a.mean != 0, ovec = a.ovec != 0;
  O *__restrict__ out = reinterpret_cast<O *>(a.out);

  float acc[PW];
#pragma unroll
  for (int v = 0; v < PW; ++v) acc[v] = -0.0f;
  bool open = false, had_head = false;
  int32_t cur = -1;  // row of the last entry taken

  for (int w = 0; w < kSegWindows; ++w) {
    // one entry of the window per lane of the group: its row, its column and its weight
    const int64_t e = c0 + (int64_t)w * lpr + geo.gl;
    GroupEntry mine = {0, 0, 0};
    float w_l = 0.0f, n_l = 1.0f;
    if (e < geo.c1) {
      const SegEntry en = slice_entry(slice, a.ptr, sp, e);
      mine.seg = (int32_t)en.seg;
      mine.col = (uint32_t)a.ind[e];
      mine.fl = kSegValid | (e + 1 == en.end ? kSegEnd : 0) | (en.start >= c0 ? kSegFresh : 0);
      w_l = a.value ? a.value[e] : 1.0f;
      if (a.scale) w_l *= a.scale[mine.col];
      n_l = (float)(en.end - en.start);
    }
    for (int j0 = 0; j0 < lpr; j0 += kQ8Batch) {  // wave-uniform: every lane answers the lane reads
      int32_t fl[kQ8Batch], sg[kQ8Batch];
      float ww[kQ8Batch], nn[kQ8Batch];
      Q8Codes<PW> xv[kQ8Batch];
#pragma unroll
      for (int u = 0; u < kQ8Batch; ++u) {
        const int j = j0 + u;
        const GroupEntry en = group_broadcast(geo, mine, j);
        fl[u] = en.fl;
        sg[u] = en.seg;
        ww[u] = lane_read(w_l, group_src(geo, j));
        nn[u] = mean ? lane_read(n_l, group_src(geo, j)) : 1.0f;
        xv[u] = Q8Codes<PW>();
        if ((fl[u] & kSegValid) && colok)
          xv[u] = q8_load<PW>(a.xq + (uint64_t)en.col * (uint64_t)F + (uint64_t)col0);
      }
#pragma unroll
      for (int u = 0; u < kQ8Batch; ++u) {
        if (fl[u] & kSegValid) {  // an entry beyond the chunk adds nothing: no 0 * NaN
          cur = sg[u];
          open = true;
          q8_fma<PW>(ww[u], xv[u], acc);
        }
        if (fl[u] & kSegEnd) {
          if (fl[u] & kSegFresh) {
            if (colok) q8_store<O, PW>(out + (uint64_t)sg[u] * (uint64_t)F + (uint64_t)col0, acc, mean, nn[u], ovec);
          } else {  // began before this chunk: the fix-up kernel finishes it
            had_head = true;
            if (colok) {
#pragma unroll
              for (int v = 0; v < PW; ++v) a.head_val[(uint64_t)chunk * (uint64_t)F + (uint64_t)col0 + v] = acc[v];
            }
            if (scribe) a.head_seg[chunk] = sg[u];
          }
#pragma unroll
          for (int v = 0; v < PW; ++v) acc[v] = -0.0f;
          open = false;
        }
      }
    }
  }
  if (c0 < e1) {
    if (open && colok) {
#pragma unroll
      for (int v = 0; v < PW; ++v) a.tail_val[(uint64_t)chunk * (uint64_t)F + (uint64_t)col0 + v] = acc[v];
    }
    group_record_ids(geo, scribe, open, had_head, cur, a.head_seg, a.tail_seg);
  }
}

// ---- fix-up ----------------------------------------------------------------------------------------------------------
template <typename O>
__global__ __launch_bounds__(kSegWaves *kWave) void spmm_q8_fixup_kernel(const Q8Args a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (b >= a.nchunks) return;
  const int64_t s = a.head_seg[b];
  if (s < 0) return;
  const int64_t start = a.ptr[s];
  const int64_t first = start / a.L;  // every chunk in [first, b) ended inside s: its tail record is a piece of s
  const float n = (float)(a.ptr[s + 1] - start);
  O *__restrict__ out = reinterpret_cast<O *>(a.out);
  for (int64_t col = lane; col < a.F; col += kWave) {
    double sum = -0.0;
    for (int64_t i = first; i < b; ++i) sum += (double)a.tail_val[(uint64_t)i * (uint64_t)a.F + (uint64_t)col];
    sum += (double)a.head_val[(uint64_t)b * (uint64_t)a.F + (uint64_t)col];
    const float r = (float)sum;
    out[(uint64_t)s * (uint64_t)a.F + (uint64_t)col] = Traits<O>::from_acc(a.mean ? r / n : r);
  }
}

// rows without entries (ptr == NULL: every row)
template <typename O>
__global__ __launch_bounds__(256) void spmm_q8_fill_kernel(const int64_t *__restrict__ ptr, O *__restrict__ out,
                                                           int64_t nseg, int64_t F) {
  const int64_t total = nseg * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / F;
    if (ptr && ptr[row] != ptr[row + 1]) continue;
    out[i] = O{};
  }
}

template <typename O>
int launch_q8_fill(const int64_t *ptr, void *out, int64_t M, int64_t F, hipStream_t stream) {
  const int64_t blocks = ceil_div(M * F, (int64_t)256);
  hipLaunchKernelGGL((spmm_q8_fill_kernel<O>), dim3((unsigned int)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     stream, ptr, reinterpret_cast<O *>(out), M, F);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

template <typename O>
int launch_spmm_q8(const Q8Plan &p, const Q8Args &a, hipStream_t stream) {
  const int st = launch_q8_fill<O>(a.ptr, a.out, a.nseg, a.F, stream);
  if (st != TSAMD_OK) return st;
  const dim3 block(kSegWaves * kWave);
  const dim3 tiles((unsigned int)ceil_div(a.E, (int64_t)kExpandTile), (unsigned int)p.blocks);
  switch (p.pw) {
    case 16: hipLaunchKernelGGL((spmm_q8_tile_kernel<O, 16>), tiles, block, 0, stream, a); break;
    case 8: hipLaunchKernelGGL((spmm_q8_tile_kernel<O, 8>), tiles, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((spmm_q8_tile_kernel<O, 4>), tiles, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((spmm_q8_tile_kernel<O, 1>), tiles, block, 0, stream, a); break;
  }
  TSAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((spmm_q8_fixup_kernel<O>), dim3((unsigned int)ceil_div(a.nchunks, (int64_t)kSegWaves)), block, 0,
                     stream, a);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

// ---- quantize_rows ---------------------------------------------------------------------------------------------------
// A group of LPR lanes per row, a lane holds VEC consecutive elements per sweep of the row.  First the absmax of the row
// (a butterfly over the group: max is exact, every lane ends with the same value), then per element the IEEE divide by
// scale = absmax / 448, the clamp to +-448 and v_cvt_pk_fp8_f32 (round-to-nearest-even), stored as one dword of four
// codes where VEC = 4.  The packet of the first sweep stays in registers; a row wider than LPR * VEC is read again.
template <typename T>
__device__ __forceinline__ float q8_to_f32(T v) {
  return Traits<T>::to_acc(v);
}

__device__ __forceinline__ float q8_scaled(float v, float scale) {
  return __builtin_fminf(__builtin_fmaxf(__fdiv_rn(v, scale), -448.0f), 448.0f);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const T *__restrict__ x, uint8_t *__restrict__ xq,
                                                            float *__restrict__ scale, int64_t N, int64_t F,
                                                            int lg_lpr) {
  const int lane = (int)(threadIdx.x & 63);
  const int lpr = 1 << lg_lpr, gl = lane & (lpr - 1);
  const int64_t row = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> lg_lpr);
  const bool rowok = row < N;  // the butterfly below is wave-wide: no lane leaves before it
  const T *__restrict__ xr = x + (uint64_t)(rowok ? row : 0) * (uint64_t)F;
  const int64_t sweep = (int64_t)lpr * VEC;

  Pack<T, VEC> first = {};
  float amax = 0.0f;
  for (int64_t f0 = (int64_t)gl * VEC; f0 < F && rowok; f0 += sweep) {
    const Pack<T, VEC> pk = *reinterpret_cast<const Pack<T, VEC> *>(xr + f0);
    if (f0 < sweep) first = pk;
#pragma unroll
    for (int v = 0; v < VEC; ++v) amax = __builtin_fmaxf(amax, __builtin_fabsf(q8_to_f32(pk.v[v])));
  }
  for (int off = 1; off < lpr; off <<= 1) amax = __builtin_fmaxf(amax, lane_xor(amax, off));
  if (!rowok) return;
  const float s = amax == 0.0f ? 1.0f : __fdiv_rn(amax, 448.0f);
  if (gl == 0) scale[row] = s;

  uint8_t *__restrict__ qr = xq + (uint64_t)row * (uint64_t)F;
  for (int64_t f0 = (int64_t)gl * VEC; f0 < F; f0 += sweep) {
    const Pack<T, VEC> pk = f0 < sweep ? first : *reinterpret_cast<const Pack<T, VEC> *>(xr + f0);
    if constexpr (VEC == 4) {
      int codes = 0;
      codes = __builtin_amdgcn_cvt_pk_fp8_f32(q8_scaled(q8_to_f32(pk.v[0]), s), q8_scaled(q8_to_f32(pk.v[1]), s), codes,
                                              false);
      codes = __builtin_amdgcn_cvt_pk_fp8_f32(q8_scaled(q8_to_f32(pk.v[2]), s), q8_scaled(q8_to_f32(pk.v[3]), s), codes,
                                              true);
      *reinterpret_cast<uint32_t *>(qr + f0) = (uint32_t)codes;
    } else {
      const float q = q8_scaled(q8_to_f32(pk.v[0]), s);
      qr[f0] = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(q, q, 0, false) & 0xff);
    }
  }
}

template <typename T>
int launch_quantize_rows(const void *x, void *xq, float *scale, int64_t N, int64_t F, hipStream_t stream) {
  // four elements per lane where the rows of x and of xq start on a packet
  const bool vec = F % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(T) - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(xq) & 3u) == 0;
  const int lg = lg_ceil(vec ? F / 4 : F);
  const int lg_lpr = lg < 6 ? lg : 6;
  const int64_t blocks = ceil_div(N << lg_lpr, (int64_t)256);
  const T *xx = reinterpret_cast<const T *>(x);
  uint8_t *qq = reinterpret_cast<uint8_t *>(xq);
  if (vec)
    hipLaunchKernelGGL((quantize_rows_kernel<T, 4>), dim3((unsigned int)blocks), dim3(256), 0, stream, xx, qq, scale, N,
                       F, lg_lpr);
  else
    hipLaunchKernelGGL((quantize_rows_kernel<T, 1>), dim3((unsigned int)blocks), dim3(256), 0, stream, xx, qq, scale, N,
                       F, lg_lpr);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

}  // namespace
}  // namespace tsamd

using namespace tsamd;

extern "C" int tsamd_spmm_q8_route(int out_dtype, int64_t F, int64_t E, const void *xq, const void *out,
                                   int64_t route[16]) {
  if (!route || F < 0 || E < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 16; ++i) route[i] = 0;
  if (!q8_out_dtype(out_dtype) || F > kQ8MaxF || !q8_indexable(0, 0, E)) return TSAMD_ERR_UNSUPPORTED;
  const Q8Plan p = q8_plan(F, xq, out);
  const SegRecords rec = q8_records(p.chunk, F, E);
  route[0] = p.pw;
  route[1] = (int64_t)1 << p.lg_lpr;
  route[2] = (int64_t)64 >> p.lg_lpr;
  route[3] = p.chunk;
  route[4] = kExpandTile;
  route[5] = p.blocks;
  route[6] = p.ovec;
  route[7] = kQ8Batch;
  route[8] = (int64_t)rec.nchunks;
  route[9] = (int64_t)(rec.off[1] - rec.off[0]);  // bytes of the head records; the tail records are as many
  route[10] = (int64_t)(rec.off[3] - rec.off[2]);  // bytes of the head row ids; the tail row ids are as many
  route[11] = (int64_t)rec.bytes();
  return TSAMD_OK;
}

extern "C" size_t tsamd_spmm_q8_workspace_bytes(int out_dtype, int64_t M, int64_t F, int64_t E) {
  if (!q8_out_dtype(out_dtype) || M < 0 || F < 0 || E < 0 || F > kQ8MaxF || !q8_indexable(M, 0, E)) return 0;
  return q8_records((int64_t)kSegWindows << q8_lg_lpr(F), F, E).bytes();
}

extern "C" int tsamd_spmm_q8(int out_dtype, int reduce, const int64_t *rowptr, const int64_t *col, const float *value,
                             const void *xq, const float *scale, void *out, int64_t M, int64_t N, int64_t F,
                             int64_t E, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (M < 0 || N < 0 || F < 0 || E < 0) return TSAMD_ERR_INVALID;
  if ((reduce != TSAMD_SUM && reduce != TSAMD_MEAN) || !q8_out_dtype(out_dtype) || F > kQ8MaxF ||
      !q8_indexable(M, N, E))
    return TSAMD_ERR_UNSUPPORTED;
  if (M * F == 0) return TSAMD_OK;  // out has no element
  if (!out) return TSAMD_ERR_INVALID;
  if (E == 0)  // every row is empty
    return out_dtype == TSAMD_F32 ? launch_q8_fill<float>(nullptr, out, M, F, stream)
                                  : launch_q8_fill<bf16_t>(nullptr, out, M, F, stream);
  if (N == 0 || !rowptr || !col || !xq) return TSAMD_ERR_INVALID;
  if (!workspace || workspace_bytes < tsamd_spmm_q8_workspace_bytes(out_dtype, M, F, E) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255u) != 0)
    return TSAMD_ERR_WORKSPACE;
  const Q8Plan p = q8_plan(F, xq, out);
  const SegRecords rec = q8_records(p.chunk, F, E);
  Q8Args a;
  a.ptr = rowptr, a.ind = col, a.value = value, a.scale = scale;
  a.xq = reinterpret_cast<const uint8_t *>(xq);
  a.out = out;
  a.head_val = rec.plane<float>(workspace, 0), a.tail_val = rec.plane<float>(workspace, 1);
  a.head_seg = rec.head_seg(workspace), a.tail_seg = rec.tail_seg(workspace);
  a.nseg = M, a.E = E, a.F = F, a.L = p.chunk, a.nchunks = (int64_t)rec.nchunks;
  a.lg_lpr = p.lg_lpr, a.mean = reduce == TSAMD_MEAN ? 1 : 0, a.ovec = p.ovec;
  return out_dtype == TSAMD_F32 ? launch_spmm_q8<float>(p, a, stream) : launch_spmm_q8<bf16_t>(p, a, stream);
}

extern "C" int tsamd_quantize_rows(int dtype, const void *x, void *xq, float *scale, int64_t N, int64_t F,
                                   void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (N < 0 || F < 0) return TSAMD_ERR_INVALID;
  if (dtype != TSAMD_F32 && dtype != TSAMD_BF16 && dtype != TSAMD_F16) return TSAMD_ERR_UNSUPPORTED;
  if (N >= ((int64_t)1 << 31) || F >= ((int64_t)1 << 31)) return TSAMD_ERR_UNSUPPORTED;
  if (N == 0) return TSAMD_OK;
  if (!scale || (F > 0 && (!x || !xq))) return TSAMD_ERR_INVALID;
  switch (dtype) {
    case TSAMD_F32: return launch_quantize_rows<float>(x, xq, scale, N, F, stream);
    case TSAMD_BF16: return launch_quantize_rows<bf16_t>(x, xq, scale, N, F, stream);
    default: return launch_quantize_rows<f16_t>(x, xq, scale, N, F, stream);
  }
}
