// edit_ann.hip -- the device side of include/edit_ann.h: the exhaustive index under the EditDistance metric.
//
// Distance: one lane per stored row runs edit_core::distance (edit_myers.h) against the match-mask table of one query,
// which the workgroup builds in LDS once and its four waves (four tiles of 64 rows) share.  The rows lie in tiles of 64
// consecutive slots, transposed [position][lane] at the tile's own greatest length, so a wave's load of position j is one
// 256-byte line; a lane stops at its own row's end under the execution mask.  A workgroup walks QUERY_TILE queries over its
// rows, and writes one uint16 distance per (query, slot) into the scratch of the pass.
//
// Selection cannot refuse: distances lie in 0..256, so the k nearest are all slots below a threshold distance t plus the
// first `need` slots at t, in slot order -- and slots are kept in (id, position) order, so "first" means "smallest id".
// Per pass: a 257-bin histogram per query (LDS, then global), the threshold, per-chunk counts of both classes, their scan,
// the ordered emit of exactly min(k, n) keys (distance << 32 | slot), and a bitonic sort of those in LDS.
//
// The 64-bit words of the distance step cost two vector instructions per add or shift on this machine; whether 32-bit words
// would do better has not been measured.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_buf.h"
#include "edit_internal.h"
#include "edit_myers.h"

using edit_host::check_csr;
using edit_host::fail;

#define HTRY(expr)                                                                                     \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(EDIT_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {

constexpr int TILE = 64;                 // rows per tile = lanes per wave
constexpr int BLOCK = 256;               // threads per workgroup, every kernel but the pair kernel
constexpr int TILES_PER_BLOCK = BLOCK / TILE;
constexpr int QUERY_TILE = 16;           // queries a distance workgroup walks over its rows
constexpr int SLOTS_PER_THREAD = 16;
constexpr int CHUNK = BLOCK * SLOTS_PER_THREAD;  // slots per select workgroup
constexpr int HIST_CHUNKS = 4;           // chunks per histogram workgroup
constexpr int BINS = edit_core::MAX_LEN + 1;
constexpr int MAX_SLICE = 4096;
constexpr size_t SCRATCH_BUDGET = (size_t)256 << 20;
constexpr int64_t MAX_ROWS = ((int64_t)1 << 31) - 64;
constexpr int64_t PAIRS_PER_LAUNCH = (int64_t)1 << 20;

// ---- the table of one pattern, built by all `threads` threads of the workgroup -------------------------------------------
// keys [TABLE_SLOTS], masks [TABLE_SLOTS * words].  Ends with a barrier: the table is readable on return.
__device__ void build_table(uint32_t *keys, uint64_t *masks, const uint32_t *pattern, int m, int words, int tid, int threads) {
  for (int i = tid; i < edit_core::TABLE_SLOTS; i += threads) keys[i] = edit_core::EMPTY_KEY;
  for (int i = tid; i < edit_core::TABLE_SLOTS * words; i += threads) masks[i] = 0;
  __syncthreads();
  for (int i = tid; i < m; i += threads) {
    const uint32_t c = edit_core::canonical(pattern[i]);
    if (edit_core::is_nan(c)) continue;
    uint32_t h = edit_core::slot_of(c);
    for (int probe = 0; probe < edit_core::TABLE_SLOTS; probe++) {  // (at most 256 keys in 512 slots: it ends long before)
      const uint32_t old = atomicCAS(&keys[h], edit_core::EMPTY_KEY, c);
      if (old == edit_core::EMPTY_KEY || old == c) break;
      h = (h + 1) & (edit_core::TABLE_SLOTS - 1);
    }
    atomicOr((unsigned long long *)&masks[(int)h * words + (i >> 6)], 1ull << (i & 63));
  }
  __syncthreads();
}

// grid (ceil(n_tiles / 4), ceil(qs / QUERY_TILE)).  tile_off in elements; row_len [n_tiles * 64], 0 on the padding slots;
// q_off [qs + 1] into q_chars; dist [qs][n_tiles * 64].
__global__ __launch_bounds__(BLOCK) void edit_distance_kernel(const uint32_t *__restrict__ tiles, const int64_t *__restrict__ tile_off,
                                                              const int32_t *__restrict__ row_len, int64_t n_tiles,
                                                              const uint32_t *__restrict__ q_chars, const int32_t *__restrict__ q_off, int qs,
                                                              uint16_t *__restrict__ dist) {
  __shared__ uint32_t keys[edit_core::TABLE_SLOTS];
  __shared__ uint64_t masks[edit_core::TABLE_SLOTS * edit_core::MAX_WORDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t tile = (int64_t)blockIdx.x * TILES_PER_BLOCK + (tid >> 6);
  const bool have = tile < n_tiles;
  const int64_t slot = tile * TILE + lane;
  const uint32_t *text = have ? tiles + tile_off[tile] + lane : tiles;
  const int len = have ? row_len[slot] : 0;
  const int64_t n_pad = n_tiles * TILE;
  const int q1 = min((int)(blockIdx.y + 1) * QUERY_TILE, qs);
  for (int q = blockIdx.y * QUERY_TILE; q < q1; q++) {
    const int o = q_off[q], m = q_off[q + 1] - o;
    __syncthreads();  // every lane is done with the previous query's table
    build_table(keys, masks, q_chars + o, m, (m + 63) >> 6, tid, BLOCK);
    if (have) dist[(size_t)q * n_pad + slot] = (uint16_t)edit_core::distance_any(keys, masks, m, text, TILE, len);
  }
}

// One workgroup of one wave per pair: a is the pattern, b the text, every lane computes the same distance.
__global__ __launch_bounds__(TILE) void edit_pairs_kernel(const uint32_t *__restrict__ a_chars, const int64_t *__restrict__ a_off,
                                                          const uint32_t *__restrict__ b_chars, const int64_t *__restrict__ b_off,
                                                          int64_t p0, int64_t n_pairs, int32_t *__restrict__ out) {
  __shared__ uint32_t keys[edit_core::TABLE_SLOTS];
  __shared__ uint64_t masks[edit_core::TABLE_SLOTS * edit_core::MAX_WORDS];
  const int64_t p = p0 + blockIdx.x;
  if (p >= n_pairs) return;
  const int m = (int)(a_off[p + 1] - a_off[p]), n = (int)(b_off[p + 1] - b_off[p]);
  build_table(keys, masks, a_chars + a_off[p], m, (m + 63) >> 6, threadIdx.x, TILE);
  const int32_t d = edit_core::distance_any(keys, masks, m, b_chars + b_off[p], 1, n);
  if (threadIdx.x == 0) out[p] = d;
}

// ---- selection ----------------------------------------------------------------------------------------------------------
// grid (ceil(n / (CHUNK * HIST_CHUNKS)), qs); hist [qs][BINS], zeroed before
__global__ __launch_bounds__(BLOCK) void edit_hist_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int64_t n, uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[BINS];
  const int tid = threadIdx.x, q = blockIdx.y;
  for (int b = tid; b < BINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const int64_t s0 = (int64_t)blockIdx.x * (CHUNK * HIST_CHUNKS), s1 = min(s0 + CHUNK * HIST_CHUNKS, n);
  const uint16_t *row = dist + (size_t)q * n_pad;
  for (int64_t s = s0 + tid; s < s1; s += BLOCK) atomicAdd(&h[min((int)row[s], BINS - 1)], 1u);
  __syncthreads();
  for (int b = tid; b < BINS; b += BLOCK)
    if (h[b]) atomicAdd(&hist[(size_t)q * BINS + b], h[b]);
}

// one thread per query: info[q] = (t, need, total below t, 0) with kq = min(k, n) >= 1
__global__ void edit_threshold_kernel(const uint32_t *__restrict__ hist, int qs, uint32_t kq, int4 *__restrict__ info) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= qs) return;
  uint32_t below = 0;
  int t = 0;
  for (; t < BINS - 1; t++) {
    const uint32_t c = hist[(size_t)q * BINS + t];
    if (below + c >= kq) break;
    below += c;
  }
  info[q] = make_int4(t, (int)(kq - below), (int)below, 0);
}

// exclusive scan of one value per thread over the workgroup; `total` is the sum.  wave_sums: LDS [BLOCK / 64]
__device__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();  // the sums of an earlier call have been read
  if (lane == 63) wave_sums[wave] = x;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; w++) {
    if (w < wave) base += wave_sums[w];
    all += wave_sums[w];
  }
  *total = all;
  return base + x - v;
}

// The 16 consecutive slots of a thread: how many lie below t (low half) and at t (high half).
__device__ uint32_t classify(const uint16_t *row, int64_t s0, int64_t n, int t) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < SLOTS_PER_THREAD; i++) {
    if (s0 + i < n) {
      const int d = row[s0 + i];
      c += d < t ? 1u : d == t ? 0x10000u : 0u;
    }
  }
  return c;
}

// grid (n_chunks, qs): cnt_lt / cnt_eq [qs][n_chunks]
__global__ __launch_bounds__(BLOCK) void edit_count_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int64_t n, const int4 *__restrict__ info,
                                                           int n_chunks, uint32_t *__restrict__ cnt_lt, uint32_t *__restrict__ cnt_eq) {
  __shared__ uint32_t wave_sums[BLOCK / 64];
  const int q = blockIdx.y;
  const int64_t s0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * SLOTS_PER_THREAD;
  uint32_t total;
  (void)block_exclusive_scan(classify(dist + (size_t)q * n_pad, s0, n, info[q].x), wave_sums, &total);
  if (threadIdx.x == 0) {
    cnt_lt[(size_t)q * n_chunks + blockIdx.x] = total & 0xffffu;
    cnt_eq[(size_t)q * n_chunks + blockIdx.x] = total >> 16;
  }
}

// grid (qs): pre_* [qs][n_chunks] = exclusive scans of cnt_* along the chunks
__global__ __launch_bounds__(BLOCK) void edit_scan_kernel(const uint32_t *__restrict__ cnt_lt, const uint32_t *__restrict__ cnt_eq, int n_chunks,
                                                          uint32_t *__restrict__ pre_lt, uint32_t *__restrict__ pre_eq) {
  __shared__ uint32_t wave_sums[BLOCK / 64];
  const size_t base = (size_t)blockIdx.x * n_chunks;
  uint32_t carry_lt = 0, carry_eq = 0;
  for (int c0 = 0; c0 < n_chunks; c0 += BLOCK) {
    const int c = c0 + threadIdx.x;
    const bool in = c < n_chunks;
    uint32_t total;
    const uint32_t e_lt = block_exclusive_scan(in ? cnt_lt[base + c] : 0u, wave_sums, &total);
    if (in) pre_lt[base + c] = carry_lt + e_lt;
    carry_lt += total;
    const uint32_t e_eq = block_exclusive_scan(in ? cnt_eq[base + c] : 0u, wave_sums, &total);
    if (in) pre_eq[base + c] = carry_eq + e_eq;
    carry_eq += total;
  }
}

// grid (n_chunks, qs): cand [qs][EDIT_MAX_K].  Writes entry r of the query's answer set exactly once for every r < min(k, n):
// the slots below t at their rank among those, then the first `need` slots at t.
__global__ __launch_bounds__(BLOCK) void edit_emit_kernel(const uint16_t *__restrict__ dist, int64_t n_pad, int64_t n, const int4 *__restrict__ info,
                                                          int n_chunks, const uint32_t *__restrict__ cnt_lt, const uint32_t *__restrict__ cnt_eq,
                                                          const uint32_t *__restrict__ pre_lt, const uint32_t *__restrict__ pre_eq,
                                                          uint64_t *__restrict__ cand) {
  __shared__ uint32_t wave_sums[BLOCK / 64];
  const int q = blockIdx.y;
  const size_t ci = (size_t)q * n_chunks + blockIdx.x;
  const int4 in = info[q];
  const uint32_t t = in.x, need = in.y, below = in.z;
  const uint32_t base_lt = pre_lt[ci], base_eq = pre_eq[ci];
  if (cnt_lt[ci] == 0 && (cnt_eq[ci] == 0 || base_eq >= need)) return;  // (uniform over the workgroup)
  const uint16_t *row = dist + (size_t)q * n_pad;
  const int64_t s0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * SLOTS_PER_THREAD;
  uint32_t total;
  const uint32_t e = block_exclusive_scan(classify(row, s0, n, (int)t), wave_sums, &total);
  uint32_t r_lt = base_lt + (e & 0xffffu), r_eq = base_eq + (e >> 16);
  uint64_t *out = cand + (size_t)q * EDIT_MAX_K;
#pragma unroll
  for (int i = 0; i < SLOTS_PER_THREAD; i++) {
    if (s0 + i < n) {
      const uint32_t d = row[s0 + i];
      const uint64_t key = ((uint64_t)d << 32) | (uint64_t)(s0 + i);
      if (d < t) {
        if (r_lt < EDIT_MAX_K) out[r_lt] = key;
        r_lt++;
      } else if (d == t) {
        if (r_eq < need && below + r_eq < EDIT_MAX_K) out[below + r_eq] = key;
        r_eq++;
      }
    }
  }
}

// grid (qs): sorts the kq keys of a query by (distance, slot) -- slots are in (id, position) order -- and writes the answer
__global__ __launch_bounds__(BLOCK) void edit_sort_kernel(const uint64_t *__restrict__ cand, const int64_t *__restrict__ ids, int64_t n, int kq, int k,
                                                          int32_t *__restrict__ out_dist, int64_t *__restrict__ out_ids) {
  __shared__ uint64_t a[EDIT_MAX_K];
  const int q = blockIdx.x, tid = threadIdx.x;
  int p = 2;
  while (p < kq) p <<= 1;
  for (int i = tid; i < p; i += BLOCK) a[i] = i < kq ? cand[(size_t)q * EDIT_MAX_K + i] : ~0ull;
  __syncthreads();
  for (int size = 2; size <= p; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < p / 2; i += BLOCK) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t x = a[lo], y = a[hi];
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += BLOCK) {
    const bool in = i < kq;
    const uint64_t key = in ? a[i] : 0;
    out_dist[(size_t)q * k + i] = in ? (int32_t)(key >> 32) : -1;
    const uint32_t slot = (uint32_t)key;
    out_ids[(size_t)q * k + i] = in && slot < n ? ids[slot] : -1;  // (every key is a slot below n: the bound is a seat belt)
  }
}

uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

hipError_t grow(Buf &b, size_t keep, size_t want) {
  if (b.p && want <= b.bytes) return hipSuccess;
  return b.grow_keep(keep, std::max(want, b.bytes + b.bytes / 2));
}

}  // namespace

struct edit_index {
  int32_t device = 0;
  bool has_ids = false;
  // the rows in arrival order
  std::vector<int64_t> off{0};
  std::vector<float> chars;
  std::vector<int64_t> ids;    // has_ids only
  std::vector<int64_t> order;  // has_ids only: slot -> position, sorted by (id, position)
  int64_t max_id = 0;
  int32_t max_len = 0;
  // the device copy: slots [0, dev_rows) are laid
  int64_t dev_rows = 0;
  std::vector<int64_t> tile_off{0};
  Buf d_tiles, d_tile_off, d_len, d_ids;
  // search scratch
  Buf d_dist, d_hist, d_info, d_cnt, d_cand, d_qoff, d_qchars, d_out_dist, d_out_ids;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int32_t slice = 0;
  float distance_ms = 0, select_ms = 0;
  int64_t pairs = 0, cells = 0;

  int64_t rows() const { return (int64_t)off.size() - 1; }
  int64_t position(int64_t slot) const { return has_ids ? order[slot] : slot; }
  ~edit_index() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// validated arguments only; the index is unchanged when this throws (every allocation comes first)
void append_rows(edit_index &ix, int64_t n, const int64_t *offsets, const float *chars, const int64_t *ids) {
  if (n == 0) return;
  const int64_t n_old = ix.rows(), c0 = offsets[0], nc = offsets[n] - c0;
  std::vector<int64_t> batch;
  if (ix.has_ids) {
    batch.resize(n);
    for (int64_t i = 0; i < n; i++) batch[i] = n_old + i;
    std::stable_sort(batch.begin(), batch.end(), [&](int64_t a, int64_t b) { return ids[a - n_old] < ids[b - n_old]; });
    ix.ids.reserve(n_old + n);
    ix.order.reserve(n_old + n);
  }
  ix.off.reserve(n_old + n + 1);
  ix.chars.reserve(ix.chars.size() + nc);
  // nothing below allocates
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = offsets[i + 1] - offsets[i];
    ix.off.push_back(ix.off.back() + len);
    ix.max_len = std::max(ix.max_len, (int32_t)len);
  }
  if (nc) ix.chars.insert(ix.chars.end(), chars + c0, chars + c0 + nc);
  if (ix.has_ids) {
    ix.ids.insert(ix.ids.end(), ids, ids + n);
    const int64_t least = ids[batch.front() - n_old], most = ids[batch.back() - n_old];
    ix.order.insert(ix.order.end(), batch.begin(), batch.end());
    if (n_old > 0 && least < ix.max_id) {  // the new rows do not all sort behind the stored ones: merge, and lay everything again
      std::inplace_merge(ix.order.begin(), ix.order.begin() + n_old, ix.order.end(), [&](int64_t a, int64_t b) {
        return ix.ids[a] != ix.ids[b] ? ix.ids[a] < ix.ids[b] : a < b;
      });
      ix.dev_rows = 0;
    }
    ix.max_id = n_old > 0 ? std::max(ix.max_id, most) : most;
  }
}

// lays slots [dev_rows rounded down to a tile, n) on the device
int sync_device(edit_index &ix) {
  HTRY(hipSetDevice(ix.device));
  const int64_t n = ix.rows();
  if (ix.dev_rows == n) return EDIT_OK;
  const int64_t t0 = ix.dev_rows / TILE, nt = (n + TILE - 1) / TILE, s0 = t0 * TILE;
  ix.dev_rows = 0;  // (a failure below lays everything again next time)
  ix.tile_off.resize(t0 + 1);
  ix.tile_off.reserve(nt + 1);
  for (int64_t t = t0; t < nt; t++) {
    int64_t longest = 0;
    for (int64_t s = t * TILE; s < std::min(n, (t + 1) * TILE); s++) {
      const int64_t p = ix.position(s);
      longest = std::max(longest, ix.off[p + 1] - ix.off[p]);
    }
    ix.tile_off.push_back(ix.tile_off.back() + longest * TILE);
  }
  const int64_t e0 = ix.tile_off[t0], e1 = ix.tile_off[nt];
  std::vector<uint32_t> stage((size_t)(e1 - e0), 0u);
  std::vector<int32_t> lens((size_t)((nt - t0) * TILE), 0);
  std::vector<int64_t> idv((size_t)((nt - t0) * TILE), -1);
  for (int64_t s = s0; s < n; s++) {
    const int64_t p = ix.position(s), len = ix.off[p + 1] - ix.off[p];
    uint32_t *dst = stage.data() + (ix.tile_off[s / TILE] - e0) + (s % TILE);
    const float *src = ix.chars.data() + ix.off[p];
    for (int64_t j = 0; j < len; j++) dst[j * TILE] = bits_of(src[j]);
    lens[s - s0] = (int32_t)len;
    idv[s - s0] = ix.has_ids ? ix.ids[p] : p;
  }
  HTRY(grow(ix.d_tiles, (size_t)e0 * 4, (size_t)e1 * 4));
  HTRY(grow(ix.d_len, (size_t)s0 * 4, (size_t)nt * TILE * 4));
  HTRY(grow(ix.d_ids, (size_t)s0 * 8, (size_t)nt * TILE * 8));
  HTRY(ix.d_tile_off.reserve((size_t)(nt + 1) * 8));
  if (e1 > e0) HTRY(hipMemcpy(ix.d_tiles.as<uint32_t>() + e0, stage.data(), (size_t)(e1 - e0) * 4, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix.d_len.as<int32_t>() + s0, lens.data(), lens.size() * 4, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix.d_ids.as<int64_t>() + s0, idv.data(), idv.size() * 8, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix.d_tile_off.p, ix.tile_off.data(), (size_t)(nt + 1) * 8, hipMemcpyHostToDevice));
  ix.dev_rows = n;
  return EDIT_OK;
}

int check_append(const edit_index *ix, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars, const int64_t *ids) {
  if (int rc = check_csr("rows", n, offsets, chars, n_chars)) return rc;
  if (n > 0 && ix->has_ids && !ids) return fail(EDIT_EINVAL, "the index was built with ids: append needs ids");
  if (n > 0 && !ix->has_ids && ids) return fail(EDIT_EINVAL, "the index was built without ids (its ids are positions): append takes ids = NULL");
  if (ix->rows() + n >= MAX_ROWS) return fail(EDIT_ELIMIT, "an index holds fewer than 2^31 - 64 rows");
  return EDIT_OK;
}

}  // namespace

extern "C" {

int edit_index_build(int32_t device, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars, const int64_t *ids,
                     edit_index_t **out) try {
  if (!out) return fail(EDIT_EINVAL, "out is NULL");
  *out = nullptr;
  if (device < 0) return fail(EDIT_EINVAL, "negative device");
  std::unique_ptr<edit_index> ix(new edit_index);
  ix->device = device;
  ix->has_ids = ids != nullptr;
  if (int rc = check_append(ix.get(), n, offsets, chars, n_chars, ids)) return rc;
  append_rows(*ix, n, offsets, chars, ids);
  *out = ix.release();
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_index_append(edit_index_t *index, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars, const int64_t *ids) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (int rc = check_append(index, n, offsets, chars, n_chars, ids)) return rc;
  append_rows(*index, n, offsets, chars, ids);
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_index_reserve(edit_index_t *index, int64_t rows, int64_t total_chars) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (rows < 0 || total_chars < 0) return fail(EDIT_EINVAL, "negative capacity");
  if (rows >= MAX_ROWS) return fail(EDIT_ELIMIT, "an index holds fewer than 2^31 - 64 rows");
  index->off.reserve((size_t)rows + 1);
  index->chars.reserve((size_t)total_chars);
  if (index->has_ids) {
    index->ids.reserve((size_t)rows);
    index->order.reserve((size_t)rows);
  }
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_index_info(const edit_index_t *index, int64_t *n, int64_t *total_chars, int32_t *max_len) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (n) *n = index->rows();
  if (total_chars) *total_chars = index->off.back();
  if (max_len) *max_len = index->max_len;
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_index_get_rows(const edit_index_t *index, int64_t i0, int64_t n, int64_t *offsets, float *chars, int64_t cap_chars,
                        int64_t *n_chars, int64_t *ids) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (i0 < 0 || n < 0 || i0 > index->rows() || n > index->rows() - i0) return fail(EDIT_EINVAL, "rows out of range");
  const int64_t c0 = index->off[i0], nc = index->off[i0 + n] - c0;
  if (n_chars) *n_chars = nc;
  if (offsets)
    for (int64_t i = 0; i <= n; i++) offsets[i] = index->off[i0 + i] - c0;
  if (ids)
    for (int64_t i = 0; i < n; i++) ids[i] = index->has_ids ? index->ids[i0 + i] : i0 + i;
  if (!chars) return EDIT_OK;
  if (cap_chars < nc) return fail(EDIT_ESPACE, "chars holds " + std::to_string(cap_chars) + " elements, " + std::to_string(nc) + " are needed");
  if (nc) std::memcpy(chars, index->chars.data() + c0, (size_t)nc * 4);
  return EDIT_OK;
} EDIT_ABI_CATCH

void edit_index_destroy(edit_index_t *index) {
  if (!index) return;
  if (index->dev_rows || index->d_dist.p) (void)hipSetDevice(index->device);
  delete index;
}

int edit_index_set_query_slice(edit_index_t *index, int32_t max_queries_per_pass) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (max_queries_per_pass < 0) return fail(EDIT_EINVAL, "negative max_queries_per_pass");
  index->slice = std::min(max_queries_per_pass, (int32_t)MAX_SLICE);
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_last_timing(const edit_index_t *index, float *distance_ms, float *select_ms) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (distance_ms) *distance_ms = index->distance_ms;
  if (select_ms) *select_ms = index->select_ms;
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_last_stats(const edit_index_t *index, int64_t *pairs, int64_t *cell_updates) try {
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (pairs) *pairs = index->pairs;
  if (cell_updates) *cell_updates = index->cells;
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_search(edit_index_t *index, int64_t nq, const int64_t *q_offsets, const float *q_chars, int64_t n_q_chars, int32_t k,
                int32_t *out_dist, int64_t *out_ids, int32_t *out_counts) try {
  if (k < 1 || k > EDIT_MAX_K) return fail(EDIT_EINVAL, "k must be in 1.." + std::to_string(EDIT_MAX_K) + ", got " + std::to_string(k));
  if (!index) return fail(EDIT_EINVAL, "index is NULL");
  if (int rc = check_csr("queries", nq, q_offsets, q_chars, n_q_chars)) return rc;
  if (nq > 0 && (!out_dist || !out_ids || !out_counts)) return fail(EDIT_EINVAL, "an output array is NULL");
  edit_index &ix = *index;
  const int64_t n = ix.rows();
  ix.pairs = nq * n;
  ix.cells = nq > 0 ? (q_offsets[nq] - q_offsets[0]) * ix.off.back() : 0;
  ix.distance_ms = ix.select_ms = 0;
  if (nq == 0) return EDIT_OK;
  if (n == 0) {
    for (int64_t i = 0; i < nq * k; i++) {
      out_dist[i] = -1;
      out_ids[i] = -1;
    }
    for (int64_t q = 0; q < nq; q++) out_counts[q] = 0;
    return EDIT_OK;
  }
  if (int rc = sync_device(ix)) return rc;
  for (hipEvent_t &e : ix.ev)
    if (!e) HTRY(hipEventCreate(&e));
  const int64_t n_tiles = (n + TILE - 1) / TILE, n_pad = n_tiles * TILE;
  const int n_chunks = (int)((n + CHUNK - 1) / CHUNK);
  const int kq = (int)std::min<int64_t>(k, n);
  const int64_t automatic = std::max<int64_t>(1, std::min<int64_t>(MAX_SLICE, (int64_t)(SCRATCH_BUDGET / ((size_t)n_pad * 2))));
  const int64_t pass = std::min<int64_t>(nq, ix.slice > 0 ? ix.slice : automatic);
  HTRY(ix.d_dist.reserve((size_t)pass * n_pad * 2));
  HTRY(ix.d_hist.reserve((size_t)pass * BINS * 4));
  HTRY(ix.d_info.reserve((size_t)pass * sizeof(int4)));
  HTRY(ix.d_cnt.reserve((size_t)pass * n_chunks * 4 * 4));
  HTRY(ix.d_cand.reserve((size_t)pass * EDIT_MAX_K * 8));
  HTRY(ix.d_qoff.reserve((size_t)(pass + 1) * 4));
  HTRY(ix.d_out_dist.reserve((size_t)pass * k * 4));
  HTRY(ix.d_out_ids.reserve((size_t)pass * k * 8));
  uint32_t *cnt_lt = ix.d_cnt.as<uint32_t>(), *cnt_eq = cnt_lt + (size_t)pass * n_chunks, *pre_lt = cnt_eq + (size_t)pass * n_chunks,
           *pre_eq = pre_lt + (size_t)pass * n_chunks;
  std::vector<int32_t> qoff;
  for (int64_t q0 = 0; q0 < nq; q0 += pass) {
    const int qs = (int)std::min<int64_t>(pass, nq - q0);
    const int64_t c0 = q_offsets[q0], nc = q_offsets[q0 + qs] - c0;
    qoff.resize(qs + 1);
    for (int i = 0; i <= qs; i++) qoff[i] = (int32_t)(q_offsets[q0 + i] - c0);
    HTRY(ix.d_qchars.reserve((size_t)nc * 4));
    HTRY(hipMemcpy(ix.d_qoff.p, qoff.data(), (size_t)(qs + 1) * 4, hipMemcpyHostToDevice));
    if (nc) HTRY(hipMemcpy(ix.d_qchars.p, q_chars + c0, (size_t)nc * 4, hipMemcpyHostToDevice));
    HTRY(hipMemsetAsync(ix.d_hist.p, 0, (size_t)qs * BINS * 4, nullptr));
    HTRY(hipEventRecord(ix.ev[0], nullptr));
    edit_distance_kernel<<<dim3((unsigned)((n_tiles + TILES_PER_BLOCK - 1) / TILES_PER_BLOCK), (unsigned)((qs + QUERY_TILE - 1) / QUERY_TILE)), BLOCK, 0, nullptr>>>(
        ix.d_tiles.as<uint32_t>(), ix.d_tile_off.as<int64_t>(), ix.d_len.as<int32_t>(), n_tiles, ix.d_qchars.as<uint32_t>(), ix.d_qoff.as<int32_t>(), qs,
        ix.d_dist.as<uint16_t>());
    HTRY(hipGetLastError());
    HTRY(hipEventRecord(ix.ev[1], nullptr));
    const uint16_t *dist = ix.d_dist.as<uint16_t>();
    const int4 *info = ix.d_info.as<int4>();
    edit_hist_kernel<<<dim3((unsigned)((n + CHUNK * HIST_CHUNKS - 1) / (CHUNK * HIST_CHUNKS)), (unsigned)qs), BLOCK, 0, nullptr>>>(dist, n_pad, n, ix.d_hist.as<uint32_t>());
    HTRY(hipGetLastError());
    edit_threshold_kernel<<<(qs + 63) / 64, 64, 0, nullptr>>>(ix.d_hist.as<uint32_t>(), qs, (uint32_t)kq, ix.d_info.as<int4>());
    HTRY(hipGetLastError());
    edit_count_kernel<<<dim3((unsigned)n_chunks, (unsigned)qs), BLOCK, 0, nullptr>>>(dist, n_pad, n, info, n_chunks, cnt_lt, cnt_eq);
    HTRY(hipGetLastError());
    edit_scan_kernel<<<qs, BLOCK, 0, nullptr>>>(cnt_lt, cnt_eq, n_chunks, pre_lt, pre_eq);
    HTRY(hipGetLastError());
    edit_emit_kernel<<<dim3((unsigned)n_chunks, (unsigned)qs), BLOCK, 0, nullptr>>>(dist, n_pad, n, info, n_chunks, cnt_lt, cnt_eq, pre_lt, pre_eq, ix.d_cand.as<uint64_t>());
    HTRY(hipGetLastError());
    edit_sort_kernel<<<qs, BLOCK, 0, nullptr>>>(ix.d_cand.as<uint64_t>(), ix.d_ids.as<int64_t>(), n, kq, k, ix.d_out_dist.as<int32_t>(), ix.d_out_ids.as<int64_t>());
    HTRY(hipGetLastError());
    HTRY(hipEventRecord(ix.ev[2], nullptr));
    HTRY(hipMemcpy(out_dist + q0 * k, ix.d_out_dist.p, (size_t)qs * k * 4, hipMemcpyDeviceToHost));
    HTRY(hipMemcpy(out_ids + q0 * k, ix.d_out_ids.p, (size_t)qs * k * 8, hipMemcpyDeviceToHost));
    float a = 0, b = 0;
    HTRY(hipEventElapsedTime(&a, ix.ev[0], ix.ev[1]));
    HTRY(hipEventElapsedTime(&b, ix.ev[1], ix.ev[2]));
    ix.distance_ms += a;
    ix.select_ms += b;
    for (int i = 0; i < qs; i++) out_counts[q0 + i] = kq;
  }
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_pair_distances(int32_t device, int64_t n_pairs, const int64_t *a_offsets, const float *a_chars, int64_t n_a_chars,
                        const int64_t *b_offsets, const float *b_chars, int64_t n_b_chars, int32_t *out) try {
  if (device < 0) return fail(EDIT_EINVAL, "negative device");
  if (int rc = check_csr("a", n_pairs, a_offsets, a_chars, n_a_chars)) return rc;
  if (int rc = check_csr("b", n_pairs, b_offsets, b_chars, n_b_chars)) return rc;
  if (n_pairs > 0 && !out) return fail(EDIT_EINVAL, "out is NULL");
  if (n_pairs == 0) return EDIT_OK;
  HTRY(hipSetDevice(device));
  Buf d_off[2], d_chars[2], d_out;
  const int64_t *offs[2] = {a_offsets, b_offsets};
  const float *chs[2] = {a_chars, b_chars};
  std::vector<int64_t> rebased((size_t)n_pairs + 1);
  for (int s = 0; s < 2; s++) {
    const int64_t c0 = offs[s][0], nc = offs[s][n_pairs] - c0;
    for (int64_t i = 0; i <= n_pairs; i++) rebased[i] = offs[s][i] - c0;
    HTRY(d_off[s].reserve(rebased.size() * 8));
    HTRY(d_chars[s].reserve((size_t)nc * 4));
    HTRY(hipMemcpy(d_off[s].p, rebased.data(), rebased.size() * 8, hipMemcpyHostToDevice));
    if (nc) HTRY(hipMemcpy(d_chars[s].p, chs[s] + c0, (size_t)nc * 4, hipMemcpyHostToDevice));
  }
  HTRY(d_out.reserve((size_t)n_pairs * 4));
  for (int64_t p0 = 0; p0 < n_pairs; p0 += PAIRS_PER_LAUNCH) {
    edit_pairs_kernel<<<(unsigned)std::min(PAIRS_PER_LAUNCH, n_pairs - p0), TILE, 0, nullptr>>>(d_chars[0].as<uint32_t>(), d_off[0].as<int64_t>(), d_chars[1].as<uint32_t>(),
                                                                                               d_off[1].as<int64_t>(), p0, n_pairs, d_out.as<int32_t>());
    HTRY(hipGetLastError());
  }
  HTRY(hipMemcpy(out, d_out.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost));
  return EDIT_OK;
} EDIT_ABI_CATCH

}  // extern "C"
