// faiss_by_id.hip -- the by-id queries of include/faiss_by_id.h on the inverted-file family and on shard sets.
//
// A by-id query is the plain search with another first half and another last step:
//   1 resolve   by_id_core.h: the seed ids are uploaded, looked up in the store's (key, position) table, and a scan of the
//               found flags gives every found seed its compact query slot
//   2 compact   by_id_compact_kernel: the store positions of the found seeds in request order, one int64 per query
//   3 search    the index's own search over (store rows, positions) (ivf_device_rows.h: search_store_out): its query
//               preparation reads row pos[i] of the store where the plain one reads row i of its queries
//               (ivf_kernels.h: store_rows_pos_kernel; opq_ann.hip: opq_transform_kernel<true>; shard_set.hip: one fp32 row
//               copy into the set's query buffer), everything after that is the plain search, answers left on the device
//   4 flatten   by_id_core.h: the counts may differ from seed to seed (short lists); the triples are packed
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>

#include "../../include/faiss_by_id.h"
#include "ann_by_id_internal.h"  // StoreView
#include "by_id_core.h"          // resolve, flatten, the scratch; Buf, g_err, fail, BTRY
#include "ivf_device_rows.h"
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, ANN_BY_ID_ENOMEM, ANN_BY_ID_EINTERNAL); }

namespace {

constexpr int MAX_K = 1024;
constexpr int MAX_NPROBE = 1024;

// qpos[slot of seed i] = pos[i] for every found seed: the queries of the search, in request order
__global__ void by_id_compact_kernel(const int64_t *__restrict__ pos, const int32_t *__restrict__ flag, const int32_t *__restrict__ slot,
                                     int64_t n, int64_t *__restrict__ qpos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  qpos[slot[i]] = pos[i];  // (slot[i] < n_found: the exclusive scan of the flags)
}

// the refusals that need nothing of the index
int check_args(const void *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k, int32_t nprobe,
               int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total, int32_t *out_counts) {
  if (k < 1 || k > MAX_K) return fail(ANN_BY_ID_EINVAL, "k must be in 1..1024");
  if (nprobe < 1 || nprobe > MAX_NPROBE) return fail(ANN_BY_ID_EINVAL, "nprobe must be in 1..1024");
  if (int rc = check_common(index, n_seeds, seeds, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  if (!store)
    return fail(ANN_BY_ID_EINVAL, "store must not be NULL: an inverted-file index keeps no fp32 rows of its own to be its own producer");
  return ANN_BY_ID_OK;
}

// What a call needs of its index or set.  search(nq, rows, pos, dist, ids, counts): search_store_out of the kind; message():
// the owning module's last error; ctl() / ctl_up(): the control bytes of the last search and the part of them that went up.
template <class Search, class Message, class Ctl, class CtlUp>
int query_by_id(const void *index, int device, int d, const char *d_name, std::shared_ptr<void> &slot, const ann_store_t *store,
                int32_t n_seeds, const int64_t *seeds, int32_t k, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                int64_t *out_total, int32_t *out_counts, Search search, Message message, Ctl ctl, CtlUp ctl_up) {
  ann_by_id::StoreView sv;
  (void)ann_by_id::store_view(store, &sv);
  if (sv.d != d)
    return fail(ANN_BY_ID_EINVAL, "the store holds rows of dimension " + std::to_string(sv.d) + ", the index takes " + d_name + " = " + std::to_string(d));
  if (sv.device != device)
    return fail(ANN_BY_ID_EINVAL, "the store is on device " + std::to_string(sv.device) + ", the index on " + std::to_string(device));
  (void)index;
  *out_total = 0;
  BTRY(hipSetDevice(device));
  Scratch *s = nullptr;
  if (int rc = get_scratch(slot, &s)) return rc;
  if (n_seeds == 0) {
    s->found = s->absent = s->h2d = s->d2h = s->d2h_result = 0;
    s->t_gather = s->t_search = s->t_flatten = 0;
    return ANN_BY_ID_OK;
  }
  KeyTable t;
  t.keys = sv.keys;
  t.kpos = sv.kpos;
  t.nt = sv.n;
  if (int rc = resolve(s, t, n_seeds, seeds)) return rc;
  if (int rc = cap_check(s, k, cap)) return rc;
  hipStream_t st = 0;
  const int32_t nq = (int32_t)s->found;
  if (nq > 0) {
    BTRY(s->qpos.reserve((size_t)nq * 8));
    BTRY(s->r_dist.reserve((size_t)nq * k * 4));
    BTRY(s->r_ids.reserve((size_t)nq * k * 8));
    BTRY(s->r_cnt.reserve((size_t)nq * 4));
    hipLaunchKernelGGL(by_id_compact_kernel, dim3((unsigned)((n_seeds + 255) / 256)), dim3(256), 0, st, s->pos.as<int64_t>(),
                       s->flag.as<int32_t>(), s->slot.as<int32_t>(), (int64_t)n_seeds, s->qpos.as<int64_t>());
    BTRY(hipGetLastError());
  }
  BTRY(hipEventRecord(s->ev[1], st));
  if (nq > 0) {
    if (int rc = search(nq, sv.rows, s->qpos.as<int64_t>(), s->r_dist.as<float>(), s->r_ids.as<int64_t>(), s->r_cnt.as<int32_t>()))
      return fail(rc, message());
    const int64_t all = ctl(), up = ctl_up();
    s->h2d += up;
    s->d2h += all - up;
  }
  if (int rc = flatten(s, n_seeds, k, s->r_dist.as<float>(), s->r_ids.as<int64_t>(), nq > 0 ? s->r_cnt.as<int32_t>() : nullptr, out_seed,
                       out_id, out_dist, out_total, out_counts))
    return rc;
  (void)hipEventElapsedTime(&s->t_gather, s->ev[0], s->ev[1]);
  if (nq > 0) (void)hipEventElapsedTime(&s->t_search, s->ev[1], s->ev[2]);
  return ANN_BY_ID_OK;
}

}  // namespace

extern "C" {

const char *ivf_by_id_last_error(void) { return g_err.c_str(); }

int ivf_batch_query_by_id(ivf_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                          int32_t nprobe, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                          int32_t *out_counts) try {
  if (int rc = check_args(index, store, n_seeds, seeds, k, nprobe, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  int32_t d = 0;
  if (int rc = ivf_index_info(index, nullptr, &d, nullptr, nullptr)) return fail(rc, ivf_last_error());
  return query_by_id(
      index, ivf_internal::device_of(index), d, "d", ivf_internal::by_id_scratch(index), store, n_seeds, seeds, k, out_seed, out_id,
      out_dist, cap, out_total, out_counts,
      [&](int32_t nq, const float *rows, const int64_t *pos, float *dd, int64_t *di, int32_t *dc) {
        return ivf_internal::search_store_out(index, nq, rows, pos, k, nprobe, dd, di, dc);
      },
      [] { return ivf_last_error(); }, [&] { return ivf_internal::last_control_bytes(index); },
      [&] { return ivf_internal::last_control_upload_bytes(index); });
} ABI_CATCH

int ivfsq_batch_query_by_id(ivfsq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                            int32_t nprobe, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                            int32_t *out_counts) try {
  if (int rc = check_args(index, store, n_seeds, seeds, k, nprobe, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  int32_t d = 0;
  if (int rc = ivfsq_index_info(index, nullptr, &d, nullptr, nullptr)) return fail(rc, ivfsq_last_error());
  return query_by_id(
      index, ivfsq_internal::device_of(index), d, "d", ivfsq_internal::by_id_scratch(index), store, n_seeds, seeds, k, out_seed, out_id,
      out_dist, cap, out_total, out_counts,
      [&](int32_t nq, const float *rows, const int64_t *pos, float *dd, int64_t *di, int32_t *dc) {
        return ivfsq_internal::search_store_out(index, nq, rows, pos, k, nprobe, dd, di, dc);
      },
      [] { return ivfsq_last_error(); }, [&] { return ivfsq_internal::last_control_bytes(index); },
      [&] { return ivfsq_internal::last_control_upload_bytes(index); });
} ABI_CATCH

int ivfpq_batch_query_by_id(ivfpq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                            int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                            int64_t *out_total, int32_t *out_counts) try {
  if (int rc = check_args(index, store, n_seeds, seeds, k, nprobe, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  int32_t d = 0;
  if (int rc = ivfpq_index_info(index, nullptr, &d, nullptr, nullptr, nullptr)) return fail(rc, ivfpq_last_error());
  return query_by_id(
      index, ivfpq_internal::device_of(index), d, "d", ivfpq_internal::by_id_scratch(index), store, n_seeds, seeds, k, out_seed, out_id,
      out_dist, cap, out_total, out_counts,
      [&](int32_t nq, const float *rows, const int64_t *pos, float *dd, int64_t *di, int32_t *dc) {
        return ivfpq_internal::search_store_out(index, nq, rows, pos, k, nprobe, ht, dd, di, dc);
      },
      [] { return ivfpq_last_error(); }, [&] { return ivfpq_internal::last_control_bytes(index); },
      [&] { return ivfpq_internal::last_control_upload_bytes(index); });
} ABI_CATCH

int opq_batch_query_by_id(opq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                          int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                          int64_t *out_total, int32_t *out_counts) try {
  if (int rc = check_args(index, store, n_seeds, seeds, k, nprobe, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  int32_t d_in = 0;
  if (int rc = opq_index_info(index, nullptr, &d_in, nullptr, nullptr, nullptr, nullptr)) return fail(rc, opq_last_error());
  return query_by_id(
      index, opq_internal::device_of(index), d_in, "d_in", opq_internal::by_id_scratch(index), store, n_seeds, seeds, k, out_seed,
      out_id, out_dist, cap, out_total, out_counts,
      [&](int32_t nq, const float *rows, const int64_t *pos, float *dd, int64_t *di, int32_t *dc) {
        return opq_internal::search_store_out(index, nq, rows, pos, k, nprobe, ht, dd, di, dc);
      },
      [] { return opq_last_error(); }, [&] { return opq_internal::last_control_bytes(index); },
      [&] { return opq_internal::last_control_upload_bytes(index); });
} ABI_CATCH

int shard_set_batch_query_by_id(shardset_t *set, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                               int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                               int64_t *out_total, int32_t *out_counts) try {
  if (int rc = check_args(set, store, n_seeds, seeds, k, nprobe, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  if (int rc = shardset_internal::check_ht(set, ht)) return fail(rc, shardset_last_error());
  return query_by_id(
      set, shardset_internal::device_of(set), shardset_internal::dimension_of(set), "dimension", shardset_internal::by_id_scratch(set),
      store, n_seeds, seeds, k, out_seed, out_id, out_dist, cap, out_total, out_counts,
      [&](int32_t nq, const float *rows, const int64_t *pos, float *dd, int64_t *di, int32_t *dc) {
        return shardset_internal::search_store_out(set, nq, rows, pos, k, nprobe, ht, dd, di, dc);
      },
      [] { return shardset_last_error(); }, [&] { return shardset_internal::last_control_bytes(set); },
      [&] { return shardset_internal::last_control_upload_bytes(set); });
} ABI_CATCH

int ivf_by_id_last_stats(int32_t kind_or_set, const void *handle, int64_t *found, int64_t *absent, int64_t *h2d_bytes,
                           int64_t *d2h_bytes, int64_t *d2h_result_bytes, float *resolve_gather_ms, float *search_ms,
                           float *flatten_ms) try {
  if (!handle) return fail(ANN_BY_ID_EINVAL, "NULL handle");
  void *h = const_cast<void *>(handle);
  const std::shared_ptr<void> *slot = nullptr;
  switch (kind_or_set) {
    case FAISS_BY_ID_IVF_FLAT: slot = &ivf_internal::by_id_scratch((ivf_index_t *)h); break;
    case FAISS_BY_ID_IVF_PQ: slot = &ivfpq_internal::by_id_scratch((ivfpq_index_t *)h); break;
    case FAISS_BY_ID_OPQ_IVF_PQ: slot = &opq_internal::by_id_scratch((opq_index_t *)h); break;
    case FAISS_BY_ID_IVF_SQ8: slot = &ivfsq_internal::by_id_scratch((ivfsq_index_t *)h); break;
    case FAISS_BY_ID_SHARD_SET: slot = &shardset_internal::by_id_scratch((shardset_t *)h); break;
    default: return fail(ANN_BY_ID_EINVAL, "kind_or_set must be one of FAISS_BY_ID_*, got " + std::to_string(kind_or_set));
  }
  static const Scratch none;
  const Scratch *s = *slot ? static_cast<const Scratch *>(slot->get()) : &none;
  if (found) *found = s->found;
  if (absent) *absent = s->absent;
  if (h2d_bytes) *h2d_bytes = s->h2d;
  if (d2h_bytes) *d2h_bytes = s->d2h;
  if (d2h_result_bytes) *d2h_result_bytes = s->d2h_result;
  if (resolve_gather_ms) *resolve_gather_ms = s->t_gather;
  if (search_ms) *search_ms = s->t_search;
  if (flatten_ms) *flatten_ms = s->t_flatten;
  return ANN_BY_ID_OK;
} ABI_CATCH

}  // extern "C"
