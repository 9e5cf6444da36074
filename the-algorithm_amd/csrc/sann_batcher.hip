// sann_batcher.hip -- the native micro-batching queue in front of the batched operator (host code only).
//
// The reference calls ApproximateCosineSimilarity.apply once per request, from Finagle worker threads, inside a Future.map
// (simclusters-ann/server/src/main/scala/com/twitter/simclustersann/candidate_source/SimClustersANNCandidateSource.scala:77-94)
// with a 40 ms budget (modules/FlagsModule.scala:8-12).  One request is 32 units of work for a 256-CU GPU (0.16 ms of
// latency, 6 k requests/s per caller thread); the GPU wants ~1000 requests per launch.  This queue folds concurrent
// single-request calls into batches:
//
//   sann_submit           copies the request (embedding, config, source tweet, Time.now) into the OPEN batch and returns a ticket
//   a batch closes        when it holds max_batch requests, or max_wait_us after its first request arrived
//   dispatcher threads    (n_dispatchers, each with a pooled batch object and HIP stream of its own) take closed batches and
//                         run them through the same call a batched caller makes (sann_get_tweet_candidates_at: every
//                         request keeps ITS OWN now_ms, so the age window of ApproximateCosineSimilarity.scala:65-72 is the
//                         one the request would have seen alone), then hand every request its rows
//   sann_wait / sann_poll the caller collects its answer (sann_batcher_get_tweet_candidates = submit + wait)
//
// Results are bit for bit those of the request run alone (tests/test_batcher_gpu.py).  Requests use the default cluster
// selection of fetchCandidates (truncate(maxScanClusters), SimClustersANNCandidateSource.scala:72-75); explicit scan keys
// stay with the batch API.
//
// The queue itself -- batches, tickets, deadlines, dispatcher threads, shutdown -- is host code with no GPU call in it and lives
// in request_queue.h; this file is what a dispatcher does on the GPU (run_batch) and the entry points.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/simclusters_ann.h"
#include "sann_host.h"
#include "abi_guard.h"
#include "request_queue.h"

using sann_host::fail;
#define ABI_CATCH catch (...) { return abi_guard::caught(sann_host::fail, SANN_ENOMEM, SANN_EINTERNAL); }

namespace {

using request_queue::Batch;
using request_queue::Request;

// pinned response buffers of one dispatcher, grown on demand
struct OutBuf {
  void *p = nullptr;
  size_t cap = 0;
  ~OutBuf() { if (p) (void)hipHostFree(p); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipHostMalloc(&p, n + n / 4, hipHostMallocDefault);
    if (e == hipSuccess) cap = n + n / 4;
    return e;
  }
};

int status_of(const request_queue::Status &s) { return s.code == SANN_OK ? SANN_OK : fail(s.code, s.message); }

}  // namespace

struct sann_batcher {
  sann_index *ix = nullptr;
  int32_t variant = 0;
  std::vector<OutBuf> out;  // one per dispatcher
  std::unique_ptr<request_queue::Queue> queue;  // (last: its dispatchers, which use the members above, end first)

  // what a dispatcher does on the GPU: the closed batch through the batched call, then every request its status and rows
  void run_batch(Batch &bt, OutBuf &ob) {
    const int nq = (int)bt.reqs.size();
    const int stride = bt.kmax;
    int rc = SANN_OK;
    std::string msg;
    int64_t *ids = nullptr;
    double *sc = nullptr;
    int32_t *cnt = nullptr, *msz = nullptr;
    const size_t row = (size_t)stride * 8, need = 2 * row * (size_t)nq + 8 * (size_t)nq;
    if (hipSetDevice(ix->device) != hipSuccess || ob.reserve(need) != hipSuccess) {
      rc = SANN_EDEVICE;
      msg = "micro-batcher: pinned response buffer";
    } else {
      ids = (int64_t *)ob.p;
      sc = (double *)((char *)ob.p + row * (size_t)nq);
      cnt = (int32_t *)((char *)ob.p + 2 * row * (size_t)nq);
      msz = cnt + nq;
      rc = sann_candidates_pooled(ix, variant, bt.now[0], bt.now.data(), nq, bt.emb_offsets.data(), bt.emb.cids.get(),
                                  bt.emb.scores.get(), bt.src.data(), bt.has_src.data(), bt.cfgs.data(), nq, nullptr, nullptr, ids, sc,
                                  stride, cnt, msz);
      if (rc != SANN_OK) msg = sann_last_error();
    }
    // hand every request its rows (its own thread may be anywhere: the copy is ours)
    for (int q = 0; q < nq; q++) {
      Request &r = *bt.reqs[(size_t)q];
      int st = rc;
      if (rc == SANN_OK) {
        const int c = cnt[q];
        if (c > r.out_cap) {
          st = SANN_EINVAL;
          r.message = "out_capacity smaller than the number of results";
        } else {
          if (c > 0) {
            memcpy(r.out_ids, ids + (size_t)q * stride, (size_t)c * 8);
            memcpy(r.out_scores, sc + (size_t)q * stride, (size_t)c * 8);
          }
          if (r.out_count) *r.out_count = c;
          if (r.out_map_size) *r.out_map_size = msz[q];
        }
      } else {
        r.message = msg;
      }
      r.status = st;
    }
  }
};

extern "C" {

int sann_batcher_create(sann_index_t *index, const sann_batcher_options_t *options, sann_batcher_t **out) try {
  if (!out) return fail(SANN_EINVAL, "out is NULL");
  *out = nullptr;
  if (!index) return fail(SANN_EINVAL, "index is NULL");
  sann_batcher_options_t o{};
  if (options) o = *options;
  if (o.variant < 0 || o.variant > 3) return fail(SANN_EINVAL, "unknown variant");
  if (o.max_batch == 0) o.max_batch = 1024;
  if (o.max_wait_us == 0) o.max_wait_us = 500;
  if (o.n_dispatchers == 0) o.n_dispatchers = 3;
  if (o.max_batch < 1 || o.max_batch > 65536 || o.max_wait_us < 0 || o.n_dispatchers < 1 || o.n_dispatchers > 16)
    return fail(SANN_EINVAL, "max_batch in 1..65536, max_wait_us >= 0, n_dispatchers in 1..16");
  std::unique_ptr<sann_batcher> b(new sann_batcher());
  b->ix = index;
  b->variant = o.variant;
  b->out = std::vector<OutBuf>((size_t)o.n_dispatchers);
  request_queue::Queue::Options qo;
  qo.variant = o.variant;
  qo.max_batch = o.max_batch;
  qo.max_wait_us = o.max_wait_us;
  qo.n_dispatchers = o.n_dispatchers;
  b->queue.reset(new request_queue::Queue(qo, [p = b.get()](int d, Batch &bt) { p->run_batch(bt, p->out[(size_t)d]); }));
  *out = b.release();
  return SANN_OK;
} ABI_CATCH

int sann_submit(sann_batcher_t *b, int64_t now_ms, int32_t n_embedding, const int32_t *cluster_ids, const double *scores,
                int64_t source_tweet_id, int32_t has_source_tweet, const sann_config_t *config, int32_t out_capacity,
                int64_t *out_ids, double *out_scores, int32_t *out_count, int32_t *out_map_size, int64_t *ticket) try {
  if (!b) return fail(SANN_EINVAL, "NULL argument");
  return status_of(b->queue->submit(now_ms, n_embedding, cluster_ids, scores, source_tweet_id, has_source_tweet, config, out_capacity,
                                    out_ids, out_scores, out_count, out_map_size, ticket));
} ABI_CATCH

int sann_wait(sann_batcher_t *b, int64_t ticket) try {
  if (!b) return fail(SANN_EINVAL, "batcher is NULL");
  return status_of(b->queue->collect(ticket, true, nullptr));
} ABI_CATCH

int sann_poll(sann_batcher_t *b, int64_t ticket, int32_t *done) try {
  if (!b || !done) return fail(SANN_EINVAL, "NULL argument");
  return status_of(b->queue->collect(ticket, false, done));
} ABI_CATCH

int sann_batcher_get_tweet_candidates(sann_batcher_t *b, int64_t now_ms, int32_t n_embedding, const int32_t *cluster_ids,
                                      const double *scores, int64_t source_tweet_id, int32_t has_source_tweet,
                                      const sann_config_t *config, int32_t out_capacity, int64_t *out_ids, double *out_scores,
                                      int32_t *out_count, int32_t *out_map_size) try {
  int64_t t = 0;
  int rc = sann_submit(b, now_ms, n_embedding, cluster_ids, scores, source_tweet_id, has_source_tweet, config, out_capacity, out_ids,
                       out_scores, out_count, out_map_size, &t);
  if (rc != SANN_OK) return rc;
  return status_of(b->queue->collect(t, true, nullptr));
} ABI_CATCH

int sann_batcher_stats(sann_batcher_t *b, sann_batcher_stats_t *stats) try {
  if (!b || !stats) return fail(SANN_EINVAL, "NULL argument");
  *stats = b->queue->stats();
  return SANN_OK;
} ABI_CATCH

int sann_batcher_destroy(sann_batcher_t *b) try {
  if (!b) return SANN_OK;
  // requests submitted before the stop are run, and a caller blocked in sann_wait gets its answer and leaves, before the
  // object goes; tickets nobody collected are dropped with it
  b->queue->shutdown();
  delete b;
  return SANN_OK;
} ABI_CATCH

}  // extern "C"
