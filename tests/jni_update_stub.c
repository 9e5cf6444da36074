/* Stand-ins for hnsw_index_info / hnsw_index_update, linked (with -Bsymbolic) into a JNI harness of its own by
 * tests/test_hnsw_update_cpu.py, so the glue's checks of AnnJni.hnswIndexUpdate run without a device: the "index" reports
 * dimension 32 and records what reaches the library. */
#include <stdint.h>

#include "../include/hnsw_ann.h"

static int64_t g_calls, g_n;
static int32_t g_efc;

int hnsw_index_info(const hnsw_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *max_m) {
  (void)index;
  if (n) *n = 100;
  if (d) *d = 32;
  if (metric) *metric = 0;
  if (max_m) *max_m = 8;
  return HNSW_OK;
}
int hnsw_index_update(hnsw_index_t *index, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction,
                      uint64_t seed, int32_t batch, int64_t *out_appended) {
  (void)index; (void)vectors; (void)ids; (void)seed; (void)batch;
  g_calls++;
  g_n = n;
  g_efc = ef_construction;
  if (out_appended) *out_appended = 0;
  return HNSW_OK;
}
int64_t stub_update_calls(void) { return g_calls; }
int64_t stub_update_n(void) { return g_n; }
int32_t stub_update_efc(void) { return g_efc; }
