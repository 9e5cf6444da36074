/*
 * ann_jni.c -- JNI glue between a JVM shim (class com.twitter.ann.gpu.AnnJni, sketched in INTEGRATION.md section 6) and the C ABIs
 * of include/dense_ann.h (exhaustive search: BruteForceIndex.scala:66-91) and include/hnsw_ann.h (HnswIndex.searchKnn:
 * HnswIndex.java:538-623), plus the index directory loader of include/ann_codec.h (SerializableHnsw.scala:170-190).
 *
 * The search entries have the shape of the reference's own JNI call, faiss `Index_search(ptr, n, x*, k, distances*, labels*)`
 * (ann/src/main/java/com/twitter/ann/faiss/swig/swigfaissJNI.java:269; Index.java:99-101), batched over n queries as faiss is;
 * a Scala adapter in the mould of QueryableIndexAdapter (ann/src/main/scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:
 * 139-195) turns rows back into NeighborWithDistance.  Buffers are direct ByteBuffers owned by the caller (little-endian): the
 * lifetime hazard QueryableIndexAdapter.scala:128-132 documents -- the JVM freeing `distances` during the call -- cannot occur.
 * All capacities are checked here, before the library writes.
 */
#ifdef SANN_JNI_MINIMAL
#include "jni_min.h"
#else
#include <jni.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/ann_by_id.h"
#include "../../include/ann_codec.h"
#include "../../include/dense_ann.h"
#include "../../include/hnsw_ann.h"

static void throw_runtime(JNIEnv *env, const char *msg) {
  jclass cls = (*env)->FindClass(env, "java/lang/RuntimeException");
  if (cls) (*env)->ThrowNew(env, cls, msg ? msg : "ann: native failure");
}
#define BUF(x) ((x) ? (*env)->GetDirectBufferAddress(env, (x)) : NULL)
#define CAP(x) ((x) ? (*env)->GetDirectBufferCapacity(env, (x)) : 0)

/* ---- exhaustive search ------------------------------------------------------------------------------------------------ */
/* long denseIndexBuild(int device, int metric, long n, int d, ByteBuffer vectors /+ float[n][d] +/, ByteBuffer ids /+ long[n] or null +/, boolean exact) */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_denseIndexBuild(JNIEnv *env, jclass cls, jint device, jint metric, jlong n, jint d,
                                                                        jobject vectors, jobject ids, jboolean exact) {
  (void)cls;
  if (n < 1 || d < 1 || !vectors || CAP(vectors) / 4 / d < n || (ids && CAP(ids) / 8 < n)) {
    throw_runtime(env, "vectors must hold n x d floats (and ids n longs)");
    return 0;
  }
  dann_index_t *ix = NULL;
  const int rc = exact ? dann_index_build_exact(device, metric, n, d, (const float *)BUF(vectors), (const int64_t *)BUF(ids), &ix)
                       : dann_index_build(device, metric, n, d, (const float *)BUF(vectors), (const int64_t *)BUF(ids), &ix);
  if (rc != DANN_OK) {
    throw_runtime(env, dann_last_error());
    return 0;
  }
  return (jlong)(intptr_t)ix;
}
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_denseIndexDestroy(JNIEnv *env, jclass cls, jlong index) {
  (void)env;
  (void)cls;
  dann_index_destroy((dann_index_t *)(intptr_t)index);
}
/* void denseIndexAppend(long index, long n, int d, ByteBuffer vectors /+ float[n][d] +/, ByteBuffer ids /+ long[n] or null +/)
 * BruteForceIndex.append for n rows (dann_index_append); one writer at a time per index */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_denseIndexAppend(JNIEnv *env, jclass cls, jlong index, jlong n, jint d, jobject vectors,
                                                                        jobject ids) {
  (void)cls;
  if (n < 0 || d < 1 || (n > 0 && (!vectors || CAP(vectors) / 4 / d < n)) || (ids && CAP(ids) / 8 < n)) {
    throw_runtime(env, "vectors must hold n x d floats (and ids n longs)");
    return;
  }
  if (!index) {
    throw_runtime(env, "null index");
    return;
  }
  int32_t dim = 0;
  if (dann_index_info((const dann_index_t *)(intptr_t)index, NULL, &dim, NULL) != DANN_OK || dim != d) {
    throw_runtime(env, "d is not the index's dimension");
    return;
  }
  if (dann_index_append((dann_index_t *)(intptr_t)index, n, (const float *)BUF(vectors), (const int64_t *)BUF(ids)) != DANN_OK)
    throw_runtime(env, dann_last_error());
}
/* void denseSearch(long index, int nq, int d, ByteBuffer x /+ float[nq][d] +/, int k, ByteBuffer distances /+ float[nq][k] +/,
 *                  ByteBuffer labels /+ long[nq][k] +/, ByteBuffer counts /+ int[nq] +/) */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_denseSearch(JNIEnv *env, jclass cls, jlong index, jint nq, jint d, jobject x, jint k,
                                                                   jobject distances, jobject labels, jobject counts) {
  (void)cls;
  if (!index || nq < 1 || d < 1 || k < 1 || !x || !distances || !labels || !counts) {
    throw_runtime(env, "index, nq >= 1, k >= 1 and four direct buffers");
    return;
  }
  if (CAP(x) / 4 / d < nq || CAP(distances) / 4 / k < nq || CAP(labels) / 8 / k < nq || CAP(counts) / 4 < nq) {
    throw_runtime(env, "a direct buffer is smaller than nq x k (nq x d) entries");
    return;
  }
  if (dann_search((dann_index_t *)(intptr_t)index, nq, (const float *)BUF(x), k, (float *)BUF(distances), (int64_t *)BUF(labels),
                  (int32_t *)BUF(counts)) != DANN_OK)
    throw_runtime(env, dann_last_error());
}

/* ---- HNSW --------------------------------------------------------------------------------------------------------------- */
/* long hnswIndexBuildInsert(int device, int metric, long n, int d, ByteBuffer vectors, ByteBuffer ids, int maxM, int efConstruction,
 *                           long seed, int nThreads)   HnswIndex.insert for every row (TypedHnswIndex.index / Hnsw.append);
 * nThreads >= 1: on that many host threads (1 = the sequential reference graph); nThreads == 0: on the device, deterministic
 * (hnsw_index_build_insert_gpu: 1M x 256 in 3.7 s, 50M in 149 s) */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswIndexBuildInsert(JNIEnv *env, jclass cls, jint device, jint metric, jlong n, jint d,
                                                                             jobject vectors, jobject ids, jint maxM, jint efConstruction,
                                                                             jlong seed, jint nThreads) {
  (void)cls;
  if (n < 0 || d < 1 || (n > 0 && (!vectors || CAP(vectors) / 4 / d < n)) || (ids && CAP(ids) / 8 < n)) {
    throw_runtime(env, "vectors must hold n x d floats (and ids n longs)");
    return 0;
  }
  hnsw_index_t *ix = NULL;
  const int rc = nThreads == 0 ? hnsw_index_build_insert_gpu(device, metric, n, d, (const float *)BUF(vectors), (const int64_t *)BUF(ids), maxM,
                                                           efConstruction, (uint64_t)seed, 0, &ix)
                               : hnsw_index_build_insert(device, metric, n, d, (const float *)BUF(vectors), (const int64_t *)BUF(ids), maxM,
                                                         efConstruction, (uint64_t)seed, nThreads, &ix);
  if (rc != HNSW_OK) {
    throw_runtime(env, hnsw_last_error());
    return 0;
  }
  return (jlong)(intptr_t)ix;
}
/* long hnswIndexLoadDirectory(int device, int metric, long n, int d, ByteBuffer vectors, ByteBuffer ids, String directory)
 * the files a reference index directory holds (hnsw_index_metadata, hnsw_internal_index/...), the vectors as a flat array */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswIndexLoadDirectory(JNIEnv *env, jclass cls, jint device, jint metric, jlong n,
                                                                               jint d, jobject vectors, jobject ids, jstring directory) {
  (void)cls;
  if (n < 0 || d < 1 || !directory || (n > 0 && (!vectors || CAP(vectors) / 4 / d < n)) || (ids && CAP(ids) / 8 < n)) {
    throw_runtime(env, "vectors must hold n x d floats (and ids n longs); directory must not be null");
    return 0;
  }
  const char *dir = (*env)->GetStringUTFChars(env, directory, NULL);
  if (!dir) return 0; /* OutOfMemoryError is pending */
  hnsw_index_t *ix = NULL;
  const int rc = hnsw_index_load_directory(device, metric, n, d, (const float *)BUF(vectors), (const int64_t *)BUF(ids), dir, &ix);
  (*env)->ReleaseStringUTFChars(env, directory, dir);
  if (rc != 0) {
    throw_runtime(env, ann_codec_last_error());
    return 0;
  }
  return (jlong)(intptr_t)ix;
}
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswIndexDestroy(JNIEnv *env, jclass cls, jlong index) {
  (void)env;
  (void)cls;
  hnsw_index_destroy((hnsw_index_t *)(intptr_t)index);
}
/* void hnswIndexAppend(long index, long n, int d, ByteBuffer vectors /+ float[n][d] +/, ByteBuffer ids /+ long[n] or null +/,
 *                      int efConstruction, long seed)
 * Hnsw.append / HnswIndex.insert for n rows on the device (hnsw_index_append, 4096 rows per round at most); a duplicate key is
 * the RuntimeException in place of IllegalDuplicateInsertException.  One writer at a time per index (Hnsw.append takes
 * readWriteFuturePool.write) */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswIndexAppend(JNIEnv *env, jclass cls, jlong index, jlong n, jint d, jobject vectors,
                                                                       jobject ids, jint efConstruction, jlong seed) {
  (void)cls;
  if (n < 0 || d < 1 || (n > 0 && (!vectors || CAP(vectors) / 4 / d < n)) || (ids && CAP(ids) / 8 < n)) {
    throw_runtime(env, "vectors must hold n x d floats (and ids n longs)");
    return;
  }
  if (!index) {
    throw_runtime(env, "null index");
    return;
  }
  int32_t dim = 0;
  if (hnsw_index_info((const hnsw_index_t *)(intptr_t)index, NULL, &dim, NULL, NULL) != HNSW_OK || dim != d) {
    throw_runtime(env, "d is not the index's dimension");
    return;
  }
  if (hnsw_index_append((hnsw_index_t *)(intptr_t)index, n, (const float *)BUF(vectors), (const int64_t *)BUF(ids), efConstruction,
                        (uint64_t)seed, 0) != HNSW_OK)
    throw_runtime(env, hnsw_last_error());
}
/* void hnswIndexUpdate(long index, long n, int d, ByteBuffer vectors /+ float[n][d] +/, ByteBuffer ids /+ long[n] +/,
 *                      int efConstruction, long seed)
 * Hnsw.update / SerializableHnsw.update for n rows on the device (hnsw_index_update, 4096 rows per round): a key already in the
 * index is re-inserted with its new embedding, an absent key inserted; ids are positions on an index created without ids.  One
 * writer at a time per index (Hnsw.update takes readWriteFuturePool.write) */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswIndexUpdate(JNIEnv *env, jclass cls, jlong index, jlong n, jint d, jobject vectors,
                                                                       jobject ids, jint efConstruction, jlong seed) {
  (void)cls;
  if (n < 0 || d < 1 || (n > 0 && (!vectors || CAP(vectors) / 4 / d < n || !ids || CAP(ids) / 8 < n))) {
    throw_runtime(env, "vectors must hold n x d floats and ids n longs");
    return;
  }
  if (!index) {
    throw_runtime(env, "null index");
    return;
  }
  int32_t dim = 0;
  if (hnsw_index_info((const hnsw_index_t *)(intptr_t)index, NULL, &dim, NULL, NULL) != HNSW_OK || dim != d) {
    throw_runtime(env, "d is not the index's dimension");
    return;
  }
  if (hnsw_index_update((hnsw_index_t *)(intptr_t)index, n, (const float *)BUF(vectors), (const int64_t *)BUF(ids), efConstruction,
                        (uint64_t)seed, 0, NULL) != HNSW_OK)
    throw_runtime(env, hnsw_last_error());
}
/* void hnswSearch(long index, int nq, int d, ByteBuffer x, int k, int ef, ByteBuffer distances, ByteBuffer labels, ByteBuffer counts)
 * = Hnsw.queryWithDistance for nq queries (HnswParams.ef; Hnsw.scala:125-147) */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswSearch(JNIEnv *env, jclass cls, jlong index, jint nq, jint d, jobject x, jint k, jint ef,
                                                                  jobject distances, jobject labels, jobject counts) {
  (void)cls;
  if (!index || nq < 1 || d < 1 || k < 1 || !x || !distances || !labels || !counts) {
    throw_runtime(env, "index, nq >= 1, k >= 1 and four direct buffers");
    return;
  }
  if (CAP(x) / 4 / d < nq || CAP(distances) / 4 / k < nq || CAP(labels) / 8 / k < nq || CAP(counts) / 4 < nq) {
    throw_runtime(env, "a direct buffer is smaller than nq x k (nq x d) entries");
    return;
  }
  int64_t n_ix = 0;
  int32_t d_ix = 0, metric = 0, max_m = 0;
  if (hnsw_index_info((hnsw_index_t *)(intptr_t)index, &n_ix, &d_ix, &metric, &max_m) != HNSW_OK || d_ix != d) {
    throw_runtime(env, "query dimension differs from the index's");
    return;
  }
  if (hnsw_search((hnsw_index_t *)(intptr_t)index, nq, (const float *)BUF(x), k, ef, (float *)BUF(distances), (int64_t *)BUF(labels),
                  (int32_t *)BUF(counts)) != HNSW_OK)
    throw_runtime(env, hnsw_last_error());
}

/* void composeShards(int nShards, int nq, int kIn, ByteBuffer ids /+ long[nShards][nq][kIn] +/, ByteBuffer distances /+ float[..] +/,
 *                    ByteBuffer counts /+ int[nShards][nq] +/, int k, ByteBuffer outIds, ByteBuffer outDistances, ByteBuffer outCounts)
 * = ComposedQueryable.queryWithDistance (ShardApi.scala:71-87) over the batched answers of one index per GPU */
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_composeShards(JNIEnv *env, jclass cls, jint nShards, jint nq, jint kIn, jobject ids,
                                                                     jobject distances, jobject counts, jint k, jobject outIds,
                                                                     jobject outDistances, jobject outCounts) {
  (void)cls;
  if (nShards < 1 || nq < 0 || kIn < 0 || k < 0 || !counts || !outCounts || (kIn > 0 && (!ids || !distances)) || (k > 0 && (!outIds || !outDistances))) {
    throw_runtime(env, "nShards >= 1, nq / kIn / k >= 0 and the direct buffers they need");
    return;
  }
  const jlong rows = (jlong)nShards * nq;
  if (CAP(counts) / 4 < rows || CAP(outCounts) / 4 < nq || (kIn > 0 && (CAP(ids) / 8 / kIn < rows || CAP(distances) / 4 / kIn < rows)) ||
      (k > 0 && (CAP(outIds) / 8 / k < nq || CAP(outDistances) / 4 / k < nq))) {
    throw_runtime(env, "a direct buffer is smaller than nShards x nq x kIn (nq x k) entries");
    return;
  }
  if (dann_compose_shards(nShards, nq, kIn, (const int64_t *)BUF(ids), (const float *)BUF(distances), (const int32_t *)BUF(counts), k,
                          (int64_t *)BUF(outIds), (float *)BUF(outDistances), (int32_t *)BUF(outCounts)) != DANN_OK)
    throw_runtime(env, dann_last_error());
}

/* ---- query by id (include/ann_by_id.h: QueryableByIdImplementation.scala:15-91) ---------------------------------------- */
/* long embeddingStoreBuild(int device, long n, int d, ByteBuffer keys /+ long[n] +/, ByteBuffer vectors /+ float[n][d] +/)
 * the EmbeddingProducer of the by-id queries, resident on the device; a repeated key is the RuntimeException */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_embeddingStoreBuild(JNIEnv *env, jclass cls, jint device, jlong n, jint d, jobject keys,
                                                                            jobject vectors) {
  (void)cls;
  if (n < 0 || d < 1 || (n > 0 && (!keys || !vectors || CAP(keys) / 8 < n || CAP(vectors) / 4 / d < n))) {
    throw_runtime(env, "keys must hold n longs and vectors n x d floats");
    return 0;
  }
  ann_store_t *st = NULL;
  if (ann_store_build(device, n, d, (const int64_t *)BUF(keys), (const float *)BUF(vectors), &st) != ANN_BY_ID_OK) {
    throw_runtime(env, ann_by_id_last_error());
    return 0;
  }
  return (jlong)(intptr_t)st;
}
JNIEXPORT void JNICALL Java_com_twitter_ann_gpu_AnnJni_embeddingStoreDestroy(JNIEnv *env, jclass cls, jlong store) {
  (void)env;
  (void)cls;
  ann_store_destroy((ann_store_t *)(intptr_t)store);
}
/* the capacities of a by-id call: seeds long[nSeeds], outSeeds / outIds long[cap], outDistances float[cap], outCounts int[nSeeds] */
static int by_id_buffers_ok(JNIEnv *env, jlong index, jint nSeeds, jobject seeds, jint k, jobject outSeeds, jobject outIds,
                            jobject outDistances, jlong cap, jobject outCounts) {
  if (!index || nSeeds < 0 || k < 1 || cap < 0 || (nSeeds > 0 && (!seeds || !outCounts)) || (cap > 0 && (!outSeeds || !outIds || !outDistances))) {
    throw_runtime(env, "index, nSeeds >= 0, k >= 1, cap >= 0 and the direct buffers they need");
    return 0;
  }
  if (CAP(seeds) / 8 < nSeeds || CAP(outCounts) / 4 < nSeeds || CAP(outSeeds) / 8 < cap || CAP(outIds) / 8 < cap || CAP(outDistances) / 4 < cap) {
    throw_runtime(env, "a direct buffer is smaller than nSeeds (cap) entries");
    return 0;
  }
  return 1;
}
/* long hnswBatchQueryById(long index, long store /+ 0: the index's own keys and rows +/, int nSeeds, ByteBuffer seeds, int k, int ef,
 *                         ByteBuffer outSeeds, ByteBuffer outIds, ByteBuffer outDistances, long cap, ByteBuffer outCounts)
 * = QueryableById.batchQueryWithDistanceById: returns the number of (seed, neighbour, distance) triples written, in seed order;
 * outCounts[i] = -1 for a seed the store does not hold */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_hnswBatchQueryById(JNIEnv *env, jclass cls, jlong index, jlong store, jint nSeeds,
                                                                           jobject seeds, jint k, jint ef, jobject outSeeds, jobject outIds,
                                                                           jobject outDistances, jlong cap, jobject outCounts) {
  (void)cls;
  if (!by_id_buffers_ok(env, index, nSeeds, seeds, k, outSeeds, outIds, outDistances, cap, outCounts)) return 0;
  int64_t total = 0;
  if (hnsw_batch_query_by_id((hnsw_index_t *)(intptr_t)index, (const ann_store_t *)(intptr_t)store, nSeeds, (const int64_t *)BUF(seeds), k, ef,
                             (int64_t *)BUF(outSeeds), (int64_t *)BUF(outIds), (float *)BUF(outDistances), cap, &total,
                             (int32_t *)BUF(outCounts)) != ANN_BY_ID_OK) {
    throw_runtime(env, ann_by_id_last_error());
    return 0;
  }
  return (jlong)total;
}
/* long denseBatchQueryById(long index, long store, int nSeeds, ByteBuffer seeds, int k, ByteBuffer outSeeds, ByteBuffer outIds,
 *                          ByteBuffer outDistances, long cap, ByteBuffer outCounts)     the same on the exhaustive index */
JNIEXPORT jlong JNICALL Java_com_twitter_ann_gpu_AnnJni_denseBatchQueryById(JNIEnv *env, jclass cls, jlong index, jlong store, jint nSeeds,
                                                                            jobject seeds, jint k, jobject outSeeds, jobject outIds,
                                                                            jobject outDistances, jlong cap, jobject outCounts) {
  (void)cls;
  if (!by_id_buffers_ok(env, index, nSeeds, seeds, k, outSeeds, outIds, outDistances, cap, outCounts)) return 0;
  int64_t total = 0;
  if (dann_batch_query_by_id((dann_index_t *)(intptr_t)index, (const ann_store_t *)(intptr_t)store, nSeeds, (const int64_t *)BUF(seeds), k,
                             (int64_t *)BUF(outSeeds), (int64_t *)BUF(outIds), (float *)BUF(outDistances), cap, &total,
                             (int32_t *)BUF(outCounts)) != ANN_BY_ID_OK) {
    throw_runtime(env, ann_by_id_last_error());
    return 0;
  }
  return (jlong)total;
}
