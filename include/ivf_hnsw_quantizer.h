/*
 * ivf_hnsw_quantizer.h -- C ABI of the HNSW coarse quantizer of the inverted-file indexes (Faiss `IVF<nlist>_HNSW<M>`), MI355X.
 *
 * What it serves: FaissRuntimeParam.quantizer_ef (ann_common.thrift:44-56), the runtime parameter of the coarse quantizer
 * that Faiss builds from `IVF<nlist>_HNSW<M>`: a small HNSW graph over the centroids, walked instead of scanned.  The
 * reference hands any factory string to index_factory (FaissIndexer.scala:82-92) and sets the parameter on the index under a
 * lock before a search (QueryableIndexAdapter.scala:70-89).
 *
 * It is a strategy of the one inverted-file core, not an index of its own: an IVF-Flat (ivf_ann.h), IVF-PQ (ivfpq_ann.h) or
 * OPQ (opq_ann.h) index has either no quantizer attached -- the exhaustive coarse search, the default, byte for byte what it
 * is without this header -- or one graph.
 *   kind    FAISS_KIND_IVF_FLAT (1), FAISS_KIND_IVF_PQ (2) or FAISS_KIND_OPQ_IVF_PQ (3) of faiss_files.h; `index` is the
 *           ivf_index_t, ivfpq_index_t or opq_index_t handle that matches (an OPQ index keeps the graph on its inner index)
 *   graph   items are positions 0..nlist-1, so the ids a walk returns are cell numbers; the vectors are the index's stored
 *           (fp16-valued) centroids.  Metric: an L2 index walks an L2 graph, an InnerProduct or Cosine index an InnerProduct
 *           graph -- the index stores unit centroids and prepares unit queries for Cosine, and the graph does not normalise
 *           a second time
 *   search  the prepared fp16 queries go into the graph's prepared-query buffer on the device, hnsw_search's walk runs with
 *           k = nprobe and ef = quantizer_ef (beam = max of the two, HnswIndex.java:545) and leaves its answer on the device,
 *           where it is inverted into the (cell, query) pairs of the scan.  A walk may find fewer than nprobe cells: a
 *           missing probe is -1 in the probe export, contributes no rows, and is not an error
 *   add     rows are assigned by the same walk with k = 1 at the quantizer_ef in force, as Faiss's add goes through the
 *           quantizer.  Training is unchanged (k-means against the exhaustive search; Faiss: quantizer_trains_alone = 2)
 * Attaching is allowed at any time.  It governs later adds and searches only: rows already assigned stay where they are.
 * A refine index (refine_ann.h) inherits the quantizer from its base when the base gets one before it is wrapped.
 * The nlist bound of the indexes (65,536) is unchanged.
 *
 * Status codes are the IVF_* numbers of ivf_ann.h.  No function throws or aborts.  One call at a time per index, the calls
 * on the borrowed graph handle (ivfhq_quantizer) included.
 */
#ifndef IVF_HNSW_QUANTIZER_H
#define IVF_HNSW_QUANTIZER_H
#include <stdint.h>

#include "hnsw_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

const char *ivfhq_last_error(void);

/* Build the graph over the stored centroids on the device, with the arithmetic of hnsw_index_build_insert_gpu (levels drawn
 * from `seed`, `batch` items per round, 0 = 4096): deterministic, two builds of one index give one graph.  The centroids are
 * staged through the host once.  Replaces any attached quantizer and puts quantizer_ef back to its default, 16 (Faiss's
 * efSearch).  The bounds are the builder's own (max_m in 2..32, ef_construction in 1..256; Faiss's efConstruction default is
 * 40); a refusal changes nothing. */
int ivfhq_build(int32_t kind, void *index, int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t batch);

/* Attach a given graph over the index's centroids: the arrays of hnsw_index_build (hnsw_ann.h).  The verbatim restore of a
 * saved quantizer, and what a test hands a hand-made graph to.  An item or neighbour outside [0, nlist), or an absent entry
 * point, is IVF_EINVAL and changes nothing. */
int ivfhq_attach_graph(int32_t kind, void *index, int32_t max_m, int64_t entry_point, int32_t max_level, int64_t n_entries,
                       const int32_t *entry_level, const int64_t *entry_item, const int64_t *entry_offsets,
                       const int64_t *entry_neighbours);

/* Back to the exhaustive quantizer (nothing happens when none is attached). */
int ivfhq_detach(int32_t kind, void *index);

/* quantizer_ef in 1..1024: state on the index, as the reference sets it.  IVF_EINVAL when no quantizer is attached. */
int ivfhq_set_ef(int32_t kind, void *index, int32_t quantizer_ef);

/* Any pointer may be NULL.  Without a quantizer: attached = 0, max_m = 0, quantizer_ef = 16. */
int ivfhq_info(int32_t kind, const void *index, int32_t *attached, int32_t *max_m, int32_t *quantizer_ef);

/* The graph as a borrowed hnsw_index_t, NULL when none is attached.  Every hnsw_index_* export and hnsw_search works on it.
 * It must not be destroyed, appended to or updated: it goes with the index, or with the next build, attach or detach. */
int ivfhq_quantizer(int32_t kind, void *index, hnsw_index_t **borrowed);

/* The prepared queries the last search walked, as fp32 (fp16 values; Cosine: unit length), [nq][d].  Two calls: sizes with
 * out = NULL, then contents.  nq = 0 when the last search walked no graph. */
int ivfhq_last_queries(int32_t kind, const void *index, int32_t *nq, int32_t *d, float *out);

/* The walks of the last search, summed: distance evaluations, layer-0 expansions, and probes the walks did not find. */
int ivfhq_last_stats(int32_t kind, const void *index, int64_t *distance_evals, int64_t *expansions, int64_t *missing_probes);

#ifdef __cplusplus
}
#endif
#endif
