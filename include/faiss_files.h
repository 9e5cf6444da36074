/*
 * faiss_files.h -- the built inverted-file indexes on disk: write one to a directory, read one back onto the device.
 *
 * In the reference an index is never queried by the process that built it (paths relative to ann/src/main/scala/com/
 * twitter/ann/faiss/):
 *   FaissIndexer.scala:82-110                    index_factory -> train -> add_with_ids -> write_index to `faiss.index`,
 *                                                then the success file
 *   FaissIndex.scala:28-, QueryableIndexAdapter.scala:19-31   loadIndex(dimension, metric, directory) reads
 *                                                directory/faiss.index
 *   FaissCommon.scala:39-43                      a directory is an index if it has `_SUCCESS` and `faiss.index`
 * The three index types of ivf_ann.h, ivfpq_ann.h and opq_ann.h get that seam here, as hnsw_index_save_directory /
 * hnsw_index_load_directory of ann_codec.h give it to the HNSW index.
 *
 * PARITY UNPINNED: the reference does not vendor the native Faiss library and the tree holds no written index, so the
 * bytes of Faiss's own write_index cannot be pinned.  The file is this project's own container.  Reading or writing a
 * native Faiss file is out of scope: a file that starts with one of Faiss's four-character codes (IxMp, IxM2, IxPT, IwPQ,
 * IwFl) is refused with a message that says so.
 *
 * The file, byte by byte.  Every integer and float is little-endian.  CRC-32 is the IEEE 802.3 one (reflected polynomial
 * 0xEDB88320, initial value and final xor 0xFFFFFFFF: zlib's crc32).
 *
 *   header, 72 bytes
 *      0  char[8]  magic "AMDIVFX" followed by a 0 byte
 *      8  u32      format version = 1
 *     12  u32      kind: 1 IVF-Flat, 2 IVF-PQ, 3 OPQ + IVF-PQ               (FAISS_KIND_*)
 *     16  u32      metric: 0 L2, 1 Cosine, 2 InnerProduct                   (IVF_METRIC_*); OPQ: that of the OPQ index
 *     20  u32      ids mode: 0 ids are positions, 1 ids were given, 2 no row was added yet (exactly when n = 0)
 *     24  u64      input dimension  (d_in of an OPQ index; otherwise the index dimension)
 *     32  u64      index dimension d (d_out of an OPQ index)
 *     40  u64      nlist
 *     48  u64      M (0 for IVF-Flat)
 *     56  u64      n, the number of rows
 *     64  u32      CRC-32 of bytes 0 .. 63
 *     68  u32      0
 *   then the sections of the kind, in this order and no other, then the end of the file:
 *     CENT  the stored centroids             f32 [nlist][d]                 the values *_index_get_centroids gives
 *     PQCB  the codebooks                    f32 [M * 256][d / M]           kinds 2, 3
 *     OPQA  the OPQ matrix                   f32 [d][input dimension]       kind 3
 *     RIDS  the id of every row              i64 [n][1]                     rows in the order added
 *     CELL  the cell of every row            i32 [n][1]
 *     ROWS  the stored row                   f16 [n][d]                     kind 1: the fp16 bits as stored
 *     CODE  the code of every row            u8  [n][M]                     kinds 2, 3
 *   a section, 32 bytes + data + 4 bytes
 *      0  char[4]  tag
 *      4  u32      bytes per element
 *      8  u64      rows
 *     16  u64      columns
 *     24  u64      length of the data in bytes = rows * columns * bytes per element
 *     32  ...      the data, row-major
 *     ..  u32      CRC-32 of the 32 bytes above and the data
 *
 * The reader does not trust the file.  faiss_file_open reads it once from end to end in pieces of 1 MiB and refuses, as
 * IVF_EINVAL with a message that names the header or the section: a wrong magic or version; a header field outside what the
 * indexes serve; truncation anywhere; a length that overruns the file; a shape whose product overflows or differs from the
 * length; a shape that disagrees with the header (n * M, nlist * d, ...); a checksum mismatch; bytes after the last
 * section.  Payloads are then read in slabs straight into pinned staging memory: no second copy of a large file is held on
 * the host.  What a checksum cannot tell -- a cell outside [0, nlist), an id that is not the row's position in a file
 * whose ids are positions -- a kernel checks on the device, per slab, before anything indexes by a loaded value; the load
 * then fails with IVF_EINVAL naming the first such row, and the partly built index is destroyed.
 *
 * A loaded index holds the values the saved one held, bit for bit: centroids are not rounded or normalised again, stored
 * rows keep their fp16 bits and their squared norms are summed in the order an add sums them; nothing is assigned,
 * encoded or trained.  It remembers whether its ids were given or are positions: a later add obeys the same rule.
 *
 * No function throws or aborts.  Status codes are those of ivf_ann.h; the message is in faiss_last_error() (per thread).
 */
#ifndef FAISS_FILES_H
#define FAISS_FILES_H
#include <stdint.h>

#include "ivf_ann.h"
#include "ivfpq_ann.h"
#include "opq_ann.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FAISS_KIND_IVF_FLAT 1
#define FAISS_KIND_IVF_PQ 2
#define FAISS_KIND_OPQ_IVF_PQ 3

#define FAISS_IDS_POSITIONS 0
#define FAISS_IDS_GIVEN 1
#define FAISS_IDS_NONE 2

#define FAISS_INDEX_FILE_NAME "faiss.index"
#define FAISS_SUCCESS_FILE_NAME "_SUCCESS"

const char *faiss_last_error(void);

/* ---- the file, host only ------------------------------------------------------------------------------------------ */
typedef struct faiss_file faiss_file_t;

/* Writes a whole file at `path` from host arrays (the sections the kind does not have are ignored and may be NULL; with
 * n = 0 so may ids, cells and payload).  The shape is checked as the reader checks it; the values are written as given. */
int faiss_file_write(const char *path, int32_t kind, int32_t metric, int32_t d_in, int32_t d, int32_t nlist, int32_t M,
                     int32_t ids_mode, int64_t n, const float *centroids, const float *codebooks, const float *matrix,
                     const int64_t *ids, const int32_t *cells, const void *payload);
/* Opens and checks the whole file (see above).  Close with faiss_file_close. */
int faiss_file_open(const char *path, faiss_file_t **out);
int faiss_file_info(const faiss_file_t *f, int32_t *kind, int32_t *metric, int32_t *d_in, int32_t *d, int32_t *nlist, int32_t *M,
                    int32_t *ids_mode, int64_t *n);
int faiss_file_read_centroids(faiss_file_t *f, float *out);
int faiss_file_read_codebooks(faiss_file_t *f, float *out); /* kinds 2, 3 */
int faiss_file_read_matrix(faiss_file_t *f, float *out);    /* kind 3 */
/* rows [row0, row0 + m): any of the three outputs may be NULL.  payload: m * d fp16 values (kind 1) or m * M bytes. */
int faiss_file_read_rows(faiss_file_t *f, int64_t row0, int64_t m, int64_t *ids, int32_t *cells, void *payload);
int faiss_file_close(faiss_file_t *f);

/* ---- directories -------------------------------------------------------------------------------------------------- */
/* FaissCommon.isValidFaissIndex: 1 if dir is a directory that holds both the success file and the index file, else 0. */
int faiss_directory_is_valid(const char *dir);

/* Writes the index to a temporary name in dir (created if absent), gives it the index file name (link + unlink: an
 * existing name is refused atomically, so of two savers into one directory neither file is replaced), flushes the
 * directory and then creates the empty success file.  A directory that holds an index file already is refused and left
 * as it is. */
int faiss_ivf_index_save_directory(const ivf_index_t *ix, const char *dir);
int faiss_ivfpq_index_save_directory(const ivfpq_index_t *ix, const char *dir);
int faiss_opq_index_save_directory(const opq_index_t *ix, const char *dir);

/* FaissIndex.loadIndex(dimension, metric, directory): the directory must be valid; expected_dimension is that of the
 * embeddings (the input dimension of an OPQ index) and, like expected_metric, must be the file's.  *kind tells which of
 * ivf_index_t, ivfpq_index_t, opq_index_t *handle is; destroy it with that type's *_index_destroy. */
int faiss_index_load_directory(int32_t device, const char *dir, int32_t expected_dimension, int32_t expected_metric,
                               int32_t *kind, void **handle);

/* The stored rows [row0, row0 + m) of an IVF-Flat index, in the order added: the fp16 bits as stored, m * d of them. */
int faiss_ivf_index_get_rows(const ivf_index_t *ix, int64_t row0, int64_t m, uint16_t *out);
/* FAISS_IDS_* of an index of the given kind. */
int faiss_index_ids_mode(int32_t kind, const void *handle, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
