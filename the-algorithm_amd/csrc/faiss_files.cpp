// faiss_files.cpp -- include/faiss_files.h: the index file (host code, no device call), the directory rules, and save /
// load of the three inverted-file indexes through the restore seam of faiss_restore.h.
//
// Built with FAISS_FILES_HOST_ONLY the file holds the codec and the directory rules alone and links without the device
// code: that is how a stand-alone program runs the reader under the host sanitizers.
#include "../../include/faiss_files.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "abi_guard.h"
#ifndef FAISS_FILES_HOST_ONLY
#include "faiss_restore.h"
#endif
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &m) {
  g_err = m;
  return code;
}

constexpr char MAGIC[8] = {'A', 'M', 'D', 'I', 'V', 'F', 'X', 0};
constexpr uint32_t VERSION = 1;
constexpr size_t HEADER_BYTES = 72, SECTION_HEAD = 32, PIECE = 1 << 20;
constexpr int KSUB = 256;

// ---- CRC-32 (IEEE 802.3, reflected), slicing by 4 ----
struct CrcTable {
  uint32_t t[4][256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 4; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 255];
  }
};
const CrcTable g_crc;
// state in, state out (start from 0xffffffff, finish with ~)
uint32_t crc_update(uint32_t c, const void *data, size_t n) {
  const uint8_t *p = (const uint8_t *)data;
  while (n >= 4) {
    c ^= (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    c = g_crc.t[3][c & 255] ^ g_crc.t[2][(c >> 8) & 255] ^ g_crc.t[1][(c >> 16) & 255] ^ g_crc.t[0][c >> 24];
    p += 4;
    n -= 4;
  }
  while (n--) c = g_crc.t[0][(c ^ *p++) & 255] ^ (c >> 8);
  return c;
}

void put32(uint8_t *p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
void put64(uint8_t *p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
uint32_t get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t get64(const uint8_t *p) { return (uint64_t)get32(p) | (uint64_t)get32(p + 4) << 32; }

struct Header {
  int32_t kind = 0, metric = 0, ids_mode = 0, d_in = 0, d = 0, nlist = 0, M = 0;
  int64_t n = 0;
};
struct SectionSpec {
  const char *tag, *what;
  uint32_t elem;
  uint64_t rows, cols;
};
enum { S_CENT, S_PQCB, S_OPQA, S_RIDS, S_CELL, S_PAYLOAD, S_COUNT };

// what the indexes serve (check_shape of the three modules) and what a header may say
int check_header(const Header &h) {
  if (h.kind < FAISS_KIND_IVF_FLAT || h.kind > FAISS_KIND_OPQ_IVF_PQ) return fail(IVF_EINVAL, "header: unknown kind of index");
  if (h.metric < IVF_METRIC_L2 || h.metric > IVF_METRIC_INNER_PRODUCT) return fail(IVF_EINVAL, "header: unknown metric");
  if (h.ids_mode < FAISS_IDS_POSITIONS || h.ids_mode > FAISS_IDS_NONE) return fail(IVF_EINVAL, "header: unknown ids mode");
  if (h.d < 16 || h.d > 512 || h.d % 16) return fail(IVF_EINVAL, "header: the index dimension must be a multiple of 16 in 16..512");
  if (h.kind == FAISS_KIND_OPQ_IVF_PQ) {
    if (h.d_in < h.d || h.d_in > 1024) return fail(IVF_EINVAL, "header: the input dimension must be in d..1024");
  } else if (h.d_in != h.d) {
    return fail(IVF_EINVAL, "header: the input dimension of an index without a transform is its dimension");
  }
  if (h.nlist < 1 || h.nlist > 65536) return fail(IVF_EINVAL, "header: nlist must be in 1..65536");
  if (h.kind == FAISS_KIND_IVF_FLAT) {
    if (h.M != 0) return fail(IVF_EINVAL, "header: M of an IVF-Flat index must be 0");
  } else if (h.M < 4 || h.M > 64 || h.M % 4 || h.d % h.M) {
    return fail(IVF_EINVAL, "header: M must be a multiple of 4 in 4..64 that divides the dimension");
  }
  if (h.n < 0 || h.n >= ((int64_t)1 << 31) - 64) return fail(IVF_EINVAL, "header: n is out of range");
  if ((h.n == 0) != (h.ids_mode == FAISS_IDS_NONE)) return fail(IVF_EINVAL, "header: the ids mode does not fit n");
  return IVF_OK;
}

// the sections of a header's kind, in file order (absent ones have tag == NULL)
void sections_of(const Header &h, SectionSpec s[S_COUNT]) {
  const bool pq = h.kind != FAISS_KIND_IVF_FLAT;
  s[S_CENT] = {"CENT", "centroids", 4, (uint64_t)h.nlist, (uint64_t)h.d};
  s[S_PQCB] = {pq ? "PQCB" : nullptr, "codebooks", 4, (uint64_t)h.M * KSUB, pq ? (uint64_t)(h.d / h.M) : 0};
  s[S_OPQA] = {h.kind == FAISS_KIND_OPQ_IVF_PQ ? "OPQA" : nullptr, "OPQ matrix", 4, (uint64_t)h.d, (uint64_t)h.d_in};
  s[S_RIDS] = {"RIDS", "ids", 8, (uint64_t)h.n, 1};
  s[S_CELL] = {"CELL", "cells", 4, (uint64_t)h.n, 1};
  if (pq) s[S_PAYLOAD] = {"CODE", "codes", 1, (uint64_t)h.n, (uint64_t)h.M};
  else s[S_PAYLOAD] = {"ROWS", "stored rows", 2, (uint64_t)h.n, (uint64_t)h.d};
}
std::string sec_name(const SectionSpec &s) { return std::string("section ") + s.tag + " (" + s.what + ")"; }

void encode_header(const Header &h, uint8_t out[HEADER_BYTES]) {
  std::memset(out, 0, HEADER_BYTES);
  std::memcpy(out, MAGIC, 8);
  put32(out + 8, VERSION);
  put32(out + 12, (uint32_t)h.kind);
  put32(out + 16, (uint32_t)h.metric);
  put32(out + 20, (uint32_t)h.ids_mode);
  put64(out + 24, (uint64_t)h.d_in);
  put64(out + 32, (uint64_t)h.d);
  put64(out + 40, (uint64_t)h.nlist);
  put64(out + 48, (uint64_t)h.M);
  put64(out + 56, (uint64_t)h.n);
  put32(out + 64, ~crc_update(0xffffffffu, out, 64));
}

struct Fd {
  int fd = -1;
  ~Fd() { reset(); }
  void reset() {
    if (fd >= 0) ::close(fd);
    fd = -1;
  }
};

// all of [off, off + n) or nothing
bool pread_all(int fd, void *buf, size_t n, uint64_t off) {
  uint8_t *p = (uint8_t *)buf;
  while (n) {
    const ssize_t r = ::pread(fd, p, n, (off_t)off);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    p += r;
    off += (uint64_t)r;
    n -= (size_t)r;
  }
  return true;
}
bool write_all(int fd, const void *buf, size_t n) {
  const uint8_t *p = (const uint8_t *)buf;
  while (n) {
    const ssize_t r = ::write(fd, p, n);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    p += r;
    n -= (size_t)r;
  }
  return true;
}

// ---- the writer: header, then sections streamed in pieces with a running checksum ----
struct Writer {
  Fd f;
  std::string path;
  uint32_t crc = 0;
  uint64_t left = 0;
  SectionSpec cur{};
  int io_fail(const char *what) { return fail(IVF_EINVAL, std::string(what) + " " + path + ": " + std::strerror(errno)); }
  int create(const std::string &p, const Header &h) {
    path = p;
    f.fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (f.fd < 0) return io_fail("cannot create");
    uint8_t hb[HEADER_BYTES];
    encode_header(h, hb);
    if (!write_all(f.fd, hb, HEADER_BYTES)) return io_fail("cannot write");
    return IVF_OK;
  }
  int begin(const SectionSpec &s) {
    cur = s;
    uint8_t sh[SECTION_HEAD] = {0};
    std::memcpy(sh, s.tag, 4);
    put32(sh + 4, s.elem);
    put64(sh + 8, s.rows);
    put64(sh + 16, s.cols);
    left = s.rows * s.cols * s.elem;  // (the header was checked: no overflow)
    put64(sh + 24, left);
    crc = crc_update(0xffffffffu, sh, SECTION_HEAD);
    if (!write_all(f.fd, sh, SECTION_HEAD)) return io_fail("cannot write");
    return IVF_OK;
  }
  int append(const void *data, uint64_t bytes) {
    if (bytes > left) return fail(IVF_EINTERNAL, sec_name(cur) + ": more data than announced");
    if (!write_all(f.fd, data, (size_t)bytes)) return io_fail("cannot write");
    crc = crc_update(crc, data, (size_t)bytes);
    left -= bytes;
    return IVF_OK;
  }
  int end() {
    if (left) return fail(IVF_EINTERNAL, sec_name(cur) + ": less data than announced");
    uint8_t c[4];
    put32(c, ~crc);
    if (!write_all(f.fd, c, 4)) return io_fail("cannot write");
    return IVF_OK;
  }
  int whole(const SectionSpec &s, const void *data) {
    if (int rc = begin(s)) return rc;
    const uint64_t bytes = left;
    if (bytes && !data) return fail(IVF_EINVAL, sec_name(s) + ": null data");
    if (bytes)
      if (int rc = append(data, bytes)) return rc;
    return end();
  }
  int finish() {
    if (::fsync(f.fd) != 0) return io_fail("cannot flush");
    const int rc = ::close(f.fd);
    f.fd = -1;
    if (rc != 0) return io_fail("cannot close");
    return IVF_OK;
  }
};

}  // namespace

struct faiss_file {
  Fd f;
  std::string path;
  Header h;
  SectionSpec sec[S_COUNT];
  uint64_t data_off[S_COUNT] = {0};  // where a section's data starts
};

namespace {

int open_checked(const char *path, std::unique_ptr<faiss_file> &out) {
  std::unique_ptr<faiss_file> f(new faiss_file);
  f->path = path;
  f->f.fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (f->f.fd < 0) return fail(IVF_EINVAL, std::string("cannot open ") + path + ": " + std::strerror(errno));
  struct stat st;
  if (::fstat(f->f.fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(IVF_EINVAL, std::string(path) + " is not a regular file");
  const uint64_t size = (uint64_t)st.st_size;
  uint8_t hb[HEADER_BYTES];
  if (size >= 4) {
    if (!pread_all(f->f.fd, hb, 4, 0)) return fail(IVF_EINVAL, "header: cannot read " + f->path);
    for (const char *cc : {"IxMp", "IxM2", "IxPT", "IwPQ", "IwFl"})
      if (std::memcmp(hb, cc, 4) == 0)
        return fail(IVF_EINVAL, std::string("header: the file starts with Faiss's four-character code ") + cc +
                                    ": native Faiss files are not read (this is the project's own container, see faiss_files.h)");
  }
  if (size < HEADER_BYTES) return fail(IVF_EINVAL, "header: the file is truncated (" + std::to_string(size) + " bytes)");
  if (!pread_all(f->f.fd, hb, HEADER_BYTES, 0)) return fail(IVF_EINVAL, "header: cannot read " + f->path);
  if (std::memcmp(hb, MAGIC, 8) != 0) return fail(IVF_EINVAL, "header: wrong magic: not an index file of this project");
  if (get32(hb + 8) != VERSION) return fail(IVF_EINVAL, "header: format version " + std::to_string(get32(hb + 8)) + " is not read (1 is)");
  if (get32(hb + 64) != (uint32_t)~crc_update(0xffffffffu, hb, 64) || get32(hb + 68) != 0)
    return fail(IVF_EINVAL, "header: checksum mismatch");
  // every field is range-checked as 64 unsigned bits before it is narrowed
  const uint64_t kind = get32(hb + 12), metric = get32(hb + 16), mode = get32(hb + 20), d_in = get64(hb + 24), d = get64(hb + 32),
                 nlist = get64(hb + 40), M = get64(hb + 48), n = get64(hb + 56);
  if (kind > 3 || metric > 2 || mode > 2 || d_in > 1024 || d > 512 || nlist > 65536 || M > 64 || n >= ((uint64_t)1 << 31))
    return fail(IVF_EINVAL, "header: a field is outside what the indexes serve (kind, metric, ids mode, dimensions, nlist, M or n)");
  Header &h = f->h;
  h.kind = (int32_t)kind;
  h.metric = (int32_t)metric;
  h.ids_mode = (int32_t)mode;
  h.d_in = (int32_t)d_in;
  h.d = (int32_t)d;
  h.nlist = (int32_t)nlist;
  h.M = (int32_t)M;
  h.n = (int64_t)n;
  if (int rc = check_header(h)) return rc;
  sections_of(h, f->sec);
  std::vector<uint8_t> piece;
  uint64_t off = HEADER_BYTES;
  for (int i = 0; i < S_COUNT; ++i) {
    const SectionSpec &s = f->sec[i];
    if (!s.tag) continue;
    const std::string name = sec_name(s);
    uint8_t sh[SECTION_HEAD];
    if (size - off < SECTION_HEAD) return fail(IVF_EINVAL, name + ": the file is truncated inside the section's header");
    if (!pread_all(f->f.fd, sh, SECTION_HEAD, off)) return fail(IVF_EINVAL, name + ": cannot read");
    if (std::memcmp(sh, s.tag, 4) != 0) return fail(IVF_EINVAL, name + ": expected here, found another tag");
    const uint64_t elem = get32(sh + 4), rows = get64(sh + 8), cols = get64(sh + 16), len = get64(sh + 24);
    uint64_t cells = 0, bytes = 0;
    if (__builtin_mul_overflow(rows, cols, &cells) || __builtin_mul_overflow(cells, elem, &bytes))
      return fail(IVF_EINVAL, name + ": the product of its shape fields overflows");
    if (len != bytes) return fail(IVF_EINVAL, name + ": its length " + std::to_string(len) + " is not the product of its shape fields");
    if (elem != s.elem || rows != s.rows || cols != s.cols)
      return fail(IVF_EINVAL, name + ": its shape [" + std::to_string(rows) + "][" + std::to_string(cols) + "] x " + std::to_string(elem) +
                                  " bytes disagrees with the header, which gives [" + std::to_string(s.rows) + "][" +
                                  std::to_string(s.cols) + "] x " + std::to_string(s.elem));
    off += SECTION_HEAD;
    if (size - off < 4 || len > size - off - 4) return fail(IVF_EINVAL, name + ": its length overruns the file (truncated?)");
    f->data_off[i] = off;
    uint32_t crc = crc_update(0xffffffffu, sh, SECTION_HEAD);
    piece.resize((size_t)std::min<uint64_t>(std::max<uint64_t>(len, 1), PIECE));
    for (uint64_t done = 0; done < len;) {
      const size_t m = (size_t)std::min<uint64_t>(PIECE, len - done);
      if (!pread_all(f->f.fd, piece.data(), m, off + done)) return fail(IVF_EINVAL, name + ": cannot read (truncated?)");
      crc = crc_update(crc, piece.data(), m);
      done += m;
    }
    off += len;
    uint8_t c[4];
    if (!pread_all(f->f.fd, c, 4, off)) return fail(IVF_EINVAL, name + ": cannot read its checksum (truncated?)");
    if (get32(c) != (uint32_t)~crc) return fail(IVF_EINVAL, name + ": checksum mismatch");
    off += 4;
  }
  if (off != size) return fail(IVF_EINVAL, "after the last section: " + std::to_string(size - off) + " bytes that belong to nothing");
  out = std::move(f);
  return IVF_OK;
}

int read_section(faiss_file *f, int which, uint64_t byte0, uint64_t bytes, void *out) {
  const SectionSpec &s = f->sec[which];
  if (!s.tag) return fail(IVF_EINVAL, std::string("this kind of index has no ") + s.what);
  if (bytes == 0) return IVF_OK;
  if (!out) return fail(IVF_EINVAL, "null output");
  // the file was whole when it was opened; one that shrank since is an error, not a short array
  if (!pread_all(f->f.fd, out, (size_t)bytes, f->data_off[which] + byte0))
    return fail(IVF_EINVAL, sec_name(s) + ": cannot read (the file changed after it was opened?)");
  return IVF_OK;
}

std::string join(const char *dir, const char *name) {
  std::string p(dir);
  if (!p.empty() && p.back() != '/') p += '/';
  return p + name;
}
bool exists(const std::string &p, bool want_dir) {
  struct stat st;
  if (::stat(p.c_str(), &st) != 0) return false;
  return want_dir ? S_ISDIR(st.st_mode) : true;
}

}  // namespace

extern "C" {

const char *faiss_last_error(void) { return g_err.c_str(); }

int faiss_file_write(const char *path, int32_t kind, int32_t metric, int32_t d_in, int32_t d, int32_t nlist, int32_t M,
                     int32_t ids_mode, int64_t n, const float *centroids, const float *codebooks, const float *matrix,
                     const int64_t *ids, const int32_t *cells, const void *payload) try {
  if (!path) return fail(IVF_EINVAL, "null path");
  Header h;
  h.kind = kind;
  h.metric = metric;
  h.ids_mode = ids_mode;
  h.d_in = d_in;
  h.d = d;
  h.nlist = nlist;
  h.M = M;
  h.n = n;
  if (int rc = check_header(h)) return rc;
  SectionSpec sec[S_COUNT];
  sections_of(h, sec);
  const void *data[S_COUNT] = {centroids, codebooks, matrix, ids, cells, payload};
  Writer w;
  if (int rc = w.create(path, h)) return rc;
  for (int i = 0; i < S_COUNT; ++i)
    if (sec[i].tag)
      if (int rc = w.whole(sec[i], data[i])) return rc;
  return w.finish();
} ABI_CATCH

int faiss_file_open(const char *path, faiss_file_t **out) try {
  if (!path || !out) return fail(IVF_EINVAL, "null argument");
  std::unique_ptr<faiss_file> f;
  if (int rc = open_checked(path, f)) return rc;
  *out = f.release();
  return IVF_OK;
} ABI_CATCH

int faiss_file_info(const faiss_file_t *f, int32_t *kind, int32_t *metric, int32_t *d_in, int32_t *d, int32_t *nlist, int32_t *M,
                    int32_t *ids_mode, int64_t *n) try {
  if (!f) return fail(IVF_EINVAL, "null file");
  if (kind) *kind = f->h.kind;
  if (metric) *metric = f->h.metric;
  if (d_in) *d_in = f->h.d_in;
  if (d) *d = f->h.d;
  if (nlist) *nlist = f->h.nlist;
  if (M) *M = f->h.M;
  if (ids_mode) *ids_mode = f->h.ids_mode;
  if (n) *n = f->h.n;
  return IVF_OK;
} ABI_CATCH

int faiss_file_read_centroids(faiss_file_t *f, float *out) try {
  if (!f) return fail(IVF_EINVAL, "null file");
  return read_section(f, S_CENT, 0, (uint64_t)f->h.nlist * f->h.d * 4, out);
} ABI_CATCH

int faiss_file_read_codebooks(faiss_file_t *f, float *out) try {
  if (!f) return fail(IVF_EINVAL, "null file");
  return read_section(f, S_PQCB, 0, (uint64_t)KSUB * f->h.d * 4, out);
} ABI_CATCH

int faiss_file_read_matrix(faiss_file_t *f, float *out) try {
  if (!f) return fail(IVF_EINVAL, "null file");
  return read_section(f, S_OPQA, 0, (uint64_t)f->h.d * f->h.d_in * 4, out);
} ABI_CATCH

int faiss_file_read_rows(faiss_file_t *f, int64_t row0, int64_t m, int64_t *ids, int32_t *cells, void *payload) try {
  if (!f) return fail(IVF_EINVAL, "null file");
  if (row0 < 0 || m < 0 || row0 > f->h.n || m > f->h.n - row0) return fail(IVF_EINVAL, "rows outside the file");
  const uint64_t rb = f->sec[S_PAYLOAD].cols * f->sec[S_PAYLOAD].elem;
  if (ids)
    if (int rc = read_section(f, S_RIDS, (uint64_t)row0 * 8, (uint64_t)m * 8, ids)) return rc;
  if (cells)
    if (int rc = read_section(f, S_CELL, (uint64_t)row0 * 4, (uint64_t)m * 4, cells)) return rc;
  if (payload)
    if (int rc = read_section(f, S_PAYLOAD, (uint64_t)row0 * rb, (uint64_t)m * rb, payload)) return rc;
  return IVF_OK;
} ABI_CATCH

int faiss_file_close(faiss_file_t *f) try {
  delete f;
  return IVF_OK;
} ABI_CATCH

int faiss_directory_is_valid(const char *dir) try {
  if (!dir) return 0;
  return exists(dir, true) && exists(join(dir, FAISS_SUCCESS_FILE_NAME), false) && exists(join(dir, FAISS_INDEX_FILE_NAME), false) ? 1 : 0;
} catch (...) {
  return 0;
}

}  // extern "C"

#ifndef FAISS_FILES_HOST_ONLY
// ---------------------------------------------------------------------------------------------
// the indexes: device -> file, file -> device
// ---------------------------------------------------------------------------------------------
namespace {

#define MCALL(expr, last_error)                       \
  do {                                                \
    int rc_ = (expr);                                 \
    if (rc_) return fail(rc_, std::string(last_error())); \
  } while (0)

int to_file_mode(int ids_mode) { return ids_mode < 0 ? FAISS_IDS_NONE : ids_mode; }
int from_file_mode(int mode) { return mode == FAISS_IDS_NONE ? -1 : mode; }

// rows [r0, r0 + m) of an index: any of ids, cells, payload
struct RowSource {
  const ivf_index *flat = nullptr;
  const ivfpq_index *pq = nullptr;
  int get(int64_t r0, int64_t m, int64_t *ids, int32_t *cells, void *payload) const {
    if (flat) MCALL(ivf_internal::export_rows(flat, r0, m, ids, cells, (uint16_t *)payload), ivf_last_error);
    else MCALL(ivfpq_internal::export_rows(pq, r0, m, ids, cells, (uint8_t *)payload), ivfpq_last_error);
    return IVF_OK;
  }
};

int sync_directory(const char *dir) {
  const int fd = ::open(dir, O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (fd < 0) return fail(IVF_EINVAL, std::string("cannot open ") + dir + ": " + std::strerror(errno));
  const int rc = ::fsync(fd);
  ::close(fd);
  if (rc != 0) return fail(IVF_EINVAL, std::string("cannot flush ") + dir + ": " + std::strerror(errno));
  return IVF_OK;
}

// temporary name -> the index file -> the success file, last.  A writer that dies leaves its faiss.index.tmp.<pid> behind:
// it is no index (the directory has no success file and no faiss.index) and is not removed by a later save.
int save(const char *dir, const Header &h, const float *centroids, const float *codebooks, const float *matrix, const RowSource &src) {
  if (!dir) return fail(IVF_EINVAL, "null directory");
  if (int rc = check_header(h)) return rc;
  if (::mkdir(dir, 0755) != 0 && errno != EEXIST) return fail(IVF_EINVAL, std::string("cannot create ") + dir + ": " + std::strerror(errno));
  if (!exists(dir, true)) return fail(IVF_EINVAL, std::string(dir) + " is not a directory");
  const std::string final_path = join(dir, FAISS_INDEX_FILE_NAME);
  if (exists(final_path, false)) return fail(IVF_EINVAL, final_path + " exists already: an index is not written over another");
  const std::string tmp = join(dir, (std::string(FAISS_INDEX_FILE_NAME) + ".tmp." + std::to_string((long)::getpid())).c_str());
  SectionSpec sec[S_COUNT];
  sections_of(h, sec);
  int rc = IVF_OK;
  {
    Writer w;
    rc = w.create(tmp, h);
    const void *small[3] = {centroids, codebooks, matrix};
    for (int i = S_CENT; i <= S_OPQA && !rc; ++i)
      if (sec[i].tag) rc = w.whole(sec[i], small[i]);
    // the per-row sections, each streamed through one slab
    const int64_t slab = std::max<int64_t>(1, (int64_t)(32 << 20) / (int64_t)std::max<uint64_t>(8, sec[S_PAYLOAD].cols * sec[S_PAYLOAD].elem));
    std::vector<uint8_t> buf;
    for (int i = S_RIDS; i <= S_PAYLOAD && !rc; ++i) {
      const uint64_t rb = sec[i].cols * sec[i].elem;
      rc = w.begin(sec[i]);
      for (int64_t r0 = 0; r0 < h.n && !rc; r0 += slab) {
        const int64_t m = std::min(slab, h.n - r0);
        buf.resize((size_t)m * rb);
        rc = src.get(r0, m, i == S_RIDS ? (int64_t *)buf.data() : nullptr, i == S_CELL ? (int32_t *)buf.data() : nullptr,
                     i == S_PAYLOAD ? buf.data() : nullptr);
        if (!rc) rc = w.append(buf.data(), (uint64_t)m * rb);
      }
      if (!rc) rc = w.end();
    }
    if (!rc) rc = w.finish();
  }
  // the temporary file takes the final name by link(), which refuses an existing name atomically: of two savers into one
  // directory one is refused, neither file is replaced
  if (!rc && ::link(tmp.c_str(), final_path.c_str()) != 0)
    rc = errno == EEXIST ? fail(IVF_EINVAL, final_path + " exists already: an index is not written over another")
                         : fail(IVF_EINVAL, "cannot name " + tmp + " " + final_path + ": " + std::strerror(errno));
  (void)::unlink(tmp.c_str());
  if (rc) return rc;
  // the name is on disk before the success file says so
  if (int rc2 = sync_directory(dir)) return rc2;
  const std::string ok = join(dir, FAISS_SUCCESS_FILE_NAME);
  const int fd = ::open(ok.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (fd < 0) return fail(IVF_EINVAL, "cannot create " + ok + ": " + std::strerror(errno));
  ::close(fd);
  return sync_directory(dir);
}

// the rows of the file -> the index, a slab at a time through the index's pinned staging memory
template <class Index, class Payload>
int restore_rows(faiss_file *f, Index *ix, int64_t slab, int (*stage)(Index *, int64_t, int64_t **, int32_t **, Payload **),
                 int (*put)(Index *, int64_t, int64_t), int (*end)(Index *), const char *(*last_error)()) {
  const int64_t n = f->h.n;
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    int64_t *ids = nullptr;
    int32_t *cells = nullptr;
    Payload *payload = nullptr;
    MCALL(stage(ix, m, &ids, &cells, &payload), last_error);
    if (int rc = faiss_file_read_rows(f, r0, m, ids, cells, payload)) return rc;
    MCALL(put(ix, r0, m), last_error);
  }
  MCALL(end(ix), last_error);
  return IVF_OK;
}

struct FileCloser {
  void operator()(faiss_file *f) const { delete f; }
};

}  // namespace

extern "C" {

int faiss_ivf_index_save_directory(const ivf_index_t *ix, const char *dir) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  Header h;
  h.kind = FAISS_KIND_IVF_FLAT;
  MCALL(ivf_index_info(ix, &h.n, &h.d, &h.metric, &h.nlist), ivf_last_error);
  h.d_in = h.d;
  h.ids_mode = to_file_mode(ivf_internal::ids_mode(ix));
  std::vector<float> cent((size_t)h.nlist * h.d);
  MCALL(ivf_index_get_centroids(ix, cent.data()), ivf_last_error);
  RowSource src;
  src.flat = ix;
  return save(dir, h, cent.data(), nullptr, nullptr, src);
} ABI_CATCH

int faiss_ivfpq_index_save_directory(const ivfpq_index_t *ix, const char *dir) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  Header h;
  h.kind = FAISS_KIND_IVF_PQ;
  MCALL(ivfpq_index_info(ix, &h.n, &h.d, &h.metric, &h.nlist, &h.M), ivfpq_last_error);
  h.d_in = h.d;
  h.ids_mode = to_file_mode(ivfpq_internal::ids_mode(ix));
  std::vector<float> cent((size_t)h.nlist * h.d), cb((size_t)KSUB * h.d);
  MCALL(ivfpq_index_get_centroids(ix, cent.data()), ivfpq_last_error);
  MCALL(ivfpq_index_get_codebooks(ix, cb.data()), ivfpq_last_error);
  RowSource src;
  src.pq = ix;
  return save(dir, h, cent.data(), cb.data(), nullptr, src);
} ABI_CATCH

int faiss_opq_index_save_directory(const opq_index_t *ix, const char *dir) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  Header h;
  h.kind = FAISS_KIND_OPQ_IVF_PQ;
  MCALL(opq_index_info(ix, &h.n, &h.d_in, &h.d, &h.metric, &h.nlist, &h.M), opq_last_error);
  const ivfpq_index *inner = opq_internal::inner(ix);
  h.ids_mode = to_file_mode(ivfpq_internal::ids_mode(inner));
  std::vector<float> cent((size_t)h.nlist * h.d), cb((size_t)KSUB * h.d), A((size_t)h.d * h.d_in);
  MCALL(opq_index_get_centroids(ix, cent.data()), opq_last_error);
  MCALL(opq_index_get_codebooks(ix, cb.data()), opq_last_error);
  MCALL(opq_index_get_matrix(ix, A.data()), opq_last_error);
  RowSource src;
  src.pq = inner;
  return save(dir, h, cent.data(), cb.data(), A.data(), src);
} ABI_CATCH

int faiss_index_load_directory(int32_t device, const char *dir, int32_t expected_dimension, int32_t expected_metric, int32_t *kind,
                               void **handle) try {
  if (!dir || !kind || !handle) return fail(IVF_EINVAL, "null argument");
  if (!faiss_directory_is_valid(dir))
    return fail(IVF_EINVAL, std::string(dir) + " is not an index directory (it needs " FAISS_SUCCESS_FILE_NAME " and " FAISS_INDEX_FILE_NAME ")");
  std::unique_ptr<faiss_file, FileCloser> f;
  {
    std::unique_ptr<faiss_file> opened;
    if (int rc = open_checked(join(dir, FAISS_INDEX_FILE_NAME).c_str(), opened)) return rc;
    f.reset(opened.release());
  }
  const Header &h = f->h;
  if (h.d_in != expected_dimension)
    return fail(IVF_EINVAL, "the index is over dimension " + std::to_string(h.d_in) + ", not the expected " + std::to_string(expected_dimension));
  if (h.metric != expected_metric)
    return fail(IVF_EINVAL, "the index has metric " + std::to_string(h.metric) + ", not the expected " + std::to_string(expected_metric));
  std::vector<float> cent((size_t)h.nlist * h.d), cb, A;
  if (int rc = faiss_file_read_centroids(f.get(), cent.data())) return rc;
  if (h.kind != FAISS_KIND_IVF_FLAT) {
    cb.resize((size_t)KSUB * h.d);
    if (int rc = faiss_file_read_codebooks(f.get(), cb.data())) return rc;
  }
  const int mode = from_file_mode(h.ids_mode);
  if (h.kind == FAISS_KIND_IVF_FLAT) {
    ivf_index *ix = nullptr;
    MCALL(ivf_internal::restore_begin(device, h.metric, h.d, h.nlist, cent.data(), mode, h.n, &ix), ivf_last_error);
    if (int rc = restore_rows<ivf_index, uint16_t>(f.get(), ix, ivf_internal::restore_slab_rows(h.d), ivf_internal::restore_stage,
                                                   ivf_internal::restore_slab, ivf_internal::restore_end, ivf_last_error)) {
      (void)ivf_index_destroy(ix);
      return rc;
    }
    *handle = ix;
  } else if (h.kind == FAISS_KIND_IVF_PQ) {
    ivfpq_index *ix = nullptr;
    MCALL(ivfpq_internal::restore_begin(device, h.metric, h.d, h.nlist, h.M, cent.data(), cb.data(), mode, h.n, &ix), ivfpq_last_error);
    if (int rc = restore_rows<ivfpq_index, uint8_t>(f.get(), ix, ivfpq_internal::restore_slab_rows(h.M), ivfpq_internal::restore_stage,
                                                    ivfpq_internal::restore_slab, ivfpq_internal::restore_end, ivfpq_last_error)) {
      (void)ivfpq_index_destroy(ix);
      return rc;
    }
    *handle = ix;
  } else {
    A.resize((size_t)h.d * h.d_in);
    if (int rc = faiss_file_read_matrix(f.get(), A.data())) return rc;
    opq_index *ix = nullptr;
    MCALL(opq_internal::restore_begin(device, h.metric, h.d_in, h.d, h.nlist, h.M, A.data(), cent.data(), cb.data(), mode, h.n, &ix),
          opq_last_error);
    if (int rc = restore_rows<ivfpq_index, uint8_t>(f.get(), opq_internal::inner(ix), ivfpq_internal::restore_slab_rows(h.M),
                                                    ivfpq_internal::restore_stage, ivfpq_internal::restore_slab,
                                                    ivfpq_internal::restore_end, ivfpq_last_error)) {
      (void)opq_index_destroy(ix);
      return rc;
    }
    *handle = ix;
  }
  *kind = h.kind;
  return IVF_OK;
} ABI_CATCH

int faiss_ivf_index_get_rows(const ivf_index_t *ix, int64_t row0, int64_t m, uint16_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  MCALL(ivf_internal::export_rows(ix, row0, m, nullptr, nullptr, out), ivf_last_error);
  return IVF_OK;
} ABI_CATCH

int faiss_index_ids_mode(int32_t kind, const void *handle, int32_t *out) try {
  if (!handle || !out) return fail(IVF_EINVAL, "null argument");
  if (kind == FAISS_KIND_IVF_FLAT) *out = to_file_mode(ivf_internal::ids_mode((const ivf_index *)handle));
  else if (kind == FAISS_KIND_IVF_PQ) *out = to_file_mode(ivfpq_internal::ids_mode((const ivfpq_index *)handle));
  else if (kind == FAISS_KIND_OPQ_IVF_PQ) *out = to_file_mode(ivfpq_internal::ids_mode(opq_internal::inner((const opq_index *)handle)));
  else return fail(IVF_EINVAL, "unknown kind of index");
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
#endif  // FAISS_FILES_HOST_ONLY
