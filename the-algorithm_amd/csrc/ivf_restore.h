// ivf_restore.h -- what the two inverted-file indexes share when a saved index is restored (faiss_restore.h): the
// validation kernel, the pinned staging memory and the upload of one slab.  Included by ivf_ann.hip and ivfpq_ann.hip, after
// ivf_kernels.h; everything is file-local.
//
// One slab is read from the file into pinned memory, copied to the device by blocking copies, validated and read back, in
// that order: nothing overlaps.  Pinned memory spares the runtime's own bounce copy of pageable memory; it buys no
// concurrency between the file read and the copy.
#pragma once
#include "ivf_kernels.h"

namespace {

// A slab of loaded (cell, id) pairs, rows [row0, row0 + m) of the index, before anything indexes by them: bad[0] becomes
// the first row whose cell is outside [0, nlist), bad[1] (positions: ids are positions) the first row whose id is not its
// position; both start at 0xffffffff.  Integer minima: any order of the threads gives the same words.
__global__ void validate_slab_kernel(const int32_t *__restrict__ cell, const int64_t *__restrict__ ids, int64_t row0, int64_t m,
                                     int nlist, int positions, uint32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int32_t c = cell[i];
  if (c < 0 || c >= nlist) atomicMin(&bad[0], (uint32_t)(row0 + i));
  if (positions && ids[i] != row0 + i) atomicMin(&bad[1], (uint32_t)(row0 + i));
}

// pinned host memory the file reader fills and the copy engine reads: ids, cells and payload of one slab
struct Pinned {
  void *p = nullptr;
  size_t bytes = 0;
  ~Pinned() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t reserve(size_t n) {
    if (n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, n ? n : 8, hipHostMallocDefault);
    if (e == hipSuccess) bytes = n ? n : 8;
    return e;
  }
};
// what a restore keeps between its steps
struct RestoreState {
  Pinned pin;
  Buf bad;
  int64_t n = 0, done = 0, slab = 0;  // rows announced, rows in, rows of the staging buffer
  int ids_mode = -1;
  bool open = false;
  size_t row_bytes = 0;  // payload bytes per row
  int64_t *ids() const { return (int64_t *)pin.p; }
  int32_t *cells() const { return (int32_t *)((char *)pin.p + (size_t)slab * 8); }
  void *payload() const { return (char *)pin.p + (((size_t)slab * 12 + 15) & ~(size_t)15); }
  void close() {  // the restore is over: the staging memory goes
    open = false;
    pin.release();
  }
  hipError_t stage(int64_t rows, size_t payload_row_bytes) {
    slab = rows;
    row_bytes = payload_row_bytes;
    return pin.reserve((((size_t)rows * 12 + 15) & ~(size_t)15) + (size_t)rows * payload_row_bytes);
  }
};
// the staged slab -> rows [r0, r0 + m) of the per-row device arrays, then the validation kernel; bad[0], bad[1] as above
inline hipError_t restore_upload(RestoreState &rs, int64_t r0, int64_t m, int nlist, int64_t *d_ids, int32_t *d_cell,
                                 void *d_payload, uint32_t bad[2]) {
  hipError_t e = rs.bad.reserve(8);
  if (e != hipSuccess) return e;
  if ((e = hipMemcpy(d_ids + r0, rs.ids(), (size_t)m * 8, hipMemcpyHostToDevice)) != hipSuccess) return e;
  if ((e = hipMemcpy(d_cell + r0, rs.cells(), (size_t)m * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
  if ((e = hipMemcpy((char *)d_payload + (size_t)r0 * rs.row_bytes, rs.payload(), (size_t)m * rs.row_bytes, hipMemcpyHostToDevice)) !=
      hipSuccess)
    return e;
  if ((e = hipMemset(rs.bad.p, 0xff, 8)) != hipSuccess) return e;
  hipLaunchKernelGGL(validate_slab_kernel, dim3(blocks_for(m)), dim3(256), 0, 0, d_cell + r0, d_ids + r0, r0, m, nlist,
                     rs.ids_mode == 0 ? 1 : 0, rs.bad.as<uint32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipMemcpy(bad, rs.bad.p, 8, hipMemcpyDeviceToHost);
}

}  // namespace
