// opq_ann.hip -- the OPQ pre-transform in front of the IVF-PQ index (`OPQ<M>[_<dout>],IVF<nlist>,PQ<M>`) for gfx950.
//
// What it replaces: the factory string the reference's Faiss path builds when the caller gives none
// (ann/src/main/python/dataflow/faiss_index_bq_dataset.py:178-188), i.e. Faiss's IndexPreTransform(OPQMatrix, IVFPQ).
// The contract is include/opq_ann.h; everything behind the transform is ivfpq_ann.hip, reached device to device through
// ivf_device_rows.h: transformed rows, queries and the training set never cross to the host.
//
// Shape of the computation.
//   * opq_transform_kernel: one workgroup per (64 rows, 64 outputs).  A K-step of 32 components of the rows and of the
//     matrix is staged in LDS ([k][64 + 4]: a thread reads its 4 rows and its 4 matrix rows as one 16-byte LDS read each,
//     the rows as a broadcast); a thread owns a 4 x 4 block of outputs and runs their 16 fp32 FMA chains in ascending i,
//     so a value depends on its row and its matrix row alone.  Cosine: the workgroup first takes the norms of its rows by
//     the arithmetic of store_rows_kernel (ivf_kernels.h) and divides while staging.  fp32-input MFMA runs at the vector
//     rate on gfx950 and would leave the order of summation to the hardware: not used.
//   * Training alternates on the device: transform -> fp16 -> product quantiser (ivfpq_ann.hip's encoder and mean kernel
//     through pq_train_plain) -> opq_decode_kernel -> opq_error_kernel -> opq_correlation_kernel (one workgroup per
//     (32 i, 32 j, 2048 rows), a thread owns 2 x 2 entries of C and walks the chunk's rows in ascending order in fp64)
//     -> opq_correlation_sum_kernel (the chunk partials in ascending chunk order).  No floating-point atomics anywhere.
//     The [d_in][d_out] correlation goes to the host, whose one-sided Jacobi (opq_procrustes) gives the next matrix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/ivf_ann.h"
#include "../../include/ivfpq_ann.h"
#include "../../include/opq_ann.h"
#include "../../include/polysemous_ann.h"
#include "sann_device.h"  // mix64
#include "ivf_device_rows.h"
#include "faiss_restore.h"
#include "ivf_error.h"  // g_err, fail, ITRY, ABI_CATCH
#include "ivf_kernels.h"

namespace {

// a call into ivfpq_ann.hip: the same status codes, its message is in ivfpq_last_error()
#define PCALL(expr)                                              \
  do {                                                           \
    int rc_ = (expr);                                            \
    if (rc_) return fail(rc_, std::string("inner index: ") + ivfpq_last_error()); \
  } while (0)

constexpr int KSUB = 256;
constexpr int MAX_M = 64;
constexpr int MAX_D_IN = 1024;
constexpr int64_t MAX_OPQ_ROWS = 65536;  // rows the matrix is trained on
constexpr int TR = 64, TJ = 64, KS = 32;  // transform tile: rows, outputs, K-step
constexpr int LDT = TR + 4;               // leading dimension of the LDS tiles (16-byte aligned rows)
constexpr int CT = 32, CRS = 32;          // correlation tile: 32 x 32 entries, 32 rows staged at a time
constexpr int CCHUNK = 2048;              // rows per correlation / error chunk

// the norm of row x by the arithmetic of store_rows_kernel; every lane of the wave calls it
__device__ __forceinline__ float row_norm(const float *__restrict__ x, int d, int lane) {
  double ss = 0;
  for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
  ss = wave_sum(ss);
  float norm = (float)sqrt(ss);
  if (!(norm > 0.0f)) norm = 1.0f;
  return norm;
}

// Y[row][j] = the FMA chain over i ascending of A[j][i] * x[row][i] (x divided by its norm first when normalise).
// grid (row tiles, output tiles), 256 threads.  POS: row r of the input is X + pos[r] * d_in -- a row of a device-resident
// store read through a position list (a by-id query, include/faiss_by_id.h); the norms and the tile load go through the
// list, everything after the load is the same statement, so Y is what the plain kernel gives for a copy of those rows.
template <bool POS>
__global__ __launch_bounds__(256) void opq_transform_kernel(const float *__restrict__ A, const float *__restrict__ X,
                                                            const int64_t *__restrict__ pos, int64_t n, int d_in, int d_out,
                                                            int normalise, float *__restrict__ Y) {
  __shared__ __attribute__((aligned(16))) float s_x[KS][LDT];
  __shared__ __attribute__((aligned(16))) float s_a[KS][LDT];
  __shared__ float s_norm[TR];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, tx = t & 15, ty = t >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int j0 = blockIdx.y * TJ;
  if (normalise) {
    for (int r = w; r < TR; r += 4) {  // (row0 + r < n is the same for every lane of the wave)
      float norm = 1.0f;
      if (row0 + r < n) norm = row_norm(X + (size_t)(POS ? pos[row0 + r] : row0 + r) * d_in, d_in, lane);
      if (lane == 0) s_norm[r] = norm;
    }
    __syncthreads();
  }
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
  for (int i0 = 0; i0 < d_in; i0 += KS) {
    const int kmax = min(KS, d_in - i0);
#pragma unroll
    for (int u = 0; u < TR * KS / 256; ++u) {
      const int e = t + 256 * u, kk = e & (KS - 1), r = e / KS;
      float xv = 0.0f, av = 0.0f;
      if (kk < kmax) {
        if (row0 + r < n) {
          xv = X[(size_t)(POS ? pos[row0 + r] : row0 + r) * d_in + i0 + kk];
          if (normalise) xv = xv / s_norm[r];
        }
        if (j0 + r < d_out) av = A[(size_t)(j0 + r) * d_in + i0 + kk];
      }
      s_x[kk][r] = xv;
      s_a[kk][r] = av;
    }
    __syncthreads();
    for (int kk = 0; kk < kmax; ++kk) {
      const float4 x4 = *(const float4 *)&s_x[kk][ty * 4];
      const float4 a4 = *(const float4 *)&s_a[kk][tx * 4];
      const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, as[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(as[c], xs[r], acc[r][c]);
    }
    __syncthreads();
  }
  const int j = j0 + tx * 4;
  if (j >= d_out) return;  // (d_out is a multiple of 16: a group of 4 outputs is inside or outside as a whole)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + ty * 4 + r;
    if (row < n) *(float4 *)&Y[(size_t)row * d_out + j] = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
  }
}

// Cosine training rows, normalised where they lie.  One wave per row.
__global__ void opq_prepare_kernel(float *__restrict__ X, int64_t n, int d) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  float *x = X + (size_t)row * d;
  const float norm = row_norm(x, d, lane);
  for (int k = lane; k < d; k += 64) x[k] = x[k] / norm;
}

// fp32 -> the fp16 the inner index stores
__global__ void opq_round16_kernel(const float *__restrict__ y, int64_t count, _Float16 *__restrict__ y16) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < count) y16[e] = (_Float16)y[e];
}

// Y^[row][m dsub + i] = cb[m][codes[row][m]][i]
__global__ void opq_decode_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ cb, int64_t n, int d, int M, int dsub,
                                  float *__restrict__ yhat) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * d) return;
  const int64_t row = e / d;
  const int c = (int)(e % d), m = c / dsub, i = c % dsub;
  yhat[e] = cb[((size_t)m * KSUB + codes[(size_t)row * M + m]) * dsub + i];
}

// One workgroup per chunk of CCHUNK rows: thread t sums (y - y^)^2 of the chunk's elements t, t + 256, ... in fp64, then a
// fixed tree over the 256 threads.  The host adds the chunk sums in ascending order.
__global__ __launch_bounds__(256) void opq_error_kernel(const _Float16 *__restrict__ y16, const float *__restrict__ yhat, int64_t n,
                                                        int d, double *__restrict__ part) {
  __shared__ double s_acc[256];
  const int t = threadIdx.x;
  const int64_t r1 = ((int64_t)blockIdx.x + 1) * CCHUNK;
  const int64_t e0 = (int64_t)blockIdx.x * CCHUNK * d, e1 = (r1 < n ? r1 : n) * d;
  double acc = 0;
  for (int64_t e = e0 + t; e < e1; e += 256) {
    const double df = (double)(float)y16[e] - (double)yhat[e];
    acc += df * df;
  }
  s_acc[t] = acc;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if (t < o) s_acc[t] += s_acc[t + o];
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = s_acc[0];
}

// part[chunk][i][j] = the sum over the chunk's rows, ascending, of x[row][i] * y^[row][j] in fp64 (the product of two
// fp32 values is exact there).  grid (i tiles, j tiles, chunks), 256 threads, a thread owns 2 x 2 entries.
__global__ __launch_bounds__(256) void opq_correlation_kernel(const float *__restrict__ X, const float *__restrict__ Yh, int64_t n,
                                                              int d_in, int d_out, double *__restrict__ part) {
  __shared__ float s_x[CRS][CT];
  __shared__ float s_y[CRS][CT];
  const int t = threadIdx.x, ti = (t >> 4) * 2, tj = (t & 15) * 2;
  const int i0 = blockIdx.x * CT, j0 = blockIdx.y * CT;
  const int64_t r_begin = (int64_t)blockIdx.z * CCHUNK, r_end = r_begin + CCHUNK < n ? r_begin + CCHUNK : n;
  double a00 = 0, a01 = 0, a10 = 0, a11 = 0;
  for (int64_t rb = r_begin; rb < r_end; rb += CRS) {
    const int rmax = r_end - rb < CRS ? (int)(r_end - rb) : CRS;
#pragma unroll
    for (int u = 0; u < CRS * CT / 256; ++u) {
      const int e = t + 256 * u, c = e & (CT - 1), r = e / CT;
      const bool in = r < rmax;
      s_x[r][c] = in && i0 + c < d_in ? X[(size_t)(rb + r) * d_in + i0 + c] : 0.0f;
      s_y[r][c] = in && j0 + c < d_out ? Yh[(size_t)(rb + r) * d_out + j0 + c] : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < rmax; ++r) {
      const double x0 = (double)s_x[r][ti], x1 = (double)s_x[r][ti + 1];
      const double y0 = (double)s_y[r][tj], y1 = (double)s_y[r][tj + 1];
      a00 += x0 * y0;
      a01 += x0 * y1;
      a10 += x1 * y0;
      a11 += x1 * y1;
    }
    __syncthreads();
  }
  double *p = part + (size_t)blockIdx.z * d_in * d_out;
  const int i = i0 + ti, j = j0 + tj;
  if (i < d_in && j < d_out) p[(size_t)i * d_out + j] = a00;
  if (i < d_in && j + 1 < d_out) p[(size_t)i * d_out + j + 1] = a01;
  if (i + 1 < d_in && j < d_out) p[(size_t)(i + 1) * d_out + j] = a10;
  if (i + 1 < d_in && j + 1 < d_out) p[(size_t)(i + 1) * d_out + j + 1] = a11;
}
// C[e] = part[0][e] + part[1][e] + ... in ascending chunk order.  One thread per entry.
__global__ void opq_correlation_sum_kernel(const double *__restrict__ part, int chunks, int64_t entries, double *__restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  double acc = 0;
  for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * entries + e];
  C[e] = acc;
}

// ---------------------------------------------------------------------------------------------
// the host's Procrustes step: one-sided Jacobi in fp64, cyclic sweeps in a fixed order
// ---------------------------------------------------------------------------------------------
double dot(const double *a, const double *b, int n) {
  double s = 0;
  for (int k = 0; k < n; ++k) s += a[k] * b[k];
  return s;
}
// v -= <u, v> u for every accepted column u, twice; returns what is left of |v|
double orthogonalise(std::vector<double> &U, const std::vector<int> &accepted, int m, double *v) {
  for (int pass = 0; pass < 2; ++pass)
    for (int l : accepted) {
      const double *u = &U[(size_t)l * m];
      const double p = dot(u, v, m);
      for (int k = 0; k < m; ++k) v[k] -= p * u[k];
    }
  return std::sqrt(dot(v, v, m));
}

void procrustes(int m /*d_in*/, int n /*d_out*/, const double *C, double *A) {
  // W = C V column by column: column k of W is W[k * m ..], of V is V[k * n ..]
  std::vector<double> W((size_t)n * m), V((size_t)n * n, 0.0);
  for (int k = 0; k < n; ++k) {
    for (int i = 0; i < m; ++i) W[(size_t)k * m + i] = C[(size_t)i * n + k];
    V[(size_t)k * n + k] = 1.0;
  }
  const double tol = std::sqrt((double)m) * 2.220446049250313e-16;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double *wp = &W[(size_t)p * m], *wq = &W[(size_t)q * m];
        const double alpha = dot(wp, wp, m), beta = dot(wq, wq, m), gamma = dot(wp, wq, m);
        if (gamma == 0.0 || std::fabs(gamma) <= tol * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tn = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + tn * tn), s = c * tn;
        for (int k = 0; k < m; ++k) {
          const double a = wp[k], b = wq[k];
          wp[k] = c * a - s * b;
          wq[k] = s * a + c * b;
        }
        double *vp = &V[(size_t)p * n], *vq = &V[(size_t)q * n];
        for (int k = 0; k < n; ++k) {
          const double a = vp[k], b = vq[k];
          vp[k] = c * a - s * b;
          vq[k] = s * a + c * b;
        }
      }
    if (!rotated) break;
  }
  // U = W / sigma, in the order of descending sigma, each column orthogonalised against those before it; a column that
  // vanishes (a singular value at rounding level) is completed from the unit vectors e_0, e_1, ...
  std::vector<double> sigma((size_t)n);
  for (int k = 0; k < n; ++k) sigma[(size_t)k] = std::sqrt(dot(&W[(size_t)k * m], &W[(size_t)k * m], m));
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sigma[(size_t)a] > sigma[(size_t)b]; });
  const double smax = n ? sigma[(size_t)order[0]] : 0.0;
  std::vector<int> accepted, missing;
  for (int k : order) {
    double *u = &W[(size_t)k * m];
    bool ok = sigma[(size_t)k] > smax * m * 2.220446049250313e-16 && sigma[(size_t)k] > 0;
    if (ok) {
      for (int i = 0; i < m; ++i) u[i] /= sigma[(size_t)k];
      const double left = orthogonalise(W, accepted, m, u);
      ok = left > 0.5;
      if (ok)
        for (int i = 0; i < m; ++i) u[i] /= left;
    }
    if (ok) accepted.push_back(k);
    else missing.push_back(k);
  }
  int next_e = 0;
  for (int k : missing) {
    double *u = &W[(size_t)k * m];
    for (;; ++next_e) {  // some unit vector keeps at least 1 / sqrt(m) of its length: fewer than m columns are accepted
      std::fill(u, u + m, 0.0);
      u[next_e % m] = 1.0;
      const double left = orthogonalise(W, accepted, m, u);
      if (left >= 0.5 / std::sqrt((double)m)) {
        for (int i = 0; i < m; ++i) u[i] /= left;
        (void)orthogonalise(W, accepted, m, u);
        const double again = std::sqrt(dot(u, u, m));
        for (int i = 0; i < m; ++i) u[i] /= again;
        ++next_e;
        break;
      }
    }
    accepted.push_back(k);
  }
  // A = V U^T: A[j][i] = sum_k V[j][k] U[i][k], k ascending
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < m; ++i) A[(size_t)j * m + i] = 0.0;
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j) {
      const double v = V[(size_t)k * n + j];
      const double *u = &W[(size_t)k * m];
      double *a = &A[(size_t)j * m];
      for (int i = 0; i < m; ++i) a[i] += v * u[i];
    }
}

}  // namespace

struct opq_index {
  int device = 0, metric = 0, d_in = 0, d_out = 0, nlist = 0, M = 0;
  ivfpq_index_t *inner = nullptr;
  Buf A;  // fp32 [d_out][d_in]
  std::vector<float> h_A;
  std::vector<double> err;
  float tr_transform = 0, tr_pq = 0, tr_corr = 0, tr_proc = 0, tr_inner = 0;  // the training
  Buf stage, y;                                                               // per-call scratch
  std::shared_ptr<void> by_id;                                                // the by-id scratch (faiss_by_id.hip)
  float t_transform = 0;                                                      // the last search
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~opq_index() {
    if (inner) (void)ivfpq_index_destroy(inner);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

int inner_metric(int metric) { return metric == IVF_METRIC_COSINE ? IVF_METRIC_INNER_PRODUCT : metric; }

int check_shape(int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M) {
  if (metric < IVF_METRIC_L2 || metric > IVF_METRIC_INNER_PRODUCT) return fail(IVF_EINVAL, "unknown metric");
  if (d_in < 16 || d_in > MAX_D_IN) return fail(IVF_EINVAL, "d_in must be in 16..1024");
  if (d_out > d_in) return fail(IVF_EINVAL, "d_out must not exceed d_in");
  if (d_out < 16 || d_out > MAX_D || d_out % 16) return fail(IVF_EINVAL, "d_out must be a multiple of 16 in 16..512");
  if (nlist < 1 || nlist > MAX_NLIST) return fail(IVF_EINVAL, "nlist must be in 1..65536");
  if (M < 4 || M > MAX_M || M % 4) return fail(IVF_EINVAL, "M must be a multiple of 4 in 4..64");
  if (d_out % M) return fail(IVF_EINVAL, "M must divide d_out");
  return IVF_OK;
}

int new_index(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, std::unique_ptr<opq_index> &ix) {
  ITRY(hipSetDevice(device));
  ix.reset(new opq_index);
  ix->device = device;
  ix->metric = metric;
  ix->d_in = d_in;
  ix->d_out = d_out;
  ix->nlist = nlist;
  ix->M = M;
  for (auto &e : ix->ev) ITRY(hipEventCreate(&e));
  ITRY(ix->A.reserve((size_t)d_out * d_in * sizeof(float)));
  return IVF_OK;
}

int set_matrix(opq_index *ix, const float *A) {
  ix->h_A.assign(A, A + (size_t)ix->d_out * ix->d_in);
  ITRY(hipMemcpy(ix->A.p, A, (size_t)ix->d_out * ix->d_in * sizeof(float), hipMemcpyHostToDevice));
  return IVF_OK;
}

// n device rows [n][d_in] -> [n][d_out] by the matrix of the index; d_pos != NULL: row r is d_x + d_pos[r] * d_in
int transform(opq_index *ix, const float *d_x, int64_t n, bool normalise, float *d_y, hipStream_t st = 0,
              const int64_t *d_pos = nullptr) {
  if (n == 0) return IVF_OK;
  const dim3 grid(blocks_for(n, TR), blocks_for(ix->d_out, TJ));
  if (d_pos)
    hipLaunchKernelGGL(opq_transform_kernel<true>, grid, dim3(256), 0, st, ix->A.as<float>(), d_x, d_pos, n, ix->d_in, ix->d_out,
                       normalise ? 1 : 0, d_y);
  else
    hipLaunchKernelGGL(opq_transform_kernel<false>, grid, dim3(256), 0, st, ix->A.as<float>(), d_x, (const int64_t *)nullptr, n,
                       ix->d_in, ix->d_out, normalise ? 1 : 0, d_y);
  ITRY(hipGetLastError());
  return IVF_OK;
}

// C = X^T Y^ of n device rows -> host, double [d_in][d_out]
int correlation(const float *d_x, const float *d_yh, int64_t n, int d_in, int d_out, Buf &part, Buf &c_dev, double *h_c) {
  const int chunks = (int)blocks_for(n, CCHUNK);
  const int64_t entries = (int64_t)d_in * d_out;
  ITRY(part.reserve((size_t)chunks * entries * sizeof(double)));
  ITRY(c_dev.reserve((size_t)entries * sizeof(double)));
  hipLaunchKernelGGL(opq_correlation_kernel, dim3(blocks_for(d_in, CT), blocks_for(d_out, CT), chunks), dim3(256), 0, 0, d_x, d_yh, n,
                     d_in, d_out, part.as<double>());
  ITRY(hipGetLastError());
  hipLaunchKernelGGL(opq_correlation_sum_kernel, dim3(blocks_for(entries)), dim3(256), 0, 0, part.as<double>(), chunks, entries,
                     c_dev.as<double>());
  ITRY(hipGetLastError());
  ITRY(hipMemcpy(h_c, c_dev.p, (size_t)entries * sizeof(double), hipMemcpyDeviceToHost));
  return IVF_OK;
}

double ms_since(std::chrono::steady_clock::time_point &t0) {
  const auto t1 = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  t0 = t1;
  return ms;
}

// the matrix: niter_opq rounds of transform -> product quantiser -> correlation -> Procrustes over the n device rows d_x
int train_matrix(opq_index *ix, const float *d_x, int64_t n, int rounds, uint64_t seed) {
  const int d_in = ix->d_in, d_out = ix->d_out, M = ix->M, dsub = d_out / M;
  std::vector<double> G((size_t)d_in * d_out), A64((size_t)d_out * d_in), C((size_t)d_in * d_out);
  std::vector<float> A32((size_t)d_out * d_in);
  auto t0 = std::chrono::steady_clock::now();
  // G^T, [d_in][d_out]
  for (int j = 0; j < d_out; ++j)
    for (int i = 0; i < d_in; ++i)
      G[(size_t)i * d_out + j] =
          (double)(sann::mix64(seed + 0xD1B54A32D192ED03ull * (uint64_t)((int64_t)j * d_in + i + 1)) >> 11) * 0x1p-53 - 0.5;
  procrustes(d_in, d_out, G.data(), A64.data());
  for (size_t e = 0; e < A32.size(); ++e) A32[e] = (float)A64[e];
  if (int rc = set_matrix(ix, A32.data())) return rc;
  ix->tr_proc += (float)ms_since(t0);
  Buf y, y16, yhat, cb, codes, part, c_dev, epart;
  const int chunks = (int)blocks_for(n, CCHUNK);
  ITRY(y.reserve((size_t)n * d_out * sizeof(float)));
  ITRY(y16.reserve((size_t)n * d_out * sizeof(_Float16)));
  ITRY(yhat.reserve((size_t)n * d_out * sizeof(float)));
  ITRY(cb.reserve((size_t)M * KSUB * dsub * sizeof(float)));
  ITRY(codes.reserve((size_t)n * M));
  ITRY(epart.reserve((size_t)chunks * sizeof(double)));
  std::vector<double> h_epart((size_t)chunks);
  ix->err.clear();
  for (int t = 0; t < rounds; ++t) {
    if (int rc = transform(ix, d_x, n, false, y.as<float>())) return rc;
    hipLaunchKernelGGL(opq_round16_kernel, dim3(blocks_for(n * d_out)), dim3(256), 0, 0, y.as<float>(), n * d_out, y16.as<_Float16>());
    ITRY(hipGetLastError());
    ITRY(hipDeviceSynchronize());
    ix->tr_transform += (float)ms_since(t0);
    PCALL(ivfpq_internal::pq_train_plain(ix->device, y16.as<_Float16>(), n, d_out, M, t == 0, t == 0 ? 40 : 4, seed,
                                         cb.as<float>(), codes.as<uint8_t>()));
    ix->tr_pq += (float)ms_since(t0);
    hipLaunchKernelGGL(opq_decode_kernel, dim3(blocks_for(n * d_out)), dim3(256), 0, 0, codes.as<uint8_t>(), cb.as<float>(), n, d_out, M,
                       dsub, yhat.as<float>());
    ITRY(hipGetLastError());
    hipLaunchKernelGGL(opq_error_kernel, dim3(chunks), dim3(256), 0, 0, y16.as<_Float16>(), yhat.as<float>(), n, d_out,
                       epart.as<double>());
    ITRY(hipGetLastError());
    if (int rc = correlation(d_x, yhat.as<float>(), n, d_in, d_out, part, c_dev, C.data())) return rc;
    ITRY(hipMemcpy(h_epart.data(), epart.p, (size_t)chunks * sizeof(double), hipMemcpyDeviceToHost));
    double err = 0;
    for (int c = 0; c < chunks; ++c) err += h_epart[(size_t)c];
    ix->err.push_back(err / (double)n);
    ix->tr_corr += (float)ms_since(t0);
    procrustes(d_in, d_out, C.data(), A64.data());
    for (size_t e = 0; e < A32.size(); ++e) A32[e] = (float)A64[e];
    if (int rc = set_matrix(ix, A32.data())) return rc;
    ix->tr_proc += (float)ms_since(t0);
  }
  return IVF_OK;
}

// host rows [r0, r0 + m) -> the staging buffer -> ix->y (prepared and transformed)
int stage_and_transform(opq_index *ix, const float *rows, int64_t m, bool timed) {
  ITRY(ix->stage.reserve((size_t)m * ix->d_in * sizeof(float)));
  ITRY(ix->y.reserve((size_t)m * ix->d_out * sizeof(float)));
  ITRY(hipMemcpy(ix->stage.p, rows, (size_t)m * ix->d_in * sizeof(float), hipMemcpyHostToDevice));
  if (timed) ITRY(hipEventRecord(ix->ev[0], 0));
  if (int rc = transform(ix, ix->stage.as<float>(), m, ix->metric == IVF_METRIC_COSINE, ix->y.as<float>())) return rc;
  if (timed) ITRY(hipEventRecord(ix->ev[1], 0));
  ITRY(hipDeviceSynchronize());
  if (timed) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ix->ev[0], ix->ev[1]);
    ix->t_transform += ms;
  }
  return IVF_OK;
}
int64_t in_slab_rows(const opq_index *ix) { return ivfpq_internal::slab_rows(ix->d_in); }

}  // namespace

// ---------------------------------------------------------------------------------------------
// restoring a saved index (faiss_restore.h): the matrix as given, the inner index begun with its stored values
// ---------------------------------------------------------------------------------------------
int opq_internal::restore_begin(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, const float *A,
                                const float *centroids, const float *codebooks, int32_t ids_mode, int64_t n, opq_index **out) try {
  if (!A || !centroids || !codebooks || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d_in, d_out, nlist, M)) return rc;
  std::unique_ptr<opq_index> ix;
  if (int rc = new_index(device, metric, d_in, d_out, nlist, M, ix)) return rc;
  if (int rc = set_matrix(ix.get(), A)) return rc;
  PCALL(ivfpq_internal::restore_begin(device, inner_metric(metric), d_out, nlist, M, centroids, codebooks, ids_mode, n, &ix->inner));
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

ivfpq_index *opq_internal::inner(const opq_index *ix) { return ix->inner; }

// ---------------------------------------------------------------------------------------------
// the device-rows seam (ivf_device_rows.h): what refine_ann.hip shares with opq_index_add and opq_search
// ---------------------------------------------------------------------------------------------
int64_t opq_internal::slab_rows(const opq_index *ix) { return std::min(in_slab_rows(ix), ivfpq_internal::slab_rows(ix->d_out)); }

int opq_internal::add_slab(opq_index *ix, int64_t r0, int64_t m, const float *d_rows) try {
  if (!ix || !d_rows) return fail(IVF_EINVAL, "null argument");
  if (m < 1 || m > slab_rows(ix)) return fail(IVF_EINVAL, "slab size out of range");
  ITRY(hipSetDevice(ix->device));
  ITRY(ix->y.reserve((size_t)m * ix->d_out * sizeof(float)));
  if (int rc = transform(ix, d_rows, m, ix->metric == IVF_METRIC_COSINE, ix->y.as<float>())) return rc;
  ITRY(hipDeviceSynchronize());
  PCALL(ivfpq_internal::add_slab(ix->inner, r0, m, ix->y.as<float>()));
  return IVF_OK;
} ABI_CATCH

namespace {
// the first half of a search over device queries [nq][d_in]: prepared and transformed where they lie into ix->y, timed;
// d_pos != NULL: query i is row d_pos[i] of the store whose first row is d_queries
int transform_queries(opq_index *ix, const float *d_queries, int32_t nq, const int64_t *d_pos = nullptr) {
  if (!ix || !d_queries) return fail(IVF_EINVAL, "null argument");
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  ITRY(hipSetDevice(ix->device));
  ix->t_transform = 0;
  ITRY(ix->y.reserve((size_t)nq * ix->d_out * sizeof(float)));
  ITRY(hipEventRecord(ix->ev[0], 0));
  if (int rc = transform(ix, d_queries, nq, ix->metric == IVF_METRIC_COSINE, ix->y.as<float>(), 0, d_pos)) return rc;
  ITRY(hipEventRecord(ix->ev[1], 0));
  ITRY(hipDeviceSynchronize());
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ix->ev[0], ix->ev[1]);
  ix->t_transform += ms;
  return IVF_OK;
}
}  // namespace

int opq_internal::search_positions(opq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t *d_pos,
                                   uint32_t *d_rank, int32_t *d_counts) try {
  if (int rc = transform_queries(ix, d_queries, nq)) return rc;
  PCALL(ivfpq_internal::search_positions(ix->inner, nq, ix->y.as<float>(), k, nprobe, d_pos, d_rank, d_counts));
  return IVF_OK;
} ABI_CATCH

int opq_internal::search_device_out(opq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht,
                                    float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (int rc = transform_queries(ix, d_queries, nq)) return rc;  // (the inner search checks k, nprobe and the outputs)
  PCALL(ivfpq_internal::search_device_out(ix->inner, nq, ix->y.as<float>(), k, nprobe, ht, d_dist, d_ids, d_counts));
  return IVF_OK;
} ABI_CATCH

int opq_internal::search_store_out(opq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k,
                                   int32_t nprobe, int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (!d_pos) return fail(IVF_EINVAL, "null argument");
  if (int rc = transform_queries(ix, d_store_rows, nq, d_pos)) return rc;
  PCALL(ivfpq_internal::search_device_out(ix->inner, nq, ix->y.as<float>(), k, nprobe, ht, d_dist, d_ids, d_counts));
  return IVF_OK;
} ABI_CATCH

int opq_internal::device_of(const opq_index *ix) { return ix->device; }
int64_t opq_internal::last_control_bytes(const opq_index *ix) { return ivfpq_internal::last_control_bytes(ix->inner); }
int64_t opq_internal::last_control_upload_bytes(const opq_index *ix) { return ivfpq_internal::last_control_upload_bytes(ix->inner); }
std::shared_ptr<void> &opq_internal::by_id_scratch(opq_index *ix) { return ix->by_id; }

namespace {
int train_index(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, int64_t n_train,
                const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed, bool polysemous, int64_t anneal_iters,
                opq_index_t **out);
}

extern "C" {

const char *opq_last_error(void) { return g_err.c_str(); }

int opq_procrustes(int32_t d_in, int32_t d_out, const double *C, double *A) try {
  if (!C || !A) return fail(IVF_EINVAL, "null argument");
  if (d_out < 1 || d_out > d_in || d_in > MAX_D_IN) return fail(IVF_EINVAL, "1 <= d_out <= d_in <= 1024");
  for (size_t e = 0; e < (size_t)d_in * d_out; ++e)
    if (!std::isfinite(C[e])) return fail(IVF_EINVAL, "the correlation holds a value that is not finite");
  procrustes(d_in, d_out, C, A);
  return IVF_OK;
} ABI_CATCH

int opq_index_load(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, const float *A,
                   const float *centroids, const float *codebooks, opq_index_t **out) try {
  if (!A || !centroids || !codebooks || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d_in, d_out, nlist, M)) return rc;
  std::unique_ptr<opq_index> ix;
  if (int rc = new_index(device, metric, d_in, d_out, nlist, M, ix)) return rc;
  if (int rc = set_matrix(ix.get(), A)) return rc;
  PCALL(ivfpq_index_load(device, inner_metric(metric), d_out, nlist, M, centroids, codebooks, &ix->inner));
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int opq_index_train(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, int64_t n_train,
                    const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed, opq_index_t **out) try {
  return train_index(device, metric, d_in, d_out, nlist, M, n_train, train_vectors, niter, niter_opq, seed, false, 0, out);
} ABI_CATCH

int opq_index_train_polysemous(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M,
                               int64_t n_train, const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed,
                               int64_t anneal_iters, opq_index_t **out) try {
  if (anneal_iters < 0) return fail(IVF_EINVAL, "anneal_iters must be 0 (500000 steps) or a number of steps");
  return train_index(device, metric, d_in, d_out, nlist, M, n_train, train_vectors, niter, niter_opq, seed, true, anneal_iters, out);
} ABI_CATCH

int opq_index_is_polysemous(const opq_index_t *ix, int32_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  PCALL(ivfpq_index_is_polysemous(ix->inner, out));
  return IVF_OK;
} ABI_CATCH

int opq_search_ht(opq_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht, float *out_dist,
                  int64_t *out_ids, int32_t *out_counts) try {
  if (ht <= 0) {  // the filter is off: opq_search itself
    if (int rc = opq_search(ix, nq, queries, k, nprobe, out_dist, out_ids, out_counts)) return rc;
    PCALL(ivfpq_internal::search_stats_unfiltered(ix->inner));
    return IVF_OK;
  }
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (nprobe < 1 || nprobe > MAX_NPROBE) return fail(IVF_EINVAL, "nprobe must be in 1..1024");
  ITRY(hipSetDevice(ix->device));
  ix->t_transform = 0;
  if (int rc = stage_and_transform(ix, queries, nq, true)) return rc;
  PCALL(ivfpq_internal::search_device_ht(ix->inner, nq, ix->y.as<float>(), k, nprobe, ht, out_dist, out_ids, out_counts));
  return IVF_OK;
} ABI_CATCH

int opq_last_query_codes(const opq_index_t *ix, int32_t *nq, int32_t *nprobe, uint8_t *out) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  PCALL(ivfpq_last_query_codes(ix->inner, nq, nprobe, out));
  return IVF_OK;
} ABI_CATCH

int opq_last_ht_stats(const opq_index_t *ix, int64_t *rows_scored) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  PCALL(ivfpq_last_ht_stats(ix->inner, rows_scored));
  return IVF_OK;
} ABI_CATCH

}  // extern "C"

namespace {

// opq_index_train; with polysemous, the final inner index is trained as ivfpq_index_train_polysemous trains
int train_index(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, int64_t n_train,
                const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed, bool polysemous, int64_t anneal_iters,
                opq_index_t **out) {
  if (!train_vectors || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d_in, d_out, nlist, M)) return rc;
  if (n_train < std::max<int64_t>(nlist, KSUB)) return fail(IVF_EINVAL, "n_train must be at least max(nlist, 256)");
  if (n_train >= ((int64_t)1 << 31)) return fail(IVF_EINVAL, "n_train out of range");
  if (niter < -1) return fail(IVF_EINVAL, "niter must be -1 (initial picks), 0 (20 rounds) or a number of rounds");
  if (niter_opq < 0) return fail(IVF_EINVAL, "niter_opq must be 0 (50 rounds) or a number of rounds");
  const int rounds = niter_opq == 0 ? 50 : niter_opq;
  std::unique_ptr<opq_index> ix;
  if (int rc = new_index(device, metric, d_in, d_out, nlist, M, ix)) return rc;
  const bool cosine = metric == IVF_METRIC_COSINE;
  {
    // the rows the matrix is trained on, prepared; they go with this block
    const int64_t n_opq = std::min(n_train, MAX_OPQ_ROWS);
    Buf x;
    ITRY(x.reserve((size_t)n_opq * d_in * sizeof(float)));
    ITRY(hipMemcpy(x.p, train_vectors, (size_t)n_opq * d_in * sizeof(float), hipMemcpyHostToDevice));
    if (cosine) {
      hipLaunchKernelGGL(opq_prepare_kernel, dim3(blocks_for(n_opq, 4)), dim3(256), 0, 0, x.as<float>(), n_opq, d_in);
      ITRY(hipGetLastError());
    }
    ITRY(hipDeviceSynchronize());
    if (int rc = train_matrix(ix.get(), x.as<float>(), n_opq, rounds, seed)) return rc;
  }
  // the inner index on A X of every training row: transformed a slab at a time, kept on the device
  auto t0 = std::chrono::steady_clock::now();
  Buf ytrain;
  ITRY(ytrain.reserve((size_t)n_train * d_out * sizeof(float)));
  const int64_t slab = in_slab_rows(ix.get());
  ITRY(ix->stage.reserve((size_t)std::min(slab, n_train) * d_in * sizeof(float)));
  for (int64_t r0 = 0; r0 < n_train; r0 += slab) {
    const int64_t m = std::min(slab, n_train - r0);
    ITRY(hipMemcpy(ix->stage.p, train_vectors + r0 * d_in, (size_t)m * d_in * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = transform(ix.get(), ix->stage.as<float>(), m, cosine, ytrain.as<float>() + (size_t)r0 * d_out)) return rc;
    ITRY(hipDeviceSynchronize());
  }
  ix->tr_transform += (float)ms_since(t0);
  if (polysemous)
    PCALL(ivfpq_internal::train_device_polysemous(device, inner_metric(metric), d_out, nlist, M, n_train, ytrain.as<float>(), niter,
                                                  seed, anneal_iters, &ix->inner));
  else
    PCALL(ivfpq_internal::train_device(device, inner_metric(metric), d_out, nlist, M, n_train, ytrain.as<float>(), niter, seed,
                                       &ix->inner));
  ix->tr_inner += (float)ms_since(t0);
  *out = ix.release();
  return IVF_OK;
}

}  // namespace

extern "C" {

int opq_index_add(opq_index_t *ix, int64_t n, const float *vectors, const int64_t *ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (n == 0) return IVF_OK;
  if (!vectors) return fail(IVF_EINVAL, "null vectors");
  ITRY(hipSetDevice(ix->device));
  PCALL(ivfpq_internal::add_begin(ix->inner, n, ids != nullptr));
  // a slab the inner index takes in one step: no wider than its own, no more than 64 MiB of rows coming in
  const int64_t slab = std::min(in_slab_rows(ix), ivfpq_internal::slab_rows(ix->d_out));
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    if (int rc = stage_and_transform(ix, vectors + r0 * ix->d_in, m, false)) return rc;
    PCALL(ivfpq_internal::add_slab(ix->inner, r0, m, ix->y.as<float>()));
  }
  PCALL(ivfpq_internal::add_end(ix->inner, n, ids));
  return IVF_OK;
} ABI_CATCH

int opq_search(opq_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
               int32_t *out_counts) try {
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (nprobe < 1 || nprobe > MAX_NPROBE) return fail(IVF_EINVAL, "nprobe must be in 1..1024");
  ITRY(hipSetDevice(ix->device));
  ix->t_transform = 0;
  if (int rc = stage_and_transform(ix, queries, nq, true)) return rc;
  PCALL(ivfpq_internal::search_device(ix->inner, nq, ix->y.as<float>(), k, nprobe, out_dist, out_ids, out_counts));
  return IVF_OK;
} ABI_CATCH

int opq_transform(opq_index_t *ix, int64_t n, const float *x, float *out_y) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (n == 0) return IVF_OK;
  if (!x || !out_y) return fail(IVF_EINVAL, "null argument");
  ITRY(hipSetDevice(ix->device));
  const int64_t slab = in_slab_rows(ix);
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    if (int rc = stage_and_transform(ix, x + r0 * ix->d_in, m, false)) return rc;
    ITRY(hipMemcpy(out_y + r0 * ix->d_out, ix->y.p, (size_t)m * ix->d_out * sizeof(float), hipMemcpyDeviceToHost));
  }
  return IVF_OK;
} ABI_CATCH

int opq_index_info(const opq_index_t *ix, int64_t *n, int32_t *d_in, int32_t *d_out, int32_t *metric, int32_t *nlist,
                   int32_t *M) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n) PCALL(ivfpq_index_info(ix->inner, n, nullptr, nullptr, nullptr, nullptr));
  if (d_in) *d_in = ix->d_in;
  if (d_out) *d_out = ix->d_out;
  if (metric) *metric = ix->metric;
  if (nlist) *nlist = ix->nlist;
  if (M) *M = ix->M;
  return IVF_OK;
} ABI_CATCH

int opq_index_get_matrix(const opq_index_t *ix, float *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  std::copy(ix->h_A.begin(), ix->h_A.end(), out);
  return IVF_OK;
} ABI_CATCH

int opq_training_errors(const opq_index_t *ix, double *out_err, int32_t *count) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (count) *count = (int32_t)ix->err.size();
  if (out_err) std::copy(ix->err.begin(), ix->err.end(), out_err);
  return IVF_OK;
} ABI_CATCH

int opq_training_stats(const opq_index_t *ix, float *transform_ms, float *pq_ms, float *correlation_ms, float *procrustes_ms,
                       float *inner_ms) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (transform_ms) *transform_ms = ix->tr_transform;
  if (pq_ms) *pq_ms = ix->tr_pq;
  if (correlation_ms) *correlation_ms = ix->tr_corr;
  if (procrustes_ms) *procrustes_ms = ix->tr_proc;
  if (inner_ms) *inner_ms = ix->tr_inner;
  return IVF_OK;
} ABI_CATCH

int opq_index_get_centroids(const opq_index_t *ix, float *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  PCALL(ivfpq_index_get_centroids(ix->inner, out));
  return IVF_OK;
} ABI_CATCH

int opq_index_get_codebooks(const opq_index_t *ix, float *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  PCALL(ivfpq_index_get_codebooks(ix->inner, out));
  return IVF_OK;
} ABI_CATCH

int opq_index_get_codes(const opq_index_t *ix, uint8_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  PCALL(ivfpq_index_get_codes(ix->inner, out));
  return IVF_OK;
} ABI_CATCH

int opq_index_list_sizes(const opq_index_t *ix, int64_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  PCALL(ivfpq_index_list_sizes(ix->inner, out));
  return IVF_OK;
} ABI_CATCH

int opq_index_get_assignment(const opq_index_t *ix, int64_t *out_ids, int32_t *out_cells) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  PCALL(ivfpq_index_get_assignment(ix->inner, out_ids, out_cells));
  return IVF_OK;
} ABI_CATCH

int opq_last_probes(const opq_index_t *ix, int32_t *nq, int32_t *nprobe, int32_t *out_cells) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  PCALL(ivfpq_last_probes(ix->inner, nq, nprobe, out_cells));
  return IVF_OK;
} ABI_CATCH

int opq_last_stats(const opq_index_t *ix, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms, float *select_ms,
                   float *transform_ms) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  PCALL(ivfpq_last_stats(ix->inner, rows_scanned, rounds, coarse_ms, scan_ms, select_ms));
  if (transform_ms) *transform_ms = ix->t_transform;
  return IVF_OK;
} ABI_CATCH

int opq_index_destroy(opq_index_t *ix) try {
  delete ix;
  return IVF_OK;
} ABI_CATCH

int opq_debug_correlation(int32_t device, int64_t n, int32_t d_in, int32_t d_out, const float *x, const float *y_hat,
                          double *out_c) try {
  if (!x || !y_hat || !out_c) return fail(IVF_EINVAL, "null argument");
  if (d_out < 1 || d_out > d_in || d_in > MAX_D_IN) return fail(IVF_EINVAL, "1 <= d_out <= d_in <= 1024");
  if (n < 1 || n > MAX_OPQ_ROWS) return fail(IVF_EINVAL, "n must be in 1..65536");
  ITRY(hipSetDevice(device));
  Buf dx, dy, part, c_dev;
  ITRY(dx.reserve((size_t)n * d_in * sizeof(float)));
  ITRY(dy.reserve((size_t)n * d_out * sizeof(float)));
  ITRY(hipMemcpy(dx.p, x, (size_t)n * d_in * sizeof(float), hipMemcpyHostToDevice));
  ITRY(hipMemcpy(dy.p, y_hat, (size_t)n * d_out * sizeof(float), hipMemcpyHostToDevice));
  return correlation(dx.as<float>(), dy.as<float>(), n, d_in, d_out, part, c_dev, out_c);
} ABI_CATCH

}  // extern "C"
