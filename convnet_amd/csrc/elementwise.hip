// HBM-bound pieces of the hot path: elementwise ops, axis reductions, output-layer kernels,
// the SGD update and the RNG-driven ops.  Reference: cudamat/cudamat.cu (host wrappers) +
// cudamat/cudamat_kernels.cu (kernels); semantics pinned by eigenmat/eigenmat.cc (the CPU oracle).
// All kernels stream float4 per lane where the pointers allow it and grid-stride over ~2048 blocks.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace chip {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

inline int blocks_for(size_t work_items) {
  size_t b = (work_items + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

// out[i] = f(i, a[i], b[i]); a/b may alias out.  Vector body + scalar tail.
template <typename F>
__global__ void map2_kernel(float* __restrict__ out, const float* a, const float* b, size_t n, bool vec, F f) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (vec) {
    const size_t n4 = n >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      const f32x4 x = reinterpret_cast<const f32x4*>(a)[i];
      const f32x4 y = b ? reinterpret_cast<const f32x4*>(b)[i] : x;
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = f(x[e], y[e]);
      reinterpret_cast<f32x4*>(out)[i] = r;
    }
    for (size_t i = (n4 << 2) + tid; i < n; i += stride) out[i] = f(a[i], b ? b[i] : a[i]);
  } else {
    for (size_t i = tid; i < n; i += stride) out[i] = f(a[i], b ? b[i] : a[i]);
  }
}

template <typename F>
int map2(cudamat* out, const cudamat* a, const cudamat* b, F f) {
  const size_t n = numel(a);
  if (!a->on_device || !out->on_device || (b && !b->on_device)) return ERROR_NOT_ON_DEVICE;
  if (numel(out) != n || (b && numel(b) != n)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (n == 0) return 0;
  const bool vec = aligned16(out->data_device) && aligned16(a->data_device) && (!b || aligned16(b->data_device));
  KernelTimer timer("map2_kernel", "elementwise", 0.0, 4.0 * n * (b ? 3 : 2));
  hipLaunchKernelGGL(map2_kernel<F>, dim3(blocks_for(n / 4 + 1)), dim3(kThreads), 0, stream(), out->data_device,
                     a->data_device, b ? b->data_device : nullptr, n, vec, f);
  return launch_status();
}

// ---- block reductions ------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
  return t;
}

// target[j] = p*target[j] + mult * sum_i g(mat[i + rows*j]) : one block per column (contiguous).
template <bool SQ>
__global__ void colsum_block_kernel(const float* __restrict__ mat, float* __restrict__ target, int rows, float mult, float p) {
  __shared__ float sh[8];
  const float* col = mat + (size_t)blockIdx.x * rows;
  float s = 0.f;
  if (((reinterpret_cast<uintptr_t>(col) & 15) == 0) && (rows & 3) == 0) {
    const f32x4* c4 = reinterpret_cast<const f32x4*>(col);
    for (int i = threadIdx.x; i < (rows >> 2); i += blockDim.x) {
      const f32x4 v = c4[i];
      s += SQ ? (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]) : (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int i = threadIdx.x; i < rows; i += blockDim.x) s += SQ ? col[i] * col[i] : col[i];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) target[blockIdx.x] = (p != 0.f ? p * target[blockIdx.x] : 0.f) + mult * s;
}

// few, very long columns (shared-bias gradient: 96 columns x 774,400 rows for conv1): split every column
// over gridDim.y blocks into a slab of partial sums, then one tiny deterministic finishing pass.
template <bool SQ>
__global__ void colsum_split_kernel(const float* __restrict__ mat, float* __restrict__ part, int rows, int per) {
  __shared__ float sh[8];
  const float* col = mat + (size_t)blockIdx.x * rows;
  const int beg = blockIdx.y * per, end = min(rows, beg + per);
  float s = 0.f;
  if (((reinterpret_cast<uintptr_t>(col) & 15) == 0) && (rows & 3) == 0 && (per & 3) == 0) {
    const f32x4* c4 = reinterpret_cast<const f32x4*>(col);
    for (int i = (beg >> 2) + threadIdx.x; i < (end >> 2); i += blockDim.x) {
      const f32x4 v = c4[i];
      s += SQ ? (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]) : (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int i = beg + threadIdx.x; i < end; i += blockDim.x) s += SQ ? col[i] * col[i] : col[i];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void colsum_finish_kernel(const float* __restrict__ part, float* __restrict__ target, int cols, int splits, float mult, float p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[(size_t)k * cols + j];
  target[j] = (p != 0.f ? p * target[j] : 0.f) + mult * s;
}

// short columns: one wave per column, 4 columns per block
template <bool SQ>
__global__ void colsum_wave_kernel(const float* __restrict__ mat, float* __restrict__ target, int rows, int cols, float mult, float p) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (j >= cols) return;
  const float* col = mat + (size_t)j * rows;
  float s = 0.f;
  for (int i = l; i < rows; i += 64) s += SQ ? col[i] * col[i] : col[i];
  s = wave_sum(s);
  if (l == 0) target[j] = (p != 0.f ? p * target[j] : 0.f) + mult * s;
}

// many short columns (the reference's two-step shared-bias gradient sums a (batch, pixels*filters) matrix over the batch first,
// src/conv_edge.cc:213-218: 1.16 M columns of 256 for conv1): float4 loads, 8 columns per wave so 8 loads are in flight before
// the first cross-lane reduction.
template <bool SQ>
__global__ void colsum_wave4_kernel(const float* __restrict__ mat, float* __restrict__ target, int rows, int cols, float mult, float p) {
  const int l = threadIdx.x & 63;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
  const int r4 = rows >> 2;
  float s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    s[u] = 0.f;
    if (j0 + u < cols) {
      const f32x4* c4 = reinterpret_cast<const f32x4*>(mat + (size_t)(j0 + u) * rows);
      for (int i = l; i < r4; i += 64) {
        const f32x4 v = c4[i];
        s[u] += SQ ? (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]) : (v[0] + v[1]) + (v[2] + v[3]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float t = wave_sum(s[u]);
    if (l == 0 && j0 + u < cols) target[j0 + u] = (p != 0.f ? p * target[j0 + u] : 0.f) + mult * t;
  }
}

// target[i] = p*target[i] + mult * sum_j g(mat[i + rows*j]) : one thread per row, coalesced over rows.
template <bool SQ>
__global__ void rowsum_kernel(const float* __restrict__ mat, float* __restrict__ target, int rows, int cols, float mult, float p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  float s = 0.f;
  for (int j = 0; j < cols; ++j) {
    const float v = mat[(size_t)i + (size_t)rows * j];
    s += SQ ? v * v : v;
  }
  target[i] = (p != 0.f ? p * target[i] : 0.f) + mult * s;
}

template <bool SQ>
int axis_sum(cudamat* mat, cudamat* target, int axis, float mult, float p) {
  if (!mat->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  const int rows = mat->size[0], cols = mat->size[1];
  if (axis == 0) {
    if (target->size[0] != 1 || target->size[1] != cols) return ERROR_INCOMPATIBLE_DIMENSIONS;
    if (rows >= 32768 && cols < 1024) {
      int splits = 2048 / cols;
      if (splits > rows / 4096) splits = rows / 4096;
      if (splits < 2) splits = 2;
      int per = ((divup(rows, splits) + 3) / 4) * 4;
      splits = divup(rows, per);
      float* part = static_cast<float*>(workspace(sizeof(float) * (size_t)splits * cols));
      KernelTimer timer(SQ ? "colsum_split_kernel<sq>" : "colsum_split_kernel", "colsum", 0.0, 4.0 * rows * cols);
      hipLaunchKernelGGL(colsum_split_kernel<SQ>, dim3(cols, splits), dim3(256), 0, stream(), mat->data_device, part, rows, per);
      hipLaunchKernelGGL(colsum_finish_kernel, dim3(divup(cols, 256)), dim3(256), 0, stream(), part, target->data_device, cols, splits, mult, p);
    } else if (rows >= 2048)
      hipLaunchKernelGGL(colsum_block_kernel<SQ>, dim3(cols), dim3(256), 0, stream(), mat->data_device, target->data_device, rows, mult, p);
    else if ((rows & 3) == 0 && rows >= 128 && cols >= 4096 && (reinterpret_cast<uintptr_t>(mat->data_device) & 15) == 0)
      hipLaunchKernelGGL(colsum_wave4_kernel<SQ>, dim3(divup(cols, 32)), dim3(256), 0, stream(), mat->data_device, target->data_device, rows, cols, mult, p);
    else
      hipLaunchKernelGGL(colsum_wave_kernel<SQ>, dim3(divup(cols, 4)), dim3(256), 0, stream(), mat->data_device, target->data_device, rows, cols, mult, p);
  } else if (axis == 1) {
    if (target->size[1] != 1 || target->size[0] != rows) return ERROR_INCOMPATIBLE_DIMENSIONS;
    hipLaunchKernelGGL(rowsum_kernel<SQ>, dim3(divup(rows, 256)), dim3(256), 0, stream(), mat->data_device, target->data_device, rows, cols, mult, p);
  } else {
    return ERROR_UNSUPPORTED;
  }
  return launch_status();
}

// Whole-matrix reductions return a float to the host (vdot/sum_all/euclid_norm do in the reference
// too: cublasSdot etc.) — a device->host sync, used off the per-step path only.
template <int MODE>  // 0: sum a, 1: sum a*b, 2: sum a*a
__global__ void reduce_all_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, float* __restrict__ out) {
  __shared__ float sh[8];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    s += MODE == 0 ? a[i] : (MODE == 1 ? a[i] * b[i] : a[i] * a[i]);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <int MODE>
float reduce_all(const cudamat* a, const cudamat* b, int* err) {
  *err = 0;
  const size_t n = numel(a);
  const int nb = blocks_for(n) > 256 ? 256 : blocks_for(n);
  float* part = static_cast<float*>(workspace(sizeof(float) * 256));
  hipLaunchKernelGGL(reduce_all_kernel<MODE>, dim3(nb), dim3(kThreads), 0, stream(), a->data_device, b ? b->data_device : nullptr, n, part);
  float host[256];
  if (hipMemcpyAsync(host, part, sizeof(float) * nb, hipMemcpyDeviceToHost, stream()) != hipSuccess ||
      hipStreamSynchronize(stream()) != hipSuccess) {
    *err = CUDA_ERROR;
    return 0.f;
  }
  double t = 0;
  for (int i = 0; i < nb; ++i) t += host[i];
  return (float)t;
}

// ---- row-vector broadcast: mat[:, j] + mult*vec[j] ----------------------------------------------------
__global__ void add_row_kernel(float* __restrict__ out, const float* __restrict__ mat, const float* __restrict__ vec, int rows,
                               size_t n, float mult, bool vec4) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (vec4) {  // rows % 4 == 0: the 4 lanes of a float4 share a column
    for (size_t i = tid; i < (n >> 2); i += stride) {
      const float b = mult * vec[(i << 2) / rows];
      f32x4 v = reinterpret_cast<const f32x4*>(mat)[i];
      v = v + b;
      reinterpret_cast<f32x4*>(out)[i] = v;
    }
  } else {
    for (size_t i = tid; i < n; i += stride) out[i] = mat[i] + mult * vec[i / rows];
  }
}

int add_row(cudamat* mat, cudamat* vec, cudamat* target, float mult) {
  if (!mat->on_device || !vec->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (mat->size[1] != vec->size[1] || vec->size[0] != 1 || mat->size[0] != target->size[0] || mat->size[1] != target->size[1])
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  const size_t n = numel(mat);
  const bool v4 = (mat->size[0] & 3) == 0 && aligned16(mat->data_device) && aligned16(target->data_device);
  hipLaunchKernelGGL(add_row_kernel, dim3(blocks_for(n / 4 + 1)), dim3(kThreads), 0, stream(), target->data_device, mat->data_device,
                     vec->data_device, mat->size[0], n, mult, v4);
  return launch_status();
}

// ---- row-norm limit (axis=1: one output unit's incoming weights), eigenmat.cc:918-968 -----------------
// A (rows x cols) weight matrix is tiled as 256 rows x `chunk` columns per block; a lane owns one row of the
// tile (loads coalesce across lanes) and keeps that row's partial sum of squares privately, so the
// per-row norms come out deterministic (slab of partials + fixed-order finish, no atomics).
//   pass 1 (optionally fused with the SGD update, which touches every weight anyway):  partial[chunk][row]
//   pass 2: factor[row] = (constraint || norm_row > limit) ? limit / norm_row : 1
//   pass 3: rescale — a block exits without touching memory when none of its 256 rows needs scaling, which
//           is the steady state of weight_norm_limit (src/optimizer.cc:75-81).
__device__ __forceinline__ void sgd_one(float& g, float& w, float& h, float l2, float clip, float eps, float mom);

template <bool DO_SGD>
__global__ void rows_sq_kernel(float* __restrict__ g, float* __restrict__ w, float* __restrict__ h, int rows, int cols, int chunk,
                               float* __restrict__ partial, float l2, float clip, float eps, float mom) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int c0 = blockIdx.y * chunk, c1 = min(cols, c0 + chunk);
  float s = 0.f;
  for (int c = c0; c < c1; ++c) {
    const size_t i = (size_t)r + (size_t)rows * c;
    float wv = w[i];
    if (DO_SGD) {
      float gv = g[i], hv = h[i];
      sgd_one(gv, wv, hv, l2, clip, eps, mom);
      g[i] = gv;
      h[i] = hv;
      w[i] = wv;
    }
    s += wv * wv;
  }
  partial[(size_t)blockIdx.y * rows + r] = s;
}

// rows % 4 == 0 and 16-byte aligned bases: a lane owns 4 consecutive rows (one float4 per tensor per column),
// two columns in flight, so each lane keeps 6 independent 16-byte loads outstanding instead of 3 scalar ones.
template <bool DO_SGD>
__global__ void rows_sq4_kernel(float* __restrict__ g, float* __restrict__ w, float* __restrict__ h, int rows, int cols, int chunk,
                                float* __restrict__ partial, float l2, float clip, float eps, float mom) {
  const int r = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= rows) return;
  const int c0 = blockIdx.y * chunk, c1 = min(cols, c0 + chunk);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  auto one = [&](int c) {
    const size_t i = (size_t)r + (size_t)rows * c;
    f32x4 wv = *reinterpret_cast<f32x4*>(w + i);
    if (DO_SGD) {
      f32x4 gv = *reinterpret_cast<f32x4*>(g + i), hv = *reinterpret_cast<f32x4*>(h + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = gv[e], b = wv[e], d = hv[e];
        sgd_one(a, b, d, l2, clip, eps, mom);
        gv[e] = a; wv[e] = b; hv[e] = d;
      }
      *reinterpret_cast<f32x4*>(g + i) = gv;
      *reinterpret_cast<f32x4*>(h + i) = hv;
      *reinterpret_cast<f32x4*>(w + i) = wv;
    }
    s += wv * wv;
  };
  int c = c0;
  for (; c + 1 < c1; c += 2) {
    one(c);
    one(c + 1);
  }
  if (c < c1) one(c);
  *reinterpret_cast<f32x4*>(partial + (size_t)blockIdx.y * rows + r) = s;
}

__global__ void row_factor_kernel(const float* __restrict__ partial, int nchunks, int rows, float norm, int constraint, float* __restrict__ factor) {
  // block = 64 rows x 4 chunk lanes; lane q sums chunks q, q+4, ... then the 4 partials combine in fixed order
  __shared__ float sh[4][64];
  const int r = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  float s = 0.f;
  if (r < rows)
    for (int k = q; k < nchunks; k += 4) s += partial[(size_t)k * rows + r];
  sh[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q != 0 || r >= rows) return;
  s = sqrtf((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]));
  factor[r] = (constraint == 1 || s > norm) ? norm / s : 1.f;
}

__global__ void row_scale_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols, int chunk, const float* __restrict__ factor) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const float f = r < rows ? factor[r] : 1.f;
  const bool in_place = src == dst;
  if (in_place && !__syncthreads_or(f != 1.f)) return;
  if (r >= rows) return;
  const int c0 = blockIdx.y * chunk, c1 = min(cols, c0 + chunk);
  for (int c = c0; c < c1; ++c) {
    const size_t i = (size_t)r + (size_t)rows * c;
    dst[i] = src[i] * f;
  }
}

// grad/history may be null (plain norm limit).  Returns launch status.
inline int rows_normlimit(float* g, float* w_in, float* w_out, float* h, int rows, int cols, float norm, int constraint, bool do_sgd,
                          float l2, float clip, float eps, float mom) {
  int chunk = 64;
  while ((long)divup(rows, 256) * divup(cols, chunk) > 4096 && chunk < cols) chunk *= 2;
  const int nchunks = divup(cols, chunk);
  float* partial = static_cast<float*>(workspace(sizeof(float) * ((size_t)nchunks * rows + rows)));
  float* factor = partial + (size_t)nchunks * rows;
  dim3 grid(divup(rows, 256), nchunks);
  const bool v4 = (rows & 3) == 0 && aligned16(w_in) && (!do_sgd || (aligned16(g) && aligned16(h)));
  // (one timer over the three launches: the fused SGD + row-norm pass reads g, w, h, writes h, w, then re-reads and re-writes w)
  KernelTimer timer(do_sgd ? "rows_sq_kernel<sgd> + row_scale_kernel" : "rows_sq_kernel + row_scale_kernel", do_sgd ? "sgd_normlimit" : "normlimit", 0.0,
                    4.0 * (double)rows * cols * (do_sgd ? 7 : 3));
  if (v4) {
    const dim3 g4(divup(rows / 4, 64), nchunks);
    if (do_sgd)
      hipLaunchKernelGGL(rows_sq4_kernel<true>, g4, dim3(64), 0, stream(), g, w_in, h, rows, cols, chunk, partial, l2, clip, eps, mom);
    else
      hipLaunchKernelGGL(rows_sq4_kernel<false>, g4, dim3(64), 0, stream(), nullptr, w_in, nullptr, rows, cols, chunk, partial, 0.f, 0.f, 0.f, 0.f);
  } else if (do_sgd)
    hipLaunchKernelGGL(rows_sq_kernel<true>, grid, dim3(256), 0, stream(), g, w_in, h, rows, cols, chunk, partial, l2, clip, eps, mom);
  else
    hipLaunchKernelGGL(rows_sq_kernel<false>, grid, dim3(256), 0, stream(), nullptr, w_in, nullptr, rows, cols, chunk, partial, 0.f, 0.f, 0.f, 0.f);
  hipLaunchKernelGGL(row_factor_kernel, dim3(divup(rows, 64)), dim3(256), 0, stream(), partial, nchunks, rows, norm, constraint, factor);
  hipLaunchKernelGGL(row_scale_kernel, grid, dim3(256), 0, stream(), w_in, w_out, rows, cols, chunk, factor);
  return launch_status();
}

__global__ void normlimit_cols_kernel(const float* __restrict__ mat, float* __restrict__ target, int rows, float norm, int constraint) {
  __shared__ float sh[8];
  const float* col = mat + (size_t)blockIdx.x * rows;
  float* out = target + (size_t)blockIdx.x * rows;
  float s = 0.f;
  for (int i = threadIdx.x; i < rows; i += blockDim.x) s += col[i] * col[i];
  s = sqrtf(block_sum(s, sh));
  const float sc = (constraint == 1 || s > norm) ? norm / s : 1.f;
  for (int i = threadIdx.x; i < rows; i += blockDim.x) out[i] = col[i] * sc;
}

// ---- output layer -------------------------------------------------------------------------------------
// "row_major" in the reference = one case per matrix ROW (eigenmat.cc:1093-1131).  A block owns 32
// consecutive rows (128 contiguous bytes per column) and G = 32 column groups (1024 threads: the 256 x 1000
// output layer is 8 blocks, so the per-lane column loop, not bandwidth, sets the time).
struct SoftmaxOut {
  float* probs;    // may alias logits
  float* deriv;    // nullable: probs with 1 subtracted at the label, times deriv_scale
  float* correct;  // nullable: 1x1 accumulator (+= number of argmax==label rows)
};

template <int G>   // column groups per block: 32 rows x G lanes-groups, G*32 threads
__global__ void __launch_bounds__(G * 32) softmax_rows_kernel(const float* logits, const float* __restrict__ labels, SoftmaxOut o, int rows, int cols, float deriv_scale) {
  __shared__ float red[G][33];
  __shared__ int redi[G][33];
  const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int row = blockIdx.x * 32 + r;
  const bool ok = row < rows;
  // pass 1: max and first argmax (strict '<' as eigenmat.cc:1278)
  float mx = -FLT_MAX;
  int am = 0x7fffffff;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const float v = logits[(size_t)j * rows + row];
      if (v > mx) { mx = v; am = j; }
    }
  red[g][r] = mx;
  redi[g][r] = am;
  __syncthreads();
  mx = red[0][r];
  am = redi[0][r];
#pragma unroll
  for (int k = 1; k < G; ++k) {
    const float v = red[k][r];
    const int a = redi[k][r];
    if (v > mx || (v == mx && a < am)) { mx = v; am = a; }
  }
  __syncthreads();
  // pass 2: exp and sum
  float s = 0.f;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const size_t x = (size_t)j * rows + row;
      const float e = expf(logits[x] - mx);
      o.probs[x] = e;
      s += e;
    }
  red[g][r] = s;
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) s += red[k][r];
  // pass 3: normalise (+ CE derivative)
  const int label = (ok && labels) ? (int)labels[row] : -1;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const size_t x = (size_t)j * rows + row;
      const float pr = o.probs[x] / s;
      o.probs[x] = pr;
      if (o.deriv) o.deriv[x] = deriv_scale * (j == label ? pr - 1.0f : pr);
    }
  if (o.correct) {
    __syncthreads();
    if (g == 0) red[0][r] = (ok && am == label) ? 1.f : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      float c = 0.f;
      for (int k = 0; k < 32; ++k) c += red[0][k];
      atomicAdd(o.correct, c);  // integer-valued partial counts: exact and order-independent in fp32
    }
  }
}


// per-row gathers on an already-normalised probability matrix
__global__ void softmax_grad_kernel(const float* __restrict__ labels, float* __restrict__ target, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) target[(size_t)i + (size_t)rows * (int)labels[i]] -= 1.0f;
}

// 32 rows x 32 column-lanes per block: lane c scans columns c, c+32, ... (coalesced over the 32 rows), then the 32 candidates of a
// row are reduced in LDS.  First maximum wins, as a sequential scan with `best < v` would pick it (cudamat.cu softmax-correct kernel).
__global__ void __launch_bounds__(1024) softmax_correct_kernel(const float* __restrict__ mat, const float* __restrict__ labels, float* __restrict__ target, int rows, int cols) {
  __shared__ float sv[32][33];
  __shared__ int si[32][33];
  const int r = threadIdx.x & 31, c = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + r;
  float best = -INFINITY;
  int am = 0x7fffffff;
  if (i < rows)
    for (int j = c; j < cols; j += 32) {
      const float v = mat[(size_t)j * rows + i];
      if (am == 0x7fffffff || best < v) { best = v; am = j; }
    }
  sv[r][c] = best;
  si[r][c] = am;
  __syncthreads();
  if (c == 0 && i < rows) {
    for (int k = 1; k < 32; ++k) {
      const float v = sv[r][k];
      const int j = si[r][k];
      if (j != 0x7fffffff && (best < v || (v == best && j < am))) { best = v; am = j; }
    }
    target[i] = ((int)labels[i] == am) ? 1.f : 0.f;
  }
}

__global__ void softmax_ce_kernel(const float* __restrict__ mat, const float* __restrict__ labels, float* __restrict__ target, int rows, float tiny) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) target[i] = -logf(mat[(size_t)rows * (int)labels[i] + i] + tiny);
}

// ---- Philox-4x32-10 (counter-based; key = (seed, call#), counter = element index / 4) -----------------
// (USER only names an instantiation.  gauss_kernel takes one of its own, USER 1: with further callers of the SAME functions hipcc
// selects other multiplies and another schedule for these rounds inside every rng_kernel — the same integers, but the listings of
// kernels that were measured as they are would move.  One source, two instantiations, rng_kernel's listings unchanged.)
struct Philox {
  unsigned k0, k1;
  template <int USER = 0>
  __device__ void round(unsigned (&c)[4], unsigned ka, unsigned kb) const {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
    c[0] = h1 ^ c[1] ^ ka; c[1] = l1; c[2] = h0 ^ c[3] ^ kb; c[3] = l0;
  }
  template <int USER = 0>
  __device__ void gen(unsigned long long idx, unsigned (&c)[4]) const {
    c[0] = (unsigned)idx; c[1] = (unsigned)(idx >> 32); c[2] = 0x9E3779B9u; c[3] = 0xBB67AE85u;
    unsigned ka = k0, kb = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      round<USER>(c, ka, kb);
      ka += 0x9E3779B9u;
      kb += 0xBB67AE85u;
    }
  }
};

__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }  // [0,1)

__device__ __forceinline__ float sigmoid1(float x) { return 1.0f / (1.0f + expf(-x)); }   // eigenmat.cc:1389; exp overflow gives 1 / inf = 0

// The four uniforms of one Philox quad to its four normals (Box-Muller, two pairs), in place: the one copy of the normal draw, shared
// by rng_kernel<1> (fill_with_randn) and gauss_kernel below, whose noise must be fill_with_randn's bit for bit.
__device__ __forceinline__ void box_muller(float (&u)[4]) {
  const float r0 = sqrtf(-2.f * logf(1.f - u[0])), r1 = sqrtf(-2.f * logf(1.f - u[2]));
  const float t0 = 6.2831853f * u[1], t1 = 6.2831853f * u[3];
  u[0] = r0 * cosf(t0); u[1] = r0 * sinf(t0); u[2] = r1 * cosf(t1); u[3] = r1 * sinf(t1);
}

// MODE 0: uniform fill; 1: normal fill (Box-Muller); 2: dropout(p,val,scale) in place; 3: bernoulli(target = u < mat);
// 4: relu then dropout(p, 0, scale); 5: sigmoid then dropout(p, 0, scale)
template <int MODE>
__global__ void rng_kernel(float* __restrict__ out, const float* __restrict__ in, size_t n, Philox ph, float p, float val, float scale) {
  const size_t n4 = (n + 3) >> 2;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
    unsigned c[4];
    ph.gen(q, c);
    float u[4] = {u01(c[0]), u01(c[1]), u01(c[2]), u01(c[3])};
    if (MODE == 1) box_muller(u);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t i = (q << 2) + e;
      if (i >= n) break;
      if (MODE <= 1) out[i] = u[e];
      else if (MODE == 2) out[i] = (p > u[e]) ? val : in[i] * scale;
      else if (MODE == 3) out[i] = (u[e] < in[i]) ? 1.f : 0.f;
      else if (MODE == 4) { const float x = in[i] > 0.f ? in[i] : 0.f; out[i] = (p > u[e]) ? 0.f : x * scale; }
      else { const float x = sigmoid1(in[i]); out[i] = (p > u[e]) ? 0.f : x * scale; }
    }
  }
}

struct RngHost { unsigned long long seed, counter; };

// the key of one call: (seed, the call counter's value)
inline Philox philox_key(unsigned long long seed, unsigned long long counter) {
  Philox ph;
  ph.k0 = (unsigned)(seed * 0x9E3779B97F4A7C15ull >> 32) ^ (unsigned)counter;
  ph.k1 = (unsigned)seed ^ (unsigned)(counter >> 32) ^ 0x85EBCA6Bu;
  return ph;
}

template <int MODE>
int rng_launch(rnd_struct* st, float* out, const float* in, size_t n, float p, float val, float scale) {
  if (!st || !st->dev_words) return ERROR_GENERIC;
  RngHost* h = reinterpret_cast<RngHost*>(st->dev_words);
  const Philox ph = philox_key(h->seed, h->counter);
  h->counter++;
  if (n == 0) return 0;
  KernelTimer timer(MODE == 2 ? "rng_kernel<dropout>" : MODE == 4 ? "rng_kernel<relu_dropout>" : MODE == 5 ? "rng_kernel<logistic_dropout>" : "rng_kernel", "rng", 0.0, 4.0 * n * (in ? 2 : 1));
  hipLaunchKernelGGL(rng_kernel<MODE>, dim3(blocks_for(n / 4 + 1)), dim3(kThreads), 0, stream(), out, in, n, ph, p, val, scale);
  return launch_status();
}

// ---- Gaussian dropout (src/layer.cc:369-377, 399-404) without a stored noise matrix ------------------------------------------------------
// noise[i] = z[i] * stddev + 1 with z[i] what fill_with_randn writes to element i under the same key: the normal e of Philox quad i / 4,
// quads counted from the FIRST element of the matrix or view.  OP 0 writes the noise; OP 1 is the forward pass in place,
// a = clip(act(a) * noise); OP 2 the backward pass, a = act'(a * noise, b / noise) [b = b / noise when `restore`], drawing the forward
// pass's noise again from its call id.
// The body moves 16 bytes per lane and array and starts at the first 16-byte boundary, `head` (0..3) floats in: lane j holds elements
// head + 4j .. head + 4j + 3, which lie in quad j and, when head != 0, in quad j + 1 — the two groupings of four do not coincide, so
// such a view draws both quads and shifts (twice the draws, on views that start off a boundary only).  The head and the tail, six
// floats at the most, go one element per lane.  Arrays that disagree in their offset (`vec` 0) run the same loop from element 0 with
// four 4-byte accesses per array.
struct GaussArgs {
  float* a;        // OP 0: target; 1: the state; 2: the derivative
  float* b;        // OP 2: the state
  size_t n, head;
  Philox ph;
  float stddev, max_act;
  int vec, restore;
};
__device__ __forceinline__ void gauss_quad(const Philox& ph, size_t q, float (&z)[4]) {
  unsigned c[4];
  ph.gen<1>(q, c);   // (an instantiation of its own: see Philox)
  z[0] = u01(c[0]); z[1] = u01(c[1]); z[2] = u01(c[2]); z[3] = u01(c[3]);
  box_muller(z);
}
template <int OP, int ACT>
__device__ __forceinline__ void gauss_one(const GaussArgs& g, float z, float& a, float& b) {
#pragma clang fp contract(off)
  const float zs = z * g.stddev;
  const float nz = zs + 1.0f;   // mult_by_scalar, then add_scalar: two roundings
  if (OP == 0) {
    a = nz;
  } else if (OP == 1) {
    float x = a;
    if (ACT == 1) x = x > 0.f ? x : 0.f;
    if (ACT == 2) x = sigmoid1(x);
    x = x * nz;
    if (g.max_act > 0.f) x = x > g.max_act ? g.max_act : (x < -g.max_act ? -g.max_act : x);
    a = x;
  } else {
    const float d = a * nz;
    const float s = b / nz;
    if (ACT == 0) a = d;
    if (ACT == 1) a = s > 0.f ? d : 0.f * d;
    if (ACT == 2) {
      const float dy = d * s;
      const float om = 1.0f - s;
      a = dy * om;
    }
    b = s;
  }
}
template <int OP, int ACT>
__global__ void gauss_kernel(const GaussArgs g) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (g.n - g.head) >> 2;
  float* const pa = g.a + g.head;
  float* const pb = OP == 2 ? g.b + g.head : nullptr;
  for (size_t j = tid; j < n4; j += stride) {
    float w[8];
    gauss_quad(g.ph, j, reinterpret_cast<float(&)[4]>(w[0]));
    if (g.head) {   // (the same in every lane)
      gauss_quad(g.ph, j + 1, reinterpret_cast<float(&)[4]>(w[4]));
      if (g.head & 1) {
#pragma unroll
        for (int k = 0; k < 7; ++k) w[k] = w[k + 1];
      }
      if (g.head & 2) {
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = w[k + 2];
      }
    }
    f32x4 a, b;
    if (g.vec) {
      if (OP != 0) a = reinterpret_cast<const f32x4*>(pa)[j];
      if (OP == 2) b = reinterpret_cast<const f32x4*>(pb)[j];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (OP != 0) a[e] = pa[4 * j + e];
        if (OP == 2) b[e] = pb[4 * j + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = OP != 0 ? a[e] : 0.f, y = OP == 2 ? b[e] : 0.f;
      gauss_one<OP, ACT>(g, w[e], x, y);
      a[e] = x;
      b[e] = y;
    }
    if (g.vec) {
      reinterpret_cast<f32x4*>(pa)[j] = a;
      if (OP == 2 && g.restore) reinterpret_cast<f32x4*>(pb)[j] = b;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pa[4 * j + e] = a[e];
        if (OP == 2 && g.restore) pb[4 * j + e] = b[e];
      }
    }
  }
  const size_t rest = g.n - (n4 << 2);   // head + tail
  for (size_t r = tid; r < rest; r += stride) {
    const size_t i = r < g.head ? r : (n4 << 2) + r;
    float z[4];
    gauss_quad(g.ph, i >> 2, z);
    const int e = (int)(i & 3);
    const float zi = e == 0 ? z[0] : e == 1 ? z[1] : e == 2 ? z[2] : z[3];
    float x = OP != 0 ? g.a[i] : 0.f, y = OP == 2 ? g.b[i] : 0.f;
    gauss_one<OP, ACT>(g, zi, x, y);
    g.a[i] = x;
    if (OP == 2 && g.restore) g.b[i] = y;
  }
}

// `a` and `b` (OP 2 only) hold n floats on the device; the key is (the state's seed, call_id)
template <int OP>
int gauss_launch(const rnd_struct* st, unsigned long long call_id, float* a, float* b, size_t n, float stddev, float max_act, int act, int restore) {
  if (n == 0) return 0;
  GaussArgs g{a, b, n, 0, philox_key(reinterpret_cast<const RngHost*>(st->dev_words)->seed, call_id), stddev, max_act, 1, restore};
  const uintptr_t off = reinterpret_cast<uintptr_t>(a) & 15;
  g.vec = (off & 3) == 0 && (OP != 2 || (reinterpret_cast<uintptr_t>(b) & 15) == off);
  g.head = g.vec ? ((16 - off) & 15) >> 2 : 0;
  if (g.head > n) g.head = n;
  // bytes: the noise is written; the state read and written; derivative and state read, the derivative (and the state) written
  const double arrays = OP == 0 ? 1 : OP == 1 ? 2 : restore ? 4 : 3;
  KernelTimer timer(OP == 0 ? "gauss_kernel<noise>" : OP == 1 ? "gauss_kernel<dropout>" : "gauss_kernel<undo>", "gaussian_dropout", 0.0, 4.0 * n * arrays);
  const dim3 grid(blocks_for(n / 4 + 1)), block(kThreads);
  if constexpr (OP == 0) {
    hipLaunchKernelGGL((gauss_kernel<0, 0>), grid, block, 0, stream(), g);
  } else {
    switch (act) {
      case 0: hipLaunchKernelGGL((gauss_kernel<OP, 0>), grid, block, 0, stream(), g); break;
      case 1: hipLaunchKernelGGL((gauss_kernel<OP, 1>), grid, block, 0, stream(), g); break;
      default: hipLaunchKernelGGL((gauss_kernel<OP, 2>), grid, block, 0, stream(), g); break;
    }
  }
  return launch_status();
}

// ---- logistic and softmax-distribution layers (src/layer.cc:579-602, src/loss_functions.cc:55-140; arithmetic of eigenmat.cc) ----------
// The stream skeleton of the element-wise entries: NI inputs, NO outputs of n floats, outputs may alias inputs (an element is read and
// written by the same lane).  When every pointer has the same offset within 16 bytes (a get_slice view of a matrix with an odd row
// count starts 4-byte aligned only) the `head` floats up to the first 16-byte boundary and the tail run scalar and the body as one
// 16-byte access per array; pointers that disagree run all scalar (head == n).
// (map2 above stays as it is — it serves every older entry and goes all scalar on such a view; it takes two inputs and one output, and
// these entries need the head, and a skeleton that extends to more arrays, without touching the kernels those entries were measured with.)
template <int NI, int NO, typename F>
struct StreamArgs {
  const float* in[NI];
  float* out[NO];
  size_t n, head;
  F f;   // void f(const float (&x)[NI], float (&y)[NO])
};
template <int NI, int NO, typename F>
__global__ void stream_kernel(const StreamArgs<NI, NO, F> a) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (a.n - a.head) >> 2;
  for (size_t i = tid; i < n4; i += stride) {
    f32x4 x[NI], y[NO];
#pragma unroll
    for (int k = 0; k < NI; ++k) x[k] = reinterpret_cast<const f32x4*>(a.in[k] + a.head)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xv[NI], yv[NO];
#pragma unroll
      for (int k = 0; k < NI; ++k) xv[k] = x[k][e];
      a.f(xv, yv);
#pragma unroll
      for (int k = 0; k < NO; ++k) y[k][e] = yv[k];
    }
#pragma unroll
    for (int k = 0; k < NO; ++k) reinterpret_cast<f32x4*>(a.out[k] + a.head)[i] = y[k];
  }
  const size_t rest = a.n - (n4 << 2);   // head + tail
  for (size_t r = tid; r < rest; r += stride) {
    const size_t i = r < a.head ? r : (n4 << 2) + r;
    float xv[NI], yv[NO];
#pragma unroll
    for (int k = 0; k < NI; ++k) xv[k] = a.in[k][i];
    a.f(xv, yv);
#pragma unroll
    for (int k = 0; k < NO; ++k) a.out[k][i] = yv[k];
  }
}
template <int NI, int NO, typename F>
int stream_launch(const char* name, const float* const (&in)[NI], float* const (&out)[NO], size_t n, F f) {
  if (n == 0) return 0;
  StreamArgs<NI, NO, F> a{{}, {}, n, 0, f};
  const uintptr_t off = reinterpret_cast<uintptr_t>(out[0]) & 15;
  bool same = (off & 3) == 0;
  for (int k = 0; k < NI; ++k) { a.in[k] = in[k]; same = same && (reinterpret_cast<uintptr_t>(in[k]) & 15) == off; }
  for (int k = 0; k < NO; ++k) { a.out[k] = out[k]; same = same && (reinterpret_cast<uintptr_t>(out[k]) & 15) == off; }
  a.head = same ? ((16 - off) & 15) >> 2 : n;
  if (a.head > n) a.head = n;
  KernelTimer timer(name, "logistic", 0.0, 4.0 * n * (NI + NO));
  hipLaunchKernelGGL((stream_kernel<NI, NO, F>), dim3(blocks_for(n / 4 + 1)), dim3(kThreads), 0, stream(), a);
  return launch_status();
}

// One case per matrix ROW, as in the softmax kernels above: a block owns 32 consecutive rows and G column groups; lane (r, g) walks
// columns g, g + G, ... of row r (coalesced over the 32 rows), the groups of a row are combined in LDS in group order.
//  * get_logistic_correct_normalized (eigenmat.cc:1344-1373): share[row] = #{t >= 0 and (p >= 0.5) == (t >= 0.5)} / #{t >= 0}, 0 when
//    nothing counts.  Both counts are integers below 2^24, so any summation order gives the reference's fp32 loop exactly.
//  * FUSED: mat holds logits; p = sigmoid into probs (may alias mat), deriv = (t < 0 ? 0 : p - t) * deriv_scale, and the block's sum of
//    its rows' shares (row order) goes to part[blockIdx.x] for accum_finish_kernel.
template <int G, bool FUSED>
__global__ void __launch_bounds__(G * 32) logistic_rows_kernel(const float* mat, const float* __restrict__ targets, float* probs, float* __restrict__ deriv,
                                                                float* __restrict__ out, int rows, int cols, float deriv_scale) {
  __shared__ float rc[G][33], rt[G][33];
  const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int row = blockIdx.x * 32 + r;
  float correct = 0.f, total = 0.f;
  if (row < rows)
    for (int j = g; j < cols; j += G) {
      const size_t x = (size_t)j * rows + row;
      const float t = targets[x];
      float p = mat[x];
      if (FUSED) {
        p = sigmoid1(p);
        probs[x] = p;
        const float d = t < 0.f ? 0.f : p - t;
        deriv[x] = d * deriv_scale;
      }
      if (!(t < 0.f)) {
        total += 1.f;
        correct += ((t >= 0.5f && p >= 0.5f) || (t < 0.5f && p < 0.5f)) ? 1.f : 0.f;
      }
    }
  rc[g][r] = correct;
  rt[g][r] = total;
  __syncthreads();
  float share = 0.f;
  if (g == 0) {
#pragma unroll
    for (int k = 1; k < G; ++k) {
      correct += rc[k][r];
      total += rt[k][r];
    }
    share = total > 0.f ? correct / total : 0.f;
  }
  if (!FUSED) {
    if (g == 0 && row < rows) out[row] = share;
    return;
  }
  if (g == 0) rc[0][r] = row < rows ? share : 0.f;   // (lane (r, 0) alone has read column r of rc)
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < 32; ++k) s += rc[0][k];
    out[blockIdx.x] = s;
  }
}

// softmax_rows_kernel's three passes (same maxima, same exponentials, same order of the row sums: bit-identical probabilities) with a
// target DISTRIBUTION per row: deriv = (p - t) * deriv_scale, and the block's sum of -t * log(p + tiny) to part[blockIdx.x]
// (per lane in column order, lanes of a row in group order, rows in row order).
template <int G>
__global__ void __launch_bounds__(G * 32) softmax_dist_rows_kernel(const float* logits, const float* __restrict__ targets, float* probs, float* __restrict__ deriv,
                                                                    float* __restrict__ part, int rows, int cols, float deriv_scale, float tiny) {
  __shared__ float red[G][33];
  const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int row = blockIdx.x * 32 + r;
  const bool ok = row < rows;
  float mx = -FLT_MAX;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const float v = logits[(size_t)j * rows + row];
      if (v > mx) mx = v;
    }
  red[g][r] = mx;
  __syncthreads();
  mx = red[0][r];
#pragma unroll
  for (int k = 1; k < G; ++k) {
    const float v = red[k][r];
    if (v > mx) mx = v;
  }
  __syncthreads();
  float s = 0.f;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const size_t x = (size_t)j * rows + row;
      const float e = expf(logits[x] - mx);
      probs[x] = e;
      s += e;
    }
  red[g][r] = s;
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) s += red[k][r];
  __syncthreads();
  float ce = 0.f;
  if (ok)
    for (int j = g; j < cols; j += G) {
      const size_t x = (size_t)j * rows + row;
      const float pr = probs[x] / s;
      const float t = targets[x];
      probs[x] = pr;
      const float d = pr - t;
      deriv[x] = d * deriv_scale;
      ce += -t * logf(pr + tiny);
    }
  red[g][r] = ce;
  __syncthreads();
  if (g == 0) {
    ce = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) ce += red[k][r];
    red[0][r] = ce;   // (lane (r, 0) alone has read column r of red)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < 32; ++k) t += red[0][k];
    part[blockIdx.x] = t;
  }
}

// accum[0] += sum of part[0 .. n) in a fixed order: one block, no atomics — the same bits from call to call
__global__ void accum_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ accum) {
  __shared__ float sh[8];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) accum[0] += s;
}

// One fused pass of SGDOptimizer::Optimize.  Explicit __fmul_rn/__fadd_rn keep each reference
// statement a separately rounded fp32 op (no fma contraction), so the update is bit-identical
// to the reference's multi-pass sequence.
__device__ __forceinline__ void sgd_one(float& g, float& w, float& h, float l2, float clip, float eps, float mom) {
  // hipcc defaults to -ffp-contract=fast, and __fmul_rn/__fadd_rn are header functions compiled
  // under that default (they still fuse).  Plain operators under contract(off) do not.
#pragma clang fp contract(off)
  if (l2 > 0.f) {
    const float t = w * l2;
    g = g + t;
  }
  if (clip > 0.f) g = g > clip ? clip : (g < -clip ? -clip : g);
  g = g * eps;
  const float hm = h * mom;
  h = hm + g;
  w = w - h;
}

// The two second-moment optimizers of src/optimizer.cc:202-279, one fused pass each, under the same rule as sgd_one: every reference
// statement is one separately rounded fp32 operation.  sqrtf and / are the correctly rounded ones (hipcc's default for fp32).
//   adagrad_one: AdagradSGDOptimizer::Optimize — a = delta + sqrt((a - delta)^2 + g^2); g /= a; g *= sqrt(step + 1); then sgd_one.
//   rmsprop_one: RMSPropSGDOptimizer::Optimize — h *= mom; L2; clip; a = sqrt(factor*a*a + (1 - factor)*g*g) left to right with
//                1 - factor formed in float; g /= a; h += eps*g; w -= h.
__device__ __forceinline__ void adagrad_one(float& g, float& w, float& h, float& a, float delta, float step_scale, float l2, float clip, float eps,
                                            float mom) {
#pragma clang fp contract(off)
  const float c = a - delta;
  const float cc = c * c;
  const float gg = g * g;
  const float s = cc + gg;
  a = delta + sqrtf(s);
  g = g / a;
  g = g * step_scale;
  sgd_one(g, w, h, l2, clip, eps, mom);
}
__device__ __forceinline__ void rmsprop_one(float& g, float& w, float& h, float& a, float factor, float l2, float clip, float eps, float mom) {
#pragma clang fp contract(off)
  h = h * mom;
  if (l2 > 0.f) {
    const float t = w * l2;
    g = g + t;
  }
  if (clip > 0.f) g = g > clip ? clip : (g < -clip ? -clip : g);
  const float fa = factor * a;
  const float faa = fa * a;
  const float omf = 1.f - factor;
  const float og = omf * g;
  const float ogg = og * g;
  const float s = faa + ogg;
  a = sqrtf(s);
  g = g / a;
  const float eg = eps * g;
  h = h + eg;
  w = w - h;
}

// An optimizer step as data: the hyper-parameters of one tensor and the per-element update over its N arrays (gradient, parameter,
// momentum history[, second-moment history]), every one of them read and written back.
struct SgdOp {
  static constexpr int N = 3;
  static constexpr bool kRefuseHuge = false;
  float l2, clip, eps, mom;
  __device__ __forceinline__ void operator()(float (&v)[N]) const { sgd_one(v[0], v[1], v[2], l2, clip, eps, mom); }
};
struct AdagradOp {
  static constexpr int N = 4;
  static constexpr bool kRefuseHuge = true;   // more than INT_MAX floats: ERROR_UNSUPPORTED, like the batch-norm entries
  float delta, step_scale, l2, clip, eps, mom;
  __device__ __forceinline__ void operator()(float (&v)[N]) const { adagrad_one(v[0], v[1], v[2], v[3], delta, step_scale, l2, clip, eps, mom); }
};
struct RmsPropOp {
  static constexpr int N = 4;
  static constexpr bool kRefuseHuge = true;
  float factor, l2, clip, eps, mom;
  __device__ __forceinline__ void operator()(float (&v)[N]) const { rmsprop_one(v[0], v[1], v[2], v[3], factor, l2, clip, eps, mom); }
};
// One tensor of a step.  The arrays never overlap (slices of different flat buffers).
template <typename Op>
struct StepItem {
  float* p[Op::N];
  unsigned long long n;
  Op op;
  int vec;   // every array 16-byte aligned
};
// The stream skeleton every fused step shares: grid-stride over 16-byte accesses when the pointers allow it, scalar tail (or all scalar).
template <typename Op>
__device__ __forceinline__ void step_range(const StepItem<Op>& t, size_t tid, size_t stride) {
  constexpr int N = Op::N;
  const size_t n = (size_t)t.n;
  size_t done = 0;
  if (t.vec) {
    const size_t n4 = n >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      f32x4 x[N];
#pragma unroll
      for (int k = 0; k < N; ++k) x[k] = reinterpret_cast<const f32x4*>(t.p[k])[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = x[k][e];
        t.op(v);
#pragma unroll
        for (int k = 0; k < N; ++k) x[k][e] = v[k];
      }
#pragma unroll
      for (int k = 0; k < N; ++k) reinterpret_cast<f32x4*>(t.p[k])[i] = x[k];
    }
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = t.p[k][i];
    t.op(v);
#pragma unroll
    for (int k = 0; k < N; ++k) t.p[k][i] = v[k];
  }
}
// Several tensors in ONE launch (the *_multi entries): AlexNet's step updates 13 small tensors (the convolution banks and every bias) with
// ~7 us launches of a few MB each; blockIdx.y picks the tensor, every tensor with its own hyper-parameters.  Same per-element update:
// bit-identical to one single-tensor call per tensor.
constexpr int kSgdMulti = 16;
template <typename Op>
struct StepBatch {
  StepItem<Op> it[kSgdMulti];
};
template <typename Op>
__device__ __forceinline__ void step_single(const StepItem<Op>& t) {
  step_range(t, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}
__global__ void sgd_kernel(const StepItem<SgdOp> t) { step_single(t); }
__global__ void adagrad_kernel(const StepItem<AdagradOp> t) { step_single(t); }
__global__ void rmsprop_kernel(const StepItem<RmsPropOp> t) { step_single(t); }
__global__ void sgd_multi_kernel(const StepBatch<SgdOp> b) { step_single(b.it[blockIdx.y]); }
__global__ void adagrad_multi_kernel(const StepBatch<AdagradOp> b) { step_single(b.it[blockIdx.y]); }
__global__ void rmsprop_multi_kernel(const StepBatch<RmsPropOp> b) { step_single(b.it[blockIdx.y]); }

// Host side of the skeleton.  `mats`: the N cudamats of one tensor in the order of StepItem::p, the parameter second.
template <typename Op>
int step_check(cudamat* const (&mats)[Op::N]) {
  const size_t n = numel(mats[1]);
  for (cudamat* m : mats)
    if (!m->on_device) return ERROR_NOT_ON_DEVICE;
  for (cudamat* m : mats)
    if (numel(m) != n) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (Op::kRefuseHuge && n > (size_t)INT_MAX) return ERROR_UNSUPPORTED;
  return 0;
}
template <typename Op>
StepItem<Op> step_item(cudamat* const (&mats)[Op::N], const Op& op) {
  StepItem<Op> t{};
  t.vec = 1;
  for (int k = 0; k < Op::N; ++k) {
    t.p[k] = mats[k]->data_device;
    t.vec &= aligned16(t.p[k]) ? 1 : 0;
  }
  t.n = numel(mats[1]);
  t.op = op;
  return t;
}
// bytes per element for KernelTimer: every array read, every array but the gradient written (what the step needs; the gradient's
// write-back keeps fused and unfused training comparable tensor for tensor and is not counted, as in sgd_kernel's 20 bytes)
template <typename Op>
constexpr double step_bytes() { return 4.0 * (2 * Op::N - 1); }

template <typename Op, typename K>
int step_launch(K kernel, const char* name, const char* family, cudamat* const (&mats)[Op::N], const Op& op) {
  if (int rc = step_check<Op>(mats)) return rc;
  const size_t n = numel(mats[1]);
  if (n == 0) return 0;
  KernelTimer timer(name, family, 0.0, step_bytes<Op>() * n);
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n / 4 + 1)), dim3(kThreads), 0, stream(), step_item<Op>(mats, op));
  return launch_status();
}
// `count` tensors in ceil(count / 16) launches; tensor(i, mats, op) fills in tensor i
template <typename Op, typename K, typename F>
int step_launch_multi(K kernel, const char* name, const char* family, int count, F tensor) {
  cudamat* mats[Op::N];
  Op op;
  for (int i = 0; i < count; ++i) {
    tensor(i, mats, op);
    if (int rc = step_check<Op>(mats)) return rc;
  }
  for (int base = 0; base < count; base += kSgdMulti) {
    StepBatch<Op> b{};
    int m = 0;
    size_t most = 0, total = 0;
    for (int i = base; i < count && i < base + kSgdMulti; ++i) {
      tensor(i, mats, op);
      const size_t n = numel(mats[1]);
      if (n == 0) continue;
      b.it[m++] = step_item<Op>(mats, op);
      most = n > most ? n : most;
      total += n;
    }
    if (m == 0) continue;
    KernelTimer timer(name, family, 0.0, step_bytes<Op>() * total);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(most / 4 + 1), m), dim3(kThreads), 0, stream(), b);
  }
  return launch_status();
}

}  // namespace chip

using namespace chip;

extern "C" {

// ---- deferred epilogues (common.h: PendingOp): does this element-wise call continue the parked one? ---------------------------------
namespace {
inline bool same_mat(const cudamat* a, const cudamat& b) { return a->on_device && a->data_device == b.data_device && numel(a) == numel(&b); }
// add_row_vec(T viewed as (N*M, F), bias(1, F), T) behind convUp(..., T): the shared bias of src/conv_edge.cc:145-148
bool absorb_bias(cudamat* mat, cudamat* vec, cudamat* target) {
  PendingOp& o = pending();
  if (o.kind != 1 || o.has_bias || o.relu) return false;   // (mat and target are both checked against the parked call's target below)
  const int F = o.desc.num_output_channels;
  if (!same_mat(mat, o.m[2]) || !same_mat(target, o.m[2]) || mat->is_trans || !vec->on_device || (int)numel(vec) != F || mat->size[1] != F) return false;
  o.bias = *vec;
  o.has_bias = 1;
  ++g_absorbed;
  return true;
}
// lower_bound_scalar(T, 0, T) behind convUp(..., T) [+ bias] or ResponseNormCrossMap(..., T): the ReLU of src/layer.cc:549-551
bool absorb_relu(cudamat* mat, float val, cudamat* target) {
  PendingOp& o = pending();
  if ((o.kind != 1 && o.kind != 4) || o.relu || val != 0.f) return false;
  const cudamat& t = o.kind == 1 ? o.m[2] : o.m[1];
  if (!same_mat(mat, t) || !same_mat(target, t)) return false;
  o.relu = 1;
  flush_pending();   // nothing more can join
  ++g_absorbed;
  return true;
}
// apply_rectified_linear_deriv(D, S, D) behind convDown(..., D) or MaxPoolUndo(images = S, ..., D): the ReLU' of src/layer.cc:556-558
bool absorb_relu_deriv(cudamat* deriv, cudamat* state, cudamat* target) {
  PendingOp& o = pending();
  if ((o.kind != 2 && o.kind != 3) || o.has_mask || !state->on_device || numel(state) != numel(deriv)) return false;
  const cudamat& t = o.kind == 2 ? o.m[2] : o.m[3];
  if (!same_mat(deriv, t) || !same_mat(target, t)) return false;
  if (o.kind == 3 && !same_mat(state, o.m[0])) return false;   // the pooling kernel masks with its own input
  o.mask = *state;
  o.has_mask = 1;
  flush_pending();
  ++g_absorbed;
  return true;
}
}  // namespace

int add_row_vec(cudamat* mat, cudamat* vec, cudamat* target) {
  if (absorb_bias(mat, vec, target)) return 0;
  return add_row(mat, vec, target, 1.0f);
}
int add_row_mult(cudamat* mat, cudamat* vec, cudamat* target, float mult) { return add_row(mat, vec, target, mult); }

int sum_by_axis(cudamat* mat, cudamat* target, int axis, float mult, float p) { return axis_sum<false>(mat, target, axis, mult, p); }
int sqsum_by_axis(cudamat* mat, cudamat* target, int axis, float mult, float p) { return axis_sum<true>(mat, target, axis, mult, p); }

float sum_all(cudamat* mat, int* err_code) { return reduce_all<0>(mat, nullptr, err_code); }
float vdot(cudamat* mat1, cudamat* mat2, int* err_code) {
  if (numel(mat1) != numel(mat2)) { *err_code = ERROR_INCOMPATIBLE_DIMENSIONS; return 0.f; }
  return reduce_all<1>(mat1, mat2, err_code);
}
float euclid_norm(cudamat* mat, int* err_code) { return sqrtf(reduce_all<2>(mat, nullptr, err_code)); }

int normlimit_by_axis(cudamat* mat, cudamat* target, int axis, float norm, int constraint) {
  if (!mat->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (mat->size[0] != target->size[0] || mat->size[1] != target->size[1]) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int rows = mat->size[0], cols = mat->size[1];
  if (axis == 0)
    hipLaunchKernelGGL(normlimit_cols_kernel, dim3(cols), dim3(256), 0, stream(), mat->data_device, target->data_device, rows, norm, constraint);
  else
    return rows_normlimit(nullptr, mat->data_device, target->data_device, nullptr, rows, cols, norm, constraint, false, 0.f, 0.f, 0.f, 0.f);
  return launch_status();
}

// SGDOptimizer::Optimize + ApplyConstraints (src/optimizer.cc:174-200,75-81) for one (rows x cols) tensor:
// the update pass also produces the per-row norms the constraint needs.
int sgd_momentum_step_normlimit(cudamat* grad, cudamat* param, cudamat* history, float l2_decay, float gradient_clip, float epsilon,
                                float momentum, float norm, int constraint) {
  const size_t n = numel(param);
  if (!grad->on_device || !param->on_device || !history->on_device) return ERROR_NOT_ON_DEVICE;
  if (numel(grad) != n || numel(history) != n) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (param->is_trans) return ERROR_TRANSPOSED;
  if (n == 0) return 0;
  return rows_normlimit(grad->data_device, param->data_device, param->data_device, history->data_device, param->size[0], param->size[1], norm,
                        constraint, true, l2_decay, gradient_clip, epsilon, momentum);
}

int lower_bound_scalar(cudamat* mat, float val, cudamat* target) {
  if (absorb_relu(mat, val, target)) return 0;
  return map2(target, mat, nullptr, [val] __device__(float x, float) { return x > val ? x : val; });
}
int upper_bound_mod_scalar(cudamat* mat, float val, cudamat* target) {
  return map2(target, mat, nullptr, [val] __device__(float x, float) { return x > val ? val : (x < -val ? -val : x); });
}
int apply_rectified_linear_deriv(cudamat* mat1, cudamat* mat2, cudamat* target) {
  if (absorb_relu_deriv(mat1, mat2, target)) return 0;
  return map2(target, mat1, mat2, [] __device__(float d, float s) { return s > 0.f ? d : 0.f * d; });
}
int assign_scalar(cudamat* mat, float alpha) {
  return map2(mat, mat, nullptr, [alpha] __device__(float, float) { return alpha; });
}
int add_scalar(cudamat* mat, float alpha, cudamat* target) {
  return map2(target, mat, nullptr, [alpha] __device__(float x, float) { return x + alpha; });
}
int mult_by_scalar(cudamat* mat, float alpha, cudamat* target, float scale_targets) {
  if (scale_targets == 0.f) return map2(target, mat, nullptr, [alpha] __device__(float x, float) { return x * alpha; });
  return map2(target, mat, target, [alpha, scale_targets] __device__(float x, float t) { return scale_targets * t + x * alpha; });
}
int divide_by_scalar(cudamat* mat, float alpha, cudamat* target) {
  return map2(target, mat, nullptr, [alpha] __device__(float x, float) { return x / alpha; });
}
int add_mult(cudamat* mat1, cudamat* mat2, float alpha) {
  // Matrix::Add(m, alpha) is one statement of the optimizers' unfused sequences (g += l2*w, h += epsilon*g): product rounded, then the
  // sum, as the reference's CPU build computes it and as sgd_one / adagrad_one / rmsprop_one do, so fused and unfused steps are equal
  // bit for bit.  (With alpha = 1 or -1, every other use in the hosts but the batch-norm running averages, an fma gives the same.)
  return map2(mat1, mat1, mat2, [alpha] __device__(float x, float y) {
#pragma clang fp contract(off)
    const float t = alpha * y;
    return x + t;
  });
}
int add_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target) {
  return map2(target, mat1, mat2, [] __device__(float x, float y) { return x + y; });
}
int subtract_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target) {
  return map2(target, mat1, mat2, [] __device__(float x, float y) { return x - y; });
}
int mult_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target, float scale_targets) {
  if (scale_targets != 0.f) return ERROR_UNSUPPORTED;
  return map2(target, mat1, mat2, [] __device__(float x, float y) { return x * y; });
}
int apply_sqrt(cudamat* mat, cudamat* target) {
  return map2(target, mat, nullptr, [] __device__(float x, float) { return sqrtf(x); });
}

int softmax_row_major_multi(cudamat* mat, int numslices, cudamat* target) {
  if (!mat->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  const size_t len = numel(mat);
  if (numslices <= 0 || len % numslices != 0 || numel(target) != len) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int rows = (int)(len / numslices), cols = numslices;
  SoftmaxOut o{target->data_device, nullptr, nullptr};
  hipLaunchKernelGGL(softmax_rows_kernel<32>, dim3(divup(rows, 32)), dim3(1024), 0, stream(), mat->data_device, nullptr, o, rows, cols, 1.0f);
  return launch_status();
}
int softmax_row_major(cudamat* mat, cudamat* target) { return softmax_row_major_multi(mat, mat->size[1], target); }

int apply_softmax_grad_row_major(cudamat* mat, cudamat* labels, cudamat* target) {
  if (!mat->on_device || !labels->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (numel(labels) != (size_t)mat->size[0] || numel(target) != numel(mat)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (target->data_device != mat->data_device) {
    int rc = copy_on_device(mat, target);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(softmax_grad_kernel, dim3(divup(mat->size[0], 256)), dim3(256), 0, stream(), labels->data_device, target->data_device, mat->size[0]);
  return launch_status();
}

int get_softmax_correct_row_major(cudamat* mat, cudamat* labels, cudamat* target) {
  if (!mat->on_device || !labels->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (target->size[0] != mat->size[0] || target->size[1] != 1 || numel(labels) != (size_t)mat->size[0]) return ERROR_INCOMPATIBLE_DIMENSIONS;
  hipLaunchKernelGGL(softmax_correct_kernel, dim3(divup(mat->size[0], 32)), dim3(1024), 0, stream(), mat->data_device, labels->data_device,
                     target->data_device, mat->size[0], mat->size[1]);
  return launch_status();
}

int get_softmax_cross_entropy_row_major(cudamat* mat, cudamat* labels, cudamat* target, float tiny) {
  if (!mat->on_device || !labels->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (target->size[0] != mat->size[0] || target->size[1] != 1 || labels->size[0] != mat->size[0] || labels->size[1] != 1)
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  hipLaunchKernelGGL(softmax_ce_kernel, dim3(divup(mat->size[0], 256)), dim3(256), 0, stream(), mat->data_device, labels->data_device,
                     target->data_device, mat->size[0], tiny);
  return launch_status();
}

int softmax_ce_grad_correct(cudamat* logits, cudamat* labels, cudamat* probs, cudamat* deriv, cudamat* correct_accum, float deriv_scale) {
  if (!logits->on_device || !labels->on_device || !probs->on_device) return ERROR_NOT_ON_DEVICE;
  if (numel(probs) != numel(logits) || (deriv && numel(deriv) != numel(logits)) || numel(labels) != (size_t)logits->size[0])
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  SoftmaxOut o{probs->data_device, deriv ? deriv->data_device : nullptr, correct_accum ? correct_accum->data_device : nullptr};
  KernelTimer timer("softmax_rows_kernel", "softmax_ce", 0.0, 4.0 * numel(logits) * (deriv ? 3 : 2));
  hipLaunchKernelGGL(softmax_rows_kernel<32>, dim3(divup(logits->size[0], 32)), dim3(1024), 0, stream(), logits->data_device, labels->data_device, o,
                     logits->size[0], logits->size[1], deriv_scale);
  return launch_status();
}

// g += l2*w; clip; g *= eps; h = mom*h + g; w -= h   (src/optimizer.cc:174-200, one pass, same op order)
int sgd_momentum_step(cudamat* grad, cudamat* param, cudamat* history, float l2_decay, float gradient_clip, float epsilon, float momentum) {
  cudamat* const mats[] = {grad, param, history};
  // reads g, w, h; writes h, w (>= 20 bytes per parameter)
  return step_launch<SgdOp>(sgd_kernel, "sgd_kernel", "sgd", mats, SgdOp{l2_decay, gradient_clip, epsilon, momentum});
}

// sgd_momentum_step on `count` tensors, each with its own hyper-parameters, in ceil(count / 16) launches
int sgd_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, const float* l2_decay, const float* gradient_clip,
                            const float* epsilon, const float* momentum) {
  if (count < 0 || (count > 0 && (!grads || !params || !histories || !l2_decay || !gradient_clip || !epsilon || !momentum))) return ERROR_GENERIC;
  return step_launch_multi<SgdOp>(sgd_multi_kernel, "sgd_multi_kernel", "sgd", count, [&](int i, cudamat* (&m)[3], SgdOp& op) {
    m[0] = grads[i]; m[1] = params[i]; m[2] = histories[i];
    op = SgdOp{l2_decay[i], gradient_clip[i], epsilon[i], momentum[i]};
  });
}

// ---- Adagrad and RMSProp (src/optimizer.cc:202-279): the reference's three entries and the fused steps ------------------------------------
namespace {
// cudamat's checks for adagrad / rms_prop / divide_elementwise (cudamat.cu:2302-2314, 3326-3337): transposedness, then element count
int second_moment_check(const cudamat* a, const cudamat* b, const cudamat* c) {
  if (!a->on_device || !b->on_device || (c && !c->on_device)) return ERROR_NOT_ON_DEVICE;
  if (a->is_trans != b->is_trans) return ERROR_TRANSPOSEDNESS;
  if (numel(a) != numel(b) || (c && numel(a) != numel(c))) return ERROR_INCOMPATIBLE_DIMENSIONS;
  return 0;
}
}  // namespace

int adagrad(cudamat* history, cudamat* grad, float delta) {
  if (int rc = second_moment_check(history, grad, nullptr)) return rc;
  return map2(history, history, grad, [delta] __device__(float h, float g) {
#pragma clang fp contract(off)
    const float c = h - delta;
    const float cc = c * c;
    const float gg = g * g;
    const float s = cc + gg;
    return delta + sqrtf(s);
  });
}
int rms_prop(cudamat* history, cudamat* grad, float factor) {
  if (int rc = second_moment_check(history, grad, nullptr)) return rc;
  return map2(history, history, grad, [factor] __device__(float h, float g) {
#pragma clang fp contract(off)
    const float fh = factor * h;
    const float fhh = fh * h;
    const float omf = 1.f - factor;
    const float og = omf * g;
    const float ogg = og * g;
    const float s = fhh + ogg;
    return sqrtf(s);
  });
}
int divide_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target) {
  if (int rc = second_moment_check(mat1, mat2, target)) return rc;
  return map2(target, mat1, mat2, [] __device__(float x, float y) { return x / y; });
}

// AdagradSGDOptimizer::Optimize (src/optimizer.cc:226-231, then :174-200, non-Nesterov) in one pass; step_scale = (float)sqrt(step + 1)
int adagrad_momentum_step(cudamat* grad, cudamat* param, cudamat* history, cudamat* adagrad_history, float delta, float step_scale, float l2_decay,
                          float gradient_clip, float epsilon, float momentum) {
  cudamat* const mats[] = {grad, param, history, adagrad_history};
  // reads g, w, h, a; writes h, a, w
  return step_launch<AdagradOp>(adagrad_kernel, "adagrad_kernel", "adagrad", mats,
                                AdagradOp{delta, step_scale, l2_decay, gradient_clip, epsilon, momentum});
}
// RMSPropSGDOptimizer::Optimize (src/optimizer.cc:257-279) in one pass
int rmsprop_momentum_step(cudamat* grad, cudamat* param, cudamat* history, cudamat* rms_history, float factor, float l2_decay, float gradient_clip,
                          float epsilon, float momentum) {
  cudamat* const mats[] = {grad, param, history, rms_history};
  return step_launch<RmsPropOp>(rmsprop_kernel, "rmsprop_kernel", "rmsprop", mats, RmsPropOp{factor, l2_decay, gradient_clip, epsilon, momentum});
}
int adagrad_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, cudamat** adagrad_histories, const float* delta,
                                const float* step_scale, const float* l2_decay, const float* gradient_clip, const float* epsilon,
                                const float* momentum) {
  if (count < 0 || (count > 0 && (!grads || !params || !histories || !adagrad_histories || !delta || !step_scale || !l2_decay || !gradient_clip ||
                                  !epsilon || !momentum)))
    return ERROR_GENERIC;
  return step_launch_multi<AdagradOp>(adagrad_multi_kernel, "adagrad_multi_kernel", "adagrad", count, [&](int i, cudamat* (&m)[4], AdagradOp& op) {
    m[0] = grads[i]; m[1] = params[i]; m[2] = histories[i]; m[3] = adagrad_histories[i];
    op = AdagradOp{delta[i], step_scale[i], l2_decay[i], gradient_clip[i], epsilon[i], momentum[i]};
  });
}
int rmsprop_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, cudamat** rms_histories, const float* factor,
                                const float* l2_decay, const float* gradient_clip, const float* epsilon, const float* momentum) {
  if (count < 0 || (count > 0 && (!grads || !params || !histories || !rms_histories || !factor || !l2_decay || !gradient_clip || !epsilon || !momentum)))
    return ERROR_GENERIC;
  return step_launch_multi<RmsPropOp>(rmsprop_multi_kernel, "rmsprop_multi_kernel", "rmsprop", count, [&](int i, cudamat* (&m)[4], RmsPropOp& op) {
    m[0] = grads[i]; m[1] = params[i]; m[2] = histories[i]; m[3] = rms_histories[i];
    op = RmsPropOp{factor[i], l2_decay[i], gradient_clip[i], epsilon[i], momentum[i]};
  });
}

// ---- logistic and softmax-distribution layers: cudamat.cuh:204,216,233,252,289 and the fused entries (include/convnet_hip.h) -----------
namespace {
// cudamat's checks (cudamat.cu:2385-2452): on device, then transposedness, then the exact sizes
int same_shape_check(const cudamat* a, const cudamat* b, const cudamat* c) {
  if (!a->on_device || !b->on_device || (c && !c->on_device)) return ERROR_NOT_ON_DEVICE;
  if (a->is_trans != b->is_trans) return ERROR_TRANSPOSEDNESS;
  if (a->size[0] != b->size[0] || a->size[1] != b->size[1] || (c && (a->size[0] != c->size[0] || a->size[1] != c->size[1])))
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  return 0;
}
inline bool is_1x1(const cudamat* m) { return m->size[0] == 1 && m->size[1] == 1; }
}  // namespace

int apply_sigmoid(cudamat* mat, cudamat* target) {
  if (int rc = same_shape_check(mat, target, nullptr)) return rc;
  const float* const in[] = {mat->data_device};
  float* const out[] = {target->data_device};
  return stream_launch("stream_kernel<sigmoid>", in, out, numel(mat), [] __device__(const float (&x)[1], float (&y)[1]) { y[0] = sigmoid1(x[0]); });
}
int apply_logistic_deriv(cudamat* mat1, cudamat* mat2, cudamat* target) {
  if (int rc = same_shape_check(mat1, mat2, target)) return rc;
  const float* const in[] = {mat1->data_device, mat2->data_device};
  float* const out[] = {target->data_device};
  return stream_launch("stream_kernel<logistic_deriv>", in, out, numel(mat1), [] __device__(const float (&x)[2], float (&y)[1]) {
#pragma clang fp contract(off)
    const float dy = x[0] * x[1];
    const float om = 1.0f - x[1];
    y[0] = dy * om;
  });
}
int apply_logistic_grad(cudamat* mat1, cudamat* mat2, cudamat* out_grad) {
  if (int rc = same_shape_check(mat1, mat2, out_grad)) return rc;
  const float* const in[] = {mat1->data_device, mat2->data_device};
  float* const out[] = {out_grad->data_device};
  return stream_launch("stream_kernel<logistic_grad>", in, out, numel(mat1),
                       [] __device__(const float (&x)[2], float (&y)[1]) { y[0] = x[1] < 0.f ? 0.f : x[0] - x[1]; });
}
int get_logistic_correct_normalized(cudamat* mat1, cudamat* mat2, cudamat* out) {
  if (!mat1->on_device || !mat2->on_device || !out->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat1->is_trans != mat2->is_trans) return ERROR_TRANSPOSEDNESS;
  if (mat1->size[0] != mat2->size[0] || mat1->size[1] != mat2->size[1] || mat1->size[0] != out->size[0] || out->size[1] != 1)
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int rows = mat1->size[0], cols = mat1->size[1];
  if (rows == 0) return 0;
  KernelTimer timer("logistic_rows_kernel", "logistic", 0.0, 4.0 * ((double)rows * cols * 2 + rows));
  hipLaunchKernelGGL((logistic_rows_kernel<32, false>), dim3(divup(rows, 32)), dim3(1024), 0, stream(), mat1->data_device, mat2->data_device, nullptr,
                     nullptr, out->data_device, rows, cols, 1.0f);
  return launch_status();
}
int compute_cross_entropy(cudamat* mat, cudamat* pow, cudamat* target, float tiny) {
  if (int rc = same_shape_check(mat, pow, target)) return rc;
  const float* const in[] = {mat->data_device, pow->data_device};
  float* const out[] = {target->data_device};
  return stream_launch("stream_kernel<cross_entropy>", in, out, numel(mat),
                       [tiny] __device__(const float (&x)[2], float (&y)[1]) { y[0] = -x[0] * logf(x[1] + tiny); });
}

int logistic_dropout(rnd_struct* st, cudamat* mat, float dropprob, float scale) {
  if (!mat->on_device) return ERROR_NOT_ON_DEVICE;
  return rng_launch<5>(st, mat->data_device, mat->data_device, numel(mat), dropprob, 0.f, scale);
}
int logistic_deriv_scaled(cudamat* deriv, cudamat* state, float scale) {
  if (int rc = same_shape_check(deriv, state, nullptr)) return rc;
  const float* const in[] = {deriv->data_device, state->data_device};
  float* const out[] = {deriv->data_device};
  return stream_launch("stream_kernel<logistic_deriv_scaled>", in, out, numel(deriv), [scale] __device__(const float (&x)[2], float (&y)[1]) {
#pragma clang fp contract(off)
    const float d = scale == 1.0f ? x[0] : x[0] * scale;
    const float dy = d * x[1];
    const float om = 1.0f - x[1];
    y[0] = dy * om;
  });
}
int logistic_ce_grad_correct(cudamat* logits, cudamat* targets, cudamat* probs, cudamat* deriv, cudamat* correct_accum, float deriv_scale) {
  if (!correct_accum->on_device) return ERROR_NOT_ON_DEVICE;
  if (int rc = same_shape_check(logits, targets, probs)) return rc;
  if (int rc = same_shape_check(logits, targets, deriv)) return rc;
  if (!is_1x1(correct_accum)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int rows = logits->size[0], cols = logits->size[1];
  if (rows == 0) return 0;
  const int nb = divup(rows, 32);
  float* part = static_cast<float*>(workspace(sizeof(float) * nb));
  // reads logits and targets, writes probs and deriv
  KernelTimer timer("logistic_rows_kernel<fused>", "logistic_ce", 0.0, 4.0 * (double)rows * cols * 4);
  hipLaunchKernelGGL((logistic_rows_kernel<32, true>), dim3(nb), dim3(1024), 0, stream(), logits->data_device, targets->data_device, probs->data_device,
                     deriv->data_device, part, rows, cols, deriv_scale);
  hipLaunchKernelGGL(accum_finish_kernel, dim3(1), dim3(256), 0, stream(), part, nb, correct_accum->data_device);
  return launch_status();
}
int softmax_dist_ce_grad(cudamat* logits, cudamat* targets, cudamat* probs, cudamat* deriv, cudamat* ce_accum, float deriv_scale, float tiny) {
  if (!ce_accum->on_device) return ERROR_NOT_ON_DEVICE;
  if (int rc = same_shape_check(logits, targets, probs)) return rc;
  if (int rc = same_shape_check(logits, targets, deriv)) return rc;
  if (!is_1x1(ce_accum)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int rows = logits->size[0], cols = logits->size[1];
  if (rows == 0) return 0;
  const int nb = divup(rows, 32);
  float* part = static_cast<float*>(workspace(sizeof(float) * nb));
  // reads logits twice, probs once and targets; writes probs twice and deriv
  KernelTimer timer("softmax_dist_rows_kernel", "softmax_dist_ce", 0.0, 4.0 * (double)rows * cols * 7);
  hipLaunchKernelGGL(softmax_dist_rows_kernel<32>, dim3(nb), dim3(1024), 0, stream(), logits->data_device, targets->data_device, probs->data_device,
                     deriv->data_device, part, rows, cols, deriv_scale, tiny);
  hipLaunchKernelGGL(accum_finish_kernel, dim3(1), dim3(256), 0, stream(), part, nb, ce_accum->data_device);
  return launch_status();
}

int init_random(rnd_struct* rnd_state, int seed) {
  RngHost* h = new RngHost{(unsigned long long)(unsigned)seed, 0ull};
  rnd_state->dev_mults = nullptr;
  rnd_state->dev_words = reinterpret_cast<unsigned long long*>(h);
  return 0;
}
int fill_with_rand(rnd_struct* st, cudamat* mat) { return rng_launch<0>(st, mat->data_device, nullptr, numel(mat), 0, 0, 0); }
int fill_with_randn(rnd_struct* st, cudamat* mat) { return rng_launch<1>(st, mat->data_device, nullptr, numel(mat), 0, 0, 0); }
int sample_bernoulli(rnd_struct* st, cudamat* mat, cudamat* target) {
  if (numel(mat) != numel(target)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  return rng_launch<3>(st, target->data_device, mat->data_device, numel(mat), 0, 0, 0);
}
int dropout(rnd_struct* st, cudamat* mat, float dropprob, float val, float scale) {
  return rng_launch<2>(st, mat->data_device, mat->data_device, numel(mat), dropprob, val, scale);
}
int relu_dropout(rnd_struct* st, cudamat* mat, float dropprob, float scale) {
  return rng_launch<4>(st, mat->data_device, mat->data_device, numel(mat), dropprob, 0.f, scale);
}

// ---- Gaussian dropout (include/convnet_hip.h).  Every check comes before the counter moves or anything is launched. ---------------------
static_assert(sizeof(size_t) == sizeof(unsigned long long), "a call id travels as size_t");
namespace {
int gauss_check(const rnd_struct* st, const cudamat* a, const cudamat* b, int act) {
  if (!st || !st->dev_words) return ERROR_GENERIC;
  if (b) {
    if (int rc = same_shape_check(a, b, nullptr)) return rc;
  } else if (!a->on_device) {
    return ERROR_NOT_ON_DEVICE;
  }
  if (act < 0 || act > 2 || numel(a) > (size_t)INT_MAX) return ERROR_UNSUPPORTED;
  return 0;
}
}  // namespace
int gaussian_dropout(rnd_struct* st, cudamat* mat, float stddev, float max_act, int act, void* call_id) {
  if (int rc = gauss_check(st, mat, nullptr, act)) return rc;
  RngHost* h = reinterpret_cast<RngHost*>(st->dev_words);
  const unsigned long long id = h->counter++;   // one counter value per call, as fill_with_randn takes
  if (call_id) *static_cast<unsigned long long*>(call_id) = id;
  return gauss_launch<1>(st, id, mat->data_device, nullptr, numel(mat), stddev, max_act, act, 0);
}
int gaussian_dropout_noise(rnd_struct* st, size_t call_id, float stddev, cudamat* target) {
  if (int rc = gauss_check(st, target, nullptr, 0)) return rc;
  return gauss_launch<0>(st, call_id, target->data_device, nullptr, numel(target), stddev, 0.f, 0, 0);
}
int gaussian_dropout_undo(rnd_struct* st, size_t call_id, float stddev, cudamat* deriv, cudamat* state, int act, int restore_state) {
  if (int rc = gauss_check(st, deriv, state, act)) return rc;
  return gauss_launch<2>(st, call_id, deriv->data_device, state->data_device, numel(deriv), stddev, 0.f, act, restore_state != 0);
}

}  // extern "C"
