// feature_rows: a layer state (N, D), case fastest, becomes rows of D contiguous floats — the layout of a feature file's dataset —
// averaged on the way: over `passes` consecutive calls (DataWriter::Write's buf.Add / buf.Divide, src/datawriter.cc:130-152) and over
// groups of `group` consecutive cases (WriteHDF5SeqBuf's slice.SumCols(buf, 1, 1 / average_online), :96-128).  One launch per call:
//   not the last pass : sum = (0 or sum) + state, element-wise;
//   last pass, group 1: a transpose through a 64 x 65 LDS tile, 16-byte loads along N and 16-byte stores along D where the bases allow;
//   last pass, group>1: a block owns 64 dims and walks the cases tile by tile; the tile is read coalesced along N, and one lane per dim
//                       sums its cases out of LDS in case order, storing a row whenever a group is full.  No atomics: the order is fixed.
#include "common.h"

namespace chip {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kFrTile = 64;            // cases x dims of a tile
constexpr int kFrLd = kFrTile + 1;     // + one 4-byte access width: column reads fall on distinct banks
constexpr int kFrThreads = 256;

__global__ void __launch_bounds__(kFrThreads) feature_sum_kernel(const float* __restrict__ state, float* sum, size_t n, bool first, bool vec) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (vec) {
    const size_t n4 = n >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      const f32x4 x = reinterpret_cast<const f32x4*>(state)[i];
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      if (!first) s = reinterpret_cast<const f32x4*>(sum)[i];
      reinterpret_cast<f32x4*>(sum)[i] = s + x;     // (0 + x on the first pass: what Add into a zeroed buffer leaves, -0 included)
    }
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += stride) sum[i] = (first ? 0.f : sum[i]) + state[i];
}

// tile[d - d0][n - n0] = v(n, d) for the part of [n0, n0 + 64) x [d0, d0 + 64) inside (N, D); v = state, or (sum + state) / passes
template <bool AVG>
__device__ __forceinline__ void fr_load_tile(float (*tile)[kFrLd], const float* __restrict__ state, const float* __restrict__ sum, int N, int D,
                                             int n0, int d0, float passes, bool vec_n) {
  const int t = threadIdx.x;
  if (vec_n) {                         // N % 4 == 0 and 16-byte bases: a float4 is inside or outside as a whole
    const int n4 = (t & 15) * 4, n = n0 + n4;
    for (int j = t >> 4; j < kFrTile; j += kFrThreads / 16) {
      const int d = d0 + j;
      if (n < N && d < D) {
        const size_t off = (size_t)n + (size_t)N * d;
        f32x4 x = *reinterpret_cast<const f32x4*>(state + off);
        if (AVG) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(sum + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = (s[e] + x[e]) / passes;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[j][n4 + e] = x[e];
      }
    }
  } else {
    const int nl = t & 63, n = n0 + nl;
    for (int j = t >> 6; j < kFrTile; j += kFrThreads / 64) {
      const int d = d0 + j;
      if (n < N && d < D) {
        const size_t off = (size_t)n + (size_t)N * d;
        const float x = state[off];
        tile[j][nl] = AVG ? (sum[off] + x) / passes : x;
      }
    }
  }
}

template <bool AVG>
__global__ void __launch_bounds__(kFrThreads) feature_rows_kernel(const float* __restrict__ state, const float* __restrict__ sum,
                                                                  float* __restrict__ rows, int N, int D, int cases, float passes,
                                                                  bool vec_n, bool vec_d) {
  __shared__ float tile[kFrTile][kFrLd];
  const int n0 = blockIdx.x * kFrTile, d0 = blockIdx.y * kFrTile, t = threadIdx.x;
  fr_load_tile<AVG>(tile, state, sum, N, D, n0, d0, passes, vec_n);
  __syncthreads();
  if (vec_d) {                         // D % 4 == 0 and a 16-byte base
    const int d4 = (t & 15) * 4, d = d0 + d4;
    for (int j = t >> 4; j < kFrTile; j += kFrThreads / 16) {
      const int n = n0 + j;
      if (n < cases && d < D) {
        const f32x4 o = {tile[d4][j], tile[d4 + 1][j], tile[d4 + 2][j], tile[d4 + 3][j]};
        *reinterpret_cast<f32x4*>(rows + (size_t)d + (size_t)D * n) = o;
      }
    }
  } else {
    const int dl = t & 63, d = d0 + dl;
    for (int j = t >> 6; j < kFrTile; j += kFrThreads / 64) {
      const int n = n0 + j;
      if (n < cases && d < D) rows[(size_t)d + (size_t)D * n] = tile[dl][j];
    }
  }
}

template <bool AVG>
__global__ void __launch_bounds__(kFrThreads) feature_group_rows_kernel(const float* __restrict__ state, const float* __restrict__ sum,
                                                                        float* __restrict__ rows, float* __restrict__ carry, int N, int D,
                                                                        int cases, float passes, int consumed, int group, float inv_group,
                                                                        bool vec_n) {
  __shared__ float tile[kFrTile][kFrLd];
  const int d0 = blockIdx.x * kFrTile, t = threadIdx.x, d = d0 + t;
  const bool owner = t < kFrTile && d < D;     // one lane per dim does the sums: lane t reads row t of the tile, 65 floats apart
  float acc = owner && consumed > 0 ? carry[d] : 0.f;
  int open = consumed, row = 0;
  for (int n0 = 0; n0 < cases; n0 += kFrTile) {
    if (n0) __syncthreads();
    fr_load_tile<AVG>(tile, state, sum, N, D, n0, d0, passes, vec_n);
    __syncthreads();
    if (owner) {
      const int lim = min(kFrTile, cases - n0);
      for (int j = 0; j < lim; ++j) {
        acc = fmaf(tile[t][j], inv_group, acc);
        if (++open == group) {
          rows[(size_t)d + (size_t)D * row] = acc;
          ++row;
          acc = 0.f;
          open = 0;
        }
      }
    }
  }
  if (owner) carry[d] = open > 0 ? acc : 0.f;
}

}  // namespace chip

using namespace chip;

extern "C" int feature_rows(cudamat* state, cudamat* sum, int pass, int passes, int cases, cudamat* carry, int consumed, int group,
                            cudamat* rows) {
  if (!state || !rows) return ERROR_GENERIC;
  if (passes < 1 || pass < 0 || pass >= passes || group < 1 || consumed < 0 || consumed >= group || cases < 0) return ERROR_GENERIC;
  const bool last = pass == passes - 1, avg = passes > 1;
  if (avg && !sum) return ERROR_GENERIC;
  if (group > 1 && !carry) return ERROR_GENERIC;
  if (!state->on_device || !rows->on_device || (avg && !sum->on_device) || (group > 1 && !carry->on_device)) return ERROR_NOT_ON_DEVICE;
  if (state->is_trans || rows->is_trans || (sum && sum->is_trans) || (carry && carry->is_trans)) return ERROR_TRANSPOSED;
  const int N = state->size[0], D = state->size[1];
  if (avg && (sum->size[0] != N || sum->size[1] != D)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int emitted = group == 1 ? cases : (consumed + cases) / group;
  if (cases > N || rows->size[0] != D || rows->size[1] < emitted) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (group > 1 && (carry->size[0] != D || carry->size[1] != 1)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const size_t n = numel(state);
  if (n == 0) return 0;
  const float* s = avg ? sum->data_device : nullptr;
  const bool vec_n = (N & 3) == 0 && aligned16(state->data_device) && aligned16(s);
  if (!last) {
    const bool vec = aligned16(state->data_device) && aligned16(s);
    size_t blocks = (n / 4 + kFrThreads) / kFrThreads;
    if (blocks > 2048) blocks = 2048;
    KernelTimer timer("feature_sum_kernel", "feature_rows", 0.0, 4.0 * n * (pass == 0 ? 2 : 3));
    hipLaunchKernelGGL(feature_sum_kernel, dim3((unsigned)blocks), dim3(kFrThreads), 0, stream(), state->data_device, sum->data_device, n,
                       pass == 0, vec);
    note_kernel("feature_sum_kernel", 0.0, (int)blocks, 1);
    return launch_status();
  }
  if (cases == 0) return 0;
  const float fp = (float)passes;
  const double bytes = 4.0 * n * (avg ? 2 : 1) + 4.0 * D * (double)(emitted + (group > 1 ? 2 : 0));
  if (group == 1) {
    const bool vec_d = (D & 3) == 0 && aligned16(rows->data_device);
    const dim3 grid(divup(cases, kFrTile), divup(D, kFrTile));
    if (grid.y > 65535u) return ERROR_UNSUPPORTED;
    KernelTimer timer(avg ? "feature_rows_kernel<avg>" : "feature_rows_kernel", "feature_rows", 0.0, bytes);
    if (avg)
      hipLaunchKernelGGL(feature_rows_kernel<true>, grid, dim3(kFrThreads), 0, stream(), state->data_device, s, rows->data_device, N, D, cases, fp,
                         vec_n, vec_d);
    else
      hipLaunchKernelGGL(feature_rows_kernel<false>, grid, dim3(kFrThreads), 0, stream(), state->data_device, s, rows->data_device, N, D, cases, fp,
                         vec_n, vec_d);
    note_kernel(avg ? "feature_rows_kernel<avg>" : "feature_rows_kernel", 0.0, (int)(grid.x * grid.y), 1);
    return launch_status();
  }
  const dim3 grid(divup(D, kFrTile));
  const float inv_group = 1.0f / (float)group;
  KernelTimer timer(avg ? "feature_group_rows_kernel<avg>" : "feature_group_rows_kernel", "feature_rows", 0.0, bytes);
  if (avg)
    hipLaunchKernelGGL(feature_group_rows_kernel<true>, grid, dim3(kFrThreads), 0, stream(), state->data_device, s, rows->data_device,
                       carry->data_device, N, D, cases, fp, consumed, group, inv_group, vec_n);
  else
    hipLaunchKernelGGL(feature_group_rows_kernel<false>, grid, dim3(kFrThreads), 0, stream(), state->data_device, s, rows->data_device,
                       carry->data_device, N, D, cases, fp, consumed, group, inv_group, vec_n);
  note_kernel(avg ? "feature_group_rows_kernel<avg>" : "feature_group_rows_kernel", 0.0, (int)grid.x, 1);
  return launch_status();
}
