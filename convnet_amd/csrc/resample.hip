// Resampling and colour transform on the CHWN layout: UpSampleGemm / DownSampleGemm (src/upsample_edge.cc through Matrix::ConvUpSample /
// ConvDownSample, src/matrix.cc:992-1011) and RGBToYUV (cudamat_conv_others.cu:296-325).  Streaming kernels in pool_norm.hip's idiom:
// one lane owns 4 consecutive images of one element, 16-byte accesses where N % 4 == 0 and the bases allow, scalar otherwise
// (get_slice views at odd N guarantee a 4-byte base only).
//   upsample   : targets[n, c, Y, X] = (scaleTargets * targets[...]) + images[n, c, Y / f, X / f].  The replicated value is the input
//                value itself: the reference forms f*f * x / (f*f) through its average-pool undo (cudamat_conv_gemm.cu:1503-1541), which
//                is x bit for bit only for power-of-two factors.  Each input element is read once and stored f*f times; no atomics.
//   downsample : the mean of each f x f block, summed row by row from 0.f and divided by (float)(f*f): the order and the division of
//                pool_fwd_kernel / pool_fwd_fixed_kernel<avg> (pool_norm.hip), so the bits are AvgPoolGemm's for kernel = stride = f.
//                Factor 2 on the 16-byte arm is handed to that pool kernel: ours measured no faster (the launcher has the figures).
//   rgb to yuv : three fused chains per pixel, explicit fmaf so the result does not depend on contraction flags.
// A bad argument sets the library's error text (get_last_cuda_error) and launches nothing.
#include <climits>
#include <cstring>

#include "common.h"

namespace chip {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f32x4 rs_ld(const float* p, int n, int N, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n + e < N) v[e] = p[e];
  return v;
}
__device__ __forceinline__ void rs_st(float* p, f32x4 v, int n, int N, bool vec) {
  if (vec) {
    *reinterpret_cast<f32x4*>(p) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n + e < N) p[e] = v[e];
}

// What both resampling kernels walk: rows = C * H rows of the SMALL map (plane c, row y: r = c * H + y), W pixels per row, nvec image
// quads per pixel.  The large map has rows * f rows of W * f pixels; row r of the small map faces rows [r * f, r * f + f) of the large
// one, whatever the plane, so neither kernel separates c from y.
struct ResampleGeo {
  int N, W, rows, f, nvec;
  unsigned total;   // rows * W * nvec work items (the launcher refuses more than INT_MAX)
};

// mode 0: overwrite (the target is not read); 1: targets + x; 2: scaleTargets * targets + x, the product and the sum each rounded
template <int F>
__global__ void __launch_bounds__(256) upsample_kernel(const float* __restrict__ in, float* __restrict__ out, ResampleGeo g, float st, int mode,
                                                       bool vec) {
  const int f = F ? F : g.f;
  const unsigned per = (unsigned)g.W * g.nvec;
  const size_t big_w = (size_t)g.W * f;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < g.total; i += gridDim.x * 256u) {
    const unsigned r = i / per, j = i - r * per;
    const unsigned x = j / g.nvec;
    const int n = 4 * (int)(j - x * g.nvec);
    const f32x4 v = rs_ld(in + ((size_t)r * g.W + x) * g.N + n, n, g.N, vec);
    float* o = out + (((size_t)r * f) * big_w + (size_t)x * f) * g.N + n;
    auto put = [&](int dy, int dx) {
      float* p = o + ((size_t)dy * big_w + dx) * g.N;
      f32x4 res = v;
      if (mode != 0) {
        const f32x4 t = rs_ld(p, n, g.N, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) res[e] = __fadd_rn(mode == 1 ? t[e] : __fmul_rn(st, t[e]), v[e]);
      }
      rs_st(p, res, n, g.N, vec);
    };
    if constexpr (F != 0) {
#pragma unroll
      for (int dy = 0; dy < F; ++dy)
#pragma unroll
        for (int dx = 0; dx < F; ++dx) put(dy, dx);
    } else {
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) put(dy, dx);
    }
  }
}

template <int F>
__global__ void __launch_bounds__(256) downsample_kernel(const float* __restrict__ in, float* __restrict__ out, ResampleGeo g, bool vec) {
  const int f = F ? F : g.f;
  const unsigned per = (unsigned)g.W * g.nvec;
  const size_t big_w = (size_t)g.W * f;
  const float cnt = (float)(f * f);
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < g.total; i += gridDim.x * 256u) {
    const unsigned r = i / per, j = i - r * per;
    const unsigned x = j / g.nvec;
    const int n = 4 * (int)(j - x * g.nvec);
    const float* s = in + (((size_t)r * f) * big_w + (size_t)x * f) * g.N + n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (F != 0) {   // every load of the block issued before the first add
      f32x4 v[F][F];
#pragma unroll
      for (int dy = 0; dy < F; ++dy)
#pragma unroll
        for (int dx = 0; dx < F; ++dx) v[dy][dx] = rs_ld(s + ((size_t)dy * big_w + dx) * g.N, n, g.N, vec);
#pragma unroll
      for (int dy = 0; dy < F; ++dy)
#pragma unroll
        for (int dx = 0; dx < F; ++dx)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], v[dy][dx][e]);
    } else {
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) {
          const f32x4 v = rs_ld(s + ((size_t)dy * big_w + dx) * g.N, n, g.N, vec);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __fdiv_rn(acc[e], cnt);
    rs_st(out + ((size_t)r * g.W + x) * g.N + n, acc, n, g.N, vec);
  }
}

// plane = pixels * N floats per colour; lane i owns floats [4i, 4i + 4) of each plane.  targets == images is allowed: a lane has read
// its three inputs before it stores.
__global__ void __launch_bounds__(256) rgb_to_yuv_kernel(const float* in, float* out, size_t plane, bool vec) {
  const size_t quads = (plane + 3) / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (size_t)gridDim.x * 256) {
    const size_t o = 4 * i;
    const int left = plane - o < 4 ? (int)(plane - o) : 4;
    const f32x4 R = rs_ld(in + o, 0, left, vec), G = rs_ld(in + plane + o, 0, left, vec), B = rs_ld(in + 2 * plane + o, 0, left, vec);
    f32x4 Y, U, V;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Y[e] = fmaf(0.0722f, B[e], fmaf(0.7152f, G[e], __fmul_rn(0.2126f, R[e])));
      U[e] = fmaf(0.436f, B[e], fmaf(-0.33609f, G[e], __fmul_rn(-0.09991f, R[e])));
      V[e] = fmaf(-0.05639f, B[e], fmaf(-0.55861f, G[e], __fmul_rn(0.615f, R[e])));
    }
    rs_st(out + o, Y, 0, left, vec);
    rs_st(out + plane + o, U, 0, left, vec);
    rs_st(out + 2 * plane + o, V, 0, left, vec);
  }
}

inline void refuse(const char* entry, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", entry, why);
  set_last_error(msg);
}

inline unsigned stream_grid(size_t items) {
  size_t b = (items + 255) / 256;
  if (b > 4096) b = 4096;
  return b ? (unsigned)b : 1u;
}

// The checks the two resampling entries share: `small` / `large` are the operands on the coarse and on the fine map.  false: refused.
bool resample_geo(const char* entry, const cudamat* small, const cudamat* large, const Shape4D* ss, const Shape4D* ls, int factor, ResampleGeo& g) {
  if (!small || !large || !ss || !ls) return refuse(entry, "NULL operand"), false;
  if (!small->on_device || !large->on_device) return refuse(entry, "operand not in device memory"), false;
  if (small->is_trans || large->is_trans) return refuse(entry, "transposed operand"), false;
  if (factor < 1) return refuse(entry, "factor < 1"), false;
  const int N = ss->shape[0], W = ss->shape[1], H = ss->shape[2], C = ss->shape[3];
  if (N < 0 || W < 0 || H < 0 || C < 0) return refuse(entry, "negative shape"), false;
  if (ls->shape[0] != N) return refuse(entry, "image counts differ"), false;
  if (ls->shape[3] != C) return refuse(entry, "channel counts differ"), false;
  if ((long long)ls->shape[1] != (long long)W * factor || (long long)ls->shape[2] != (long long)H * factor)
    return refuse(entry, "the fine map is not factor x the coarse map on both axes"), false;
  const size_t small_cols = (size_t)W * H * C, large_cols = small_cols * factor * factor;
  if (small->size[0] != N || (size_t)small->size[1] != small_cols || large->size[0] != N || (size_t)large->size[1] != large_cols)
    return refuse(entry, "a matrix does not have the size of its shape"), false;
  const size_t items = (size_t)C * H * W * (size_t)divup(N, 4);
  if ((size_t)C * H > INT_MAX || items > INT_MAX) return refuse(entry, "more than 2^31 - 1 work items"), false;
  g.N = N; g.W = W; g.rows = C * H; g.f = factor; g.nvec = divup(N, 4);
  g.total = (unsigned)items;
  return true;
}

inline bool rs_vec(int N, const void* a, const void* b) { return N % 4 == 0 && aligned16(a) && aligned16(b); }
#define RS_NAME(vec, name) ((vec) ? name "/vec" : name "/scalar")

void upsample(cudamat* images, cudamat* targets, Shape4D* is, Shape4D* ts, int factor, float scaleTargets) {
  ResampleGeo g;
  if (!resample_geo("UpSampleGemm", images, targets, is, ts, factor, g)) return;
  if (g.total == 0) return;
  const float* in = images->data_device;
  float* out = targets->data_device;
  const bool vec = rs_vec(g.N, in, out);
  const int mode = scaleTargets == 0.f ? 0 : scaleTargets == 1.f ? 1 : 2;
  const dim3 grid(stream_grid(g.total));
  const double small_b = 4.0 * numel(images), large_b = 4.0 * numel(targets);
  KernelTimer timer("upsample_kernel", "upsample", 0.0, small_b + large_b * (mode ? 2 : 1));
#define RS_UP(F, name)                                                                                              \
  {                                                                                                                 \
    hipLaunchKernelGGL(upsample_kernel<F>, grid, dim3(256), 0, stream(), in, out, g, scaleTargets, mode, vec);      \
    note_kernel(RS_NAME(vec, name), 0.0, (int)grid.x, 1);                                                           \
    break;                                                                                                          \
  }
  switch (factor) {
    case 2: RS_UP(2, "upsample_kernel<2>")
    case 3: RS_UP(3, "upsample_kernel<3>")
    case 4: RS_UP(4, "upsample_kernel<4>")
    default: RS_UP(0, "upsample_kernel<generic>")
  }
#undef RS_UP
}

void downsample(cudamat* images, cudamat* targets, Shape4D* is, Shape4D* ts, int factor) {
  ResampleGeo g;
  if (!resample_geo("DownSampleGemm", targets, images, ts, is, factor, g)) return;
  if (g.total == 0) return;
  const float* in = images->data_device;
  float* out = targets->data_device;
  const bool vec = rs_vec(g.N, in, out);
  if (factor == 2 && vec && is->shape[2] <= 65535 && is->shape[3] <= 65535) {
    // What pool_norm.hip's fixed 2 x 2 window kernel serves goes to it: it reads each element once too and leaves the same bits, and
    // downsample_kernel<2> measured no faster (N 128, C 64, 112 x 112 -> 56 x 56: 0.097 [0.091-0.103] against 0.094 [0.090-0.106] ms,
    // DESIGN.md 2.16)
    ConvDesc d;
    memset(&d, 0, sizeof d);
    d.num_input_channels = d.num_output_channels = d.input_channel_end = d.output_channel_end = is->shape[3];
    d.kernel_size_y = d.kernel_size_x = d.stride_y = d.stride_x = factor;
    d.kernel_size_t = d.stride_t = d.num_groups = 1;
    return AvgPoolGemm(images, targets, is, ts, d, 0.f, 1.f);
  }
  const dim3 grid(stream_grid(g.total));
  KernelTimer timer("downsample_kernel", "downsample", 0.0, 4.0 * numel(images) + 4.0 * numel(targets));
#define RS_DOWN(F, name)                                                                         \
  {                                                                                              \
    hipLaunchKernelGGL(downsample_kernel<F>, grid, dim3(256), 0, stream(), in, out, g, vec);     \
    note_kernel(RS_NAME(vec, name), 0.0, (int)grid.x, 1);                                        \
    break;                                                                                       \
  }
  switch (factor) {
    case 2: RS_DOWN(2, "downsample_kernel<2>")
    case 3: RS_DOWN(3, "downsample_kernel<3>")
    case 4: RS_DOWN(4, "downsample_kernel<4>")
    default: RS_DOWN(0, "downsample_kernel<generic>")
  }
#undef RS_DOWN
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" {

void UpSampleGemm(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor, float scaleTargets) {
  upsample(images, targets, images_shape, targets_shape, factor, scaleTargets);
}
void UpSample(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor, float scaleTargets) {
  upsample(images, targets, images_shape, targets_shape, factor, scaleTargets);
}
void DownSampleGemm(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor) {
  downsample(images, targets, images_shape, targets_shape, factor);
}
void DownSample(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor) {
  downsample(images, targets, images_shape, targets_shape, factor);
}

void RGBToYUV(cudamat* images, cudamat* targets) {
  const char* entry = "RGBToYUV";
  if (!images || !targets) return refuse(entry, "NULL operand");
  if (!images->on_device || !targets->on_device) return refuse(entry, "operand not in device memory");
  if (images->is_trans || targets->is_trans) return refuse(entry, "transposed operand");
  if (images->size[0] != targets->size[0] || images->size[1] != targets->size[1]) return refuse(entry, "images and targets differ in size");
  if (images->size[0] < 0 || images->size[1] < 0 || images->size[1] % 3 != 0) return refuse(entry, "the column count is not divisible by 3");
  const size_t plane = (size_t)images->size[0] * (size_t)(images->size[1] / 3);
  if (plane == 0) return;
  const float* in = images->data_device;
  float* out = targets->data_device;
  const bool vec = plane % 4 == 0 && aligned16(in) && aligned16(out);
  const dim3 grid(stream_grid((plane + 3) / 4));
  KernelTimer timer("rgb_to_yuv_kernel", "rgb_to_yuv", 0.0, 24.0 * plane);
  hipLaunchKernelGGL(rgb_to_yuv_kernel, grid, dim3(256), 0, stream(), in, out, plane, vec);
  note_kernel(RS_NAME(vec, "rgb_to_yuv_kernel"), 0.0, (int)grid.x, 1);
}

}  // extern "C"
