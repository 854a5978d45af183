// Locally connected layers (LocalEdge, src/local_edge.cc): fprop, dgrad and wgrad as per-module GEMMs on the matrix pipe.  gfx950 only.
//
// Layouts (include/convnet_hip.h, "locally connected layers"):
//   images  (N, H·W·C)    element (n, c, y, x)  at n + N·(x + W·(y + H·c))
//   outputs (N, My·Mx·F)  element (n, f, m)     at n + N·(m + M·f),  m = my·Mx + mx
//   bank    (F, K·M)      module m owns the F·K floats at m·F·K; (f, c, ky, kx) of a block at f + F·(kx + Kx·(ky + Ky·c))
//
// One kernel template, three problem kinds; each is "for every module, a small GEMM with gathered operands":
//   UP    module m:      out_m[f, n]  = Σ_k   W_m[f, k]           · patch_m[k, n]                   rows F, cols N, depth K
//   DOWN  input pixel p: dx_p[c, n]   = Σ_(t,f) W_m(t)[f, (c, t)] · dy[n, f, m(t)]                   rows C, cols N, depth Ky·Kx·F
//         (a gather: t runs over the taps of the pixel, m(t) is the module whose tap t lands on p, invalid (t, p) pairs are zero)
//   OUTP  module m:      dW_m[f, k]   = Σ_n   dy[n, f, m]         · patch_m[k, n]                    rows F, cols K, depth N
// A block is four independent waves, each one 16 x 16 output tile of the same module and row range (the block tile is 16 rows x 64
// columns): the 16-row tile keeps thin layers (F = 16 / 32, C = 3) unpadded.  No LDS, no barrier, no atomics, no scratch: every lane
// gathers its eight depth slots of one A row and one B column straight from global memory, with bounds and padding handled per element,
// so ragged N / F / C and any stride / padding take the same path.  The depth loop runs in chunks of 32 in a fixed order — results are
// bit-identical from call to call.
//   matrix path 0: v_mfma_f32_16x16x4_f32, eight per chunk (lane (li, lh) supplies depth slot 8·lh + e to the e-th instruction);
//   matrix path 1: the exact bf16 three-way split (Split8, gather_gemm.h), six v_mfma_f32_16x16x32_bf16 per chunk.
#include "gather_gemm.h"

namespace chip {
namespace {

enum { LC_UP = 0, LC_DOWN = 1, LC_OUTP = 2 };

struct LCParams {
  const float* W;     // bank (UP / DOWN)
  const float* x;     // images (UP / OUTP)
  const float* dy;    // output derivatives (DOWN / OUTP)
  float* out;         // UP: outputs, DOWN: image derivatives, OUTP: bank gradient
  const float* bias;  // UP only, nullable: element j added to output column j
  int N, C, H, Wd, F, Ky, Kx, sy, sx, py, px, My, Mx;   // py / px: the ConvDesc (negated) padding
  int K, M;           // K = C·Ky·Kx, M = My·Mx
  int R, NC, D;       // rows, columns, depth of one module's GEMM
  float st, so;       // scaleTargets, scaleOutput
  int relu;
};

// Running position inside the depth of one problem: lane-local, started with divisions once per chunk, then stepped.
struct Walk {
  int a, b, c;   // UP / OUTP-B: (c, ky, kx) of tap k;  DOWN: (ky, kx, f) of depth d = (ky·Kx + kx)·F + f
};

__device__ __forceinline__ void walk_start_k(const LCParams& p, int k, Walk& w) {
  const int kk = p.Ky * p.Kx;
  w.a = k / kk;
  const int t = k - w.a * kk;
  w.b = t / p.Kx;
  w.c = t - w.b * p.Kx;
}
__device__ __forceinline__ void walk_step_k(const LCParams& p, Walk& w) {
  if (++w.c == p.Kx) {
    w.c = 0;
    if (++w.b == p.Ky) {
      w.b = 0;
      ++w.a;
    }
  }
}
// image element offset / N of tap (c, ky, kx) of module (my, mx), or -1 on a padding tap
__device__ __forceinline__ int patch_pix(const LCParams& p, const Walk& w, int my, int mx) {
  const int iy = my * p.sy + p.py + w.b, ix = mx * p.sx + p.px + w.c;
  if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.Wd) return -1;
  return ix + p.Wd * (iy + p.H * w.a);
}

// The eight depth slots d0 .. d0 + 7 of A row r and of B column col for one module.
template <int KIND>
__device__ __forceinline__ void lc_load(const LCParams& p, int mod, int r, int col, int d0, float (&a)[8], float (&b)[8]) {
  const bool rok = r < p.R, cok = col < p.NC;
  if constexpr (KIND == LC_UP) {
    // A = W_m[f = r, k], B = patch_m[k, n = col]
    const int my = mod / p.Mx, mx = mod - my * p.Mx;
    const float* wm = p.W + (size_t)mod * p.F * p.K + r;
    Walk w;
    walk_start_k(p, d0, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = d0 + e;
      const bool kok = k < p.K;
      a[e] = (rok && kok) ? wm[(size_t)p.F * k] : 0.f;
      const int pix = kok ? patch_pix(p, w, my, mx) : -1;
      b[e] = (cok && pix >= 0) ? p.x[col + (size_t)p.N * pix] : 0.f;
      walk_step_k(p, w);
    }
  } else if constexpr (KIND == LC_OUTP) {
    // A = dy[n, f = r, m], B = patch_m[k = col, n]
    const int my = mod / p.Mx, mx = mod - my * p.Mx;
    Walk w;
    int pix = -1;
    if (cok) {
      walk_start_k(p, col, w);
      pix = patch_pix(p, w, my, mx);
    }
    const float* dyr = p.dy + (size_t)p.N * (mod + (size_t)p.M * r);
    const float* xs = p.x + (size_t)p.N * (pix < 0 ? 0 : pix);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = d0 + e;
      const bool nok = n < p.N;
      a[e] = (rok && nok) ? dyr[n] : 0.f;
      b[e] = (nok && pix >= 0) ? xs[n] : 0.f;
    }
  } else {
    // DOWN, module = input pixel (iy, ix) and channel c = r:  A = W_m(t)[f, (c, t)], B = dy[n = col, f, m(t)]
    const int iy = mod / p.Wd, ix = mod - iy * p.Wd;
    const int t0 = d0 / p.F;
    int f = d0 - t0 * p.F, ky = t0 / p.Kx, kx = t0 - ky * p.Kx;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int m = -1;
      if (ky < p.Ky) {
        const int ty = iy - p.py - ky, tx = ix - p.px - kx;
        if (ty >= 0 && tx >= 0) {
          const int my = ty / p.sy, mx = tx / p.sx;
          if (my * p.sy == ty && mx * p.sx == tx && my < p.My && mx < p.Mx) m = my * p.Mx + mx;
        }
      }
      a[e] = (rok && m >= 0) ? p.W[(size_t)m * p.F * p.K + f + (size_t)p.F * (kx + p.Kx * (ky + p.Ky * r))] : 0.f;
      b[e] = (cok && m >= 0) ? p.dy[col + (size_t)p.N * (m + (size_t)p.M * f)] : 0.f;
      if (++f == p.F) {
        f = 0;
        if (++kx == p.Kx) {
          kx = 0;
          ++ky;
        }
      }
    }
  }
}

template <int KIND, bool SPLIT>
__global__ __launch_bounds__(256) void lc_kernel(LCParams p) {
  const int mod = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 15, lh = lane >> 4;
  const int r0 = blockIdx.z * 16, c0 = (blockIdx.y * 4 + wave) * 16;
  if (c0 >= p.NC) return;   // (waves are independent: no barrier below)
  const int r = r0 + li, col = c0 + li;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < p.D; d += 32) {
    float a[8], b[8];
    lc_load<KIND>(p, mod, r, col, d + 8 * lh, a, b);
    if constexpr (KIND == LC_DOWN) {
      // a chunk none of whose taps reaches this pixel (strided layers: most of them) issues no MFMA
      bool any = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) any |= (a[e] != 0.f) | (b[e] != 0.f);
      if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
    }
    if constexpr (SPLIT) {
      Split8 sa, sb;
      split8(a, sa);
      split8(b, sb);
      acc = split_mac(sa, sb, acc);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    }
  }
  // D register q of lane (li, lh): row 4·lh + q, column li
  if (col >= p.NC) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = r0 + 4 * lh + q;
    if (row >= p.R) continue;
    size_t o;
    if constexpr (KIND == LC_UP) o = col + (size_t)p.N * (mod + (size_t)p.M * row);
    else if constexpr (KIND == LC_DOWN) o = col + (size_t)p.N * (mod + (size_t)p.H * p.Wd * row);
    else o = (size_t)mod * p.F * p.K + row + (size_t)p.F * col;
    float v = KIND == LC_OUTP ? p.so * acc[q] : acc[q];
    if (p.st != 0.f) v = p.st * p.out[o] + v;
    if constexpr (KIND == LC_UP) {
      if (p.bias) v = v + p.bias[mod + (size_t)p.M * row];
      if (p.relu) v = v > 0.f ? v : 0.f;
    }
    p.out[o] = v;
  }
}

struct LocalGeo {
  int N, C, H, W, F, Ky, Kx, sy, sx, py, px, My, Mx;
};

// The consistency checks of _convUpGemm (cudamat_conv_gemm.cu:586-610) with filterModuleMult = M: the bank is (F, Kx·Ky·C·M) and its
// Shape4D is (F, Kx, Ky, C·My·Mx) (src/local_edge.cc, SetMemory).
LocalGeo local_geo(const Shape4D* img, const Shape4D* flt, const Shape4D* out, const ConvDesc& d, const cudamat* mi, const cudamat* mf,
                   const cudamat* mo) {
  LocalGeo g;
  g.N = img->shape[0]; g.W = img->shape[1]; g.H = img->shape[2]; g.C = img->shape[3];
  g.Mx = out->shape[1]; g.My = out->shape[2]; g.F = out->shape[3];
  g.Ky = d.kernel_size_y; g.Kx = d.kernel_size_x; g.sy = d.stride_y; g.sx = d.stride_x;
  g.py = d.padding_y; g.px = d.padding_x;
  const int M = g.My * g.Mx;
  CHIP_REQUIRE(out->shape[0] == g.N);
  CHIP_REQUIRE(d.num_input_channels == g.C && d.num_output_channels == g.F);
  CHIP_REQUIRE(d.num_groups == 1);
  CHIP_REQUIRE(d.input_channel_begin == 0 && (d.input_channel_end == 0 || d.input_channel_end == g.C));
  CHIP_REQUIRE(d.output_channel_begin == 0 && (d.output_channel_end == 0 || d.output_channel_end == g.F));
  CHIP_REQUIRE(d.kernel_size_t <= 1);
  CHIP_REQUIRE(g.sy >= 1 && g.sx >= 1 && g.Ky >= 1 && g.Kx >= 1 && g.py <= 0 && g.px <= 0);
  CHIP_REQUIRE(flt->shape[0] == g.F && flt->shape[1] == g.Kx && flt->shape[2] == g.Ky && flt->shape[3] == g.C * M);
  CHIP_REQUIRE(mi->size[0] == g.N && mi->size[1] == g.H * g.W * g.C);
  CHIP_REQUIRE(mo->size[0] == g.N && mo->size[1] == M * g.F);
  CHIP_REQUIRE(mf->size[0] == g.F && (size_t)mf->size[1] == (size_t)g.Ky * g.Kx * g.C * M);
  CHIP_REQUIRE(g.My == (g.H - 2 * g.py - g.Ky) / g.sy + 1 && g.Mx == (g.W - 2 * g.px - g.Kx) / g.sx + 1);
  CHIP_REQUIRE(g.My >= 1 && g.Mx >= 1);
  CHIP_REQUIRE((size_t)g.N * g.H * g.W * g.C < (1ull << 31) && (size_t)g.N * M * g.F < (1ull << 31));
  return g;
}

LCParams lc_params(const LocalGeo& g) {
  LCParams p = {};
  p.N = g.N; p.C = g.C; p.H = g.H; p.Wd = g.W; p.F = g.F; p.Ky = g.Ky; p.Kx = g.Kx; p.sy = g.sy; p.sx = g.sx; p.py = g.py; p.px = g.px;
  p.My = g.My; p.Mx = g.Mx;
  p.K = g.C * g.Ky * g.Kx;
  p.M = g.My * g.Mx;
  p.so = 1.f;
  return p;
}

template <int KIND>
void lc_launch(const LCParams& p, int modules, const char* op, double flops, double bytes) {
  static const char* names[3][2] = {{"lc_kernel<up,fp32>", "lc_kernel<up,split>"},
                                    {"lc_kernel<down,fp32>", "lc_kernel<down,split>"},
                                    {"lc_kernel<outp,fp32>", "lc_kernel<outp,split>"}};
  const bool split = matrix_path() != 0;
  const dim3 grid((unsigned)modules, (unsigned)divup(p.NC, 64), (unsigned)divup(p.R, 16));
  CHIP_REQUIRE(grid.y < 65536 && grid.z < 65536);
  note_kernel(names[KIND][split], flops, (int)(grid.x * grid.y * grid.z), 1);
  hipStream_t s = stream();   // (flushes a parked call first)
  KernelTimer timer(names[KIND][split], op, flops, bytes);
  if (split) hipLaunchKernelGGL((lc_kernel<KIND, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((lc_kernel<KIND, false>), grid, dim3(256), 0, s, p);
  CHIP_CHECK(hipGetLastError());
}

void local_up_impl(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets, Shape4D* is, Shape4D* fs, Shape4D* ts,
                   const ConvDesc& d, float scaleTargets, int relu) {
  const LocalGeo g = local_geo(is, fs, ts, d, images, filters, targets);
  LCParams p = lc_params(g);
  if (bias) CHIP_REQUIRE(bias->on_device && numel(bias) == (size_t)p.F * p.M);
  p.W = filters->data_device; p.x = images->data_device; p.out = targets->data_device;
  p.bias = bias ? bias->data_device : nullptr;
  p.R = p.F; p.NC = p.N; p.D = p.K;
  p.st = scaleTargets; p.relu = relu != 0;
  const double flops = 2.0 * p.N * p.F * (double)p.K * p.M;
  const double bytes = 4.0 * ((double)p.F * p.K * p.M + (double)p.N * p.H * p.Wd * p.C + (double)p.N * p.F * p.M * (scaleTargets != 0.f ? 2 : 1));
  lc_launch<LC_UP>(p, p.M, "local_fprop", flops, bytes);
}

void local_down_impl(cudamat* derivs, cudamat* filters, cudamat* targets, Shape4D* ds, Shape4D* fs, Shape4D* ts, const ConvDesc& d,
                     float scaleTargets) {
  const LocalGeo g = local_geo(ts, fs, ds, d, targets, filters, derivs);
  LCParams p = lc_params(g);
  p.W = filters->data_device; p.dy = derivs->data_device; p.out = targets->data_device;
  p.R = p.C; p.NC = p.N; p.D = p.Ky * p.Kx * p.F;
  p.st = scaleTargets;
  const double flops = 2.0 * p.N * p.F * (double)p.K * p.M;
  const double bytes = 4.0 * ((double)p.F * p.K * p.M + (double)p.N * p.F * p.M + (double)p.N * p.H * p.Wd * p.C * (scaleTargets != 0.f ? 2 : 1));
  lc_launch<LC_DOWN>(p, p.H * p.Wd, "local_dgrad", flops, bytes);
}

void local_outp_impl(cudamat* images, cudamat* derivs, cudamat* targets, Shape4D* is, Shape4D* ds, Shape4D* ts, const ConvDesc& d,
                     float scaleTargets, float scaleOutput) {
  const LocalGeo g = local_geo(is, ts, ds, d, images, targets, derivs);
  LCParams p = lc_params(g);
  p.x = images->data_device; p.dy = derivs->data_device; p.out = targets->data_device;
  p.R = p.F; p.NC = p.K; p.D = p.N;
  p.st = scaleTargets; p.so = scaleOutput;
  const double flops = 2.0 * p.N * p.F * (double)p.K * p.M;
  const double bytes = 4.0 * ((double)p.F * p.K * p.M * (scaleTargets != 0.f ? 2 : 1) + (double)p.N * p.H * p.Wd * p.C + (double)p.N * p.F * p.M);
  lc_launch<LC_OUTP>(p, p.M, "local_wgrad", flops, bytes);
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" {

void localUpGemm(cudamat* images, cudamat* filters, cudamat* targets, Shape4D* images_shape, Shape4D* filters_shape,
                 Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets) {
  local_up_impl(images, filters, nullptr, targets, images_shape, filters_shape, targets_shape, conv_desc, scaleTargets, 0);
}
void localDownGemm(cudamat* derivs, cudamat* filters, cudamat* targets, Shape4D* derivs_shape, Shape4D* filters_shape,
                   Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets) {
  local_down_impl(derivs, filters, targets, derivs_shape, filters_shape, targets_shape, conv_desc, scaleTargets);
}
void localOutpGemm(cudamat* images, cudamat* derivs, cudamat* targets, Shape4D* images_shape, Shape4D* derivs_shape,
                   Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets, float scaleOutput) {
  local_outp_impl(images, derivs, targets, images_shape, derivs_shape, targets_shape, conv_desc, scaleTargets, scaleOutput);
}
void localUp(cudamat* images, cudamat* filters, cudamat* targets, Shape4D* images_shape, Shape4D* filters_shape,
             Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets) {
  local_up_impl(images, filters, nullptr, targets, images_shape, filters_shape, targets_shape, conv_desc, scaleTargets, 0);
}
void localDown(cudamat* derivs, cudamat* filters, cudamat* targets, Shape4D* derivs_shape, Shape4D* filters_shape,
               Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets) {
  local_down_impl(derivs, filters, targets, derivs_shape, filters_shape, targets_shape, conv_desc, scaleTargets);
}
void localOutp(cudamat* images, cudamat* derivs, cudamat* targets, Shape4D* images_shape, Shape4D* derivs_shape,
               Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets, float scaleOutput) {
  local_outp_impl(images, derivs, targets, images_shape, derivs_shape, targets_shape, conv_desc, scaleTargets, scaleOutput);
}
void localUpBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets, Shape4D* images_shape, Shape4D* filters_shape,
                    Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets, int relu) {
  local_up_impl(images, filters, bias, targets, images_shape, filters_shape, targets_shape, conv_desc, scaleTargets, relu);
}

}  // extern "C"
