// Spatio-temporal (3-D) convolution, response norm and pooling (reference: cudamat/cudamat_conv3d_gemm.cu, five host loops over the
// 2-D entries; pooling: cudamat_conv_gemm.cu:153-300, natively 3-D).  gfx950 only.
//
// Layouts (include/convnet_hip.h, "spatio-temporal convolution"): time is the OUTERMOST index,
//   activations (N, X·Y·C·T)     element (n, x, y, c, t)     at n + N·(x + W·(y + H·(c + C·t)))
//   bank        (F, Kx·Ky·C·Kt)  element (f, kx, ky, c, kt)  at f + F·(kx + Kx·(ky + Ky·(c + C·kt)))
// so frame t of a tensor is a contiguous column range, and output frame m of a 3-D convolution is the 2-D convolution of the C·Kt
// contiguous channels that start at input frame m·st.
//
//   fprop  Mt frame launches of the 2-D forward path on column slices; the bank's planes / tap-major copy are built by the first frame
//          and shared by the others (filter_planes_share, patch_gemm.hip).
//   wgrad  Mt frame launches of the 2-D weight gradient that write their split-K slabs into one arena, then ONE reduction that applies
//          scaleTargets / scaleOutput: dW is written once per call (wg_batch_begin / wg_batch_end, gather_gemm.hip).
//   dgrad  a GATHER over time.  Input frame ti receives from the output frames m with 0 <= ti - m·st < Kt; these are consecutive, and
//          consecutive output frames are contiguous channels of derivs.  So frame ti is ONE 2-D dgrad over the F·nv channels that start
//          at frame m_lo, with the bank  W'[f + F·j, kx, ky, c] = W[f, kx, ky, c, kt0 - j·st],  kt0 = ti - m_lo·st.
//          Frames with the same (kt0, nv) share a bank; conv3d_dgrad_bank_kernel lays the banks of all classes out once per call.
//          Every input frame is written exactly once with the caller's scaleTargets (no Scale pass, no read-modify-write of overlapping
//          windows), which also makes the fused ReLU' epilogue of convDownMask legal.  Frames no window covers get scaleTargets·targets.
//          Used when C % 16 == 0, where it was measured faster than the reference's loop; other C run that loop (conv3d_down).
//   rnorm  the 2-D operation on each frame.
//   pool   pooling over time lives with the other pooling kernels (pool_norm.hip: pool3d_fwd_kernel / pool3d_undo_kernel).
// The caller's cudamat structs are never written (the reference moves their data_device and size[1] during its loops): every launch
// gets slice copies.  None of the entries is parked as a deferred epilogue; a parked call is flushed before the first launch.
#include <algorithm>
#include <cfloat>
#include <map>
#include <utility>
#include <vector>

#include "common.h"

namespace chip {

namespace {

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int grid_for(size_t items) {
  size_t b = (items + 255) / 256;
  if (b > 4096) b = 4096;
  return b ? (int)b : 1;
}

// Class bank of the time gather: Wc (F·nv, K2) column-major, Wc[f + F·j, k] = W[f, k, kt0 - j·st]  (K2 = Kx·Ky·C).
__global__ void conv3d_dgrad_bank_kernel(const float* __restrict__ W, float* __restrict__ Wc, int F, int K2, int nv, int kt0, int st) {
  const size_t rows = (size_t)F * nv, total = rows * K2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i % rows), k = (int)(i / rows);
    const int f = r % F, j = r / F;
    Wc[i] = W[f + (size_t)F * (k + (size_t)K2 * (kt0 - j * st))];
  }
}

// An input frame no window covers: dst = scaleTargets·dst, with convDownMask's epilogue when there is a mask.
__global__ void conv3d_scale_frame_kernel(float* __restrict__ dst, const float* __restrict__ mask, size_t n, float st, float post_scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = st != 0.f ? st * dst[i] : 0.f;
    if (mask) v = mask[i] > 0.f ? v * post_scale : 0.f;
    dst[i] = v;
  }
}

}  // namespace

namespace {

// Which batched forms run (DESIGN.md 2.6 has the measurements behind the default).  CONVNET_CONV3D_BATCH, read once per process, for
// A/B runs of tools/conv3d_bench.py: bit 0 = filter-bank preparation shared by the frames of a call, bit 1 = one dW reduction per call.
// No setting changes what is computed beyond the summation order of dW.
inline int batch_forms() { return CHIP_KNOB("CONVNET_CONV3D_BATCH", 3); }

// Geometry of one 3-D convolution call and the 2-D descriptor of its frame launches.
struct Geo3D {
  int N, X, Y, C, T, Mx, My, F, Mt, Kt, st, K2;
  size_t in_frame, out_frame;   // floats per image of one frame
  ConvDesc d2;                  // kernel_size_t = 1, C·Kt input channels
};

Geo3D geo3d(const Shape4D* img, const Shape4D* flt, const Shape4D* out, const ConvDesc& d, const cudamat* mi, const cudamat* mf,
            const cudamat* mo) {
  Geo3D g;
  CHIP_REQUIRE(mi->on_device && mf->on_device && mo->on_device);
  CHIP_REQUIRE(d.padding_t == 0);   // cudamat_conv3d_gemm.cu:23 asserts the same
  g.Kt = d.kernel_size_t > 1 ? d.kernel_size_t : 1;
  g.st = d.stride_t > 1 ? d.stride_t : 1;
  g.C = d.num_input_channels;
  g.F = d.num_output_channels;
  CHIP_REQUIRE(g.C > 0 && g.F > 0 && d.num_groups == 1);
  // whole channel ranges only (the reference: "only full slices are supported in 3d conv")
  CHIP_REQUIRE(d.input_channel_begin == 0 && (d.input_channel_end == 0 || d.input_channel_end == g.C));
  CHIP_REQUIRE(d.output_channel_begin == 0 && (d.output_channel_end == 0 || d.output_channel_end == g.F));
  g.N = img->shape[0]; g.X = img->shape[1]; g.Y = img->shape[2];
  g.Mx = out->shape[1]; g.My = out->shape[2];
  CHIP_REQUIRE(img->shape[3] > 0 && img->shape[3] % g.C == 0 && out->shape[3] > 0 && out->shape[3] % g.F == 0);
  g.T = img->shape[3] / g.C;
  g.Mt = out->shape[3] / g.F;
  CHIP_REQUIRE(g.T >= g.Kt && g.Mt == (g.T - g.Kt) / g.st + 1);
  CHIP_REQUIRE(out->shape[0] == g.N);
  CHIP_REQUIRE(flt->shape[0] == g.F && flt->shape[1] == d.kernel_size_x && flt->shape[2] == d.kernel_size_y && flt->shape[3] == g.C * g.Kt);
  g.K2 = d.kernel_size_x * d.kernel_size_y * g.C;
  g.in_frame = (size_t)g.X * g.Y * g.C;
  g.out_frame = (size_t)g.Mx * g.My * g.F;
  CHIP_REQUIRE(mi->size[0] == g.N && (size_t)mi->size[1] == g.in_frame * g.T);
  CHIP_REQUIRE(mo->size[0] == g.N && (size_t)mo->size[1] == g.out_frame * g.Mt);
  CHIP_REQUIRE(mf->size[0] == g.F && (size_t)mf->size[1] == (size_t)g.K2 * g.Kt);
  g.d2 = d;
  g.d2.kernel_size_t = 1;
  g.d2.stride_t = 1;
  g.d2.num_input_channels = g.C * g.Kt;
  g.d2.input_channel_end = d.input_channel_end ? g.C * g.Kt : 0;
  return g;
}

// `frames` frames of `m`, starting at frame `first`, as a view of its own (the caller's struct is only read)
cudamat frame_view(const cudamat* m, size_t frame_floats, int first, int frames) {
  cudamat v = *m;
  v.data_host = nullptr;
  v.on_host = 0;
  v.owns_data = 0;
  v.is_trans = 0;
  v.data_device = m->data_device + frame_floats * (size_t)m->size[0] * first;
  v.size[1] = (int)(frame_floats * frames);
  return v;
}

Shape4D shape4(int a, int b, int c, int e) {
  Shape4D s;
  s.shape[0] = a; s.shape[1] = b; s.shape[2] = c; s.shape[3] = e;
  return s;
}

void conv3d_up(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets, Shape4D* is, Shape4D* fs, Shape4D* ts, const ConvDesc& d,
               float scaleTargets, int relu) {
  const Geo3D g = geo3d(is, fs, ts, d, images, filters, targets);
  Shape4D is2 = shape4(g.N, g.X, g.Y, g.C * g.Kt), ts2 = shape4(g.N, g.Mx, g.My, g.F);
  (void)stream();   // a parked call goes out before the share scope opens
  filter_planes_share((batch_forms() & 1) != 0);   // the bank's planes / tap-major copy: built by the first frame, shared by all
  for (int m = 0; m < g.Mt; ++m) {
    cudamat iv = frame_view(images, g.in_frame, m * g.st, g.Kt), tv = frame_view(targets, g.out_frame, m, 1);
    convUpBiasAct(&iv, filters, bias, &tv, &is2, fs, &ts2, g.d2, scaleTargets, relu);
  }
  filter_planes_share(false);
}

void conv3d_outp(cudamat* images, cudamat* derivs, cudamat* targets, cudamat* bias_grad, Shape4D* is, Shape4D* ds, Shape4D* ts,
                 const ConvDesc& d, float scaleTargets, float scaleOutput) {
  const Geo3D g = geo3d(is, ts, ds, d, images, targets, derivs);
  Shape4D is2 = shape4(g.N, g.X, g.Y, g.C * g.Kt), ds2 = shape4(g.N, g.Mx, g.My, g.F);
  // ONE reduction (batch_forms() & 2): every frame writes its split-K slabs into one arena and wg_batch_end() sums them and applies
  // scaleTargets / scaleOutput once.  Otherwise, or when the arena would be too large, the frames accumulate into dW one by one.
  (void)stream();
  // (slabs above 128 MiB are not worth an arena: the batched form measured equal to the loop, within 1 % either way, at 223 MB and
  // 446 MB — they no longer fit the last-level cache between the frame launches and the reduction)
  if ((batch_forms() & 2) != 0 && g.Mt > 1) wg_batch_begin(g.Mt, workspace_slabs, size_t(128) << 20);
  for (int m = 0; m < g.Mt; ++m) {
    cudamat iv = frame_view(images, g.in_frame, m * g.st, g.Kt), dv = frame_view(derivs, g.out_frame, m, 1);
    const float stm = (m == 0 || wg_batch_active()) ? scaleTargets : 1.f;
    if (bias_grad) convOutpBias(&iv, &dv, targets, bias_grad, &is2, &ds2, ts, g.d2, stm, scaleOutput);
    else convOutpGemm(&iv, &dv, targets, &is2, &ds2, ts, g.d2, stm, scaleOutput);
  }
  wg_batch_end();
}

void conv3d_down(cudamat* derivs, cudamat* filters, cudamat* state, cudamat* targets, Shape4D* ds, Shape4D* fs, Shape4D* ts,
                 const ConvDesc& d, float scaleTargets, float post_scale) {
  const Geo3D g = geo3d(ts, fs, ds, d, targets, filters, derivs);
  if (state) CHIP_REQUIRE(state->on_device && numel(state) == numel(targets));
  if (g.C % 16 != 0) {
    // Few or ragged input channels: the 2-D dgrad then runs its generic kernel, whose rows are the C channels of ONE frame here but the
    // C·Kt channels of a window in the reference's form — measured 2.8x slower as a gather at C = 3 (profiles/conv3d_bench.json).  So
    // this case ships as the reference's loop: scale once, every output frame accumulates into its window, the mask last.
    const size_t n = g.in_frame * g.N * g.T;
    {
      KernelTimer timer("conv3d_scale_frame_kernel", "conv_dgrad", 0.0, (scaleTargets != 0.f ? 8.0 : 4.0) * n);
      hipLaunchKernelGGL(conv3d_scale_frame_kernel, dim3(grid_for(n)), dim3(256), 0, stream(), targets->data_device, (const float*)nullptr, n,
                         scaleTargets, 1.0f);
    }
    Shape4D ds2 = shape4(g.N, g.Mx, g.My, g.F), ts2 = shape4(g.N, g.X, g.Y, g.C * g.Kt);
    for (int m = 0; m < g.Mt; ++m) {
      cudamat dv = frame_view(derivs, g.out_frame, m, 1), tv = frame_view(targets, g.in_frame, m * g.st, g.Kt);
      convDownMask(&dv, filters, nullptr, &tv, &ds2, fs, &ts2, g.d2, 1.0f, 1.0f);
    }
    if (state) {
      KernelTimer timer("conv3d_scale_frame_kernel", "conv_dgrad", 0.0, 12.0 * n);
      hipLaunchKernelGGL(conv3d_scale_frame_kernel, dim3(grid_for(n)), dim3(256), 0, stream(), targets->data_device,
                         (const float*)state->data_device, n, 1.0f, post_scale);
    }
    return;
  }
  // frame ti gathers from output frames [m_lo, m_hi]; its class is (kt0 = ti - m_lo·st, nv = m_hi - m_lo + 1)
  struct Frame { int m_lo, nv, kt0; };
  std::vector<Frame> frames(g.T);
  std::map<std::pair<int, int>, size_t> bank_off;   // class -> float offset in the bank arena
  size_t bank_floats = 0;
  for (int ti = 0; ti < g.T; ++ti) {
    const int m_hi = std::min(g.Mt - 1, ti / g.st);
    const int m_lo = ti < g.Kt ? 0 : (ti - g.Kt) / g.st + 1;
    Frame& f = frames[ti];
    f.m_lo = m_lo; f.nv = m_hi - m_lo + 1; f.kt0 = ti - m_lo * g.st;
    if (f.nv <= 0) continue;
    CHIP_REQUIRE(f.kt0 < g.Kt && f.kt0 - (f.nv - 1) * g.st >= 0);
    const auto key = std::make_pair(f.kt0, f.nv);
    if (!bank_off.count(key)) {
      bank_off[key] = bank_floats;
      bank_floats += ((size_t)g.F * f.nv * g.K2 + 63) / 64 * 64;
    }
  }
  float* banks = bank_floats ? static_cast<float*>(workspace_banks(sizeof(float) * bank_floats)) : nullptr;
  for (const auto& kv : bank_off) {
    const int kt0 = kv.first.first, nv = kv.first.second;
    const size_t elems = (size_t)g.F * nv * g.K2;
    KernelTimer timer("conv3d_dgrad_bank_kernel", "conv_dgrad", 0.0, 8.0 * elems);
    hipLaunchKernelGGL(conv3d_dgrad_bank_kernel, dim3(grid_for(elems)), dim3(256), 0, stream(), filters->data_device, banks + kv.second, g.F, g.K2,
                       nv, kt0, g.st);
  }
  Shape4D ts2 = shape4(g.N, g.X, g.Y, g.C);
  filter_planes_share((batch_forms() & 1) != 0);   // consecutive frames of one class: the class bank's bf16 planes are built once
  for (int ti = 0; ti < g.T; ++ti) {
    const Frame& f = frames[ti];
    cudamat tv = frame_view(targets, g.in_frame, ti, 1);
    cudamat sv{};
    if (state) sv = frame_view(state, g.in_frame, ti, 1);
    if (f.nv <= 0) {
      const size_t n = g.in_frame * g.N;
      KernelTimer timer("conv3d_scale_frame_kernel", "conv_dgrad", 0.0, (scaleTargets != 0.f ? 8.0 : 4.0) * n);
      hipLaunchKernelGGL(conv3d_scale_frame_kernel, dim3(grid_for(n)), dim3(256), 0, stream(), tv.data_device,
                         state ? (const float*)sv.data_device : nullptr, n, scaleTargets, post_scale);
      continue;
    }
    cudamat dv = frame_view(derivs, g.out_frame, f.m_lo, f.nv);
    cudamat bank{};
    bank.data_device = banks + bank_off[std::make_pair(f.kt0, f.nv)];
    bank.on_device = 1;
    bank.size[0] = g.F * f.nv;
    bank.size[1] = g.K2;
    Shape4D ds2 = shape4(g.N, g.Mx, g.My, g.F * f.nv), fs2 = shape4(g.F * f.nv, d.kernel_size_x, d.kernel_size_y, g.C);
    ConvDesc dc = d;
    dc.kernel_size_t = 1;
    dc.stride_t = 1;
    dc.num_output_channels = g.F * f.nv;
    dc.output_channel_end = d.output_channel_end ? g.F * f.nv : 0;
    convDownMask(&dv, &bank, state ? &sv : nullptr, &tv, &ds2, &fs2, &ts2, dc, scaleTargets, post_scale);
  }
  filter_planes_share(false);
}

cudamat whole_view(const cudamat* m, size_t frame_floats, int t) {
  cudamat v = *m;
  v.data_host = nullptr;
  v.on_host = 0;
  v.owns_data = 0;
  v.data_device = m->data_device + frame_floats * t;
  v.size[0] = (int)frame_floats;   // (rnorm reads only the element count)
  v.size[1] = 1;
  return v;
}

void rnorm3d_fwd(cudamat* images, cudamat* targets, int numFilters, int sizeF, float addScale, float powScale, bool blocked, int T, bool relu) {
  const size_t total = numel(images);
  CHIP_REQUIRE(images->on_device && targets->on_device && T > 0 && numel(targets) == total && total % T == 0);
  const size_t frame = total / T;
  CHIP_REQUIRE(frame < (size_t(1) << 31));
  (void)stream();   // a parked call goes out first
  for (int t = 0; t < T; ++t) {
    cudamat iv = whole_view(images, frame, t), tv = whole_view(targets, frame, t);
    if (relu) ResponseNormCrossMapRelu(&iv, &tv, numFilters, sizeF, addScale, powScale, blocked);
    else ResponseNormCrossMapGemm(&iv, &tv, numFilters, sizeF, addScale, powScale, blocked);
  }
  (void)stream();   // ... and the last frame is not left parked
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" {

void convUp3DGemm(cudamat* images, cudamat* filters, cudamat* targets, Shape4D* is, Shape4D* fs, Shape4D* ts, ConvDesc d, float scaleTargets) {
  conv3d_up(images, filters, nullptr, targets, is, fs, ts, d, scaleTargets, 0);
}

void convUp3DBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets, Shape4D* is, Shape4D* fs, Shape4D* ts, ConvDesc d,
                     float scaleTargets, int relu) {
  if (bias) CHIP_REQUIRE(bias->size[0] * bias->size[1] == d.num_output_channels);
  conv3d_up(images, filters, bias, targets, is, fs, ts, d, scaleTargets, relu);
}

void convDown3DGemm(cudamat* derivs, cudamat* filters, cudamat* targets, Shape4D* ds, Shape4D* fs, Shape4D* ts, ConvDesc d, float scaleTargets) {
  conv3d_down(derivs, filters, nullptr, targets, ds, fs, ts, d, scaleTargets, 1.0f);
}

void convDown3DMask(cudamat* derivs, cudamat* filters, cudamat* state, cudamat* targets, Shape4D* ds, Shape4D* fs, Shape4D* ts, ConvDesc d,
                    float scaleTargets, float post_scale) {
  CHIP_REQUIRE(state != nullptr);
  conv3d_down(derivs, filters, state, targets, ds, fs, ts, d, scaleTargets, post_scale);
}

void convOutp3DGemm(cudamat* images, cudamat* derivs, cudamat* targets, Shape4D* is, Shape4D* ds, Shape4D* ts, ConvDesc d, float scaleTargets,
                    float scaleOutput) {
  conv3d_outp(images, derivs, targets, nullptr, is, ds, ts, d, scaleTargets, scaleOutput);
}

void convOutp3DBias(cudamat* images, cudamat* derivs, cudamat* targets, cudamat* bias_grad, Shape4D* is, Shape4D* ds, Shape4D* ts, ConvDesc d,
                    float scaleTargets, float scaleOutput) {
  CHIP_REQUIRE(bias_grad != nullptr);
  conv3d_outp(images, derivs, targets, bias_grad, is, ds, ts, d, scaleTargets, scaleOutput);
}

void ResponseNormCrossMap3DGemm(cudamat* images, cudamat* targets, int numFilters, int sizeF, float addScale, float powScale, bool blocked,
                                int image_size_t) {
  rnorm3d_fwd(images, targets, numFilters, sizeF, addScale, powScale, blocked, image_size_t, false);
}

void ResponseNormCrossMap3DRelu(cudamat* images, cudamat* targets, int numFilters, int sizeF, float addScale, float powScale, bool blocked,
                                int image_size_t) {
  rnorm3d_fwd(images, targets, numFilters, sizeF, addScale, powScale, blocked, image_size_t, true);
}

void ResponseNormCrossMap3DUndoGemm(cudamat* outGrads, cudamat* inputs, cudamat* targets, int numFilters, int sizeF, float addScale,
                                    float powScale, bool blocked, int image_size_t) {
  const size_t total = numel(inputs);
  const int T = image_size_t;
  CHIP_REQUIRE(outGrads->on_device && inputs->on_device && targets->on_device);
  CHIP_REQUIRE(T > 0 && numel(targets) == total && numel(outGrads) == total && total % T == 0);
  const size_t frame = total / T;
  CHIP_REQUIRE(frame < (size_t(1) << 31));
  for (int t = 0; t < T; ++t) {
    cudamat gv = whole_view(outGrads, frame, t), iv = whole_view(inputs, frame, t), tv = whole_view(targets, frame, t);
    ResponseNormCrossMapUndoGemm(&gv, &iv, &tv, numFilters, sizeF, addScale, powScale, blocked);
  }
}

}  // extern "C"
