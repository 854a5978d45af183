// Runs the new code of convnet_amd/csrc/conv3d.hip FUNCTIONALLY on the CPU — compiled as host C++ against tests/emu/hip/hip_runtime.h —
// through the C ABI: the 3-D entries' frame slicing, the time gather of convDown3DGemm with conv3d_dgrad_bank_kernel's class banks and
// conv3d_scale_frame_kernel, the frame accumulation of convOutp3DGemm, and, through the pooling entries of pool_norm.hip, pool3d_fwd_kernel / pool3d_undo_kernel.  The 2-D CONVOLUTION entries the
// 3-D ones launch per frame are replaced here by plain loops over the 2-D definition (they are tested on their own), so what is under
// test is exactly what conv3d.hip adds.  Reference: a direct double-precision evaluation of the 3-D definitions (include/convnet_hip.h).
// Convolution operands are small integers, so every sum is exact in fp32 and dgrad (bank re-layout) and max pooling compare EXACTLY.
// Prints one line per case; exit status 0 only if all pass.  tests/test_conv3d_emulated.py builds and runs it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../convnet_amd/csrc/common.h"

namespace chip {
alignas(16) float rn_smem[40960];   // pool_norm.hip's dynamic LDS array (160 KB: the block's LDS)
// This program replaces gather_gemm.hip on purpose (the 2-D entries below), so what that file defines beside them is defined here: the
// hooks conv3d.hip holds around its frame launches.  Everything else it needs of the library is the real state.hip.
void filter_planes_share(bool) {}
void wg_batch_begin(int, void* (*)(size_t), size_t) {}
bool wg_batch_active() { return false; }
int wg_batch_frame() { return 0; }
void wg_batch_end() {}
}  // namespace chip

// ---- the 2-D entries conv3d.hip launches per frame, as plain loops over their definition ----------------------------------------------
struct G2 {
  int N, C, H, W, F, Ky, Kx, sy, sx, py, px, My, Mx;   // py / px: ConvDesc (negated) padding
};
static G2 g2_of(const Shape4D* img, const Shape4D* out, const ConvDesc& d) {
  G2 g{img->shape[0], img->shape[3], img->shape[2], img->shape[1], out->shape[3], d.kernel_size_y, d.kernel_size_x, d.stride_y, d.stride_x,
       d.padding_y, d.padding_x, out->shape[2], out->shape[1]};
  if (d.num_input_channels != g.C || d.num_output_channels != g.F || d.kernel_size_t != 1) {
    printf("FAIL 2-D stub: descriptor does not match the slice shapes\n");
    exit(1);
  }
  return g;
}
template <typename Fn>
static void taps2(const G2& g, Fn fn) {   // fn(x index / N, w index, out index / N)
  for (int my = 0; my < g.My; ++my)
    for (int mx = 0; mx < g.Mx; ++mx)
      for (int c = 0; c < g.C; ++c)
        for (int ky = 0; ky < g.Ky; ++ky)
          for (int kx = 0; kx < g.Kx; ++kx) {
            const int iy = my * g.sy + ky + g.py, ix = mx * g.sx + kx + g.px;
            if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
            for (int f = 0; f < g.F; ++f)
              fn((size_t)ix + g.W * (iy + (size_t)g.H * c), (size_t)f + (size_t)g.F * (kx + g.Kx * (ky + g.Ky * c)),
                 (size_t)mx + g.Mx * (my + (size_t)g.My * f));
          }
}

extern "C" {
void convUpBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets, Shape4D* is, Shape4D* fs, Shape4D* ts, ConvDesc d,
                   float st, int relu) {
  const G2 g = g2_of(is, ts, d);
  std::vector<double> acc((size_t)g.N * g.My * g.Mx * g.F, 0.0);
  taps2(g, [&](size_t xi, size_t wi, size_t oi) {
    for (int n = 0; n < g.N; ++n) acc[n + g.N * oi] += (double)filters->data_device[wi] * images->data_device[n + g.N * xi];
  });
  for (size_t i = 0; i < acc.size(); ++i) {
    float v = (st != 0.f ? st * targets->data_device[i] : 0.f) + (float)acc[i];
    if (bias) v += bias->data_device[i / ((size_t)g.N * g.My * g.Mx)];
    targets->data_device[i] = relu ? (v > 0.f ? v : 0.f) : v;
  }
}
void convDownMask(cudamat* derivs, cudamat* filters, cudamat* state, cudamat* targets, Shape4D* ds, Shape4D* fs, Shape4D* ts, ConvDesc d,
                  float st, float post_scale) {
  const G2 g = g2_of(ts, ds, d);
  if (filters->size[0] != g.F || filters->size[1] != g.C * g.Ky * g.Kx || fs->shape[0] != g.F || fs->shape[3] != g.C) {
    printf("FAIL 2-D stub: class bank shape\n");
    exit(1);
  }
  std::vector<double> acc((size_t)g.N * g.H * g.W * g.C, 0.0);
  taps2(g, [&](size_t xi, size_t wi, size_t oi) {
    for (int n = 0; n < g.N; ++n) acc[n + g.N * xi] += (double)filters->data_device[wi] * derivs->data_device[n + g.N * oi];
  });
  for (size_t i = 0; i < acc.size(); ++i) {
    float v = (st != 0.f ? st * targets->data_device[i] : 0.f) + (float)acc[i];
    if (state) v = state->data_device[i] > 0.f ? v * post_scale : 0.f;
    targets->data_device[i] = v;
  }
}
void convOutpBias(cudamat* images, cudamat* derivs, cudamat* targets, cudamat* bias_grad, Shape4D* is, Shape4D* ds, Shape4D* ts, ConvDesc d,
                  float st, float so) {
  const G2 g = g2_of(is, ds, d);
  std::vector<double> acc((size_t)g.F * g.C * g.Ky * g.Kx, 0.0);
  taps2(g, [&](size_t xi, size_t wi, size_t oi) {
    for (int n = 0; n < g.N; ++n) acc[wi] += (double)derivs->data_device[n + g.N * oi] * images->data_device[n + g.N * xi];
  });
  for (size_t i = 0; i < acc.size(); ++i) targets->data_device[i] = (st != 0.f ? st * targets->data_device[i] : 0.f) + so * (float)acc[i];
  if (bias_grad)
    for (int f = 0; f < g.F; ++f) {
      double s = 0;
      for (size_t i = 0; i < (size_t)g.N * g.My * g.Mx; ++i) s += derivs->data_device[i + (size_t)g.N * g.My * g.Mx * f];
      bias_grad->data_device[f] = (st != 0.f ? st * bias_grad->data_device[f] : 0.f) + so * (float)s;
    }
}
void convOutpGemm(cudamat* images, cudamat* derivs, cudamat* targets, Shape4D* is, Shape4D* ds, Shape4D* ts, ConvDesc d, float st, float so) {
  convOutpBias(images, derivs, targets, nullptr, is, ds, ts, d, st, so);
}
}

// ---- the 3-D cases ------------------------------------------------------------------------------------------------------------------------
struct G3 {
  int N, C, H, W, T, F, Ky, Kx, Kt, sy, sx, st, py, px;   // py / px >= 0 (pbtxt padding)
  int My() const { return (H + 2 * py - Ky) / sy + 1; }
  int Mx() const { return (W + 2 * px - Kx) / sx + 1; }
  int Mt() const { return (T - Kt) / st + 1; }
};

static cudamat mat(std::vector<float>& v, int rows, size_t cols, size_t skip = 0) {
  cudamat m = {};
  m.data_device = v.data() + skip;
  m.on_device = 1;
  m.size[0] = rows;
  m.size[1] = (int)cols;
  return m;
}

static const size_t GUARD = 64;

static bool run_conv(const G3& g, float st, float so, bool masked) {
  const int My = g.My(), Mx = g.Mx(), Mt = g.Mt(), K2 = g.Kx * g.Ky * g.C;
  const size_t in_el = (size_t)g.N * g.W * g.H * g.C * g.T, out_el = (size_t)g.N * Mx * My * g.F * Mt, w_el = (size_t)g.F * K2 * g.Kt;
  std::mt19937 rng(g.N * 131 + g.T * 7 + g.Kt);
  std::uniform_int_distribution<int> id(-3, 3);
  auto fill = [&](std::vector<float>& v) { for (auto& e : v) e = (float)id(rng); };
  std::vector<float> x(in_el), w(w_el), dy(out_el), state(in_el), bias(g.F);
  fill(x); fill(w); fill(dy); fill(state); fill(bias);
  // outputs with guard regions before and after
  std::vector<float> out(out_el + 2 * GUARD), dx(in_el + 2 * GUARD), dw(w_el + 2 * GUARD), db(g.F + 2 * GUARD);
  fill(out); fill(dx); fill(dw); fill(db);
  const std::vector<float> out0 = out, dx0 = dx, dw0 = dw, db0 = db;
  std::vector<double> rout(out_el), rdx(in_el), rdw(w_el), rdb(g.F);
  for (size_t i = 0; i < out_el; ++i) rout[i] = st * out0[GUARD + i];
  for (size_t i = 0; i < in_el; ++i) rdx[i] = st * dx0[GUARD + i];
  for (size_t i = 0; i < w_el; ++i) rdw[i] = st * dw0[GUARD + i];
  for (int f = 0; f < g.F; ++f) rdb[f] = st * db0[GUARD + f];
  for (int m = 0; m < Mt; ++m)
    for (int kt = 0; kt < g.Kt; ++kt)
      for (int my = 0; my < My; ++my)
        for (int mx = 0; mx < Mx; ++mx)
          for (int c = 0; c < g.C; ++c)
            for (int ky = 0; ky < g.Ky; ++ky)
              for (int kx = 0; kx < g.Kx; ++kx) {
                const int iy = my * g.sy + ky - g.py, ix = mx * g.sx + kx - g.px, t = m * g.st + kt;
                if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
                for (int f = 0; f < g.F; ++f) {
                  const size_t wi = f + (size_t)g.F * (kx + g.Kx * (ky + g.Ky * (c + (size_t)g.C * kt)));
                  for (int n = 0; n < g.N; ++n) {
                    const size_t xi = n + (size_t)g.N * (ix + g.W * (iy + (size_t)g.H * (c + (size_t)g.C * t)));
                    const size_t oi = n + (size_t)g.N * (mx + Mx * (my + (size_t)My * (f + (size_t)g.F * m)));
                    rout[oi] += (double)w[wi] * x[xi];
                    rdx[xi] += (double)w[wi] * dy[oi];
                    rdw[wi] += (double)so * dy[oi] * x[xi];
                  }
                }
              }
  for (size_t i = 0; i < out_el; ++i) {
    const int f = (int)((i / ((size_t)g.N * Mx * My)) % g.F);
    if (masked) rout[i] = std::fmax(rout[i] + bias[f], 0.0);   // the fused forward: bias and ReLU
    rdb[f] += (double)so * dy[i];
  }
  if (masked)
    for (size_t i = 0; i < in_el; ++i) rdx[i] = state[i] > 0.f ? 0.5 * rdx[i] : 0.0;
  Shape4D is = {{g.N, g.W, g.H, g.C * g.T}}, os = {{g.N, Mx, My, g.F * Mt}}, fs = {{g.F, g.Kx, g.Ky, g.C * g.Kt}};
  ConvDesc d = {};
  d.num_input_channels = g.C; d.num_output_channels = g.F; d.kernel_size_y = g.Ky; d.kernel_size_x = g.Kx; d.kernel_size_t = g.Kt;
  d.stride_y = g.sy; d.stride_x = g.sx; d.stride_t = g.st; d.padding_y = -g.py; d.padding_x = -g.px; d.num_groups = 1;
  d.input_channel_end = g.C; d.output_channel_end = g.F;
  cudamat mx_ = mat(x, g.N, in_el / g.N), mw = mat(w, g.F, (size_t)K2 * g.Kt), mdy = mat(dy, g.N, out_el / g.N), ms = mat(state, g.N, in_el / g.N);
  cudamat mo = mat(out, g.N, out_el / g.N, GUARD), mdx = mat(dx, g.N, in_el / g.N, GUARD), mdw = mat(dw, g.F, (size_t)K2 * g.Kt, GUARD);
  cudamat mb = mat(bias, 1, g.F), mdb = mat(db, 1, g.F, GUARD);
  const cudamat keep[4] = {mx_, mw, mdy, mdx};
  if (masked) {
    convUp3DBiasAct(&mx_, &mw, &mb, &mo, &is, &fs, &os, d, st, 1);
    convDown3DMask(&mdy, &mw, &ms, &mdx, &os, &fs, &is, d, st, 0.5f);
    convOutp3DBias(&mx_, &mdy, &mdw, &mdb, &is, &os, &fs, d, st, so);
  } else {
    convUp3DGemm(&mx_, &mw, &mo, &is, &fs, &os, d, st);
    convDown3DGemm(&mdy, &mw, &mdx, &os, &fs, &is, d, st);
    convOutp3DGemm(&mx_, &mdy, &mdw, &is, &os, &fs, d, st, so);
  }
  const cudamat now[4] = {mx_, mw, mdy, mdx};
  const bool structs = std::memcmp(keep, now, sizeof keep) == 0;   // the caller's structs are never written
  bool guard = true;
  auto guards = [&](const std::vector<float>& a, const std::vector<float>& a0, size_t n) {
    for (size_t i = 0; i < GUARD; ++i) guard &= a[i] == a0[i] && a[GUARD + n + i] == a0[GUARD + n + i];
  };
  guards(out, out0, out_el); guards(dx, dx0, in_el); guards(dw, dw0, w_el);
  if (masked) guards(db, db0, g.F);
  size_t bad_up = 0, bad_down = 0, bad_outp = 0, bad_db = 0;
  for (size_t i = 0; i < out_el; ++i) bad_up += (double)out[GUARD + i] != rout[i];
  for (size_t i = 0; i < in_el; ++i) bad_down += (double)dx[GUARD + i] != rdx[i];
  for (size_t i = 0; i < w_el; ++i) bad_outp += (double)dw[GUARD + i] != rdw[i];
  if (masked)
    for (int f = 0; f < g.F; ++f) bad_db += (double)db[GUARD + f] != rdb[f];
  const bool ok = structs && guard && !bad_up && !bad_down && !bad_outp && !bad_db;
  printf("%s conv3d %s N=%d C=%d %dx%dx%d F=%d k%dx%dx%d s%dx%dx%d p%dx%d st=%g so=%g: mismatches up %zu down %zu outp %zu db %zu guard %d structs %d\n",
         ok ? "PASS" : "FAIL", masked ? "fused" : "plain", g.N, g.C, g.H, g.W, g.T, g.F, g.Ky, g.Kx, g.Kt, g.sy, g.sx, g.st, g.py, g.px, st, so,
         bad_up, bad_down, bad_outp, bad_db, (int)guard, (int)structs);
  return ok;
}

static bool run_rnorm() {
  // the 3-D entries against the 2-D entries (the real kernels of pool_norm.hip) on each frame's slice: bit for bit
  const int N = 4, C = 6, frame = N * 3 * 5 * C, T = 4;   // frame = N x (X Y C) floats
  std::vector<float> x((size_t)frame * T), dy(x.size()), y(x.size() + 2 * GUARD, 7.f), yr = y, dx = y, y2(x.size()), yr2(x.size()), dx2(x.size());
  std::mt19937 rng(5);
  std::normal_distribution<float> nd;
  for (auto& e : x) e = nd(rng);
  for (auto& e : dy) e = nd(rng);
  cudamat mx_ = mat(x, N, x.size() / N), mdy = mat(dy, N, x.size() / N), my = mat(y, N, x.size() / N, GUARD), myr = mat(yr, N, x.size() / N, GUARD),
          mdx = mat(dx, N, x.size() / N, GUARD);
  ResponseNormCrossMap3DGemm(&mx_, &my, C, 3, 0.1f, 0.75f, false, T);
  ResponseNormCrossMap3DRelu(&mx_, &myr, C, 3, 0.1f, 0.75f, false, T);
  ResponseNormCrossMap3DUndoGemm(&mdy, &mx_, &mdx, C, 3, 0.1f, 0.75f, false, T);
  for (int t = 0; t < T; ++t) {
    const size_t o = (size_t)frame * t;
    cudamat fx = mat(x, N, frame / N, o), fdy = mat(dy, N, frame / N, o), fy = mat(y2, N, frame / N, o), fyr = mat(yr2, N, frame / N, o),
            fdx = mat(dx2, N, frame / N, o);
    ResponseNormCrossMapGemm(&fx, &fy, C, 3, 0.1f, 0.75f, false);
    ResponseNormCrossMapRelu(&fx, &fyr, C, 3, 0.1f, 0.75f, false);
    ResponseNormCrossMapUndoGemm(&fdy, &fx, &fdx, C, 3, 0.1f, 0.75f, false);
  }
  bool ok = mx_.size[1] == (int)(x.size() / N) && mx_.data_device == x.data();
  bool moved = false;
  for (size_t i = 0; i < x.size(); ++i) {
    ok &= y[GUARD + i] == y2[i] && yr[GUARD + i] == yr2[i] && dx[GUARD + i] == dx2[i];
    moved |= y2[i] != x[i] && y2[i] != 0.f;
  }
  for (size_t i = 0; i < GUARD; ++i) ok &= y[i] == 7.f && y[GUARD + x.size() + i] == 7.f && dx[i] == 7.f && dx[GUARD + x.size() + i] == 7.f;
  ok &= moved;
  printf("%s rnorm3d frame walk\n", ok ? "PASS" : "FAIL");
  return ok;
}

struct P3 {
  int N, C, H, W, T, Ky, Kx, Kt, sy, sx, st, py, px, pt;   // paddings >= 0 (pbtxt)
};

static bool run_pool(const P3& p, float st, bool vec) {
  struct { int N, C, H, W, T, Ky, Kx, Kt, sy, sx, st, py, px, pt, My, Mx, Mt, nvec; } g{};
  g.N = p.N; g.C = p.C; g.H = p.H; g.W = p.W; g.T = p.T; g.Ky = p.Ky; g.Kx = p.Kx; g.Kt = p.Kt; g.sy = p.sy; g.sx = p.sx; g.st = p.st;
  g.py = -p.py; g.px = -p.px; g.pt = -p.pt;
  g.My = (p.H + 2 * p.py - p.Ky) / p.sy + 1; g.Mx = (p.W + 2 * p.px - p.Kx) / p.sx + 1; g.Mt = (p.T + 2 * p.pt - p.Kt) / p.st + 1;
  g.nvec = (p.N + 3) / 4;
  const size_t in_el = (size_t)p.N * p.W * p.H * p.C * p.T, out_el = (size_t)p.N * g.Mx * g.My * p.C * g.Mt;
  std::mt19937 rng(p.N * 31 + p.T);
  std::uniform_int_distribution<int> id(-3, 3);   // small integers: many ties, exact sums
  alignas(16) static float xs[1 << 16], dys[1 << 16];
  if (in_el + 8 > (1 << 16)) return false;
  float* x = xs + (vec ? 0 : 1);   // the scalar path must cope with unaligned tensors
  float* dy = dys + (vec ? 0 : 1);
  for (size_t i = 0; i < in_el; ++i) x[i] = (float)id(rng);
  for (size_t i = 0; i < out_el; ++i) dy[i] = (float)id(rng);
  std::vector<float> ymax(out_el + 2 * GUARD, 9.f), yavg = ymax, dmax(in_el + 2 * GUARD, 9.f), davg = dmax, dmax0 = dmax;
  for (auto& e : dmax) e = (float)id(rng);
  davg = dmax0 = dmax;
  std::vector<double> rmax(out_el, -1e30), ravg(out_el, 0.0), rdmax(in_el), rdavg(in_el);
  for (size_t i = 0; i < in_el; ++i) rdmax[i] = rdavg[i] = st * dmax0[GUARD + i];
  auto xi = [&](int n, int ix, int iy, int c, int t) { return n + (size_t)p.N * (ix + p.W * (iy + (size_t)p.H * (c + (size_t)p.C * t))); };
  auto oi = [&](int n, int mx, int my, int c, int mt) { return n + (size_t)p.N * (mx + g.Mx * (my + (size_t)g.My * (c + (size_t)p.C * mt))); };
  for (int pass = 0; pass < 2; ++pass)
    for (int mt = 0; mt < g.Mt; ++mt)
      for (int my = 0; my < g.My; ++my)
        for (int mx = 0; mx < g.Mx; ++mx) {
          const int t0 = std::max(0, mt * p.st - p.pt), t1 = std::min(p.T, mt * p.st - p.pt + p.Kt);
          const int y0 = std::max(0, my * p.sy - p.py), y1 = std::min(p.H, my * p.sy - p.py + p.Ky);
          const int x0 = std::max(0, mx * p.sx - p.px), x1 = std::min(p.W, mx * p.sx - p.px + p.Kx);
          const double size = (double)(t1 - t0) * (y1 - y0) * (x1 - x0);
          for (int c = 0; c < p.C; ++c)
            for (int n = 0; n < p.N; ++n) {
              const size_t o = oi(n, mx, my, c, mt);
              for (int t = t0; t < t1; ++t)
                for (int y = y0; y < y1; ++y)
                  for (int xx = x0; xx < x1; ++xx) {
                    const size_t i = xi(n, xx, y, c, t);
                    if (pass == 0) {
                      rmax[o] = std::fmax(rmax[o], x[i]);
                      ravg[o] += x[i] / size;
                    } else {
                      if ((double)x[i] == rmax[o]) rdmax[i] += dy[o];
                      rdavg[i] += dy[o] / size;
                    }
                  }
            }
        }
  // through the pooling entries: shape[3] = C*T with C = num_input_channels sends them to pool3d_fwd_kernel / pool3d_undo_kernel
  Shape4D is = {{p.N, p.W, p.H, p.C * p.T}}, os = {{p.N, g.Mx, g.My, p.C * g.Mt}};
  ConvDesc d = {};
  d.num_input_channels = d.num_output_channels = p.C; d.kernel_size_y = p.Ky; d.kernel_size_x = p.Kx; d.kernel_size_t = p.Kt;
  d.stride_y = p.sy; d.stride_x = p.sx; d.stride_t = p.st; d.padding_y = -p.py; d.padding_x = -p.px; d.padding_t = -p.pt; d.num_groups = 1;
  auto view = [&](float* ptr, size_t el) {
    cudamat m = {};
    m.data_device = ptr; m.on_device = 1; m.size[0] = p.N; m.size[1] = (int)(el / p.N);
    return m;
  };
  cudamat mx_ = view(x, in_el), mdy = view(dy, out_el), mymax = view(ymax.data() + GUARD, out_el), myavg = view(yavg.data() + GUARD, out_el),
          mdmax = view(dmax.data() + GUARD, in_el), mdavg = view(davg.data() + GUARD, in_el);
  MaxPoolGemm(&mx_, &mymax, &is, &os, d, 0.f, 1.f);
  AvgPoolGemm(&mx_, &myavg, &is, &os, d, 0.f, 1.f);
  MaxPoolUndoGemm(&mx_, &mdy, &mymax, &mdmax, &is, &os, d, st);
  AvgPoolUndoGemm(&mdy, &mdavg, &os, &is, d, st);
  size_t bad_max = 0, bad_dmax = 0;
  double e_avg = 0, e_davg = 0;
  for (size_t i = 0; i < out_el; ++i) {
    bad_max += (double)ymax[GUARD + i] != rmax[i];
    e_avg = std::fmax(e_avg, std::fabs(yavg[GUARD + i] - ravg[i]));
  }
  for (size_t i = 0; i < in_el; ++i) {
    bad_dmax += (double)dmax[GUARD + i] != rdmax[i];
    e_davg = std::fmax(e_davg, std::fabs(davg[GUARD + i] - rdavg[i]));
  }
  bool guard = true;
  for (size_t i = 0; i < GUARD; ++i)
    guard &= ymax[i] == 9.f && ymax[GUARD + out_el + i] == 9.f && yavg[i] == 9.f && yavg[GUARD + out_el + i] == 9.f && dmax[i] == dmax0[i] &&
             dmax[GUARD + in_el + i] == dmax0[GUARD + in_el + i] && davg[i] == dmax0[i] && davg[GUARD + in_el + i] == dmax0[GUARD + in_el + i];
  // averages of integers in [-3, 3] over at most a few hundred elements: |values| <= 3 + |targets|, fp32 rounding ~1e-6
  const bool ok = !bad_max && !bad_dmax && e_avg < 1e-5 && e_davg < 1e-5 && guard;
  printf("%s pool3d N=%d C=%d %dx%dx%d k%dx%dx%d s%dx%dx%d p%dx%dx%d st=%g vec=%d: max mismatches fwd %zu undo %zu, avg err fwd %.2e undo %.2e guard %d\n",
         ok ? "PASS" : "FAIL", p.N, p.C, p.H, p.W, p.T, p.Ky, p.Kx, p.Kt, p.sy, p.sx, p.st, p.py, p.px, p.pt, st, (int)vec, bad_max, bad_dmax, e_avg,
         e_davg, (int)guard);
  return ok;
}

int main() {
  const G3 convs[] = {
      // C % 16 == 0: dgrad is the time gather over class banks
      {3, 16, 5, 4, 5, 3, 3, 2, 3, 2, 1, 1, 1, 0},   // st 1: every class of a Kt = 3 window, clipped ends
      {2, 16, 4, 4, 7, 2, 2, 2, 2, 1, 1, 2, 0, 0},   // ragged T: the last frame is never read
      {4, 16, 3, 3, 8, 3, 1, 1, 2, 1, 1, 3, 0, 0},   // st > Kt: uncovered frames in the middle and at the end
      {1, 32, 4, 5, 9, 2, 3, 3, 5, 2, 2, 2, 1, 1},   // Kt = 5, st = 2
      // other C: dgrad is the accumulating loop
      {2, 2, 3, 3, 4, 2, 2, 2, 4, 1, 1, 1, 0, 0},    // Kt = T: one output frame
      {2, 2, 4, 4, 6, 3, 3, 3, 1, 1, 1, 1, 1, 1},    // Kt = 1
      {2, 1, 3, 3, 11, 2, 2, 2, 3, 1, 1, 3, 0, 0},   // st = Kt: disjoint windows, ragged end
  };
  bool ok = true;
  int i = 0;
  for (const G3& g : convs) {
    ok &= run_conv(g, (i & 1) ? 1.f : 0.f, (i & 1) ? 0.5f : 1.f, false);
    ok &= run_conv(g, (i & 1) ? 0.f : 1.f, 0.25f, true);
    ++i;
  }
  ok &= run_rnorm();
  const P3 pools[] = {
      {4, 2, 6, 5, 7, 3, 2, 3, 2, 1, 2, 1, 0, 1},    // padded and clipped in time and y
      {5, 3, 5, 5, 6, 2, 2, 2, 2, 2, 2, 0, 0, 0},    // N % 4 != 0
      {8, 1, 4, 4, 9, 3, 3, 2, 1, 1, 3, 1, 1, 0},    // stride_t > kernel_size_t: frames nobody pools
      {4, 2, 3, 3, 5, 3, 3, 5, 3, 3, 1, 0, 0, 0},    // one box over everything
      {4, 2, 5, 4, 6, 3, 3, 1, 2, 2, 2, 0, 0, 0},    // Kt = 1 with a time stride
  };
  i = 0;
  for (const P3& p : pools) {
    ok &= run_pool(p, (i & 1) ? 1.f : 0.f, p.N % 4 == 0);
    if (p.N % 4 == 0) ok &= run_pool(p, (i & 1) ? 0.f : 1.f, false);
    ++i;
  }
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return ok ? 0 : 1;
}
