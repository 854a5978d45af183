// Runs the locally connected layer kernels (convnet_amd/csrc/local_conv.hip) FUNCTIONALLY on the CPU — compiled as host C++ against
// tests/emu/hip/hip_runtime.h — through the C ABI on small ragged problems, on both matrix paths, against a direct double-precision
// evaluation of the definition (include/convnet_hip.h, "locally connected layers").  Prints one line per case; exit status 0 only if
// all pass.  tests/test_local_emulated.py builds and runs it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../convnet_amd/csrc/gather_gemm.h"

struct G {
  int N, C, H, W, F, Ky, Kx, sy, sx, py, px;   // py / px >= 0 (pbtxt padding)
  int My() const { return (H + 2 * py - Ky) / sy + 1; }
  int Mx() const { return (W + 2 * px - Kx) / sx + 1; }
};

static cudamat mat(std::vector<float>& v, int rows, int cols) {
  cudamat m = {};
  m.data_device = v.data();
  m.on_device = 1;
  m.size[0] = rows;
  m.size[1] = cols;
  return m;
}

static double rel(const std::vector<float>& a, const std::vector<double>& b) {
  double num = 0, den = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    num += (a[i] - b[i]) * (a[i] - b[i]);
    den += b[i] * b[i];
  }
  return std::sqrt(num / (den > 0 ? den : 1));
}

static bool run(const G& g, int path, float st, float so) {
  convnet_hip_set_matrix_path(path);
  const int My = g.My(), Mx = g.Mx(), M = My * Mx, K = g.C * g.Ky * g.Kx;
  std::mt19937 rng(g.N * 131 + g.C * 7 + path);
  std::normal_distribution<float> nd;
  std::vector<float> x((size_t)g.N * g.H * g.W * g.C), w((size_t)g.F * K * M + 64), dy((size_t)g.N * M * g.F);
  for (auto& v : x) v = nd(rng);
  for (auto& v : w) v = nd(rng);
  for (auto& v : dy) v = nd(rng);
  std::vector<float> out(dy.size()), dx(x.size()), dw(w.size());
  for (auto& v : out) v = nd(rng);
  for (auto& v : dx) v = nd(rng);
  for (auto& v : dw) v = nd(rng);
  const std::vector<float> out0 = out, dx0 = dx, dw0 = dw;
  std::vector<double> rout(out.size()), rdx(dx.size()), rdw((size_t)g.F * K * M);
  for (size_t i = 0; i < rout.size(); ++i) rout[i] = st * out0[i];
  for (size_t i = 0; i < rdx.size(); ++i) rdx[i] = st * dx0[i];
  for (size_t i = 0; i < rdw.size(); ++i) rdw[i] = st * dw0[i];
  for (int my = 0; my < My; ++my)
    for (int mx = 0; mx < Mx; ++mx)
      for (int c = 0; c < g.C; ++c)
        for (int ky = 0; ky < g.Ky; ++ky)
          for (int kx = 0; kx < g.Kx; ++kx) {
            const int iy = my * g.sy + ky - g.py, ix = mx * g.sx + kx - g.px;
            if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
            const int m = my * Mx + mx, k = kx + g.Kx * (ky + g.Ky * c);
            for (int f = 0; f < g.F; ++f) {
              const size_t wi = (size_t)m * g.F * K + f + (size_t)g.F * k;
              for (int n = 0; n < g.N; ++n) {
                const size_t xi = n + (size_t)g.N * (ix + g.W * (iy + (size_t)g.H * c)), oi = n + (size_t)g.N * (m + (size_t)M * f);
                rout[oi] += (double)w[wi] * x[xi];
                rdx[xi] += (double)w[wi] * dy[oi];
                rdw[wi] += (double)so * dy[oi] * x[xi];
              }
            }
          }
  Shape4D is = {{g.N, g.W, g.H, g.C}}, os = {{g.N, Mx, My, g.F}}, fs = {{g.F, g.Kx, g.Ky, g.C * M}};
  ConvDesc d = {};
  d.num_input_channels = g.C; d.num_output_channels = g.F; d.kernel_size_y = g.Ky; d.kernel_size_x = g.Kx; d.kernel_size_t = 1;
  d.stride_y = g.sy; d.stride_x = g.sx; d.stride_t = 1; d.padding_y = -g.py; d.padding_x = -g.px; d.num_groups = 1;
  cudamat mx_ = mat(x, g.N, g.H * g.W * g.C), mw = mat(w, g.F, K * M), mdy = mat(dy, g.N, M * g.F);
  cudamat mo = mat(out, g.N, M * g.F), mdx = mat(dx, g.N, g.H * g.W * g.C), mdw = mat(dw, g.F, K * M);
  localUpGemm(&mx_, &mw, &mo, &is, &fs, &os, d, st);
  localDownGemm(&mdy, &mw, &mdx, &os, &fs, &is, d, st);
  localOutpGemm(&mx_, &mdy, &mdw, &is, &os, &fs, d, st, so);
  bool guard = true;   // the 64 floats after the bank must be untouched
  for (size_t i = rdw.size(); i < dw.size(); ++i) guard &= dw[i] == dw0[i];
  std::vector<float> dwb(dw.begin(), dw.begin() + rdw.size());
  const double e0 = rel(out, rout), e1 = rel(dx, rdx), e2 = rel(dwb, rdw);
  const bool ok = e0 < 1e-5 && e1 < 1e-5 && e2 < 1e-5 && guard;
  printf("%s local path=%d N=%d C=%d %dx%d F=%d k%dx%d s%dx%d p%dx%d st=%g so=%g: up %.2e down %.2e outp %.2e guard %d\n", ok ? "PASS" : "FAIL",
         path, g.N, g.C, g.H, g.W, g.F, g.Ky, g.Kx, g.sy, g.sx, g.py, g.px, st, so, e0, e1, e2, (int)guard);
  return ok;
}

int main() {
  const G geoms[] = {
      {6, 3, 7, 6, 7, 3, 2, 2, 1, 1, 0},      // N % 4 != 0, C = 3, F % 4 != 0, rectangular
      {33, 4, 5, 5, 17, 3, 3, 1, 1, 1, 1},    // two column tiles of a wave, two row tiles
      {5, 2, 9, 9, 3, 2, 2, 3, 3, 0, 0},      // stride > kernel
  };
  bool ok = true;
  for (const G& g : geoms)
    for (int path = 0; path < 2; ++path) ok &= run(g, path, path ? 1.f : 0.f, path ? 0.5f : 1.f);
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return ok ? 0 : 1;
}
