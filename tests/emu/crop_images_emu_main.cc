// Runs crop_images_u8 (convnet_amd/csrc/input_staging.hip) FUNCTIONALLY on the CPU — the kernel source compiled as host C++ against
// tests/emu/hip/hip_runtime.h — through the C ABI, against a direct evaluation of the definition in include/convnet_hip.h: resize the
// whole image in two 8-bit passes, crop, mirror, planar.  Crops 1 x 1, 5 x 7, 4 x 8, 3 x 67, 6 x 256 and 2 x 300 at output addresses
// 0 ... 3 past an aligned one, inside a buffer of a fill byte; then tables of random numbers, which must leave every access inside the
// exact-size heap buffers (add -fsanitize=address to both compiles and the link to have that checked).  Prints one line per case; exit
// status 0 only if all pass.  tests/test_crop_images_emulated.py builds and runs it.
#include "crop_images_emu_prelude.h"
#include <cstdio>
#include <random>
#include <vector>
#include "common.h"
namespace chip {
hipStream_t stream() { return nullptr; }
KernelTimer::KernelTimer(const char*, const char*, double, double, double) : slot(-1) {}
KernelTimer::~KernelTimer() {}
}
struct Tap { int s, a0, a1; };
static std::vector<Tap> mk_taps(int ssize, int dsize) {
  std::vector<Tap> t;
  double scale = 1.0 / (dsize / (double)ssize);
  for (int d = 0; d < dsize; ++d) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int s = (int)std::floor(fx);
    fx -= s;
    if (s < 0) { s = 0; fx = 0; }
    if (s >= ssize - 1) { s = ssize - 1; fx = 0; }
    t.push_back({s, (int)std::rint((1.f - fx) * 2048.f), (int)std::rint(fx * 2048.f)});
  }
  return t;
}
static bool run(int W, int H, int N, unsigned seed, int misalign) {
  std::mt19937 rng(seed);
  const int sizes[][2] = {{9, 7}, {6, 8}, {1, 9}, {13, 1}, {150, 40}, {40, 170}, {W, H}};
  const int ni = 7;
  std::vector<unsigned char> bytes(3, 0);
  std::vector<long long> table;
  std::vector<int> taps;
  std::vector<std::vector<unsigned char>> resized;
  std::vector<int> nws, nhs;
  for (int i = 0; i < ni; ++i) {
    int w = sizes[i][0], h = sizes[i][1];
    int new_w, new_h;
    if ((long)W * h < (long)H * w) { new_h = H; new_w = (w * H) / h; } else { new_w = W; new_h = (h * W) / w; }
    size_t off = bytes.size();
    for (int k = 0; k < w * h * 3; ++k) bytes.push_back(rng() & 255);
    auto ct = mk_taps(w, new_w), rt = mk_taps(h, new_h);
    table.insert(table.end(), {(long long)off, w, h, new_w, new_h, (long long)(taps.size() / 3)});
    for (auto& t : ct) taps.insert(taps.end(), {t.s, t.a0, t.a1});
    for (auto& t : rt) taps.insert(taps.end(), {t.s, t.a0, t.a1});
    std::vector<unsigned char> big((size_t)new_w * new_h * 3);
    const unsigned char* p = bytes.data() + off;
    auto hrow = [&](int y, int x, int c) {
      const Tap& t = ct[x];
      int v = p[((size_t)y * w + t.s) * 3 + c] * t.a0 + p[((size_t)y * w + std::min(t.s + 1, w - 1)) * 3 + c] * t.a1;
      return (((2048 * (v >> 4)) >> 16) + 2) >> 2;
    };
    for (int y = 0; y < new_h; ++y)
      for (int x = 0; x < new_w; ++x)
        for (int c = 0; c < 3; ++c) {
          const Tap& t = rt[y];
          int h0 = hrow(t.s, x, c), h1 = hrow(std::min(t.s + 1, h - 1), x, c);
          big[((size_t)y * new_w + x) * 3 + c] = (((t.a0 * ((2048 * h0) >> 4)) >> 16) + ((t.a1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2;
        }
    resized.push_back(big); nws.push_back(new_w); nhs.push_back(new_h);
  }
  std::vector<int> cases;
  const size_t dims = (size_t)3 * H * W;
  std::vector<unsigned char> want(N * dims);
  for (int n = 0; n < N; ++n) {
    int k = rng() % ni, left = rng() % (nws[k] - W + 1), top = rng() % (nhs[k] - H + 1), mir = rng() & 1;
    cases.insert(cases.end(), {k, left, top, mir});
    for (int c = 0; c < 3; ++c) for (int r = 0; r < H; ++r) for (int x = 0; x < W; ++x)
      want[n * dims + ((size_t)c * H + r) * W + x] = resized[k][((size_t)(top + r) * nws[k] + left + (mir ? W - 1 - x : x)) * 3 + c];
  }
  // exact-size heap buffers, so that an address sanitizer sees any overrun; the output starts `misalign` bytes in
  std::vector<unsigned char> b2(bytes), out(N * dims + misalign + 8, 0xAB);   // `misalign` fill bytes in front, 8 behind
  std::vector<long long> t2(table); std::vector<int> tp2(taps), c2(cases);
  int rc = crop_images_u8(b2.data(), b2.size(), t2.data(), ni, tp2.data(), (int)(tp2.size() / 3), c2.data(), N, out.data() + misalign, W, H);
  bool ok = rc == 0;
  for (int i = 0; i < misalign; ++i) ok &= out[i] == 0xAB;
  for (int i = 0; i < 8; ++i) ok &= out[misalign + N * dims + i] == 0xAB;
  size_t bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += out[misalign + i] != want[i];
  ok &= bad == 0;
  // garbage tables: must stay in bounds (ASan) and return 0
  std::vector<int> cg(cases), tg(taps); std::vector<long long> ig(table);
  for (auto& v : cg) v = (int)rng() ; for (auto& v : tg) v = (int)rng(); for (auto& v : ig) v = ((long long)rng() << 32) ^ rng() ^ ((rng() & 1) ? -1LL : 0);
  std::vector<unsigned char> out2(N * dims, 0);
  int rc2 = crop_images_u8(b2.data(), b2.size(), ig.data(), ni, tg.data(), (int)(tg.size() / 3), cg.data(), N, out2.data(), W, H);
  int rc3 = crop_images_u8(b2.data(), b2.size(), t2.data(), ni, tg.data(), (int)(tg.size() / 3), cg.data(), N, out2.data(), W, H);
  ok &= rc2 == 0 && rc3 == 0;
  printf("%s W=%d H=%d N=%d mis=%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", W, H, N, misalign, rc, bad);
  return ok;
}
int main() {
  bool ok = true;
  const int geo[][3] = {{1, 1, 3}, {7, 5, 65}, {8, 4, 65}, {67, 3, 5}, {256, 6, 3}, {300, 2, 2}};   // W, H, cases
  for (auto& g : geo) for (int mis = 0; mis < 4; mis += 1) ok &= run(g[0], g[1], g[2], 7 * g[0] + g[1] + mis, mis);
  unsigned char x; 
  ok &= crop_images_u8(nullptr, 1, &x, 1, &x, 1, &x, 1, &x, 1, 1) == ERROR_GENERIC;
  ok &= crop_images_u8(&x, 0, &x, 1, &x, 1, &x, 1, &x, 1, 1) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= crop_images_u8(&x, 1, &x, (1 << 24) + 1, &x, 1, &x, 1, &x, 1, 1) == ERROR_UNSUPPORTED;
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return !ok;
}
