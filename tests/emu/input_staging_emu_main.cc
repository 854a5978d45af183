// Runs the four byte-staging entries of convnet_amd/csrc/input_staging.hip FUNCTIONALLY on the CPU — the kernel source compiled as host
// C++ against tests/emu/hip/hip_runtime.h — through the C ABI, each against a direct scalar evaluation of its definition in
// include/convnet_hip.h, exact to the bit.
// * crop_images_u8: resize the whole image in two 8-bit passes, crop, mirror, planar.  Crops 1 x 1, 5 x 7, 4 x 8, 3 x 67, 6 x 256 and
//   2 x 300 at output addresses 0 ... 3 past an aligned one, inside a buffer of a fill byte; then tables of random numbers, which must
//   leave every access inside the exact-size heap buffers.
// * stage_images_u8: the same tables and crops (5 x 7 and 3 x 67, 3 and 65 cases) taken through the float cast, mean / std and a
//   jittered patch smaller than the crop, in all four (norm, jitter) builds; then the tables of random numbers.
// * stage_patches_u8 and stage_clips_u8 (clips of 3 frames, both grid modes): 3 colours of 5 x 70 into patches of 4 x 66 — wider than
//   the 64-column tile — for 1, 5, 37, 64 and 68 cases (a narrow tile, a wide one that is no multiple of 4, a full one on the 16-byte
//   store path, a second tile), all four builds; offsets from 0 to the maximum, flip values on both sides of 0.5, repeated columns.
// * the entries' error codes.
// Add -fsanitize=address to every compile and the link to have the buffer bounds checked.  Prints one line per case; exit status 0 only
// if all pass.  tests/test_input_staging_emulated.py builds and runs it.
#include "input_staging_emu_prelude.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "common.h"
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
static cudamat mat(std::vector<float>& v, int rows, int cols) {
  cudamat m = {};
  m.data_device = v.data();
  m.on_device = 1;
  m.size[0] = rows;
  m.size[1] = cols;
  return m;
}
// Seven images, their tables, N cases and the cases' crops by the definition; then the same tables as random numbers.  Exact-size heap
// buffers, so that an address sanitizer sees any overrun.
struct Scene {
  static const int ni = 7;
  std::vector<unsigned char> bytes, want;   // want: N crops of 3 x H x W
  std::vector<long long> table, table_g;
  std::vector<int> taps, cases, taps_g, cases_g;
  Scene(int W, int H, int N, std::mt19937& rng) : bytes(3, 0) {
    const int sizes[][2] = {{9, 7}, {6, 8}, {1, 9}, {13, 1}, {150, 40}, {40, 170}, {W, H}};
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
    const size_t dims = (size_t)3 * H * W;
    want.resize(N * dims);
    for (int n = 0; n < N; ++n) {
      int k = rng() % ni, left = rng() % (nws[k] - W + 1), top = rng() % (nhs[k] - H + 1), mir = rng() & 1;
      cases.insert(cases.end(), {k, left, top, mir});
      for (int c = 0; c < 3; ++c) for (int r = 0; r < H; ++r) for (int x = 0; x < W; ++x)
        want[n * dims + ((size_t)c * H + r) * W + x] = resized[k][((size_t)(top + r) * nws[k] + left + (mir ? W - 1 - x : x)) * 3 + c];
    }
    bytes = std::vector<unsigned char>(bytes); table = std::vector<long long>(table);   // (copies: exactly their size)
    taps = std::vector<int>(taps); cases = std::vector<int>(cases);
    cases_g = cases; taps_g = taps; table_g = table;
    for (auto& v : cases_g) v = (int)rng();
    for (auto& v : taps_g) v = (int)rng();
    for (auto& v : table_g) v = ((long long)rng() << 32) ^ rng() ^ ((rng() & 1) ? -1LL : 0);
  }
  int num_taps() const { return (int)(taps.size() / 3); }
};
static bool run(int W, int H, int N, unsigned seed, int misalign) {
  std::mt19937 rng(seed);
  Scene s(W, H, N, rng);
  const size_t dims = (size_t)3 * H * W;
  std::vector<unsigned char> out(N * dims + misalign + 8, 0xAB);   // `misalign` fill bytes in front, 8 behind
  int rc = crop_images_u8(s.bytes.data(), s.bytes.size(), s.table.data(), s.ni, s.taps.data(), s.num_taps(), s.cases.data(), N,
                          out.data() + misalign, W, H);
  bool ok = rc == 0;
  for (int i = 0; i < misalign; ++i) ok &= out[i] == 0xAB;
  for (int i = 0; i < 8; ++i) ok &= out[misalign + N * dims + i] == 0xAB;
  size_t bad = 0;
  for (size_t i = 0; i < s.want.size(); ++i) bad += out[misalign + i] != s.want[i];
  ok &= bad == 0;
  // garbage tables: must stay in bounds (ASan) and return 0
  std::vector<unsigned char> out2(N * dims, 0);
  int rc2 = crop_images_u8(s.bytes.data(), s.bytes.size(), s.table_g.data(), s.ni, s.taps_g.data(), s.num_taps(), s.cases_g.data(), N, out2.data(), W, H);
  int rc3 = crop_images_u8(s.bytes.data(), s.bytes.size(), s.table.data(), s.ni, s.taps_g.data(), s.num_taps(), s.cases_g.data(), N, out2.data(), W, H);
  ok &= rc2 == 0 && rc3 == 0;
  printf("%s W=%d H=%d N=%d mis=%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", W, H, N, misalign, rc, bad);
  return ok;
}
// What a batch of N cases draws: offsets that walk 0 ... the maximum (with a fraction, which the cast drops), flip values on both sides
// of 0.5 (0.5 itself does not flip), a column per case with the first one repeated, and mean / std per source pixel.
struct Draw {
  std::vector<float> wo, ho, fl, index, mean, sdev;
  cudamat mwo, mho, mfl, mindex, mmean, msdev;
  Draw(int N, int max_wo, int max_ho, int columns, int dims, std::mt19937& rng) : wo(N), ho(N), fl(N), index(N), mean(dims), sdev(dims) {
    const float flips[] = {0.2f, 0.5f, 0.50001f, 0.9f};
    for (int n = 0; n < N; ++n) {
      wo[n] = n % (max_wo + 1) + (n % 3) * 0.3f;
      ho[n] = (n / 2) % (max_ho + 1) + (n % 2) * 0.6f;
      fl[n] = flips[(n + n / 4) % 4];
      index[n] = (float)((n * 5) % columns);
    }
    if (N > 1) index[1] = index[0];
    if (N > 2) { wo[N - 1] = (float)max_wo; ho[N - 1] = (float)max_ho; index[N - 1] = (float)(columns - 1); }
    for (auto& v : mean) v = (rng() % 2551) * 0.1f;
    for (auto& v : sdev) v = 0.5f + (rng() % 997) * 0.07f;
    mwo = mat(wo, 1, N); mho = mat(ho, 1, N); mfl = mat(fl, 1, N); mindex = mat(index, 1, N);
    mmean = mat(mean, dims, 1); msdev = mat(sdev, dims, 1);
  }
};
// patches[n + N (dc + pw (row + ph plane))] by the definition, from `pixel(n, t, s)`: byte s (inside a case of `dims` bytes) of plane
// group t of case n
template <typename Pixel>
static std::vector<float> direct(const Draw& d, bool norm, bool jitter, int N, int T, int colors, int W, int H, int pw, int ph, Pixel pixel) {
  std::vector<float> want((size_t)N * T * colors * ph * pw);
  for (int n = 0; n < N; ++n) for (int t = 0; t < T; ++t) for (int c = 0; c < colors; ++c) for (int r = 0; r < ph; ++r) for (int dc = 0; dc < pw; ++dc) {
    int sr = r, sc = dc;
    if (jitter) {
      sr += (int)d.ho[n];
      sc += (int)d.wo[n];
      if (d.fl[n] > 0.5f) sc = W - sc - 1;
    }
    const int s = sc + W * (sr + H * c);
    float v = (float)pixel(n, t, s);
    if (norm) v = (v - d.mean[s]) / d.sdev[s];
    want[(size_t)n + (size_t)N * (dc + (size_t)pw * (r + (size_t)ph * ((size_t)t * colors + c)))] = v;
  }
  return want;
}
static size_t differing(const std::vector<float>& a, const std::vector<float>& b) {
  size_t bad = a.size() != b.size();
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) bad += std::memcmp(&a[i], &b[i], 4) != 0;
  return bad;
}
// T == 1: stage_patches_u8 on a chunk of 9 cases; T > 1: stage_clips_u8 on a buffer of 12 frames, in grid mode `grid`
static bool run_columns(int N, int T, int grid, bool norm, bool jitter) {
  const int colors = 3, W = 70, H = 5, pw = jitter ? 66 : W, ph = jitter ? 4 : H, dims = colors * W * H;
  const int columns = T == 1 ? 9 : 12;
  std::mt19937 rng(1000 * N + 10 * T + 2 * norm + jitter);
  std::vector<unsigned char> data((size_t)dims * columns);
  for (auto& v : data) v = rng() & 255;
  Draw d(N, W - pw, H - ph, columns - T + 1, dims, rng);
  std::vector<float> out((size_t)N * T * colors * ph * pw);
  std::memset(out.data(), 0xAB, out.size() * 4);
  cudamat mo = mat(out, N, T * colors * ph * pw);
  cudamat *mean = norm ? &d.mmean : nullptr, *sdev = norm ? &d.msdev : nullptr;
  cudamat *wo = jitter ? &d.mwo : nullptr, *ho = jitter ? &d.mho : nullptr, *fl = jitter ? &d.mfl : nullptr;
  int rc;
  if (T == 1) {
    rc = stage_patches_u8(data.data(), dims, columns, &d.mindex, mean, sdev, &mo, wo, ho, fl, W, H, pw, ph);
  } else {
    convnet_hip_set_stage_clips_grid(grid);
    rc = stage_clips_u8(data.data(), dims, columns, &d.mindex, T, mean, sdev, &mo, wo, ho, fl, W, H, pw, ph);
    convnet_hip_set_stage_clips_grid(0);
  }
  const auto want = direct(d, norm, jitter, N, T, colors, W, H, pw, ph,
                           [&](int n, int t, int s) { return data[(size_t)dims * ((int)d.index[n] + t) + s]; });
  const size_t bad = differing(out, want);
  const bool ok = rc == 0 && bad == 0;
  if (T == 1) printf("%s patches N=%d norm=%d jitter=%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", N, norm, jitter, rc, bad);
  else printf("%s clips T=%d grid=%d N=%d norm=%d jitter=%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", T, grid, N, norm, jitter, rc, bad);
  return ok;
}
static bool run_images(int W, int H, int N, bool norm, bool jitter) {
  std::mt19937 rng(77 * W + 5 * N + 2 * norm + jitter);
  Scene s(W, H, N, rng);
  const int pw = jitter ? W - 1 : W, ph = jitter ? H - 1 : H, dims = 3 * H * W;
  Draw d(N, W - pw, H - ph, 1, dims, rng);
  std::vector<float> out((size_t)N * 3 * ph * pw);
  std::memset(out.data(), 0xAB, out.size() * 4);
  cudamat mo = mat(out, N, 3 * ph * pw);
  cudamat *mean = norm ? &d.mmean : nullptr, *sdev = norm ? &d.msdev : nullptr;
  cudamat *wo = jitter ? &d.mwo : nullptr, *ho = jitter ? &d.mho : nullptr, *fl = jitter ? &d.mfl : nullptr;
  int rc = stage_images_u8(s.bytes.data(), s.bytes.size(), s.table.data(), s.ni, s.taps.data(), s.num_taps(), s.cases.data(), mean, sdev, &mo,
                           wo, ho, fl, W, H, pw, ph);
  const auto want = direct(d, norm, jitter, N, 1, 3, W, H, pw, ph, [&](int n, int, int src) { return s.want[(size_t)n * dims + src]; });
  const size_t bad = differing(out, want);
  // garbage tables: must stay in bounds (ASan) and return 0
  int rc2 = stage_images_u8(s.bytes.data(), s.bytes.size(), s.table_g.data(), s.ni, s.taps_g.data(), s.num_taps(), s.cases_g.data(), mean, sdev,
                            &mo, wo, ho, fl, W, H, pw, ph);
  int rc3 = stage_images_u8(s.bytes.data(), s.bytes.size(), s.table.data(), s.ni, s.taps_g.data(), s.num_taps(), s.cases_g.data(), mean, sdev,
                            &mo, wo, ho, fl, W, H, pw, ph);
  const bool ok = rc == 0 && bad == 0 && rc2 == 0 && rc3 == 0;
  printf("%s images W=%d H=%d N=%d norm=%d jitter=%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", W, H, N, norm, jitter, rc, bad);
  return ok;
}
// the codes of the staging entries and their precedence, on arguments that are right but for what each line breaks
static bool run_errors() {
  const int N = 2, W = 3, H = 2, dims = 3 * W * H;
  std::vector<float> v(dims * N, 1.f), out(dims * N, 0.f);
  std::vector<unsigned char> x(dims * 4, 0);
  cudamat idx = mat(v, 1, N), mean = mat(v, dims, 1), sdev = mat(v, dims, 1), dst = mat(out, N, dims), wo = mat(v, 1, N), short_wo = mat(v, 1, N - 1);
  cudamat host_dst = dst, trans_dst = dst;
  host_dst.on_device = 0;
  trans_dst.is_trans = 1;
  void* p = x.data();
  bool ok = true;
  ok &= stage_patches_u8(nullptr, dims, 4, &idx, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_NOT_ON_DEVICE;
  ok &= stage_patches_u8(p, dims, 4, nullptr, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_NOT_ON_DEVICE;
  ok &= stage_patches_u8(p, dims, 4, &idx, &mean, nullptr, &host_dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= stage_patches_u8(p, dims, 4, &idx, nullptr, nullptr, &host_dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_NOT_ON_DEVICE;
  ok &= stage_patches_u8(p, dims, 0, &idx, nullptr, nullptr, &trans_dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_TRANSPOSED;
  ok &= stage_patches_u8(p, dims, 0, &idx, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= stage_patches_u8(p, dims, 4, &idx, nullptr, nullptr, &dst, &short_wo, &wo, &wo, W, H, W, H) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= stage_patches_u8(p, dims, (1 << 24) + 1, &idx, &mean, &sdev, &dst, &wo, &wo, &wo, W, H, W, H) == ERROR_UNSUPPORTED;
  ok &= stage_patches_u8(p, dims, 4, &idx, &mean, &sdev, &dst, &wo, &wo, &wo, W, H, W, H) == 0;
  ok &= stage_clips_u8(p, dims, 4, nullptr, 1, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_NOT_ON_DEVICE;
  ok &= stage_clips_u8(p, dims, 4, &idx, 0, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= stage_clips_u8(p, dims, 4, &idx, 2, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= stage_clips_u8(p, dims, 4, &idx, 1, nullptr, nullptr, &dst, nullptr, nullptr, nullptr, W, H, W, H) == 0;
  const auto images = [&](void* bytes, size_t num_bytes, void* table, int num_images, int num_taps, cudamat* patches, cudamat* m, int width) {
    return stage_images_u8(bytes, num_bytes, table, num_images, p, num_taps, p, m, &sdev, patches, nullptr, nullptr, nullptr, width, H, W, H);
  };
  ok &= images(nullptr, 0, p, 1, 1, &dst, &mean, W) == ERROR_GENERIC;
  ok &= images(p, 1, nullptr, 1, 1, &dst, &mean, W) == ERROR_GENERIC;
  ok &= images(p, 1, p, 1, 1, nullptr, &mean, W) == ERROR_GENERIC;
  ok &= images(p, 0, p, 1, 1, &host_dst, &mean, W) == ERROR_INCOMPATIBLE_DIMENSIONS;   // (before anything the shared checker reports)
  ok &= images(p, 1, p, 1, 0, &host_dst, &mean, W) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= images(p, 1, p, 1, 1, &host_dst, &mean, 0) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= images(p, 1, p, 1, 1, &dst, nullptr, W) == ERROR_INCOMPATIBLE_DIMENSIONS;        // std without mean
  ok &= images(p, 1, p, 1, 1, &host_dst, &mean, W) == ERROR_NOT_ON_DEVICE;
  ok &= images(p, 1, p, 0, 1, &trans_dst, &mean, W) == ERROR_TRANSPOSED;
  ok &= images(p, 1, p, 0, 1, &dst, &mean, W) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= images(p, 1, p, (1 << 24) + 1, 1, &dst, &mean, W + 1) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= images(p, 1, p, (1 << 24) + 1, 1, &dst, &mean, W) == ERROR_UNSUPPORTED;
  ok &= images(p, x.size(), p, 1, 1, &dst, &mean, W) == 0;
  unsigned char b;
  ok &= crop_images_u8(nullptr, 1, &b, 1, &b, 1, &b, 1, &b, 1, 1) == ERROR_GENERIC;
  ok &= crop_images_u8(&b, 0, &b, 1, &b, 1, &b, 1, &b, 1, 1) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= crop_images_u8(&b, 1, &b, (1 << 24) + 1, &b, 1, &b, 1, &b, 1, 1) == ERROR_UNSUPPORTED;
  printf("%s errors\n", ok ? "PASS" : "FAIL");
  return ok;
}
int main() {
  bool ok = true;
  const int geo[][3] = {{1, 1, 3}, {7, 5, 65}, {8, 4, 65}, {67, 3, 5}, {256, 6, 3}, {300, 2, 2}};   // W, H, cases
  for (auto& g : geo) for (int mis = 0; mis < 4; mis += 1) ok &= run(g[0], g[1], g[2], 7 * g[0] + g[1] + mis, mis);
  for (int N : {1, 5, 37, 64, 68})
    for (int build = 0; build < 4; ++build) {
      ok &= run_columns(N, 1, 0, build & 1, build >> 1);
      for (int grid = 1; grid <= 2; ++grid) ok &= run_columns(N, 3, grid, build & 1, build >> 1);
    }
  const int image_geo[][2] = {{7, 5}, {67, 3}};   // W, H: a narrow crop, and one wider than the tile
  for (auto& g : image_geo)
    for (int N : {3, 65})
      for (int build = 0; build < 4; ++build) ok &= run_images(g[0], g[1], N, build & 1, build >> 1);
  ok &= run_errors();
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return !ok;
}
