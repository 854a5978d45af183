// Runs stage_images_jitter_u8 of convnet_amd/csrc/input_staging.hip FUNCTIONALLY on the CPU — the kernel source compiled as host C++
// against tests/emu/hip/hip_runtime.h — through the C ABI, on scenes that tests/test_stage_images_jitter_emulated.py writes from the host
// definition (convnet_amd/image_iterators.py): one file per scene,
//   12 x int64   {num_bytes, num_images, num_taps, N, rotated, norm, jitter, W, H, pw, ph, seed}
//   bytes u8[num_bytes], image table int64[num_images][11], taps int32[num_taps][3], case table int32[N][4],
//   mean f32[3 H W], std f32[3 H W], width offsets f32[N], height offsets f32[N], flip f32[N], expected patches f32[N * 3 * ph * pw].
// Every buffer is an exact-size heap vector, so that an address sanitizer sees any overrun (add -fsanitize=address to every compile and
// the link).  Per scene: the output, pre-filled, must equal the expectation to the bit; then the same launch with the image table, the
// taps and the case table replaced by random numbers, in both arms, must return 0 (and, under a sanitizer, stay inside the buffers).
// Then the entry's error codes.  Prints one line per scene; exit status 0 only if all pass.
#include "input_staging_emu_prelude.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "common.h"
static cudamat mat(std::vector<float>& v, int rows, int cols) {
  cudamat m = {};
  m.data_device = v.data();
  m.on_device = 1;
  m.size[0] = rows;
  m.size[1] = cols;
  return m;
}
template <typename T>
static bool read(FILE* f, std::vector<T>& v, size_t n) {
  v = std::vector<T>(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static bool run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  std::vector<long long> head, table;
  std::vector<unsigned char> bytes;
  std::vector<int> taps, cases;
  std::vector<float> mean, sdev, wo, ho, fl, want;
  bool ok = read(f, head, 12);
  if (!ok) return false;
  const int ni = (int)head[1], nt = (int)head[2], N = (int)head[3], rotated = (int)head[4], norm = (int)head[5], jitter = (int)head[6];
  const int W = (int)head[7], H = (int)head[8], pw = (int)head[9], ph = (int)head[10];
  const size_t dims = (size_t)3 * H * W, width = (size_t)3 * ph * pw;
  ok = ok && read(f, bytes, (size_t)head[0]) && read(f, table, (size_t)ni * 11) && read(f, taps, (size_t)nt * 3) && read(f, cases, (size_t)N * 4);
  ok = ok && read(f, mean, dims) && read(f, sdev, dims) && read(f, wo, N) && read(f, ho, N) && read(f, fl, N) && read(f, want, N * width);
  fclose(f);
  if (!ok) return false;
  std::vector<float> out(N * width);
  std::memset(out.data(), 0xAB, out.size() * 4);
  cudamat mo = mat(out, N, (int)width), mmean = mat(mean, (int)dims, 1), msdev = mat(sdev, (int)dims, 1);
  cudamat mwo = mat(wo, 1, N), mho = mat(ho, 1, N), mfl = mat(fl, 1, N);
  cudamat *pm = norm ? &mmean : nullptr, *ps = norm ? &msdev : nullptr;
  cudamat *pwo = jitter ? &mwo : nullptr, *pho = jitter ? &mho : nullptr, *pfl = jitter ? &mfl : nullptr;
  const int rc = stage_images_jitter_u8(bytes.data(), bytes.size(), table.data(), ni, taps.data(), nt, cases.data(), rotated, pm, ps, &mo, pwo, pho,
                                        pfl, W, H, pw, ph);
  size_t bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += std::memcmp(&out[i], &want[i], 4) != 0;
  // tables of random numbers: any pixels, no access outside the buffers
  std::mt19937 rng((unsigned)head[11]);
  std::vector<long long> table_g(table.size());
  std::vector<int> taps_g(taps.size()), cases_g(cases.size());
  for (auto& v : table_g) v = ((long long)rng() << 32) ^ rng() ^ ((rng() & 1) ? -1LL : 0);
  for (auto& v : taps_g) v = (int)rng();
  for (auto& v : cases_g) v = (int)rng();
  int rcg = 0;
  for (int arm = 0; arm < 2; ++arm) {
    rcg |= stage_images_jitter_u8(bytes.data(), bytes.size(), table_g.data(), ni, taps_g.data(), nt, cases_g.data(), arm, pm, ps, &mo, pwo, pho, pfl,
                                  W, H, pw, ph);
    rcg |= stage_images_jitter_u8(bytes.data(), bytes.size(), table.data(), ni, taps_g.data(), nt, cases_g.data(), arm, pm, ps, &mo, pwo, pho, pfl, W,
                                  H, pw, ph);
    rcg |= stage_images_jitter_u8(bytes.data(), bytes.size(), table_g.data(), ni, taps.data(), nt, cases.data(), arm, pm, ps, &mo, pwo, pho, pfl, W, H,
                                  pw, ph);
  }
  ok = rc == 0 && bad == 0 && rcg == 0;
  printf("%s jitter N=%d W=%d H=%d pw=%d ph=%d rotated=%d norm=%d jitter=%d rc=%d bad=%zu garbage=%d\n", ok ? "PASS" : "FAIL", N, W, H, pw, ph,
         rotated, norm, jitter, rc, bad, rcg);
  return ok;
}
static bool run_errors() {
  const int N = 2, W = 3, H = 2, dims = 3 * W * H;
  std::vector<float> v(dims * N, 1.f), out(dims * N, 7.f);
  std::vector<long long> x(64, 0);
  cudamat mean = mat(v, dims, 1), sdev = mat(v, dims, 1), dst = mat(out, N, dims), wo = mat(v, 1, N);
  cudamat host_dst = dst;
  host_dst.on_device = 0;
  void* p = x.data();
  const auto call = [&](void* bytes, size_t num_bytes, void* table, int num_images, int num_taps, cudamat* patches, cudamat* m, cudamat* offs,
                        int width) {
    return stage_images_jitter_u8(bytes, num_bytes, table, num_images, p, num_taps, p, 1, m, &sdev, patches, offs, nullptr, nullptr, width, H, W, H);
  };
  bool ok = true;
  ok &= call(nullptr, 0, p, 1, 1, &dst, &mean, nullptr, W) == ERROR_GENERIC;
  ok &= call(p, 1, nullptr, 1, 1, &dst, &mean, nullptr, W) == ERROR_GENERIC;
  ok &= call(p, 1, p, 1, 1, nullptr, &mean, nullptr, W) == ERROR_GENERIC;
  ok &= call(p, 0, p, 1, 1, &host_dst, &mean, nullptr, W) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= call(p, 1, p, 1, 0, &dst, &mean, nullptr, W) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= call(p, 1, p, 1, 1, &dst, nullptr, nullptr, W) == ERROR_INCOMPATIBLE_DIMENSIONS;     // std without mean
  ok &= call(p, 1, p, 1, 1, &dst, &mean, &wo, W) == ERROR_INCOMPATIBLE_DIMENSIONS;           // one offset without the others
  ok &= call(p, 1, p, 1, 1, &host_dst, &mean, nullptr, W) == ERROR_NOT_ON_DEVICE;
  ok &= call(p, 1, p, 0, 1, &dst, &mean, nullptr, W) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= call(p, 1, p, (1 << 24) + 1, 1, &dst, &mean, nullptr, W) == ERROR_UNSUPPORTED;
  for (float o : out) ok &= o == 7.f;                                                           // nothing ran
  ok &= call(p, x.size() * 8, p, 1, 1, &dst, &mean, nullptr, W) == 0;
  printf("%s errors\n", ok ? "PASS" : "FAIL");
  return ok;
}
int main(int argc, char** argv) {
  bool ok = argc > 1;
  for (int i = 1; i < argc; ++i) ok &= run(argv[i]);
  ok &= run_errors();
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return !ok;
}
