// Runs resize_frames_u8 of convnet_amd/csrc/input_staging.hip FUNCTIONALLY on the CPU — the kernel source compiled as host C++ against
// tests/emu/hip/hip_runtime.h — through the C ABI, against a direct scalar evaluation of the definition in include/convnet_hip.h
// (h(y), then result; 64-bit integers), compared with memcmp.
// * the geometries of tests/test_resize_frames_gpu.py (w x h -> W x H): 5x7 -> 70x66 (3 and 65 frames), 70x66 -> 5x7, 5x7 -> 5x7,
//   1x1 -> 9x4, 1100x3 -> 1030x3 (2 frames), 9x300 -> 9x20, 9x20 -> 9x300 and 700x5 -> 150x3 (a width shrunk past what a tile stages: the
//   scalar arm); each mirrored and not, the source 0 ... 3 bytes past an aligned address and the output likewise, the output inside a
//   buffer of a fill byte, the source in an exact-size heap buffer.
// * tap tables whose source indices are random numbers: the clamps hold, and the bytes are the definition's with the same clamps.
// * the entry's error codes in their precedence.
// Add -fsanitize=address to every compile and the link to have the buffer bounds checked.  Prints one line per case; the last line is
// ALL PASSED and the exit status 0 only if all pass.  tests/test_resize_frames_emulated.py builds and runs it.
#include "input_staging_emu_prelude.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "common.h"
typedef long long i64;
static void mk_taps(int ssize, int dsize, std::vector<int>& out) {
  const double scale = 1.0 / (dsize / (double)ssize);
  for (int d = 0; d < dsize; ++d) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int s = (int)std::floor(fx);
    fx -= s;
    if (s < 0) { s = 0; fx = 0; }
    if (s >= ssize - 1) { s = ssize - 1; fx = 0; }
    out.insert(out.end(), {s, (int)std::rint((1.f - fx) * 2048.f), (int)std::rint(fx * 2048.f)});
  }
}
// the definition, with the entry's clamps of the source indices
static std::vector<unsigned char> direct(const unsigned char* bytes, int N, int w, int h, const std::vector<int>& taps, int W, int H, bool mirrored) {
  std::vector<unsigned char> want((size_t)N * 3 * H * W);
  const auto clamp = [](i64 v, i64 hi) { return std::min(std::max(v, (i64)0), hi); };
  for (int n = 0; n < N; ++n) {
    const unsigned char* p = bytes + (size_t)n * w * h * 3;
    for (int c = 0; c < 3; ++c) for (int r = 0; r < H; ++r) for (int x = 0; x < W; ++x) {
      const int* ct = &taps[3 * (size_t)(mirrored ? W - 1 - x : x)];
      const int* rt = &taps[3 * (size_t)(W + r)];
      const i64 sx = clamp(ct[0], w - 1), sx1 = std::min(sx + 1, (i64)w - 1), sy = clamp(rt[0], h - 1), sy1 = std::min(sy + 1, (i64)h - 1);
      const auto hrow = [&](i64 y) {
        const i64 v = (i64)p[(y * w + sx) * 3 + c] * ct[1] + (i64)p[(y * w + sx1) * 3 + c] * ct[2];
        return (((2048 * (v >> 4)) >> 16) + 2) >> 2;
      };
      want[(((size_t)n * 3 + c) * H + r) * W + x] =
          (unsigned char)(((((i64)rt[1] * ((2048 * hrow(sy)) >> 4)) >> 16) + (((i64)rt[2] * ((2048 * hrow(sy1)) >> 4)) >> 16) + 2) >> 2);
    }
  }
  return want;
}
static bool run(int w, int h, int W, int H, int N, bool mirrored, int mis_in, int mis_out, bool wild) {
  std::mt19937 rng(1000 * w + 100 * h + 10 * W + H + N + mirrored + 2 * wild);
  const size_t in_bytes = (size_t)N * w * h * 3, out_bytes = (size_t)N * 3 * H * W;
  // posix_memalign'd, exactly mis_in + in_bytes long: the frames start mis_in past a 256-byte boundary and end where the buffer ends
  void* raw = nullptr;
  if (posix_memalign(&raw, 256, mis_in + in_bytes)) return false;
  unsigned char* bytes = (unsigned char*)raw + mis_in;
  for (size_t i = 0; i < in_bytes; ++i) bytes[i] = rng() & 255;
  std::vector<int> taps;
  mk_taps(w, W, taps);
  mk_taps(h, H, taps);
  if (wild)
    for (size_t i = 0; i < taps.size(); i += 3) taps[i] = (int)rng() >> (rng() % 24);   // any sign, any size
  taps = std::vector<int>(taps);   // exactly its size
  void* raw_out = nullptr;
  if (posix_memalign(&raw_out, 256, mis_out + out_bytes + 8)) return false;
  unsigned char* out = (unsigned char*)raw_out;
  std::memset(out, 0xAB, mis_out + out_bytes + 8);
  const int rc = resize_frames_u8(bytes, in_bytes, N, w, h, taps.data(), W, H, mirrored, out + mis_out);
  const auto want = direct(bytes, N, w, h, taps, W, H, mirrored);
  bool ok = rc == 0 && std::memcmp(out + mis_out, want.data(), out_bytes) == 0;
  for (int i = 0; i < mis_out; ++i) ok &= out[i] == 0xAB;
  for (int i = 0; i < 8; ++i) ok &= out[mis_out + out_bytes + i] == 0xAB;
  size_t bad = 0;
  for (size_t i = 0; i < out_bytes; ++i) bad += out[mis_out + i] != want[i];
  printf("%s %s %dx%d->%dx%d N=%d mirrored=%d in+%d out+%d rc=%d bad=%zu\n", ok ? "PASS" : "FAIL", wild ? "wild" : "frames", w, h, W, H, N,
         (int)mirrored, mis_in, mis_out, rc, bad);
  std::free(raw);
  std::free(raw_out);
  return ok;
}
// the codes and their precedence, on arguments that are right but for what each line breaks
static bool run_errors() {
  unsigned char b[12] = {0}, out[3] = {7, 7, 7};
  int t[6] = {0, 2048, 0, 0, 2048, 0};
  bool ok = true;
  ok &= resize_frames_u8(nullptr, 0, 0, 1, 1, t, 1, 1, 0, out) == ERROR_GENERIC;                  // (before the sizes)
  ok &= resize_frames_u8(b, 3, 1, 1, 1, nullptr, 0, 1, 0, out) == ERROR_GENERIC;
  ok &= resize_frames_u8(b, 3, 1, 1, 1, t, 1, 1, 0, nullptr) == ERROR_GENERIC;
  ok &= resize_frames_u8(b, 3, 0, 1, 1, t, 1, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 3, 1, 0, 1, t, 1, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 3, 1, 1, -1, t, 1, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 3, 1, 1, 1, t, 0, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 3, 1, 1, 1, t, 1, 0, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 2, 1, 1, 1, t, 1, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;
  ok &= resize_frames_u8(b, 12, 0x7fffffff, 1, 1, t, 1 << 30, 1 << 30, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;   // (before the grid)
  ok &= resize_frames_u8(b, 12, 0x7fffffff, 0x7fffffff, 0x7fffffff, t, 1, 1, 0, out) == ERROR_INCOMPATIBLE_DIMENSIONS;   // (no overflow)
  ok &= resize_frames_u8(b, 12, 4, 1, 1, t, 1 << 30, 1 << 30, 0, out) == ERROR_UNSUPPORTED;
  ok &= out[0] == 7 && out[1] == 7 && out[2] == 7;
  ok &= resize_frames_u8(b, 3, 1, 1, 1, t, 1, 1, 0, out) == 0 && out[0] == 0;
  printf("%s errors\n", ok ? "PASS" : "FAIL");
  return ok;
}
int main() {
  bool ok = true;
  const int geo[][5] = {{5, 7, 70, 66, 3},   {5, 7, 70, 66, 65}, {70, 66, 5, 7, 3}, {5, 7, 5, 7, 3},  {1, 1, 9, 4, 3},
                        {1100, 3, 1030, 3, 2}, {9, 300, 9, 20, 3},  {9, 20, 9, 300, 3}, {700, 5, 150, 3, 2}};   // w, h, W, H, frames
  int k = 0;
  for (auto& g : geo)
    for (int mirrored = 0; mirrored < 2; ++mirrored, ++k) ok &= run(g[0], g[1], g[2], g[3], g[4], mirrored, k & 3, (k >> 1) & 3, false);
  const int wild[][5] = {{5, 7, 70, 66, 3}, {70, 66, 5, 7, 3}, {1100, 3, 1030, 3, 2}, {9, 300, 9, 20, 1}, {1, 1, 9, 4, 1}};
  for (auto& g : wild)
    for (int mirrored = 0; mirrored < 2; ++mirrored, ++k) ok &= run(g[0], g[1], g[2], g[3], g[4], mirrored, k & 3, (k >> 1) & 3, true);
  ok &= run_errors();
  printf(ok ? "ALL PASSED\n" : "SOME FAILED\n");
  return !ok;
}
