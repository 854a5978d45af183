// What tests/test_image_jitter_cpu.py compares JitterStream with: libstdc++'s std::default_random_engine seeded with 0 behind a
// uniform_real_distribution<float>(0, 1).  argv: random_rotate_max_angle, min_scale.  Prints the bit patterns of the first 4096 draws,
// then of 64 (angle, trans_x, trans_y, scale) rows drawn from a fresh engine through a const int angle and a const float scale.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const float angle_field = (float)atof(argv[1]);
  const int max_angle = angle_field;
  const float min_scale = (float)atof(argv[2]);
  std::default_random_engine first, second;
  first.seed(0);
  second.seed(0);
  std::uniform_real_distribution<float> u(0, 1), v(0, 1);
  for (int i = 0; i < 4096; ++i) printf("%08x\n", bits(u(first)));
  for (int i = 0; i < 64; ++i) {
    const float angle = 2 * max_angle * (v(second) - 0.5);
    const float tx = v(second);
    const float ty = v(second);
    const float scale = min_scale + (1 - min_scale) * v(second);
    printf("%08x %08x %08x %08x\n", bits(angle), bits(tx), bits(ty), bits(scale));
  }
  return 0;
}
