// chunk_moments_u8: the raw integer moments of a range of cases of a byte chunk, added into 2 * dims + C * C unsigned 64-bit sums — what
// apps/compute_mean.cc:70-80 gathers per batch (mean_batch.Add(state); Dot(state, state, pixel_cov, ..., true, false) on the
// (-1, num_colors) reshape; state.Mult(state); var_batch.Add(state)) as five float passes, here as ONE read of the bytes and in integers,
// which makes every sum exact and independent of the order it was formed in.
//   A block owns a tile of 64 * V consecutive pixels (V = 4: one dword load per lane, colour and case; V = 1: byte loads, for a pixel
//   count or a base that is no multiple of 4) and a share of the cases; its 4 waves take every 4th case of the share.  Per owned dim a
//   lane keeps the sum and the sum of squares in 32 bits, per colour pair the dot product of the two colours' words (v_dot4_u32_u8: 4
//   pixels per instruction).  No 32-bit partial can overflow before it is flushed: a wave takes at most kCasesPerWave cases, and
//     sum of squares of one dim, the block's 4 waves together : 4 * 255^2 * 8192 = 2 130 739 200 < 2^32   (one dim overflows at 66 052 cases)
//     dot product of 4 pixels, one wave                       : 4 * 255^2 * 8192 = 2 130 739 200 < 2^32
//   Flush: the waves' per-dim partials are summed through LDS, then ONE 64-bit vector atomic per dim and moment and block — a wave's
//   atomics cover 512 contiguous bytes.  The atomics are what bounds the pass (measured: a 3 x 256 x 256 chunk of 1 280 cases takes
//   44 us with 2 shares of the cases and 600 us with 64 when every lane flushes its own sums), so the cases are split no further than
//   fills the chip: about 8 waves per CU with 8 cases' loads in flight each.  The C x C block: the diagonal is the sum over the owned
//   pixels of the sums of squares; wave reduction, a sum over the waves in LDS, one 64-bit atomic per entry and block.  Integer atomics
//   only: any split gives the same bits.
#include "common.h"

namespace chip {
namespace {

using u64 = unsigned long long;
constexpr int kCmThreads = 256, kCmWaves = kCmThreads / 64;
constexpr int kCasesPerWave = 8192;
static_assert(255ull * 255ull * 4ull * kCasesPerWave < (1ull << 32), "a 32-bit partial could overflow before its flush");
static_assert(255ull * 255ull * kCmWaves * kCasesPerWave < (1ull << 32), "the 32-bit sum over a block's waves could overflow");

// chunk: the first byte of the first case of the range.  P = pixels per colour, dims = C * P.
template <int C, int V>
__global__ void __launch_bounds__(kCmThreads) chunk_moments_kernel(const unsigned char* __restrict__ chunk, int P, int cases, int cases_per_block,
                                                                   u64* __restrict__ acc) {
  constexpr int TP = 64 * V;             // pixels of a tile
  __shared__ unsigned part[kCmWaves][C][2][TP];
  __shared__ u64 cross_sh[kCmWaves][C * C];
  const size_t dims = (size_t)C * P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile0 = blockIdx.x * TP, p0 = tile0 + lane * V;
  const bool active = p0 < P;            // (V == 4 only where P % 4 == 0: a lane's pixels are all inside or all outside)
  const int n0 = blockIdx.y * cases_per_block, n1 = min(n0 + cases_per_block, cases);
  unsigned s[C][V], q[C][V], x[C][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int e = 0; e < V; ++e) s[c][e] = q[c][e] = 0;
#pragma unroll
    for (int d = 0; d < C; ++d) x[c][d] = 0;
  }
  if (active) {
    const unsigned char* src = chunk + (size_t)(n0 + wave) * dims + p0;
#pragma unroll 8
    for (int n = n0 + wave; n < n1; n += kCmWaves, src += kCmWaves * dims) {
      unsigned w[C];
#pragma unroll
      for (int c = 0; c < C; ++c)
        w[c] = V == 4 ? *reinterpret_cast<const unsigned*>(src + (size_t)c * P) : (unsigned)src[(size_t)c * P];
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const unsigned b = (w[c] >> (8 * e)) & 255u;
          s[c][e] += b;
          q[c][e] += b * b;
        }
#pragma unroll
        for (int d = c + 1; d < C; ++d) x[c][d] = __builtin_amdgcn_udot4(w[c], w[d], x[c][d], false);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      part[wave][c][0][lane * V + e] = s[c][e];
      part[wave][c][1][lane * V + e] = q[c][e];
    }
  }
  // the C x C block: upper triangle per lane -> wave -> (below) block
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int d = c; d < C; ++d) {
      u64 v = x[c][d];
      if (d == c) {
        v = 0;
#pragma unroll
        for (int e = 0; e < V; ++e) v += q[c][e];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) cross_sh[wave][c * C + d] = v;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < TP; t += kCmThreads) {     // lane t: pixel t of the tile, every colour and moment
    if (tile0 + t < P) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          unsigned v = 0;
#pragma unroll
          for (int w = 0; w < kCmWaves; ++w) v += part[w][c][m][t];
          atomicAdd(acc + m * dims + (size_t)c * P + tile0 + t, (u64)v);
        }
      }
    }
  }
  if (threadIdx.x < C * C) {             // one atomic per entry: both halves of the symmetric block
    const int c = threadIdx.x / C, d = threadIdx.x % C;
    const int k = c <= d ? c * C + d : d * C + c;
    u64 v = 0;
#pragma unroll
    for (int w = 0; w < kCmWaves; ++w) v += cross_sh[w][k];
    if (v) atomicAdd(acc + 2 * dims + threadIdx.x, v);
  }
}

template <int C>
int launch_chunk_moments(const unsigned char* first, int P, int cases, u64* acc) {
  const bool vec = (P & 3) == 0 && (reinterpret_cast<uintptr_t>(first) & 3) == 0;   // then every case and colour starts on a dword
  const int tiles = divup(P, vec ? 256 : 64);
  // shares of the cases: what overflow asks for; beyond that only until about 512 blocks fill the chip, and never fewer than 32 cases
  // (8 per wave) a share — every share costs 2 * dims atomics
  int splits = max(divup(cases, kCmWaves * kCasesPerWave), min(divup(512, tiles), divup(cases, 32)));
  const int per_block = divup(cases, splits);
  splits = divup(cases, per_block);
  if (splits > 65535) return ERROR_UNSUPPORTED;
  const dim3 grid(tiles, splits);
  const char* name = vec ? "chunk_moments_kernel<4>" : "chunk_moments_kernel<1>";
  KernelTimer timer(name, "dataset_moments", 0.0, (double)C * P * (cases + 16.0 * splits));
  if (vec)
    hipLaunchKernelGGL((chunk_moments_kernel<C, 4>), grid, dim3(kCmThreads), 0, stream(), first, P, cases, per_block, acc);
  else
    hipLaunchKernelGGL((chunk_moments_kernel<C, 1>), grid, dim3(kCmThreads), 0, stream(), first, P, cases, per_block, acc);
  note_kernel(name, 0.0, tiles * splits, 1);
  return launch_status();
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" int chunk_moments_u8(void* chunk, int dims, int num_cases, int first_case, int cases, int num_colors, void* acc) {
  if (!chunk || !acc || (reinterpret_cast<uintptr_t>(acc) & 7) != 0) return ERROR_GENERIC;
  if (dims <= 0 || num_cases < 0 || num_colors <= 0 || dims % num_colors != 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (cases < 0 || first_case < 0 || (long)first_case + cases > (long)num_cases) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (num_colors > 4) return ERROR_UNSUPPORTED;
  if (cases == 0) return 0;
  const unsigned char* first = static_cast<const unsigned char*>(chunk) + (size_t)first_case * dims;
  u64* sums = static_cast<u64*>(acc);
  const int P = dims / num_colors;
  switch (num_colors) {
    case 1: return launch_chunk_moments<1>(first, P, cases, sums);
    case 2: return launch_chunk_moments<2>(first, P, cases, sums);
    case 3: return launch_chunk_moments<3>(first, P, cases, sums);
    default: return launch_chunk_moments<4>(first, P, cases, sums);
  }
}
