// Batch normalisation (Layer::ApplyBatchNormalization / ApplyDerivativeofBatchNormalization, src/layer.cc:452-510, and the cudamat
// entries bn_bprop_inplace / bn_bprop / bn_grad, cudamat.cu:1651,3454,3479).  gfx950 only.
//
// Layout: the layer's (N, X·Y·C) state read as Reshape(-1, C) — column c is the contiguous run of H = N·X·Y floats of
// channel c, and every statistic is a reduction down one column.
//
// Three kernel families, each an HBM stream:
//   stats   one read of x.  Every wave owns one segment of one column (a column of VGG conv1 at N = 128 is split over 128 waves, an FC
//           column of 128 floats is one wave) and writes one partial to a slab: forward (count, mean, M2) by per-lane Welford over
//           float4s and Chan's combine across lanes; backward the three sums Σd, Σd·z, Σz with z = (x - a)·r.
//   finish  one thread per column combines that column's partials in segment order (Chan for the forward) and writes the outputs the
//           reference writes (batch mean / std and the running averages; dgamma, dbeta) plus per-column coefficients for the apply.
//   apply   one read (and one write) of every element: forward (x - m)·(gamma/sigma) + beta [then max(., 0)]; backward
//           st·out + k2·(d - k1·z - k0).
// No float atomics and a fixed combine order everywhere: results are bit-identical from call to call.  The backward never writes the
// state it reads (the reference recovers y in place and restores it); y lives in registers.
#include <algorithm>
#include <climits>

#include "common.h"

namespace chip {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kThreads = 256;   // four waves; every wave is an independent unit of the stats kernels
constexpr int kWaves = kThreads / 64;

// Chan et al.: merge (nb, mb, m2b) into (n, mean, m2).  Either side may be empty.
__device__ inline void chan(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  if (n == 0.f) {
    n = nb, mean = mb, m2 = m2b;
    return;
  }
  const float nn = n + nb, d = mb - mean, r = nb / nn;
  mean += d * r;
  m2 += m2b + d * d * n * r;
  n = nn;
}

struct Seg {
  int H, S, L;   // column length, segments per column, segment length (a multiple of 256 floats)
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kThreads) bn_stats_kernel(const float* __restrict__ x, f32x4* __restrict__ part, Seg g, int units) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= units) return;   // whole waves only: nothing below synchronises across waves
  const int c = w / g.S, s = w - c * g.S;
  const int beg = s * g.L, end = min(g.H, beg + g.L);
  const float* col = x + (size_t)c * g.H;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (VEC) {
    for (int i = beg + 4 * lane; i < end; i += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(col + i);
      const float cm = (v.x + v.y + v.z + v.w) * 0.25f;
      const float a = v.x - cm, b = v.y - cm, e = v.z - cm, f = v.w - cm;
      chan(n, mean, m2, 4.f, cm, a * a + b * b + e * e + f * f);
    }
  } else {
    for (int i = beg + lane; i < end; i += 64) {
      const float v = col[i];
      n += 1.f;
      const float d = v - mean;
      mean += d / n;
      m2 += d * (v - mean);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float nb = __shfl_xor(n, o), mb = __shfl_xor(mean, o), m2b = __shfl_xor(m2, o);
    chan(n, mean, m2, nb, mb, m2b);
  }
  if (lane == 0) part[w] = f32x4{n, mean, m2, 0.f};
}

// coef[c] = {m, gamma/sigma, beta, 0}: train -> batch statistics from the slab (and the running averages, layer.cc:468-471);
// test -> the running statistics (layer.cc:473-474).
__global__ void bn_fwd_finish_kernel(const f32x4* __restrict__ part, int S, int C, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, float* __restrict__ mu, float* __restrict__ sigma,
                                     float* __restrict__ batch_mu, float* __restrict__ batch_sigma, float f, float eps, int train,
                                     f32x4* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float m, sd;
  if (train) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int s = 0; s < S; ++s) {
      const f32x4 p = part[(size_t)c * S + s];
      chan(n, mean, m2, p.x, p.y, p.z);
    }
    m = mean;
    sd = sqrtf(m2 / n + eps);   // biased variance; eps before the sqrt (layer.cc:462-464)
    batch_mu[c] = m;
    batch_sigma[c] = sd;
    const float g = 1.f - f;
    mu[c] = mu[c] * f + g * m;           // the running average of the STD, not of the variance
    sigma[c] = sigma[c] * f + g * sd;
  } else {
    m = mu[c];
    sd = sigma[c];
  }
  coef[c] = f32x4{m, gamma[c] / sd, beta[c], 0.f};
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) bn_fwd_apply_kernel(float* x, const f32x4* __restrict__ coef, unsigned H, unsigned n, int relu) {
  const unsigned stride = gridDim.x * blockDim.x;
  if (VEC) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (n >> 2); i += stride) {
      const f32x4 k = coef[(i << 2) / H];   // H % 4 == 0: the four floats share a column
      f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
      v = (v - k.x) * k.y + k.z;
      if (relu) v = f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
      reinterpret_cast<f32x4*>(x)[i] = v;
    }
  } else {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const f32x4 k = coef[i / H];
      float v = (x[i] - k.x) * k.y + k.z;
      if (relu) v = fmaxf(v, 0.f);
      x[i] = v;
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// z = (x - a[c]) · r[c], r = 1 / rdiv[c]; a == nullptr -> 0, rdiv == nullptr -> r = 1.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) bn_sums_kernel(const float* __restrict__ d, const float* __restrict__ x, const float* __restrict__ a,
                                                           const float* __restrict__ rdiv, f32x4* __restrict__ part, Seg g, int units) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= units) return;
  const int c = w / g.S, s = w - c * g.S;
  const int beg = s * g.L, end = min(g.H, beg + g.L);
  const float* dc = d + (size_t)c * g.H;
  const float* xc = x + (size_t)c * g.H;
  const float sh = a ? a[c] : 0.f, r = rdiv ? 1.f / rdiv[c] : 1.f;
  float sd = 0.f, sdz = 0.f, sz = 0.f;
  if (VEC) {
    for (int i = beg + 4 * lane; i < end; i += 256) {
      const f32x4 dv = *reinterpret_cast<const f32x4*>(dc + i);
      const f32x4 z = (*reinterpret_cast<const f32x4*>(xc + i) - sh) * r;
      sd += (dv.x + dv.y) + (dv.z + dv.w);
      sdz += (dv.x * z.x + dv.y * z.y) + (dv.z * z.z + dv.w * z.w);
      sz += (z.x + z.y) + (z.z + z.w);
    }
  } else {
    for (int i = beg + lane; i < end; i += 64) {
      const float dv = dc[i], z = (xc[i] - sh) * r;
      sd += dv;
      sdz += dv * z;
      sz += z;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sd += __shfl_xor(sd, o);
    sdz += __shfl_xor(sdz, o);
    sz += __shfl_xor(sz, o);
  }
  if (lane == 0) part[w] = f32x4{sd, sdz, sz, 0.f};
}

enum { BN_FUSED = 0, BN_INPLACE = 1, BN_BPROP = 2, BN_GRAD = 3 };

struct BwdArgs {
  const float* gamma;   // FUSED, BPROP
  const float* beta;    // FUSED: a = beta, rdiv = gamma
  const float* mu;      // BPROP, GRAD: a = mu
  const float* sigma;   // FUSED: batch sigma; BPROP: sigma; GRAD: rdiv = sigma
  float* dgamma;        // FUSED (mean), INPLACE (mean), GRAD (sum)
  float* dbeta;         // FUSED (mean), GRAD (sum)
};

// coef[2c] = {k0, k1, k2, a}, coef[2c + 1] = {r, ...}: out = st·out + k2·(d - k1·z - k0), z = (x - a)·r
__global__ void bn_bwd_finish_kernel(const f32x4* __restrict__ part, int S, int C, int H, int mode, BwdArgs p, f32x4* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float Sd = 0.f, Sdz = 0.f, Sz = 0.f;
  for (int s = 0; s < S; ++s) {
    const f32x4 q = part[(size_t)c * S + s];
    Sd += q.x, Sdz += q.y, Sz += q.z;
  }
  const float h = (float)H;
  float k0 = 0.f, k1 = 0.f, k2 = 1.f, a = 0.f, r = 1.f;
  if (mode == BN_FUSED) {
    // layer.cc:493-498: dbeta = mean(d); dgamma = mean(d·y); d -= dgamma·y; d -= mean(d); d *= gamma / batch_sigma
    k1 = Sdz / h;
    p.dgamma[c] = k1;
    p.dbeta[c] = Sd * (1.f / h);
    k0 = (Sd - k1 * Sz) / h;
    k2 = p.gamma[c] / p.sigma[c];
    a = p.beta[c];
    r = 1.f / p.gamma[c];
  } else if (mode == BN_INPLACE) {   // kBNBpropInplace (cudamat_kernels.cu:2113-2142)
    k1 = Sdz / h;
    p.dgamma[c] = k1;
    k0 = (Sd - k1 * Sz) / h;
  } else if (mode == BN_BPROP) {     // kBNBprop (cudamat_kernels.cu:2077-2111)
    const float sg = p.sigma[c];
    k1 = Sdz / ((h - 1.f) * sg * sg);
    k2 = p.gamma[c] / sg;
    k0 = (Sd - k1 * Sz) / h;
    a = p.mu[c];
  } else {                           // kBNGrad (cudamat_kernels.cu:2144-2168): sums, not means
    p.dgamma[c] = Sdz;
    p.dbeta[c] = Sd;
    return;
  }
  coef[2 * c] = f32x4{k0, k1, k2, a};
  coef[2 * c + 1] = f32x4{r, 0.f, 0.f, 0.f};
}

// `d` and `out` may be the same matrix (in place); `x` is only read.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_kernel(const float* d, const float* __restrict__ x, float* out,
                                                                const f32x4* __restrict__ coef, unsigned H, unsigned n, float st) {
  const unsigned stride = gridDim.x * blockDim.x;
  if (VEC) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (n >> 2); i += stride) {
      const unsigned c = (i << 2) / H;
      const f32x4 k = coef[2 * c];
      const float r = coef[2 * c + 1].x;
      const f32x4 z = (reinterpret_cast<const f32x4*>(x)[i] - k.w) * r;
      f32x4 v = (reinterpret_cast<const f32x4*>(d)[i] - k.y * z - k.x) * k.z;
      if (st != 0.f) v += st * reinterpret_cast<const f32x4*>(out)[i];
      reinterpret_cast<f32x4*>(out)[i] = v;
    }
  } else {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const unsigned c = i / H;
      const f32x4 k = coef[2 * c];
      const float z = (x[i] - k.w) * coef[2 * c + 1].x;
      float v = (d[i] - k.y * z - k.x) * k.z;
      if (st != 0.f) v += st * out[i];
      out[i] = v;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// About 8192 waves in all (32 per CU), at least 256 floats per wave, segment boundaries on 256-float (float4 x 64 lanes) steps.
Seg plan(int H, int C) {
  const long per_col = std::max(1L, 8192L / C);
  long L = (H + per_col - 1) / per_col;
  L = std::max(256L, (L + 255) / 256 * 256);
  return Seg{H, (int)((H + L - 1) / L), (int)L};
}

int apply_blocks(size_t items) { return (int)std::min<size_t>((items + kThreads - 1) / kThreads, 8192); }

bool is_vec(const cudamat* m, int C) { return m && m->on_device && (int)numel(m) == C; }

// Sums + finish (+ apply unless GRAD) of one backward mode.
int bn_backward(int mode, const float* d, const float* x, float* out, float st, int H, int C, BwdArgs p, const float* a,
                const float* rdiv) {
  const Seg g = plan(H, C);
  const int units = C * g.S;
  const size_t part_bytes = sizeof(f32x4) * (size_t)units;
  char* ws = static_cast<char*>(workspace(part_bytes + sizeof(f32x4) * 2 * (size_t)C));
  f32x4* part = reinterpret_cast<f32x4*>(ws);
  f32x4* coef = reinterpret_cast<f32x4*>(ws + part_bytes);
  const size_t n = (size_t)H * C;
  const bool vec = (H & 3) == 0 && aligned16(d) && aligned16(x) && aligned16(out);
  {
    KernelTimer timer(vec ? "bn_sums_kernel<vec>" : "bn_sums_kernel", "bn_bwd_sums", 0.0, 8.0 * n);
    if (vec)
      hipLaunchKernelGGL(bn_sums_kernel<true>, dim3(divup(units, kWaves)), dim3(kThreads), 0, stream(), d, x, a, rdiv, part, g, units);
    else
      hipLaunchKernelGGL(bn_sums_kernel<false>, dim3(divup(units, kWaves)), dim3(kThreads), 0, stream(), d, x, a, rdiv, part, g, units);
  }
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(divup(C, 256)), dim3(256), 0, stream(), part, g.S, C, H, mode, p, coef);
  if (mode != BN_GRAD) {
    KernelTimer timer(vec ? "bn_bwd_apply_kernel<vec>" : "bn_bwd_apply_kernel", "bn_bwd_apply", 0.0, (st != 0.f ? 16.0 : 12.0) * n);
    if (vec)
      hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(apply_blocks(n / 4)), dim3(kThreads), 0, stream(), d, x, out, coef, (unsigned)H,
                         (unsigned)n, st);
    else
      hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(apply_blocks(n)), dim3(kThreads), 0, stream(), d, x, out, coef, (unsigned)H,
                         (unsigned)n, st);
  }
  return launch_status();
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" {

int bn_fprop_act(cudamat* state, cudamat* gamma, cudamat* beta, cudamat* mu, cudamat* sigma, cudamat* batch_mu, cudamat* batch_sigma,
                 float bn_f, float bn_epsilon, int train, int relu) {
  if (!state->on_device) return ERROR_NOT_ON_DEVICE;
  if (state->is_trans) return ERROR_TRANSPOSED;
  const int C = (int)numel(gamma);
  if (C <= 0 || !is_vec(gamma, C) || !is_vec(beta, C) || !is_vec(mu, C) || !is_vec(sigma, C)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (train && (!is_vec(batch_mu, C) || !is_vec(batch_sigma, C))) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const size_t n = numel(state);
  if (n % C != 0 || n == 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (n > (size_t)INT_MAX) return ERROR_UNSUPPORTED;   // unsigned grid strides never wrap; H fits an int
  const int H = (int)(n / C);
  const Seg g = plan(H, C);
  const int units = C * g.S;
  const size_t part_bytes = train ? sizeof(f32x4) * (size_t)units : 0;
  char* ws = static_cast<char*>(workspace(part_bytes + sizeof(f32x4) * (size_t)C));
  f32x4* part = reinterpret_cast<f32x4*>(ws);
  f32x4* coef = reinterpret_cast<f32x4*>(ws + part_bytes);
  float* x = static_cast<float*>(state->data_device);
  const bool vec = (H & 3) == 0 && aligned16(x);
  if (train) {
    KernelTimer timer(vec ? "bn_stats_kernel<vec>" : "bn_stats_kernel", "bn_fwd_stats", 0.0, 4.0 * n);
    if (vec)
      hipLaunchKernelGGL(bn_stats_kernel<true>, dim3(divup(units, kWaves)), dim3(kThreads), 0, stream(), x, part, g, units);
    else
      hipLaunchKernelGGL(bn_stats_kernel<false>, dim3(divup(units, kWaves)), dim3(kThreads), 0, stream(), x, part, g, units);
  }
  hipLaunchKernelGGL(bn_fwd_finish_kernel, dim3(divup(C, 256)), dim3(256), 0, stream(), part, g.S, C,
                     static_cast<const float*>(gamma->data_device), static_cast<const float*>(beta->data_device),
                     static_cast<float*>(mu->data_device), static_cast<float*>(sigma->data_device),
                     train ? static_cast<float*>(batch_mu->data_device) : nullptr,
                     train ? static_cast<float*>(batch_sigma->data_device) : nullptr, bn_f, bn_epsilon, train, coef);
  {
    KernelTimer timer(vec ? "bn_fwd_apply_kernel<vec>" : "bn_fwd_apply_kernel", "bn_fwd_apply", 0.0, 8.0 * n);
    if (vec)
      hipLaunchKernelGGL(bn_fwd_apply_kernel<true>, dim3(apply_blocks(n / 4)), dim3(kThreads), 0, stream(), x, coef, (unsigned)H,
                         (unsigned)n, relu);
    else
      hipLaunchKernelGGL(bn_fwd_apply_kernel<false>, dim3(apply_blocks(n)), dim3(kThreads), 0, stream(), x, coef, (unsigned)H,
                         (unsigned)n, relu);
  }
  return launch_status();
}

int bn_bprop_fused(cudamat* deriv, cudamat* state, cudamat* gamma, cudamat* beta, cudamat* batch_sigma, cudamat* dgamma, cudamat* dbeta) {
  if (!deriv->on_device || !state->on_device) return ERROR_NOT_ON_DEVICE;
  if (deriv->is_trans || state->is_trans) return ERROR_TRANSPOSED;
  const int C = (int)numel(gamma);
  if (C <= 0 || !is_vec(gamma, C) || !is_vec(beta, C) || !is_vec(batch_sigma, C) || !is_vec(dgamma, C) || !is_vec(dbeta, C))
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  const size_t n = numel(deriv);
  if (numel(state) != n || n % C != 0 || n == 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (n > (size_t)INT_MAX) return ERROR_UNSUPPORTED;   // unsigned grid strides never wrap; H fits an int
  BwdArgs p{static_cast<const float*>(gamma->data_device), static_cast<const float*>(beta->data_device), nullptr,
            static_cast<const float*>(batch_sigma->data_device), static_cast<float*>(dgamma->data_device),
            static_cast<float*>(dbeta->data_device)};
  float* d = static_cast<float*>(deriv->data_device);
  return bn_backward(BN_FUSED, d, static_cast<const float*>(state->data_device), d, 0.f, (int)(n / C), C, p, p.beta, p.gamma);
}

// ---- the reference's cudamat entries (cudamat.cuh:298-303), with its checks and error codes ------------------------------------------
int bn_bprop_inplace(cudamat* deriv, cudamat* act, cudamat* dgamma) {
  const int h = deriv->size[0], w = deriv->size[1];
  if (!deriv->on_device || !act->on_device) return ERROR_NOT_ON_DEVICE;
  if (deriv->is_trans || act->is_trans) return ERROR_TRANSPOSED;
  if (act->size[0] != h || act->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (dgamma->size[0] != 1 || dgamma->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (h <= 0 || w <= 0) return 0;
  if ((size_t)h * w > (size_t)INT_MAX) return ERROR_UNSUPPORTED;
  BwdArgs p{nullptr, nullptr, nullptr, nullptr, static_cast<float*>(dgamma->data_device), nullptr};
  float* d = static_cast<float*>(deriv->data_device);
  return bn_backward(BN_INPLACE, d, static_cast<const float*>(act->data_device), d, 0.f, h, w, p, nullptr, nullptr);
}

int bn_bprop(cudamat* deriv, cudamat* input, cudamat* gamma, cudamat* mu, cudamat* sigma, cudamat* target, float scale_targets) {
  const int h = deriv->size[0], w = deriv->size[1];
  if (input->size[0] != h || input->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (target->size[0] != h || target->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (gamma->size[0] != 1 || gamma->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (mu->size[0] != 1 || mu->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (sigma->size[0] != 1 || sigma->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (h <= 0 || w <= 0) return 0;
  if ((size_t)h * w > (size_t)INT_MAX) return ERROR_UNSUPPORTED;
  BwdArgs p{static_cast<const float*>(gamma->data_device), nullptr, static_cast<const float*>(mu->data_device),
            static_cast<const float*>(sigma->data_device), nullptr, nullptr};
  return bn_backward(BN_BPROP, static_cast<const float*>(deriv->data_device), static_cast<const float*>(input->data_device),
                     static_cast<float*>(target->data_device), scale_targets, h, w, p, p.mu, nullptr);
}

int bn_grad(cudamat* deriv, cudamat* input, cudamat* mu, cudamat* sigma, cudamat* dgamma, cudamat* dbeta) {
  const int h = deriv->size[0], w = deriv->size[1];
  if (input->size[0] != h || input->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (mu->size[0] != 1 || mu->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (sigma->size[0] != 1 || sigma->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (dgamma->size[0] != 1 || dgamma->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (dbeta->size[0] != 1 || dbeta->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (h <= 0 || w <= 0) return 0;
  if ((size_t)h * w > (size_t)INT_MAX) return ERROR_UNSUPPORTED;
  BwdArgs p{nullptr, nullptr, static_cast<const float*>(mu->data_device), static_cast<const float*>(sigma->data_device),
            static_cast<float*>(dgamma->data_device), static_cast<float*>(dbeta->data_device)};
  float* d = static_cast<float*>(deriv->data_device);
  return bn_backward(BN_GRAD, d, static_cast<const float*>(input->data_device), d, 0.f, h, w, p, p.mu, p.sigma);
}

}  // extern "C"
