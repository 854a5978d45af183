// GPU-side input staging: the step right before the hot path.  The reference's DataHandler keeps a chunk
// of the dataset on the GPU as a (dims, cases) matrix — one case per COLUMN, [colour][row][col] contiguous — and every
// GetBatch turns a slice of it into the CHWN batch the conv kernels read (src/datahandler.cc:146-198,496-532):
//   extract_patches  random crop + horizontal flip + transpose to CHWN   (cudamat.cu:2699-2742, kExtractPatches2 :1655)
//   copy_transpose   the no-jitter case                                   (state.hip)
//   shuffleColumns   in-place pairwise column swaps by a permutation      (cudamat.cu:2655, kShuffleColumns :947)
//   add_col_vec / add_col_mult / div_by_col_vec / normalize_by_axis       mean/std normalisation (DataIterator::Preprocess)
//   add_to_each_pixel / mult_by_row_vec / div_by_row_vec                  PCA colour noise (DataIterator::AddPCANoise)
// Semantics pinned by eigenmat/eigenmat.cc:325-370,499-560,970-1005,1962-1988,2046-2090 (the CPU oracle).
// All HBM-bound byte shuffling: coalesced on both sides (LDS tile transpose where the two sides disagree), no GEMMs.
#include "common.h"

namespace chip {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;
inline int blocks_for(size_t items) {
  size_t b = (items + kThreads - 1) / kThreads;
  if (b > 4096) b = 4096;
  return b ? (int)b : 1;
}

// tile = 32 images x 32 patch columns of one (colour, patch row).  Read side: lane tx walks the source columns of image
// ty (128 contiguous bytes, reversed when flipped); write side: lane tx walks the images of patch column ty (128
// contiguous bytes of the CHWN batch).
__global__ void __launch_bounds__(256) extract_patches_kernel(const float* __restrict__ images, float* __restrict__ patches,
                                                              const float* __restrict__ wo, const float* __restrict__ ho,
                                                              const float* __restrict__ flip, int N, int W, int H, int pw, int ph,
                                                              int colors) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int c0 = blockIdx.x * 32;
  const int row = blockIdx.y % ph, color = blockIdx.y / ph;
  const int n0 = blockIdx.z * 32;
  for (int j = ty; j < 32; j += 8) {
    const int n = n0 + j, dc = c0 + tx;
    if (n < N && dc < pw) {
      int sc = (int)wo[n] + dc;
      if (flip[n] > 0.5f) sc = W - sc - 1;
      const int sr = (int)ho[n] + row;
      tile[j][tx] = images[(size_t)sc + (size_t)W * (sr + (size_t)H * (color + (size_t)colors * n))];
    }
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int dc = c0 + j, n = n0 + tx;
    if (n < N && dc < pw) patches[(size_t)n + (size_t)N * (dc + (size_t)pw * (row + (size_t)ph * color))] = tile[tx][j];
  }
}

// What the jitter of case n contributes to every address of patch row `row`: the source row (clamped into the image), the source column of
// patch column 0 and the direction the patch columns walk in (-1: flipped).  Patch column dc reads source column first + step * dc,
// clamped into the image by its reader.  No jitter: the patch is the image.
struct Jitter {
  int row, first, step;
};
template <bool JITTER>
__device__ __forceinline__ Jitter jitter_terms(const float* __restrict__ wo, const float* __restrict__ ho, const float* __restrict__ flip, int n,
                                               int row, int W, int H, int pw, int ph) {
  int sr = row, first = 0, step = 1;
  if (JITTER) {
    // (an offset beyond the image lands on the nearest border whatever its size: cut it short, so that nothing below overflows)
    sr += min(max((int)ho[n], -H - ph), H + ph);
    first = min(max((int)wo[n], -W - pw), W + pw);
    if (flip[n] > 0.5f) {
      first = W - first - 1;
      step = -1;
    }
  }
  return {min(max(sr, 0), H - 1), first, step};
}

// The write side of a 64 x 64 tile of one plane row, transposed: lane tx walks the images of patch column j, so a wave stores 256
// contiguous bytes of the CHWN batch.  `out` is where the plane row starts: patch column dc of image n is out[n + N * dc].
__device__ __forceinline__ void store_tile(const float (&tile)[64][65], float* __restrict__ out, int N, int n0, int pw, int c0, int tx, int ty) {
#pragma unroll 4
  for (int j = ty; j < 64; j += 4) {
    const int dc = c0 + j, n = n0 + tx;
    if (n < N && dc < pw) out[(size_t)n + (size_t)N * dc] = tile[tx][j];
  }
}

// The same crop + flip + transpose from a chunk kept in its stored type (one unsigned byte per pixel), with the cast and the mean / std
// normalisation of the SOURCE pixel on the way.  tile = 64 images x 64 patch columns of one (colour, patch row): twice the float
// kernel's in both directions, because a byte run of 32 columns is only 32 B.  Read side: the 64 lanes of a wave walk the source
// columns of one image (64 contiguous bytes, reversed when flipped, at any alignment; mean / std beside them as 256 contiguous bytes),
// 16 images per wave with all their loads in flight.  Write side: the 64 lanes walk the images of one patch column (256 contiguous,
// aligned bytes of the CHWN batch per wave store — the side that carries 4 of the 5 bytes per pixel).  What an image contributes to
// every address of its row — chunk column, source row, first source column and walking direction — is worked out once per block by
// the first wave and kept in LDS, so the pixel loop issues one global load per pixel (three with mean / std) instead of five (seven).
// The case index, the source row and the source column are clamped into range: no value in case_index / offsets / flip reads outside
// the chunk.
template <bool NORM, bool JITTER>
__global__ void __launch_bounds__(256) stage_patches_u8_kernel(const unsigned char* __restrict__ chunk, const float* __restrict__ case_index,
                                                               int num_cases, int colors, const float* __restrict__ mean,
                                                               const float* __restrict__ sdev, float* __restrict__ patches,
                                                               const float* __restrict__ wo, const float* __restrict__ ho,
                                                               const float* __restrict__ flip, int N, int W, int H, int pw, int ph) {
  __shared__ float tile[64][65];
  __shared__ size_t case_base[64];   // where the image's case starts in the chunk
  __shared__ int row_base[64];       // where its source row starts inside a case (< dims)
  __shared__ int col_first[64];      // source column of patch column 0 ...
  __shared__ int col_step[64];       // ... and the direction the patch columns walk in (-1: flipped)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  const int c0 = blockIdx.x * 64;
  const int row = blockIdx.y % ph, color = blockIdx.y / ph;
  const int n0 = blockIdx.z * 64;
  if (ty == 0 && n0 + tx < N) {
    const int n = n0 + tx;
    const Jitter k = jitter_terms<JITTER>(wo, ho, flip, n, row, W, H, pw, ph);
    const int col = min(max((int)case_index[n], 0), num_cases - 1);
    case_base[tx] = (size_t)colors * W * H * (size_t)col;
    row_base[tx] = W * (k.row + H * color);
    col_first[tx] = k.first;
    col_step[tx] = k.step;
  }
  __syncthreads();
#pragma unroll 4
  for (int j = ty; j < 64; j += 4) {
    const int n = n0 + j, dc = c0 + tx;
    if (n < N && dc < pw) {
      const int sc = min(max(col_first[j] + col_step[j] * dc, 0), W - 1);
      const int src = row_base[j] + sc;
      float v = (float)chunk[case_base[j] + (size_t)src];
      if (NORM) v = (v - mean[src]) / sdev[src];
      tile[j][tx] = v;
    }
  }
  __syncthreads();
  store_tile(tile, patches + (size_t)N * pw * (row + (size_t)ph * color), N, n0, pw, c0, tx, ty);
}

// The same staging for CLIPS out of a buffer that holds every frame once (one frame per column, [colour][row][col]): plane
// t * colours + c of a case is colour c of frame first_frame[case] + t, so a clip is clip_frames consecutive columns and overlapping
// clips share them.  The tile, the LDS transpose and the wave stores are stage_patches_u8_kernel's.  What differs: the source pixel —
// and with it mean / std — does not depend on t, so a block walks frames_per_block planes of its (colour, patch row, tile) with the 16
// source offsets of every lane and their mean / std in registers: per patch pixel one byte in and four out, and the 8 B of mean / std
// once per frames_per_block planes.  The bytes of plane t + 1 are loaded into registers before plane t is stored, so the gather's
// latency lies behind the stores.  Write side: where N is a multiple of 4 a lane stores 4 images of a patch column as one 16-B store
// (a quarter of the store instructions, which is what bounds the pass at small batches).  Rows of the tile past N and columns past the
// patch are loaded with image 0's LDS terms or clamped (in range) and never stored.
template <bool NORM, bool JITTER>
__global__ void __launch_bounds__(256) stage_clips_u8_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ first_frame,
                                                             int num_frames, int clip_frames, int frames_per_block, int colors,
                                                             const float* __restrict__ mean, const float* __restrict__ sdev,
                                                             float* __restrict__ patches, const float* __restrict__ wo,
                                                             const float* __restrict__ ho, const float* __restrict__ flip, int N, int W,
                                                             int H, int pw, int ph) {
  __shared__ float tile[64][65];
  __shared__ int frame_first[64];    // the clip's first frame column, clamped into the buffer
  __shared__ int row_base[64];       // where the source row starts inside a frame (< frame_dims)
  __shared__ int col_first[64];      // source column of patch column 0 ...
  __shared__ int col_step[64];       // ... and the direction the patch columns walk in (-1: flipped)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  const int c0 = blockIdx.x * 64;
  const int rows = ph * colors;
  const int rc = blockIdx.y % rows, t0 = (blockIdx.y / rows) * frames_per_block;
  const int t1 = min(t0 + frames_per_block, clip_frames);
  const int row = rc % ph, color = rc / ph;
  const int n0 = blockIdx.z * 64;
  if (ty == 0) {
    const int n = n0 + tx < N ? n0 + tx : 0;
    const Jitter k = jitter_terms<JITTER>(wo, ho, flip, n, row, W, H, pw, ph);
    frame_first[tx] = min(max((int)first_frame[n], 0), num_frames - 1);
    row_base[tx] = W * (k.row + H * color);
    col_first[tx] = k.first;
    col_step[tx] = k.step;
  }
  __syncthreads();
  const size_t frame_dims = (size_t)colors * W * H;
  const bool wide = N - n0 > 32;   // rows 32 ... of the tile hold an image (not in a batch of 32 or a tail tile); the same for the whole block
  auto each_row = [&](auto body) {   // this wave's tile rows j = ty + 4 i
#pragma unroll
    for (int i = 0; i < 8; ++i) body(i, ty + 4 * i);
    if (wide) {
#pragma unroll
      for (int i = 8; i < 16; ++i) body(i, ty + 4 * i);
    }
  };
  int src[16], px[16];
  float mu[16], sd[16];
  each_row([&](int i, int j) {
    src[i] = row_base[j] + min(max(col_first[j] + col_step[j] * (c0 + tx), 0), W - 1);
    if (NORM) {
      mu[i] = mean[src[i]];
      sd[i] = sdev[src[i]];
    }
  });
  auto load_plane = [&](int t) {
    each_row([&](int i, int j) { px[i] = frames[(size_t)min(frame_first[j] + t, num_frames - 1) * frame_dims + (size_t)src[i]]; });
  };
  load_plane(t0);
  const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(patches) & 15) == 0;   // four images of a patch column are one aligned 16-B store
  for (int t = t0; t < t1; ++t) {
    each_row([&](int i, int j) {
      float v = (float)px[i];
      if (NORM) v = (v - mu[i]) / sd[i];
      tile[j][tx] = v;
    });
    __syncthreads();
    if (t + 1 < t1) load_plane(t + 1);   // in flight behind this plane's stores
    float* out = patches + (size_t)N * pw * (row + (size_t)ph * ((size_t)t * colors + color));
    if (vec) {   // a lane takes 4 images of one patch column, a wave 4 columns of all 64: four runs of 256 contiguous bytes per store
      const int g = 4 * (tx & 15), n = n0 + g;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * (ty + 4 * k) + (tx >> 4), dc = c0 + j;
        if (n < N && dc < pw) {
          const f32x4 v = {tile[g][j], tile[g + 1][j], tile[g + 2][j], tile[g + 3][j]};
          *reinterpret_cast<f32x4*>(out + (size_t)n + (size_t)N * dc) = v;
        }
      }
    } else {
      store_tile(tile, out, N, n0, pw, c0, tx, ty);
    }
    __syncthreads();
  }
}

// The same staging out of DECODED IMAGE FILES kept at their original sizes (interleaved RGB rows, images back to back in one byte
// buffer), with the 8-bit bilinear resize of the crop's pixels on the way: the resized image is never stored.  Every image has one row
// of the image table {byte offset, w, h, new_w, new_h, first tap} (64-bit) and new_w column taps followed by new_h row taps
// {source index, coefficient 0, coefficient 1} (32-bit), built on the host; every case names its image, where the crop starts in the
// resized image and whether the crop is mirrored.  The tile, the LDS transpose and the wave stores are stage_patches_u8_kernel's, for the
// three colours of a patch pixel at once: one thread resamples one pixel in all three colours, because its four source pixels are 12
// interleaved bytes of two source rows (so the colours share their cache lines), and the tile is three planes of 64 x 65 floats.  A block
// owns one patch row, so what a case contributes to every pixel of it — the image's base and width, the two source rows and the row
// coefficients, where its column taps start, the first crop column and the walking direction — is worked out once by the first wave and
// kept in LDS; the pixel loop loads one column tap (12 B, consecutive lanes consecutive taps unless mirrored) and 12 bytes.
// Integer arithmetic only up to the cast (include/convnet_hip.h has the formula).  Everything read from a table is clamped: the image
// number, the tap numbers, the source row and column, the byte address.
struct ImageRow {
  size_t row0, row1;      // byte offsets of the two source rows in the buffer
  long col_taps;          // number of the image's first column tap
  int width, new_w;       // source and resized width, >= 1
  int b0, b1;             // the row coefficients
  int left, mirror;       // where the crop starts in the resized row, and whether it walks backwards
};

// Crop row r (0 ... img_height - 1) of the case whose case-table row is c, resolved through the image and tap tables.  The tables come
// from the host, so every value read from them is clamped here, once: the image number, the sizes (1 ... 2^30), the tap numbers, the
// crop's corner (+-2^30, so that the 64-bit sums below cannot overflow), the source row and the byte address.
__device__ __forceinline__ ImageRow image_row(const int* __restrict__ c, const long long* __restrict__ image_table, int num_images,
                                              const int* __restrict__ taps, long num_taps, size_t last, int r) {
  const long long* im = image_table + 6 * (size_t)min(max(c[0], 0), num_images - 1);
  const auto dim = [](long long v) { return (int)min(max(v, 1LL), 1LL << 30); };
  const int w = dim(im[1]), h = dim(im[2]), new_w = dim(im[3]), new_h = dim(im[4]);
  const long first_tap = (long)min(max(im[5], 0LL), (long long)num_taps - 1);
  const long rr = min(max((long)min(max(c[2], -(1 << 30)), 1 << 30) + r, 0L), (long)new_h - 1);   // the row of the resized image
  const int* t = taps + 3 * min(first_tap + new_w + rr, num_taps - 1);
  const int sy = min(max(t[0], 0), h - 1);
  const size_t base = (size_t)min(max(im[0], 0LL), (long long)last);
  ImageRow k;
  k.row0 = base + (size_t)sy * w * 3;
  k.row1 = base + (size_t)min(sy + 1, h - 1) * w * 3;
  k.col_taps = first_tap;
  k.width = w;
  k.new_w = new_w;
  k.b0 = t[1];
  k.b1 = t[2];
  k.left = min(max(c[1], -(1 << 30)), 1 << 30);
  k.mirror = c[3] != 0;
  return k;
}

__device__ inline int resample_row(const unsigned char* __restrict__ bytes, size_t last, size_t at0, size_t at1, int a0, int a1) {
  const int p0 = bytes[at0 < last ? at0 : last], p1 = bytes[at1 < last ? at1 : last];
  return (((2048 * ((p0 * a0 + p1 * a1) >> 4)) >> 16) + 2) >> 2;
}

// The three colours of crop column c (0 ... W - 1) of that row: the column of the resized image, its tap, the width pass on both source
// rows and the height pass (include/convnet_hip.h has the formula).  A pixel's 12 source bytes are interleaved in the two rows.
__device__ __forceinline__ void resample_pixel(const unsigned char* __restrict__ bytes, size_t last, const int* __restrict__ taps, long num_taps,
                                               const ImageRow& k, int c, int W, int (&v)[3]) {
  const long rc = min(max((long)k.left + (k.mirror ? W - 1 - c : c), 0L), (long)k.new_w - 1);   // the column of the resized image
  const int* t = taps + 3 * min(k.col_taps + rc, num_taps - 1);
  const int sx = min(max(t[0], 0), k.width - 1), a0 = t[1], a1 = t[2];
  const size_t x0 = (size_t)sx * 3, x1 = (size_t)min(sx + 1, k.width - 1) * 3;
#pragma unroll
  for (int color = 0; color < 3; ++color) {
    const int h0 = resample_row(bytes, last, k.row0 + x0 + color, k.row0 + x1 + color, a0, a1);
    const int h1 = resample_row(bytes, last, k.row1 + x0 + color, k.row1 + x1 + color, a0, a1);
    v[color] = (((k.b0 * ((2048 * h0) >> 4)) >> 16) + ((k.b1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2;
  }
}

// (stage_images_u8_kernel keeps its own spelling of the case terms, the jitter, the resample and the store — ImageCase and the kernel
// below — instead of jitter_terms / image_row / resample_pixel / store_tile: built on them it took 3 % longer on the MI355X, NOTES.md.  A
// clamp that changes in image_row changes here too.)
struct ImageCase {
  size_t row0, row1;      // byte offsets of the two source rows in the buffer
  int width;              // source width, >= 1
  int b0, b1;             // the row coefficients
  int new_w;              // resized width, >= 1
  long col_taps;          // number of the image's first column tap
  int left, mirror;       // where the crop starts in the resized row, and whether it walks backwards
  int col_first, col_step, crop_row;   // the jitter: crop column of patch column 0, direction, crop row
};

template <bool NORM, bool JITTER>
__global__ void __launch_bounds__(256) stage_images_u8_kernel(const unsigned char* __restrict__ bytes, size_t num_bytes,
                                                              const long long* __restrict__ image_table, int num_images,
                                                              const int* __restrict__ taps, long num_taps,
                                                              const int* __restrict__ case_table, const float* __restrict__ mean,
                                                              const float* __restrict__ sdev, float* __restrict__ patches,
                                                              const float* __restrict__ wo, const float* __restrict__ ho,
                                                              const float* __restrict__ flip, int N, int W, int H, int pw, int ph) {
  __shared__ float tile[3][64][65];
  __shared__ ImageCase cases[64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  const int c0 = blockIdx.x * 64;
  const int row = blockIdx.y;
  const int n0 = blockIdx.z * 64;
  const size_t last = num_bytes - 1;
  if (ty == 0 && n0 + tx < N) {
    const int n = n0 + tx;
    int sr = row, first = 0, step = 1;
    if (JITTER) {
      sr += min(max((int)ho[n], -H - ph), H + ph);
      first = min(max((int)wo[n], -W - pw), W + pw);
      if (flip[n] > 0.5f) {
        first = W - first - 1;
        step = -1;
      }
    }
    sr = min(max(sr, 0), H - 1);
    const int* c = case_table + 4 * (size_t)n;
    const long long* im = image_table + 6 * (size_t)min(max(c[0], 0), num_images - 1);
    const auto dim = [](long long v) { return (int)min(max(v, 1LL), 1LL << 30); };
    const int w = dim(im[1]), h = dim(im[2]), new_w = dim(im[3]), new_h = dim(im[4]);
    const long first_tap = (long)min(max(im[5], 0LL), (long long)num_taps - 1);
    const int rr = min(max(min(max(c[2], -(1 << 30)), 1 << 30) + sr, 0), new_h - 1);   // the row of the resized image
    const int* t = taps + 3 * min(first_tap + new_w + rr, num_taps - 1);
    const int sy = min(max(t[0], 0), h - 1);
    const size_t base = (size_t)min(max(im[0], 0LL), (long long)last);
    ImageCase& k = cases[tx];
    k.row0 = base + (size_t)sy * w * 3;
    k.row1 = base + (size_t)min(sy + 1, h - 1) * w * 3;
    k.width = w;
    k.b0 = t[1];
    k.b1 = t[2];
    k.new_w = new_w;
    k.col_taps = first_tap;
    k.left = min(max(c[1], -(1 << 30)), 1 << 30);
    k.mirror = c[3] != 0;
    k.col_first = first;
    k.col_step = step;
    k.crop_row = sr;
  }
  __syncthreads();
#pragma unroll 2
  for (int j = ty; j < 64; j += 4) {
    const int n = n0 + j, dc = c0 + tx;
    if (n < N && dc < pw) {
      const ImageCase& k = cases[j];
      const int sc = min(max(k.col_first + k.col_step * dc, 0), W - 1);                  // the column of the crop
      const int rc = min(max(k.left + (k.mirror ? W - 1 - sc : sc), 0), k.new_w - 1);      // the column of the resized image
      const int* t = taps + 3 * min(k.col_taps + rc, num_taps - 1);
      const int sx = min(max(t[0], 0), k.width - 1), a0 = t[1], a1 = t[2];
      const size_t x0 = (size_t)sx * 3, x1 = (size_t)min(sx + 1, k.width - 1) * 3;
      const int src = sc + W * k.crop_row;
#pragma unroll
      for (int color = 0; color < 3; ++color) {
        const int h0 = resample_row(bytes, last, k.row0 + x0 + color, k.row0 + x1 + color, a0, a1);
        const int h1 = resample_row(bytes, last, k.row1 + x0 + color, k.row1 + x1 + color, a0, a1);
        float v = (float)((((k.b0 * ((2048 * h0) >> 4)) >> 16) + ((k.b1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2);
        if (NORM) {
          const int s = src + W * H * color;
          v = (v - mean[s]) / sdev[s];
        }
        tile[color][j][tx] = v;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int color = 0; color < 3; ++color) {
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {
      const int dc = c0 + j, n = n0 + tx;
      if (n < N && dc < pw) patches[(size_t)n + (size_t)N * (dc + (size_t)pw * (row + (size_t)ph * color))] = tile[color][tx][j];
    }
  }
}

// The same staging for a jitter_raw_image stream (src/image_iterators.cc:231-285: the random translated crop, zoom and rotation of the
// decoded image): an image-table row of 11 values describes a VIEW of the file (first byte, crop width and height, the file's row
// stride), the size the crop is resized to, and — for a rotated image — where its rotation rows start in the tap table and the size of
// the window that is cut from the rotated image (include/convnet_hip.h has the layout and the formula).  A case's crop lies in that
// window.  An unrotated pixel is the resized crop's byte, as in stage_images_u8_kernel; a rotated pixel is the fixed-point blend of up to
// four resized-crop bytes around its source point, each the two-pass value of up to four source bytes, 0 outside the resized crop.  The
// tile, the LDS transpose, the wave stores and the three colours per thread are stage_images_u8_kernel's (a source pixel's colours are
// adjacent bytes).  Once per block the first wave works out what a (case, patch row) contributes to all its pixels: the view, the sizes,
// the tap rows, the crop column walk, and for an unrotated image the two source rows and the row coefficients, for a rotated one X0 / Y0
// of the window row.  A rotated pixel loads its column's rotation row, then per neighbour of non-zero weight a column tap, a row tap and
// 12 bytes; neighbours of weight 0 (a turn by a multiple of 90 degrees has only those) and neighbours outside the resized crop load
// nothing.  ROTATE false is the arm for a launch without a rotated image: a rotated flag in the table is then not honoured.
// Integer arithmetic only up to the cast.  Everything read from a table is clamped: the image number, the sizes (1 ... 2^30), the stride
// (0 ... 2^32), the tap and rotation rows, the window's column and row, the source indices inside the view, X / Y (+-2^30), the byte address.
struct JitterCase {
  size_t base;            // the view's first byte in the buffer
  size_t stride;          // bytes from one row of the view to the next
  size_t row0, row1;      // unrotated: byte offsets of the two source rows
  long taps;              // number of the image's first column tap; its row taps follow the new_w column taps
  long rot;               // rotated: number of the rotation row of window column 0
  int width, height;      // the view's size, >= 1
  int new_w, new_h;       // the size it is resized to, >= 1
  int win_w;              // the window's width (unrotated: new_w)
  int b0, b1;             // unrotated: the row coefficients
  int x0, y0;             // rotated: X0 and Y0 of the window row
  int rotated;
  int left, mirror;       // where the crop starts in the window's row, and whether it walks backwards
  int col_first, col_step, crop_row;   // the patch jitter: crop column of patch column 0, direction, crop row
};

// The three colours of pixel (ry, rx) of the resized view, 0 <= rx < new_w and 0 <= ry < new_h: both taps, the width pass on both
// source rows and the height pass.
__device__ __forceinline__ void resized_view_pixel(const unsigned char* __restrict__ bytes, size_t last, const int* __restrict__ taps,
                                                   long num_taps, const JitterCase& k, int rx, int ry, int (&v)[3]) {
  const int* tc = taps + 3 * min(k.taps + rx, num_taps - 1);
  const int* tr = taps + 3 * min(k.taps + k.new_w + ry, num_taps - 1);
  const int sx = min(max(tc[0], 0), k.width - 1), a0 = tc[1], a1 = tc[2];
  const int sy = min(max(tr[0], 0), k.height - 1), b0 = tr[1], b1 = tr[2];
  const size_t row0 = k.base + (size_t)sy * k.stride, row1 = k.base + (size_t)min(sy + 1, k.height - 1) * k.stride;
  const size_t x0 = (size_t)sx * 3, x1 = (size_t)min(sx + 1, k.width - 1) * 3;
#pragma unroll
  for (int color = 0; color < 3; ++color) {
    const int h0 = resample_row(bytes, last, row0 + x0 + color, row0 + x1 + color, a0, a1);
    const int h1 = resample_row(bytes, last, row1 + x0 + color, row1 + x1 + color, a0, a1);
    v[color] = (((b0 * ((2048 * h0) >> 4)) >> 16) + ((b1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2;
  }
}

template <bool NORM, bool JITTER, bool ROTATE>
__global__ void __launch_bounds__(256) stage_images_jitter_u8_kernel(const unsigned char* __restrict__ bytes, size_t num_bytes,
                                                                     const long long* __restrict__ image_table, int num_images,
                                                                     const int* __restrict__ taps, long num_taps,
                                                                     const int* __restrict__ case_table, const float* __restrict__ mean,
                                                                     const float* __restrict__ sdev, float* __restrict__ patches,
                                                                     const float* __restrict__ wo, const float* __restrict__ ho,
                                                                     const float* __restrict__ flip, int N, int W, int H, int pw, int ph) {
  __shared__ float tile[3][64][65];
  __shared__ JitterCase cases[64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  const int c0 = blockIdx.x * 64;
  const int row = blockIdx.y;
  const int n0 = blockIdx.z * 64;
  const size_t last = num_bytes - 1;
  if (ty == 0 && n0 + tx < N) {
    const int n = n0 + tx;
    int sr = row, first = 0, step = 1;
    if (JITTER) {
      sr += min(max((int)ho[n], -H - ph), H + ph);
      first = min(max((int)wo[n], -W - pw), W + pw);
      if (flip[n] > 0.5f) {
        first = W - first - 1;
        step = -1;
      }
    }
    sr = min(max(sr, 0), H - 1);
    const int* c = case_table + 4 * (size_t)n;
    const long long* im = image_table + 11 * (size_t)min(max(c[0], 0), num_images - 1);
    const auto dim = [](long long v) { return (int)min(max(v, 1LL), 1LL << 30); };
    const auto tap = [num_taps](long long v) { return (long)min(max(v, 0LL), (long long)num_taps - 1); };
    JitterCase& k = cases[tx];
    k.base = (size_t)min(max(im[0], 0LL), (long long)last);
    k.width = dim(im[1]);
    k.height = dim(im[2]);
    k.new_w = dim(im[3]);
    k.new_h = dim(im[4]);
    k.taps = tap(im[5]);
    k.stride = (size_t)min(max(im[6], 0LL), 1LL << 32);
    k.rotated = ROTATE && im[7] != 0;
    k.rot = tap(im[8]);
    k.win_w = k.rotated ? dim(im[9]) : k.new_w;
    const int win_h = k.rotated ? dim(im[10]) : k.new_h;
    const int wr = min(max(min(max(c[2], -(1 << 30)), 1 << 30) + sr, 0), win_h - 1);   // the row of the window
    k.row0 = k.row1 = 0;
    k.b0 = k.b1 = k.x0 = k.y0 = 0;
    if (k.rotated) {
      const int* t = taps + 3 * min(k.rot + k.win_w + wr, num_taps - 1);
      k.x0 = t[0];
      k.y0 = t[1];
    } else {
      const int* t = taps + 3 * min(k.taps + k.new_w + wr, num_taps - 1);
      const int sy = min(max(t[0], 0), k.height - 1);
      k.row0 = k.base + (size_t)sy * k.stride;
      k.row1 = k.base + (size_t)min(sy + 1, k.height - 1) * k.stride;
      k.b0 = t[1];
      k.b1 = t[2];
    }
    k.left = min(max(c[1], -(1 << 30)), 1 << 30);
    k.mirror = c[3] != 0;
    k.col_first = first;
    k.col_step = step;
    k.crop_row = sr;
  }
  __syncthreads();
#pragma unroll 2
  for (int j = ty; j < 64; j += 4) {
    const int n = n0 + j, dc = c0 + tx;
    if (n < N && dc < pw) {
      const JitterCase& k = cases[j];
      const int sc = min(max(k.col_first + k.col_step * dc, 0), W - 1);                  // the column of the crop
      const int wc = min(max(k.left + (k.mirror ? W - 1 - sc : sc), 0), k.win_w - 1);      // the column of the window
      int v[3] = {0, 0, 0};
      if (ROTATE && k.rotated) {
        const int* t = taps + 3 * min(k.rot + wc, num_taps - 1);                           // {adelta, bdelta, -}
        const long bound = 1L << 30;
        const int X = (int)min(max(((long)k.x0 + t[0]) >> 5, -bound), bound), Y = (int)min(max(((long)k.y0 + t[1]) >> 5, -bound), bound);
        const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rx = sx + (q & 1), ry = sy + (q >> 1);
          const int weight = ((q & 1) ? fx : 32 - fx) * ((q >> 1) ? fy : 32 - fy);
          if (weight != 0 && rx >= 0 && rx < k.new_w && ry >= 0 && ry < k.new_h) {
            int p[3];
            resized_view_pixel(bytes, last, taps, num_taps, k, rx, ry, p);
#pragma unroll
            for (int color = 0; color < 3; ++color) v[color] += weight * p[color];
          }
        }
#pragma unroll
        for (int color = 0; color < 3; ++color) v[color] = (v[color] + 512) >> 10;
      } else {
        const int* t = taps + 3 * min(k.taps + wc, num_taps - 1);
        const int sx = min(max(t[0], 0), k.width - 1), a0 = t[1], a1 = t[2];
        const size_t x0 = (size_t)sx * 3, x1 = (size_t)min(sx + 1, k.width - 1) * 3;
#pragma unroll
        for (int color = 0; color < 3; ++color) {
          const int h0 = resample_row(bytes, last, k.row0 + x0 + color, k.row0 + x1 + color, a0, a1);
          const int h1 = resample_row(bytes, last, k.row1 + x0 + color, k.row1 + x1 + color, a0, a1);
          v[color] = (((k.b0 * ((2048 * h0) >> 4)) >> 16) + ((k.b1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2;
        }
      }
      const int src = sc + W * k.crop_row;
#pragma unroll
      for (int color = 0; color < 3; ++color) {
        float f = (float)v[color];
        if (NORM) {
          const int s = src + W * H * color;
          f = (f - mean[s]) / sdev[s];
        }
        tile[color][j][tx] = f;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int color = 0; color < 3; ++color) {
#pragma unroll 4
    for (int j = ty; j < 64; j += 4) {
      const int dc = c0 + j, n = n0 + tx;
      if (n < N && dc < pw) patches[(size_t)n + (size_t)N * (dc + (size_t)pw * (row + (size_t)ph * color))] = tile[color][tx][j];
    }
  }
}

// The crops of the same decoded image files as STORED BYTES: case n's img_height x img_width crop of its resized image, planar R, G, B,
// at rows + n * 3 * H * W — a row of an HDF5 byte dataset, a column of a byte chunk (image2hdf5).  The tables and the integer arithmetic
// are stage_images_u8's; there is no cast, no mean / std and no patch.  The output is contiguous along the crop column, so nothing is
// transposed and no tile goes through LDS: consecutive lanes take consecutive groups of four crop columns of one (case, crop row),
// `1 << lanes_shift` lanes per row (64 from 256 columns on, fewer for a narrow crop so that its lanes are not idle), 256 >> lanes_shift
// rows per block.  What a (case, crop row) contributes to all its pixels is worked out once by one thread and kept in LDS, where its
// lanes read it: the two source rows' byte offsets, the row coefficients, the image's width, its first column tap, the left edge, the
// mirror flag (image_row's terms) and where the row starts in the output.  A thread resamples its four pixels in all three colours (the 12 source bytes of
// a pixel are interleaved in two source rows) and stores each colour as ONE dword where it owns four columns and the address is 4-byte
// aligned, as single bytes elsewhere: 3 * H * W and H * W need not be multiples of 4, so that differs per case and per plane.
// Everything read from a table is clamped as in stage_images_u8_kernel; every store lies inside rows by construction.
struct CropRow {
  ImageRow image;
  size_t out;             // where the crop row starts in the R plane of its case
};

__global__ void __launch_bounds__(256) crop_images_u8_kernel(const unsigned char* __restrict__ bytes, size_t num_bytes,
                                                             const long long* __restrict__ image_table, int num_images,
                                                             const int* __restrict__ taps, long num_taps,
                                                             const int* __restrict__ case_table, unsigned char* __restrict__ rows,
                                                             long total_rows, int W, int H, int lanes_shift) {
  __shared__ CropRow terms[256];
  const int rows_per_block = 256 >> lanes_shift;
  const long first_row = (long)blockIdx.x * rows_per_block;
  const size_t last = num_bytes - 1;
  const size_t plane = (size_t)H * W;
  if ((int)threadIdx.x < rows_per_block && first_row + threadIdx.x < total_rows) {
    const long row = first_row + threadIdx.x;      // (case, crop row), the crop row fastest
    const long n = row / H;
    const int r = (int)(row - n * H);
    terms[threadIdx.x].image = image_row(case_table + 4 * (size_t)n, image_table, num_images, taps, num_taps, last, r);
    terms[threadIdx.x].out = (size_t)n * 3 * plane + (size_t)r * W;
  }
  __syncthreads();
  const int j = threadIdx.x >> lanes_shift, lane = threadIdx.x & ((1 << lanes_shift) - 1);
  if (first_row + j >= total_rows) return;
  const CropRow k = terms[j];
  for (long c0 = 4L * lane; c0 < W; c0 += 4L << lanes_shift) {
    const int count = (int)min(4L, W - c0);          // the columns of this group inside the crop
    unsigned int px[3] = {0u, 0u, 0u};               // four columns of a colour, the first in the low byte
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < count) {
        int v[3];
        resample_pixel(bytes, last, taps, num_taps, k.image, (int)c0 + i, W, v);
#pragma unroll
        for (int color = 0; color < 3; ++color) px[color] |= (unsigned int)(v[color] & 255) << (8 * i);
      }
    }
#pragma unroll
    for (int color = 0; color < 3; ++color) {
      unsigned char* p = rows + k.out + plane * color + (size_t)c0;
      if (count == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned int*>(p) = px[color];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < count) p[i] = (unsigned char)(px[color] >> (8 * i));
      }
    }
  }
}

// The frames of ONE geometry resized to stored bytes (video2hdf5): every frame is `height` rows of `width` interleaved R, G, B pixels,
// the frames back to back, and every frame becomes new_height x new_width planar R, G, B bytes by the same new_width column taps and
// new_height row taps.  What crop_images_u8 reads per (case, row) and per pixel from global tables is the same for every frame here, so a
// block owns a tile of kRfRows x kRfCols output pixels of one frame and keeps in LDS
//   the tile's column and row taps (source indices clamped into the frame, the column mirrored), read once;
//   the source rows the tile needs, cut to the source columns it needs: 16-byte loads where the address allows, dwords and single bytes
//     at the two ragged ends of a row (a frame starts anywhere), kept at their alignment so that LDS and global chunks coincide;
//   the width pass h(y, .) of each of those rows, computed ONCE as bytes, planar, four columns to a dword;
// and takes the height pass from there: a thread makes four adjacent columns in all three colours and stores each colour as one dword
// where the address is 4-byte aligned, as single bytes elsewhere.  The source rows of a tile are the span from the smallest to the
// largest row its row taps name when that span fits the kRfSlots slots (adjacent output rows then share their source rows: every resize
// that shrinks the height less than 2x), else the two rows of every output row side by side (nothing shared, nothing lost).  A tile whose
// source columns do not fit a slot (a width shrunk more than ~2.5x, or taps that name columns all over the row) is not staged: its
// width pass reads the bytes from global memory one by one (resample_row), the scalar arm.  Both decisions come from the clamped taps'
// minima and maxima, so taps in any order give the pixels of the definition and never an access outside the buffers.  h(y, .) is kept
// as a byte, which it is for taps whose coefficients sum to 2048.
constexpr int kRfCols = 128;                 // output columns of a tile: 32 lanes x 4
constexpr int kRfRows = 16;                  // output rows of a tile
constexpr int kRfSlots = 2 * kRfRows;        // source rows of a tile
constexpr int kRfPitch = 1040;               // bytes of a staged source row, its lead of up to 15 and the over-read of the last pixel included
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

// the three bytes at byte `at` of an LDS row as one value (two aligned dwords)
__device__ __forceinline__ unsigned int lds_pixel(const unsigned int* row, int at) {
  const unsigned long long two = ((unsigned long long)row[(at >> 2) + 1] << 32) | row[at >> 2];
  return (unsigned int)(two >> (8 * (at & 3)));
}

__global__ void __launch_bounds__(256) resize_frames_u8_kernel(const unsigned char* __restrict__ bytes, size_t num_bytes, int width, int height,
                                                               const int* __restrict__ taps, int W, int H, int mirrored,
                                                               unsigned char* __restrict__ rows, int col_tiles, int row_tiles) {
  __shared__ __attribute__((aligned(16))) unsigned int src[kRfSlots][kRfPitch / 4];
  __shared__ unsigned int hb[kRfSlots][3][kRfCols / 4];   // h(slot's row, column) of a colour, four columns to a dword
  __shared__ int col_tap[kRfCols][4];                     // {x0, x1, a0, a1} of the tile's output columns
  __shared__ int row_tap[kRfRows][4];                     // {y0, y1, b0, b1} of its output rows
  __shared__ int row_slot[kRfRows][2];                    // the slots of y0 and y1
  __shared__ int slot_y[kRfSlots], slot_lead[kRfSlots];   // a slot's source row, and its first byte's address mod 16
  __shared__ int tile[6];                                 // first source column, staged bytes per row, staged, first source row, dense, slots
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = blockIdx.x % col_tiles, rt = (blockIdx.x / col_tiles) % row_tiles;
  const size_t n = blockIdx.x / col_tiles / row_tiles;
  const int c0 = ct * kRfCols, r0 = rt * kRfRows;
  const int ncols = min(kRfCols, W - c0), nrows = min(kRfRows, H - r0);
  const unsigned char* frame = bytes + n * ((size_t)width * height * 3);
  if (tid < kRfCols) {   // (columns past the tile's last repeat it: every entry is a tap of the table)
    const int c = c0 + min(tid, ncols - 1);
    const int* t = taps + 3 * (size_t)(mirrored ? W - 1 - c : c);
    const int x0 = min(max(t[0], 0), width - 1);
    col_tap[tid][0] = x0, col_tap[tid][1] = min(x0 + 1, width - 1), col_tap[tid][2] = t[1], col_tap[tid][3] = t[2];
  } else if (tid < kRfCols + kRfRows) {
    const int i = tid - kRfCols;
    const int* t = taps + 3 * ((size_t)W + r0 + min(i, nrows - 1));
    const int y0 = min(max(t[0], 0), height - 1);
    row_tap[i][0] = y0, row_tap[i][1] = min(y0 + 1, height - 1), row_tap[i][2] = t[1], row_tap[i][3] = t[2];
  }
  __syncthreads();
  if (wave < 2) {   // wave 0: the source columns of the tile; wave 1: its source rows
    int lo = wave == 0 ? min(col_tap[lane][0], col_tap[lane + 64][0]) : row_tap[lane & (kRfRows - 1)][0];
    int hi = wave == 0 ? max(col_tap[lane][1], col_tap[lane + 64][1]) : row_tap[lane & (kRfRows - 1)][1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      if (wave == 0) {
        const long len = 3L * ((long)hi - lo + 1);
        tile[0] = lo, tile[1] = (int)min(len, (long)kRfPitch), tile[2] = len + 32 <= kRfPitch;
      } else {
        const long span = (long)hi - lo + 1;
        tile[3] = lo, tile[4] = span <= kRfSlots, tile[5] = span <= kRfSlots ? (int)span : 2 * nrows;
      }
    }
  }
  __syncthreads();
  const int lo = tile[0], len = tile[1], staged = tile[2], ymin = tile[3], dense = tile[4], slots = tile[5];
  if (tid < slots) {
    const int y = dense ? ymin + tid : row_tap[tid >> 1][tid & 1];
    slot_y[tid] = y;
    slot_lead[tid] = (int)(reinterpret_cast<uintptr_t>(frame + (size_t)y * width * 3 + (size_t)lo * 3) & 15);
  } else if (tid >= 64 && tid < 64 + kRfRows) {
    const int i = tid - 64;
    row_slot[i][0] = dense ? row_tap[i][0] - ymin : 2 * i;
    row_slot[i][1] = dense ? row_tap[i][1] - ymin : 2 * i + 1;
  }
  __syncthreads();
  if (staged) {   // a wave per source row: byte k of the LDS row is byte k - lead of the row's needed part, so 16-byte chunks coincide
    for (int s = wave; s < slots; s += 4) {
      const int lead = slot_lead[s], end = lead + len;
      const unsigned char* g = frame + (size_t)slot_y[s] * width * 3 + (size_t)lo * 3 - lead;   // 16-byte aligned; read from g + lead on
      unsigned char* row = reinterpret_cast<unsigned char*>(src[s]);
      for (int k = 16 * lane; k < end; k += 16 * 64) {
        if (k >= lead && k + 16 <= end) {
          *reinterpret_cast<u32x4*>(row + k) = *reinterpret_cast<const u32x4*>(g + k);
        } else {
#pragma unroll
          for (int d = k; d < k + 16; d += 4) {
            if (d >= lead && d + 4 <= end) {
              *reinterpret_cast<unsigned int*>(row + d) = *reinterpret_cast<const unsigned int*>(g + d);
            } else {
#pragma unroll
              for (int b = d; b < d + 4; ++b)
                if (b >= lead && b < end) row[b] = g[b];
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const int group = tid & 31, sub = tid >> 5;   // four adjacent columns; one of 8 rows at a time
  if (4 * group < ncols) {
    int x0[4], x1[4], a0[4], a1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int* t = col_tap[4 * group + i];
      x0[i] = 3 * (t[0] - lo), x1[i] = 3 * (t[1] - lo), a0[i] = t[2], a1[i] = t[3];
    }
    for (int s = sub; s < slots; s += 8) {
      unsigned int h[3] = {0u, 0u, 0u};
      if (staged) {
        const unsigned int* row = src[s];
        const int lead = slot_lead[s];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned int p0 = lds_pixel(row, lead + x0[i]), p1 = lds_pixel(row, lead + x1[i]);
#pragma unroll
          for (int color = 0; color < 3; ++color) {
            const int v = (int)((p0 >> (8 * color)) & 255) * a0[i] + (int)((p1 >> (8 * color)) & 255) * a1[i];
            h[color] |= (unsigned int)(((((2048 * (v >> 4)) >> 16) + 2) >> 2) & 255) << (8 * i);
          }
        }
      } else {
        const size_t at = n * ((size_t)width * height * 3) + ((size_t)slot_y[s] * width + lo) * 3, last = num_bytes - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int color = 0; color < 3; ++color)
            h[color] |= (unsigned int)(resample_row(bytes, last, at + x0[i] + color, at + x1[i] + color, a0[i], a1[i]) & 255) << (8 * i);
      }
#pragma unroll
      for (int color = 0; color < 3; ++color) hb[s][color][group] = h[color];
    }
  }
  __syncthreads();
  if (4 * group >= ncols) return;
  const size_t plane = (size_t)H * W;
  const int count = min(4, ncols - 4 * group);
  for (int i = sub; i < nrows; i += 8) {
    const int s0 = row_slot[i][0], s1 = row_slot[i][1], b0 = row_tap[i][2], b1 = row_tap[i][3];
#pragma unroll
    for (int color = 0; color < 3; ++color) {
      const unsigned int h0 = hb[s0][color][group], h1 = hb[s1][color][group];
      unsigned int px = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v0 = (int)((h0 >> (8 * k)) & 255), v1 = (int)((h1 >> (8 * k)) & 255);
        px |= (unsigned int)(((((b0 * ((2048 * v0) >> 4)) >> 16) + ((b1 * ((2048 * v1) >> 4)) >> 16) + 2) >> 2) & 255) << (8 * k);
      }
      unsigned char* p = rows + n * 3 * plane + plane * color + (size_t)(r0 + i) * W + (size_t)(c0 + 4 * group);
      if (count == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned int*>(p) = px;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < count) p[k] = (unsigned char)(px >> (8 * k));
      }
    }
  }
}

// 0: the launcher's choice; 1: every block stages all the clip's planes of its tile; 2: one plane per block (tools/clips_bench.py's A/B)
int g_stage_clips_grid = 0;

// one block per column pair (2j, 2j+1): swap columns idx[2j] and idx[2j+1] of the matrix in place
__global__ void shuffle_columns_kernel(float* __restrict__ m, const float* __restrict__ idx, int height, int width) {
  const int c = 2 * blockIdx.x;
  if (c + 1 >= width) return;   // odd tail: the reference copies the column onto itself
  float* a = m + (size_t)height * (int)idx[c];
  float* b = m + (size_t)height * (int)idx[c + 1];
  if (a == b) return;
  const bool v4 = (height & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  if (v4) {
    for (int i = threadIdx.x; i < (height >> 2); i += blockDim.x) {
      const f32x4 x = reinterpret_cast<f32x4*>(a)[i], y = reinterpret_cast<f32x4*>(b)[i];
      reinterpret_cast<f32x4*>(a)[i] = y;
      reinterpret_cast<f32x4*>(b)[i] = x;
    }
  } else {
    for (int i = threadIdx.x; i < height; i += blockDim.x) {
      const float x = a[i], y = b[i];
      a[i] = y;
      b[i] = x;
    }
  }
}

// target[i + h*j] = f(mat[i + h*j], i, j)
template <typename F>
__global__ void rowcol_map_kernel(const float* __restrict__ mat, float* __restrict__ target, int h, size_t n, F f) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    const size_t j = k / h;
    const int i = (int)(k - j * h);
    target[k] = f(mat[k], i, (int)j);
  }
}

template <typename F>
int rowcol_map(cudamat* mat, cudamat* target, F f) {
  const size_t n = numel(mat);
  if (n == 0) return 0;
  hipLaunchKernelGGL(rowcol_map_kernel<F>, dim3(blocks_for(n)), dim3(kThreads), 0, stream(), mat->data_device, target->data_device,
                     mat->size[0], n, f);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

// column j: target = mat - mean(mat[:, j])   (normalize_by_axis axis 0, eigenmat.cc:982-997)
__global__ void center_columns_kernel(const float* __restrict__ mat, float* __restrict__ target, int height) {
  __shared__ float sh[4];
  const float* col = mat + (size_t)blockIdx.x * height;
  float* out = target + (size_t)blockIdx.x * height;
  float s = 0.f;
  for (int i = threadIdx.x; i < height; i += blockDim.x) s += col[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  const float mean = ((sh[0] + sh[1]) + (sh[2] + sh[3])) / (float)height;
  for (int i = threadIdx.x; i < height; i += blockDim.x) out[i] = col[i] - mean;
}

int check_colvec(const cudamat* mat, const cudamat* vec, const cudamat* target) {
  if (!mat->on_device || !vec->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (mat->size[0] != vec->size[0] || vec->size[1] != 1 || mat->size[0] != target->size[0] || mat->size[1] != target->size[1])
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  return 0;
}
int check_rowvec(const cudamat* mat, const cudamat* vec, const cudamat* target) {
  if (!mat->on_device || !vec->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (mat->size[1] != vec->size[1] || vec->size[0] != 1 || mat->size[0] != target->size[0] || mat->size[1] != target->size[1])
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  return 0;
}

// The arguments the byte-staging entries (stage_patches_u8, stage_clips_u8, stage_images_u8) share and what checking them works out.  A
// case is ``planes`` columns of ``dims`` bytes out of ``count`` (1: a chunk of cases or of images; clip_frames: a buffer of frames),
// ``index`` names the (first) column of every case where the entry has one (nullptr: stage_images_u8, whose tables are plain device
// pointers), and a block stages ``planes_per_block`` planes of ``colors_per_block`` colours of its 64 x 64 tile.
struct StageU8 {
  int dims, count;
  cudamat *index, *mean, *sdev, *patches, *width_offset, *height_offset, *flip;
  int img_width, img_height, patch_width, patch_height, planes, planes_per_block, colors_per_block;
  bool norm, jitter;
  int num_colors, num_images;   // (0 images: nothing to launch)
  long grid_y;
  const float *index_dev, *mean_dev, *sdev_dev, *wo_dev, *ho_dev, *flip_dev;   // the operands on the device; nullptr: not given
};

// Error code or 0, in the precedence tests/test_stage_patches_gpu.py, test_stage_clips_gpu.py and test_stage_images_gpu.py list, behind
// the entry's own code for a null pointer.
int check_stage_u8(StageU8& s) {
  s.norm = s.mean || s.sdev;
  s.jitter = s.width_offset || s.height_offset || s.flip;
  if ((s.norm && !(s.mean && s.sdev)) || (s.jitter && !(s.width_offset && s.height_offset && s.flip))) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if ((s.index && !s.index->on_device) || !s.patches->on_device || (s.norm && (!s.mean->on_device || !s.sdev->on_device)) ||
      (s.jitter && (!s.width_offset->on_device || !s.height_offset->on_device || !s.flip->on_device)))
    return ERROR_NOT_ON_DEVICE;
  if (s.patches->is_trans) return ERROR_TRANSPOSED;
  if (s.dims <= 0 || s.count <= 0 || s.planes <= 0 || s.img_width <= 0 || s.img_height <= 0 || s.patch_width <= 0 || s.patch_height <= 0)
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (s.patch_width > s.img_width || s.patch_height > s.img_height) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (!s.jitter && (s.patch_width != s.img_width || s.patch_height != s.img_height)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (s.dims % ((long)s.img_width * s.img_height) != 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  s.num_colors = s.dims / (s.img_width * s.img_height);
  const size_t num_images = s.num_images = s.patches->size[0];
  if ((long)s.patches->size[1] != (long)s.planes * s.num_colors * s.patch_width * s.patch_height || (s.index && numel(s.index) != num_images))
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (s.norm && (s.mean->size[0] != s.dims || s.mean->size[1] != 1 || s.sdev->size[0] != s.dims || s.sdev->size[1] != 1))
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (s.jitter && (numel(s.width_offset) != num_images || numel(s.height_offset) != num_images || numel(s.flip) != num_images))
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (s.count > (1 << 24)) return ERROR_UNSUPPORTED;   // a column number must be exact as a float
  const auto dev = [](const cudamat* m) { return m ? m->data_device : nullptr; };
  s.index_dev = dev(s.index), s.mean_dev = dev(s.mean), s.sdev_dev = dev(s.sdev);
  s.wo_dev = dev(s.width_offset), s.ho_dev = dev(s.height_offset), s.flip_dev = dev(s.flip);
  if (num_images == 0) return 0;
  s.grid_y = (long)s.patch_height * divup(s.num_colors, s.colors_per_block) * divup(s.planes, s.planes_per_block);
  return s.grid_y > 65535 || divup(s.num_images, 64) > 65535 ? ERROR_UNSUPPORTED : 0;
}

// the instantiation of a byte-staging kernel template for (norm, jitter)
#define STAGE_U8_KERNEL(kernel, s) \
  ((s).norm ? ((s).jitter ? kernel<true, true> : kernel<true, false>) : ((s).jitter ? kernel<false, true> : kernel<false, false>))

// ``source``: the kernel's own arguments, in front of the shared operands and the geometry
template <typename Kernel, typename... Source>
int launch_stage_u8(const StageU8& s, Kernel kernel, Source... source) {
  const dim3 grid(divup(s.patch_width, 64), (unsigned)s.grid_y, divup(s.num_images, 64));
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream(), source..., s.mean_dev, s.sdev_dev, s.patches->data_device, s.wo_dev, s.ho_dev,
                     s.flip_dev, s.num_images, s.img_width, s.img_height, s.patch_width, s.patch_height);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

// What stage_images_u8 and crop_images_u8 take alike — the decoded images, their three tables and the crop size — and the codes both
// report first; ``target`` is where the entry writes.
int check_image_tables(const void* bytes, size_t num_bytes, const void* image_table, const void* taps, int num_taps, const void* case_table,
                       const void* target, int img_width, int img_height) {
  if (!bytes || !image_table || !taps || !case_table || !target) return ERROR_GENERIC;
  return num_bytes == 0 || num_taps <= 0 || img_width <= 0 || img_height <= 0 ? ERROR_INCOMPATIBLE_DIMENSIONS : 0;
}

}  // namespace
}  // namespace chip

using namespace chip;

extern "C" {

int extract_patches(cudamat* images, cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip, int img_width,
                    int img_height, int patch_width, int patch_height) {
  if (!images->on_device || !patches->on_device || !width_offset->on_device || !height_offset->on_device || !flip->on_device)
    return ERROR_NOT_ON_DEVICE;
  if (img_width <= 0 || img_height <= 0 || patch_width <= 0 || patch_height <= 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int num_images = images->size[1];
  const int num_colors = images->size[0] / (img_width * img_height);
  if (patches->size[1] != num_colors * patch_width * patch_height || patches->size[0] != num_images) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if ((int)numel(width_offset) != num_images || (int)numel(height_offset) != num_images || (int)numel(flip) != num_images)
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (num_images == 0 || num_colors == 0) return 0;
  if (patch_height * num_colors > 65535 || divup(num_images, 32) > 65535) return ERROR_UNSUPPORTED;
  KernelTimer timer("extract_patches_kernel", "input_staging", 0.0, 8.0 * numel(patches));
  const dim3 grid(divup(patch_width, 32), patch_height * num_colors, divup(num_images, 32));
  hipLaunchKernelGGL(extract_patches_kernel, grid, dim3(256), 0, stream(), images->data_device, patches->data_device,
                     width_offset->data_device, height_offset->data_device, flip->data_device, num_images, img_width, img_height,
                     patch_width, patch_height, num_colors);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

int stage_patches_u8(void* chunk, int dims, int num_cases, cudamat* case_index, cudamat* mean, cudamat* sdev, cudamat* patches,
                     cudamat* width_offset, cudamat* height_offset, cudamat* flip, int img_width, int img_height, int patch_width,
                     int patch_height) {
  if (!chunk || !case_index || !patches) return ERROR_NOT_ON_DEVICE;
  StageU8 s{dims, num_cases, case_index, mean, sdev, patches, width_offset, height_offset, flip, img_width, img_height, patch_width,
            patch_height, 1, 1, 1};
  if (const int e = check_stage_u8(s); e || s.num_images == 0) return e;
  KernelTimer timer("stage_patches_u8_kernel", "input_staging", 0.0, 5.0 * numel(patches));
  return launch_stage_u8(s, STAGE_U8_KERNEL(stage_patches_u8_kernel, s), static_cast<const unsigned char*>(chunk), s.index_dev, num_cases,
                         s.num_colors);
}

void convnet_hip_set_stage_clips_grid(int mode) { g_stage_clips_grid = mode == 1 || mode == 2 ? mode : 0; }

int stage_clips_u8(void* frames, int frame_dims, int num_frames, cudamat* first_frame, int clip_frames, cudamat* mean, cudamat* sdev,
                   cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip, int img_width, int img_height,
                   int patch_width, int patch_height) {
  if (!frames || !first_frame || !patches) return ERROR_NOT_ON_DEVICE;
  const int frames_per_block = g_stage_clips_grid == 2 ? 1 : clip_frames;
  StageU8 s{frame_dims, num_frames, first_frame, mean, sdev, patches, width_offset, height_offset, flip, img_width, img_height,
            patch_width, patch_height, clip_frames, frames_per_block, 1};
  if (const int e = check_stage_u8(s); e || s.num_images == 0) return e;
  KernelTimer timer("stage_clips_u8_kernel", "input_staging", 0.0, (5.0 + (s.norm ? 8.0 / frames_per_block : 0.0)) * numel(patches));
  return launch_stage_u8(s, STAGE_U8_KERNEL(stage_clips_u8_kernel, s), static_cast<const unsigned char*>(frames), s.index_dev, num_frames,
                         clip_frames, frames_per_block, s.num_colors);
}

int stage_images_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                    cudamat* mean, cudamat* sdev, cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip,
                    int img_width, int img_height, int patch_width, int patch_height) {
  if (const int e = check_image_tables(bytes, num_bytes, image_table, taps, num_taps, case_table, patches, img_width, img_height)) return e;
  if ((long)img_width * img_height > (1 << 28)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  // the rest is stage_patches_u8's checker on a crop of three colours, which a block stages together
  StageU8 s{3 * img_width * img_height, num_images, nullptr, mean, sdev, patches, width_offset, height_offset, flip, img_width, img_height,
            patch_width, patch_height, 1, 1, 3};
  if (const int e = check_stage_u8(s); e || s.num_images == 0) return e;
  KernelTimer timer("stage_images_u8_kernel", "input_staging", 0.0, 16.0 * numel(patches));
  return launch_stage_u8(s, STAGE_U8_KERNEL(stage_images_u8_kernel, s), static_cast<const unsigned char*>(bytes), num_bytes,
                         static_cast<const long long*>(image_table), num_images, static_cast<const int*>(taps), (long)num_taps,
                         static_cast<const int*>(case_table));
}

int stage_images_jitter_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                           int rotated, cudamat* mean, cudamat* sdev, cudamat* patches, cudamat* width_offset, cudamat* height_offset,
                           cudamat* flip, int img_width, int img_height, int patch_width, int patch_height) {
  if (const int e = check_image_tables(bytes, num_bytes, image_table, taps, num_taps, case_table, patches, img_width, img_height)) return e;
  if ((long)img_width * img_height > (1 << 28)) return ERROR_INCOMPATIBLE_DIMENSIONS;
  // the rest is stage_images_u8's: stage_patches_u8's checker on a crop of three colours, which a block stages together
  StageU8 s{3 * img_width * img_height, num_images, nullptr, mean, sdev, patches, width_offset, height_offset, flip, img_width, img_height,
            patch_width, patch_height, 1, 1, 3};
  if (const int e = check_stage_u8(s); e || s.num_images == 0) return e;
  KernelTimer timer(rotated ? "stage_images_jitter_u8_kernel<rotate>" : "stage_images_jitter_u8_kernel", "input_staging", 0.0,
                    (rotated ? 52.0 : 16.0) * numel(patches));
  const auto launch = [&](auto kernel) {
    return launch_stage_u8(s, kernel, static_cast<const unsigned char*>(bytes), num_bytes, static_cast<const long long*>(image_table),
                           num_images, static_cast<const int*>(taps), (long)num_taps, static_cast<const int*>(case_table));
  };
  if (rotated) {
    if (s.norm) return s.jitter ? launch(stage_images_jitter_u8_kernel<true, true, true>) : launch(stage_images_jitter_u8_kernel<true, false, true>);
    return s.jitter ? launch(stage_images_jitter_u8_kernel<false, true, true>) : launch(stage_images_jitter_u8_kernel<false, false, true>);
  }
  if (s.norm) return s.jitter ? launch(stage_images_jitter_u8_kernel<true, true, false>) : launch(stage_images_jitter_u8_kernel<true, false, false>);
  return s.jitter ? launch(stage_images_jitter_u8_kernel<false, true, false>) : launch(stage_images_jitter_u8_kernel<false, false, false>);
}

int crop_images_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                   int num_cases, void* rows, int img_width, int img_height) {
  if (const int e = check_image_tables(bytes, num_bytes, image_table, taps, num_taps, case_table, rows, img_width, img_height)) return e;
  if (num_images <= 0 || num_cases <= 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (num_images > (1 << 24)) return ERROR_UNSUPPORTED;
  int lanes_shift = 0;   // lanes per (case, crop row): the power of two that covers its groups of four columns, 64 at the most
  while (lanes_shift < 6 && (4L << lanes_shift) < img_width) ++lanes_shift;
  const long total_rows = (long)num_cases * img_height;
  const long rows_per_block = 256 >> lanes_shift;
  const long blocks = (total_rows + rows_per_block - 1) / rows_per_block;
  if (blocks > 0x7fffffffL) return ERROR_UNSUPPORTED;
  KernelTimer timer("crop_images_u8_kernel", "input_staging", 0.0, 5.0 * 3.0 * (double)total_rows * img_width);
  hipLaunchKernelGGL(crop_images_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream(), static_cast<const unsigned char*>(bytes),
                     num_bytes, static_cast<const long long*>(image_table), num_images, static_cast<const int*>(taps), (long)num_taps,
                     static_cast<const int*>(case_table), static_cast<unsigned char*>(rows), total_rows, img_width, img_height,
                     lanes_shift);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

int resize_frames_u8(void* bytes, size_t num_bytes, int num_frames, int width, int height, void* taps, int new_width, int new_height,
                     int mirrored, void* rows) {
  if (!bytes || !taps || !rows) return ERROR_GENERIC;
  if (num_frames <= 0 || width <= 0 || height <= 0 || new_width <= 0 || new_height <= 0) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const size_t pixels = (size_t)width * height;   // (< 2^62)
  if (pixels > ~(size_t)0 / 3 / (size_t)num_frames || num_bytes < pixels * 3 * (size_t)num_frames) return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int col_tiles = divup(new_width, kRfCols), row_tiles = divup(new_height, kRfRows);
  const long tiles = (long)col_tiles * row_tiles;
  if (tiles > 0x7fffffffL / num_frames || width > 0x7fffffff / 3) return ERROR_UNSUPPORTED;   // (a source row's bytes are counted in an int)
  KernelTimer timer("resize_frames_u8_kernel", "input_staging", 0.0,
                    3.0 * num_frames * ((double)pixels + (double)new_width * new_height));
  hipLaunchKernelGGL(resize_frames_u8_kernel, dim3((unsigned)(tiles * num_frames)), dim3(256), 0, stream(),
                     static_cast<const unsigned char*>(bytes), num_bytes, width, height, static_cast<const int*>(taps), new_width, new_height,
                     mirrored != 0, static_cast<unsigned char*>(rows), col_tiles, row_tiles);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

int shuffleColumns(cudamat* source, cudamat* rand_perm_indices) {
  if (!source->on_device || !rand_perm_indices->on_device) return ERROR_NOT_ON_DEVICE;
  const int h = source->size[0], w = source->size[1];
  if (rand_perm_indices->size[0] != 1 || rand_perm_indices->size[1] != w) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (w < 2 || h == 0) return 0;
  KernelTimer timer("shuffle_columns_kernel", "input_staging", 0.0, 8.0 * numel(source));
  hipLaunchKernelGGL(shuffle_columns_kernel, dim3(w / 2), dim3(256), 0, stream(), source->data_device, rand_perm_indices->data_device, h, w);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

int add_col_mult(cudamat* mat, cudamat* vec, cudamat* target, float mult) {
  if (const int e = check_colvec(mat, vec, target)) return e;
  const float* v = vec->data_device;
  return rowcol_map(mat, target, [=] __device__(float x, int i, int) { return x + mult * v[i]; });
}
int add_col_vec(cudamat* mat, cudamat* vec, cudamat* target) { return add_col_mult(mat, vec, target, 1.0f); }

int div_by_col_vec(cudamat* mat, cudamat* vec, cudamat* target) {
  if (const int e = check_colvec(mat, vec, target)) return e;
  const float* v = vec->data_device;
  return rowcol_map(mat, target, [=] __device__(float x, int i, int) { return x / v[i]; });
}

int mult_by_row_vec(cudamat* mat, cudamat* vec, cudamat* target) {
  if (const int e = check_rowvec(mat, vec, target)) return e;
  const float* v = vec->data_device;
  return rowcol_map(mat, target, [=] __device__(float x, int, int j) { return x * v[j]; });
}

int div_by_row_vec(cudamat* mat, cudamat* vec, cudamat* target) {
  if (const int e = check_rowvec(mat, vec, target)) return e;
  const float* v = vec->data_device;
  return rowcol_map(mat, target, [=] __device__(float x, int, int j) { return x / v[j]; });
}

// target[i] = mat1[i] + mult * mat2[i % height + height * (i / num_pix)],  num_pix = height*width / num_colors
// (mat1 = a (cases, colours*pixels) batch, mat2 = (cases, colours) per-case colour noise; eigenmat.cc:346-366)
int add_to_each_pixel(cudamat* mat1, cudamat* mat2, cudamat* target, float mult) {
  if (!mat1->on_device || !mat2->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat1->is_trans || mat2->is_trans) return ERROR_TRANSPOSED;
  if (mat1->size[0] != mat2->size[0] || mat2->size[1] == 0 || mat1->size[1] % mat2->size[1] != 0 || mat1->size[0] != target->size[0] ||
      mat1->size[1] != target->size[1])
    return ERROR_INCOMPATIBLE_DIMENSIONS;
  const int height = mat1->size[0];
  const int cols_per_color = mat1->size[1] / mat2->size[1];   // i / num_pix == j / cols_per_color
  const float* v = mat2->data_device;
  return rowcol_map(mat1, target, [=] __device__(float x, int i, int j) { return x + mult * v[i + (size_t)height * (j / cols_per_color)]; });
}

int normalize_by_axis(cudamat* mat, cudamat* target, int axis) {
  if (!mat->on_device || !target->on_device) return ERROR_NOT_ON_DEVICE;
  if (mat->is_trans) return ERROR_TRANSPOSED;
  if (target->size[0] != mat->size[0] || target->size[1] != mat->size[1]) return ERROR_INCOMPATIBLE_DIMENSIONS;
  if (axis != 0) return ERROR_UNSUPPORTED;   // as eigenmat.cc:999-1002
  if (numel(mat) == 0) return 0;
  hipLaunchKernelGGL(center_columns_kernel, dim3(mat->size[1]), dim3(256), 0, stream(), mat->data_device, target->data_device, mat->size[0]);
  return hipGetLastError() == hipSuccess ? 0 : CUDA_ERROR;
}

}  // extern "C"
