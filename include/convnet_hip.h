/* convnet_hip.h — C ABI of libconvnet_hip.so: the MI355X (gfx950) implementation of
 * TorontoDeepLearning/convnet's data-parallel training hot path.
 *
 * This is the reference's "seam #2" (SURVEY.md §8b): the extern "C" cudamat interface that
 * src/matrix.cc and the cudamat ctypes modules bind.  Every entry point below keeps the reference's symbol name,
 * argument order, argument meaning and error convention, so a build of the reference that links
 * this library instead of libcudamat.so + libcudamat_conv_gemm.so needs no source change in
 * the reference's edge / layer / optimizer.cc / convnet.cc.  Each declaration
 * cites the reference interface it replaces.
 *
 * Plain C: pointers, ints, floats.  No torch / HIP types cross this boundary (hipStream_t is passed
 * as void*).  All matrices are column-major fp32; activations are (num_images, X*Y*C) with the
 * image index fastest ("CHWN"), filters (F, Kx*Ky*C)            — cudamat_conv_gemm.cuh:5-10.
 * ConvDesc.padding_* hold the NEGATED pbtxt padding               — src/edge.cc:97-99.
 *
 * Error convention (cudamat.cuh:3-11): functions returning int give 0 or a negative ERROR_* code;
 * the conv/pool/norm functions return void and abort the process on inconsistent shapes, as the
 * reference does (cudamat_conv_gemm.cu:35-42,586-610).
 */
#ifndef CONVNET_HIP_H_
#define CONVNET_HIP_H_

#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ERROR_INCOMPATIBLE_DIMENSIONS -1
#define CUBLAS_ERROR -2   /* kept for numbering; never returned (no BLAS library is used) */
#define CUDA_ERROR -3     /* any HIP runtime failure */
#define VIEW_ERROR -4
#define ERROR_TRANSPOSED -5
#define ERROR_GENERIC -6
#define ERROR_TRANSPOSEDNESS -7
#define ERROR_NOT_ON_DEVICE -8
#define ERROR_UNSUPPORTED -9

/* Bit-identical to `struct cudamat` (cudamat/cudamat.cuh:28-37; ctypes mirror cudamat.py:127-135).
 * `tex_obj` was a cudaTextureObject_t (64-bit); it is kept as an opaque 64-bit slot. */
typedef struct cudamat {
  float* data_host;
  float* data_device;
  int on_device;
  int on_host;
  int size[2];      /* size[0] = rows = leading dimension */
  int is_trans;     /* 0 or 1; honoured by dot() only */
  int owns_data;
  unsigned long long tex_obj;
} cudamat;
typedef cudamat hipmat;

/* cudamat/cudamat.cuh:86-107 (== eigenmat/common.h:4-27) */
typedef struct Shape4D {
  int shape[4];     /* {num_images, size_x, size_y, channels} — src/layer.cc:257-258 */
} Shape4D;

typedef struct ConvDesc {
  int num_input_channels;
  int num_output_channels;
  int kernel_size_y;
  int kernel_size_x;
  int kernel_size_t;
  int stride_y;
  int stride_x;
  int stride_t;
  int padding_y;
  int padding_x;
  int padding_t;
  int input_channel_begin;
  int input_channel_end;
  int output_channel_begin;
  int output_channel_end;
  int num_groups;
} ConvDesc;

/* ---- library state (new; the reference used the legacy default stream + per-call cudaMalloc) ---
 * All work is enqueued on ONE current stream per host thread-less global (the reference is not
 * thread-safe either).  Scratch (split-K partials, dgrad filter images) comes from a
 * library-owned arena that only grows; nothing in the ABI passes a workspace.
 * ONE DEVICE PER PROCESS (the reference's model: one process per GPU, src/convnet_cpu.cc / src/convnet.cc:407-450 over MPI ranks).  The
 * zero page, the scratch arenas, the launch settings cached per kernel (hipFuncSetAttribute, occupancy, CU count) and the wide kernels'
 * slot counts are process-wide and belong to the device that was current at the first call; cuda_set_device to ANOTHER device after
 * work has been issued is not supported (the tables that ARE keyed by device — the generic-k table, the exchange's stream and events —
 * do not change that). */
int convnet_hip_init(int device_id);                 /* cuda_set_device + cublas_init (cudamat.cuh:93-96) */
void convnet_hip_shutdown(void);                     /* cublas_shutdown */
void convnet_hip_set_stream(void* hip_stream);       /* hipStream_t; NULL = default stream */
void* convnet_hip_get_stream(void);
int convnet_hip_reserve_workspace(size_t bytes);     /* optional pre-size (avoids growth mid-run) */
const char* convnet_hip_version(void);
/* How the GEMM-shaped kernels (conv fprop / dgrad / wgrad, dot) form their fp32 products.  Operands, accumulation and results
 * are fp32 either way.
 *   0 (the library's default): v_mfma_f32_32x32x2_f32 — exact fp32 products, IEEE behaviour for inf / NaN / huge operands, what a
 *     host that links this library in place of cudamat + cublasSgemm (cudamat.cu:2130-2152) gets unless it asks otherwise.
 *   1 (what bench.py, the Python trainer and the tests select explicitly — 1.45x the training throughput): on the bf16 matrix pipe
 *     from EXACT three-way splits x = h + m + l (each term a bf16), six of the nine cross
 *     products per operand pair (hh, hm, mh, hl, lh, mm; the dropped ml, lm, ll are <= 2^-23 of a product), fp32 accumulate in
 *     v_mfma_f32_32x32x16_bf16.  Error against double, measured on the product kernels at the exact conv2 / conv4 / fc6 shapes
 *     (tests/test_split_arithmetic_gpu.py, profiles/r03_split_arithmetic.txt; unit 2^-24 of sum|ab|): N(0,1) data 4.2-4.7 vs
 *     4.4-6.1 for path 0 — accumulation rounding dominates both; terms 2^40 apart inside one dot product 14-19 vs 11-14; terms that
 *     cancel in pairs to 2^-12 (only exact products survive) 0.11 vs 0.05.
 *     Where path 1 is NOT plain fp32 arithmetic (a split product cannot be: inf * w = inf*w_h + inf*w_m is inf - inf or inf * 0
 *     whenever the weight's second term has the other sign or is zero):
 *       - an ACTIVATION / DERIVATIVE operand with |x| > 3.396e38 (0x7F7F7FFF; the top 0.2 % of the fp32 range, and +-inf) makes
 *         the outputs it touches NaN (its first split term is a bf16 inf, the residual inf - inf) where path 0 gives +-inf or a
 *         huge finite number.  NaN operands behave as on path 0.
 *       - a conv FILTER operand (pre-split outside the loops, filter_planes_rt_kernel) above that range (or +-inf) saturates to
 *         +-3.3895e38 (bf16 max); an FC weight or a weight-gradient operand (split inside the loops) gives NaN like an activation.
 *       - operands below ~2^-110 in magnitude: their second / third split terms are denormals, which the matrix pipe flushes;
 *         the product then carries 8-16 instead of 24 significant bits (measured <= 2^-20 of sum|ab| at |x| ~ 2^-116 on the conv2 /
 *         conv4 samples; up to 2^-18.2, 12 x path 0, over every output of the per-build rows, profiles/split_error_builds.txt).
 *     Per build (tests/split_cases.py: every split kernel family, epilogue, tail-split and split-K launch): within the shared bounds
 *     on N(0,1), wide-range and huge data except where the two paths run different launches (k order, split-K / tail plan): the
 *     ratio of their maxima reaches 1.3 x, 2.1-2.4 x on conv3-type dgrad where path 0 splits the reduction.  Pairwise cancellation
 *     along taps (C = 3), on reductions of K < 1000 and in the local kernels costs both paths up to 0.96 units (path 0) and 0.93 (path 1).
 * Initial value: environment CONVNET_GG_SPLIT (0/1), else 0.  May be changed between calls at any time. */
void convnet_hip_set_matrix_path(int path);
int convnet_hip_get_matrix_path(void);
/* Which gather-GEMM kernel runs conv fprop / dgrad of the 3x3 / 5x5 layers on matrix path 1 (N % 64 == 0, 16-channel blocks; same
 * arithmetic, same results to rounding — a schedule choice, for A/B runs and tests):
 *   0: ggp_kernel — one output pixel x 256 images per block, every tap a fresh fetch of the source;
 *   1: gpp_kernel, raw  — 4 neighbouring pixels x 64 images per block; the source pixels of a whole tap row staged once, as fp32;
 *   2: gpp_kernel, planes — the same tile reading the source from bf16 planes written by one extra pass (act_planes_kernel);
 *   3: gpw_kernel — 8 neighbouring pixels x 64 images x 128 rows per block, raw fp32 source, the block's four waves stage for
 *      themselves: 3x3 stride-1 gathers with output rows >= 8 pixels whose blocks fill their rounds on the chip (its launch policy,
 *      patch_gemm.hip: wide_plan); every other shape runs as in mode 0.  The default since round 5 (first run on the MI355X there:
 *      parity green, conv3 fprop / conv4 / conv5 7-12 % faster than mode 0).
 *   4: as 3 without the launch policy — gpw_kernel wherever the shape allows (the parity tests' small geometries, A/B runs).
 * Initial value: environment CONVNET_GG_PATCH, else 3. */
void convnet_hip_set_patch_mode(int mode);
int convnet_hip_get_patch_mode(void);
/* Which kernel runs the weight gradients (conv wgrad, FC wgrad) on matrix path 1 — a schedule choice like the one above:
 *   0: wg_kernel — 128 x 128 tile, four waves of 64 x 64, two blocks per CU;
 *   1: wgw_kernel — 256 x 256 (or 256 x 192) tile, four waves of 128 x 128, one block per CU: conv weight gradients with N % 32 == 0,
 *      K >= 256, F >= 192 and >= 64 chunks of reduction; other shapes (conv1, the FC layers) stay on wg_kernel.  The default since
 *      round 5 (first run on the MI355X there: parity green, conv2-5 weight gradients 24-29 % faster).
 * Initial value: environment CONVNET_WG_TILE, else 1. */
void convnet_hip_set_wgrad_tile(int mode);
int convnet_hip_get_wgrad_tile(void);
/* Deferred epilogues, for hosts that issue the reference's UNFUSED call sequence (the reference's own src/*.cc): with the switch on,
 * convUp / convUpGemm, convDown / convDownGemm, MaxPoolUndo / MaxPoolUndoGemm and ResponseNormCrossMap(Gemm) are parked — one call
 * deep — instead of launched, and the element-wise pass the reference issues right behind them on the same matrix is absorbed into the
 * parked call's fused epilogue: add_row_vec of the shared bias and lower_bound_scalar(.., 0, ..) behind a convolution
 * (src/conv_edge.cc:145-148, src/layer.cc:549-551), lower_bound_scalar behind a response normalisation, apply_rectified_linear_deriv
 * behind convDown or MaxPoolUndo (src/layer.cc:556-558).  ANY other library call launches the parked one first, so results are those
 * of the eager sequence (bit for bit on finite data: the fused epilogues add, clamp and mask in the same order; a masked-out
 * derivative is +0 where the eager pass gives 0 * d).  Initial value: environment CONVNET_DEFER_EPILOGUES, else 0. */
void convnet_hip_set_deferred_epilogues(int on);
int convnet_hip_get_deferred_epilogues(void);
long convnet_hip_deferred_absorbed(void);              /* element-wise calls absorbed into a parked call since the library was loaded */
const char* get_last_cuda_error(void);               /* cudamat.cuh:109 */
int cuda_set_device(int deviceId);                   /* cudamat.cuh:116 */
void cuda_sync_threads(void);                        /* cudamat.cuh:123 — synchronises the current stream */
/* Event trio the reference's Matrix::SetReady / WaitTillReady use for cross-stream ordering (cudamat.cuh:110-112,
 * cudamat.cu:70-91).  `t` points at a hipEvent_t (an opaque pointer, spelled void* here so this header needs no HIP
 * include).  record: on the library's current stream; synchronize: the CURRENT STREAM waits (hipStreamWaitEvent), the
 * host does not block — exactly the reference's behaviour.  Return 0 on success, non-zero on failure. */
int cuda_create_event(void** t);
int cuda_record_event(void** t);
int cuda_synchronize_event(void** t);
int cublas_init(void);                               /* cudamat.cuh:93 — no BLAS handle here: returns 0 */
int cublas_shutdown(void);                           /* cudamat.cuh:94 — frees the scratch arenas */
int destroy_tex(cudamat* mat);                       /* cudamat.cuh:127 — called by the reference's Matrix destructor; no textures here */

/* ---- memory / views (cudamat.cuh:124-153) -------------------------------------------------------- */
int allocate_device_memory(cudamat* mat);
int free_device_memory(cudamat* mat);
int copy_to_host(cudamat* mat);
int copy_to_device(cudamat* mat);
int copy_to_host_slice(cudamat* mat, size_t start, size_t end);     /* column range */
int copy_to_device_slice(cudamat* mat, size_t start, size_t end);
int copy_on_device(cudamat* mat1, cudamat* mat2);                   /* mat2 = mat1 */
int copy_transpose(cudamat* source, cudamat* target);
int reshape(cudamat* mat, int m, int n);                            /* -1 allowed for one dim */
int get_slice(cudamat* source, cudamat* target, unsigned int first_col, unsigned int last_col);
void init_from_array(cudamat* mat, float* data, int m, int n);
int init_empty(cudamat* mat, int m, int n);
int write_at(cudamat* mat, int row, int col, float val);
float read_from(cudamat* mat, int row, int col, int* err_code);

/* ---- GPU-side input staging: the DataHandler step right before the hot path (datahandler.cc:146-198,496-532) --------
 * The dataset chunk lives on the GPU as (dims, cases): one case per COLUMN, [colour][row][col] contiguous. */
/* random crop + horizontal flip + transpose into the (cases, colours*ph*pw) CHWN batch (cudamat.cuh:265, cudamat.cu:2699);
 * width_offset / height_offset / flip hold one float per case (flip > 0.5 mirrors the source column). */
int extract_patches(cudamat* images, cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip,
                    int img_width, int img_height, int patch_width, int patch_height);
/* The same staging from a chunk kept in its stored type: `chunk` is dims x num_cases unsigned bytes on the device, one case per
 * column as above.  case_index holds one float per batch case: the chunk column that case comes from (exact up to 2^24 columns; a
 * wider chunk is ERROR_UNSUPPORTED).  Per element v = (float)byte, then — mean / std are (dims, 1), or both NULL — v = (v - mean[s]) /
 * std[s] with s the SOURCE pixel: bit for bit what add_col_mult(-1), div_by_col_vec and extract_patches leave on the float cast of
 * the chunk.  width_offset / height_offset / flip as in extract_patches, or all three NULL for no jitter (the patch is then the whole
 * image).  The case index and the source row and column are clamped into range on the device. */
int stage_patches_u8(void* chunk, int dims, int num_cases, cudamat* case_index, cudamat* mean, cudamat* std, cudamat* patches,
                     cudamat* width_offset, cudamat* height_offset, cudamat* flip, int img_width, int img_height, int patch_width,
                     int patch_height);
/* Dataset statistics from the same byte chunk (apps/compute_mean.cc:70-80; csrc/dataset_moments.hip): the raw integer moments of
 * columns first_case ... first_case + cases - 1, ADDED into acc, which is 2 * dims + num_colors^2 unsigned 64-bit integers on the
 * device (8-byte aligned) and is never cleared here:
 *   acc[d]                    += sum over the cases of x[d]
 *   acc[dims + d]             += sum over the cases of x[d]^2
 *   acc[2 * dims + c * C + c'] += sum over the cases and the pixels p of x[c, p] * x[c', p]      (C = num_colors, the full symmetric block)
 * One read of the range, no workspace.  Every sum is an integer, so the result does not depend on how the cases are split over blocks:
 * bit for bit numpy's int64 sums, from call to call.  The range's start need not be aligned.  num_colors 1 ... 4 are served.
 * ERROR_GENERIC for a NULL chunk or acc (or an acc that is not 8-byte aligned); ERROR_INCOMPATIBLE_DIMENSIONS for dims or num_colors
 * < 1, dims % num_colors != 0, cases < 0 or a range outside [0, num_cases); then ERROR_UNSUPPORTED for num_colors > 4.  cases == 0
 * succeeds and touches nothing. */
int chunk_moments_u8(void* chunk, int dims, int num_cases, int first_case, int cases, int num_colors, void* acc);
/* Clips out of a byte buffer that holds every frame ONCE: `frames` is frame_dims x num_frames unsigned bytes on the device, one frame per
 * column, [colour][row][col].  first_frame holds one float per batch case: the column of the clip's first frame (exact up to 2^24
 * columns; more is ERROR_UNSUPPORTED).  patches is (cases, clip_frames * colours * ph * pw): plane t * colours + c of case n is colour c
 * of frame column min(max((int)first_frame[n], 0) + t, num_frames - 1) — time outermost, the layout of a layer with image_size_t > 1.
 * Per element the arithmetic is stage_patches_u8's with s the source pixel INSIDE the frame (mean / std are (frame_dims, 1), or both
 * NULL): bit for bit what add_col_mult(-1), div_by_col_vec and extract_patches leave on the float cast of the materialised clips with
 * mean / std tiled clip_frames times.  Offsets / flip: one value per case (the whole clip shares its crop), or all three NULL.  The
 * frame column and the source row and column are clamped on the device; shape errors return stage_patches_u8's codes. */
int stage_clips_u8(void* frames, int frame_dims, int num_frames, cudamat* first_frame, int clip_frames, cudamat* mean, cudamat* std,
                   cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip, int img_width, int img_height,
                   int patch_width, int patch_height);
/* stage_clips_u8's grid, for A/B timing (tools/clips_bench.py); the results are the same.  0: the library's choice; 1: a block stages
 * all clip_frames planes of its (colour, patch row, tile) with mean / std in registers; 2: one plane per block. */
void convnet_hip_set_stage_clips_grid(int mode);
/* The same staging out of decoded image files kept at their ORIGINAL sizes, resized on the way (src/image_iterators.cc:22-30,143-187:
 * Resize, GetCoordinates, crop, mirror; the resized image is never stored).  All buffers are plain device pointers:
 *   bytes        num_bytes unsigned bytes: the images back to back, each h rows of w interleaved R, G, B pixels.
 *   image_table  num_images rows of 6 signed 64-bit values {byte offset, w, h, new_w, new_h, first_tap} (8-byte aligned).
 *   taps         num_taps rows of 3 signed 32-bit values {source index, coefficient 0, coefficient 1}: image i owns rows first_tap ...
 *                first_tap + new_w - 1 (one per column of the resized image) and the next new_h (one per row of it).
 *   case_table   one row of 4 signed 32-bit values per case of patches: {image, left, top, mirrored (0 / 1)}.
 * patches is (cases, 3 * ph * pw), planar R, G, B in the layer's layout.  For case n the crop of img_height x img_width pixels is:
 * crop column c is resized column left + (mirrored ? img_width - 1 - c : c), crop row r is resized row top + r.  On that crop the
 * semantics are exactly stage_patches_u8's: v = (float)byte, then (v - mean[s]) / std[s] with s the pixel of the CROP (mean / std are
 * (3 * img_height * img_width, 1), or both NULL); width_offset / height_offset / flip pick the patch inside the crop as in
 * extract_patches, or all three NULL (the patch is then the whole crop).  Bit for bit what add_col_mult(-1), div_by_col_vec and
 * extract_patches leave on the float cast of the crops.
 * One byte of the resized image, integers only (arithmetic shifts): with the column's taps (sx, a0, a1), the row's (sy, b0, b1) and
 * p(y, x) the source byte of that colour, x + 1 and y + 1 clamped to the last index,
 *   h(y)   = ((((2048 * ((p(y, sx) * a0 + p(y, sx + 1) * a1) >> 4)) >> 16) + 2) >> 2            the width pass, rounded to a byte
 *   result = ((((b0 * ((2048 * h(sy)) >> 4)) >> 16) + ((b1 * ((2048 * h(sy + 1)) >> 4)) >> 16) + 2) >> 2
 * — two 8-bit bilinear resizes, first the width at the old height, then the height.  A pass that keeps its size has taps (i, 2048, 0)
 * and is the identity.  The taps are the caller's (convnet_amd/image_iterators.py: Taps builds them in the exact float sequence).
 * Every index read from a table is clamped on the device: the image into [0, num_images), tap rows into [0, num_taps), source
 * indices into [0, w - 1] / [0, h - 1], the byte address below num_bytes, w / h / new_w / new_h to at least 1: a wrong table gives
 * wrong pixels, never a read outside bytes / image_table / taps.
 * ERROR_GENERIC for a NULL bytes / image_table / taps / case_table / patches; ERROR_INCOMPATIBLE_DIMENSIONS for num_bytes == 0,
 * num_taps or num_images < 1 and for every shape mismatch stage_patches_u8 reports (patches not (cases, 3 * ph * pw), mean / std not
 * (3 * H * W, 1) or only one of them, offsets not one per case or not all three, a patch larger than the crop, no jitter but patch !=
 * crop); ERROR_UNSUPPORTED for more than 2^24 images.  Nothing is launched on an error.  One launch per call, no atomics, no
 * workspace. */
int stage_images_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                    cudamat* mean, cudamat* std, cudamat* patches, cudamat* width_offset, cudamat* height_offset, cudamat* flip,
                    int img_width, int img_height, int patch_width, int patch_height);
/* stage_images_u8 for a jitter_raw_image stream (src/image_iterators.cc:189-202, 231-285: per file a random translated crop, a zoom and
 * a rotation of the decoded image, drawn anew for every chunk; convnet_amd/image_iterators.py: Transform).  The arguments, the case
 * table, the cast, mean / std, the patch offsets, the output and the error codes are stage_images_u8's; what differs is the image:
 *   image_table  num_images rows of 11 signed 64-bit values
 *                {byte offset, w, h, new_w, new_h, first_tap, row stride, rotated (0 / 1), first rotation row, win_w, win_h}:
 *                the image is a VIEW of its file — the w x h region Transform crops, whose pixel (y, x) of colour k is the byte at
 *                byte offset + y * row stride + 3 * x + k — resized to new_w x new_h by the two-pass definition above (x + 1 and y + 1
 *                clamped to the VIEW's last index, not the file's) with the new_w column taps and new_h row taps from first_tap on.
 *                rotated 0: that resized view is the image the case table's {left, top, mirrored} refer to (win_w / win_h are not
 *                read).  rotated 1: the resized view R is rotated and the case table refers to a window of win_w x win_h pixels cut
 *                from the rotated image.
 *   taps         also holds, for a rotated image, win_w + win_h rotation rows of 3 signed 32-bit values from `first rotation row` on:
 *                {adelta, bdelta, unused} of every window column, then {X0, Y0, unused} of every window row.
 *   rotated      0 promises that no row of image_table is rotated: the launch takes the arm without the blend, which reads every image
 *                as unrotated.
 * The rotation, pinned to this text and not to an OpenCV build (it is modelled on the INTER_LINEAR fixed-point warpAffine: coordinates
 * with 10 fractional bits reduced to 5, constant border 0).  Host side, in double, for new_w x new_h = RX x RY and an angle in degrees:
 *   a = cos(angle * (pi / 180)), b = sin(angle * (pi / 180)), cx = RX / 2, cy = RY / 2 (integer halves)
 *   M  = [a, b, (1 - a) * cx - b * cy;  -b, a, b * cx + (1 - a) * cy]                      the forward matrix
 *   D  = 1 / (M0 * M4 - M1 * M3);  M0' = M4 * D, M4' = M0 * D, M1' = -M1 * D, M3' = -M3 * D
 *   M2' = -M0' * M2 - M1' * M5,  M5' = -M3' * M2 - M4' * M5                                its inverse
 *   adelta[x] = rint(M0' * x * 1024), bdelta[x] = rint(M3' * x * 1024)                     rint rounds half to even
 *   X0[y] = rint((M1' * y + M2') * 1024) + 16,  Y0[y] = rint((M4' * y + M5') * 1024) + 16
 * The window is cut at (ox, oy) = (RX / 2 - win_w / 2, RY / 2 - win_h / 2): window column c has the rotation row of x = ox + c, window
 * row r that of y = oy + r.  Per pixel of the window, integers only, arithmetic shifts:
 *   X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;  sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31
 *   out = ((32 - fx) * (32 - fy) * R(sy, sx) + fx * (32 - fy) * R(sy, sx + 1) + (32 - fx) * fy * R(sy + 1, sx)
 *          + fx * fy * R(sy + 1, sx + 1) + 512) >> 10,        R(., .) = 0 outside [0, RY) x [0, RX)
 * (the weights are the warp's 15-bit table entries / 32: at steps of 1/32 they are exact and sum to 32 768, so there is no table and
 * no fix-up).  A turn by 90 degrees of an odd square is np.rot90 of it, by -90 np.rot90(., -1), by 180 both flips, bit for bit.
 * Every index read from a table is clamped on the device: the image, tap rows and rotation rows into [0, num_taps), source indices into
 * the view, the byte address below num_bytes, all sizes to 1 ... 2^30, the row stride to 0 ... 2^32, the window's column and row into
 * the window, X and Y into +-2^30: a wrong table gives wrong pixels, never a read outside bytes / image_table / taps.  One launch per
 * call, no atomics, no workspace; nothing is launched on an error. */
int stage_images_jitter_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                           int rotated, cudamat* mean, cudamat* std, cudamat* patches, cudamat* width_offset, cudamat* height_offset,
                           cudamat* flip, int img_width, int img_height, int patch_width, int patch_height);
/* The crops of the same decoded image files as STORED BYTES (apps/image2hdf5.cc; convnet_amd/image2hdf5.py).  bytes / num_bytes,
 * image_table / num_images, taps / num_taps and case_table are stage_images_u8's, with the same meaning; case_table has num_cases rows.
 * rows is a plain device pointer to num_cases * 3 * img_height * img_width unsigned bytes: case n owns bytes n * 3 * H * W ..., planar
 * R, G, B, row-major inside a plane — the row RawImageFileIterator::GetNext leaves in its buffer, a row of dataset `data`, and a column
 * of the dims x num_cases byte chunk stage_patches_u8 and chunk_moments_u8 take.  Each byte is the resized-image byte of the
 * definition above (h(y), then result; integers only): crop column c is resized column left + (mirrored ? img_width - 1 - c : c),
 * crop row r is resized row top + r.  No cast, no mean / std, no patch offsets.  Every index read from a table is clamped on the
 * device exactly as in stage_images_u8 (the image number, the tap rows, the source indices, the byte address, sizes >= 1): a wrong
 * table gives wrong pixels, never a read outside bytes / image_table / taps or a write outside rows.  rows needs no alignment: a colour
 * of four adjacent columns is stored as one dword where its address is 4-byte aligned and as single bytes elsewhere.
 * ERROR_GENERIC for a NULL pointer; ERROR_INCOMPATIBLE_DIMENSIONS for num_bytes == 0 or any of num_taps, num_images, num_cases,
 * img_height, img_width below 1; ERROR_UNSUPPORTED for more than 2^24 images (or a grid beyond 2^31 - 1 blocks).  Nothing is launched
 * on an error.  One launch per call, no atomics, no workspace. */
int crop_images_u8(void* bytes, size_t num_bytes, void* image_table, int num_images, void* taps, int num_taps, void* case_table,
                   int num_cases, void* rows, int img_width, int img_height);
/* The frames of a video as STORED BYTES (apps/video2hdf5.cc over RawVideoFileIterator, src/video_iterators.cc:150-165;
 * convnet_amd/video2hdf5.py): num_frames frames of ONE geometry, each stretched to new_height x new_width — resizeOCV applied
 * unconditionally, no aspect ratio kept, no crop.  All buffers are plain device pointers:
 *   bytes  num_bytes unsigned bytes: the frames back to back, each `height` rows of `width` interleaved R, G, B pixels.  No alignment
 *          is asked for (width * height * 3 need not be a multiple of 4): wide loads are used where an address allows them.
 *   taps   new_width + new_height rows of 3 signed 32-bit values {source index, coefficient 0, coefficient 1}: the column taps, then
 *          the row taps — ImageTaps(width, height, new_width, new_height) concatenated, stage_images_u8's layout for one image.
 *   rows   num_frames * 3 * new_height * new_width unsigned bytes: frame n owns bytes n * 3 * H * W ..., planar R, G, B, row-major in
 *          a plane — a row of dataset `data`.  No alignment is asked for: a colour of four adjacent columns is stored as one dword
 *          where its address is 4-byte aligned and as single bytes elsewhere, as in crop_images_u8.
 * Each byte is the resized-image byte of the definition above (h(y), then result; integers only, h(y) kept as a byte), of resized
 * column (mirrored ? new_width - 1 - c : c) for output column c.  Source indices read from taps are clamped on the device into
 * [0, width - 1] and [0, height - 1], every store lies inside rows by construction and the host check below keeps every load inside
 * bytes: a wrong tap table gives wrong pixels, never an access outside the buffers.
 * ERROR_GENERIC for a NULL pointer; ERROR_INCOMPATIBLE_DIMENSIONS for any of num_frames, width, height, new_width, new_height below 1
 * or num_bytes < num_frames * width * height * 3 (computed in size_t); ERROR_UNSUPPORTED for a grid beyond 2^31 - 1 blocks (or a
 * source row of more than 2^31 - 1 bytes).  Nothing is launched on an error.  One launch per call, no atomics, no workspace. */
int resize_frames_u8(void* bytes, size_t num_bytes, int num_frames, int width, int height, void* taps, int new_width, int new_height,
                     int mirrored, void* rows);
/* ---- feature extraction: src/datawriter.cc (DataWriter::Write / WriteHDF5SeqBuf; csrc/feature_rows.hip) -------------------------
 * A layer state becomes rows of a feature file's dataset, averaged on the way.  state is (N, D), case fastest; sum has its shape (NULL
 * is fine when passes == 1); rows is (D, R): R rows of D contiguous floats; carry is (D, 1) (NULL is fine when group == 1).
 *   pass < passes - 1: sum = state (pass == 0; as 0 + state) or sum + state.  Nothing else is touched.
 *   last pass        : v = state (passes == 1) or (sum + state) / passes — bit for bit add_elementwise into a zeroed buffer `passes`
 *                      times, then divide_by_scalar (buf.Add(m) ...; buf.Divide(average_batches)).  sum is not written.
 *     group == 1     : rows[:, n] = v[n, :] for n < cases: an exact transpose; later columns of rows and carry are untouched.
 *     group  > 1     : the `cases` columns of v are consumed in order into groups of `group` consecutive cases; the open group already
 *                      holds `consumed` (< group) cases in carry.  Every completed group writes the next column of rows (from 0): the
 *                      carry, then fma(member, 1 / group, .) member by member in case order — (consumed + cases) / group columns.  On
 *                      return carry holds the partial of the still-open group, or zeros.  No atomics: the same bits from call to call.
 * ERROR_GENERIC for a NULL or out-of-range argument, ERROR_TRANSPOSED for a transposed operand, ERROR_INCOMPATIBLE_DIMENSIONS when sum
 * differs from state, rows has not D rows or fewer columns than are written, carry is not (D, 1) or cases > N.  get_slice views are
 * fine: 16-byte loads along N need N % 4 == 0 and 16-byte bases of state and sum, 16-byte stores along D need D % 4 == 0 and a 16-byte
 * base of rows; otherwise that side runs scalar.  One launch per call, no workspace. */
int feature_rows(cudamat* state, cudamat* sum, int pass, int passes, int cases, cudamat* carry, int consumed, int group, cudamat* rows);
/* in place: for every column pair (2j, 2j+1) swap columns idx[2j] and idx[2j+1] (cudamat.cu:2655, kShuffleColumns) */
int shuffleColumns(cudamat* source, cudamat* rand_perm_indices);
int add_col_vec(cudamat* mat, cudamat* vec, cudamat* target);                 /* cudamat.cuh:165 */
int add_col_mult(cudamat* mat, cudamat* vec, cudamat* target, float mult);    /* mean subtraction: mult = -1 */
int div_by_col_vec(cudamat* mat, cudamat* vec, cudamat* target);              /* cudamat.cuh:176: divide by std */
int mult_by_row_vec(cudamat* mat, cudamat* vec, cudamat* target);
int div_by_row_vec(cudamat* mat, cudamat* vec, cudamat* target);
int add_to_each_pixel(cudamat* mat1, cudamat* mat2, cudamat* target, float mult);   /* PCA colour noise */
int normalize_by_axis(cudamat* mat, cudamat* target, int axis);               /* axis 0: subtract each column's mean */

/* ---- convolution: cudamat/cudamat_conv_gemm.cuh:36-49 ----------------------------------------------
 * targets = scaleTargets*targets + conv(...).  scaleTargets is the reference's 0/1 accumulate flag but
 * any value is honoured.  Implemented as implicit-GEMM on fp32 MFMA (no im2col buffer).
 * Restrictions, the reference's own: num_groups == 1 (cudamat_conv_gemm.cu:599-600 asserts the same and the host
 * never passes anything else, src/edge.cc:104), whole channel ranges (input/output_channel_begin/end = 0/0 or
 * 0/channels), kernel_size_t <= 1.  These entries are void in the reference's ABI, so a violated restriction or a
 * shape mismatch cannot be returned as a code: it prints "check failed: <condition>" with file:line to stderr and
 * aborts, as the reference's assert() does.  The int-returning entries return the reference's error codes instead. */
void convUpGemm(cudamat* images, cudamat* filters, cudamat* targets,
                Shape4D* images_shape, Shape4D* filters_shape,
                Shape4D* targets_shape, ConvDesc conv_desc,
                float scaleTargets);
void convDownGemm(cudamat* derivs, cudamat* filters, cudamat* targets,
                  Shape4D* derivs_shape, Shape4D* filters_shape,
                  Shape4D* targets_shape, ConvDesc conv_desc,
                  float scaleTargets);
void convOutpGemm(cudamat* images, cudamat* derivs, cudamat* targets,
                  Shape4D* images_shape, Shape4D* derivs_shape,
                  Shape4D* targets_shape, ConvDesc conv_desc,
                  float scaleTargets, float scaleOutput);
/* convnet2-style names of the same operations (cudamat/cudamat_conv.cuh:10-29); partialSum* are
 * accepted and ignored (the split-K factor is chosen internally and reduced deterministically). */
void convUp(cudamat* images, cudamat* filters, cudamat* targets,
            Shape4D* images_shape, Shape4D* filters_shape, Shape4D* targets_shape,
            ConvDesc conv_desc, float scaleTargets);
void convDown(cudamat* derivs, cudamat* filters, cudamat* targets,
              Shape4D* derivs_shape, Shape4D* filters_shape, Shape4D* targets_shape,
              ConvDesc conv_desc, float scaleTargets);
void convOutp(cudamat* images, cudamat* derivs, cudamat* targets,
              Shape4D* images_shape, Shape4D* derivs_shape, Shape4D* targets_shape,
              ConvDesc conv_desc, int partialSumY, int partialSumX, float scaleTargets,
              float scaleOutput);

/* ---- locally connected layers: cudamat_conv.cuh:14-33 and cudamat_conv_gemm.cuh:56-69 (src/local_edge.cc; csrc/local_conv.hip) ----
 * A convolution whose every module (output pixel m = my*Mx + mx, M = My*Mx) has its own filter bank.  Layouts as above; the bank is
 * (F, Kx*Ky*C*M) column-major: module m owns the F*K floats (K = Kx*Ky*C) at offset m*F*K, and element (f, c, ky, kx) of that block sits at
 * f + F*(kx + Kx*(ky + Ky*c)) — exactly a conv bank.  Its Shape4D is (F, Kx, Ky, C*My*Mx) (local_edge.cc SetMemory).
 *   localUp:   targets[n, f, m] = scaleTargets*targets + sum_k W_m[f, k] * patch_m[k, n]
 *   localDown: targets = scaleTargets*targets + the adjoint of localUp in the images
 *   localOutp: targets = scaleTargets*targets + scaleOutput * sum_n derivs (x) patch, per module
 * Padding (negated) and strides come from conv_desc; num_groups == 1 and the channel ranges as for convUp; kernel_size_t <= 1.  Shape
 * mismatches abort through the same checks as convUpGemm, with filterModuleMult = M.  Both matrix paths; no atomics: bit-identical from
 * call to call.  The plain and the *Gemm names are the same functions.
 * REFERENCE QUIRK, not reproduced: the reference's _convUpGemm / _convDownGemm / _convOutpGemm with conv == false
 * (cudamat_conv_gemm.cu:657, 800, 944) advance the bank pointer BEFORE the first module's GEMM, so module m uses block m + 1, the last
 * module reads past the bank and its localOutp writes past dW (into the bias gradient that follows it in the edge's slice).  This library
 * implements the definition above, which is also what the reference's non-GEMM localUp (filterActs) computes.
 * localUpBiasAct (new, the analogue of convUpBiasAct): localUp, then bias element j added to output column j (the (F, M) bias slice read
 * as (1, F*M), local_edge.cc ComputeUp: AddRowVec), then max(x, 0) when relu != 0 — bit-identical to localUp + add_row_vec
 * [+ lower_bound_scalar(.., 0, ..)].  bias may be NULL. */
void localUp(cudamat* images, cudamat* filters, cudamat* targets,
             Shape4D* images_shape, Shape4D* filters_shape, Shape4D* targets_shape,
             ConvDesc conv_desc, float scaleTargets);
void localDown(cudamat* derivs, cudamat* filters, cudamat* targets,
               Shape4D* derivs_shape, Shape4D* filters_shape, Shape4D* targets_shape,
               ConvDesc conv_desc, float scaleTargets);
void localOutp(cudamat* images, cudamat* derivs, cudamat* targets,
               Shape4D* images_shape, Shape4D* derivs_shape, Shape4D* targets_shape,
               ConvDesc conv_desc, float scaleTargets, float scaleOutput);
void localUpGemm(cudamat* images, cudamat* filters, cudamat* targets,
                Shape4D* images_shape, Shape4D* filters_shape,
                Shape4D* targets_shape, ConvDesc conv_desc,
                float scaleTargets);
void localDownGemm(cudamat* derivs, cudamat* filters, cudamat* targets,
                  Shape4D* derivs_shape, Shape4D* filters_shape,
                  Shape4D* targets_shape, ConvDesc conv_desc,
                  float scaleTargets);
void localOutpGemm(cudamat* images, cudamat* derivs, cudamat* targets,
                  Shape4D* images_shape, Shape4D* derivs_shape,
                  Shape4D* targets_shape, ConvDesc conv_desc,
                  float scaleTargets, float scaleOutput);
void localUpBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets,
                    Shape4D* images_shape, Shape4D* filters_shape, Shape4D* targets_shape,
                    ConvDesc conv_desc, float scaleTargets, int relu);

/* ---- spatio-temporal (3-D) convolution: cudamat_conv_gemm.cuh:115-138 (cudamat_conv3d_gemm.cu; src/conv_edge.cc:153-245; csrc/conv3d.hip)
 * Time is the OUTERMOST index.  Activations are (N, X*Y*C*T): element (n, x, y, c, t) at n + N*(x + W*(y + H*(c + C*t))), Shape4D
 * (N, X, Y, C*T); frame t is the column range [t*X*Y*C, (t+1)*X*Y*C).  The bank is (F, Kx*Ky*C*Kt): element (f, kx, ky, c, kt) at
 * f + F*(kx + Kx*(ky + Ky*(c + C*kt))), Shape4D (F, Kx, Ky, C*Kt).  C = conv_desc.num_input_channels, F = conv_desc.num_output_channels,
 * T = images_shape[3] / C, Mt = targets_shape[3] / F = (T - Kt) / stride_t + 1.
 *   convUp3DGemm:   output frame m = convUpGemm of input frames [m*stride_t, m*stride_t + Kt) read as C*Kt channels
 *   convDown3DGemm: targets = scaleTargets*targets + sum over m of convDownGemm(derivs frame m) into input frames [m*st, m*st + Kt);
 *                   overlapping windows add; input frames that no window covers become scaleTargets*targets
 *   convOutp3DGemm: targets = scaleTargets*targets + scaleOutput * sum over m of convOutpGemm(input frames of m, derivs frame m)
 *   ResponseNormCrossMap3D[Undo]Gemm: the 2-D operation on each of image_size_t frames
 * Restrictions: padding_t == 0 (the reference asserts it), num_groups == 1, whole channel ranges; a violation or a shape mismatch
 * prints "check failed: ..." and aborts, as for convUpGemm.  kernel_size_t <= 0 and stride_t <= 0 are read as 1.
 * Unlike the reference, which moves data_device and size[1] of the caller's cudamat structs during its loops and restores them, these
 * entries never write the caller's structs.  They are not parked as deferred epilogues.  Both matrix paths; no atomics: bit-identical
 * from call to call.
 * How they run: convUp3DGemm is bit-identical to the loop of convUpGemm over get_slice views; the bank's bf16 planes /
 * tap-major copy are built once per call.  convOutp3DGemm writes dW once: the frames' split-K slabs go to one arena and a single
 * reduction sums them in fixed order and applies scaleTargets / scaleOutput (tolerance-equal to the accumulating loop).  convDown3DGemm, when C % 16 == 0, is a gather over
 * time: each input frame is ONE 2-D dgrad over the contiguous output frames whose windows contain it, with a bank re-laid per frame
 * class, so every input frame is written exactly once (tolerance-equal to the reference's accumulating loop: the summation order
 * differs); for other C it is that loop (one scale pass, then every output frame accumulates into its window).
 * Fused variants (new), each bit-identical to the unfused sequence on every frame:
 *   convUp3DBiasAct : convUp3DGemm + the shared bias (1, F) added to every output frame [+ max(x, 0)]   (conv_edge.cc:155-164)
 *   convDown3DMask  : targets = (state > 0) ? post_scale * (convDown3DGemm result) : 0 — in the gather's epilogue (each frame is
 *                     written once), as a last pass behind the loop
 *   convOutp3DBias  : convOutp3DGemm AND bias_grad(1, F) = scaleTargets*bias_grad + scaleOutput * sum of derivs over images, pixels
 *                     and frames (conv_edge.cc:228-238)
 *   ResponseNormCrossMap3DRelu : ResponseNormCrossMap3DGemm + the ReLU of the destination layer */
void convUp3DGemm(cudamat* images, cudamat* filters, cudamat* targets,
                  Shape4D* images_shape, Shape4D* filters_shape,
                  Shape4D* targets_shape, ConvDesc conv_desc,
                  float scaleTargets);
void convDown3DGemm(cudamat* derivs, cudamat* filters, cudamat* targets,
                    Shape4D* derivs_shape, Shape4D* filters_shape,
                    Shape4D* targets_shape, ConvDesc conv_desc,
                    float scaleTargets);
void convOutp3DGemm(cudamat* images, cudamat* derivs, cudamat* targets,
                    Shape4D* images_shape, Shape4D* derivs_shape,
                    Shape4D* targets_shape, ConvDesc conv_desc,
                    float scaleTargets, float scaleOutput);
void ResponseNormCrossMap3DGemm(cudamat* images, cudamat* targets, int numFilters, int sizeF, float addScale,
                                float powScale, bool blocked, int image_size_t);
void ResponseNormCrossMap3DUndoGemm(cudamat* outGrads, cudamat* inputs, cudamat* targets,
                                    int numFilters, int sizeF, float addScale, float powScale, bool blocked,
                                    int image_size_t);
void convUp3DBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets,
                     Shape4D* images_shape, Shape4D* filters_shape, Shape4D* targets_shape,
                     ConvDesc conv_desc, float scaleTargets, int relu);
void convDown3DMask(cudamat* derivs, cudamat* filters, cudamat* state, cudamat* targets,
                    Shape4D* derivs_shape, Shape4D* filters_shape, Shape4D* targets_shape,
                    ConvDesc conv_desc, float scaleTargets, float post_scale);
void convOutp3DBias(cudamat* images, cudamat* derivs, cudamat* targets, cudamat* bias_grad,
                    Shape4D* images_shape, Shape4D* derivs_shape, Shape4D* targets_shape,
                    ConvDesc conv_desc, float scaleTargets, float scaleOutput);
void ResponseNormCrossMap3DRelu(cudamat* images, cudamat* targets, int numFilters, int sizeF, float addScale,
                                float powScale, bool blocked, int image_size_t);

/* ---- pooling: cudamat_conv_gemm.cuh:72-92 (and cudamat_conv.cuh:58-70) ------------------------------
 * Pooling over time: when images_shape[3] = C*T with C = conv_desc.num_input_channels and T > 1, the tensors hold T frames (layout as
 * for the 3-D convolution) and the windows are Ky x Kx x Kt boxes with stride_t / padding_t, clipped to the clip as they are to the
 * image; output element (n, mx, my, c, mt), Mt = (T - 2*padding_t - Kt) / stride_t + 1.  The average (forward and undo) divides by
 * the CLIPPED box; the max undo routes to every input of a box that equals its maximum and sums over overlapping boxes
 * (cudamat_conv_gemm.cu:163-293).  With T == 1 nothing changes; with T > 1 and Kt <= 1, stride_t <= 1, padding_t == 0 the call is
 * the 2-D one on C*T channels, bit for bit.  MaxPoolMask / MaxPoolUndoMask return ERROR_UNSUPPORTED for windows with a time extent. */
void MaxPoolGemm(cudamat* images, cudamat* targets, Shape4D* images_shape,
                 Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets,
                 float scaleOutput);
void MaxPoolUndoGemm(cudamat* images, cudamat* maxGrads, cudamat* maxActs,
                     cudamat* targets, Shape4D* images_shape,
                     Shape4D* maxGrads_shape, ConvDesc conv_desc,
                     float scaleTargets);
void AvgPoolGemm(cudamat* images, cudamat* targets, Shape4D* images_shape,
                 Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets,
                 float scaleOutput);
void AvgPoolUndoGemm(cudamat* avgGrads, cudamat* targets,
                     Shape4D* avgGrads_shape, Shape4D* targets_shape,
                     ConvDesc conv_desc, float scaleTargets);
void MaxPool(cudamat* images, cudamat* targets, Shape4D* images_shape,
             Shape4D* targets_shape, ConvDesc conv_desc);
void AvgPool(cudamat* images, cudamat* targets, Shape4D* images_shape,
             Shape4D* targets_shape, ConvDesc conv_desc);
void MaxPoolUndo(cudamat* images, cudamat* maxGrads, cudamat* maxActs,
                 cudamat* targets, Shape4D* images_shape, Shape4D* maxGrads_shape,
                 ConvDesc conv_desc, float scaleTargets);
void AvgPoolUndo(cudamat* avgGrads, cudamat* targets, Shape4D* avgGrads_shape,
                 Shape4D* targets_shape, ConvDesc conv_desc, float scaleTargets);

/* ---- resampling and colour transform: cudamat_conv_gemm.cuh:94-97, cudamat_conv.cuh:72-78 (csrc/resample.hip) ---------
 * UpSampleGemm: targets (N, X*f, Y*f, C) from images (N, X, Y, C), f = factor >= 1, the image need not be square:
 *   scaleTargets == 0:  targets[n, c, Y, X] = images[n, c, Y / f, X / f]; the target is not read (NaNs in it do not survive);
 *   otherwise:          targets = scaleTargets * targets + images[...], one multiply and one add, each rounded (scaleTargets == 1: one add).
 *   The replicated value is the input value ITSELF.  The reference forms f*f * x / (f*f) through its average-pool undo
 *   (cudamat_conv_gemm.cu:1503-1541; CPU build: f*f * (x * (1 / (f*f))), src/CPUMatrix.cc:869-899): bit for bit x for power-of-two
 *   factors, within 2^-22 relative of x (three roundings of 2^-24, with slack) for the others.
 * DownSampleGemm: targets (N, X, Y, C) = the mean of each f x f block of images (N, X*f, Y*f, C), overwriting: bit for bit what
 *   AvgPoolGemm leaves for kernel = stride = f, padding 0, scaleTargets 0, scaleOutput 1 on the same operands.
 * RGBToYUV: operands (N, 3 * pixels), colour planes outermost (cudamat_conv_others.cu:296-325, the constants of src/matrix.cc:1013-1028):
 *   Y = fmaf(0.0722f, B, fmaf(0.7152f, G, 0.2126f * R)), U = fmaf(0.436f, B, fmaf(-0.33609f, G, -0.09991f * R)),
 *   V = fmaf(-0.05639f, B, fmaf(-0.55861f, G, 0.615f * R)); targets == images is allowed.
 * A NULL or transposed operand, an operand that is not on the device, factor < 1, targets that are not factor x images on both axes,
 * differing image or channel counts, a matrix that does not have the size of its shape, a column count not divisible by 3: the call
 * leaves a text that begins with the entry's -Gemm name in get_last_cuda_error() and launches nothing.  Views from get_slice are served:
 * the 16-byte arm needs N % 4 == 0 and 16-byte bases (RGBToYUV: N * pixels % 4 == 0), anything else runs the scalar arm.
 * UpSample / DownSample are the same functions, as for the pool entries. */
void UpSampleGemm(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor, float scaleTargets);
void DownSampleGemm(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor);
void UpSample(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor, float scaleTargets);
void DownSample(cudamat* images, cudamat* targets, Shape4D* images_shape, Shape4D* targets_shape, int factor);
void RGBToYUV(cudamat* images, cudamat* targets);

/* ---- cross-map response normalisation: cudamat_conv_gemm.cuh:100-106, cudamat_conv.cuh:35-42 ---------
 * In place: targets == images (forward, also ...Relu) is allowed for numFilters <= 768 only — above that the kernel walks the
 * channels in global memory and subtracts from its window sum channels it has already overwritten: the call prints
 * "check failed: ..." and aborts, as for convUpGemm;
 * targets == outGrads (undo) is allowed for every channel count (outGrads has been consumed before the first element is written).
 * targets == inputs is never allowed in the undo. */
void ResponseNormCrossMapGemm(cudamat* images, cudamat* targets, int numFilters, int sizeF,
                              float addScale, float powScale, bool blocked);
void ResponseNormCrossMapUndoGemm(cudamat* outGrads, cudamat* inputs, cudamat* targets,
                                  int numFilters, int sizeF, float addScale, float powScale,
                                  bool blocked);
void ResponseNormCrossMap(cudamat* images, cudamat* targets, int numFilters, int sizeF,
                          float addScale, float powScale, bool blocked);
void ResponseNormCrossMapUndo(cudamat* outGrads, cudamat* inputs, cudamat* acts, cudamat* targets,
                              int numFilters, int sizeF, float addScale, float powScale,
                              bool blocked);

/* ---- dense ops (cudamat.cuh:170-263) ------------------------------------------------------------- */
/* target = beta*target + alpha*op(mat1)*op(mat2), op = transpose iff is_trans (cudamat.cu:2130-2152).
 * fc_edge.cc's three uses (NT fwd, NN dgrad, TN wgrad, alpha on the TN side) run on fp32 MFMA; the remaining cases of the
 * reference's contract (T,T; alpha != 1 with a non-transposed mat1) run on a plain LDS-tiled fp32 kernel. */
int dot(cudamat* mat1, cudamat* mat2, cudamat* target, float beta, float alpha);
float vdot(cudamat* mat1, cudamat* mat2, int* err_code);
int add_row_vec(cudamat* mat, cudamat* vec, cudamat* target);
int add_row_mult(cudamat* mat, cudamat* vec, cudamat* target, float mult);
int sum_by_axis(cudamat* mat, cudamat* target, int axis, float mult, float p);   /* target = p*target + mult*sum */
int sqsum_by_axis(cudamat* mat, cudamat* target, int axis, float mult, float p);
float sum_all(cudamat* mat, int* err_code);
float euclid_norm(cudamat* mat, int* err_code);
int normlimit_by_axis(cudamat* mat, cudamat* target, int axis, float norm, int constraint);
int lower_bound_scalar(cudamat* mat, float val, cudamat* target);
int upper_bound_mod_scalar(cudamat* mat, float val, cudamat* target);
int apply_rectified_linear_deriv(cudamat* mat1, cudamat* mat2, cudamat* target);
int assign_scalar(cudamat* mat, float alpha);
int add_scalar(cudamat* mat, float alpha, cudamat* target);
int mult_by_scalar(cudamat* mat, float alpha, cudamat* target, float scale_targets);
int divide_by_scalar(cudamat* mat, float alpha, cudamat* target);
int add_mult(cudamat* mat1, cudamat* mat2, float alpha);                         /* mat1 += alpha*mat2, product rounded first */
int add_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target);
int subtract_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target);
int mult_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target, float scale_targets);
int apply_sqrt(cudamat* mat, cudamat* target);

/* ---- Adagrad / RMSProp: cudamat.cuh:229,275-276 (src/optimizer.cc:226-231,257-279; csrc/elementwise.hip) --------------------------------
 * The three entries behind AdagradSGDOptimizer and RMSPropSGDOptimizer.  Checks as in cudamat: ERROR_TRANSPOSEDNESS when the operands
 * differ in is_trans, then ERROR_INCOMPATIBLE_DIMENSIONS when they differ in element count; views (slices of a flat buffer) are fine.
 * Every statement is one separately rounded fp32 operation, square root and division the correctly rounded ones.
 *  adagrad : history = delta + sqrt((history - delta)^2 + grad^2)
 *  rms_prop: history = sqrt(factor*history*history + (1 - factor)*grad*grad), left to right, 1 - factor formed in float */
int adagrad(cudamat* history, cudamat* grad, float delta);
int rms_prop(cudamat* history, cudamat* grad, float factor);
int divide_elementwise(cudamat* mat1, cudamat* mat2, cudamat* target);

/* ---- batch normalisation: cudamat.cuh:298-303 (src/matrix.cc:1077-1102; csrc/batch_norm.hip) ------------------------------------
 * Column c of the (h, w) matrices is one channel's contiguous run (Layer::ApplyBatchNormalization reshapes the state to (-1, C)); the
 * vectors are (1, w).  The reference's checks and error codes.  Sums run as per-wave slab partials combined in a fixed order (no
 * atomics): bit-identical from call to call, and tolerance-equal (fp32 summation order) to the reference's 32-thread column loops.
 *  bn_bprop_inplace: dgamma = mean(deriv·act); deriv -= dgamma·act; deriv -= mean(deriv)            (kBNBpropInplace)
 *  bn_bprop        : cs = Σ(x-mu)·d / ((h-1)·sigma²); v = gamma·(d - (x-mu)·cs)/sigma; target = scale_targets·target + v - mean(v)
 *  bn_grad         : dgamma = Σ (x-mu)/sigma · d; dbeta = Σ d  (sums, not means)                          (kBNGrad)
 * Unlike eigenmat's bn_bprop_inplace (eigenmat.cc:2515-2537, which has no return statement), these return 0 on success. */
int bn_bprop_inplace(cudamat* deriv, cudamat* act, cudamat* dgamma);
int bn_bprop(cudamat* deriv, cudamat* input, cudamat* gamma, cudamat* mu, cudamat* sigma, cudamat* target, float scale_targets);
int bn_grad(cudamat* deriv, cudamat* input, cudamat* mu, cudamat* sigma, cudamat* dgamma, cudamat* dbeta);

/* ---- output layer (cudamat.cuh:249-262) ------------------------------------------------------------ */
int softmax_row_major(cudamat* mat, cudamat* target);
int softmax_row_major_multi(cudamat* mat, int numslices, cudamat* target);
int apply_softmax_grad_row_major(cudamat* mat, cudamat* labels, cudamat* target);
int get_softmax_correct_row_major(cudamat* mat, cudamat* labels, cudamat* target);
int get_softmax_cross_entropy_row_major(cudamat* mat, cudamat* labels, cudamat* target, float tiny);

/* ---- logistic and softmax-distribution layers: cudamat.cuh:204,216,233,252,289 (src/layer.cc:579-602, src/loss_functions.cc:55-140) ----
 * Arithmetic of the reference's CPU build (eigenmat.cc:1133-1151,1344-1392,1543-1557,1771-1786), the whole-net parity target.  Checks:
 * ERROR_NOT_ON_DEVICE, then ERROR_TRANSPOSEDNESS when the first two operands differ in is_trans, then ERROR_INCOMPATIBLE_DIMENSIONS
 * unless every operand has the same (rows, cols).  Views are fine (a get_slice that starts 4-byte aligned only runs its first floats
 * scalar, then 16-byte accesses), and so is target == an operand.
 *  apply_sigmoid       : target = 1 / (1 + exp(-mat)): exactly 1 for large x, 0 or a denormal for very negative x (exp overflows to
 *                        inf, 1 / inf = 0: no NaN from overflow), NaN for NaN.
 *  apply_logistic_deriv: target = (mat1 * mat2) * (1 - mat2), mat1 the derivative, mat2 the logistic state; three separately rounded
 *                        fp32 operations.
 *  apply_logistic_grad : out_grad = mat2 < 0 ? 0 : mat1 - mat2, mat1 the probabilities, mat2 the targets; a negative target means
 *                        "don't care".
 *  get_logistic_correct_normalized: out is (rows, 1); out[row] = the share of the row's entries with target >= 0 whose (p >= 0.5)
 *                        agrees with (target >= 0.5); 0 when the row has no entry with target >= 0.  Exact (integer counts).
 *  compute_cross_entropy: target = -mat * log(pow + tiny), mat the target distribution, pow the probabilities.  (eigenmat's second
 *                        size check compares pow with itself; here pow must have mat's size.) */
int apply_sigmoid(cudamat* mat, cudamat* target);
int apply_logistic_deriv(cudamat* mat1, cudamat* mat2, cudamat* target);
int apply_logistic_grad(cudamat* mat1, cudamat* mat2, cudamat* out_grad);
int get_logistic_correct_normalized(cudamat* mat1, cudamat* mat2, cudamat* out);
int compute_cross_entropy(cudamat* mat, cudamat* pow, cudamat* target, float tiny);

/* ---- RNG (cudamat.cuh:117-119,154-164).  The reference's GPU (multiply-with-carry) and CPU
 * (std::default_random_engine) streams already differ from each other; this
 * library uses a counter-based Philox-4x32-10 keyed by (seed, call counter, element index). --------- */
typedef struct rnd_struct {
  unsigned int* dev_mults;          /* unused; layout kept (cudamat.cuh:50-53) */
  unsigned long long* dev_words;    /* points at a host-side {seed, counter} pair owned by the library */
} rnd_struct;
int init_random(rnd_struct* rnd_state, int seed);
int fill_with_rand(rnd_struct* rnd_state, cudamat* mat);
int fill_with_randn(rnd_struct* rnd_state, cudamat* mat);
int sample_bernoulli(rnd_struct* rnd_state, cudamat* mat, cudamat* target);
int dropout(rnd_struct* rnd_state, cudamat* mat, float dropprob, float val, float scale);

/* ---- fused entry points (new; SURVEY.md §7 "offer fused entry points in the ABI") ------------------
 * Same arithmetic as the unfused sequences they replace, fewer passes over HBM.
 *  convUpBiasAct      : convUpGemm + reshape/add_row_vec(shared bias) [+ lower_bound_scalar(0)]
 *                        (src/conv_edge.cc:138-149 + src/layer.cc:549-551)
 *  dotBiasAct         : dot(NT) + add_row_vec [+ ReLU]   (src/fc_edge.cc:51-61)
 *  sgd_momentum_step  : SGDOptimizer::Optimize, non-Nesterov (src/optimizer.cc:174-200) in one pass
 *                        (row-norm constraint excluded: call normlimit_by_axis after).
 *  softmax_ce_grad_correct: softmax + SoftmaxCEDeriv + SoftmaxCorrect accumulation
 *                        (src/layer.cc:570-572, src/loss_functions.cc:81-83,114-120); `correct_accum`
 *                        is a 1x1 device matrix accumulated with atomics-free per-call add, so the
 *                        host can read it every print_after steps instead of every step.
 *  relu_dropout       : lower_bound_scalar(0) then dropout(p, 0, scale) (src/layer.cc:391,549). */
void convUpBiasAct(cudamat* images, cudamat* filters, cudamat* bias, cudamat* targets,
                   Shape4D* images_shape, Shape4D* filters_shape, Shape4D* targets_shape,
                   ConvDesc conv_desc, float scaleTargets, int relu);
int dotBiasAct(cudamat* mat1, cudamat* mat2, cudamat* bias, cudamat* target, float beta, float alpha,
               int relu);
int sgd_momentum_step(cudamat* grad, cudamat* param, cudamat* history, float l2_decay,
                      float gradient_clip, float epsilon, float momentum);
int sgd_momentum_step_normlimit(cudamat* grad, cudamat* param, cudamat* history, float l2_decay,
                                float gradient_clip, float epsilon, float momentum, float norm,
                                int constraint);
/* sgd_momentum_step on `count` tensors in one launch per 16 of them (the arrays hold one entry per tensor): the many small tensors of a
 * step — convolution banks, every bias — otherwise cost a launch each.  Element for element the same update: bit-identical to `count`
 * calls of sgd_momentum_step. */
int sgd_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, const float* l2_decay,
                            const float* gradient_clip, const float* epsilon, const float* momentum);   /* + ApplyConstraints (src/optimizer.cc:75-81), axis=1 */
/* The second-moment optimizers in one pass over gradient, parameter and both histories, bit-identical to the reference's call sequences
 * (and, like sgd_momentum_step, leaving in `grad` what that sequence leaves there):
 *  adagrad_momentum_step: AdagradSGDOptimizer::Optimize (src/optimizer.cc:226-231, then :174-200, non-Nesterov) — adagrad(a, g, delta);
 *                         g /= a; g *= step_scale; g += l2*w; clip; g *= epsilon; h = momentum*h + g; w -= h.  step_scale is the host's
 *                         sqrt(step + 1), rounded to float once.  Replaces 9 passes.
 *  rmsprop_momentum_step: RMSPropSGDOptimizer::Optimize (:257-279) — h *= momentum; g += l2*w; clip; rms_prop(a, g, factor); g /= a;
 *                         h += epsilon*g; w -= h.
 * The *_multi forms are the same steps on `count` tensors in one launch per 16 of them, like sgd_momentum_step_multi: bit-identical to
 * `count` single calls.  ERROR_INCOMPATIBLE_DIMENSIONS on differing element counts, ERROR_UNSUPPORTED above INT_MAX (2^31 - 1) floats. */
int adagrad_momentum_step(cudamat* grad, cudamat* param, cudamat* history, cudamat* adagrad_history, float delta, float step_scale,
                          float l2_decay, float gradient_clip, float epsilon, float momentum);
int rmsprop_momentum_step(cudamat* grad, cudamat* param, cudamat* history, cudamat* rms_history, float factor, float l2_decay,
                          float gradient_clip, float epsilon, float momentum);
int adagrad_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, cudamat** adagrad_histories,
                                const float* delta, const float* step_scale, const float* l2_decay, const float* gradient_clip,
                                const float* epsilon, const float* momentum);
int rmsprop_momentum_step_multi(int count, cudamat** grads, cudamat** params, cudamat** histories, cudamat** rms_histories,
                                const float* factor, const float* l2_decay, const float* gradient_clip, const float* epsilon,
                                const float* momentum);
int softmax_ce_grad_correct(cudamat* logits, cudamat* labels, cudamat* probs, cudamat* deriv,
                            cudamat* correct_accum, float deriv_scale);
int relu_dropout(rnd_struct* rnd_state, cudamat* mat, float dropprob, float scale);
/* The logistic and softmax-distribution layers in fewer passes.  Error codes as for the entries they replace; the accumulators must be
 * 1x1 device matrices (ERROR_INCOMPATIBLE_DIMENSIONS otherwise).
 *  logistic_dropout     : apply_sigmoid(mat, mat) then dropout(p, 0, scale) (src/layer.cc:391,597) in one pass over mat.  Draws the
 *                         Philox value dropout would draw for each element and advances the call counter once, as dropout does: the
 *                         same mask and the same bits as the two calls.
 *  logistic_deriv_scaled: mult_by_scalar(deriv, scale) then apply_logistic_deriv(deriv, state, deriv) (Layer::ApplyDerivativeofDropout
 *                         + LogisticLayer::ApplyDerivativeOfActivation, src/layer.cc:399-413,600-602) in place:
 *                         deriv = ((deriv * scale) * state) * (1 - state), every product separately rounded, bit-identical to the two
 *                         calls; scale == 1 skips the first product (no dropout: the reference issues no Mult either).
 *  logistic_ce_grad_correct: apply_sigmoid(logits, probs) + apply_logistic_grad(probs, targets, deriv) + mult_by_scalar(deriv,
 *                         deriv_scale) + get_logistic_correct_normalized + the sum of its (rows, 1) result (src/layer.cc:597,
 *                         src/loss_functions.cc:93-95,130-135).  probs may alias logits.  probs and deriv are bit-identical to the
 *                         sequence; the sum over rows of the normalised correct share is ADDED to correct_accum: per-block partials in
 *                         row order, then one block adds them in a fixed order — no atomics, the same bits from call to call, and no
 *                         device-to-host copy, so the host reads it every print_after steps.
 *  softmax_dist_ce_grad : softmax_row_major(logits, probs) + subtract_elementwise(probs, targets, deriv) + mult_by_scalar(deriv,
 *                         deriv_scale) + compute_cross_entropy(targets, probs, .., tiny) + the sum of its result (src/layer.cc:570,
 *                         src/loss_functions.cc:100-110); targets holds one distribution per row.  probs may alias logits.  probs and
 *                         deriv are bit-identical to the sequence; the sum of -t * log(p + tiny) is ADDED to ce_accum the same
 *                         atomics-free way (fp32 partial sums: tolerance-equal to a float64 sum). */
int logistic_dropout(rnd_struct* rnd_state, cudamat* mat, float dropprob, float scale);
int logistic_deriv_scaled(cudamat* deriv, cudamat* state, float scale);
int logistic_ce_grad_correct(cudamat* logits, cudamat* targets, cudamat* probs, cudamat* deriv, cudamat* correct_accum,
                             float deriv_scale);
int softmax_dist_ce_grad(cudamat* logits, cudamat* targets, cudamat* probs, cudamat* deriv, cudamat* ce_accum, float deriv_scale,
                         float tiny);
/* Gaussian dropout (Layer with dropprob > 0 and gaussian_dropout, src/layer.cc:369-377 and 399-404) in one pass each way and without a
 * stored noise matrix: the backward pass draws the forward pass's noise again from the counter value that call used (its call id).
 *   z[i]     = the float fill_with_randn writes to element i of a matrix of the same element count when the state's call counter
 *              equals the call id: same key, Philox quad i / 4 counted from the first element of the matrix or view, same Box-Muller.
 *   noise[i] = (z[i] * stddev) + 1, two separately rounded fp32 operations.  stddev is the layer's dropprob: a standard deviation.
 *  gaussian_dropout      : takes the counter's value as this call's id, writes it to *call_id (call_id: NULL, or the address of an
 *                          unsigned 64-bit integer) and advances the counter once, as fill_with_randn does.  In place:
 *                          x = act(mat[i]) with act 0 the identity, 1 lower_bound_scalar(0), 2 apply_sigmoid's arithmetic;
 *                          x = x * noise[i]; when max_act > 0, upper_bound_mod_scalar(max_act).  Bit for bit what the sequence
 *                          [activation entry,] fill_with_randn, mult_by_scalar, add_scalar, mult_elementwise[, upper_bound_mod_scalar]
 *                          leaves in the state.
 *  gaussian_dropout_noise: target = noise of the given call id — the matrix that sequence holds in its noise matrix.  The seed comes
 *                          from rnd_state; the counter is neither read nor advanced.
 *  gaussian_dropout_undo : the counter is untouched.  n = noise[i]; d = deriv[i] * n; s = state[i] / n (IEEE division, as
 *                          divide_elementwise); deriv[i] = d (act 0), apply_rectified_linear_deriv(d, s) (act 1) or
 *                          apply_logistic_deriv(d, s) with its three roundings (act 2): Layer::ApplyDerivativeofDropout followed by the
 *                          layer's ApplyDerivativeOfActivation at the restored state.  restore_state != 0 also writes s to state[i]
 *                          (the reference's bits); 0 leaves the state untouched.
 * One launch per call, no workspace, no atomics, the same bits from call to call.  ERROR_GENERIC for a NULL or uninitialised rnd_state,
 * ERROR_NOT_ON_DEVICE, ERROR_INCOMPATIBLE_DIMENSIONS when deriv and state differ in shape, ERROR_UNSUPPORTED for act outside 0..2 and
 * for more than INT_MAX (2^31 - 1) floats; nothing is launched and no counter moves on an error.  (A call id is a 64-bit counter value;
 * it travels as size_t, which is 64 bits wide on every platform this library builds for.) */
int gaussian_dropout(rnd_struct* rnd_state, cudamat* mat, float stddev, float max_act, int act, void* call_id);
int gaussian_dropout_noise(rnd_struct* rnd_state, size_t call_id, float stddev, cudamat* target);
int gaussian_dropout_undo(rnd_struct* rnd_state, size_t call_id, float stddev, cudamat* deriv, cudamat* state, int act,
                          int restore_state);
/* Batch normalisation of a layer's state in place, `state` read as (numel / C, C) with C = numel(gamma) (layer.cc:454: Reshape(-1, C));
 * gamma, beta, mu, sigma, batch_mu, batch_sigma are C-float device vectors.
 *  bn_fprop_act  : Layer::ApplyBatchNormalization(train) (src/layer.cc:452-480) [+ ReLULayer::ApplyActivation, layer.cc:549-551 when
 *                  relu != 0].  train != 0: batch_mu = mean, batch_sigma = sqrt(biased variance + bn_epsilon) from ONE read of the
 *                  state (per-wave Welford partials, Chan's combine in segment order; tolerance-equal to the reference's centred two
 *                  passes SumRows / AddRowVec / SqSumAxis / Add / Sqrt), mu = bn_f·mu + (1-bn_f)·batch_mu, sigma likewise (the running
 *                  average of the STD); then state = (state - m)·(gamma/s) + beta with (m, s) = the batch statistics (train) or
 *                  (mu, sigma) (train == 0; batch_mu / batch_sigma are then not touched and may be empty).  Replaces 12 calls
 *                  (9 passes over the state, 11 with the ReLU) by 3 passes; per element within a few ulp of the reference sequence.
 *  bn_bprop_fused: Layer::ApplyDerivativeofBatchNormalization (src/layer.cc:482-510) without the optimizer steps: with
 *                  y = (state - beta)/gamma recovered in registers, dbeta = mean(deriv), dgamma = mean(deriv·y),
 *                  deriv = (deriv - dgamma·y - mean(deriv - dgamma·y))·gamma/batch_sigma.  `state` is only read (the reference
 *                  rewrites it twice), so a weight gradient reading it on another stream needs no ordering.  Replaces 8 calls
 *                  (19 passes) by 5 passes; tolerance-equal to the reference sequence.
 * Both return ERROR_UNSUPPORTED for tensors of more than INT_MAX (2^31 - 1) floats, as do the three entries above.  Bit-identical
 * from call to call. */
int bn_fprop_act(cudamat* state, cudamat* gamma, cudamat* beta, cudamat* mu, cudamat* sigma, cudamat* batch_mu, cudamat* batch_sigma,
                 float bn_f, float bn_epsilon, int train, int relu);
int bn_bprop_fused(cudamat* deriv, cudamat* state, cudamat* gamma, cudamat* beta, cudamat* batch_sigma, cudamat* dgamma,
                   cudamat* dbeta);
/* Backward fusions: the producing kernel applies the consumer layer's ReLU' (and dropout' scale) in
 * its epilogue instead of a separate read-modify-write pass over the derivative
 * (Layer::ApplyDerivativeofDropout + ReLULayer::ApplyDerivativeOfActivation, src/layer.cc:399-413,556-558):
 *   targets = (state > 0) ? post_scale * (scaleTargets*targets + op(...)) : 0.
 * Valid when the layer has a single outgoing edge (src/convnet.cc:390-404 applies them after ALL edges). */
void convDownMask(cudamat* derivs, cudamat* filters, cudamat* state, cudamat* targets,
                  Shape4D* derivs_shape, Shape4D* filters_shape, Shape4D* targets_shape,
                  ConvDesc conv_desc, float scaleTargets, float post_scale);
int dotMask(cudamat* mat1, cudamat* mat2, cudamat* state, cudamat* target, float beta, float alpha,
            float post_scale);
void MaxPoolUndoRelu(cudamat* images, cudamat* maxGrads, cudamat* maxActs, cudamat* targets,
                     Shape4D* images_shape, Shape4D* maxGrads_shape, ConvDesc conv_desc,
                     float scaleTargets);
/* MaxPoolEdge::ComputeUp / ComputeDown (src/maxpool_edge.cc:27-45) with a window mask instead of a second pass over the layer's input:
 * MaxPoolMask = MaxPool (scaleTargets 0, scaleOutput 1) that ALSO writes, per pooled element, 16 bits into `mask`: bit 3*dy + dx set when
 * input (dy, dx) of its window lies inside the image and equals the maximum (float ==, every tie: what kMaxPoolUndo tests,
 * cudamat_conv_gemm.cu:220-262), bit 9 set when the maximum is > 0.  `mask` is any device matrix of at least numel(targets) / 2 floats,
 * 16-byte aligned, laid out as uint16 in the pooled tensor's own element order.  MaxPoolUndoMask = MaxPoolUndo (relu == 0) or
 * MaxPoolUndoRelu (relu != 0) computed from (maxGrads, mask) alone — neither the layer's input nor its maxima are read — and bit-identical
 * to them as long as `mask` is what MaxPoolMask wrote for the tensors the undo would have been given.  3 x 3 windows, stride 2,
 * padding >= 0, N % 4 == 0 only, and relu != 0 only with scaleTargets == 0 (MaxPoolUndoRelu masks the accumulated target too, by
 * input > 0, which the masks hold only for inputs that are a maximum): anything else returns ERROR_UNSUPPORTED and touches nothing
 * (call MaxPool / MaxPoolUndo / MaxPoolUndoRelu). */
int MaxPoolMask(cudamat* images, cudamat* targets, cudamat* mask, Shape4D* images_shape, Shape4D* targets_shape, ConvDesc conv_desc);
int MaxPoolUndoMask(cudamat* maxGrads, cudamat* mask, cudamat* targets, Shape4D* targets_shape, Shape4D* maxGrads_shape,
                    ConvDesc conv_desc, float scaleTargets, int relu);
/* ResponseNormEdge::ComputeUp + the ReLU of a RECTIFIED_LINEAR destination layer (layer.cc:549) in one pass. */
void ResponseNormCrossMapRelu(cudamat* images, cudamat* targets, int numFilters, int sizeF,
                              float addScale, float powScale, bool blocked);
/* ConvEdge::ComputeOuter (conv_edge.cc:183-221) in one call: dW as convOutpGemm AND the shared-bias gradient
 * bias_grad(1,F) = scaleTargets*bias_grad + scaleOutput * sum over images and output pixels of derivs — the reference's
 * two-step SumRows (:210-221).  The bias row rides as a virtual tap with constant input 1 in the weight-gradient tile
 * when the tile has a spare row (conv1: 147 -> 148 of 160), else the library falls back to a column sum. */
void convOutpBias(cudamat* images, cudamat* derivs, cudamat* targets, cudamat* bias_grad,
                  Shape4D* images_shape, Shape4D* derivs_shape, Shape4D* targets_shape,
                  ConvDesc conv_desc, float scaleTargets, float scaleOutput);

/* ---- introspection: what the last conv / dot / pooling / response-norm call launched ---------------
 * A pooling or response-norm call overwrites the report of the conv / dot call before it: read it right after the call it is about. */
typedef struct ConvnetHipKernelInfo {
  const char* name;      /* conv / dot: kernel family.  Pooling / response norm: the kernel build and the arm the grid cannot show
                            ("pool_undo_kernel<max>/scalar", "rnorm_undo_lds_kernel<16>/512/vec"; a string literal of the library) */
  double flops;          /* algorithmic flops of that call (2*M*N*K); 0 for pooling / response norm */
  int grid_blocks;       /* blocks launched (pooling / response norm: idle XCD-order blocks included) */
  int split_k;           /* 1 for pooling / response norm */
} ConvnetHipKernelInfo;
void convnet_hip_last_kernel_info(ConvnetHipKernelInfo* out);
/* Per-launch HIP-event timing on the library stream (used by bench.py's roofline leg).  While enabled
 * every conv/FC/pool/norm launch is bracketed by two hipEventRecord calls; the report synchronises,
 * aggregates by (kernel, op) into text lines "kernel|op|launches|total_ms|total_flops|total_bytes|total_executed_flops"
 * (flops = algorithmic work; executed = MFMA work issued, larger for dgrad gathers that run border taps on the zero page). */
void convnet_hip_profile_enable(int on);
size_t convnet_hip_profile_report(char* buf, size_t cap);
/* What the chip sustains on the instruction the default GEMM kernels execute (v_mfma_f32_32x32x16_bf16, six per fp32 product block),
 * with nothing else in the way: one wave per SIMD, sixteen accumulators, register operands — the h / m / l planes of N(0,1) values
 * (random_operands = 1) or zeros (0) — for about `seconds`.  The part clocks to its power budget, so this is the ceiling a kernel of
 * these instructions has on this box, beside the nominal 2.5 PFLOP/s (csrc/probe.hip).  out4 = {executed bf16 TFLOP/s, the same / 6 =
 * algorithmic fp32 TFLOP/s, GHz by the shader-cycle counter over wall time, GHz the MFMA issue rate implies}.  Returns 0 or an error code. */
int convnet_hip_probe_matrix_pipe(int random_operands, double seconds, double* out4);

/* ---- data-parallel gradient exchange (csrc/comm.hip): replaces ConvNet::Accumulate + ConvNet::Broadcast ------------------
 * Reference (src/convnet.cc:407-450, behind USE_MPI): after Bprop the whole flat gradient goes device -> host, rank 0
 * MPI_Recv-sums every rank's copy, divides by num_processes_ (:431), copies it back and MPI_Bcasts it; UpdateWeights (:440-450)
 * then steps every edge.  Here: one process per GPU, RCCL over xGMI, every slice (or bucket of slices) of the flat gradient is
 * all-reduced on a communication stream from the moment it is final, and the compute stream waits — on the device, not the
 * host — right before the optimizer step that consumes it.  librccl is dlopen'ed by convnet_hip_comm_init.
 *
 *   rank 0:   convnet_hip_comm_unique_id(id);  ship the 128 bytes to the other ranks (MPI_Bcast / a file / a socket)
 *   all:      convnet_hip_comm_init(rank, nranks, id);  convnet_hip_comm_broadcast(&parameters, 0);      // convnet.cc:309
 *   Bprop(output, input, edge), after edge.ComputeOuter:  convnet_hip_comm_allreduce_avg(&grad_parameters, off, n, slot);
 *   UpdateWeights, before edge->UpdateWeights():          convnet_hip_comm_wait(slot);
 * `slot` (0..255) names the done-event of one post; it stays waitable until the same slot is posted again.
 * grad[off .. off+n) becomes sum over ranks / nranks (true division, as :431).  Returns 0 or a cudamat error code
 * (get_last_cuda_error() has the RCCL text). */
#define CONVNET_HIP_COMM_ID_BYTES 128
int convnet_hip_comm_unique_id(char* id_out);
int convnet_hip_comm_init(int rank, int nranks, const char* id_in);
int convnet_hip_comm_rank(void);
int convnet_hip_comm_size(void);
int convnet_hip_comm_max_slots(void);   /* slots [0, max_slots) exist (256): plan the posts of one step against it up front */
int convnet_hip_comm_broadcast(cudamat* mat, int root);
int convnet_hip_comm_allreduce_avg(cudamat* flat, size_t offset, size_t count, int slot);
int convnet_hip_comm_wait(int slot);
int convnet_hip_comm_sync(void);      /* host-blocking drain of the communication stream */
int convnet_hip_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif  /* CONVNET_HIP_H_ */
