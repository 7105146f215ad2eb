// Plane producers of the perceptual metrics (lpips.hip, lpips_alex.hip, dists.hip, fid.hip): what they share.  A producer writes the A
// operand of a convolution directly as slice-major bf16x3 planes (split3.h).  All of them are bandwidth work with one lane pattern: a
// lane owns 8 columns of one 32-column slice of one row and moves 16 bytes per plane (s3_store8); lanes run along the slice, then
// the rows, so a wave writes whole 64-byte slices of neighbouring rows: consecutive bytes in each plane.  Plain C++ and vector stores
// only.  The four files are built with -ffp-contract=off: one IEEE operation per written operation (the producers are compared for
// equality).
#pragma once
#include <math.h>

#include "common.h"
#include "split3.h"

constexpr int NT = 256;              // threads of every kernel of the four files
constexpr int MAX_GRID = 1 << 20;    // grid-stride launches
constexpr long ROW_LIMIT = 1l << 31;

inline unsigned grid_for(size_t threads) {
  const size_t g = (threads + NT - 1) / NT;
  return (unsigned)(g < 1 ? 1 : (g > (size_t)MAX_GRID ? (size_t)MAX_GRID : g));
}
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ s3_f32x4 relu4(s3_f32x4 v) { return s3_f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }
__device__ __forceinline__ s3_f32x4 max4(s3_f32x4 a, s3_f32x4 b) {
  return s3_f32x4{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)};
}

// the LPIPS input layer of channel c of a u8 value (lpips.hip, and the table of lpips_alex.hip)
struct LpipsNorm {
  __device__ __forceinline__ float operator()(unsigned u, int c) const {
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    return ((float)u / 255.0f * 2.0f - 1.0f - shift[c]) / scale[c];
  }
};

// u8 (B, H, W, 3) -> norm(u, c) -> the interior of the planes [3][1][Btot (H+2) (W+2)][32] of images img0 .. img0+B-1.  Four lanes per
// pixel: lane 0 carries the three values, the others zeros.
template <class Norm>
__global__ __launch_bounds__(NT) void input_halo_kernel(const unsigned char *__restrict__ img, int B, int H, int W, int Btot, int img0,
                                                        unsigned short *__restrict__ planes, Norm norm) {
  const size_t rows = (size_t)Btot * (H + 2) * (W + 2), plane = rows * 32;
  const size_t total = (size_t)B * H * W * 4;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i & 3);
    size_t t = i >> 2;
    const unsigned char *px = img + t * 3;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const size_t prow = ((size_t)(b + img0) * (H + 2) + y + 1) * (W + 2) + x + 1;
    s3_f32x4 v0 = {0.f, 0.f, 0.f, 0.f};
    if (q == 0) v0 = s3_f32x4{norm(px[0], 0), norm(px[1], 1), norm(px[2], 2), 0.f};
    s3_store8(planes, plane, prow * 32 + q * 8, v0, s3_f32x4{0.f, 0.f, 0.f, 0.f});
  }
}

// the checks and the launch of an input-layer entry point `func`
template <class Norm>
inline int input_halo_launch(const char *func, const char *kernel, const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                             uint16_t *d_halo_planes, sgic_stream_t stream) {
  SGIC_REQUIRE_AS(func, d_img && d_halo_planes, "null pointer");
  SGIC_REQUIRE_AS(func, B >= 1 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE_AS(func, image_offset >= 0 && total_images >= 1 && (long)image_offset + B <= (long)total_images, "image slots");
  SGIC_REQUIRE_AS(func, (long)total_images * (H + 2) * (W + 2) < (1l << 31), "too many pixels");
  SGIC_REQUIRE_AS(func, aligned16(d_halo_planes), "planes must be 16-byte aligned");
  input_halo_kernel<<<grid_for((size_t)B * H * W * 4), NT, 0, to_stream(stream)>>>(d_img, B, H, W, total_images, image_offset, d_halo_planes, Norm());
  return sgic::check_launch(kernel);
}

// fp32 (B H W, C) -> op: the 8 channels slice 32 + q 8 .. of output pixel (b, oy, ox) of an OH x OW map -> the interior of the planes
// [3][C / 32][B (OH+2) (OW+2)][32].  op(in, b, oy, ox, slice, q, H, W, C, v0, v1) reads what it needs of `in` and leaves the values in
// (v0, v1); the halo ring is never written (it stays zero, ops.halo_planes_buffer).
template <class Op>
__global__ __launch_bounds__(NT) void halo_producer_kernel(const float *__restrict__ in, int B, int H, int W, int C, int OH, int OW,
                                                           unsigned short *__restrict__ planes, Op op) {
  const size_t rows = (size_t)B * (OH + 2) * (OW + 2), plane = rows * C;
  const size_t total = (size_t)(C >> 5) * B * OH * OW * 4;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i & 3);
    size_t t = i >> 2;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    t /= OH;
    const int b = (int)(t % B);
    const int slice = (int)(t / B);
    s3_f32x4 v0, v1;
    op(in, b, oy, ox, slice, q, H, W, C, v0, v1);
    const size_t prow = ((size_t)b * (OH + 2) + oy + 1) * (OW + 2) + ox + 1;
    s3_store8(planes, plane, ((size_t)slice * rows + prow) * 32 + q * 8, v0, v1);
  }
}

// the launch the halo entry points share, after their own checks; `kernel`: the name a launch error reports
template <class Op>
inline int halo_producer_launch(const char *kernel, const float *d_in, int B, int H, int W, int C, int OH, int OW, uint16_t *d_halo_planes,
                                sgic_stream_t stream) {
  halo_producer_kernel<<<grid_for((size_t)(C / 32) * B * OH * OW * 4), NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, OH, OW, d_halo_planes, Op());
  return sgic::check_launch(kernel);
}
