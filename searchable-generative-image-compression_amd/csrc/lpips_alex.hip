// LPIPS (AlexNet) producers (include/sgic.h): the operands of the two convolutions that do not fit the implicit
// 3x3 path are written as patch matrices, directly as slice-major bf16x3 planes (split3.h), and run through sgic_gemm_split3_f32;
// the 3x3 / stride 2 max-pool in front of the third convolution writes that convolution's zero-halo planes through the shared
// halo_producer_kernel.  The lane pattern and the helpers are those of producers.h; the two patch kernels keep their own loops (their
// index maps differ).
#include "producers.h"

namespace {

constexpr int K1 = 363, K1P = 384;   // 11 * 11 * 3 columns of the first patch matrix, padded to whole slices
constexpr int ROWK = 33;             // columns of one ky: 11 pixels x 3 channels, consecutive bytes of an image row

// u8 (B, H, W, 3) -> rows (img0 + b, oy, ox) of the A operand [3][12][Btot h1 w1][32] of the 11x11 / stride 4 / pad 2 convolution:
// column k = (ky 11 + kx) 3 + c holds the input layer at pixel (4 oy - 2 + ky, 4 ox - 2 + kx), zero outside the image and for
// k >= 363.  For one ky the 33 columns are 33 consecutive bytes of image row 4 oy - 2 + ky, from byte 3 (4 ox - 2): a lane's 8
// columns are 8 consecutive bytes (of one or two ky).  The input layer has 256 values per channel: a workgroup first tabulates
// them in LDS with the definition's own operations, the lanes then look their bytes up.
__global__ __launch_bounds__(NT) void alex_conv1_patches_kernel(const unsigned char *__restrict__ img, int B, int H, int W, int h1, int w1,
                                                                int Btot, int img0, unsigned short *__restrict__ planes) {
  __shared__ float lut[3 * 256];
#pragma unroll
  for (int c = 0; c < 3; ++c) lut[c * 256 + threadIdx.x] = LpipsNorm()(threadIdx.x, c);
  __syncthreads();
  const size_t rows = (size_t)Btot * h1 * w1, plane = rows * K1P;
  const size_t total = (size_t)(K1P / 32) * B * h1 * w1 * 4;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i & 3);
    size_t t = i >> 2;
    const int ox = (int)(t % w1);
    t /= w1;
    const int oy = (int)(t % h1);
    t /= h1;
    const int b = (int)(t % B);
    const int slice = (int)(t / B);
    const int k0 = slice * 32 + q * 8, iy0 = 4 * oy - 2, ix0 = 4 * ox - 2;
    const unsigned char *im = img + (size_t)b * H * W * 3;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j, ky = k / ROWK, rem = k - ky * ROWK, dx = rem / 3, c = rem - dx * 3;
      const int iy = iy0 + ky, ix = ix0 + dx;
      const bool ok = k < K1 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      v[j] = 0.0f;
      if (ok) v[j] = lut[c * 256 + im[((long)iy * W + ix0) * 3 + rem]];     // ix >= 0, so 3 ix0 + rem >= 0
    }
    const size_t row = ((size_t)(b + img0) * h1 + oy) * w1 + ox;
    s3_store8(planes, plane, ((size_t)slice * rows + row) * 32 + q * 8, s3_f32x4{v[0], v[1], v[2], v[3]}, s3_f32x4{v[4], v[5], v[6], v[7]});
  }
}

// halo_producer_kernel's op: relu -> max over the 3 x 3 window at (2 oy, 2 ox) of 8 channels (3x3 / stride 2, floor); relu is
// monotone, so the maximum starts at 0
struct ReluMaxPool3 {
  __device__ __forceinline__ void operator()(const float *__restrict__ in, int b, int oy, int ox, int slice, int q, int H, int W, int C,
                                             s3_f32x4 &v0, s3_f32x4 &v1) const {
    const float *p = in + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + slice * 32 + q * 8;
    v0 = s3_f32x4{0.f, 0.f, 0.f, 0.f};
    v1 = v0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const s3_f32x4 *s = reinterpret_cast<const s3_f32x4 *>(p + ((size_t)dy * W + dx) * C);
        v0 = max4(v0, s[0]);
        v1 = max4(v1, s[1]);
      }
    }
  }
};

// fp32 (B H W, C) -> relu -> max-pool 3x3 / 2 (floor) to PH x PW -> the A operand [3][25 C / 32][B PH PW][32] of the 5x5 / pad 2
// convolution: column k = (ky 5 + kx) C + c of row (b, oy, ox) holds the pooled value at (oy + ky - 2, ox + kx - 2), zero outside
// the pooled map.  A lane owns 8 channels of one position (py, px) of the pooled map extended by 2 on every side, pools it once
// (nine 32-byte reads; zero in the extension) and writes it to the up to 25 rows (py - ky + 2, px - kx + 2) whose tap (ky, kx) it
// is: every (row, tap) has exactly one source position in the extended map, so the whole operand is written, the zeros too.  For
// one tap the lanes of a wave (4 per position, positions along px) write whole 64-byte slices of neighbouring rows.
__global__ __launch_bounds__(NT) void relu_maxpool3_patches5_kernel(const float *__restrict__ in, int B, int H, int W, int C, int PH, int PW,
                                                                    unsigned short *__restrict__ planes) {
  const int EH = PH + 4, EW = PW + 4, CS = C >> 5;
  const size_t rows = (size_t)B * PH * PW, plane = rows * 25 * C;
  const size_t total = (size_t)CS * B * EH * EW * 4;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i & 3);
    size_t t = i >> 2;
    const int ex = (int)(t % EW);
    t /= EW;
    const int ey = (int)(t % EH);
    t /= EH;
    const int b = (int)(t % B);
    const int cs = (int)(t / B);
    const int py = ey - 2, px = ex - 2;
    s3_f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if ((unsigned)py < (unsigned)PH && (unsigned)px < (unsigned)PW) ReluMaxPool3()(in, b, py, px, cs, q, H, W, C, v0, v1);
    for (int ky = 0; ky < 5; ++ky) {
      const int oy = ey - ky;
      if ((unsigned)oy >= (unsigned)PH) continue;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const int ox = ex - kx;
        if ((unsigned)ox >= (unsigned)PW) continue;
        const size_t row = ((size_t)b * PH + oy) * PW + ox;
        s3_store8(planes, plane, ((size_t)((ky * 5 + kx) * CS + cs) * rows + row) * 32 + q * 8, v0, v1);
      }
    }
  }
}

}  // namespace

extern "C" int sgic_lpips_alex_conv1_patches_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                                                    uint16_t *d_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_img && d_planes, "null pointer");
  SGIC_REQUIRE(B >= 1, "empty batch");
  SGIC_REQUIRE(H >= 7 && W >= 7, "the 11x11 / stride 4 / pad 2 convolution would leave no row or column");
  SGIC_REQUIRE(image_offset >= 0 && total_images >= 1 && (long)image_offset + B <= (long)total_images, "image slots");
  const int h1 = (H - 7) / 4 + 1, w1 = (W - 7) / 4 + 1;
  SGIC_REQUIRE((long)total_images * h1 * w1 < ROW_LIMIT && (long)B * H * W < ROW_LIMIT, "too many rows");
  SGIC_REQUIRE(aligned16(d_planes), "planes must be 16-byte aligned");
  alex_conv1_patches_kernel<<<grid_for((size_t)(K1P / 32) * B * h1 * w1 * 4), NT, 0, to_stream(stream)>>>(d_img, B, H, W, h1, w1, total_images,
                                                                                                         image_offset, d_planes);
  return sgic::check_launch("alex_conv1_patches_kernel");
}

extern "C" int sgic_relu_maxpool3_patches5_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_planes, "null pointer");
  SGIC_REQUIRE(B >= 1, "empty batch");
  SGIC_REQUIRE(H >= 3 && W >= 3, "the pool would leave no row or column");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  const int PH = (H - 3) / 2 + 1, PW = (W - 3) / 2 + 1;
  SGIC_REQUIRE((long)B * H * W < ROW_LIMIT && (long)B * (PH + 4) * (PW + 4) < ROW_LIMIT, "too many rows");
  SGIC_REQUIRE(aligned16(d_in) && aligned16(d_planes), "buffers must be 16-byte aligned");
  relu_maxpool3_patches5_kernel<<<grid_for((size_t)(C / 32) * B * (PH + 4) * (PW + 4) * 4), NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, PH, PW,
                                                                                                                     d_planes);
  return sgic::check_launch("relu_maxpool3_patches5_kernel");
}

extern "C" int sgic_relu_maxpool3_halo_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_halo_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_halo_planes, "null pointer");
  SGIC_REQUIRE(B >= 1, "empty batch");
  SGIC_REQUIRE(H >= 3 && W >= 3, "the pool would leave no row or column");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  const int PH = (H - 3) / 2 + 1, PW = (W - 3) / 2 + 1;
  SGIC_REQUIRE((long)B * H * W < ROW_LIMIT && (long)B * (PH + 2) * (PW + 2) < ROW_LIMIT, "too many rows");
  SGIC_REQUIRE(aligned16(d_in) && aligned16(d_halo_planes), "buffers must be 16-byte aligned");
  return halo_producer_launch<ReluMaxPool3>("relu_maxpool3_halo_kernel", d_in, B, H, W, C, PH, PW, d_halo_planes, stream);
}
