// LPIPS (VGG16) glue around the split 3x3 convolutions (sgic_conv3x3_split3_f32): the input layer, ReLU (+ 2x2 max-pool) into the
// next convolution's zero-halo operand planes, and the LPIPS head (include/sgic.h).  All three are bandwidth
// work: every lane moves 16 bytes along the 32-channel slice of the slice-major plane layout (split3.h).  The head has no float
// atomics: a workgroup writes one partial and a last kernel adds the partials of an image in a fixed order, so two runs give the
// same bits.  Built with -ffp-contract=off: one IEEE operation per written operation (the input layer is compared for equality).
#include <math.h>

#include "common.h"
#include "split3.h"

namespace {

typedef unsigned lp_u32x4 __attribute__((ext_vector_type(4)));
typedef float lp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;              // threads of every kernel here
constexpr int MAX_GRID = 1 << 20;    // grid-stride launches
constexpr int HEAD_LANES = 16;       // lanes that share a pixel in the head
constexpr int HEAD_PIX = 128;        // pixels per workgroup: 16 groups x 8 passes

inline unsigned grid_for(size_t threads) {
  const size_t g = (threads + NT - 1) / NT;
  return (unsigned)(g < 1 ? 1 : (g > (size_t)MAX_GRID ? (size_t)MAX_GRID : g));
}

// u8 (B, H, W, 3) -> the interior of the planes [3][1][Btot (H+2) (W+2)][32] of images img0 .. img0+B-1.  Four lanes per pixel, 16
// bytes (8 channels) each and plane: lane 0 carries the three values, the others zeros.
__global__ __launch_bounds__(NT) void lpips_input_kernel(const unsigned char *__restrict__ img, int B, int H, int W, int Btot, int img0,
                                                         unsigned short *__restrict__ planes) {
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
    lp_u32x4 o0 = {0u, 0u, 0u, 0u}, o1 = o0, o2 = o0;
    if (q == 0) {
      const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = (float)px[c] / 255.0f * 2.0f - 1.0f;
        v[c] = (u - shift[c]) / scale[c];
      }
      unsigned a0, b0, c0, a1, b1, c1;
      s3_split_pair(v[0], v[1], a0, b0, c0);
      s3_split_pair(v[2], 0.0f, a1, b1, c1);
      o0.x = a0, o0.y = a1;
      o1.x = b0, o1.y = b1;
      o2.x = c0, o2.y = c1;
    }
    const size_t dst = prow * 32 + q * 8;
    *reinterpret_cast<lp_u32x4 *>(planes + dst) = o0;
    *reinterpret_cast<lp_u32x4 *>(planes + plane + dst) = o1;
    *reinterpret_cast<lp_u32x4 *>(planes + 2 * plane + dst) = o2;
  }
}

__device__ __forceinline__ lp_f32x4 relu4(lp_f32x4 v) { return lp_f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }
__device__ __forceinline__ lp_f32x4 max4(lp_f32x4 a, lp_f32x4 b) {
  return lp_f32x4{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)};
}

// fp32 (B H W, C) -> relu -> optional 2x2 / stride 2 max-pool (floor) -> the interior of the planes [3][C / 32][B (OH+2) (OW+2)][32].
// A lane owns 8 channels of one output pixel; lanes run along the slice, then the row, so a wave writes whole 64-byte slices of
// neighbouring pixels: consecutive bytes in each plane.
template <int POOL>
__global__ __launch_bounds__(NT) void relu_pool_halo_kernel(const float *__restrict__ in, int B, int H, int W, int C,
                                                            unsigned short *__restrict__ planes) {
  const int OH = POOL ? H >> 1 : H, OW = POOL ? W >> 1 : W;
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
    const int iy = POOL ? oy * 2 : oy, ix = POOL ? ox * 2 : ox;
    const float *p = in + (((size_t)b * H + iy) * W + ix) * C + slice * 32 + q * 8;
    lp_f32x4 v0 = reinterpret_cast<const lp_f32x4 *>(p)[0], v1 = reinterpret_cast<const lp_f32x4 *>(p)[1];
    if (POOL) {
      const float *pr = p + C, *pd = p + (size_t)W * C, *pdr = pd + C;
      v0 = max4(max4(v0, reinterpret_cast<const lp_f32x4 *>(pr)[0]),
                max4(reinterpret_cast<const lp_f32x4 *>(pd)[0], reinterpret_cast<const lp_f32x4 *>(pdr)[0]));
      v1 = max4(max4(v1, reinterpret_cast<const lp_f32x4 *>(pr)[1]),
                max4(reinterpret_cast<const lp_f32x4 *>(pd)[1], reinterpret_cast<const lp_f32x4 *>(pdr)[1]));
    }
    v0 = relu4(v0);       // relu is monotone: relu(max) == max(relu)
    v1 = relu4(v1);
    unsigned a[4], m[4], l[4];
    s3_split_pair(v0.x, v0.y, a[0], m[0], l[0]);
    s3_split_pair(v0.z, v0.w, a[1], m[1], l[1]);
    s3_split_pair(v1.x, v1.y, a[2], m[2], l[2]);
    s3_split_pair(v1.z, v1.w, a[3], m[3], l[3]);
    const lp_u32x4 o0 = {a[0], a[1], a[2], a[3]}, o1 = {m[0], m[1], m[2], m[3]}, o2 = {l[0], l[1], l[2], l[3]};
    const size_t prow = ((size_t)b * (OH + 2) + oy + 1) * (OW + 2) + ox + 1;
    const size_t dst = ((size_t)slice * rows + prow) * 32 + q * 8;
    *reinterpret_cast<lp_u32x4 *>(planes + dst) = o0;
    *reinterpret_cast<lp_u32x4 *>(planes + plane + dst) = o1;
    *reinterpret_cast<lp_u32x4 *>(planes + 2 * plane + dst) = o2;
  }
}

__device__ __forceinline__ double group_sum(double v) {   // over the HEAD_LANES lanes of a pixel (they sit inside one wave)
#pragma unroll
  for (int o = HEAD_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one workgroup: HEAD_PIX pixels of one image pair.  Sixteen lanes share a pixel: each takes every 16th group of four channels,
// the two squared norms and the weighted sum are reduced with wave shuffles; fp64 throughout (a few operations per 4 bytes read).
// The second pass reads the pixel's two rows again (they are in cache) so that no per-lane array is needed whatever C is.
__global__ __launch_bounds__(NT) void lpips_head_kernel(const float *__restrict__ feat, const float *__restrict__ w, int B, long HW, int C,
                                                        double *__restrict__ part) {
  __shared__ double sh[NT / HEAD_LANES];
  const int lane = threadIdx.x & (HEAD_LANES - 1), grp = threadIdx.x / HEAD_LANES;
  const int b = blockIdx.y, C4 = C >> 2;
  const long pix0 = (long)blockIdx.x * HEAD_PIX;
  double gsum = 0.0;
  for (int pass = 0; pass < HEAD_PIX / (NT / HEAD_LANES); ++pass) {
    const long p = pix0 + pass * (NT / HEAD_LANES) + grp;
    const bool valid = p < HW;
    const long pc = valid ? p : HW - 1;      // uniform control flow around the shuffles: a pixel past the end is computed and dropped
    const lp_f32x4 *fa = reinterpret_cast<const lp_f32x4 *>(feat + ((size_t)b * HW + pc) * C);
    const lp_f32x4 *fb = reinterpret_cast<const lp_f32x4 *>(feat + ((size_t)(B + b) * HW + pc) * C);
    double sa = 0.0, sb = 0.0;
    for (int c = lane; c < C4; c += HEAD_LANES) {
      const lp_f32x4 x = relu4(fa[c]), y = relu4(fb[c]);
      sa += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
      sb += (double)y.x * y.x + (double)y.y * y.y + (double)y.z * y.z + (double)y.w * y.w;
    }
    const double ia = 1.0 / (sqrt(group_sum(sa)) + 1e-10), ib = 1.0 / (sqrt(group_sum(sb)) + 1e-10);
    double acc = 0.0;
    for (int c = lane; c < C4; c += HEAD_LANES) {
      const lp_f32x4 x = relu4(fa[c]), y = relu4(fb[c]), ww = reinterpret_cast<const lp_f32x4 *>(w)[c];
      const double d0 = x.x * ia - y.x * ib, d1 = x.y * ia - y.y * ib, d2 = x.z * ia - y.z * ib, d3 = x.w * ia - y.w * ib;
      acc += (double)ww.x * (d0 * d0) + (double)ww.y * (d1 * d1) + (double)ww.z * (d2 * d2) + (double)ww.w * (d3 * d3);
    }
    acc = group_sum(acc);
    gsum += valid ? acc : 0.0;
  }
  if (lane == 0) sh[grp] = gsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < NT / HEAD_LANES; ++g) s += sh[g];
    part[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// d[b] = (sum of image b's partials) / HW: thread t adds partials t, t + 256, ... in order, then a fixed tree over the 256 sums
__global__ __launch_bounds__(NT) void lpips_head_sum_kernel(const double *__restrict__ part, int nwg, long HW, double *__restrict__ d) {
  __shared__ double sh[NT];
  const double *p = part + (size_t)blockIdx.x * nwg;
  double s = 0.0;
  for (int i = threadIdx.x; i < nwg; i += NT) s += p[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) d[blockIdx.x] = sh[0] / (double)HW;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline size_t head_wgs(long HW) { return (size_t)((HW + HEAD_PIX - 1) / HEAD_PIX); }

}  // namespace

extern "C" int sgic_lpips_input_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                                       uint16_t *d_halo_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_img && d_halo_planes, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(image_offset >= 0 && total_images >= 1 && (long)image_offset + B <= (long)total_images, "image slots");
  SGIC_REQUIRE((long)total_images * (H + 2) * (W + 2) < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned16(d_halo_planes), "planes must be 16-byte aligned");
  lpips_input_kernel<<<grid_for((size_t)B * H * W * 4), NT, 0, to_stream(stream)>>>(d_img, B, H, W, total_images, image_offset, d_halo_planes);
  return sgic::check_launch("lpips_input_kernel");
}

extern "C" int sgic_relu_pool_halo_split3(const float *d_in, int B, int H, int W, int C, int pool2x2, uint16_t *d_halo_planes,
                                          sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_halo_planes, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  SGIC_REQUIRE(!pool2x2 || (H >= 2 && W >= 2), "the pool would leave no row or column");
  SGIC_REQUIRE((long)B * (H + 2) * (W + 2) < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned16(d_in) && aligned16(d_halo_planes), "buffers must be 16-byte aligned");
  const int OH = pool2x2 ? H / 2 : H, OW = pool2x2 ? W / 2 : W;
  const unsigned grid = grid_for((size_t)(C / 32) * B * OH * OW * 4);
  if (pool2x2) relu_pool_halo_kernel<1><<<grid, NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, d_halo_planes);
  else relu_pool_halo_kernel<0><<<grid, NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, d_halo_planes);
  return sgic::check_launch("relu_pool_halo_kernel");
}

extern "C" int sgic_lpips_head_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes && B >= 1 && B <= 65535 && H >= 1 && W >= 1, "args");
  *bytes = (size_t)B * head_wgs((long)H * W) * sizeof(double);
  return SGIC_OK;
}

extern "C" int sgic_lpips_head(const float *d_feat, const float *d_w, int B, int H, int W, int C, uint8_t *d_work, size_t work_bytes,
                               double *d_d, sgic_stream_t stream) {
  SGIC_REQUIRE(d_feat && d_w && d_work && d_d, "null pointer");
  SGIC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  SGIC_REQUIRE(2l * B * H * W < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned16(d_feat) && aligned16(d_w) && aligned16(d_work) && ((uintptr_t)d_d & 7) == 0, "buffers must be 16-byte aligned");
  const long HW = (long)H * W;
  const size_t nwg = head_wgs(HW);
  SGIC_REQUIRE(work_bytes >= (size_t)B * nwg * sizeof(double), "workspace too small (sgic_lpips_head_work_bytes)");
  hipStream_t st = to_stream(stream);
  lpips_head_kernel<<<dim3((unsigned)nwg, (unsigned)B), NT, 0, st>>>(d_feat, d_w, B, HW, C, reinterpret_cast<double *>(d_work));
  int rc = sgic::check_launch("lpips_head_kernel");
  if (rc != SGIC_OK) return rc;
  lpips_head_sum_kernel<<<B, NT, 0, st>>>(reinterpret_cast<const double *>(d_work), (int)nwg, HW, d_d);
  return sgic::check_launch("lpips_head_sum_kernel");
}
