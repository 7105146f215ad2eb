// LPIPS (VGG16) glue around the split 3x3 convolutions (sgic_conv3x3_split3_f32): the input layer, ReLU (+ 2x2 max-pool) into the
// next convolution's zero-halo operand planes, and the LPIPS head (include/sgic.h).  The first two are the
// shared producer kernels of producers.h with LpipsNorm and this file's ReluPool2.  The head has no float atomics: a workgroup writes
// one partial and a last kernel adds the partials of an image in a fixed order, so two runs give the same bits.
#include "producers.h"

namespace {

constexpr int HEAD_LANES = 16;       // lanes that share a pixel in the head
constexpr int HEAD_PIX = 128;        // pixels per workgroup: 16 groups x 8 passes

// halo_producer_kernel's op: relu, after a 2x2 / stride 2 max-pool (floor) when POOL
template <int POOL>
struct ReluPool2 {
  __device__ __forceinline__ void operator()(const float *__restrict__ in, int b, int oy, int ox, int slice, int q, int H, int W, int C,
                                             s3_f32x4 &v0, s3_f32x4 &v1) const {
    const int iy = POOL ? oy * 2 : oy, ix = POOL ? ox * 2 : ox;
    const float *p = in + (((size_t)b * H + iy) * W + ix) * C + slice * 32 + q * 8;
    v0 = reinterpret_cast<const s3_f32x4 *>(p)[0], v1 = reinterpret_cast<const s3_f32x4 *>(p)[1];
    if (POOL) {
      const float *pr = p + C, *pd = p + (size_t)W * C, *pdr = pd + C;
      v0 = max4(max4(v0, reinterpret_cast<const s3_f32x4 *>(pr)[0]),
                max4(reinterpret_cast<const s3_f32x4 *>(pd)[0], reinterpret_cast<const s3_f32x4 *>(pdr)[0]));
      v1 = max4(max4(v1, reinterpret_cast<const s3_f32x4 *>(pr)[1]),
                max4(reinterpret_cast<const s3_f32x4 *>(pd)[1], reinterpret_cast<const s3_f32x4 *>(pdr)[1]));
    }
    v0 = relu4(v0);       // relu is monotone: relu(max) == max(relu)
    v1 = relu4(v1);
  }
};

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
    const s3_f32x4 *fa = reinterpret_cast<const s3_f32x4 *>(feat + ((size_t)b * HW + pc) * C);
    const s3_f32x4 *fb = reinterpret_cast<const s3_f32x4 *>(feat + ((size_t)(B + b) * HW + pc) * C);
    double sa = 0.0, sb = 0.0;
    for (int c = lane; c < C4; c += HEAD_LANES) {
      const s3_f32x4 x = relu4(fa[c]), y = relu4(fb[c]);
      sa += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
      sb += (double)y.x * y.x + (double)y.y * y.y + (double)y.z * y.z + (double)y.w * y.w;
    }
    const double ia = 1.0 / (sqrt(group_sum(sa)) + 1e-10), ib = 1.0 / (sqrt(group_sum(sb)) + 1e-10);
    double acc = 0.0;
    for (int c = lane; c < C4; c += HEAD_LANES) {
      const s3_f32x4 x = relu4(fa[c]), y = relu4(fb[c]), ww = reinterpret_cast<const s3_f32x4 *>(w)[c];
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

inline size_t head_wgs(long HW) { return (size_t)((HW + HEAD_PIX - 1) / HEAD_PIX); }

}  // namespace

extern "C" int sgic_lpips_input_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                                       uint16_t *d_halo_planes, sgic_stream_t stream) {
  return input_halo_launch<LpipsNorm>(__func__, "lpips_input_kernel", d_img, B, H, W, total_images, image_offset, d_halo_planes, stream);
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
  if (pool2x2) return halo_producer_launch<ReluPool2<1>>("relu_pool_halo_kernel", d_in, B, H, W, C, OH, OW, d_halo_planes, stream);
  return halo_producer_launch<ReluPool2<0>>("relu_pool_halo_kernel", d_in, B, H, W, C, OH, OW, d_halo_planes, stream);
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
