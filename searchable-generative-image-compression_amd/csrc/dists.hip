// DISTS (VGG16) glue around the split 3x3 convolutions (sgic_conv3x3_split3_f32): the input layer, the exact u8 moments of tap 0, ReLU
// + L2 (Hanning) pool into the next convolution's zero-halo operand planes, and the second-order moments and head of taps 1..5
// (include/sgic.h).  The input layer and the pool are the shared producer kernels of producers.h with DistsNorm
// and ReluL2Pool; the moments move 16 bytes per lane along a pixel's channel row.  No float atomics: a workgroup writes one partial
// per channel and later kernels add the partials and the channels in a fixed order, so the same input gives the same bits (the u8
// moments are integers; their 64-bit atomic adds are exact in any order).
//
// L2 pool, per channel, fp32: r_t = max(v_t, 0) for the nine taps t = (ky, kx) of the 3x3 window centred on input (2 oy, 2 ox), a tap
// outside the image counting as 0; s = w_00 r_00^2, then s = s + w_t (r_t r_t) for t = 01, 02, 10, 11, 12, 20, 21, 22 in this order,
// w = (1, 2, 1) x (1, 2, 1) / 16 (powers of two: the products by w are exact); out = sqrtf(s + 1e-12f).
#include "producers.h"

namespace {

typedef unsigned long long ds_u64;

constexpr int U8_PIX = 4096;         // pixels of one pair per workgroup of the u8 moments: 16 per thread, so the u32 sums cannot overflow
constexpr int MOM_PIX = 256;         // the pixel range of a moments workgroup is a multiple of this ...
constexpr int MOM_MAX_WG = 256;      // ... chosen so that a pair has at most this many workgroups
constexpr int SUM_ROWS = 8;          // rows of threads that share a channel in the sum kernel

// the DISTS input layer of channel c of a u8 value
struct DistsNorm {
  __device__ __forceinline__ float operator()(unsigned u, int c) const {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    return ((float)u / 255.0f - mean[c]) / stdv[c];
  }
};

__device__ __forceinline__ ds_u64 wave_sum(ds_u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// tap 0: one workgroup adds up U8_PIX pixels of one pair; out (B, 3, 5) int64 += (sum a, sum b, sum a^2, sum b^2, sum a b) per channel.
// A thread sees at most 16 pixels, so its u32 sums stay below 16 * 255^2; waves and workgroups are added as 64-bit integers.
__global__ __launch_bounds__(NT) void dists_moments_u8_kernel(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b,
                                                              long HW, ds_u64 *__restrict__ out) {
  __shared__ ds_u64 sh[NT / 64][15];
  const int pair = blockIdx.y;
  const long p0 = (long)blockIdx.x * U8_PIX, p1 = p0 + U8_PIX < HW ? p0 + U8_PIX : HW;
  unsigned acc[3][5];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[c][k] = 0u;
  for (long p = p0 + threadIdx.x; p < p1; p += NT) {
    const unsigned char *pa = a + ((size_t)pair * HW + p) * 3, *pb = b + ((size_t)pair * HW + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned ua = pa[c], ub = pb[c];
      acc[c][0] += ua;
      acc[c][1] += ub;
      acc[c][2] += ua * ua;
      acc[c][3] += ub * ub;
      acc[c][4] += ua * ub;
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const ds_u64 s = wave_sum((ds_u64)acc[c][k]);
      if (lane == 0) sh[wave][c * 5 + k] = s;
    }
  __syncthreads();
  if (threadIdx.x < 15) {
    ds_u64 s = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += sh[w][threadIdx.x];
    atomicAdd(out + (size_t)pair * 15 + threadIdx.x, s);
  }
}

// halo_producer_kernel's op: relu -> square -> 3x3 Hanning window, stride 2, zero padding 1 -> + 1e-12 -> sqrt, OH = (H + 1) / 2.  The
// order of the sum is in the header comment.
struct ReluL2Pool {
  __device__ __forceinline__ void operator()(const float *__restrict__ in, int b, int oy, int ox, int slice, int q, int H, int W, int C,
                                             s3_f32x4 &o0, s3_f32x4 &o1) const {
    s3_f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float wgt = (ky == 1 ? 2.0f : 1.0f) * (kx == 1 ? 2.0f : 1.0f) * 0.0625f;
        s3_f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (inside) {
          const float *p = in + (((size_t)b * H + iy) * W + ix) * C + slice * 32 + q * 8;
          v0 = relu4(reinterpret_cast<const s3_f32x4 *>(p)[0]);
          v1 = relu4(reinterpret_cast<const s3_f32x4 *>(p)[1]);
        }
        s0 = s0 + wgt * (v0 * v0);
        s1 = s1 + wgt * (v1 * v1);
      }
    }
    s0 = s0 + 1e-12f;
    s1 = s1 + 1e-12f;
    o0 = s3_f32x4{sqrtf(s0.x), sqrtf(s0.y), sqrtf(s0.z), sqrtf(s0.w)};
    o1 = s3_f32x4{sqrtf(s1.x), sqrtf(s1.y), sqrtf(s1.z), sqrtf(s1.w)};
  }
};

// One workgroup: pixels [blockIdx.x ppw, (blockIdx.x + 1) ppw) of pair blockIdx.y, all C channels.  Thread t owns the four channels
// 4 (t % G) .. of the pixels t / G, t / G + PL, ... with G = C / 4, PL = 256 / G (threads past PL G idle): a pass of the workgroup
// reads 4 KiB of consecutive bytes of each side.  fp64 sums of relu(x), relu(y), their squares and their product (the products of two
// fp32 values are exact in fp64).  The PL threads of a channel are then added through LDS in the order of their rows, one of the five
// quantities at a time; part[pair][workgroup][quantity][C].
__global__ __launch_bounds__(NT) void dists_moments_kernel(const float *__restrict__ feat, int B, long HW, int C, long ppw,
                                                           double *__restrict__ part) {
  __shared__ double sh[NT][4];
  const int G = C >> 2, PL = NT / G;
  const int g = threadIdx.x % G, prow = threadIdx.x / G;
  const int b = blockIdx.y;
  const long p0 = (long)blockIdx.x * ppw, p1 = p0 + ppw < HW ? p0 + ppw : HW;
  double sx[4] = {0., 0., 0., 0.}, sy[4] = {0., 0., 0., 0.}, sxx[4] = {0., 0., 0., 0.}, syy[4] = {0., 0., 0., 0.}, sxy[4] = {0., 0., 0., 0.};
  if (prow < PL) {
    const s3_f32x4 *fa = reinterpret_cast<const s3_f32x4 *>(feat + (size_t)b * HW * C) + g;
    const s3_f32x4 *fb = reinterpret_cast<const s3_f32x4 *>(feat + (size_t)(B + b) * HW * C) + g;
    for (long p = p0 + prow; p < p1; p += PL) {
      const s3_f32x4 xv = relu4(fa[(size_t)p * G]), yv = relu4(fb[(size_t)p * G]);
      const double x[4] = {xv.x, xv.y, xv.z, xv.w}, y[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sx[j] += x[j];
        sy[j] += y[j];
        sxx[j] += x[j] * x[j];
        syy[j] += y[j] * y[j];
        sxy[j] += x[j] * y[j];
      }
    }
  }
  double *dst = part + ((size_t)b * gridDim.x + blockIdx.x) * 5 * C + 4 * g;
#define DS_REDUCE(acc, qi)                                                 \
  do {                                                                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) sh[threadIdx.x][j] = acc[j]; \
    __syncthreads();                                                       \
    if (prow == 0) {                                                       \
      double s[4] = {sh[g][0], sh[g][1], sh[g][2], sh[g][3]};              \
      for (int r = 1; r < PL; ++r)                                         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) s[j] += sh[r * G + g][j]; \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) dst[(size_t)(qi) * C + j] = s[j]; \
    }                                                                      \
    __syncthreads();                                                       \
  } while (0)
  DS_REDUCE(sx, 0);
  DS_REDUCE(sy, 1);
  DS_REDUCE(sxx, 2);
  DS_REDUCE(syy, 3);
  DS_REDUCE(sxy, 4);
#undef DS_REDUCE
}

// sums[pair][quantity][c] = the pair's partials added in a fixed order: SUM_ROWS rows of threads share 32 channels, row r adds the
// workgroups r, r + 8, ... in order, then the rows are added in order.  Grid (C / 32, pairs).
__global__ __launch_bounds__(NT) void dists_moments_sum_kernel(const double *__restrict__ part, int nwg, int C, double *__restrict__ sums) {
  __shared__ double sh[5][SUM_ROWS][32];
  const int lane = threadIdx.x & 31, r = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + lane, b = blockIdx.y;
  double a[5] = {0., 0., 0., 0., 0.};
  for (int w = r; w < nwg; w += SUM_ROWS) {
    const double *p = part + ((size_t)b * nwg + w) * 5 * C + c;
#pragma unroll
    for (int q = 0; q < 5; ++q) a[q] += p[(size_t)q * C];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) sh[q][r][lane] = a[q];
  __syncthreads();
  if (r == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double s = sh[q][0][lane];
#pragma unroll
      for (int k = 1; k < SUM_ROWS; ++k) s += sh[q][k][lane];
      sums[((size_t)b * 5 + q) * C + c] = s;
    }
  }
}

// one workgroup per pair: terms[pair] = (sum_c alpha_c (1 - S1_c), sum_c beta_c (1 - S2_c)).  Thread t adds the channels t, t + 256,
// ... in order, then a fixed tree over the 256 sums.  The variances and the covariance are one expression, E[uv] - E[u] E[v], so that
// x == y gives S2 == 1 (and S1 == 1) exactly.
__global__ __launch_bounds__(NT) void dists_head_kernel(const double *__restrict__ sums, const float *__restrict__ alpha,
                                                        const float *__restrict__ beta, int C, double n, double *__restrict__ terms) {
  __shared__ double sh[2][NT];
  const double *s = sums + (size_t)blockIdx.x * 5 * C;
  double t1 = 0.0, t2 = 0.0;
  for (int c = threadIdx.x; c < C; c += NT) {
    const double mx = s[c] / n, my = s[C + c] / n;
    const double vx = s[2 * C + c] / n - mx * mx, vy = s[3 * C + c] / n - my * my, cxy = s[4 * C + c] / n - mx * my;
    const double S1 = (2.0 * (mx * my) + 1e-6) / ((mx * mx + my * my) + 1e-6);
    const double S2 = (2.0 * cxy + 1e-6) / ((vx + vy) + 1e-6);
    t1 += (double)alpha[c] * (1.0 - S1);
    t2 += (double)beta[c] * (1.0 - S2);
  }
  sh[0][threadIdx.x] = t1;
  sh[1][threadIdx.x] = t2;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    terms[(size_t)blockIdx.x * 2] = sh[0][0];
    terms[(size_t)blockIdx.x * 2 + 1] = sh[1][0];
  }
}

inline bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }
inline long mom_ppw(long HW) {      // pixels per moments workgroup: a multiple of MOM_PIX that leaves at most MOM_MAX_WG workgroups
  const long per = (long)MOM_PIX * MOM_MAX_WG;
  return MOM_PIX * ((HW + per - 1) / per);
}
inline size_t mom_wgs(long HW) {
  const long ppw = mom_ppw(HW);
  return (size_t)((HW + ppw - 1) / ppw);
}

}  // namespace

extern "C" int sgic_dists_input_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                                       uint16_t *d_halo_planes, sgic_stream_t stream) {
  return input_halo_launch<DistsNorm>(__func__, "dists_input_kernel", d_img, B, H, W, total_images, image_offset, d_halo_planes, stream);
}

extern "C" int sgic_dists_moments_u8(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, int64_t *d_sums, sgic_stream_t stream) {
  SGIC_REQUIRE(d_a && d_b && d_sums, "null pointer");
  SGIC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE((long)B * H * W < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned8(d_sums), "sums must be 8-byte aligned");
  const long HW = (long)H * W;
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(d_sums, 0, (size_t)B * 15 * sizeof(int64_t), st) != hipSuccess) return sgic::check_launch("dists_moments_u8 memset");
  dists_moments_u8_kernel<<<dim3((unsigned)((HW + U8_PIX - 1) / U8_PIX), (unsigned)B), NT, 0, st>>>(d_a, d_b, HW,
                                                                                                     reinterpret_cast<ds_u64 *>(d_sums));
  return sgic::check_launch("dists_moments_u8_kernel");
}

extern "C" int sgic_relu_l2pool_halo_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_halo_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_halo_planes, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  SGIC_REQUIRE((long)B * (H + 2) * (W + 2) < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned16(d_in) && aligned16(d_halo_planes), "buffers must be 16-byte aligned");
  return halo_producer_launch<ReluL2Pool>("relu_l2pool_halo_kernel", d_in, B, H, W, C, (H + 1) / 2, (W + 1) / 2, d_halo_planes, stream);
}

extern "C" int sgic_dists_moments_work_bytes(int B, int H, int W, int C, size_t *bytes) {
  SGIC_REQUIRE(bytes && B >= 1 && B <= 65535 && H >= 1 && W >= 1, "args");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0 && C <= 1024, "C must be a multiple of 32, at most 1024");
  *bytes = (size_t)B * mom_wgs((long)H * W) * 5 * C * sizeof(double);
  return SGIC_OK;
}

extern "C" int sgic_dists_moments(const float *d_feat, int B, int H, int W, int C, uint8_t *d_work, size_t work_bytes, double *d_sums,
                                  sgic_stream_t stream) {
  SGIC_REQUIRE(d_feat && d_work && d_sums, "null pointer");
  SGIC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0 && C <= 1024, "C must be a multiple of 32, at most 1024");
  SGIC_REQUIRE(2l * B * H * W < (1l << 31), "too many pixels");
  SGIC_REQUIRE(aligned16(d_feat) && aligned16(d_work) && aligned8(d_sums), "buffers must be 16-byte aligned");
  const long HW = (long)H * W;
  const size_t nwg = mom_wgs(HW);
  SGIC_REQUIRE(work_bytes >= (size_t)B * nwg * 5 * C * sizeof(double), "workspace too small (sgic_dists_moments_work_bytes)");
  hipStream_t st = to_stream(stream);
  double *part = reinterpret_cast<double *>(d_work);
  dists_moments_kernel<<<dim3((unsigned)nwg, (unsigned)B), NT, 0, st>>>(d_feat, B, HW, C, mom_ppw(HW), part);
  int rc = sgic::check_launch("dists_moments_kernel");
  if (rc != SGIC_OK) return rc;
  dists_moments_sum_kernel<<<dim3((unsigned)(C / 32), (unsigned)B), NT, 0, st>>>(part, (int)nwg, C, d_sums);
  return sgic::check_launch("dists_moments_sum_kernel");
}

extern "C" int sgic_dists_head(const double *d_sums, const float *d_alpha, const float *d_beta, int B, int H, int W, int C,
                               double *d_terms, sgic_stream_t stream) {
  SGIC_REQUIRE(d_sums && d_alpha && d_beta && d_terms, "null pointer");
  SGIC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "empty batch or image");
  SGIC_REQUIRE(C >= 32 && C % 32 == 0, "C must be a multiple of 32");
  SGIC_REQUIRE(aligned8(d_sums) && aligned8(d_terms) && ((uintptr_t)d_alpha & 3) == 0 && ((uintptr_t)d_beta & 3) == 0, "misaligned buffer");
  dists_head_kernel<<<B, NT, 0, to_stream(stream)>>>(d_sums, d_alpha, d_beta, C, (double)((long)H * W), d_terms);
  return sgic::check_launch("dists_head_kernel");
}
