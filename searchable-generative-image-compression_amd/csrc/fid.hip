// FID / KID kernels (include/sgic.h): the input step of pytorch-fid's Inception-v3, the one generic patch producer
// that writes a convolution's A operand directly as slice-major bf16x3 planes (split3.h) for sgic_gemm_split3_f32, the three pools of
// the Inception graph with the ReLU applied on read, the final ReLU + spatial mean, and an fp64 Gram kernel for the second moments of
// FID and the kernel sums of KID.  All bandwidth work except the Gram.  The patch producer has the lane pattern and the helpers of
// producers.h and its own loop (its index map is generic in kernel, stride and padding).  No atomics.
#include "producers.h"

namespace {

constexpr int S = 299;               // the Inception input extent

// the source position of output index d of an `in` -> 299 bilinear resize, align_corners = False: src = max((d + 0.5) in / 299 - 0.5, 0)
// = max((2 d + 1) in - 299, 0) / 598, in integers: i0 = floor(src), lambda = the remainder / 598 (one fp32 division)
__device__ __forceinline__ void src_of(int d, int in, int &i0, int &i1, float &lam) {
  const long num = (long)(2 * d + 1) * in - S;
  const long nn = num < 0 ? 0 : num;
  i0 = (int)(nn / (2 * S));
  lam = (float)(int)(nn - (long)i0 * (2 * S)) / (float)(2 * S);
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
}

// u8 canvas (B, H, W, 3), descriptors (image, y0, x0, h, w) -> fp32 (n, 299, 299, 3): x = u / 255, the window resized bilinearly
// (PyTorch's align_corners = False, no antialiasing), y = 2 x - 1.  One lane per output pixel, three channels.
__global__ __launch_bounds__(NT) void fid_resize299_kernel(const unsigned char *__restrict__ canvas, int H, int W, const int *__restrict__ desc,
                                                           int n, float *__restrict__ out) {
  const size_t total = (size_t)n * S * S;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int ox = (int)(i % S);
    const size_t t = i / S;
    const int oy = (int)(t % S), p = (int)(t / S);
    const int *d = desc + 5 * p;
    const int img = d[0], y0 = d[1], x0 = d[2], h = d[3], w = d[4];
    int ya, yb, xa, xb;
    float ly, lx;
    src_of(oy, h, ya, yb, ly);
    src_of(ox, w, xa, xb, lx);
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const unsigned char *base = canvas + ((size_t)img * H * W) * 3;
    const unsigned char *r0 = base + ((size_t)(y0 + ya) * W + x0) * 3, *r1 = base + ((size_t)(y0 + yb) * W + x0) * 3;
    float *o = out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p00 = (float)r0[xa * 3 + c] / 255.0f, p01 = (float)r0[xb * 3 + c] / 255.0f;
      const float p10 = (float)r1[xa * 3 + c] / 255.0f, p11 = (float)r1[xb * 3 + c] / 255.0f;
      const float top = hx * p00 + lx * p01, bot = hx * p10 + lx * p11;
      const float x = hy * top + ly * bot;
      o[c] = 2.0f * x - 1.0f;
    }
  }
}

// fp32 NHWC rows of leading dimension ld, columns col0 .. col0 + C - 1 -> optional relu -> the kh x kw patches with stride (sh, sw)
// and zero padding (ph, pw) as the A operand [3][Kp / 32][B OH OW][32]: column k = (ky kw + kx) C + c of row (b, oy, ox) holds the
// input at (oy sh - ph + ky, ox sw - pw + kx), zero outside the map and for k >= kh kw C.  Every element of the operand is written.
// FAST (C % 8 == 0, 16-byte aligned rows): a lane's 8 columns are 32 consecutive bytes of one tap.
template <bool FAST>
__global__ __launch_bounds__(NT) void patches_split3_kernel(const float *__restrict__ in, int ld, int col0, int B, int H, int W, int C, int kh, int kw,
                                                            int sh, int sw, int ph, int pw, int OH, int OW, int Kp, int relu,
                                                            unsigned short *__restrict__ planes) {
  const size_t rows = (size_t)B * OH * OW, plane = rows * Kp;
  const size_t total = (size_t)(Kp >> 5) * rows * 4;
  const int taps = kh * kw, K = taps * C;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i & 3);
    const size_t t = i >> 2;
    const size_t row = t % rows;
    const int slice = (int)(t / rows);
    const int ox = (int)(row % OW);
    const size_t t2 = row / OW;
    const int oy = (int)(t2 % OH), b = (int)(t2 / OH);
    const int k0 = slice * 32 + q * 8, iy0 = oy * sh - ph, ix0 = ox * sw - pw;
    const float *im = in + (size_t)b * H * W * ld + col0;
    s3_f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (FAST) {
      const int tap = k0 / C, c = k0 - tap * C, ky = tap / kw, kx = tap - ky * kw;
      const int iy = iy0 + ky, ix = ix0 + kx;
      if (tap < taps && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
        const s3_f32x4 *s = reinterpret_cast<const s3_f32x4 *>(im + ((size_t)iy * W + ix) * ld + c);
        v0 = s[0];
        v1 = s[1];
        if (relu) {
          v0 = relu4(v0);
          v1 = relu4(v1);
        }
      }
    } else {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + j, tap = k / C, c = k - tap * C, ky = tap / kw, kx = tap - ky * kw;
        const int iy = iy0 + ky, ix = ix0 + kx;
        v[j] = 0.0f;
        if (k < K && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
          const float x = im[((size_t)iy * W + ix) * ld + c];
          v[j] = relu ? fmaxf(x, 0.f) : x;
        }
      }
      v0 = s3_f32x4{v[0], v[1], v[2], v[3]};
      v1 = s3_f32x4{v[4], v[5], v[6], v[7]};
    }
    s3_store8(planes, plane, ((size_t)slice * rows + row) * 32 + q * 8, v0, v1);
  }
}

// fp32 (B H W, C) BEFORE relu -> relu -> a 3 x 3 pool -> fp32 rows of leading dimension ldo at column co.  MODE 0: max, stride 2, no
// padding, floor.  MODE 1: average, stride 1, zero padding 1, the divisor is the number of taps inside the map; the taps are summed
// in row-major order, then divided once.  MODE 2: max, stride 1, padding 1 (relu >= 0, so a tap outside the map never wins).
// A lane owns 4 channels of one output position.
template <int MODE>
__global__ __launch_bounds__(NT) void relu_pool3_kernel(const float *__restrict__ in, int B, int H, int W, int C, int OH, int OW, float *__restrict__ out,
                                                        int ldo, int co) {
  const int C4 = C >> 2;
  const size_t total = (size_t)B * OH * OW * C4;
  constexpr int st = MODE == 0 ? 2 : 1, pad = MODE == 0 ? 0 : 1;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int c4 = (int)(i % C4);
    const size_t row = i / C4;
    const int ox = (int)(row % OW);
    const size_t t2 = row / OW;
    const int oy = (int)(t2 % OH), b = (int)(t2 / OH);
    s3_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = oy * st - pad + dy;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = ox * st - pad + dx;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
          const s3_f32x4 s = relu4(*reinterpret_cast<const s3_f32x4 *>(in + (((size_t)b * H + iy) * W + ix) * C + c4 * 4));
          if (MODE == 1) {
            acc = s3_f32x4{acc.x + s.x, acc.y + s.y, acc.z + s.z, acc.w + s.w};
            ++cnt;
          } else {
            acc = max4(acc, s);
          }
        }
      }
    }
    if (MODE == 1) {
      const float d = (float)cnt;
      acc = s3_f32x4{acc.x / d, acc.y / d, acc.z / d, acc.w / d};
    }
    *reinterpret_cast<s3_f32x4 *>(out + row * ldo + co + c4 * 4) = acc;
  }
}

// fp32 (B R, C) BEFORE relu -> out[b][c] = (relu(x[b][0][c]) + relu(x[b][1][c]) + ... in row order, one fp32 accumulator) / R.  One lane
// per (b, c): the order does not depend on B or on the launch.
__global__ __launch_bounds__(NT) void relu_mean_rows_kernel(const float *__restrict__ in, int B, int R, int C, float *__restrict__ out) {
  const size_t total = (size_t)B * C;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int c = (int)(i % C);
    const size_t b = i / C;
    const float *p = in + b * R * C + c;
    float acc = 0.0f;
    for (int r = 0; r < R; ++r) acc = acc + fmaxf(p[(size_t)r * C], 0.f);
    out[i] = acc / (float)R;
  }
}

// C[i][j] = sum_k A[ia[i]][k] B[ib[j]][k] in fp64 from fp32 inputs; k runs 0 .. K - 1 in order in one accumulator per element (the
// products of two fp32 values are exact in fp64, so the fma is one rounding either way), so the result does not depend on the tiling.  A workgroup owns a 64 x 64 tile of
// C, a lane 4 x 4 of it; 16 k at a time pass through LDS, transposed (k-major).  A row index outside [0, rows) reads as a zero row.
constexpr int GT = 64, GK = 16;
__global__ __launch_bounds__(NT) void gram_f64_kernel(const float *__restrict__ A, long lda, const int *__restrict__ ia, int rows_a, int n,
                                                      const float *__restrict__ Bm, long ldb, const int *__restrict__ ib, int rows_b, int m, int K,
                                                      double *__restrict__ Cm, long ldc) {
  __shared__ alignas(16) float As[GK][GT + 4], Bs[GK][GT + 4];      // read as 16-byte vectors: rows of 68 floats = 17 x 16 bytes
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;      // this lane loads 4 k of row lr of both tiles
  long ra = -1, rb = -1;
  if (i0 + lr < n) {
    const long r = ia ? (long)ia[i0 + lr] : (long)(i0 + lr);
    if (r >= 0 && r < rows_a) ra = r;
  }
  if (j0 + lr < m) {
    const long r = ib ? (long)ib[j0 + lr] : (long)(j0 + lr);
    if (r >= 0 && r < rows_b) rb = r;
  }
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + lk + j;
      As[lk + j][lr] = (ra >= 0 && k < K) ? A[ra * lda + k] : 0.0f;
      Bs[lk + j][lr] = (rb >= 0 && k < K) ? Bm[rb * ldb + k] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GK; ++k) {
      const s3_f32x4 a4 = *reinterpret_cast<const s3_f32x4 *>(&As[k][ty * 4]), b4 = *reinterpret_cast<const s3_f32x4 *>(&Bs[k][tx * 4]);
      const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
      const double b[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[p][r] = fma(a[p], b[r], acc[p][r]);      // the product is exact in fp64: the bits of multiply, then add
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + ty * 4 + p;
    if (i >= n) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + tx * 4 + r;
      if (j < m) Cm[(long)i * ldc + j] = acc[p][r];
    }
  }
}

inline int pool_check(const float *d_in, int B, int H, int W, int C, const float *d_out, int ldo, int co, bool stride2) {
  SGIC_REQUIRE(d_in && d_out, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "empty extent");
  SGIC_REQUIRE(!stride2 || (H >= 3 && W >= 3), "the pool would leave no row or column");
  SGIC_REQUIRE(C >= 4 && C % 4 == 0, "C must be a multiple of 4");
  SGIC_REQUIRE(co >= 0 && co % 4 == 0 && ldo % 4 == 0 && (long)co + C <= (long)ldo, "the output slice must be 16-byte aligned and inside ldo");
  SGIC_REQUIRE((long)B * H * W < ROW_LIMIT, "too many rows");
  SGIC_REQUIRE(aligned16(d_in) && aligned16(d_out), "buffers must be 16-byte aligned");
  return SGIC_OK;
}

}  // namespace

extern "C" int sgic_fid_resize299(const uint8_t *d_canvas, int B, int H, int W, const int32_t *h_desc, const int32_t *d_desc, int n, float *d_out,
                                  sgic_stream_t stream) {
  SGIC_REQUIRE(d_canvas && h_desc && d_desc && d_out, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && n >= 1, "empty extent");
  SGIC_REQUIRE((long)B * H * W < ROW_LIMIT && (long)n * S * S < ROW_LIMIT, "too many rows");
  for (int p = 0; p < n; ++p) {
    const int32_t *d = h_desc + 5 * p;
    SGIC_REQUIRE(d[0] >= 0 && d[0] < B, "descriptor: image outside the canvas");
    SGIC_REQUIRE(d[3] >= 1 && d[4] >= 1 && d[1] >= 0 && d[2] >= 0 && (long)d[1] + d[3] <= (long)H && (long)d[2] + d[4] <= (long)W,
                 "descriptor: window outside the canvas");
  }
  fid_resize299_kernel<<<grid_for((size_t)n * S * S), NT, 0, to_stream(stream)>>>(d_canvas, H, W, d_desc, n, d_out);
  return sgic::check_launch("fid_resize299_kernel");
}

extern "C" int sgic_patches_split3(const float *d_in, int ld, int col0, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                                   int relu, uint16_t *d_planes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_planes, "null pointer");
  SGIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "empty extent");
  SGIC_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1 && ph >= 0 && pw >= 0 && kh <= 64 && kw <= 64, "kernel, stride, padding");
  SGIC_REQUIRE(col0 >= 0 && (long)col0 + C <= (long)ld, "the column slice must lie inside ld");
  SGIC_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "the convolution would leave no row or column");
  SGIC_REQUIRE((long)kh * kw * C < (1l << 24), "too many columns");
  const int OH = (H + 2 * ph - kh) / sh + 1, OW = (W + 2 * pw - kw) / sw + 1, Kp = (kh * kw * C + 31) / 32 * 32;
  SGIC_REQUIRE((long)B * H * W < ROW_LIMIT && (long)B * OH * OW < ROW_LIMIT, "too many rows");
  SGIC_REQUIRE(aligned16(d_planes), "planes must be 16-byte aligned");
  const unsigned grid = grid_for((size_t)(Kp / 32) * B * OH * OW * 4);
  if (C % 8 == 0 && ld % 4 == 0 && col0 % 4 == 0 && aligned16(d_in))
    patches_split3_kernel<true><<<grid, NT, 0, to_stream(stream)>>>(d_in, ld, col0, B, H, W, C, kh, kw, sh, sw, ph, pw, OH, OW, Kp, relu != 0, d_planes);
  else
    patches_split3_kernel<false><<<grid, NT, 0, to_stream(stream)>>>(d_in, ld, col0, B, H, W, C, kh, kw, sh, sw, ph, pw, OH, OW, Kp, relu != 0, d_planes);
  return sgic::check_launch("patches_split3_kernel");
}

extern "C" int sgic_relu_maxpool3s2(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream) {
  const int rc = pool_check(d_in, B, H, W, C, d_out, ldo, co, true);
  if (rc != SGIC_OK) return rc;
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  relu_pool3_kernel<0><<<grid_for((size_t)B * OH * OW * (C / 4)), NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, OH, OW, d_out, ldo, co);
  return sgic::check_launch("relu_pool3_kernel<max, 2>");
}

extern "C" int sgic_relu_avgpool3s1p1(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream) {
  const int rc = pool_check(d_in, B, H, W, C, d_out, ldo, co, false);
  if (rc != SGIC_OK) return rc;
  relu_pool3_kernel<1><<<grid_for((size_t)B * H * W * (C / 4)), NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, H, W, d_out, ldo, co);
  return sgic::check_launch("relu_pool3_kernel<avg, 1>");
}

extern "C" int sgic_relu_maxpool3s1p1(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream) {
  const int rc = pool_check(d_in, B, H, W, C, d_out, ldo, co, false);
  if (rc != SGIC_OK) return rc;
  relu_pool3_kernel<2><<<grid_for((size_t)B * H * W * (C / 4)), NT, 0, to_stream(stream)>>>(d_in, B, H, W, C, H, W, d_out, ldo, co);
  return sgic::check_launch("relu_pool3_kernel<max, 1>");
}

extern "C" int sgic_relu_mean_rows(const float *d_in, int B, int R, int C, float *d_out, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out, "null pointer");
  SGIC_REQUIRE(B >= 1 && R >= 1 && C >= 1, "empty extent");
  SGIC_REQUIRE((long)B * R < ROW_LIMIT && (long)B * C < ROW_LIMIT, "too many rows");
  relu_mean_rows_kernel<<<grid_for((size_t)B * C), NT, 0, to_stream(stream)>>>(d_in, B, R, C, d_out);
  return sgic::check_launch("relu_mean_rows_kernel");
}

extern "C" int sgic_gram_f64(const float *d_a, long lda, const int32_t *d_ia, int rows_a, int n, const float *d_b, long ldb, const int32_t *d_ib,
                             int rows_b, int m, int K, double *d_c, long ldc, sgic_stream_t stream) {
  SGIC_REQUIRE(d_a && d_b && d_c, "null pointer");
  SGIC_REQUIRE(n >= 1 && m >= 1 && K >= 1 && rows_a >= 1 && rows_b >= 1, "empty extent");
  SGIC_REQUIRE(lda >= K && ldb >= K && ldc >= m, "leading dimensions");
  SGIC_REQUIRE(d_ia || n <= rows_a, "without row indices n rows of A are read");
  SGIC_REQUIRE(d_ib || m <= rows_b, "without row indices m rows of B are read");
  SGIC_REQUIRE((n + GT - 1) / GT <= 65535, "too many rows");
  const dim3 grid((unsigned)((m + GT - 1) / GT), (unsigned)((n + GT - 1) / GT));
  gram_f64_kernel<<<grid, NT, 0, to_stream(stream)>>>(d_a, lda, d_ia, rows_a, n, d_b, ldb, d_ib, rows_b, m, K, d_c, ldc);
  return sgic::check_launch("gram_f64_kernel");
}
