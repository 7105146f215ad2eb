// HBM-bound data-movement / elementwise kernels of the transform path (all fp32, float4-vectorised,
// coalesced along the channel axis).  Feature maps are "token x channel" (NHWC); the 16x16-tile-major
// row order TM16 (row = ((b*nH + y/16)*nW + x/16)*256 + (y%16)*16 + x%16) makes the reference's
// tile <-> stack rearranges (models/codec_sq_fixbpp.py:123-125, models/cross_blocks.py:78-79,96-97)
// the identity, so no gather/scatter pass is ever needed.
#include "common.h"
#include "pil_resample.h"
#include <limits.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long fmap_row(int b, int y, int x, int H, int W, int tile16) {
  if (!tile16) return ((long)b * H + y) * W + x;
  const int nH = H >> 4, nW = W >> 4;
  return ((((long)b * nH + (y >> 4)) * nW + (x >> 4)) << 8) + ((y & 15) << 4) + (x & 15);
}

#define GRID_STRIDE(i, n) for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)
static inline unsigned ew_grid(long n) {
  long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ------------------------------------------------------------------------------------------------
// im2col for non-overlapping PxP patches of an NCHW image, with the affine x*mul+add fused
// (codec: x*0.5+0.5 then patch_embed, codec_sq_fixbpp.py:855 + titok/blocks.py:98-100; CLIP conv1).
// out[(patch), c*P*P + ky*P + kx]; patch order plain (b,gy,gx) or TM16 over the patch grid.
// ------------------------------------------------------------------------------------------------
__global__ void im2col_patch_kernel(const float *__restrict__ x, int B, int C, int H, int W, int P, float mul, float add,
                                    int tile16, float *__restrict__ out) {
  const int gh = H / P, gw = W / P, K = C * P * P, P4 = P >> 2;
  const long total = (long)B * gh * gw * C * P * P4;  // float4 units
  GRID_STRIDE(i, total) {
    long t = i;
    const int kx4 = (int)(t % P4);
    t /= P4;
    const int ky = (int)(t % P);
    t /= P;
    const int c = (int)(t % C);
    t /= C;
    const int gx = (int)(t % gw);
    t /= gw;
    const int gy = (int)(t % gh);
    const int b = (int)(t / gh);
    f32x4 v = *reinterpret_cast<const f32x4 *>(x + (((long)b * C + c) * H + gy * P + ky) * W + gx * P + kx4 * 4);
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = v[e] * mul + add;
    const long row = fmap_row(b, gy, gx, gh, gw, tile16);
    *reinterpret_cast<f32x4 *>(out + row * K + (c * P + ky) * P + kx4 * 4) = v;
  }
}

extern "C" int sgic_im2col_patch(const float *d_x, int B, int C, int H, int W, int P, float mul, float add, int tile16,
                                 float *d_out, sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_out && B > 0 && C > 0 && P >= 4 && (P & 3) == 0 && H % P == 0 && W % P == 0, "args");
  SGIC_REQUIRE(!tile16 || ((H / P) % 16 == 0 && (W / P) % 16 == 0), "tile-major order needs a patch grid multiple of 16");
  SGIC_REQUIRE((W & 3) == 0 && ((uintptr_t)d_x & 15) == 0 && ((uintptr_t)d_out & 15) == 0, "alignment");
  const long total = (long)B * (H / P) * (W / P) * C * P * (P / 4);
  im2col_patch_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_x, B, C, H, W, P, mul, add, tile16, d_out);
  return sgic::check_launch("im2col_patch_kernel");
}

// ------------------------------------------------------------------------------------------------
// Token assembly:  out[n, 0]       = cls + pos[0]
//                  out[n, 1+p]     = emb[n*P + p] + pos[1+p]          p < P
//                  out[n, 1+P+t]   = lat[t] + latpos[t]               t < T   (T may be 0)
// (codec_sq_fixbpp.py:127-138; CLIP class/positional embedding)
// ------------------------------------------------------------------------------------------------
__global__ void assemble_tokens_kernel(const float *__restrict__ emb, const float *__restrict__ cls,
                                       const float *__restrict__ pos, const float *__restrict__ lat,
                                       const float *__restrict__ latpos, int N, int P, int T, int D,
                                       float *__restrict__ out) {
  const int L = 1 + P + T, D4 = D >> 2;
  const long total = (long)N * L * D4;
  GRID_STRIDE(i, total) {
    const int d4 = (int)(i % D4);
    const long r = i / D4;
    const int l = (int)(r % L);
    const int n = (int)(r / L);
    f32x4 a, b;
    if (l == 0) {
      a = reinterpret_cast<const f32x4 *>(cls)[d4];
      b = reinterpret_cast<const f32x4 *>(pos)[d4];
    } else if (l <= P) {
      a = reinterpret_cast<const f32x4 *>(emb + ((long)n * P + (l - 1)) * D)[d4];
      b = reinterpret_cast<const f32x4 *>(pos + (long)l * D)[d4];
    } else {
      a = reinterpret_cast<const f32x4 *>(lat + (long)(l - 1 - P) * D)[d4];
      b = reinterpret_cast<const f32x4 *>(latpos + (long)(l - 1 - P) * D)[d4];
    }
    reinterpret_cast<f32x4 *>(out + r * D)[d4] = a + b;
  }
}

extern "C" int sgic_assemble_tokens(const float *d_emb, const float *d_cls, const float *d_pos, const float *d_lat,
                                    const float *d_latpos, int N, int P, int T, int D, float *d_out,
                                    sgic_stream_t stream) {
  SGIC_REQUIRE(d_emb && d_cls && d_pos && d_out && N > 0 && P > 0 && T >= 0 && D > 0 && (D & 3) == 0, "args");
  SGIC_REQUIRE(T == 0 || (d_lat && d_latpos), "latent tokens");
  const long total = (long)N * (1 + P + T) * (D / 4);
  assemble_tokens_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_emb, d_cls, d_pos, d_lat, d_latpos, N, P, T, D,
                                                                         d_out);
  return sgic::check_launch("assemble_tokens_kernel");
}

// ------------------------------------------------------------------------------------------------
// out[n*oseg + l, :] = in[n*iseg + l, :] + vec[l, :]     l < Lr   (positional-embedding adds into a
// slice of a larger token buffer: models/cross_blocks.py:82-84).  vec may be null (pure strided copy).
// ------------------------------------------------------------------------------------------------
__global__ void add_rows_bcast_kernel(const float *__restrict__ in, int ldi, int iseg, const float *__restrict__ vec,
                                      float *__restrict__ out, int ldo, int oseg, int Nn, int Lr, int D) {
  const int D4 = D >> 2;
  const long total = (long)Nn * Lr * D4;
  GRID_STRIDE(i, total) {
    const int d4 = (int)(i % D4);
    const long r = i / D4;
    const int l = (int)(r % Lr);
    const int n = (int)(r / Lr);
    f32x4 a = reinterpret_cast<const f32x4 *>(in + ((long)n * iseg + l) * ldi)[d4];
    if (vec) a += reinterpret_cast<const f32x4 *>(vec + (long)l * D)[d4];
    reinterpret_cast<f32x4 *>(out + ((long)n * oseg + l) * ldo)[d4] = a;
  }
}

extern "C" int sgic_add_rows_bcast(const float *d_in, int ldi, int iseg, const float *d_vec, float *d_out, int ldo,
                                   int oseg, int Nn, int Lr, int D, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out && Nn > 0 && Lr > 0 && D > 0 && (D & 3) == 0 && (ldi & 3) == 0 && (ldo & 3) == 0, "args");
  const long total = (long)Nn * Lr * (D / 4);
  add_rows_bcast_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_in, ldi, iseg, d_vec, d_out, ldo, oseg, Nn, Lr, D);
  return sgic::check_launch("add_rows_bcast_kernel");
}

// ------------------------------------------------------------------------------------------------
// Depthwise kxk conv, stride 1, zero padding k/2, NHWC (plain or TM16 rows); weights re-laid as
// [k*k][C]; optional per-channel pre-scale (ConvNeXt applies layer_scale BEFORE the conv,
// blocks/conv_blocks.py:74-75; DepthConv dw3x3, blocks/dcvc.py:21,35).
// ------------------------------------------------------------------------------------------------
__global__ void dwconv_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                              const float *__restrict__ prescale, float *__restrict__ y, int B, int H, int W, int C,
                              int k, int tile16) {
  const int C4 = C >> 2, pad = k >> 1;
  const long total = (long)B * H * W * C4;
  GRID_STRIDE(i, total) {
    const int c4 = (int)(i % C4);
    long t = i / C4;
    const int xx = (int)(t % W);
    t /= W;
    const int yy = (int)(t % H);
    const int b = (int)(t / H);
    f32x4 acc = bias ? reinterpret_cast<const f32x4 *>(bias)[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ps = prescale ? reinterpret_cast<const f32x4 *>(prescale)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
    for (int ky = 0; ky < k; ky++) {
      const int sy = yy + ky - pad;
      if (sy < 0 || sy >= H) continue;
      for (int kx = 0; kx < k; kx++) {
        const int sx = xx + kx - pad;
        if (sx < 0 || sx >= W) continue;
        f32x4 v = reinterpret_cast<const f32x4 *>(x + fmap_row(b, sy, sx, H, W, tile16) * C)[c4];
        if (prescale) v *= ps;
        const f32x4 wv = reinterpret_cast<const f32x4 *>(w + (long)(ky * k + kx) * C)[c4];
        acc += v * wv;
      }
    }
    reinterpret_cast<f32x4 *>(y + fmap_row(b, yy, xx, H, W, tile16) * C)[c4] = acc;
  }
}

// Same convolution, four output pixels of one row per thread: the KS + 3 input float4s of a kernel row are loaded
// once and shared by the four outputs (65 loads per 4 outputs at 5x5 instead of 200).  Per output the taps are still
// accumulated in (ky, kx) order with separate multiply and add, so the result is bit-identical to dwconv_kernel
// (out-of-range taps contribute an exact zero).
template <int KS>
__global__ __launch_bounds__(256) void dwconv_x4_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                        const float *__restrict__ bias, const float *__restrict__ prescale,
                                                        float *__restrict__ y, int B, int H, int W, int C, int tile16) {
  constexpr int pad = KS >> 1;
  const int C4 = C >> 2, XG = W >> 2;
  const long total = (long)B * H * XG * C4;
  // XCD-aware order: workgroup ids are dealt round-robin over the 8 XCDs (each with its own L2); give every XCD a
  // contiguous eighth of the work so the KS rows a pixel needs are fetched into ONE L2 instead of up to KS of them
  long blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  for (long i = blk * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    long t = i / C4;
    const int x0 = (int)(t % XG) * 4;
    t /= XG;
    const int yy = (int)(t % H);
    const int b = (int)(t / H);
    const f32x4 bz = bias ? reinterpret_cast<const f32x4 *>(bias)[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 ps = prescale ? reinterpret_cast<const f32x4 *>(prescale)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
    f32x4 acc[4] = {bz, bz, bz, bz};
#pragma unroll
    for (int ky = 0; ky < KS; ky++) {
      const int sy = yy + ky - pad;
      if (sy < 0 || sy >= H) continue;
      f32x4 in[KS + 3];
#pragma unroll
      for (int j = 0; j < KS + 3; j++) {
        const int sx = x0 + j - pad;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (sx >= 0 && sx < W) {
          v = reinterpret_cast<const f32x4 *>(x + fmap_row(b, sy, sx, H, W, tile16) * C)[c4];
          if (prescale) v *= ps;
        }
        in[j] = v;
      }
#pragma unroll
      for (int kx = 0; kx < KS; kx++) {
        const f32x4 wv = reinterpret_cast<const f32x4 *>(w + (long)(ky * KS + kx) * C)[c4];
#pragma unroll
        for (int o = 0; o < 4; o++) acc[o] += in[o + kx] * wv;
      }
    }
#pragma unroll
    for (int o = 0; o < 4; o++) reinterpret_cast<f32x4 *>(y + fmap_row(b, yy, x0 + o, H, W, tile16) * C)[c4] = acc[o];
  }
}

extern "C" int sgic_dwconv_nhwc(const float *d_x, const float *d_w, const float *d_bias, const float *d_prescale,
                                float *d_y, int B, int H, int W, int C, int k, int tile16, sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_w && d_y && d_x != d_y && B > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && (k & 1) == 1, "args");
  SGIC_REQUIRE(!tile16 || (H % 16 == 0 && W % 16 == 0), "tile-major layout needs H,W multiples of 16");
  const long total = (long)B * H * W * (C / 4);
  if ((W & 3) == 0 && (k == 3 || k == 5)) {
    const unsigned grid = (unsigned)((total / 4 + 255) / 256);   // one pass, no grid stride: the XCD remap needs the exact grid
    if (k == 5) dwconv_x4_kernel<5><<<grid, 256, 0, to_stream(stream)>>>(d_x, d_w, d_bias, d_prescale, d_y, B, H, W, C, tile16);
    else dwconv_x4_kernel<3><<<grid, 256, 0, to_stream(stream)>>>(d_x, d_w, d_bias, d_prescale, d_y, B, H, W, C, tile16);
    return sgic::check_launch("dwconv_x4_kernel");
  }
  dwconv_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_x, d_w, d_bias, d_prescale, d_y, B, H, W, C, k, tile16);
  return sgic::check_launch("dwconv_kernel");
}

// ------------------------------------------------------------------------------------------------
// im2col for the 2x2 stride-2 conv of feat_out (codec_sq_fixbpp.py:90): NHWC (TM16 or plain) in,
// out[(b, y/2, x/2) plain][(ky*2+kx)*C + c]
// ------------------------------------------------------------------------------------------------
__global__ void im2col_2x2_kernel(const float *__restrict__ x, int B, int H, int W, int C, int tile16,
                                  float *__restrict__ out) {
  const int C4 = C >> 2, OH = H >> 1, OW = W >> 1;
  const long total = (long)B * OH * OW * 4 * C4;
  GRID_STRIDE(i, total) {
    const int c4 = (int)(i % C4);
    long t = i / C4;
    const int kk = (int)(t & 3);
    t >>= 2;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const f32x4 v = reinterpret_cast<const f32x4 *>(x + fmap_row(b, oy * 2 + (kk >> 1), ox * 2 + (kk & 1), H, W, tile16) * C)[c4];
    reinterpret_cast<f32x4 *>(out + ((((long)b * OH + oy) * OW + ox) * 4 + kk) * C)[c4] = v;
  }
}

extern "C" int sgic_im2col_2x2(const float *d_x, int B, int H, int W, int C, int tile16, float *d_out,
                               sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_out && B > 0 && H > 0 && W > 0 && (H & 1) == 0 && (W & 1) == 0 && (C & 3) == 0, "args");
  const long total = (long)B * (H / 2) * (W / 2) * C;
  im2col_2x2_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_x, B, H, W, C, tile16, d_out);
  return sgic::check_launch("im2col_2x2_kernel");
}

// ------------------------------------------------------------------------------------------------
// ConvFFN3 gate: out[m,c] = LeakyReLU_0.1(x[m,c]) + LeakyReLU_0.01(x[m,C2+c])   (blocks/dcvc.py:50-53)
// ------------------------------------------------------------------------------------------------
__global__ void gated_lrelu_kernel(const float *__restrict__ x, float *__restrict__ out, long M, int C2) {
  const int C4 = C2 >> 2;
  const long total = M * C4;
  GRID_STRIDE(i, total) {
    const int c4 = (int)(i % C4);
    const long m = i / C4;
    const f32x4 a = reinterpret_cast<const f32x4 *>(x + m * 2 * C2)[c4];
    const f32x4 b = reinterpret_cast<const f32x4 *>(x + m * 2 * C2 + C2)[c4];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = (a[e] >= 0.f ? a[e] : 0.1f * a[e]) + (b[e] >= 0.f ? b[e] : 0.01f * b[e]);
    reinterpret_cast<f32x4 *>(out + m * C2)[c4] = o;
  }
}

extern "C" int sgic_gated_lrelu(const float *d_x, float *d_out, int M, int C2, sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_out && M > 0 && C2 > 0 && (C2 & 3) == 0, "args");
  gated_lrelu_kernel<<<ew_grid((long)M * C2 / 4), 256, 0, to_stream(stream)>>>(d_x, d_out, M, C2);
  return sgic::check_launch("gated_lrelu_kernel");
}

// ------------------------------------------------------------------------------------------------
// Broadcast column ops on (M, C) rows, vec has `vrows` rows of C and row m uses vec[m % vrows]:
//   mode 0: y = x * v          (enc_q / dec_q scaling, models/sq_bottleneck.py:111,117; y_hat*q_step)
//   mode 1: y = x / max(v,0.5) (y / clamp_min(q_step, 0.5), entropy/compression_model.py:325-326)
//   mode 2: y = x * max(v,0.5) (y_hat * clamp_min(q_step, 0.5), entropy/compression_model.py:355,414)
// ------------------------------------------------------------------------------------------------
__global__ void colop_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ v, int ldv, int vrows,
                             float *__restrict__ y, int ldy, long M, int C, int mode) {
  const int C4 = C >> 2;
  const long total = M * C4;
  GRID_STRIDE(i, total) {
    const int c4 = (int)(i % C4);
    const long m = i / C4;
    const f32x4 a = reinterpret_cast<const f32x4 *>(x + m * ldx)[c4];
    const f32x4 b = reinterpret_cast<const f32x4 *>(v + (m % vrows) * ldv)[c4];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = mode == 0 ? a[e] * b[e] : (mode == 1 ? a[e] / fmaxf(b[e], 0.5f) : a[e] * fmaxf(b[e], 0.5f));
    reinterpret_cast<f32x4 *>(y + m * ldy)[c4] = o;
  }
}

extern "C" int sgic_colop(const float *d_x, int ldx, const float *d_v, int ldv, int vrows, float *d_y, int ldy, int M,
                          int C, int mode, sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_v && d_y && M > 0 && C > 0 && (C & 3) == 0 && vrows > 0 && (mode >= 0 && mode <= 2), "args");
  SGIC_REQUIRE((ldx & 3) == 0 && (ldv & 3) == 0 && (ldy & 3) == 0, "leading dims multiple of 4");
  colop_kernel<<<ew_grid((long)M * C / 4), 256, 0, to_stream(stream)>>>(d_x, ldx, d_v, ldv, vrows, d_y, ldy, M, C, mode);
  return sgic::check_launch("colop_kernel");
}

// ------------------------------------------------------------------------------------------------
// "fake 2-D" reshape of the latent tokens (codec_sq_fixbpp.py:175-177): the (T, D) row-major block of
// each sequence is REINTERPRETED as (D, T); conv_out then contracts over the first axis.  We emit
// out[n][t][c] = in[n][c*T + t] so that conv_out is a plain GEMM over c.
// ------------------------------------------------------------------------------------------------
__global__ void fake2d_transpose_kernel(const float *__restrict__ in, long in_seq_stride, float *__restrict__ out, int N,
                                        int T, int D) {
  const long total = (long)N * T * D;
  GRID_STRIDE(i, total) {
    const int c = (int)(i % D);
    const long r = i / D;
    const int t = (int)(r % T);
    const int n = (int)(r / T);
    out[i] = in[(long)n * in_seq_stride + (long)c * T + t];
  }
}

extern "C" int sgic_fake2d_transpose(const float *d_in, long in_seq_stride, float *d_out, int N, int T, int D,
                                     sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out && N > 0 && T > 0 && D > 0, "args");
  fake2d_transpose_kernel<<<ew_grid((long)N * T * D), 256, 0, to_stream(stream)>>>(d_in, in_seq_stride, d_out, N, T, D);
  return sgic::check_launch("fake2d_transpose_kernel");
}

// nblocks runs of block_elems contiguous floats, run i from d_src + i*src_stride to d_dst + i*dst_stride: an exact strided
// device copy (the token rows a pruned last block keeps, out of every sequence of the residual stream).
extern "C" int sgic_copy_blocks_f32(const float *d_src, long src_stride, float *d_dst, long dst_stride, long block_elems,
                                    int nblocks, sgic_stream_t stream) {
  SGIC_REQUIRE(d_src && d_dst && block_elems > 0 && nblocks > 0, "args");
  SGIC_REQUIRE(src_stride >= block_elems && dst_stride >= block_elems, "strides");
  SGIC_HIP(hipMemcpy2DAsync(d_dst, (size_t)dst_stride * 4, d_src, (size_t)src_stride * 4, (size_t)block_elems * 4, (size_t)nblocks,
                            hipMemcpyDeviceToDevice, to_stream(stream)));
  return SGIC_OK;
}

// ------------------------------------------------------------------------------------------------
// TiTok VQ nearest code with l2-normalised tokens and codebook (titok/quantizer.py:46-61):
// d = |z|^2 + |e|^2 - 2 z.e ; argmin (first minimum).  Codes strided over lanes.
// ------------------------------------------------------------------------------------------------
// VQ_TPW tokens per workgroup, codes strided over its 256 threads: a thread normalises each of its codes ONCE and scores
// it against those tokens (their normalised vectors sit in LDS and are read as broadcasts), instead of one wave
// re-normalising the whole codebook per token in 64 latency-bound steps.  Per (token, code) the arithmetic is
// unchanged -- same normalisation, same d-order dot product, same dist = |z|^2 + |e|^2 - 2 z.e, first minimum wins
// (ties resolve to the lower code index at every reduction level) -- so the indices are identical.
#define VQ_TPW 4
__global__ __launch_bounds__(256) void vq_argmin_kernel(const float *__restrict__ z, int ldz, const float *__restrict__ cb,
                                                        int ncodes, int dim, int M, int l2norm, int *__restrict__ idx) {
  __shared__ float s_z[VQ_TPW][17];       // [token][dim (<= 16) | |z|^2]
  __shared__ float s_best[4][VQ_TPW];
  __shared__ int s_besti[4][VQ_TPW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * VQ_TPW;
  if (tid < VQ_TPW) {
    const int m = min(m0 + tid, M - 1);
    float zv[16];
    float zn = 0.f;
#pragma unroll
    for (int d = 0; d < 16; d++) {
      zv[d] = d < dim ? z[(long)m * ldz + d] : 0.f;
      if (d < dim) zn += zv[d] * zv[d];
    }
    if (l2norm) {
      const float inv = 1.0f / fmaxf(sqrtf(zn), 1e-12f);
      zn = 0.f;
#pragma unroll
      for (int d = 0; d < 16; d++) {
        zv[d] *= inv;
        if (d < dim) zn += zv[d] * zv[d];
      }
    }
#pragma unroll
    for (int d = 0; d < 16; d++) s_z[tid][d] = zv[d];
    s_z[tid][16] = zn;
  }
  __syncthreads();
  float best[VQ_TPW];
  int besti[VQ_TPW];
#pragma unroll
  for (int t = 0; t < VQ_TPW; t++) best[t] = INFINITY, besti[t] = 0x7fffffff;
  for (int c = tid; c < ncodes; c += 256) {
    float ev[16];
    float en = 0.f;
#pragma unroll
    for (int d = 0; d < 16; d++) {
      ev[d] = d < dim ? cb[(long)c * dim + d] : 0.f;
      if (d < dim) en += ev[d] * ev[d];
    }
    if (l2norm) {
      const float inv = 1.0f / fmaxf(sqrtf(en), 1e-12f);
      en = 0.f;
#pragma unroll
      for (int d = 0; d < 16; d++) {
        ev[d] *= inv;
        if (d < dim) en += ev[d] * ev[d];
      }
    }
#pragma unroll
    for (int t = 0; t < VQ_TPW; t++) {
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < 16; d++)
        if (d < dim) dot += s_z[t][d] * ev[d];
      const float dist = s_z[t][16] + en - 2.0f * dot;
      if (dist < best[t]) best[t] = dist, besti[t] = c;   // c ascends per thread: strict '<' keeps the first minimum
    }
  }
#pragma unroll
  for (int t = 0; t < VQ_TPW; t++) {
    float b = best[t];
    int bi = besti[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(b, o);
      const int oi = __shfl_xor(bi, o);
      if (ob < b || (ob == b && oi < bi)) b = ob, bi = oi;
    }
    if (lane == 0) s_best[wave][t] = b, s_besti[wave][t] = bi;
  }
  __syncthreads();
  if (tid < VQ_TPW && m0 + tid < M) {
    float b = s_best[0][tid];
    int bi = s_besti[0][tid];
    for (int w = 1; w < 4; w++) {
      const float ob = s_best[w][tid];
      const int oi = s_besti[w][tid];
      if (ob < b || (ob == b && oi < bi)) b = ob, bi = oi;
    }
    // no distance compared below +inf (a NaN / Inf token, or every distance NaN): besti is still its initial value, which is not
    // an index -- return code 0, as torch.argmin does on an all-NaN row
    idx[m0 + tid] = bi == 0x7fffffff ? 0 : bi;
  }
}

extern "C" int sgic_vq_argmin(const float *d_z, int ldz, const float *d_codebook, int ncodes, int dim, int M, int l2norm,
                              int32_t *d_idx, sgic_stream_t stream) {
  SGIC_REQUIRE(d_z && d_codebook && d_idx && M > 0 && ncodes > 0 && dim > 0 && dim <= 16 && ldz >= dim, "args");
  vq_argmin_kernel<<<cdiv(M, VQ_TPW), 256, 0, to_stream(stream)>>>(d_z, ldz, d_codebook, ncodes, dim, M, l2norm, d_idx);
  return sgic::check_launch("vq_argmin_kernel");
}

// ------------------------------------------------------------------------------------------------
// CLIP head: unit-normalise each row and u8-quantise  q = clip(rint((z*0.5+0.5)*255), 0, 255)
// (compress.py:73,77)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_u8_kernel(const float *__restrict__ x, int ldx, int M, int D,
                                                        float *__restrict__ unit, uint8_t *__restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = x[(long)m * ldx + d];
    s += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float nrm = sqrtf(s);
  for (int d = lane; d < D; d += 64) {
    const float u = x[(long)m * ldx + d] / nrm;
    unit[(long)m * D + d] = u;
    const float r = rintf((u * 0.5f + 0.5f) * 255.0f);
    q[(long)m * D + d] = (uint8_t)fminf(fmaxf(r, 0.f), 255.f);
  }
}

extern "C" int sgic_l2norm_u8(const float *d_x, int ldx, int M, int D, float *d_unit, uint8_t *d_q, sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && d_unit && d_q && M > 0 && D > 0 && ldx >= D, "args");
  l2norm_u8_kernel<<<cdiv(M, 4), 256, 0, to_stream(stream)>>>(d_x, ldx, M, D, d_unit, d_q);
  return sgic::check_launch("l2norm_u8_kernel");
}

// ------------------------------------------------------------------------------------------------
// CLIP text tower front / back ends (open_clip CLIP.encode_text, called from search.py:93-97):
//   embed:  out[b*L + l, :] = table[clamp(ids[b*L + l]), :] + pos[l, :]
//   pool :  out[b, :] = x[b*L + argmax_l ids[b, l], :]   (first maximum, like torch.argmax: the EOT token
//           has the largest id of the BPE vocabulary)
// ------------------------------------------------------------------------------------------------
__global__ void embed_tokens_kernel(const int *__restrict__ ids, const float *__restrict__ table,
                                    const float *__restrict__ pos, float *__restrict__ out, int B, int L, int D, int vocab) {
  const int D4 = D >> 2;
  const long total = (long)B * L * D4;
  GRID_STRIDE(i, total) {
    const int d4 = (int)(i % D4);
    const long r = i / D4;
    const int l = (int)(r % L);
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f32x4 a = reinterpret_cast<const f32x4 *>(table + (long)id * D)[d4];
    const f32x4 p = reinterpret_cast<const f32x4 *>(pos + (long)l * D)[d4];
    reinterpret_cast<f32x4 *>(out + r * D)[d4] = a + p;
  }
}

extern "C" int sgic_embed_tokens(const int *d_ids, const float *d_table, const float *d_pos, float *d_out, int B, int L,
                                 int D, int vocab, sgic_stream_t stream) {
  SGIC_REQUIRE(d_ids && d_table && d_pos && d_out && B > 0 && L > 0 && D > 0 && (D & 3) == 0 && vocab > 0, "args");
  const long total = (long)B * L * (D / 4);
  embed_tokens_kernel<<<ew_grid(total), 256, 0, to_stream(stream)>>>(d_ids, d_table, d_pos, d_out, B, L, D, vocab);
  return sgic::check_launch("embed_tokens_kernel");
}

__global__ __launch_bounds__(64) void gather_eot_rows_kernel(const int *__restrict__ ids, const float *__restrict__ x,
                                                              int ldx, float *__restrict__ out, int L, int D) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int best = INT_MIN, pos = 0;
  for (int l = lane; l < L; l += 64) {  // ascending l per lane => strict '>' keeps the first maximum
    const int v = ids[(long)b * L + l];
    if (v > best) { best = v; pos = l; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int ob = __shfl_xor(best, o), op = __shfl_xor(pos, o);
    if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
  }
  const float *src = x + ((long)b * L + pos) * ldx;
  for (int d = lane; d < D; d += 64) out[(long)b * D + d] = src[d];
}

extern "C" int sgic_gather_eot_rows(const int *d_ids, const float *d_x, int ldx, float *d_out, int B, int L, int D,
                                    sgic_stream_t stream) {
  SGIC_REQUIRE(d_ids && d_x && d_out && B > 0 && L > 0 && D > 0 && ldx >= D, "args");
  gather_eot_rows_kernel<<<B, 64, 0, to_stream(stream)>>>(d_ids, d_x, ldx, d_out, L, D);
  return sgic::check_launch("gather_eot_rows_kernel");
}

// ------------------------------------------------------------------------------------------------
// F.pad(x, (pl, pr, pt, pb), mode="replicate") on NCHW fp32 (compress.py:258-261: pad every image to a multiple of
// 256 on the right / bottom before the encoder).  Pure data movement: out[b,c,y,x] = in[b,c,clamp(y-pt),clamp(x-pl)].
// ------------------------------------------------------------------------------------------------
__global__ void pad_replicate_kernel(const float *__restrict__ in, float *__restrict__ out, int BC, int H, int W, int pl,
                                     int pt, int OH, int OW) {
  const long total = (long)BC * OH * OW;
  GRID_STRIDE(i, total) {
    const int ox = (int)(i % OW);
    long t = i / OW;
    const int oy = (int)(t % OH);
    const long bc = t / OH;
    const int sy = min(max(oy - pt, 0), H - 1), sx = min(max(ox - pl, 0), W - 1);
    out[i] = in[(bc * H + sy) * W + sx];
  }
}

extern "C" int sgic_pad_replicate(const float *d_in, float *d_out, int BC, int H, int W, int pl, int pr, int pt, int pb,
                                  sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out && d_in != d_out && BC > 0 && H > 0 && W > 0 && pl >= 0 && pr >= 0 && pt >= 0 && pb >= 0, "args");
  const int OH = H + pt + pb, OW = W + pl + pr;
  pad_replicate_kernel<<<ew_grid((long)BC * OH * OW), 256, 0, to_stream(stream)>>>(d_in, d_out, BC, H, W, pl, pt, OH, OW);
  return sgic::check_launch("pad_replicate_kernel");
}

// ------------------------------------------------------------------------------------------------
// Image ingest (compress.py:151-168 Test_Dataset + :258-261): decoded RGB u8 HWC (what PIL hands over, copied to the
// device as bytes -- a quarter of the fp32 PCIe traffic) -> ToTensor (x / 255) -> x * 2 - 1 -> NCHW fp32, with the
// replicate padding to a multiple of 256 fused into the same pass.  One IEEE division, one multiply, one subtract per
// sample (this file is built with -ffp-contract=off), so the result is bit-identical to
// `transforms.ToTensor()(img) * 2.0 - 1.0` followed by F.pad(mode="replicate").
// ------------------------------------------------------------------------------------------------
__global__ void u8hwc_to_f32chw_pad_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, int B, int H, int W, int pl,
                                           int pt, int OH, int OW) {
  const long total = (long)B * 3 * OH * OW;
  GRID_STRIDE(i, total) {
    const int ox = (int)(i % OW);
    long t = i / OW;
    const int oy = (int)(t % OH);
    t /= OH;
    const int c = (int)(t % 3);
    const long b = t / 3;
    const int sy = min(max(oy - pt, 0), H - 1), sx = min(max(ox - pl, 0), W - 1);
    const float v = (float)in[((b * H + sy) * W + sx) * 3 + c];
    out[i] = __fdiv_rn(v, 255.0f) * 2.0f - 1.0f;
  }
}

extern "C" int sgic_u8hwc_to_f32chw_pad(const uint8_t *d_in, float *d_out, int B, int H, int W, int pl, int pr, int pt, int pb,
                                        sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out && B > 0 && H > 0 && W > 0 && pl >= 0 && pr >= 0 && pt >= 0 && pb >= 0, "args");
  const int OH = H + pt + pb, OW = W + pl + pr;
  u8hwc_to_f32chw_pad_kernel<<<ew_grid((long)B * 3 * OH * OW), 256, 0, to_stream(stream)>>>(d_in, d_out, B, H, W, pl, pt, OH, OW);
  return sgic::check_launch("u8hwc_to_f32chw_pad_kernel");
}

// ------------------------------------------------------------------------------------------------
// Ragged batches: images of different sizes that pad to one geometry (ingest.py pad_to) share a batch.  The per-image
// geometry travels as KERNEL ARGUMENTS (host arrays, validated here, up to RAGGED_CHUNK images per launch): there is no H2D
// copy to schedule, and no extent the host has not bounds-checked reaches a kernel.
// ------------------------------------------------------------------------------------------------
#define RAGGED_CHUNK 32

struct RaggedExtents {
  int hw[RAGGED_CHUNK][2];   // (h, w) of image j of the chunk
};

// u8 canvas (B, Hc, Wc, 3) with image b at its top left, extent (h_b, w_b) -> (B, 3, OH, OW) fp32: ToTensor, *2-1 and replicate
// padding from the image's OWN right / bottom edge.  The operation order of u8hwc_to_f32chw_pad_kernel: bit-identical to it per image.
__global__ void u8canvas_to_f32chw_pad_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, RaggedExtents ext, int Hc, int Wc,
                                              int OH, int OW) {
  const int b = blockIdx.y;
  const int h = ext.hw[b][0], w = ext.hw[b][1];
  const uint8_t *src = in + (long)b * Hc * Wc * 3;
  float *dst = out + (long)b * 3 * OH * OW;
  const long total = 3L * OH * OW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OW);
    const long t = i / OW;
    const int oy = (int)(t % OH);
    const int c = (int)(t / OH);
    const int sy = min(oy, h - 1), sx = min(ox, w - 1);
    const float v = (float)src[((long)sy * Wc + sx) * 3 + c];
    dst[i] = __fdiv_rn(v, 255.0f) * 2.0f - 1.0f;
  }
}

extern "C" int sgic_u8canvas_to_f32chw_pad(const uint8_t *d_in, const int32_t *h_hw, float *d_out, int B, int Hc, int Wc, int OH, int OW,
                                           sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && h_hw && d_out && B > 0 && Hc > 0 && Wc > 0 && OH > 0 && OW > 0, "args");
  for (int b = 0; b < B; b++) {
    const int h = h_hw[2 * b], w = h_hw[2 * b + 1];
    SGIC_REQUIRE(h > 0 && w > 0 && h <= Hc && w <= Wc && h <= OH && w <= OW, "extent outside the canvas or the padded geometry");
  }
  hipStream_t st = to_stream(stream);
  const long per = 3L * OH * OW;
  const unsigned gx = (unsigned)std::min((per + 255) / 256, 2048L);
  for (int c0 = 0; c0 < B; c0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - c0);
    RaggedExtents ext{};
    for (int j = 0; j < n; j++) {
      ext.hw[j][0] = h_hw[2 * (c0 + j)];
      ext.hw[j][1] = h_hw[2 * (c0 + j) + 1];
    }
    u8canvas_to_f32chw_pad_kernel<<<dim3(gx, n), 256, 0, st>>>(d_in + (long)c0 * Hc * Wc * 3, d_out + (long)c0 * per, ext, Hc, Wc, OH, OW);
    const int rc = sgic::check_launch("u8canvas_to_f32chw_pad_kernel");
    if (rc) return rc;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// CLIP preprocessing, bit-exact with ToPILImage -> PIL bicubic(antialias) resize -> centre crop -> ToTensor -> Normalize
// (compress.py:70-71 + open_clip's image transform).  Every image of the batch has its own resize geometry (H, W, OH, OW, top, left)
// and its own Pillow bicubic tables, BUILT ON THE DEVICE in double precision in the operation order of Pillow's precompute_coeffs +
// normalize_coeffs_8bpc (clip.py pil_coeffs; this file is built with -ffp-contract=off and the divisions are correctly
// rounded), so only six ints per image leave the host.  Per chunk of RAGGED_CHUNK images:
//   tables:     bounds (first input index, count) and 22-bit fixed-point coefficients of both passes
//   horizontal: u8 -> u8 (Pillow's ImagingResampleHorizontal_8bpc) over the S columns the centre crop keeps and only the source rows
//               the vertical pass reads, bounds_v[top].xmin up to bounds_v[top + S - 1].xmin + count (both ends are non-decreasing in
//               the output index): the intermediate is 3 x rows x S u8.  The one stage that depends on where the pixels come from:
//               an fp32 image in [-1, 1] (truncated to a planar u8 copy first, as ToPILImage does) or the u8 canvas of the ingest
//   vertical:   u8 -> (v / 255 - mean) / std fp32 (3, S, S)
// The coefficient rule, the 8-bit accumulator and the LDS staging of an interleaved row are pil_resample.h's, shared with resize.hip.
// ------------------------------------------------------------------------------------------------
__global__ void pil_coeffs_kernel(int in_size, int out_size, int ksize, int *__restrict__ bounds, int *__restrict__ kk) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx < out_size) pil_coeff_row<PilBicubic>(in_size, out_size, ksize, xx, bounds, kk);
}

extern "C" int sgic_clip_resize_coeffs(int in_size, int out_size, int ksize, int32_t *d_bounds, int32_t *d_kk, sgic_stream_t stream) {
  SGIC_REQUIRE(d_bounds && d_kk && in_size > 0 && out_size > 0, "args");
  SGIC_REQUIRE(ksize == pil_ksize<PilBicubic>(in_size, out_size), "ksize");
  pil_coeffs_kernel<<<cdiv(out_size, 64), 64, 0, to_stream(stream)>>>(in_size, out_size, ksize, d_bounds, d_kk);
  return sgic::check_launch("pil_coeffs_kernel");
}

// OH, OW < 2^30: a bounds table is indexed with the int 2 * index + 1 and the table kernel counts OW + OH rows in an int; every
// other expression over OH, OW, ksize and the offsets is 64-bit or a double
#define CLIP_MAX_OUT 0x3fffffff

struct ClipImg {
  int g[8];            // H, W, OH, OW, top, left, ksize_h, ksize_v
  int rows_cap;        // rows of the intermediate: an upper bound of the row window, from the geometry alone
  int tile;            // canvas route: output columns a workgroup resamples from one LDS fill (<= U8C_THREADS)
  long long off[6];    // workspace byte offsets: bounds_h (OW x 2 int32), kk_h (OW x ksize_h), bounds_v (OH x 2), kk_v (OH x ksize_v),
                       // the planar u8 copy (3 x H x W; fp32 route only, empty on the canvas route) and the horizontal-pass
                       // output (3 x rows_cap x S)
};

struct ClipChunk {
  ClipImg img[RAGGED_CHUNK];
};

// one image's geometry (func: the entry point it is checked for) and its slice of the workspace, at byte offset *off (advanced past
// it): its four tables, its planar u8 copy if the route has one, its horizontal-pass output, each 16-byte aligned
static int clip_image(const char *func, const int32_t *q, int S, bool planar, long long *off, ClipImg *m) {
  const int H = q[0], W = q[1], OH = q[2], OW = q[3], top = q[4], left = q[5];
  SGIC_REQUIRE_AS(func, H > 0 && W > 0 && OH > 0 && OW > 0 && H <= 65535 && W <= 65535 && OH <= CLIP_MAX_OUT && OW <= CLIP_MAX_OUT,
                  "image geometry");
  SGIC_REQUIRE_AS(func, top >= 0 && left >= 0 && S <= OH && S <= OW && top <= OH - S && left <= OW - S, "crop window");
  m->g[0] = H, m->g[1] = W, m->g[2] = OH, m->g[3] = OW, m->g[4] = top, m->g[5] = left;
  m->g[6] = pil_ksize<PilBicubic>(W, OW), m->g[7] = pil_ksize<PilBicubic>(H, OH);
  m->rows_cap = (int)std::min((double)H, std::floor(u8c_span_bound(H, OH, S)) + 2.0);
  // the largest tile whose window is sure to fit one LDS fill; a window that does not fit (one output with more than U8C_TILE_PX
  // taps) is resampled in several fills
  m->tile = u8c_tile(W, OW, std::min(S, U8C_THREADS));
  const long long size[6] = {8LL * OW, 4LL * OW * m->g[6], 8LL * OH, 4LL * OH * m->g[7], planar ? 3LL * H * W : 0LL, 3LL * m->rows_cap * S};
  for (int k = 0; k < 6; k++) {
    m->off[k] = *off;
    *off += (size[k] + 15) & ~15LL;
  }
  return 0;
}

__global__ void clip_ragged_coeffs_kernel(ClipChunk ch, uint8_t *__restrict__ work) {
  const ClipImg &m = ch.img[blockIdx.y];
  const int H = m.g[0], W = m.g[1], OH = m.g[2], OW = m.g[3];
  int *bh = reinterpret_cast<int *>(work + m.off[0]), *kh = reinterpret_cast<int *>(work + m.off[1]);
  int *bv = reinterpret_cast<int *>(work + m.off[2]), *kv = reinterpret_cast<int *>(work + m.off[3]);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < OW + OH; t += (long)gridDim.x * blockDim.x) {
    if (t < OW) pil_coeff_row<PilBicubic>(W, OW, m.g[6], (int)t, bh, kh);
    else pil_coeff_row<PilBicubic>(H, OH, m.g[7], (int)t - OW, bv, kv);
  }
}

// the source rows the vertical pass reads for output rows top .. top + S - 1 (bv: its bounds table): first row *r0 -> their number
__device__ __forceinline__ int clip_row_window(const ClipImg &m, const int *__restrict__ bv, int S, int *r0) {
  const int top = m.g[4];
  *r0 = bv[2 * top];
  return min(bv[2 * (top + S - 1)] + bv[2 * (top + S - 1) + 1] - *r0, m.rows_cap);
}

__global__ void clip_ragged_to_u8_kernel(const float *__restrict__ x, long img_stride, long ch_stride, int ldx, ClipChunk ch,
                                         uint8_t *__restrict__ work) {
  const ClipImg &m = ch.img[blockIdx.y];
  const int H = m.g[0], W = m.g[1];
  const float *src = x + (long)blockIdx.y * img_stride;
  uint8_t *out = work + m.off[4];
  const long total = 3L * H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % W);
    const long t = i / W;
    const int yy = (int)(t % H);
    const int c = (int)(t / H);
    float v = src[c * ch_stride + (long)yy * ldx + xx];
    v = fminf(fmaxf(v, -1.f), 1.f);
    v = (v * 0.5f + 0.5f) * 255.f;
    out[i] = (uint8_t)v;  // .byte() truncates
  }
}

__global__ void clip_ragged_resize_h_kernel(ClipChunk ch, int S, uint8_t *__restrict__ work) {
  const ClipImg &m = ch.img[blockIdx.y];
  const int H = m.g[0], W = m.g[1], left = m.g[5], ksize = m.g[6], rows_cap = m.rows_cap;
  const int *bounds = reinterpret_cast<const int *>(work + m.off[0]), *kk = reinterpret_cast<const int *>(work + m.off[1]);
  int r0;
  const int rows = clip_row_window(m, reinterpret_cast<const int *>(work + m.off[2]), S, &r0);
  const uint8_t *in = work + m.off[4];
  uint8_t *out = work + m.off[5];
  const long total = 3L * rows_cap * S;   // i: the intermediate's own index, (c * rows_cap + r) * S + xx; rows past the window stay unwritten
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % S);
    const int t = (int)(i / S);           // < 3 * rows_cap <= 3 * 65535
    const int c = (t >= rows_cap) + (t >= 2 * rows_cap);
    const int r = t - c * rows_cap;
    if (r >= rows) continue;
    const int ox = xx + left;
    const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
    out[i] = (uint8_t)pil_resample_u8(in + ((long)c * H + r0 + r) * W + xmin, 1, kk + (long)ox * ksize, cnt);
  }
}

// the horizontal pass straight from the u8 canvas of the ingest (B, Hc, Wc, 3 interleaved RGB; image b is the top-left H_b x W_b
// region, the rest of the canvas holds stale bytes and is never read): the decoded bytes are resampled AS THEY ARE -- what
// `preprocess(Image.open(path))` does in the reference's build-images.  A workgroup takes one source row: it loads the segment of
// the row its output columns read with 16-byte loads, de-interleaves it into three planes in LDS, and every lane resamples one
// output column of the three channels from there.
__global__ __launch_bounds__(U8C_THREADS) void clip_u8canvas_resize_h_kernel(const uint8_t *__restrict__ canvas, long img_stride, int Wc,
                                                                             ClipChunk ch, int S, uint8_t *__restrict__ work) {
  __shared__ __attribute__((aligned(16))) uint8_t px[3][U8C_TILE_PX];
  const ClipImg &m = ch.img[blockIdx.y];
  const int W = m.g[1], left = m.g[5], ksize = m.g[6], tile = m.tile, rows_cap = m.rows_cap;
  const int *bh = reinterpret_cast<const int *>(work + m.off[0]), *kh = reinterpret_cast<const int *>(work + m.off[1]);
  int r0;
  const int rows = clip_row_window(m, reinterpret_cast<const int *>(work + m.off[2]), S, &r0);
  uint8_t *out = work + m.off[5];
  const uint8_t *img = canvas + (long)blockIdx.y * img_stride;
  const int tid = threadIdx.x;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const uint8_t *row = img + (long)(r0 + r) * Wc * 3;
    for (int t0 = 0; t0 < S; t0 += tile) {
      const int nt = min(tile, S - t0);
      const int last = left + t0 + nt - 1;
      const int w0 = bh[2 * (left + t0)], w1 = min(bh[2 * last] + bh[2 * last + 1], W);
      const bool active = tid < nt;
      const int ox = left + t0 + (active ? tid : 0);
      const int xmin = bh[2 * ox], xend = xmin + bh[2 * ox + 1];
      const int *k = kh + (long)ox * ksize;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;   // pil_resample_u8's accumulator, three channels per tap
      for (int c0 = w0; c0 < w1; c0 += U8C_TILE_PX) {
        const int n = min(U8C_TILE_PX, w1 - c0);
        __syncthreads();   // the previous fill has been read
        u8c_stage_row(row + 3L * c0, 3 * n, px, U8C_THREADS);
        __syncthreads();
        if (active) {
          const int lo = max(xmin, c0), hi = min(xend, c0 + n);
          for (int x = lo; x < hi; x++) {
            const int kv = k[x - xmin], i = x - c0;
            a0 += (int)px[0][i] * kv;
            a1 += (int)px[1][i] * kv;
            a2 += (int)px[2][i] * kv;
          }
        }
      }
      if (active) {
        uint8_t *o = out + (long)r * S + t0 + tid;
        o[0] = (uint8_t)pil_acc_to_u8(a0);
        o[(long)rows_cap * S] = (uint8_t)pil_acc_to_u8(a1);
        o[2L * rows_cap * S] = (uint8_t)pil_acc_to_u8(a2);
      }
    }
  }
}

// vertical pass over the row window the horizontal stage left (3 x rows_cap x S, its row 0 the source row r0) + normalise
__global__ void clip_resize_v_norm_kernel(ClipChunk ch, int S, const uint8_t *__restrict__ work, float m0, float m1, float m2, float s0,
                                          float s1, float s2, float *__restrict__ out) {
  const ClipImg &m = ch.img[blockIdx.y];
  const int top = m.g[4], ksize = m.g[7], rows_cap = m.rows_cap;
  const int *bounds = reinterpret_cast<const int *>(work + m.off[2]), *kk = reinterpret_cast<const int *>(work + m.off[3]);
  const uint8_t *in = work + m.off[5];
  const int r0 = bounds[2 * top];
  float *dst = out + (long)blockIdx.y * 3 * S * S;
  const long total = 3L * S * S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % S);
    const long t = i / S;
    const int yy = (int)(t % S);
    const int c = (int)(t / S);
    const int oy = yy + top;
    const int ymin = bounds[2 * oy] - r0, cnt = min(bounds[2 * oy + 1], rows_cap - ymin);
    const int u = pil_resample_u8(in + ((long)c * rows_cap + ymin) * S + xx, S, kk + (long)oy * ksize, cnt);
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    dst[i] = ((float)u / 255.0f - mean) / sd;
  }
}

static int clip_workspace(const char *func, int B, const int32_t *h_geo, int S, bool planar, size_t *bytes) {
  SGIC_REQUIRE_AS(func, B > 0 && h_geo && S > 0 && bytes, "args");
  long long off = 0;
  ClipImg m;
  for (int b = 0; b < B; b++) {
    const int rc = clip_image(func, h_geo + 6 * b, S, planar, &off, &m);
    if (rc) return rc;
  }
  *bytes = (size_t)off;
  return 0;
}

static unsigned clip_grid(long n) { return (unsigned)std::min((n + 255) / 256, 1024L); }

// both routes, RAGGED_CHUNK images per launch.  The route brings fits(image) -- the image lies inside its source -- and
// horizontal(chunk, first image, images, most pixels of an image, most rows_cap), which leaves the row window in the workspace
template <class Fits, class Horizontal>
static int clip_preprocess(const char *func, const char *too_small, bool planar, int B, const int32_t *h_geo, int S, const float *mean3,
                           const float *std3, uint8_t *d_work, size_t work_bytes, float *d_out, hipStream_t st, Fits fits,
                           Horizontal horizontal) {
  SGIC_REQUIRE_AS(func, (((uintptr_t)d_work) & 15) == 0, "workspace alignment");
  long long off = 0;
  for (int c0 = 0; c0 < B; c0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - c0);
    ClipChunk ch{};
    long mx_tab = 0, mx_px = 0, mx_rows = 0;
    for (int j = 0; j < n; j++) {
      ClipImg &m = ch.img[j];
      int rc = clip_image(func, h_geo + 6 * (c0 + j), S, planar, &off, &m);
      if (rc) return rc;
      SGIC_REQUIRE_AS(func, (size_t)off <= work_bytes, too_small);
      rc = fits(m);
      if (rc) return rc;
      mx_tab = std::max(mx_tab, (long)m.g[2] + m.g[3]);
      mx_px = std::max(mx_px, (long)m.g[0] * m.g[1]);
      mx_rows = std::max(mx_rows, (long)m.rows_cap);
    }
    clip_ragged_coeffs_kernel<<<dim3(cdiv((size_t)mx_tab, 64), n), 64, 0, st>>>(ch, d_work);
    int rc = sgic::check_launch("clip_ragged_coeffs_kernel");
    if (rc) return rc;
    rc = horizontal(ch, c0, n, mx_px, mx_rows);
    if (rc) return rc;
    clip_resize_v_norm_kernel<<<dim3(clip_grid(3L * S * S), n), 256, 0, st>>>(ch, S, d_work, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                                                                            std3[2], d_out + (long)c0 * 3 * S * S);
    rc = sgic::check_launch("clip_resize_v_norm_kernel");
    if (rc) return rc;
  }
  return 0;
}

extern "C" int sgic_clip_preprocess_ragged_workspace(int B, const int32_t *h_geo, int S, size_t *bytes) {
  return clip_workspace(__func__, B, h_geo, S, true, bytes);
}

extern "C" int sgic_clip_preprocess_ragged(const float *d_x, long img_stride, long ch_stride, int ldx, int B, const int32_t *h_geo, int S,
                                           const float *mean3, const float *std3, uint8_t *d_work, size_t work_bytes, float *d_out,
                                           sgic_stream_t stream) {
  SGIC_REQUIRE(d_x && h_geo && d_work && d_out && mean3 && std3 && B > 0 && S > 0, "args");
  const char *func = __func__;
  hipStream_t st = to_stream(stream);
  return clip_preprocess(
      func, "workspace too small (sgic_clip_preprocess_ragged_workspace)", true, B, h_geo, S, mean3, std3, d_work, work_bytes, d_out, st,
      [=](const ClipImg &m) -> int {
        SGIC_REQUIRE_AS(func, m.g[1] <= ldx, "image wider than the row stride");
        return 0;
      },
      [=](const ClipChunk &ch, int c0, int n, long mx_px, long mx_rows) -> int {
        clip_ragged_to_u8_kernel<<<dim3(clip_grid(3 * mx_px), n), 256, 0, st>>>(d_x + (long)c0 * img_stride, img_stride, ch_stride, ldx, ch,
                                                                               d_work);
        const int rc = sgic::check_launch("clip_ragged_to_u8_kernel");
        if (rc) return rc;
        clip_ragged_resize_h_kernel<<<dim3(clip_grid(3 * mx_rows * S), n), 256, 0, st>>>(ch, S, d_work);
        return sgic::check_launch("clip_ragged_resize_h_kernel");
      });
}

extern "C" int sgic_clip_preprocess_u8canvas_workspace(int B, const int32_t *h_geo, int S, size_t *bytes) {
  return clip_workspace(__func__, B, h_geo, S, false, bytes);
}

extern "C" int sgic_clip_preprocess_u8canvas(const uint8_t *d_canvas, int Hc, int Wc, int B, const int32_t *h_geo, int S,
                                             const float *mean3, const float *std3, uint8_t *d_work, size_t work_bytes, float *d_out,
                                             sgic_stream_t stream) {
  SGIC_REQUIRE(d_canvas && h_geo && d_work && d_out && mean3 && std3 && B > 0 && S > 0 && Hc > 0 && Wc > 0, "args");
  const char *func = __func__;
  hipStream_t st = to_stream(stream);
  const long img_stride = 3L * Hc * Wc;
  return clip_preprocess(
      func, "workspace too small (sgic_clip_preprocess_u8canvas_workspace)", false, B, h_geo, S, mean3, std3, d_work, work_bytes, d_out, st,
      [=](const ClipImg &m) -> int {
        SGIC_REQUIRE_AS(func, m.g[0] <= Hc && m.g[1] <= Wc, "extent outside the canvas");
        return 0;
      },
      [=](const ClipChunk &ch, int c0, int n, long, long mx_rows) -> int {
        clip_u8canvas_resize_h_kernel<<<dim3((unsigned)std::min(mx_rows, 2048L), n), U8C_THREADS, 0, st>>>(d_canvas + (long)c0 * img_stride,
                                                                                                         img_stride, Wc, ch, S, d_work);
        return sgic::check_launch("clip_u8canvas_resize_h_kernel");
      });
}
