// Pillow's 8-bit resampling (ImagingResample, Resample.c) restated once for its two users: the CLIP preprocessing of misc.hip and the
// image resize of resize.hip.  The coefficient rule (precompute_coeffs + normalize_coeffs_8bpc) runs on the device and on the host
// from the same text; the files that include this are built with -ffp-contract=off, and the divisions are correctly rounded on both
// sides, so every double operation is a single IEEE operation wherever it runs.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PIL_DDIV(a, b) __ddiv_rn((a), (b))
#else
#define PIL_DDIV(a, b) ((a) / (b))
#endif

// the filters: support and f(x), Pillow's bicubic_filter (a = -0.5) and lanczos_filter
struct PilBicubic {
  static constexpr double support = 2.0;
  __host__ __device__ static __forceinline__ double f(double x) {
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
  }
};

struct PilLanczos {
  static constexpr double support = 3.0;
  __host__ __device__ static __forceinline__ double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return PIL_DDIV(sin(x), x);
  }
  __host__ __device__ static __forceinline__ double f(double x) {
    if (-3.0 <= x && x < 3.0) return sinc(x) * sinc(PIL_DDIV(x, 3.0));
    return 0.0;
  }
};

// taps per table row of an in_size -> out_size resample: int(ceil(support * max(in / out, 1))) * 2 + 1 (clip.py pil_coeffs)
template <class F>
static inline int pil_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  return (int)std::ceil(F::support * (scale > 1.0 ? scale : 1.0)) * 2 + 1;
}

// Pillow's (bounds, 22-bit ints) for output index xx of an in_size -> out_size resample with filter F; the kk row is zero past its
// count, as in pil_coeffs
template <class F>
__host__ __device__ inline void pil_coeff_row(int in_size, int out_size, int ksize, int xx, int *__restrict__ bounds, int *__restrict__ kk) {
  const double scale = PIL_DDIV((double)in_size, (double)out_size);
  const double fscale = scale > 1.0 ? scale : 1.0;
  const double support = F::support * fscale;
  const double ss = PIL_DDIV(1.0, fscale);
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  xmin = xmin > 0 ? xmin : 0;
  int xmax = (int)(center + support + 0.5);
  xmax = (xmax < in_size ? xmax : in_size) - xmin;
  xmax = xmax < ksize ? xmax : ksize;
  double ww = 0.0;
  for (int x = 0; x < xmax; x++) ww += F::f(((double)(x + xmin) - center + 0.5) * ss);
  int *k = kk + (long)xx * ksize;
  for (int x = 0; x < ksize; x++) {
    int q = 0;
    if (x < xmax) {
      double v = F::f(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) v = PIL_DDIV(v, ww);
      q = v < 0.0 ? (int)(-0.5 + v * 4194304.0) : (int)(0.5 + v * 4194304.0);
    }
    k[x] = q;
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

// the tail of Pillow's 8bpc passes: the accumulator starts at half an output unit (22 fractional bits) and ends as a clamped byte
__device__ __forceinline__ int pil_acc_to_u8(int ss) {
  ss >>= 22;
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// one output sample of one channel: cnt taps p[0], p[stride], ... against the 22-bit coefficients k
__device__ __forceinline__ int pil_resample_u8(const uint8_t *__restrict__ p, long stride, const int *__restrict__ k, int cnt) {
  int ss = 1 << 21;
  for (int t = 0; t < cnt; t++) ss += (int)p[t * stride] * k[t];
  return pil_acc_to_u8(ss);
}

#define U8C_TILE_PX 4096   // horizontal pass over interleaved RGB: source pixels of a row held in LDS at a time (three planes: 12 KiB)
#define U8C_THREADS 256

// the window of n consecutive outputs of an in_size -> out_size resample spans fewer than (n - 1) * scale + 2 * support + 1 inputs
// (first index > centre_0 - support - 0.5, end <= centre_{n-1} + support + 0.5; clamping to [0, in_size] only shrinks it);
// filter_support: 2 for bicubic, 3 for Lanczos
static inline double u8c_span_bound(int in_size, int out_size, int n, double filter_support = 2.0) {
  const double scale = (double)in_size / (double)out_size;
  return (double)(n - 1) * scale + 2.0 * filter_support * (scale > 1.0 ? scale : 1.0) + 1.0;
}

// the most output columns (at most `most`) whose window is sure to fit one LDS fill; a window that does not fit (one output with more
// than U8C_TILE_PX taps) is resampled in several fills, one output per thread of which a single one is active: 1
static inline int u8c_tile(int in_size, int out_size, int most, double filter_support = 2.0) {
  const double per = (double)in_size / (double)out_size, room = (double)U8C_TILE_PX - u8c_span_bound(in_size, out_size, 1, filter_support);
  return room > 0.0 ? (int)std::min((double)most, std::floor(room / per) + 1.0) : 1;
}

// nbytes of interleaved RGB starting at a pixel boundary -> px[c][i], by the nthreads threads of the workgroup: 16-byte loads over
// the aligned middle, single bytes for the up to 15 bytes on either side, so that no byte outside [p, p + nbytes) is touched
__device__ __forceinline__ void u8c_stage_row(const uint8_t *__restrict__ p, int nbytes, uint8_t (*px)[U8C_TILE_PX], int nthreads) {
  const int head = min(nbytes, (int)((16u - (unsigned)((uintptr_t)p & 15)) & 15u));
  const int nvec = (nbytes - head) >> 4;
  const int tail0 = head + (nvec << 4);
  for (int i = threadIdx.x; i < head + nbytes - tail0; i += nthreads) {
    const int o = i < head ? i : tail0 + (i - head);
    px[o % 3][o / 3] = p[o];
  }
  for (int v = threadIdx.x; v < nvec; v += nthreads) {
    const int o = head + (v << 4);
    const uint4 q = *reinterpret_cast<const uint4 *>(p + o);
    const unsigned w4[4] = {q.x, q.y, q.z, q.w};
    int pix = o / 3, c = o - 3 * pix;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      px[c][pix] = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
      if (++c == 3) c = 0, pix++;
    }
  }
}
