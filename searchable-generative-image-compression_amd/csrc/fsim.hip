// FSIM and FSIMc of evaluate.py --fsim (include/sgic.h): the reduced Y / I / Q planes, the log-Gabor filter
// bank, phase congruency by dense fp64 DFT passes, an exact median by radix select, Scharr gradients and the pooled sums.
// Everything is fp64.  No float atomics: a workgroup writes the partial sums of its tile and a one-workgroup-per-image pass combines
// them in a fixed order, so a value does not depend on the batch or the slot an image came in.  Built with -ffp-contract=off: one
// IEEE operation per written operation (the reduced planes have to be the CPU restatement's bits, equal images have to give exactly
// 1), except the tap loops of the transform, which ask for fma by name.
#include <math.h>

#include "common.h"

namespace {

constexpr int NT = 256;                  // threads of every kernel here but the select
constexpr int TH = 16, TW = 32;          // a workgroup's tile of an output map
constexpr int MAX_GRID_Y = 32768;
constexpr int NS = 4, NO = 4;            // scales, orientations
constexpr int MAX_SIDE = 2048;           // of a transformed plane: the twiddle table of one axis lives in LDS (32 KiB)
constexpr int R = 8;                     // outputs along the transformed axis per thread of a pass
constexpr int UT = R * (NT / 64);        // outputs along that axis per workgroup (a wave owns R of them for 64 lines)
constexpr int SEL_NT = 1024;             // threads of the select
constexpr size_t CHUNK_BYTES = (size_t)512 << 20;      // planes are transformed in chunks whose scratch stays under this

bool dims_ok(int B, int H, int W) { return B >= 1 && B <= 65536 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384; }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// F = max(1, floor(min(H, W) / 256 + 0.5)); the reduced plane keeps rows and columns 0, F, 2F, ..
int reduction(int H, int W, int *h, int *w) {
  const int m = H < W ? H : W;
  int F = (int)floor((double)m / 256.0 + 0.5);
  if (F < 1) F = 1;
  *h = (H + F - 1) / F;
  *w = (W + F - 1) / F;
  return F;
}

// a fixed tree over the workgroup: the wave's lanes by shuffles, then the waves in order; thread 0 holds the sum
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) t += red[w];
  __syncthreads();
  return t;
}

// ---------------------------------------------------------------------------------------------------------------- planes

// blockIdx.x: a tile of the reduced plane, blockIdx.y: the image.  out[img][{Y, I, Q}][h][w]: the F x F mean of the unrounded
// plane over input rows i F + F / 2 - F + 1 .. i F + F / 2 (columns alike), samples outside counting 0, the taps added row by
// row from the lowest offset and the sum divided by F F.
__global__ __launch_bounds__(NT) void fsim_planes_kernel(const uint8_t *__restrict__ img, int B, int H, int W, int F, int h, int w,
                                                         int tx, double *__restrict__ out) {
  const int oy = (blockIdx.x / tx) * TH, ox = (blockIdx.x % tx) * TW;
  const int lo = F / 2 - F + 1;
  const double ff = (double)(F * F);
  for (int q = blockIdx.y; q < B; q += gridDim.y) {
    const uint8_t *src = img + (size_t)q * H * W * 3;
    double *dst = out + (size_t)q * 3 * h * w;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = threadIdx.x + k * NT;
      const int i = oy + o / TW, j = ox + o % TW;
      if (i >= h || j >= w) continue;
      double y = 0.0, ci = 0.0, cq = 0.0;
      for (int u = 0; u < F; ++u) {
        const int yy = i * F + lo + u;
        for (int v = 0; v < F; ++v) {
          const int xx = j * F + lo + v;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;      // adding 0 changes nothing
          const uint8_t *p = src + ((size_t)yy * W + xx) * 3;
          const double r = (double)p[0], g = (double)p[1], b = (double)p[2];
          y += (0.299 * r + 0.587 * g) + 0.114 * b;
          ci += (0.596 * r - 0.274 * g) - 0.322 * b;
          cq += (0.211 * r - 0.523 * g) + 0.312 * b;
        }
      }
      const size_t at = (size_t)i * w + j;
      dst[at] = y / ff;
      dst[(size_t)h * w + at] = ci / ff;
      dst[2 * (size_t)h * w + at] = cq / ff;
    }
  }
}

// One workgroup per plane: flat[plane] = (max == min).
__global__ __launch_bounds__(NT) void fsim_flat_kernel(const double *__restrict__ planes, size_t stride, size_t n, int *__restrict__ flat) {
  __shared__ double smin[NT / 64], smax[NT / 64];
  const double *p = planes + (size_t)blockIdx.x * stride;
  double lo = p[0], hi = p[0];
  for (size_t i = threadIdx.x; i < n; i += NT) {
    lo = fmin(lo, p[i]);
    hi = fmax(hi, p[i]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = fmin(lo, __shfl_down(lo, d, 64));
    hi = fmax(hi, __shfl_down(hi, d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = lo;
    smax[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NT / 64; ++k) {
      lo = fmin(lo, smin[k]);
      hi = fmax(hi, smax[k]);
    }
    flat[blockIdx.x] = hi == lo ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- filters

// the ifftshifted frequency coordinate k of an axis of length n
__device__ __forceinline__ double axis_coord(int k, int n) {
  int kk = k + n / 2;
  if (kk >= n) kk -= n;
  return (n & 1) ? ((double)kk - (double)(n - 1) / 2.0) / (double)(n - 1) : ((double)kk - (double)n / 2.0) / (double)n;
}

// lg[s][j][k]: the log-Gabor of scale s times the low-pass; sp[o][j][k]: the angular spread of orientation o
__global__ __launch_bounds__(NT) void fsim_filter_kernel(int h, int w, double *__restrict__ lg, double *__restrict__ sp) {
  const size_t hw = (size_t)h * w;
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
  if (p >= hw) return;
  const int j = (int)(p / w), k = (int)(p % w);
  const double x = axis_coord(k, w), y = axis_coord(j, h);
  double radius = sqrt(x * x + y * y);
  const double theta = atan2(-y, x);
  const double lp = 1.0 / (1.0 + pow(radius / 0.45, 30.0));
  if (p == 0) radius = 1.0;
  const double l55 = log(0.55);
  double wavelength = 6.0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double fo = 1.0 / wavelength;
    const double l = log(radius / fo);
    lg[s * hw + p] = p == 0 ? 0.0 : exp(-(l * l) / (2.0 * (l55 * l55))) * lp;
    wavelength = wavelength * 2.0;
  }
  const double st = sin(theta), ct = cos(theta);
  const double sigma = M_PI / 4.0 / 1.2;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const double angl = (double)o * M_PI / 4.0;
    const double ds = st * cos(angl) - ct * sin(angl);
    const double dc = ct * cos(angl) + st * sin(angl);
    const double dt = atan2(ds, dc);
    sp[o * hw + p] = exp(-(dt * dt) / (2.0 * (sigma * sigma)));
  }
}

// One workgroup per orientation o: fc[o] = {sum filter_{0,o}^2, S2, Sij}, the last two by Parseval from the Hermitian-symmetrised
// filters Fh_s[k] = (F_s[k] + F_s[-k]) / 2, whose inverse transforms are the real parts g_s / sqrt(h w).  Thread i takes samples
// i, i + 256, ..; then the tree.
__global__ __launch_bounds__(NT) void fsim_fstat_kernel(const double *__restrict__ lg, const double *__restrict__ sp, int h, int w,
                                                        double *__restrict__ fc) {
  __shared__ double red[NT / 64];
  const size_t hw = (size_t)h * w;
  const double *spo = sp + blockIdx.x * hw;
  double a0 = 0.0, s2 = 0.0, sij = 0.0;
  for (size_t p = threadIdx.x; p < hw; p += NT) {
    const int j = (int)(p / w), k = (int)(p % w);
    const size_t pp = (size_t)(j ? h - j : 0) * w + (k ? w - k : 0);
    const double a = spo[p], b = spo[pp];
    double f[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) f[s] = 0.5 * (lg[s * hw + p] * a + lg[s * hw + pp] * b);
    const double f0 = lg[p] * a;
    a0 += f0 * f0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      s2 += f[s] * f[s];
#pragma unroll
      for (int t = s + 1; t < NS; ++t) sij += f[s] * f[t];
    }
  }
  a0 = block_sum(a0, red);
  s2 = block_sum(s2, red);
  sij = block_sum(sij, red);
  if (threadIdx.x == 0) {
    fc[blockIdx.x * 3] = a0;
    fc[blockIdx.x * 3 + 1] = s2;
    fc[blockIdx.x * 3 + 2] = sij;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the transform

// One pass of a dense 2-D DFT along the slower axis of its input: out[x][u] = sum_t in[t][x] tw[(t u) mod n], n = nt, for nx
// independent lines x, written TRANSPOSED, so that two passes transform both axes and restore the layout.  tw[m] =
// exp(-+ 2 pi i m / n) from sincospi, in LDS; the index (t u) mod n is carried in integers (idx += u, one conditional subtraction).
// Lane = line x (coalesced loads), a wave owns R consecutive u and reads their twiddles as LDS broadcasts; the four waves of a
// workgroup share the loads through L1.  blockIdx.x: 64 lines, blockIdx.y: UT outputs, blockIdx.z: the plane (times the
// orientation for the inverse modes).
//   FWD_REAL  in: real planes (h, w), t = row -> out (w, h) complex, e^-
//   FWD_CPLX  in: that (w, h), t = column     -> out X (h, w), e^-
//   INV_FILT  in: X (h, w) times filter_{s,o} = lg[s] sp[o], four scales at once -> out U[plane][o][s] (w, h), e^+
//   INV_LAST  in: U[plane][o][s] (w, h) -> EO_s (h, w) / (h w) in registers -> the orientation's maps: energy, sumA, |EO_0|^2
enum { FWD_REAL, FWD_CPLX, INV_FILT, INV_LAST };

struct PassArgs {
  const double *in_real;      // FWD_REAL
  size_t in_stride;           // doubles between planes of in_real
  const double2 *in;          // the other modes
  const double *lg, *sp;      // INV_FILT
  double2 *out;               // but INV_LAST
  double *energy, *suma, *a2; // INV_LAST: [plane][o][h][w]
  const int *flat;            // [plane]: nothing to do
  int nt, nx;
  double inv_hw;
};

template <int MODE>
__global__ __launch_bounds__(NT) void fsim_dft_pass_kernel(PassArgs a) {
  constexpr int M = (MODE == INV_FILT || MODE == INV_LAST) ? NS : 1;      // transforms a thread carries
  constexpr bool INV = MODE == INV_FILT || MODE == INV_LAST;
  __shared__ double2 tw[MAX_SIDE];
  const int n = a.nt, nx = a.nx;
  const size_t hw = (size_t)n * nx;
  const int plane = INV ? blockIdx.z / NO : blockIdx.z;
  const int o = INV ? blockIdx.z % NO : 0;
  if (a.flat[plane]) return;
  for (int m = threadIdx.x; m < n; m += NT) {
    double s, c;
    sincospi((double)(2 * m) / (double)n, &s, &c);
    tw[m] = make_double2(c, INV ? s : -s);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int u0 = (blockIdx.y * (NT / 64) + wave) * R;
  if (u0 >= n) return;
  const int x = blockIdx.x * 64 + lane;
  const int xc = x < nx ? x : nx - 1;        // lanes past the last line load the last line and store nothing
  int idx[R], step[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    idx[i] = 0;
    step[i] = u0 + i < n ? u0 + i : n - 1;   // outputs past the axis are computed and dropped
  }
  double re[M][R], im[M][R];
#pragma unroll
  for (int s = 0; s < M; ++s)
#pragma unroll
    for (int i = 0; i < R; ++i) re[s][i] = im[s][i] = 0.0;

  const double *pr = MODE == FWD_REAL ? a.in_real + (size_t)plane * a.in_stride + xc : nullptr;
  const double2 *pc = nullptr;
  const double *plg = nullptr, *psp = nullptr;
  if (MODE == FWD_CPLX) pc = a.in + (size_t)plane * hw + xc;
  if (MODE == INV_FILT) {
    pc = a.in + (size_t)plane * hw + xc;
    plg = a.lg + xc;
    psp = a.sp + (size_t)o * hw + xc;
  }
  if (MODE == INV_LAST) pc = a.in + (size_t)blockIdx.z * NS * hw + xc;

#pragma unroll 2
  for (int t = 0; t < n; ++t) {
    const size_t at = (size_t)t * nx;
    double vr[M], vi[M];
    if (MODE == FWD_REAL) {
      vr[0] = pr[at];
      vi[0] = 0.0;
    } else if (MODE == FWD_CPLX) {
      const double2 v = pc[at];
      vr[0] = v.x;
      vi[0] = v.y;
    } else if (MODE == INV_FILT) {
      const double2 v = pc[at];
      const double so = psp[at];
#pragma unroll
      for (int s = 0; s < M; ++s) {
        const double f = plg[s * hw + at] * so;
        vr[s] = v.x * f;
        vi[s] = v.y * f;
      }
    } else {
#pragma unroll
      for (int s = 0; s < M; ++s) {
        const double2 v = pc[s * hw + at];
        vr[s] = v.x;
        vi[s] = v.y;
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const double2 wv = tw[idx[i]];
      idx[i] += step[i];
      if (idx[i] >= n) idx[i] -= n;
#pragma unroll
      for (int s = 0; s < M; ++s) {
        re[s][i] = __builtin_fma(vr[s], wv.x, re[s][i]);
        im[s][i] = __builtin_fma(vr[s], wv.y, im[s][i]);
        if (MODE != FWD_REAL) {
          re[s][i] = __builtin_fma(-vi[s], wv.y, re[s][i]);
          im[s][i] = __builtin_fma(vi[s], wv.x, im[s][i]);
        }
      }
    }
  }
  if (x >= nx) return;

  if (MODE != INV_LAST) {
    double2 *dst = a.out + (size_t)blockIdx.z * M * hw + (size_t)x * n;      // FWD: M = 1 and blockIdx.z = plane
#pragma unroll
    for (int s = 0; s < M; ++s)
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (u0 + i < n) dst[s * hw + u0 + i] = make_double2(re[s][i], im[s][i]);
  } else {
    const size_t base = (size_t)blockIdx.z * hw + (size_t)x * n;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (u0 + i >= n) break;
      double er[NS], ei[NS], sum_e = 0.0, sum_o = 0.0, sum_a = 0.0, a0 = 0.0;
#pragma unroll
      for (int s = 0; s < M; ++s) {
        er[s] = re[s][i] * a.inv_hw;
        ei[s] = im[s][i] * a.inv_hw;
        const double an = sqrt(er[s] * er[s] + ei[s] * ei[s]);
        if (s == 0) a0 = an;
        sum_e += er[s];
        sum_o += ei[s];
        sum_a += an;
      }
      const double xe = sqrt(sum_e * sum_e + sum_o * sum_o) + 1e-4;
      const double me = sum_e / xe, mo = sum_o / xe;
      double en = 0.0;
#pragma unroll
      for (int s = 0; s < M; ++s) en += (er[s] * me + ei[s] * mo) - fabs(er[s] * mo - ei[s] * me);
      a.energy[base + u0 + i] = en;
      a.suma[base + u0 + i] = sum_a;
      a.a2[base + u0 + i] = a0 * a0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the threshold

// One workgroup per (plane, orientation): the exact median of a2[0 .. n) (all >= 0, so the fp64 bit patterns order as unsigned
// integers) by a radix select, eight bits a round from the top; for an even n the second middle value comes from one more pass
// (how many values are <= the first, and the smallest above it).  Integer LDS atomics only.  Thread 0 then forms the noise
// threshold T of the orientation from the median and the filter constants fc[o] = {sum filter_{0,o}^2, S2, Sij}.
__global__ __launch_bounds__(SEL_NT) void fsim_threshold_kernel(const double *__restrict__ a2, int n, const int *__restrict__ flat,
                                                                const double *__restrict__ fc, double *__restrict__ T) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix, s_min;
  __shared__ unsigned s_k, s_cnt;
  if (flat[blockIdx.x / NO]) return;
  const unsigned long long *v = reinterpret_cast<const unsigned long long *>(a2) + (size_t)blockIdx.x * n;
  const int tid = threadIdx.x;
  const unsigned k1 = (unsigned)(n - 1) / 2;      // the median of an odd count, the lower middle of an even one
  unsigned long long prefix = 0, mask = 0;
  unsigned k = k1;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SEL_NT) {
      const unsigned long long bits = v[i];
      if ((bits & mask) == prefix) atomicAdd(&hist[(unsigned)(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0;
      int d = 0;
      while (d < 255 && k >= cum + hist[d]) cum += hist[d++];
      s_prefix = prefix | ((unsigned long long)d << shift);
      s_k = k - cum;
    }
    __syncthreads();
    prefix = s_prefix;
    k = s_k;
    mask |= 255ull << shift;
  }
  unsigned long long second = prefix;
  if ((n & 1) == 0) {
    if (tid == 0) {
      s_cnt = 0;
      s_min = ~0ull;
    }
    __syncthreads();
    unsigned cnt = 0;
    unsigned long long mn = ~0ull;
    for (int i = tid; i < n; i += SEL_NT) {
      const unsigned long long bits = v[i];
      if (bits <= prefix) ++cnt;
      else if (bits < mn) mn = bits;
    }
    atomicAdd(&s_cnt, cnt);
    atomicMin(&s_min, mn);
    __syncthreads();
    second = s_cnt >= k1 + 2 ? prefix : s_min;
  }
  if (tid == 0) {
    const double lo = __longlong_as_double((long long)prefix), hi = __longlong_as_double((long long)second);
    const double med = (n & 1) ? lo : (lo + hi) / 2.0;
    const double *c = fc + (blockIdx.x % NO) * 3;
    const double noise_power = (-med / log(0.5)) / c[0];
    const double tau = sqrt((2.0 * noise_power * c[1] + 4.0 * noise_power * c[2]) / 2.0);
    T[blockIdx.x] = (tau * sqrt(M_PI / 2.0) + 2.0 * sqrt((2.0 - M_PI / 2.0) * (tau * tau))) / 1.7;
  }
}

// PC = sum_o max(Energy_o - T_o, 0) / sum_o sumA_o, 0 where the denominator is 0 and everywhere on a flat plane.
// blockIdx.y: the plane of the chunk.
__global__ __launch_bounds__(NT) void fsim_pc_kernel(const double *__restrict__ energy, const double *__restrict__ suma,
                                                     const double *__restrict__ T, const int *__restrict__ flat, size_t hw,
                                                     double *__restrict__ pc) {
  const int plane = blockIdx.y;
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
  if (p >= hw) return;
  double v = 0.0;
  if (!flat[plane]) {
    double e = 0.0, an = 0.0;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const size_t at = ((size_t)plane * NO + o) * hw + p;
      const double d = energy[at] - T[plane * NO + o];
      e += d > 0.0 ? d : 0.0;
      an += suma[at];
    }
    v = an == 0.0 ? 0.0 : e / an;
  }
  pc[(size_t)plane * hw + p] = v;
}

// ---------------------------------------------------------------------------------------------------------------- pooling

// blockIdx.x: a tile of the reduced map, blockIdx.y: the pair.  red[q][{Y, I, Q}][h][w] and pc[q][h][w] with the originals at
// q = img and the reconstructions at q = B + img.  The tile of both Y planes and a border of one sample (zero past the plane) are
// staged in LDS for the Scharr gradients; the tile's sums of Spc Sg PCm, Spc Sg PCm C and PCm and its count of samples at which
// the two images' reduced planes differ go to part[(img * tiles + tile) * 4 + {0, 1, 2, 3}].
__global__ __launch_bounds__(NT) void fsim_pool_kernel(const double *__restrict__ red, const double *__restrict__ pc, int h, int w,
                                                       int tx, int tiles, int B, double *__restrict__ part) {
  __shared__ double sa[TH + 2][TW + 2], sb[TH + 2][TW + 2];
  __shared__ double redsum[NT / 64];
  const int tid = threadIdx.x;
  const int oy = (blockIdx.x / tx) * TH, ox = (blockIdx.x % tx) * TW;
  const size_t hw = (size_t)h * w;
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    const double *pa = red + (size_t)img * 3 * hw, *pb = red + (size_t)(B + img) * 3 * hw;
    const double *ca = pc + (size_t)img * hw, *cb = pc + (size_t)(B + img) * hw;
    for (int idx = tid; idx < (TH + 2) * (TW + 2); idx += NT) {
      const int r = idx / (TW + 2), c = idx - r * (TW + 2);
      const int i = oy + r - 1, j = ox + c - 1;
      const bool in = i >= 0 && i < h && j >= 0 && j < w;
      sa[r][c] = in ? pa[(size_t)i * w + j] : 0.0;
      sb[r][c] = in ? pb[(size_t)i * w + j] : 0.0;
    }
    __syncthreads();
    double num = 0.0, numc = 0.0, den = 0.0, diff = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      if (oy + r >= h || ox + c >= w) continue;
      // the taps row by row, the zeros of the kernels left out: dx = [[3, 0, -3], [10, 0, -10], [3, 0, -3]] / 16, dy = dx^T
      const double ax = 0.1875 * sa[r][c] + -0.1875 * sa[r][c + 2] + 0.625 * sa[r + 1][c] + -0.625 * sa[r + 1][c + 2] +
                        0.1875 * sa[r + 2][c] + -0.1875 * sa[r + 2][c + 2];
      const double ay = 0.1875 * sa[r][c] + 0.625 * sa[r][c + 1] + 0.1875 * sa[r][c + 2] + -0.1875 * sa[r + 2][c] +
                        -0.625 * sa[r + 2][c + 1] + -0.1875 * sa[r + 2][c + 2];
      const double bx = 0.1875 * sb[r][c] + -0.1875 * sb[r][c + 2] + 0.625 * sb[r + 1][c] + -0.625 * sb[r + 1][c + 2] +
                        0.1875 * sb[r + 2][c] + -0.1875 * sb[r + 2][c + 2];
      const double by = 0.1875 * sb[r][c] + 0.625 * sb[r][c + 1] + 0.1875 * sb[r][c + 2] + -0.1875 * sb[r + 2][c] +
                        -0.625 * sb[r + 2][c + 1] + -0.1875 * sb[r + 2][c + 2];
      const double g1 = sqrt(ax * ax + ay * ay), g2 = sqrt(bx * bx + by * by);
      const size_t at = (size_t)(oy + r) * w + ox + c;
      const double p1 = ca[at], p2 = cb[at];
      const double i1 = pa[hw + at], i2 = pb[hw + at], q1 = pa[2 * hw + at], q2 = pb[2 * hw + at];
      const double spc = (2.0 * p1 * p2 + 0.85) / (p1 * p1 + p2 * p2 + 0.85);
      const double sg = (2.0 * g1 * g2 + 160.0) / (g1 * g1 + g2 * g2 + 160.0);
      const double pcm = p1 > p2 ? p1 : p2;
      const double si = (2.0 * i1 * i2 + 200.0) / (i1 * i1 + i2 * i2 + 200.0);
      const double sq = (2.0 * q1 * q2 + 200.0) / (q1 * q1 + q2 * q2 + 200.0);
      const double cc = si * sq;
      double C = pow(fabs(cc), 0.03);
      if (cc < 0.0) C = C * cos(0.03 * M_PI);
      const double sl = spc * sg * pcm;
      num += sl;
      numc += sl * C;
      den += pcm;
      if (sa[r + 1][c + 1] != sb[r + 1][c + 1] || i1 != i2 || q1 != q2) diff += 1.0;
    }
    num = block_sum(num, redsum);
    numc = block_sum(numc, redsum);
    den = block_sum(den, redsum);
    diff = block_sum(diff, redsum);
    if (tid == 0) {
      double *dst = part + ((size_t)img * tiles + blockIdx.x) * 4;
      dst[0] = num;
      dst[1] = numc;
      dst[2] = den;
      dst[3] = diff;
    }
  }
}

// One workgroup per pair: the tiles' sums in a fixed order (thread i takes tiles i, i + 256, ..; then the tree) and the two
// quotients; where sum PCm is 0 (both planes flat) 1 for equal reduced planes, else 0.
__global__ __launch_bounds__(NT) void fsim_final_kernel(const double *__restrict__ part, int tiles, double *__restrict__ fsim,
                                                        double *__restrict__ fsimc) {
  __shared__ double red[NT / 64];
  const double *src = part + (size_t)blockIdx.x * tiles * 4;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < tiles; i += NT)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += src[(size_t)i * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = block_sum(v[k], red);
  if (threadIdx.x == 0) {
    const double flatv = v[3] == 0.0 ? 1.0 : 0.0;
    fsim[blockIdx.x] = v[2] == 0.0 ? flatv : v[0] / v[2];
    fsimc[blockIdx.x] = v[2] == 0.0 ? flatv : v[1] / v[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host

// the scratch of phase congruency for N planes of h x w: the filter bank and its constants once, then per plane of a chunk the
// spectrum X, the sixteen half-transformed products U (the forward pass's intermediate lives there too) and the twelve maps
struct PcPlan {
  size_t hw;
  int chunk;      // planes transformed at a time
  size_t off_lg, off_sp, off_fc, off_flat, off_T, off_X, off_U, off_maps, bytes;
};

bool make_pcplan(int N, int h, int w, PcPlan *p) {
  if (N < 1 || N > 2 * 65536 || h < 2 || w < 2 || h > MAX_SIDE || w > MAX_SIDE) return false;
  p->hw = (size_t)h * w;
  const size_t per_plane = p->hw * (16 + NO * NS * 16 + 3 * NO * 8);
  size_t chunk = CHUNK_BYTES / per_plane;
  if (chunk < 1) chunk = 1;
  if (chunk > (size_t)N) chunk = N;
  if (chunk > 8192) chunk = 8192;      // gridDim.z = chunk * NO stays under 65536
  p->chunk = (int)chunk;
  size_t at = 0;
  p->off_lg = at;
  at = align16(at + NS * p->hw * 8);
  p->off_sp = at;
  at = align16(at + NO * p->hw * 8);
  p->off_fc = at;
  at = align16(at + NO * 3 * 8);
  p->off_flat = at;
  at = align16(at + chunk * sizeof(int));
  p->off_T = at;
  at = align16(at + chunk * NO * 8);
  p->off_X = at;
  at = align16(at + chunk * p->hw * 16);
  p->off_U = at;
  at = align16(at + chunk * NO * NS * p->hw * 16);
  p->off_maps = at;
  at = align16(at + 3 * chunk * NO * p->hw * 8);
  p->bytes = at;
  return true;
}

// planes: N planes of (h, w), `stride` doubles apart -> pc (N, h, w)
void run_phasecong(const double *planes, size_t stride, int N, int h, int w, const PcPlan &p, uint8_t *work, double *pc,
                   hipStream_t st) {
  double *lg = reinterpret_cast<double *>(work + p.off_lg), *sp = reinterpret_cast<double *>(work + p.off_sp);
  double *fc = reinterpret_cast<double *>(work + p.off_fc), *T = reinterpret_cast<double *>(work + p.off_T);
  int *flat = reinterpret_cast<int *>(work + p.off_flat);
  double2 *X = reinterpret_cast<double2 *>(work + p.off_X), *U = reinterpret_cast<double2 *>(work + p.off_U);
  double *energy = reinterpret_cast<double *>(work + p.off_maps);
  const unsigned pix_blocks = (unsigned)((p.hw + NT - 1) / NT);
  fsim_filter_kernel<<<pix_blocks, NT, 0, st>>>(h, w, lg, sp);
  fsim_fstat_kernel<<<NO, NT, 0, st>>>(lg, sp, h, w, fc);
  for (int p0 = 0; p0 < N; p0 += p.chunk) {
    const int C = N - p0 < p.chunk ? N - p0 : p.chunk;
    double *suma = energy + (size_t)C * NO * p.hw, *a2 = suma + (size_t)C * NO * p.hw;
    const double *src = planes + (size_t)p0 * stride;
    fsim_flat_kernel<<<C, NT, 0, st>>>(src, stride, p.hw, flat);
    PassArgs a = {};
    a.flat = flat;
    a.lg = lg;
    a.sp = sp;
    a.inv_hw = 1.0 / (double)p.hw;
    a.energy = energy;
    a.suma = suma;
    a.a2 = a2;
    // along the rows' axis (length h, w lines), then along the columns' (length w, h lines)
    const dim3 gh((w + 63) / 64, (h + UT - 1) / UT, C), gw((h + 63) / 64, (w + UT - 1) / UT, C);
    a.in_real = src;
    a.in_stride = stride;
    a.out = U;
    a.nt = h;
    a.nx = w;
    fsim_dft_pass_kernel<FWD_REAL><<<gh, NT, 0, st>>>(a);
    a.in = U;
    a.out = X;
    a.nt = w;
    a.nx = h;
    fsim_dft_pass_kernel<FWD_CPLX><<<gw, NT, 0, st>>>(a);
    a.in = X;
    a.out = U;
    a.nt = h;
    a.nx = w;
    fsim_dft_pass_kernel<INV_FILT><<<dim3(gh.x, gh.y, C * NO), NT, 0, st>>>(a);
    a.in = U;
    a.out = nullptr;
    a.nt = w;
    a.nx = h;
    fsim_dft_pass_kernel<INV_LAST><<<dim3(gw.x, gw.y, C * NO), NT, 0, st>>>(a);
    fsim_threshold_kernel<<<C * NO, SEL_NT, 0, st>>>(a2, (int)p.hw, flat, fc, T);
    fsim_pc_kernel<<<dim3(pix_blocks, C), NT, 0, st>>>(energy, suma, T, flat, p.hw, pc + (size_t)p0 * p.hw);
  }
}

struct FsimPlan {
  int F, h, w, tx, tiles;
  PcPlan pc;
  size_t off_red, off_pc, off_part, off_work, bytes;
};

bool make_fsimplan(int B, int H, int W, FsimPlan *p) {
  if (!dims_ok(B, H, W) || H < 2 || W < 2) return false;
  p->F = reduction(H, W, &p->h, &p->w);
  if (!make_pcplan(2 * B, p->h, p->w, &p->pc)) return false;
  p->tx = (p->w + TW - 1) / TW;
  p->tiles = p->tx * ((p->h + TH - 1) / TH);
  const size_t hw = p->pc.hw;
  size_t at = 0;
  p->off_red = at;
  at = align16(at + (size_t)2 * B * 3 * hw * 8);
  p->off_pc = at;
  at = align16(at + (size_t)2 * B * hw * 8);
  p->off_part = at;
  at = align16(at + (size_t)B * p->tiles * 4 * 8);
  p->off_work = at;
  p->bytes = at + p->pc.bytes;
  return true;
}

void launch_planes(const uint8_t *img, int B, int H, int W, const FsimPlan &p, double *out, hipStream_t st) {
  dim3 grid(p.tiles, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  fsim_planes_kernel<<<grid, NT, 0, st>>>(img, B, H, W, p.F, p.h, p.w, p.tx, out);
}

}  // namespace

#define FSIM_DIMS "1 <= B <= 65536, 2 <= H, W <= 16384, the reduced longer side <= 2048"

extern "C" int sgic_fsim_planes_u8(const uint8_t *d_img, int B, int H, int W, double *d_out, sgic_stream_t stream) {
  FsimPlan p;
  SGIC_REQUIRE(make_fsimplan(B, H, W, &p), FSIM_DIMS);
  SGIC_REQUIRE(d_img && d_out, "null pointer");
  launch_planes(d_img, B, H, W, p, d_out, to_stream(stream));
  return sgic::check_launch("sgic_fsim_planes_u8");
}

extern "C" int sgic_fsim_phasecong_work_bytes(int B, int h, int w, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  PcPlan p;
  SGIC_REQUIRE(B <= 65536 && make_pcplan(B, h, w, &p), "1 <= B <= 65536, 2 <= h, w <= 2048");
  *bytes = p.bytes;
  return SGIC_OK;
}

extern "C" int sgic_fsim_phasecong(const double *d_planes, int B, int h, int w, uint8_t *d_work, size_t work_bytes, double *d_pc,
                                   sgic_stream_t stream) {
  PcPlan p;
  SGIC_REQUIRE(B <= 65536 && make_pcplan(B, h, w, &p), "1 <= B <= 65536, 2 <= h, w <= 2048");
  SGIC_REQUIRE(d_planes && d_work && d_pc, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= p.bytes, "the workspace is smaller than sgic_fsim_phasecong_work_bytes says");
  run_phasecong(d_planes, p.hw, B, h, w, p, d_work, d_pc, to_stream(stream));
  return sgic::check_launch("sgic_fsim_phasecong");
}

extern "C" int sgic_fsim_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  FsimPlan p;
  SGIC_REQUIRE(make_fsimplan(B, H, W, &p), FSIM_DIMS);
  *bytes = p.bytes;
  return SGIC_OK;
}

extern "C" int sgic_fsim(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, uint8_t *d_work, size_t work_bytes,
                         double *d_fsim, double *d_fsimc, sgic_stream_t stream) {
  FsimPlan p;
  SGIC_REQUIRE(make_fsimplan(B, H, W, &p), FSIM_DIMS);
  SGIC_REQUIRE(d_a && d_b && d_work && d_fsim && d_fsimc, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= p.bytes, "the workspace is smaller than sgic_fsim_work_bytes says");
  hipStream_t st = to_stream(stream);
  const size_t hw = p.pc.hw;
  double *red = reinterpret_cast<double *>(d_work + p.off_red), *pc = reinterpret_cast<double *>(d_work + p.off_pc);
  double *part = reinterpret_cast<double *>(d_work + p.off_part);
  launch_planes(d_a, B, H, W, p, red, st);
  launch_planes(d_b, B, H, W, p, red + (size_t)B * 3 * hw, st);
  run_phasecong(red, 3 * hw, 2 * B, p.h, p.w, p.pc, d_work + p.off_work, pc, st);
  dim3 grid(p.tiles, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  fsim_pool_kernel<<<grid, NT, 0, st>>>(red, pc, p.h, p.w, p.tx, p.tiles, B, part);
  fsim_final_kernel<<<B, NT, 0, st>>>(part, p.tiles, d_fsim, d_fsimc);
  return sgic::check_launch("sgic_fsim");
}
