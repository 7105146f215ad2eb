// The block sums of NIQE for a batch of u8 images (sgic_niqe_u8, include/sgic.h).  Everything up to the local
// mean and variance is integers: the BT.601 luma with round-half-even, the half-size plane of MATLAB's imresize (numerators over
// 65536), and per pixel the ten class sums of (x - centre) and (x - centre)^2 over the 7 x 7 window.  The sign of an MSCN sample is
// the sign of ten products of a window weight with an exact integer, added in a fixed order: the same on any IEEE machine, exactly
// 0 where the neighbourhood is flat or antisymmetric.  A workgroup owns one 96 x 96 (48 x 48) block: it keeps the block's MSCN map
// in LDS, because the four product maps pair every sample with a circularly shifted one of the same block, and reduces the five
// maps in a fixed order (wave shuffles, then the waves in order).  No float atomics: two runs give the same bits.  Built with
// -ffp-contract=off: one IEEE operation per written operation.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

constexpr int BS = 96;                   // block side at scale 1
constexpr int HALO = 3;
constexpr int NT = 512;                  // threads of the block kernel
constexpr int LT = 256;                  // threads of the luma kernel
constexpr int LTILE = 32;                // its tile of the cropped luma plane (16 x 16 half-size outputs); divides 96
constexpr int LREG = LTILE + 6;          // with the three samples the eight taps reach to either side
constexpr int MAX_GRID_Y = 32768;
constexpr int NSTAT = 25;                // five maps x {cnt_neg, cnt_pos, ssq_neg, ssq_pos, sabs}

struct NiqeWeights {
  double w[10];
};

struct NiqePlan {
  int nbh, nbw, Hc, Wc;
  size_t half_off, bytes;
};

bool make_plan(int B, int H, int W, NiqePlan *p) {
  if (B < 1 || B > 65536 || H < BS || W < BS || H > 16384 || W > 16384) return false;
  p->nbh = H / BS;
  p->nbw = W / BS;
  p->Hc = p->nbh * BS;
  p->Wc = p->nbw * BS;
  const size_t luma = (size_t)B * p->Hc * p->Wc;
  p->half_off = (luma + 15) & ~(size_t)15;
  p->bytes = p->half_off + (luma / 4) * sizeof(int32_t);
  return true;
}

// symmetric extension of imresize: -1 -> 0, -2 -> 1, n -> n - 1, n + 1 -> n - 2 (|overhang| <= 3 < n)
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// u8 RGB -> the cropped luma plane (u8) and the half-size numerators (int32) in one pass.  A workgroup owns a 32 x 32 tile of the
// cropped plane: it forms the luma of the 38 x 38 region its 16 x 16 outputs read (mirrored at the cropped plane's edges, so every
// load lies inside the crop), writes the interior, runs the eight taps along the rows into LDS and then along the columns.
__global__ __launch_bounds__(LT) void niqe_luma_half_kernel(const uint8_t *__restrict__ img, int B, int H, int W, int Hc, int Wc,
                                                            uint8_t *__restrict__ luma, int32_t *__restrict__ half) {
  __shared__ uint8_t sy[LREG][LREG + 2];
  __shared__ int32_t sh[LREG][LTILE / 2];
  const int tid = threadIdx.x;
  const int tx = Wc / LTILE;
  const int oy = (blockIdx.x / tx) * LTILE, ox = (blockIdx.x % tx) * LTILE;
  const int taps[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    for (int idx = tid; idx < LREG * LREG; idx += LT) {
      const int r = idx / LREG, c = idx - r * LREG;
      const int y = mirror(oy + r - HALO, Hc), x = mirror(ox + c - HALO, Wc);
      const uint8_t *px = img + (((size_t)b * H + y) * W + x) * 3;
      const int n = 65481 * (int)px[0] + 128553 * (int)px[1] + 24966 * (int)px[2];      // <= 255 * 219000
      int q = n / 255000;
      const int rem = n - q * 255000;
      q += (2 * rem > 255000 || (2 * rem == 255000 && (q & 1))) ? 1 : 0;                // round half to even
      const uint8_t v = (uint8_t)(16 + q);
      sy[r][c] = v;
      if (r >= HALO && r < HALO + LTILE && c >= HALO && c < HALO + LTILE)
        luma[((size_t)b * Hc + (oy + r - HALO)) * Wc + (ox + c - HALO)] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < LREG * (LTILE / 2); idx += LT) {
      const int r = idx / (LTILE / 2), j = idx - r * (LTILE / 2);
      int acc = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += taps[k] * (int)sy[r][2 * j + k];               // input 2 j - 3 + k is column 2 j + k of the region
      sh[r][j] = acc;
    }
    __syncthreads();
    {
      const int i = tid / (LTILE / 2), j = tid - i * (LTILE / 2);                       // 256 threads, 16 x 16 outputs
      int acc = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += taps[k] * sh[2 * i + k][j];                    // |.| <= 235 * 304 * 304 < 2^25
      half[((size_t)b * (Hc / 2) + (oy / 2 + i)) * (Wc / 2) + (ox / 2 + j)] = acc;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// One workgroup per block of S x S samples of one scale's integer plane (T = u8: the luma, values x; T = int32: the half-size
// numerators, values x 2^-16).  Q holds a class's sum of squares: 8 x 255^2 fits int32, 8 x (2.1e7)^2 < 2^52 needs int64 and is
// exact as a double.  stats: (B, nbh, nbw, 2, 5, 5) doubles, this launch writes scale `scale`; sharp: (B, nbh, nbw), scale 0 only.
template <int S, typename T>
__global__ __launch_bounds__(NT) void niqe_block_kernel(const T *__restrict__ plane, int B, int nbh, int nbw, int scale,
                                                        double unit, NiqeWeights wt, double *__restrict__ stats,
                                                        double *__restrict__ sharp) {
  using Q = typename std::conditional<std::is_same<T, uint8_t>::value, int, long long>::type;
  constexpr int R = S + 2 * HALO;
  constexpr int RP = std::is_same<T, uint8_t>::value ? ((R + 3) & ~3) : R;
  // dynamic LDS (the 96 x 96 doubles are beyond the 64 KiB a kernel gets without asking): the MSCN block, the waves' sums, the plane
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double(*sn)[S] = reinterpret_cast<double(*)[S]>(smem);
  double(*red)[NSTAT + 1] = reinterpret_cast<double(*)[NSTAT + 1]>(smem + sizeof(double) * S * S);
  T(*sx)[RP] = reinterpret_cast<T(*)[RP]>(smem + sizeof(double) * (S * S + (NT / 64) * (NSTAT + 1)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ih = blockIdx.x / nbw, iw = blockIdx.x - ih * nbw;
  const int Hp = nbh * S, Wp = nbw * S;
  const double unit2 = unit * unit;

  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    // the block and three samples around it, replicated past the plane's edges: every index is clamped into the plane
    const T *src = plane + (size_t)b * Hp * Wp;
    for (int idx = tid; idx < R * R; idx += NT) {
      const int r = idx / R, c = idx - r * R;
      int y = ih * S + r - HALO, x = iw * S + c - HALO;
      y = y < 0 ? 0 : (y >= Hp ? Hp - 1 : y);
      x = x < 0 ? 0 : (x >= Wp ? Wp - 1 : x);
      sx[r][c] = src[(size_t)y * Wp + x];
    }
    __syncthreads();
    double sig_sum = 0.0;
    for (int idx = tid; idx < S * S; idx += NT) {
      const int i = idx / S, j = idx - i * S;
      const int c = (int)sx[i + HALO][j + HALO];
      int s[10];
      Q q[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        s[k] = 0;
        q[k] = 0;
      }
#pragma unroll
      for (int di = -3; di <= 3; ++di)
#pragma unroll
        for (int dj = -3; dj <= 3; ++dj) {
          const int ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj;
          const int a = ai < aj ? ai : aj, bb = ai < aj ? aj : ai;
          const int k = a * 4 - a * (a - 1) / 2 + (bb - a);        // (0,0) (0,1) .. (3,3) in ascending order
          const int d = (int)sx[i + HALO + di][j + HALO + dj] - c;
          s[k] += d;
          q[k] += (Q)d * (Q)d;
        }
      double m = 0.0, v = 0.0;
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        m += wt.w[k] * ((double)s[k] * unit);
        v += wt.w[k] * ((double)q[k] * unit2);
      }
      const double sigma = sqrt(fabs(v - m * m));
      sn[i][j] = (0.0 - m) / (sigma + 1.0);
      sig_sum += sigma;
    }
    __syncthreads();
    int cneg[5] = {0, 0, 0, 0, 0}, cpos[5] = {0, 0, 0, 0, 0};
    double qneg[5] = {0, 0, 0, 0, 0}, qpos[5] = {0, 0, 0, 0, 0}, sabs[5] = {0, 0, 0, 0, 0};
    for (int idx = tid; idx < S * S; idx += NT) {
      const int i = idx / S, j = idx - i * S;
      const int iu = i == 0 ? S - 1 : i - 1, jl = j == 0 ? S - 1 : j - 1, jr = j == S - 1 ? 0 : j + 1;
      const double n = sn[i][j];
      // np.roll(n, (si, sj))[i][j] = n[i - si][j - sj], circular inside the block: shifts (0,1), (1,0), (1,1), (1,-1)
      const double val[5] = {n, n * sn[i][jl], n * sn[iu][j], n * sn[iu][jl], n * sn[iu][jr]};
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double x = val[k], xx = x * x;
        if (x < 0.0) {
          cneg[k] += 1;
          qneg[k] += xx;
        } else if (x > 0.0) {
          cpos[k] += 1;
          qpos[k] += xx;
        }
        sabs[k] += fabs(x);
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int cn = wave_sum(cneg[k]), cp = wave_sum(cpos[k]);
      const double qn = wave_sum(qneg[k]), qp = wave_sum(qpos[k]), sa = wave_sum(sabs[k]);
      if (lane == 0) {
        red[wave][k * 5 + 0] = (double)cn;
        red[wave][k * 5 + 1] = (double)cp;
        red[wave][k * 5 + 2] = qn;
        red[wave][k * 5 + 3] = qp;
        red[wave][k * 5 + 4] = sa;
      }
    }
    sig_sum = wave_sum(sig_sum);
    if (lane == 0) red[wave][NSTAT] = sig_sum;
    __syncthreads();
    if (tid < NSTAT + 1) {
      double t = red[0][tid];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) t += red[w][tid];
      const size_t blk = ((size_t)b * nbh + ih) * nbw + iw;
      if (tid < NSTAT)
        stats[(blk * 2 + scale) * NSTAT + tid] = t;
      else if (scale == 0)
        sharp[blk] = t / (double)(S * S);
    }
    __syncthreads();
  }
}

template <int S, typename T>
constexpr size_t block_lds() {
  constexpr int R = S + 2 * HALO;
  constexpr int RP = std::is_same<T, uint8_t>::value ? ((R + 3) & ~3) : R;
  return sizeof(double) * (S * S + (NT / 64) * (NSTAT + 1)) + sizeof(T) * R * RP;
}

template <int S, typename T>
int launch_blocks(const T *plane, int B, const NiqePlan &p, int scale, double unit, const NiqeWeights &wt, double *stats,
                  double *sharp, hipStream_t st) {
  constexpr size_t lds = block_lds<S, T>();
  static_assert(lds <= 128 * 1024, "one workgroup's LDS");
  static bool lds_raised = false;   // beyond the default 64 KiB a kernel has to be allowed its dynamic LDS once
  if (lds > 60 * 1024 && !lds_raised) {
    SGIC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(niqe_block_kernel<S, T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 128 * 1024));
    lds_raised = true;
  }
  dim3 grid(p.nbh * p.nbw, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  niqe_block_kernel<S, T><<<grid, NT, lds, st>>>(plane, B, p.nbh, p.nbw, scale, unit, wt, stats, sharp);
  return sgic::check_launch("sgic_niqe_u8");
}

}  // namespace

extern "C" int sgic_niqe_u8_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  NiqePlan p;
  SGIC_REQUIRE(make_plan(B, H, W, &p), "1 <= B <= 65536, 96 <= H, W <= 16384");
  *bytes = p.bytes;
  return SGIC_OK;
}

extern "C" int sgic_niqe_u8(const uint8_t *d_img, int B, int H, int W, const double *h_weights, uint8_t *d_work, size_t work_bytes,
                            double *d_stats, double *d_sharp, sgic_stream_t stream) {
  NiqePlan p;
  SGIC_REQUIRE(make_plan(B, H, W, &p), "1 <= B <= 65536, 96 <= H, W <= 16384");
  SGIC_REQUIRE(d_img && h_weights && d_work && d_stats && d_sharp, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= p.bytes, "the workspace is smaller than sgic_niqe_u8_work_bytes says");
  NiqeWeights wt;
  for (int k = 0; k < 10; ++k) {
    SGIC_REQUIRE(h_weights[k] > 0.0 && h_weights[k] < 1.0, "the ten class weights lie in (0, 1)");
    wt.w[k] = h_weights[k];
  }
  hipStream_t st = to_stream(stream);
  uint8_t *luma = d_work;
  int32_t *half = reinterpret_cast<int32_t *>(d_work + p.half_off);
  const int gy = B < MAX_GRID_Y ? B : MAX_GRID_Y;
  {
    dim3 grid((p.Hc / LTILE) * (p.Wc / LTILE), gy);
    niqe_luma_half_kernel<<<grid, LT, 0, st>>>(d_img, B, H, W, p.Hc, p.Wc, luma, half);
  }
  const int rc = launch_blocks<BS, uint8_t>(luma, B, p, 0, 1.0, wt, d_stats, d_sharp, st);
  if (rc != SGIC_OK) return rc;
  return launch_blocks<BS / 2, int32_t>(half, B, p, 1, 1.0 / 65536.0, wt, d_stats, d_sharp, st);
}
