// The hand-crafted full-reference measures of evaluate.py --hvs on fp64 luma planes (include/sgic.h):
// sgic_hvs_luma_u8 (Y = 0.299 R + 0.587 G + 0.114 B, unrounded), sgic_hvs_vifp (pixel-domain VIF over four scales),
// sgic_hvs_gmsd (gradient magnitude similarity deviation) and sgic_hvs_psnr (PSNR-HVS and PSNR-HVS-M over 8 x 8 DCT blocks).
// Everything is fp64.  No float atomics: a workgroup writes the partial result of its tile (block group) and a last pass combines
// the partials of one image in a fixed order, so a result does not depend on the batch an image came in.  Built with
// -ffp-contract=off: one IEEE operation per written operation (the luma has to be the CPU restatement's bits), except the tap loops
// of VIFp's filters, which ask for fma: they are most of that measure's arithmetic, and x == y still gives s1 == s2 == s12.
#include <math.h>

#include "common.h"

namespace {

constexpr int NT = 256;                  // threads of every kernel here
constexpr int TH = 16, TW = 32;          // a workgroup's tile of an output map
constexpr int MAX_GRID_Y = 32768;
constexpr int VS = 4;                    // VIFp scales
constexpr int VN_MAX = 17;               // the widest VIFp window
constexpr int BPW = 8;                   // 8 x 8 blocks a wave transforms, one after the other
constexpr int BPG = BPW * (NT / 64);     // blocks of a workgroup

bool dims_ok(int B, int H, int W) { return B >= 1 && B <= 65536 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384; }

// ---------------------------------------------------------------------------------------------------------------- luma

__global__ __launch_bounds__(NT) void hvs_luma_kernel(const uint8_t *__restrict__ img, size_t n, double *__restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const uint8_t *p = img + i * 3;
    y[i] = 0.299 * (double)p[0] + 0.587 * (double)p[1] + 0.114 * (double)p[2];
  }
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

// One workgroup per image: out[img][k] = the sum of part[img][0 .. n)[k], k < 2 (thread i takes i, i + 256, ...; then the tree).
__global__ __launch_bounds__(NT) void hvs_sum2_kernel(const double *__restrict__ part, int n, double *__restrict__ out) {
  __shared__ double red[NT / 64];
  const double *src = part + (size_t)blockIdx.x * n * 2;
  double v0 = 0.0, v1 = 0.0;
  for (int i = threadIdx.x; i < n; i += NT) {
    v0 += src[(size_t)i * 2];
    v1 += src[(size_t)i * 2 + 1];
  }
  v0 = block_sum(v0, red);
  v1 = block_sum(v1, red);
  if (threadIdx.x == 0) {
    out[(size_t)blockIdx.x * 2] = v0;
    out[(size_t)blockIdx.x * 2 + 1] = v1;
  }
}

// ---------------------------------------------------------------------------------------------------------------- VIFp

struct VWin {
  double g[VN_MAX];
};

struct VScale {
  int H, W;          // the plane of this scale
  int tx;            // tiles per row of tiles of the valid map
  int tile0, ntiles; // this scale's tiles within an image's tile list
  size_t off;        // doubles from the start of one image's pyramid to this scale's plane (scales 2..4)
};

struct VPlan {
  VScale sc[VS];
  int tiles;         // of one image over all scales
  size_t img_elems;  // doubles of one image's pyramid (scales 2..4)
  size_t part_off;   // bytes from d_work to the partial sums
  size_t bytes;
};

void make_window(int N, VWin *w) {
  const double sd = (double)N / 5.0;
  double sum = 0.0;
  for (int i = 0; i < VN_MAX; ++i) w->g[i] = 0.0;
  for (int i = 0; i < N; ++i) {
    const double d = (double)(i - N / 2);
    w->g[i] = exp(-(d * d) / (2.0 * sd * sd));
    sum += w->g[i];
  }
  for (int i = 0; i < N; ++i) w->g[i] /= sum;
}

// false when scale 4 has no valid sample (a side below 41)
bool make_vplan(int B, int H, int W, VPlan *p) {
  if (!dims_ok(B, H, W)) return false;
  int h = H, w = W, tile0 = 0;
  size_t off = 0;
  for (int s = 0; s < VS; ++s) {
    const int N = (1 << (VS - s)) + 1;       // 17, 9, 5, 3
    if (s > 0) {                             // filtered with this scale's window, every second sample kept
      if (h < N || w < N) return false;
      h = (h - N + 2) / 2;
      w = (w - N + 2) / 2;
    }
    if (h < N || w < N) return false;
    VScale &S = p->sc[s];
    S.H = h;
    S.W = w;
    S.tx = (w - N + 1 + TW - 1) / TW;
    S.ntiles = S.tx * ((h - N + 1 + TH - 1) / TH);
    S.tile0 = tile0;
    tile0 += S.ntiles;
    S.off = off;
    if (s > 0) off += (size_t)h * w;
  }
  p->tiles = tile0;
  p->img_elems = off;
  p->part_off = 2 * (size_t)B * off * sizeof(double);
  p->bytes = p->part_off + (size_t)B * tile0 * 2 * sizeof(double);
  return true;
}

// The plane of the next scale for both images: dst[i][j] = sum_u sum_v g[u] g[v] src[2 i + u][2 j + v], the valid filter kept at
// every second sample.  blockIdx.x: a tile of dst; blockIdx.y: image q of 2 B (the originals, then the reconstructions).  The row
// pass leaves the 2 (TH - 1) + N rows the tile reads in LDS, at the tile's even columns only.
template <int N>
__global__ __launch_bounds__(NT) void vif_down_kernel(const double *__restrict__ sa, const double *__restrict__ sb, size_t sstride,
                                                      int Hs, int Ws, double *__restrict__ da, double *__restrict__ db,
                                                      size_t dstride, int Hd, int Wd, int tx, int B, VWin w) {
  constexpr int RR = 2 * (TH - 1) + N;
  __shared__ double hp[RR][TW];
  const int tid = threadIdx.x;
  const int oy = (blockIdx.x / tx) * TH, ox = (blockIdx.x % tx) * TW;
  for (int q = blockIdx.y; q < 2 * B; q += gridDim.y) {
    const double *src = q < B ? sa + (size_t)q * sstride : sb + (size_t)(q - B) * sstride;
    double *dst = q < B ? da + (size_t)q * dstride : db + (size_t)(q - B) * dstride;
    for (int idx = tid; idx < RR * TW; idx += NT) {
      const int r = idx / TW, c = idx - r * TW;
      const int y = 2 * oy + r;
      double v = 0.0;
      if (y < Hs && ox + c < Wd) {       // 2 (Wd - 1) + N - 1 <= Ws - 1: the taps stay inside the row
        const double *p = src + (size_t)y * Ws + 2 * (ox + c);
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma clang fp contract(fast)
          v += w.g[i] * p[i];
        }
      }
      hp[r][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      if (oy + r < Hd && ox + c < Wd) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma clang fp contract(fast)
          v += w.g[i] * hp[2 * r + i][c];
        }
        dst[(size_t)(oy + r) * Wd + ox + c] = v;
      }
    }
    __syncthreads();
  }
}

// The two sums of one scale: blockIdx.x is a tile of the scale's valid map, blockIdx.y the image.  The row pass writes the five
// filtered moments of the tile's TH + N - 1 rows to LDS, the column pass leaves two samples per thread in registers, the clamps of
// the definition follow in its order, and the tile's sums of log10(1 + g^2 s1 / (sv + 2)) and log10(1 + s1 / 2) go to
// part[(img * tiles + tile0 + tile) * 2 + {0, 1}].
template <int N>
__global__ __launch_bounds__(NT) void vif_stats_kernel(const double *__restrict__ sa, const double *__restrict__ sb, size_t sstride,
                                                       int Hs, int Ws, int tx, int tile0, int tiles, int B,
                                                       double *__restrict__ part, VWin w) {
  constexpr int RH = TH + N - 1;
  __shared__ double hp[5][RH][TW];
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x;
  const int oy = (blockIdx.x / tx) * TH, ox = (blockIdx.x % tx) * TW;
  const int vh = Hs - N + 1, vw = Ws - N + 1;
  const double eps = 1e-10;
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    const double *pa = sa + (size_t)img * sstride, *pb = sb + (size_t)img * sstride;
    for (int idx = tid; idx < RH * TW; idx += NT) {
      const int r = idx / TW, c = idx - r * TW;
      const int y = oy + r, x = ox + c;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
      if (y < Hs && x < vw) {            // x + N - 1 <= Ws - 1
        const double *p = pa + (size_t)y * Ws + x, *q = pb + (size_t)y * Ws + x;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma clang fp contract(fast)
          const double X = p[i], Y = q[i], gi = w.g[i];
          m0 += gi * X;
          m1 += gi * Y;
          m2 += gi * (X * X);
          m3 += gi * (Y * Y);
          m4 += gi * (X * Y);
        }
      }
      hp[0][r][c] = m0;
      hp[1][r][c] = m1;
      hp[2][r][c] = m2;
      hp[3][r][c] = m3;
      hp[4][r][c] = m4;
    }
    __syncthreads();
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma clang fp contract(fast)
        const double gi = w.g[i];
        m0 += gi * hp[0][r + i][c];
        m1 += gi * hp[1][r + i][c];
        m2 += gi * hp[2][r + i][c];
        m3 += gi * hp[3][r + i][c];
        m4 += gi * hp[4][r + i][c];
      }
      double s1 = m2 - m0 * m0, s2 = m3 - m1 * m1;
      const double s12 = m4 - m0 * m1;
      if (s1 < 0.0) s1 = 0.0;
      if (s2 < 0.0) s2 = 0.0;
      double g = s12 / (s1 + eps);
      double sv = s2 - g * s12;
      if (s1 < eps) {
        g = 0.0;
        sv = s2;
        s1 = 0.0;
      }
      if (s2 < eps) {
        g = 0.0;
        sv = 0.0;
      }
      if (g < 0.0) {
        sv = s2;
        g = 0.0;
      }
      if (sv <= eps) sv = eps;
      if (oy + r < vh && ox + c < vw) {   // samples past a partial tile contribute nothing
        num += log10(1.0 + g * g * s1 / (sv + 2.0));
        den += log10(1.0 + s1 / 2.0);
      }
    }
    num = block_sum(num, red);
    den = block_sum(den, red);
    if (tid == 0) {
      double *dst = part + ((size_t)img * tiles + tile0 + blockIdx.x) * 2;
      dst[0] = num;
      dst[1] = den;
    }
  }
}

template <int N>
void launch_down(const double *sa, const double *sb, size_t sstride, const VScale &S, double *da, double *db, size_t dstride,
                 const VScale &D, int B, hipStream_t st) {
  VWin w;
  make_window(N, &w);
  const int tx = (D.W + TW - 1) / TW, ty = (D.H + TH - 1) / TH;
  dim3 grid(tx * ty, 2 * B < MAX_GRID_Y ? 2 * B : MAX_GRID_Y);
  vif_down_kernel<N><<<grid, NT, 0, st>>>(sa, sb, sstride, S.H, S.W, da, db, dstride, D.H, D.W, tx, B, w);
}

template <int N>
void launch_stats(const double *sa, const double *sb, size_t sstride, const VScale &S, int tiles, int B, double *part,
                  hipStream_t st) {
  VWin w;
  make_window(N, &w);
  dim3 grid(S.ntiles, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  vif_stats_kernel<N><<<grid, NT, 0, st>>>(sa, sb, sstride, S.H, S.W, S.tx, S.tile0, tiles, B, part, w);
}

// ---------------------------------------------------------------------------------------------------------------- GMSD

// (count, mean, sum of squared deviations) of two disjoint sets -> of their union (Chan et al.); an empty set changes nothing
__device__ __forceinline__ void merge_moments(double &n, double &mean, double &m2, double nb, double meanb, double m2b) {
  const double nn = n + nb;
  if (nb == 0.0) return;
  if (n == 0.0) {
    n = nb;
    mean = meanb;
    m2 = m2b;
    return;
  }
  const double d = meanb - mean;
  mean = mean + d * (nb / nn);
  m2 = (m2 + m2b) + d * d * (n * nb / nn);
  n = nn;
}

// blockIdx.x: a tile of the half-size map, blockIdx.y: the image.  The tile and a border of one sample of the 2 x 2 means of both
// luma planes (zero past the plane, as the zero-padded filters ask) are staged in LDS; every thread forms the Prewitt magnitudes
// and the similarity of two samples; the tile's count, mean and sum of squared deviations from ITS mean go to
// part[(img * tiles + tile) * 3 + {0, 1, 2}].
__global__ __launch_bounds__(NT) void gmsd_tile_kernel(const double *__restrict__ ya, const double *__restrict__ yb, int H, int W,
                                                       int Hd, int Wd, int tx, int tiles, int B, double *__restrict__ part) {
  __shared__ double sa[TH + 2][TW + 2], sb[TH + 2][TW + 2];
  __shared__ double red[NT / 64];
  __shared__ double tile_mean;
  const int tid = threadIdx.x;
  const int oy = (blockIdx.x / tx) * TH, ox = (blockIdx.x % tx) * TW;
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    const double *pa = ya + (size_t)img * H * W, *pb = yb + (size_t)img * H * W;
    for (int idx = tid; idx < (TH + 2) * (TW + 2); idx += NT) {
      const int r = idx / (TW + 2), c = idx - r * (TW + 2);
      const int i = oy + r - 1, j = ox + c - 1;
      double va = 0.0, vb = 0.0;
      if (i >= 0 && i < Hd && j >= 0 && j < Wd) {
        const int y = 2 * i, x = 2 * j;                     // y < H and x < W; the second row and column may lie outside
        const bool y1 = y + 1 < H, x1 = x + 1 < W;
        const size_t o = (size_t)y * W + x;
        va = 0.25 * (((pa[o] + (x1 ? pa[o + 1] : 0.0)) + (y1 ? pa[o + W] : 0.0)) + (y1 && x1 ? pa[o + W + 1] : 0.0));
        vb = 0.25 * (((pb[o] + (x1 ? pb[o + 1] : 0.0)) + (y1 ? pb[o + W] : 0.0)) + (y1 && x1 ? pb[o + W + 1] : 0.0));
      }
      sa[r][c] = va;
      sb[r][c] = vb;
    }
    __syncthreads();
    double gms[TH * TW / NT];
    double cnt = 0.0, sum = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      const double ax = ((sa[r][c + 2] - sa[r][c]) + (sa[r + 1][c + 2] - sa[r + 1][c]) + (sa[r + 2][c + 2] - sa[r + 2][c])) / 3.0;
      const double ay = ((sa[r + 2][c] - sa[r][c]) + (sa[r + 2][c + 1] - sa[r][c + 1]) + (sa[r + 2][c + 2] - sa[r][c + 2])) / 3.0;
      const double bx = ((sb[r][c + 2] - sb[r][c]) + (sb[r + 1][c + 2] - sb[r + 1][c]) + (sb[r + 2][c + 2] - sb[r + 2][c])) / 3.0;
      const double by = ((sb[r + 2][c] - sb[r][c]) + (sb[r + 2][c + 1] - sb[r][c + 1]) + (sb[r + 2][c + 2] - sb[r][c + 2])) / 3.0;
      const double m1 = sqrt(ax * ax + ay * ay), m2 = sqrt(bx * bx + by * by);
      const bool in = oy + r < Hd && ox + c < Wd;
      gms[k] = in ? (2.0 * m1 * m2 + 170.0) / ((m1 * m1 + m2 * m2) + 170.0) : 0.0;
      if (in) {
        cnt += 1.0;
        sum += gms[k];
      }
    }
    cnt = block_sum(cnt, red);
    sum = block_sum(sum, red);
    if (tid == 0) tile_mean = sum / cnt;       // every tile of the grid holds at least one sample
    __syncthreads();
    const double mean = tile_mean;
    double dev = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      if (oy + r < Hd && ox + c < Wd) dev += (gms[k] - mean) * (gms[k] - mean);
    }
    dev = block_sum(dev, red);
    if (tid == 0) {
      double *dst = part + ((size_t)img * tiles + blockIdx.x) * 3;
      dst[0] = cnt;
      dst[1] = mean;
      dst[2] = dev;
    }
    __syncthreads();
  }
}

// One workgroup per image: the tiles' moments merged in a fixed order (thread i merges tiles i, i + 256, ... in turn, the lanes of a
// wave in a shuffle tree, the waves in order) -> out[img] = sqrt(M2 / n), the population standard deviation of the map.
__global__ __launch_bounds__(NT) void gmsd_final_kernel(const double *__restrict__ part, int tiles, double *__restrict__ out) {
  __shared__ double red[NT / 64][3];
  const double *src = part + (size_t)blockIdx.x * tiles * 3;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int i = threadIdx.x; i < tiles; i += NT) merge_moments(n, mean, m2, src[(size_t)i * 3], src[(size_t)i * 3 + 1], src[(size_t)i * 3 + 2]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const double nb = __shfl_down(n, d, 64), meanb = __shfl_down(mean, d, 64), m2b = __shfl_down(m2, d, 64);
    merge_moments(n, mean, m2, nb, meanb, m2b);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = n;
    red[threadIdx.x >> 6][1] = mean;
    red[threadIdx.x >> 6][2] = m2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) merge_moments(n, mean, m2, red[w][0], red[w][1], red[w][2]);
    out[blockIdx.x] = sqrt(m2 / n);
  }
}

// ---------------------------------------------------------------------------------------------------------------- PSNR-HVS

struct HvsTables {
  double dct[64];      // dct[u * 8 + k] = c(u) cos((2 k + 1) u pi / 16), the orthonormal DCT-II matrix
  double csf[64];      // 2.5735088 (10 / Q)
  double maskcof[64];  // (10 / Q)^2
};

// sums over groups of lanes by xor butterflies: every lane of a group ends with the same bits (a + b and b + a round alike)
__device__ __forceinline__ double quad_sum(double v) {      // the 4 x 4 quadrant of lane (i, j) = (lane >> 3, lane & 7)
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  return v;
}
__device__ __forceinline__ double quads_to_block(double v) {   // from the quadrant sums to the sum over the block
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// One wave per group of BPW consecutive 8 x 8 blocks (row-major over the image's grid of whole blocks), lane (i, j) holding sample
// (i, j) of the block and then coefficient (u, v) = (i, j): both DCT passes read the other lanes' values by shuffles.  Every lane adds
// its coefficient's errors over the wave's blocks in block order, one shuffle tree adds the lanes, and the workgroup's waves are added
// in order -> part[(img * groups + group) * 2 + {hvs, hvs_m}].
__global__ __launch_bounds__(NT) void psnr_hvs_kernel(const double *__restrict__ ya, const double *__restrict__ yb, int H, int W,
                                                      int nbx, int nblocks, int groups, int B, double *__restrict__ part,
                                                      HvsTables t) {
  __shared__ double red[NT / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane >> 3, j = lane & 7;
  double ci[8], cj[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ci[k] = t.dct[i * 8 + k];
    cj[k] = t.dct[j * 8 + k];
  }
  const double csf = t.csf[lane], maskcof = t.maskcof[lane];
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    const double *pa = ya + (size_t)img * H * W, *pb = yb + (size_t)img * H * W;
    double acc = 0.0, acc_m = 0.0;
    for (int k = 0; k < BPW; ++k) {
      const int blk = (blockIdx.x * (NT / 64) + wave) * BPW + k;     // wave-uniform
      if (blk >= nblocks) break;
      const int by = blk / nbx, bx = blk - by * nbx;
      const size_t o = (size_t)(by * 8 + i) * W + bx * 8 + j;        // by * 8 + 7 < H, bx * 8 + 7 < W: whole blocks only
      const double x[2] = {pa[o], pb[o]};
      double D[2], mask = 0.0;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        double tr = 0.0, d = 0.0;
#pragma unroll
        for (int n = 0; n < 8; ++n) tr += __shfl(x[q], (lane & 56) | n, 64) * cj[n];
#pragma unroll
        for (int n = 0; n < 8; ++n) d += ci[n] * __shfl(tr, (n << 3) | j, 64);
        D[q] = d;
        const double m = quads_to_block(quad_sum(lane ? d * d * maskcof : 0.0));
        const double qs = quad_sum(x[q]);
        const double dq = x[q] - qs / 16.0, db = x[q] - quads_to_block(qs) / 64.0;
        const double vari_quads = quads_to_block(quad_sum(dq * dq) / 15.0 * 16.0);
        double pop = quads_to_block(quad_sum(db * db)) / 63.0 * 64.0;
        if (pop != 0.0) pop = vari_quads / pop;
        const double mk = sqrt(m * pop) / 32.0;
        if (mk > mask) mask = mk;
      }
      double u = fabs(D[0] - D[1]);
      const double e = (u * csf) * (u * csf);
      if (lane) {
        const double thr = mask / maskcof;
        u = u < thr ? 0.0 : u - thr;
      }
      const double e_m = (u * csf) * (u * csf);
      acc += e;            // per coefficient over the wave's blocks, in block order
      acc_m += e_m;
    }
    acc = quads_to_block(quad_sum(acc));
    acc_m = quads_to_block(quad_sum(acc_m));
    if (lane == 0) {
      red[wave][0] = acc;
      red[wave][1] = acc_m;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      double v = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) v += red[w][threadIdx.x];
      part[((size_t)img * groups + blockIdx.x) * 2 + threadIdx.x] = v;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int sgic_hvs_luma_u8(const uint8_t *d_img, int B, int H, int W, double *d_y, sgic_stream_t stream) {
  SGIC_REQUIRE(dims_ok(B, H, W), "1 <= B <= 65536, 1 <= H, W <= 16384");
  SGIC_REQUIRE(d_img && d_y, "null pointer");
  const size_t n = (size_t)B * H * W;
  const size_t blocks = (n + NT - 1) / NT;
  hvs_luma_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), NT, 0, to_stream(stream)>>>(d_img, n, d_y);
  return sgic::check_launch("sgic_hvs_luma_u8");
}

extern "C" int sgic_hvs_vifp_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  VPlan p;
  SGIC_REQUIRE(make_vplan(B, H, W, &p), "1 <= B <= 65536, 41 <= H, W <= 16384");
  *bytes = p.bytes;
  return SGIC_OK;
}

extern "C" int sgic_hvs_vifp(const double *d_ya, const double *d_yb, int B, int H, int W, uint8_t *d_work, size_t work_bytes,
                             double *d_out, sgic_stream_t stream) {
  VPlan p;
  SGIC_REQUIRE(make_vplan(B, H, W, &p), "1 <= B <= 65536, 41 <= H, W <= 16384");
  SGIC_REQUIRE(d_ya && d_yb && d_work && d_out, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= p.bytes, "the workspace is smaller than sgic_hvs_vifp_work_bytes says");
  hipStream_t st = to_stream(stream);
  double *pyr_a = reinterpret_cast<double *>(d_work), *pyr_b = pyr_a + (size_t)B * p.img_elems;
  double *part = reinterpret_cast<double *>(d_work + p.part_off);
  const size_t s0 = (size_t)H * W, s = p.img_elems;
  const VScale *S = p.sc;
  launch_stats<17>(d_ya, d_yb, s0, S[0], p.tiles, B, part, st);
  launch_down<9>(d_ya, d_yb, s0, S[0], pyr_a + S[1].off, pyr_b + S[1].off, s, S[1], B, st);
  launch_stats<9>(pyr_a + S[1].off, pyr_b + S[1].off, s, S[1], p.tiles, B, part, st);
  launch_down<5>(pyr_a + S[1].off, pyr_b + S[1].off, s, S[1], pyr_a + S[2].off, pyr_b + S[2].off, s, S[2], B, st);
  launch_stats<5>(pyr_a + S[2].off, pyr_b + S[2].off, s, S[2], p.tiles, B, part, st);
  launch_down<3>(pyr_a + S[2].off, pyr_b + S[2].off, s, S[2], pyr_a + S[3].off, pyr_b + S[3].off, s, S[3], B, st);
  launch_stats<3>(pyr_a + S[3].off, pyr_b + S[3].off, s, S[3], p.tiles, B, part, st);
  hvs_sum2_kernel<<<B, NT, 0, st>>>(part, p.tiles, d_out);
  return sgic::check_launch("sgic_hvs_vifp");
}

extern "C" int sgic_hvs_gmsd_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  SGIC_REQUIRE(dims_ok(B, H, W), "1 <= B <= 65536, 1 <= H, W <= 16384");
  const int Hd = (H + 1) / 2, Wd = (W + 1) / 2;
  *bytes = (size_t)B * ((Wd + TW - 1) / TW) * ((Hd + TH - 1) / TH) * 3 * sizeof(double);
  return SGIC_OK;
}

extern "C" int sgic_hvs_gmsd(const double *d_ya, const double *d_yb, int B, int H, int W, uint8_t *d_work, size_t work_bytes,
                             double *d_out, sgic_stream_t stream) {
  SGIC_REQUIRE(dims_ok(B, H, W), "1 <= B <= 65536, 1 <= H, W <= 16384");
  SGIC_REQUIRE(d_ya && d_yb && d_work && d_out, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  const int Hd = (H + 1) / 2, Wd = (W + 1) / 2;
  const int tx = (Wd + TW - 1) / TW, tiles = tx * ((Hd + TH - 1) / TH);
  SGIC_REQUIRE(work_bytes >= (size_t)B * tiles * 3 * sizeof(double), "the workspace is smaller than sgic_hvs_gmsd_work_bytes says");
  hipStream_t st = to_stream(stream);
  double *part = reinterpret_cast<double *>(d_work);
  dim3 grid(tiles, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  gmsd_tile_kernel<<<grid, NT, 0, st>>>(d_ya, d_yb, H, W, Hd, Wd, tx, tiles, B, part);
  gmsd_final_kernel<<<B, NT, 0, st>>>(part, tiles, d_out);
  return sgic::check_launch("sgic_hvs_gmsd");
}

extern "C" int sgic_hvs_psnr_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  SGIC_REQUIRE(dims_ok(B, H, W) && H >= 8 && W >= 8, "1 <= B <= 65536, 8 <= H, W <= 16384");
  const int nblocks = (H / 8) * (W / 8);
  *bytes = (size_t)B * ((nblocks + BPG - 1) / BPG) * 2 * sizeof(double);
  return SGIC_OK;
}

extern "C" int sgic_hvs_psnr(const double *d_ya, const double *d_yb, int B, int H, int W, const int *h_q, uint8_t *d_work,
                             size_t work_bytes, double *d_out, sgic_stream_t stream) {
  SGIC_REQUIRE(dims_ok(B, H, W) && H >= 8 && W >= 8, "1 <= B <= 65536, 8 <= H, W <= 16384");
  SGIC_REQUIRE(d_ya && d_yb && h_q && d_work && d_out, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  const int nbx = W / 8, nblocks = (H / 8) * nbx, groups = (nblocks + BPG - 1) / BPG;
  SGIC_REQUIRE(work_bytes >= (size_t)B * groups * 2 * sizeof(double), "the workspace is smaller than sgic_hvs_psnr_work_bytes says");
  HvsTables t;
  for (int k = 0; k < 64; ++k) {
    SGIC_REQUIRE(h_q[k] >= 1 && h_q[k] <= 255, "a quantisation step outside 1..255");
    const double r = 10.0 / (double)h_q[k];
    t.csf[k] = 2.5735088 * r;
    t.maskcof[k] = r * r;
    const int u = k >> 3, n = k & 7;
    t.dct[k] = (u == 0 ? sqrt(0.125) : 0.5) * cos((double)((2 * n + 1) * u) * M_PI / 16.0);
  }
  hipStream_t st = to_stream(stream);
  double *part = reinterpret_cast<double *>(d_work);
  dim3 grid(groups, B < MAX_GRID_Y ? B : MAX_GRID_Y);
  psnr_hvs_kernel<<<grid, NT, 0, st>>>(d_ya, d_yb, H, W, nbx, nblocks, groups, B, part, t);
  hvs_sum2_kernel<<<B, NT, 0, st>>>(part, groups, d_out);
  return sgic::check_launch("sgic_hvs_psnr");
}
