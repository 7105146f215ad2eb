// Rate-distortion measurement of a batch of u8 image pairs (sgic_quality_u8, include/sgic.h): the exact integer squared error per
// image and channel, and the ssim / cs means of the five MS-SSIM levels (pytorch_msssim.ms_ssim, data_range 1, 11-tap Gaussian of
// sigma 1.5) in fp64.  The pyramid is integers: level s + 1 is the 2 x 2 SUM of level s (u16 numerators over 255 * 4^s), so the five
// moments X, Y, XX, YY, XY of a level are exact integers and the only rounding is in the two filter passes and the ssim / cs maps.
// No float atomics: a workgroup writes the partial sums of its tile and a last pass adds them in a fixed order, so two runs on the
// same input give the same bits.  Built with -ffp-contract=off: one IEEE operation per written operation.
#include <math.h>

#include "common.h"

namespace {

constexpr int QL = 5;                    // levels
constexpr int QT = 11;                   // filter taps
constexpr int TH = 16, TW = 32;          // a workgroup's tile of the valid-filter output
constexpr int RH = TH + QT - 1, RW = TW + QT - 1;   // its input region
constexpr int NT = 256;                  // threads of every kernel here
constexpr int MAX_GRID_Y = 32768;

struct QLevel {
  int H, W;          // the plane
  int tx;            // tiles per row of tiles
  int tile0, ntiles; // this level's tiles within a plane's tile list
  size_t off;        // u16 elements from the start of one image's pyramid to this level (levels 1..4)
  double inv;        // 1 / (255 * 4^s)
};

struct QPlan {
  QLevel lv[QL];
  double g[QT];
  int B, tiles;      // tiles: of one plane over all levels
  size_t img_elems;  // u16 elements of one image's pyramid (levels 1..4, all planes), a multiple of 8
  size_t part_off;   // bytes from d_work to the partial sums
  size_t bytes;
};

bool make_plan(int B, int H, int W, QPlan *p) {
  if (B < 1 || B > 65536 || H <= 160 || W <= 160 || H > 16384 || W > 16384) return false;
  int h = H, w = W, tile0 = 0;
  size_t off = 0;
  double scale = 255.0;
  for (int s = 0; s < QL; ++s) {
    QLevel &L = p->lv[s];
    L.H = h;
    L.W = w;
    L.tx = (w - (QT - 1) + TW - 1) / TW;
    L.ntiles = L.tx * ((h - (QT - 1) + TH - 1) / TH);
    L.tile0 = tile0;
    tile0 += L.ntiles;
    L.off = off;
    if (s > 0) off += (size_t)3 * B * h * w;
    L.inv = 1.0 / scale;
    scale *= 4.0;
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  double sum = 0.0;
  for (int i = 0; i < QT; ++i) {
    p->g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5);
    sum += p->g[i];
  }
  for (int i = 0; i < QT; ++i) p->g[i] /= sum;
  p->B = B;
  p->tiles = tile0;
  p->img_elems = (off + 7) & ~(size_t)7;
  p->part_off = 2 * p->img_elems * sizeof(uint16_t);
  p->bytes = p->part_off + (size_t)3 * B * tile0 * 2 * sizeof(double);
  return true;
}

// Level 1 of both pyramids from the u8 images, and the squared error: every level-0 sample lies in exactly one 2 x 2 cell (the cells
// start at -(H % 2), -(W % 2)), so the pass that pools also sees every sample once.  One thread per cell, all three channels.
__global__ __launch_bounds__(NT) void quality_pool0_sse_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int B,
                                                               int H, int W, int H1, int W1, uint16_t *__restrict__ pa,
                                                               uint16_t *__restrict__ pb, unsigned long long *__restrict__ sse) {
  __shared__ unsigned red[NT / 64][3];
  const int cell = blockIdx.x * NT + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    unsigned e[3] = {0, 0, 0};
    if (cell < H1 * W1) {
      const int i = cell / W1, j = cell - i * W1;
      const int y0 = 2 * i - (H & 1), x0 = 2 * j - (W & 1);
      unsigned na[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int y = y0 + dy, x = x0 + dx;
          if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t o = (((size_t)img * H + y) * W + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int va = a[o + c], vb = b[o + c];
              na[c] += va;
              nb[c] += vb;
              e[c] += (unsigned)((va - vb) * (va - vb));
            }
          }
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t o = (((size_t)img * 3 + c) * H1 + i) * W1 + j;
        pa[o] = (uint16_t)na[c];
        pb[o] = (uint16_t)nb[c];
      }
    }
    // <= 4 * 255^2 per thread, so a workgroup's sum fits 32 bits
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) e[c] += (unsigned)__shfl_down((int)e[c], d, 64);
      if (lane == 0) red[wave][c] = e[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      unsigned t = 0;
#pragma unroll
      for (int v = 0; v < NT / 64; ++v) t += red[v][threadIdx.x];
      if (t) atomicAdd(&sse[(size_t)img * 3 + threadIdx.x], (unsigned long long)t);
    }
    __syncthreads();
  }
}

// Level s + 1 from level s (s >= 1) for the planes of both images: u16 numerators, 2 x 2 sums, cells outside the plane count 0.
__global__ __launch_bounds__(NT) void quality_pool_kernel(uint16_t *__restrict__ pyr, size_t img_elems, size_t off_src, size_t off_dst,
                                                          int planes, int Hs, int Ws, int Hd, int Wd) {
  const int cell = blockIdx.x * NT + threadIdx.x;
  if (cell >= Hd * Wd) return;
  const int i = cell / Wd, j = cell - i * Wd;
  const int y0 = 2 * i - (Hs & 1), x0 = 2 * j - (Ws & 1);
  for (int q = blockIdx.y; q < 2 * planes; q += gridDim.y) {
    const size_t base = (q >= planes ? img_elems : 0);
    const int pl = q >= planes ? q - planes : q;
    const uint16_t *src = pyr + base + off_src + (size_t)pl * Hs * Ws;
    unsigned n = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int y = y0 + dy, x = x0 + dx;
        if (y >= 0 && y < Hs && x >= 0 && x < Ws) n += src[(size_t)y * Ws + x];
      }
    pyr[base + off_dst + ((size_t)pl * Hd + i) * Wd + j] = (uint16_t)n;
  }
}

// All five levels of all planes in one launch: blockIdx.x is a tile of a plane's tile list (level 0 first), blockIdx.y the plane
// (image b, channel c).  The tile's input region of both images is staged in LDS as integers (zero past the plane's edges), the
// horizontal pass writes the five filtered moments of its 26 rows to LDS in fp64, the vertical pass leaves two output samples per
// thread in registers, and the tile's sums of ssim and cs go to part[(plane * tiles + tile) * 2 + {0, 1}].
__global__ __launch_bounds__(NT) void quality_level_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                           const uint16_t *__restrict__ pyr, double *__restrict__ part, QPlan p) {
  __shared__ uint16_t sx[RH][RW], sy[RH][RW];
  __shared__ double hp[5][RH][TW];
  __shared__ double red[NT / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  // the level of this tile: static indices only, so that the by-value plan stays in scalar registers
  int s = 0, Hs = p.lv[0].H, Ws = p.lv[0].W, tx = p.lv[0].tx, tile0 = 0;
  size_t off = 0;
  double inv = p.lv[0].inv;
#pragma unroll
  for (int k = 1; k < QL; ++k)
    if (tile >= p.lv[k].tile0) {
      s = k; Hs = p.lv[k].H; Ws = p.lv[k].W; tx = p.lv[k].tx; tile0 = p.lv[k].tile0; off = p.lv[k].off; inv = p.lv[k].inv;
    }
  const int t = tile - tile0;
  const int oy = (t / tx) * TH, ox = (t % tx) * TW;
  const int vh = Hs - (QT - 1), vw = Ws - (QT - 1);      // the valid map
  const double inv2 = inv * inv;
  const int H0 = p.lv[0].H, W0 = p.lv[0].W;

  for (int plane = blockIdx.y; plane < 3 * p.B; plane += gridDim.y) {
    for (int idx = tid; idx < RH * RW; idx += NT) {
      const int r = idx / RW, c = idx - r * RW;
      const int y = oy + r, x = ox + c;
      uint16_t va = 0, vb = 0;
      if (y < Hs && x < Ws) {
        if (s == 0) {
          const int img = plane / 3, ch = plane - img * 3;
          const size_t o = (((size_t)img * H0 + y) * W0 + x) * 3 + ch;
          va = a[o];
          vb = b[o];
        } else {
          const size_t o = off + ((size_t)plane * Hs + y) * Ws + x;
          va = pyr[o];
          vb = pyr[p.img_elems + o];
        }
      }
      sx[r][c] = va;
      sy[r][c] = vb;
    }
    __syncthreads();
    for (int idx = tid; idx < RH * TW; idx += NT) {
      const int r = idx / TW, c = idx - r * TW;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const unsigned X = sx[r][c + i], Y = sy[r][c + i];   // < 2^16: the products fit 32 bits and are exact in fp64
        const double gi = p.g[i];
        m0 += gi * (double)X;
        m1 += gi * (double)Y;
        m2 += gi * (double)(X * X);
        m3 += gi * (double)(Y * Y);
        m4 += gi * (double)(X * Y);
      }
      hp[0][r][c] = m0;
      hp[1][r][c] = m1;
      hp[2][r][c] = m2;
      hp[3][r][c] = m3;
      hp[4][r][c] = m4;
    }
    __syncthreads();
    double sum_ssim = 0.0, sum_cs = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / NT; ++k) {
      const int o = tid + k * NT;
      const int r = o / TW, c = o - r * TW;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const double gi = p.g[i];
        m0 += gi * hp[0][r + i][c];
        m1 += gi * hp[1][r + i][c];
        m2 += gi * hp[2][r + i][c];
        m3 += gi * hp[3][r + i][c];
        m4 += gi * hp[4][r + i][c];
      }
      const double mu1 = m0 * inv, mu2 = m1 * inv;
      const double mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
      const double s1 = m2 * inv2 - mu11, s2 = m3 * inv2 - mu22, s12 = m4 * inv2 - mu12;
      const double cs = (2.0 * s12 + 9e-4) / (s1 + s2 + 9e-4);
      const double ssim = (2.0 * mu12 + 1e-4) / (mu11 + mu22 + 1e-4) * cs;
      if (oy + r < vh && ox + c < vw) {   // rows and columns past a partial tile contribute nothing
        sum_ssim += ssim;
        sum_cs += cs;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      sum_ssim += __shfl_down(sum_ssim, d, 64);
      sum_cs += __shfl_down(sum_cs, d, 64);
    }
    if (lane == 0) {
      red[wave][0] = sum_ssim;
      red[wave][1] = sum_cs;
    }
    __syncthreads();
    if (tid < 2) {
      double v = red[0][tid];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) v += red[w][tid];
      part[((size_t)plane * p.tiles + tile) * 2 + tid] = v;
    }
    __syncthreads();
  }
}

// One workgroup per (plane, level): its tiles' partial sums in a fixed order (thread i takes tiles i, i + 256, ...; then a fixed
// tree), divided by the size of the valid map -> levels[plane][level][{ssim, cs}].
__global__ __launch_bounds__(NT) void quality_final_kernel(const double *__restrict__ part, double *__restrict__ levels, QPlan p) {
  __shared__ double red[NT / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = blockIdx.x / QL, s = blockIdx.x - plane * QL;
  int Hs = p.lv[0].H, Ws = p.lv[0].W, tile0 = 0, ntiles = p.lv[0].ntiles;
#pragma unroll
  for (int k = 1; k < QL; ++k)
    if (s == k) {
      Hs = p.lv[k].H; Ws = p.lv[k].W; tile0 = p.lv[k].tile0; ntiles = p.lv[k].ntiles;
    }
  const double *src = part + ((size_t)plane * p.tiles + tile0) * 2;
  double v0 = 0.0, v1 = 0.0;
  for (int i = tid; i < ntiles; i += NT) {
    v0 += src[(size_t)i * 2];
    v1 += src[(size_t)i * 2 + 1];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    v0 += __shfl_down(v0, d, 64);
    v1 += __shfl_down(v1, d, 64);
  }
  if (lane == 0) {
    red[wave][0] = v0;
    red[wave][1] = v1;
  }
  __syncthreads();
  if (tid < 2) {
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) v += red[w][tid];
    levels[(size_t)blockIdx.x * 2 + tid] = v / ((double)(Hs - (QT - 1)) * (double)(Ws - (QT - 1)));
  }
}

}  // namespace

extern "C" int sgic_quality_u8_work_bytes(int B, int H, int W, size_t *bytes) {
  SGIC_REQUIRE(bytes != nullptr, "null output");
  QPlan p;
  SGIC_REQUIRE(make_plan(B, H, W, &p), "1 <= B <= 65536, 160 < H, W <= 16384");
  *bytes = p.bytes;
  return SGIC_OK;
}

extern "C" int sgic_quality_u8(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, uint8_t *d_work, size_t work_bytes,
                               int64_t *d_sse, double *d_levels, sgic_stream_t stream) {
  QPlan p;
  SGIC_REQUIRE(make_plan(B, H, W, &p), "1 <= B <= 65536, 160 < H, W <= 16384");
  SGIC_REQUIRE(d_a && d_b && d_work && d_sse && d_levels, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= p.bytes, "the workspace is smaller than sgic_quality_u8_work_bytes says");
  hipStream_t st = to_stream(stream);
  uint16_t *pyr = reinterpret_cast<uint16_t *>(d_work);
  double *part = reinterpret_cast<double *>(d_work + p.part_off);
  const int planes = 3 * B;
  SGIC_HIP(hipMemsetAsync(d_sse, 0, (size_t)planes * sizeof(int64_t), st));
  {
    const QLevel &L1 = p.lv[1];
    dim3 grid(cdiv((size_t)L1.H * L1.W, NT), B < MAX_GRID_Y ? B : MAX_GRID_Y);
    quality_pool0_sse_kernel<<<grid, NT, 0, st>>>(d_a, d_b, B, H, W, L1.H, L1.W, pyr + L1.off, pyr + p.img_elems + L1.off,
                                                  reinterpret_cast<unsigned long long *>(d_sse));
  }
  for (int s = 1; s + 1 < QL; ++s) {
    const QLevel &S = p.lv[s], &D = p.lv[s + 1];
    dim3 grid(cdiv((size_t)D.H * D.W, NT), 2 * planes < MAX_GRID_Y ? 2 * planes : MAX_GRID_Y);
    quality_pool_kernel<<<grid, NT, 0, st>>>(pyr, p.img_elems, S.off, D.off, planes, S.H, S.W, D.H, D.W);
  }
  {
    dim3 grid(p.tiles, planes < MAX_GRID_Y ? planes : MAX_GRID_Y);
    quality_level_kernel<<<grid, NT, 0, st>>>(d_a, d_b, pyr, part, p);
  }
  quality_final_kernel<<<planes * QL, NT, 0, st>>>(part, d_levels, p);
  return sgic::check_launch("sgic_quality_u8");
}
