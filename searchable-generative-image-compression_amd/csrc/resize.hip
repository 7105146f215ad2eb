// Image.resize for u8 RGB on the device: (B, H, W, 3) -> (B, OH, OW, 3), the bytes of Pillow's
// `Image.fromarray(x).resize((OW, OH), filter)` for filter 2 (bicubic) and 1 (Lanczos): ImagingResample for 8-bit images, the
// horizontal pass first, its output rounded to u8, then the vertical pass over that intermediate.  Both passes always run; a pass
// whose size does not change has the single tap 2^22 and copies.
//
// The tables (bounds and 22-bit coefficients of both axes, pil_resample.h's pil_coeff_row) are made ON THE HOST inside the call and
// uploaded on the stream: Lanczos needs sin(), Pillow's comes from the host's libm, and the device's double sin may differ from it
// in the last place.  They depend on the geometry alone and are a few KiB.  Built with -ffp-contract=off.
//
// Workspace: bounds_h (OW x 2 int32), kk_h (OW x ksize_h), bounds_v (OH x 2), kk_v (OH x ksize_v), each 16-byte aligned and
// uploaded as one block, then the intermediate (B x H rows of OW x 3 bytes at a row stride rounded up to 16 bytes, so that the
// vertical pass reads aligned dwords).
#include <algorithm>
#include <vector>

#include "common.h"
#include "pil_resample.h"

#define RS_MAX_SIDE 16384
#define RS_COEF_INTS 8192   // coefficients of a column tile held in LDS (32 KiB); a larger tile reads them from memory
#define RS_V_THREADS 256

// Horizontal pass.  A workgroup owns `tile` output columns, one per thread, and walks rows of the flattened (B x H) row list.  The
// tile's coefficient rows are staged in LDS once (KLDS), the source span of every row with 16-byte loads into three byte planes
// (u8c_stage_row), in several fills when one output has more taps than a fill holds.  Row strides of ksize ints are odd, so the
// lanes of a wave read distinct banks.
template <bool KLDS>
__global__ __launch_bounds__(U8C_THREADS) void resize_h_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ mid,
                                                               const int *__restrict__ bh, const int *__restrict__ kh, int ksize, long rows,
                                                               int W, int OW, int tile, int mid_stride) {
  __shared__ __attribute__((aligned(16))) uint8_t px[3][U8C_TILE_PX];
  __shared__ int kl[KLDS ? RS_COEF_INTS : 1];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int t0 = blockIdx.x * tile, nt = min(tile, OW - t0), last = t0 + nt - 1;
  const int w0 = bh[2 * t0], w1 = min(bh[2 * last] + bh[2 * last + 1], W);   // both ends of a window grow with the output index
  const bool active = tid < nt;
  const int ox = t0 + (active ? tid : 0);
  const int xmin = bh[2 * ox], xend = xmin + bh[2 * ox + 1];
  const int *kg = kh + (long)ox * ksize;
  const int kbase = (active ? tid : 0) * ksize;
  if (KLDS)      // visible after the barriers of the first fill
    for (int i = tid; i < nt * ksize; i += nth) kl[i] = kh[(long)t0 * ksize + i];
  for (long r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint8_t *row = in + r * W * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int c0 = w0; c0 < w1; c0 += U8C_TILE_PX) {
      const int n = min(U8C_TILE_PX, w1 - c0);
      __syncthreads();   // the previous fill has been read
      u8c_stage_row(row + 3L * c0, 3 * n, px, nth);
      __syncthreads();
      if (active) {
        const int lo = max(xmin, c0), hi = min(xend, c0 + n);
        for (int x = lo; x < hi; x++) {
          const int kv = KLDS ? kl[kbase + x - xmin] : kg[x - xmin], i = x - c0;
          a0 += (int)px[0][i] * kv;
          a1 += (int)px[1][i] * kv;
          a2 += (int)px[2][i] * kv;
        }
      }
    }
    if (active) {
      uint8_t *o = mid + r * mid_stride + 3 * ox;
      o[0] = (uint8_t)pil_acc_to_u8(a0);
      o[1] = (uint8_t)pil_acc_to_u8(a1);
      o[2] = (uint8_t)pil_acc_to_u8(a2);
    }
  }
}

// Vertical pass.  Consecutive threads take consecutive dwords of an output row (n = OW x 3 bytes): every tap is one coalesced read
// of an intermediate row, and the row's coefficients are the same for the whole workgroup.  The bytes of the last dword past n are
// padding of the intermediate and are not stored.
__global__ __launch_bounds__(RS_V_THREADS) void resize_v_kernel(const uint8_t *__restrict__ mid, uint8_t *__restrict__ out,
                                                                const int *__restrict__ bv, const int *__restrict__ kv, int ksize, long rows,
                                                                int H, int OH, int n, int mid_stride) {
  const int x = 4 * (blockIdx.x * RS_V_THREADS + threadIdx.x);
  if (x >= n) return;
  for (long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long b = r / OH;
    const int oy = (int)(r - b * OH);
    const int ymin = bv[2 * oy], cnt = bv[2 * oy + 1];
    const int *k = kv + (long)oy * ksize;
    const uint8_t *p = mid + (b * H + ymin) * mid_stride + x;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
    for (int j = 0; j < cnt; j++) {
      const unsigned w = *reinterpret_cast<const unsigned *>(p + (long)j * mid_stride);
      const int kj = k[j];
      a0 += (int)(w & 255u) * kj;
      a1 += (int)((w >> 8) & 255u) * kj;
      a2 += (int)((w >> 16) & 255u) * kj;
      a3 += (int)(w >> 24) * kj;
    }
    const unsigned q = (unsigned)pil_acc_to_u8(a0) | (unsigned)pil_acc_to_u8(a1) << 8 | (unsigned)pil_acc_to_u8(a2) << 16 |
                       (unsigned)pil_acc_to_u8(a3) << 24;
    uint8_t *o = out + r * n + x;
    if (x + 4 <= n && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<unsigned *>(o) = q;
    } else {
      for (int i = 0; i < min(4, n - x); i++) o[i] = (uint8_t)(q >> (8 * i));
    }
  }
}

struct ResizePlan {
  int ksize_h, ksize_v, tile, mid_stride;
  bool klds;
  size_t off[5];   // bounds_h, kk_h, bounds_v, kk_v, intermediate
  size_t total;
};

static bool resize_geometry_ok(int B, int H, int W, int OH, int OW, int filter) {
  const auto side = [](int v) { return v >= 1 && v <= RS_MAX_SIDE; };
  return B >= 1 && side(H) && side(W) && side(OH) && side(OW) && (filter == 1 || filter == 2);
}

template <class F>
static void resize_plan(int B, int H, int W, int OH, int OW, ResizePlan *p) {
  p->ksize_h = pil_ksize<F>(W, OW), p->ksize_v = pil_ksize<F>(H, OH);
  p->tile = u8c_tile(W, OW, std::min(OW, U8C_THREADS), F::support);
  p->klds = (long)p->tile * p->ksize_h <= RS_COEF_INTS;
  p->mid_stride = (OW * 3 + 15) & ~15;
  const size_t size[5] = {8u * (size_t)OW, 4u * (size_t)OW * p->ksize_h, 8u * (size_t)OH, 4u * (size_t)OH * p->ksize_v,
                          (size_t)B * H * p->mid_stride};
  size_t off = 0;
  for (int i = 0; i < 5; i++) {
    p->off[i] = off;
    off += (size[i] + 15) & ~(size_t)15;
  }
  p->total = off;
}

template <class F>
static void resize_tables(int in_size, int out_size, int ksize, int32_t *bounds, int32_t *kk) {
  for (int xx = 0; xx < out_size; xx++) pil_coeff_row<F>(in_size, out_size, ksize, xx, bounds, kk);
}

extern "C" size_t sgic_resize_u8_work_bytes(int B, int H, int W, int OH, int OW, int filter) {
  if (!resize_geometry_ok(B, H, W, OH, OW, filter)) return 0;
  ResizePlan p;
  if (filter == 2) resize_plan<PilBicubic>(B, H, W, OH, OW, &p);
  else resize_plan<PilLanczos>(B, H, W, OH, OW, &p);
  return p.total;
}

extern "C" int sgic_resize_u8_coeffs(int in_size, int out_size, int filter, int ksize, int32_t *h_bounds, int32_t *h_kk) {
  SGIC_REQUIRE(h_bounds && h_kk && in_size >= 1 && in_size <= RS_MAX_SIDE && out_size >= 1 && out_size <= RS_MAX_SIDE, "args");
  SGIC_REQUIRE(filter == 1 || filter == 2, "filter: 2 bicubic, 1 Lanczos");
  SGIC_REQUIRE(ksize == (filter == 2 ? pil_ksize<PilBicubic>(in_size, out_size) : pil_ksize<PilLanczos>(in_size, out_size)), "ksize");
  if (filter == 2) resize_tables<PilBicubic>(in_size, out_size, ksize, h_bounds, h_kk);
  else resize_tables<PilLanczos>(in_size, out_size, ksize, h_bounds, h_kk);
  return 0;
}

extern "C" int sgic_resize_u8_batch(const uint8_t *d_in, int B, int H, int W, uint8_t *d_out, int OH, int OW, int filter, uint8_t *d_work,
                                    size_t work_bytes, sgic_stream_t stream) {
  SGIC_REQUIRE(d_in && d_out && d_work, "null pointer");
  SGIC_REQUIRE(resize_geometry_ok(B, H, W, OH, OW, filter), "B >= 1, sides in [1, 16384], filter 2 (bicubic) or 1 (Lanczos)");
  SGIC_REQUIRE((((uintptr_t)d_work) & 15) == 0, "workspace alignment");
  ResizePlan p;
  if (filter == 2) resize_plan<PilBicubic>(B, H, W, OH, OW, &p);
  else resize_plan<PilLanczos>(B, H, W, OH, OW, &p);
  SGIC_REQUIRE(work_bytes >= p.total, "workspace too small (sgic_resize_u8_work_bytes)");
  hipStream_t st = to_stream(stream);
  // the tables: a pageable source, so the copy has left this buffer when hipMemcpyAsync returns (as the encoder's quantisation tables)
  std::vector<int32_t> tab(p.off[4] / 4, 0);
  int32_t *hb[4];
  for (int i = 0; i < 4; i++) hb[i] = tab.data() + p.off[i] / 4;
  if (filter == 2) {
    resize_tables<PilBicubic>(W, OW, p.ksize_h, hb[0], hb[1]);
    resize_tables<PilBicubic>(H, OH, p.ksize_v, hb[2], hb[3]);
  } else {
    resize_tables<PilLanczos>(W, OW, p.ksize_h, hb[0], hb[1]);
    resize_tables<PilLanczos>(H, OH, p.ksize_v, hb[2], hb[3]);
  }
  SGIC_HIP(hipMemcpyAsync(d_work, tab.data(), p.off[4], hipMemcpyHostToDevice, st));
  const int *bh = reinterpret_cast<const int *>(d_work + p.off[0]), *kh = reinterpret_cast<const int *>(d_work + p.off[1]);
  const int *bv = reinterpret_cast<const int *>(d_work + p.off[2]), *kv = reinterpret_cast<const int *>(d_work + p.off[3]);
  uint8_t *mid = d_work + p.off[4];

  const long rows_h = (long)B * H, rows_v = (long)B * OH;
  const dim3 gh(cdiv(OW, p.tile), (unsigned)std::min((rows_h + 3) / 4, 4096L));
  const unsigned threads_h = (unsigned)((std::min(p.tile, U8C_THREADS) + 63) & ~63);
  if (p.klds) resize_h_kernel<true><<<gh, threads_h, 0, st>>>(d_in, mid, bh, kh, p.ksize_h, rows_h, W, OW, p.tile, p.mid_stride);
  else resize_h_kernel<false><<<gh, threads_h, 0, st>>>(d_in, mid, bh, kh, p.ksize_h, rows_h, W, OW, p.tile, p.mid_stride);
  int rc = sgic::check_launch("resize_h_kernel");
  if (rc) return rc;
  const int n = OW * 3;
  const dim3 gv(cdiv(cdiv(n, 4), RS_V_THREADS), (unsigned)std::min(rows_v, 4096L));
  resize_v_kernel<<<gv, RS_V_THREADS, 0, st>>>(mid, d_out, bv, kv, p.ksize_v, rows_v, H, OH, n, p.mid_stride);
  return sgic::check_launch("resize_v_kernel");
}
