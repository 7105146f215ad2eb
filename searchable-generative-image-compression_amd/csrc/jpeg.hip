// Baseline JPEG decode on the GPU for the compress driver's ingest (replaces the pixel decode inside the reference's
// Test_Dataset, compress.py:151-168: `Image.open(path).convert("RGB")`), BIT-EXACT with Pillow / libjpeg-turbo's default decoder:
// Huffman decode -> dequantise + "islow" integer IDCT (jidctint.c) -> fancy (triangle) chroma upsampling (jdsample.c: h2v1, h2v2,
// h1v2) -> YCbCr -> RGB with the fixed-point tables of jdcolor.c -> u8 HWC, the layout sgic_u8hwc_to_f32chw_pad consumes.
// The host (sgic_amd/jpeg.py) only parses markers, builds the Huffman lookup tables and strips the 0xFF00 stuffing / RSTn markers
// (byte shuffling, no entropy decoding); every coded bit is decoded here.
//
// Three kernels over a batch:
//   jpeg_huff_kernel      one wave per image.  The entropy-coded segment is a serial bit stream, so the wave runs the decode loop as
//                         wave-uniform code (every lane computes the same state -- the cost of one lane) and uses its 64 lanes for
//                         what IS parallel: streaming the scan through a 4 KiB LDS ring in 1 KiB coalesced chunks, zeroing /
//                         storing each 64-coefficient block (lane = coefficient), holding the lookup tables in LDS.
//   jpeg_idct_kernel      one thread per 8x8 block: dequantise, two 1-D passes of the LL&M integer IDCT, range limit -> u8 planes.
//   jpeg_color_kernel     one thread per output pixel: chroma upsampling of the 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 layouts + colour
//                         conversion (or grey -> RGB).
// Progressive / multi-scan files replace the first kernel by jpeg_scan_kernel (one wave per (image, scan), one launch per dependency
// level of the batch's scans) and then run the same two.
// All integer arithmetic: parity with Pillow is exact (tests/test_gpu_jpeg.py, tests/test_gpu_jpeg_scans.py), not a tolerance.
#include "common.h"

#define JPG_NP 64            // int32 parameters per image (sgic_amd/jpeg.py: PARAM_*)
#define JPG_LOOK 9           // bits of the fast Huffman lookup
#define JPG_TAB_BYTES 1424   // one table: u16 fast[512] | i32 maxcode[18] | i32 valoff[17] | pad 4 | u8 huffval[256]
#define JPG_RING 4096     // LDS: ring 4 KiB + tables 5.6 KiB = 9.9 KiB: the wave fits BESIDE a 144 KiB GEMM workgroup on the same CU
#define JPG_CHUNK 1024

enum {
  P_SCAN_OFF = 0, P_SCAN_LEN, P_TAB_OFF, P_QUANT_OFF, P_NCOMP, P_W, P_H, P_HMAX, P_VMAX, P_MCUS_X, P_MCUS_Y, P_RESTART, P_SEG_OFF, P_NSEG,
  P_SCAN_BYTES = 14,   // the scan's own length in bytes (P_SCAN_LEN is that length padded with zeros to whole chunks)
  P_COMP0 = 16,   // per component, 12 ints: h, v, qtab, dctab, actab, blocks_w, blocks_h, comp_w, comp_h, coef_off (blocks), plane_off (bytes), unused
  P_CSTRIDE = 12
};

__constant__ unsigned char jpg_natural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                                              6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                              39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// ---- the entropy-coded segment, shared by jpeg_huff_kernel and jpeg_scan_kernel --------------------------------------------------------
// One wave reads one cleaned segment: 1 KiB coalesced chunks (lane = 16 B) into a 4 KiB LDS ring, and a 64-bit bit accumulator that every
// lane holds identically (wave-uniform state).  The segment is padded by the host to a multiple of JPG_CHUNK with zeros.
struct JpgBits {
  unsigned char *ring;
  const unsigned char *src;
  int total, lane;
  int filled;   // bytes of the segment staged so far (wave-uniform)
  // bit reader: `acc` holds `cnt` valid bits, MSB first; rp = byte position of the next 32-bit word to fetch
  unsigned long long acc;
  int cnt, rp, bad;

  __device__ __forceinline__ void fill() {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + filled);
    uint4 *d4 = reinterpret_cast<uint4 *>(ring + (filled & (JPG_RING - 1)));
#pragma unroll
    for (int i = 0; i < JPG_CHUNK / 16 / 64; i++) d4[lane + 64 * i] = s4[lane + 64 * i];
    filled += JPG_CHUNK;
  }
  __device__ __forceinline__ void start(unsigned char *ring_, const unsigned char *src_, int total_, int lane_) {
    ring = ring_;
    src = src_;
    total = total_;
    lane = lane_;
    filled = 0;
    acc = 0;
    cnt = rp = bad = 0;
    fill();
    if (total > JPG_CHUNK) fill();
  }
  __device__ __forceinline__ void refill() {
    while (cnt <= 32) {
      if (filled - rp < JPG_CHUNK + 8 && filled < total) {   // uniform: stage the next chunk (the ring keeps > 4 KiB unread at most)
        fill();
        __syncthreads();
      }
      unsigned w = 0;
      if (rp < total) w = *reinterpret_cast<const unsigned *>(ring + (rp & (JPG_RING - 1)));
      w = __builtin_bswap32(w);
      acc |= (unsigned long long)w << (32 - cnt);
      cnt += 32;
      rp += 4;
    }
  }
  __device__ __forceinline__ void seek(int byte_off) {   // restart boundary: continue at a byte offset of the cleaned segment
    const int aligned = byte_off & ~3;
    if (aligned >= filled || aligned < filled - JPG_RING + JPG_CHUNK) {   // outside the staged window: restage from there
      filled = aligned & ~(JPG_CHUNK - 1);
      fill();
      if (filled < total) fill();
      __syncthreads();
    }
    rp = aligned;
    acc = 0;
    cnt = 0;
    refill();
    const int skip = (byte_off - aligned) * 8;
    acc <<= skip;
    cnt -= skip;
  }
  __device__ __forceinline__ int decode(const unsigned char *T) {   // one Huffman symbol
    refill();
    const unsigned e = reinterpret_cast<const unsigned short *>(T)[(unsigned)(acc >> (64 - JPG_LOOK))];
    if (e) {
      const int nb = e >> 8;
      acc <<= nb;
      cnt -= nb;
      return e & 255;
    }
    const int *maxcode = reinterpret_cast<const int *>(T + 1024), *valoff = maxcode + 18;
    const unsigned code16 = (unsigned)(acc >> 48);
    int l = JPG_LOOK + 1;
    while (l <= 16 && (int)(code16 >> (16 - l)) > maxcode[l]) l++;
    if (l > 16) {
      bad = 1;
      return 0;
    }
    const int sym = T[1024 + 72 + 68 + 4 + ((valoff[l] + (int)(code16 >> (16 - l))) & 255)];
    acc <<= l;
    cnt -= l;
    return sym;
  }
  __device__ __forceinline__ unsigned bits(int n) {   // n raw bits, 1 <= n <= 32 (after a refill)
    const unsigned v = (unsigned)(acc >> (64 - n));
    acc <<= n;
    cnt -= n;
    return v;
  }
  // bytes of the segment the decode has used so far: from the bit position (rp counts the words prefetched into `acc`, of which `cnt`
  // bits are still unread), not from the prefetch pointer
  __device__ __forceinline__ int consumed() const { return (rp * 8 - cnt + 7) >> 3; }
  __device__ __forceinline__ int receive(int s) {   // s extra bits, sign-extended (jdhuff.c HUFF_EXTEND)
    const int v = (int)bits(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  }
};

// ---- Huffman decode: one wave per image -------------------------------------------------------------------------------------------
// params / scan / tabs / segs / quant_in may live in PINNED HOST memory (the kernel pulls them over PCIe: a batch is ~1 MB, read once,
// in coalesced 1 KiB chunks) -- there is then no H2D copy to schedule; the descriptors and quantisation tables the two later kernels
// need are left in device memory (params_dev, quant_dev) by this one.
__global__ __launch_bounds__(64) void jpeg_huff_kernel(const int *__restrict__ params, const unsigned char *__restrict__ scan,
                                                       const unsigned char *__restrict__ tabs, const int *__restrict__ segs,
                                                       const unsigned short *__restrict__ quant_in, int *__restrict__ params_dev,
                                                       unsigned short *__restrict__ quant_dev, short *__restrict__ coef,
                                                       int *__restrict__ err) {
  __shared__ __attribute__((aligned(16))) unsigned char ring[JPG_RING];
  __shared__ __attribute__((aligned(16))) unsigned char tab[4 * JPG_TAB_BYTES];
  __shared__ short blk[64];
  const int img = blockIdx.x, lane = threadIdx.x;
  __shared__ int Ps[JPG_NP];
  Ps[lane] = params[(size_t)img * JPG_NP + lane];
  params_dev[(size_t)img * JPG_NP + lane] = Ps[lane];
  __syncthreads();
  const int *P = Ps;
  for (int i = lane; i < 256; i += 64) quant_dev[(size_t)img * 256 + i] = quant_in[P[P_QUANT_OFF] + i];
  {
    const uint4 *t4 = reinterpret_cast<const uint4 *>(tabs + P[P_TAB_OFF]);
    for (int i = lane; i < 4 * JPG_TAB_BYTES / 16; i += 64) reinterpret_cast<uint4 *>(tab)[i] = t4[i];
  }
  JpgBits br;
  br.start(ring, scan + P[P_SCAN_OFF], P[P_SCAN_LEN], lane);
  __syncthreads();
  int &bad = br.bad;

  const int ncomp = P[P_NCOMP], mcus = P[P_MCUS_X] * P[P_MCUS_Y], mcus_x = P[P_MCUS_X], restart = P[P_RESTART];
  const int *seg = segs + P[P_SEG_OFF];
  int pred[3] = {0, 0, 0};
  int next_seg = 1;
  for (int mcu = 0; mcu < mcus && !bad; mcu++) {
    if (restart && mcu && mcu % restart == 0) {
      if (next_seg >= P[P_NSEG]) {
        bad = 2;
        break;
      }
      br.seek(seg[next_seg++]);
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int my = mcu / mcus_x, mx = mcu - my * mcus_x;
    for (int c = 0; c < ncomp; c++) {
      const int *C = P + P_COMP0 + c * P_CSTRIDE;
      const int hs = ncomp == 1 ? 1 : C[0], vs = ncomp == 1 ? 1 : C[1];   // a single-component scan is not interleaved: one block per MCU
      const unsigned char *Tdc = tab + C[3] * JPG_TAB_BYTES, *Tac = tab + (2 + C[4]) * JPG_TAB_BYTES;
      for (int by = 0; by < vs; by++)
        for (int bx = 0; bx < hs; bx++) {
          blk[lane] = 0;
          int s = br.decode(Tdc);
          if (s > 15) {   // not a magnitude category (the host refuses such a DC table: sgic_amd/jpeg.py _check_dc_table)
            bad = 1;
            s = 0;
          }
          if (s) {
            br.refill();
            pred[c] += br.receive(s);
          }
          if (lane == 0) blk[0] = (short)pred[c];
          for (int k = 1; k < 64;) {
            const int rs = br.decode(Tac);
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;   // EOB
              k += 16;
              continue;
            }
            k += r;
            br.refill();
            const int v = br.receive(s);
            if (lane == 0) blk[jpg_natural[k]] = (short)v;   // k <= 63 + 15: the table is padded to 80 entries
            k++;
          }
          const size_t b = (size_t)C[9] + (size_t)(my * vs + by) * C[5] + (mx * hs + bx);
          coef[b * 64 + lane] = blk[lane];
        }
    }
  }
  // a valid encoder pads its last byte with ones and stops: a decode that needed more bits than the scan holds read the zero padding
  if (!bad && br.consumed() > P[P_SCAN_BYTES]) bad = 3;
  if (lane == 0) err[img] = bad;
}

// ---- progressive / multi-scan decode: one wave per (image, scan) ------------------------------------------------------------------
// The decode procedures of T.81 G.1.2 as libjpeg-turbo's jdphuff.c runs them, plus the sequential block loop above for one scan of a
// baseline or multi-scan sequential file.  The host (sgic_amd/jpeg.py ScanJpegBatch) groups the scans of a batch into dependency
// levels: the scans of one level touch disjoint (component, coefficient) sets of the coefficient array, so one launch runs a whole
// level and stream order between the launches is the only synchronisation.  A scan therefore stores ONLY the coefficients of its
// band (2-byte stores), never a whole 64-entry block, and reads only its band (refinement scans).  The array is zeroed beforehand.
enum {   // per-scan descriptor, 32 int32 (sgic_amd/jpeg.py: S_*)
  S_IMG = 0, S_MODE, S_NCOMP, S_COMP0, S_SS = 6, S_SE, S_AH, S_AL, S_RESTART, S_SCAN_OFF, S_SCAN_LEN, S_SEG_OFF, S_NSEG,
  S_GW = 15, S_GH,   // units of the scan: MCUs of the frame (interleaved) or the component's own ceil(cw/8) x ceil(ch/8) blocks
  S_NTAB = 17, S_TAB0,   // the scan's (<= 4) Huffman tables: indices into the batch's table pool
  S_DC0 = 22, S_AC0 = 25,   // per scan component: its DC / AC table among the scan's (0..3)
  S_FIRST = 28,   // the image's first scan (level 0): copies params / quant into device memory for the IDCT / colour kernels
  S_SCAN_BYTES = 29,   // the scan's own length in bytes (S_SCAN_LEN is that length padded with zeros to whole chunks)
  JPG_NS = 32
};
enum { M_SEQ = 0, M_DC_FIRST, M_DC_REFINE, M_AC_FIRST, M_AC_REFINE };

__global__ __launch_bounds__(64) void jpeg_scan_kernel(const int *__restrict__ params, const int *__restrict__ descs,
                                                       const unsigned char *__restrict__ scan, const unsigned char *__restrict__ tabs,
                                                       const int *__restrict__ segs, const unsigned short *__restrict__ quant_in,
                                                       int *__restrict__ params_dev, unsigned short *__restrict__ quant_dev,
                                                       short *__restrict__ coef, int *__restrict__ err) {
  __shared__ __attribute__((aligned(16))) unsigned char ring[JPG_RING];
  __shared__ __attribute__((aligned(16))) unsigned char tab[4 * JPG_TAB_BYTES];
  __shared__ int Ps[JPG_NP], Ss_[JPG_NS];
  const int lane = threadIdx.x;
  if (lane < JPG_NS) Ss_[lane] = descs[(size_t)blockIdx.x * JPG_NS + lane];
  __syncthreads();
  const int *S = Ss_;
  const int img = S[S_IMG];
  Ps[lane] = params[(size_t)img * JPG_NP + lane];
  if (S[S_FIRST]) params_dev[(size_t)img * JPG_NP + lane] = Ps[lane];
  __syncthreads();
  const int *P = Ps;
  if (S[S_FIRST])
    for (int i = lane; i < 256; i += 64) quant_dev[(size_t)img * 256 + i] = quant_in[P[P_QUANT_OFF] + i];
  for (int t = 0; t < S[S_NTAB]; t++) {
    const uint4 *t4 = reinterpret_cast<const uint4 *>(tabs + (size_t)S[S_TAB0 + t] * JPG_TAB_BYTES);
    for (int i = lane; i < JPG_TAB_BYTES / 16; i += 64) reinterpret_cast<uint4 *>(tab + t * JPG_TAB_BYTES)[i] = t4[i];
  }
  JpgBits br;
  br.start(ring, scan + S[S_SCAN_OFF], S[S_SCAN_LEN], lane);
  __syncthreads();

  const int mode = S[S_MODE], ns = S[S_NCOMP], Ss = S[S_SS], Se = S[S_SE], Al = S[S_AL], restart = S[S_RESTART];
  const int gw = S[S_GW], units = S[S_GW] * S[S_GH];
  const int *seg = segs + S[S_SEG_OFF];
  // block `j` (scan order) of unit `u` -> index of the block in the coefficient array
  auto block_of = [&](int u, int j) -> size_t {
    const int uy = u / gw, ux = u - uy * gw;
    if (ns == 1) {
      const int *C = P + P_COMP0 + S[S_COMP0] * P_CSTRIDE;
      return (size_t)C[9] + (size_t)uy * C[5] + ux;
    }
    for (int i = 0;; i++) {
      const int *C = P + P_COMP0 + S[S_COMP0 + i] * P_CSTRIDE;
      const int hs = C[0], vs = C[1];
      if (j < hs * vs || i == ns - 1) {
        const int by = j / hs, bx = j - by * hs;
        return (size_t)C[9] + (size_t)(uy * vs + by) * C[5] + (ux * hs + bx);
      }
      j -= hs * vs;
    }
  };
  int bpu = 0;   // blocks per unit
  for (int i = 0; i < ns; i++) {
    const int *C = P + P_COMP0 + S[S_COMP0 + i] * P_CSTRIDE;
    bpu += ns == 1 ? 1 : C[0] * C[1];
  }
  // lane = zig-zag index k of the coefficient it holds (AC scans and the sequential loop)
  const int nat = jpg_natural[lane];
  const bool inband = lane >= Ss && lane <= Se;
  const unsigned long long band = (~0ull >> (63 - Se)) & (~0ull << Ss);
  int pred[3] = {0, 0, 0};
  int eobrun = 0, next_seg = 1;
  int &bad = br.bad;

  if (mode == M_DC_REFINE) {
    // one raw bit per block, no Huffman code: lane-parallel over 32 blocks at a time (within a restart interval)
    const int p1 = 1 << Al;
    for (int u0 = 0; u0 < units && !bad;) {
      if (restart && u0) {
        if (next_seg >= S[S_NSEG]) {
          bad = 2;
          break;
        }
        br.seek(seg[next_seg++]);
      }
      const int u1 = restart ? min(u0 + restart, units) : units;
      const int nb = (u1 - u0) * bpu;
      for (int j0 = 0; j0 < nb; j0 += 32) {
        const int m = min(32, nb - j0);
        br.refill();
        const unsigned b = br.bits(m);
        const int j = j0 + lane;
        if (lane < m && ((b >> (m - 1 - lane)) & 1)) {
          const int q = j / bpu;
          short *c = coef + block_of(u0 + q, j - q * bpu) * 64;
          c[0] = (short)(c[0] | p1);
        }
      }
      u0 = u1;
    }
  } else if (mode == M_AC_REFINE) {
    const int p1 = 1 << Al;
    const unsigned char *Tac = tab + S[S_AC0] * JPG_TAB_BYTES;
    const unsigned long long below = (1ull << lane) - 1;   // zig-zag positions before this lane's
    int nextv = inband && units ? coef[block_of(0, 0) * 64 + nat] : 0;
    for (int u = 0; u < units && !bad; u++) {
      if (restart && u && u % restart == 0) {
        if (next_seg >= S[S_NSEG]) {
          bad = 2;
          break;
        }
        br.seek(seg[next_seg++]);
        eobrun = 0;
      }
      const size_t blk = block_of(u, 0);
      int v = nextv;   // this block's band, loaded one block ahead: the load latency hides under the previous block's decode
      if (inband && u + 1 < units) nextv = coef[block_of(u + 1, 0) * 64 + nat];
      const unsigned long long nz = __ballot(v != 0) & band;   // the band's already-nonzero coefficients (wave-uniform)
      // correction bits, in zig-zag order, for the nonzero coefficients of mask `cm`: each lane applies its own bit
      auto correct = [&](unsigned long long cm) {
        const int n = __popcll(cm), rank = __popcll(cm & below);
        const bool mine = (cm >> lane) & 1;
        for (int done = 0; done < n; done += 32) {
          const int m = min(32, n - done);
          br.refill();
          const unsigned b = br.bits(m);
          if (mine && rank >= done && rank < done + m && ((b >> (m - 1 - (rank - done))) & 1) && (v & p1) == 0) v += v >= 0 ? p1 : -p1;
        }
      };
      int k = Ss;
      if (eobrun == 0) {
        while (k <= Se) {
          const int rs = br.decode(Tac);
          if (bad) break;
          const int r = rs >> 4, s = rs & 15;
          int sv = 0;
          if (s) {   // a new coefficient of magnitude 1 << Al (s != 1 only in a corrupt file; libjpeg takes it the same way)
            br.refill();
            sv = br.bits(1) ? p1 : -p1;
          } else if (r != 15) {   // EOBn: the rest of this block and eobrun - 1 more take correction bits only
            eobrun = 1 << r;
            if (r) {
              br.refill();
              eobrun += (int)br.bits(r);
            }
            break;
          }
          // skip r zero coefficients (ZRL: 15, and the 16th is skipped too) taking a correction bit for every nonzero one passed
          unsigned long long z = ~nz & band & (~0ull << k);
          for (int i = 0; i < r && z; i++) z &= z - 1;
          const int t = z ? __ffsll((long long)z) - 1 : Se + 1;
          correct(nz & (~0ull << k) & (t > 63 ? ~0ull : (1ull << t) - 1));
          if (s) {
            if (t > Se) {   // a new coefficient past the band end: corrupt
              bad = 3;
              break;
            }
            if (lane == t) v = sv;
          }
          k = t + 1;
        }
      }
      if (eobrun > 0 && !bad) {
        if (k <= Se) correct(nz & (~0ull << k));
        eobrun--;
      }
      if (inband) coef[blk * 64 + nat] = (short)v;
    }
  } else {
    for (int u = 0; u < units && !bad; u++) {
      if (restart && u && u % restart == 0) {
        if (next_seg >= S[S_NSEG]) {
          bad = 2;
          break;
        }
        br.seek(seg[next_seg++]);
        pred[0] = pred[1] = pred[2] = 0;
        eobrun = 0;
      }
      for (int i = 0, j = 0; i < ns && !bad; i++) {
        const int *C = P + P_COMP0 + S[S_COMP0 + i] * P_CSTRIDE;
        const int nbl = ns == 1 ? 1 : C[0] * C[1];
        const unsigned char *Tdc = tab + S[S_DC0 + i] * JPG_TAB_BYTES, *Tac = tab + S[S_AC0 + i] * JPG_TAB_BYTES;
        for (int q = 0; q < nbl; q++, j++) {
          const size_t blk = block_of(u, j);
          if (mode == M_SEQ || mode == M_DC_FIRST) {
            int s = br.decode(Tdc);
            if (s > 15) bad = 1;
            if (bad) break;
            if (s) {
              br.refill();
              pred[i] += br.receive(s);
            }
            if (mode == M_DC_FIRST) {
              if (lane == 0) coef[blk * 64] = (short)(int)((unsigned)pred[i] << Al);
              continue;
            }
          }
          // AC first (Ss..Se, EOBRUN) or the sequential block (1..63): the value of zig-zag position `lane`
          if (mode == M_AC_FIRST && eobrun > 0) {
            eobrun--;
            continue;
          }
          int v = mode == M_SEQ && lane == 0 ? pred[i] : 0;
          bool any = mode == M_SEQ;
          for (int k = mode == M_SEQ ? 1 : Ss; k <= (mode == M_SEQ ? 63 : Se);) {
            const int rs = br.decode(Tac);
            if (bad) break;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
              if (r == 15) {   // ZRL
                k += 16;
                continue;
              }
              if (mode == M_AC_FIRST) {   // EOBn
                eobrun = 1 << r;
                if (r) {
                  br.refill();
                  eobrun += (int)br.bits(r);
                }
                eobrun--;
              }
              break;
            }
            k += r;
            if (k > (mode == M_SEQ ? 63 : Se)) {   // a coefficient past the band end: corrupt
              bad = 3;
              break;
            }
            br.refill();
            const int val = br.receive(s);
            if (lane == k) v = (int)((unsigned)val << Al);
            any = true;
            k++;
          }
          if (any && (mode == M_SEQ || inband)) coef[blk * 64 + nat] = (short)v;
        }
      }
    }
  }
  if (!bad && br.consumed() > S[S_SCAN_BYTES]) bad = 3;   // the scan ended before its last unit (as in jpeg_huff_kernel)
  if (lane == 0 && bad) atomicMax(err + img, bad);
}

// ---- dequantise + islow IDCT (jidctint.c jpeg_idct_islow), one thread per block ------------------------------------------------------
#define JC(x) ((int)(x))
#define J_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
__device__ __forceinline__ void jpg_idct_1d(const int in[8], int out[8], int shift) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * JC(4433);
  int tmp2 = z1 + z3 * -JC(15137);
  int tmp3 = z1 + z2 * JC(6270);
  z2 = in[0];
  z3 = in[4];
  int tmp0 = (z2 + z3) << 13;
  int tmp1 = (z2 - z3) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * JC(9633);
  tmp0 *= JC(2446);
  tmp1 *= JC(16819);
  tmp2 *= JC(25172);
  tmp3 *= JC(12299);
  z1 *= -JC(7373);
  z2 *= -JC(20995);
  z3 *= -JC(16069);
  z4 *= -JC(3196);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = J_DESCALE(tmp10 + tmp3, shift);
  out[7] = J_DESCALE(tmp10 - tmp3, shift);
  out[1] = J_DESCALE(tmp11 + tmp2, shift);
  out[6] = J_DESCALE(tmp11 - tmp2, shift);
  out[2] = J_DESCALE(tmp12 + tmp1, shift);
  out[5] = J_DESCALE(tmp12 - tmp1, shift);
  out[3] = J_DESCALE(tmp13 + tmp0, shift);
  out[4] = J_DESCALE(tmp13 - tmp0, shift);
}

__device__ __forceinline__ unsigned char jpg_range_limit(int v) {   // libjpeg's range_limit table behind `& RANGE_MASK`, centred at 128
  const int i = v & 1023;
  return (unsigned char)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

__global__ void jpeg_idct_kernel(const int *__restrict__ params, const short *__restrict__ coef, const unsigned short *__restrict__ quant,
                                 unsigned char *__restrict__ planes, int max_blocks) {
  const int img = blockIdx.y;
  const int *P = params + (size_t)img * JPG_NP;
  const int ncomp = P[P_NCOMP];
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < max_blocks; t += gridDim.x * blockDim.x) {
    int c = 0, local = t;
    while (c < ncomp) {   // which component does block t of this image belong to?
      const int nb = P[P_COMP0 + c * P_CSTRIDE + 5] * P[P_COMP0 + c * P_CSTRIDE + 6];
      if (local < nb) break;
      local -= nb;
      c++;
    }
    if (c >= ncomp) continue;
    const int *C = P + P_COMP0 + c * P_CSTRIDE;
    const int bw = C[5], by = local / bw, bx = local - by * bw;
    const short *cf = coef + ((size_t)C[9] + local) * 64;
    const unsigned short *q = quant + (size_t)img * 256 + (C[2] & 3) * 64;   // quant_dev of jpeg_huff_kernel: image-major, 4 tables each
    int ws[64];
    // pass 1: columns
#pragma unroll
    for (int x = 0; x < 8; x++) {
      int in[8], o[8];
#pragma unroll
      for (int y = 0; y < 8; y++) in[y] = (int)cf[y * 8 + x] * (int)q[y * 8 + x];
      jpg_idct_1d(in, o, 13 - 2);
#pragma unroll
      for (int y = 0; y < 8; y++) ws[y * 8 + x] = o[y];
    }
    // pass 2: rows
    unsigned char *dst = planes + (size_t)C[10] + (size_t)(by * 8) * (bw * 8) + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
      int o[8];
      jpg_idct_1d(ws + y * 8, o, 13 + 2 + 3);
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int x = 0; x < 4; x++) {
        lo |= (unsigned)jpg_range_limit(o[x]) << (8 * x);
        hi |= (unsigned)jpg_range_limit(o[x + 4]) << (8 * x);
      }
      *reinterpret_cast<uint2 *>(dst + (size_t)y * (bw * 8)) = make_uint2(lo, hi);
    }
  }
}

// ---- chroma upsampling (jdsample.c fancy upsamplers) + YCbCr -> RGB (jdcolor.c) -----------------------------------------------------
__device__ __forceinline__ int jpg_chroma(const unsigned char *pl, int stride, int cw, int ch, int hs, int vs, int x, int y) {
  // value of a chroma plane (downsampled cw x ch, row stride `stride`) at full-resolution pixel (x, y); hs / vs = luma samples per chroma
  // sample horizontally / vertically (1 or 2)
  if (hs == 1 && vs == 1) return pl[(size_t)y * stride + x];
  if (vs == 1) {   // h2v1_fancy_upsample
    const unsigned char *r = pl + (size_t)y * stride;
    const int c = x >> 1;
    if (x & 1) return c == cw - 1 ? r[c] : (3 * r[c] + r[c + 1] + 2) >> 2;
    return c == 0 ? r[0] : (3 * r[c] + r[c - 1] + 1) >> 2;
  }
  const int cy = y >> 1, v = y & 1;
  const int fy = v ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const unsigned char *r0 = pl + (size_t)cy * stride, *r1 = pl + (size_t)fy * stride;
  if (hs == 1) return (3 * r0[x] + r1[x] + (v ? 2 : 1)) >> 2;   // h1v2_fancy_upsample
  // h2v2_fancy_upsample: 9/16, 3/16, 3/16, 1/16
  const int c = x >> 1;
  const int cur = 3 * r0[c] + r1[c];
  if (x & 1) {
    if (c == cw - 1) return (cur * 4 + 7) >> 4;
    return (cur * 3 + 3 * r0[c + 1] + r1[c + 1] + 7) >> 4;
  }
  if (c == 0) return (cur * 4 + 8) >> 4;
  return (cur * 3 + 3 * r0[c - 1] + r1[c - 1] + 8) >> 4;
}

// out is a (B, H, W, 3) canvas: image img (its own P_W x P_H, at most H x W) lands at its top left; the rest is not written
__global__ void jpeg_color_kernel(const int *__restrict__ params, const unsigned char *__restrict__ planes, unsigned char *__restrict__ out,
                                  int H, int W) {
  const int img = blockIdx.y;
  const int *P = params + (size_t)img * JPG_NP;
  const int ncomp = P[P_NCOMP];
  const int *C0 = P + P_COMP0, *C1 = C0 + P_CSTRIDE, *C2 = C1 + P_CSTRIDE;
  const int hmax = P[P_HMAX], vmax = P[P_VMAX];
  const int w = min(P[P_W], W), h = min(P[P_H], H);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)h * w; t += (long)gridDim.x * blockDim.x) {
    const int y = (int)(t / w), x = (int)(t - (long)y * w);
    const int yy = planes[(size_t)C0[10] + (size_t)y * (C0[5] * 8) + x];
    int r = yy, g = yy, b = yy;
    if (ncomp == 3) {
      const int hs = hmax / C1[0], vs = vmax / C1[1];
      const int cb = jpg_chroma(planes + C1[10], C1[5] * 8, C1[7], C1[8], hs, vs, x, y) - 128;
      const int cr = jpg_chroma(planes + C2[10], C2[5] * 8, C2[7], C2[8], hs, vs, x, y) - 128;
      // jdcolor.c build_ycc_rgb_table: SCALEBITS 16, ONE_HALF 32768, FIX(1.40200) 91881, FIX(1.77200) 116130, FIX(0.71414) 46802, FIX(0.34414) 22554
      r = yy + ((91881 * cr + 32768) >> 16);
      b = yy + ((116130 * cb + 32768) >> 16);
      g = yy + ((-22554 * cb + 32768 + -46802 * cr) >> 16);
      r = min(max(r, 0), 255);
      g = min(max(g, 0), 255);
      b = min(max(b, 0), 255);
    }
    unsigned char *o = out + (((size_t)img * H + y) * W + x) * 3;
    o[0] = (unsigned char)r;
    o[1] = (unsigned char)g;
    o[2] = (unsigned char)b;
  }
}

// Decode a batch of B baseline JPEGs of equal geometry (H, W) to RGB u8 HWC (B, H, W, 3) on the device.
//   d_params  B x 64 int32 (layout above, built by sgic_amd/jpeg.py), d_scan the cleaned entropy-coded segments (each padded to a
//   multiple of 2048 bytes), d_tabs B x 4 Huffman tables (dc0, dc1, ac0, ac1) of 1424 bytes, d_segs the restart-interval byte offsets,
//   d_quant u16 quantisation tables in natural order, d_coef / d_planes workspaces (total_blocks * 64 int16 / plane_bytes u8),
//   d_err B int32 (0 ok, 1 invalid Huffman code or DC size, 2 missing restart segment, 3 the scan ended before the last MCU: more bytes
//   were consumed than the unpadded length in params[14]).  max_blocks = the largest per-image block count.
//   The five input arrays may be device memory or device-accessible PINNED host memory (no copy is then needed at all);
//   d_work_params (B x 64 int32) / d_work_quant (B x 256 u16): device scratch for the copies the later kernels read.
extern "C" int sgic_jpeg_decode_batch(const int32_t *d_params, const uint8_t *d_scan, const uint8_t *d_tabs, const int32_t *d_segs,
                                      const uint16_t *d_quant, int32_t *d_work_params, uint16_t *d_work_quant, int16_t *d_coef,
                                      uint8_t *d_planes, uint8_t *d_out, int32_t *d_err, int B, int H, int W, int max_blocks,
                                      sgic_stream_t stream) {
  SGIC_REQUIRE(d_params && d_scan && d_tabs && d_segs && d_quant && d_work_params && d_work_quant && d_coef && d_planes && d_out && d_err, "null");
  SGIC_REQUIRE(B > 0 && H > 0 && W > 0 && max_blocks > 0, "shape");
  SGIC_REQUIRE((((uintptr_t)d_scan | (uintptr_t)d_tabs | (uintptr_t)d_planes) & 15) == 0, "16-byte alignment");
  hipStream_t st = to_stream(stream);
  jpeg_huff_kernel<<<B, 64, 0, st>>>(d_params, d_scan, d_tabs, d_segs, d_quant, d_work_params, d_work_quant, d_coef, d_err);
  int rc = sgic::check_launch("jpeg_huff_kernel");
  if (rc) return rc;
  jpeg_idct_kernel<<<dim3(cdiv(max_blocks, 64), B), 64, 0, st>>>(d_work_params, d_coef, d_work_quant, d_planes, max_blocks);
  rc = sgic::check_launch("jpeg_idct_kernel");
  if (rc) return rc;
  const long px = (long)H * W;
  jpeg_color_kernel<<<dim3((unsigned)min((px + 255) / 256, 4096L), B), 256, 0, st>>>(d_work_params, d_planes, d_out, H, W);
  return sgic::check_launch("jpeg_color_kernel");
}

// Decode a batch of B JPEGs of equal geometry given as SCANS (progressive files, multi-scan sequential files, and baseline files as one
// sequential scan each) to RGB u8 HWC (B, H, W, 3).  d_descs: nscans x 32 int32 scan descriptors sorted by dependency level, level l
// being descriptors [h_level_start[l], h_level_start[l + 1]) (host array, nlevels + 1 entries); d_tabs: the batch's Huffman table pool
// (1424 B each).  Other arguments as sgic_jpeg_decode_batch; d_err[b]: 0 ok, 1 invalid Huffman code or DC size, 2 missing restart segment,
// 3 corrupt scan data: a coefficient past the end of its band, or the scan ended before its last unit (more bytes consumed than the
// unpadded length in descriptor slot 29).
extern "C" int sgic_jpeg_decode_scans_batch(const int32_t *d_params, const int32_t *d_descs, const uint8_t *d_scan, const uint8_t *d_tabs,
                                            const int32_t *d_segs, const uint16_t *d_quant, int32_t *d_work_params, uint16_t *d_work_quant,
                                            int16_t *d_coef, uint8_t *d_planes, uint8_t *d_out, int32_t *d_err, int B, int H, int W,
                                            long total_blocks, int max_blocks, const int32_t *h_level_start, int nlevels,
                                            sgic_stream_t stream) {
  SGIC_REQUIRE(d_params && d_descs && d_scan && d_tabs && d_segs && d_quant && d_work_params && d_work_quant && d_coef && d_planes && d_out &&
                   d_err && h_level_start, "null");
  SGIC_REQUIRE(B > 0 && H > 0 && W > 0 && max_blocks > 0 && total_blocks > 0 && nlevels > 0, "shape");
  SGIC_REQUIRE((((uintptr_t)d_scan | (uintptr_t)d_tabs | (uintptr_t)d_planes) & 15) == 0, "16-byte alignment");
  hipStream_t st = to_stream(stream);
  SGIC_HIP(hipMemsetAsync(d_coef, 0, (size_t)total_blocks * 64 * sizeof(int16_t), st));
  SGIC_HIP(hipMemsetAsync(d_err, 0, (size_t)B * sizeof(int32_t), st));
  for (int l = 0; l < nlevels; l++) {
    const int n = h_level_start[l + 1] - h_level_start[l];
    SGIC_REQUIRE(n > 0, "empty level");
    jpeg_scan_kernel<<<n, 64, 0, st>>>(d_params, d_descs + (size_t)h_level_start[l] * JPG_NS, d_scan, d_tabs, d_segs, d_quant,
                                       d_work_params, d_work_quant, d_coef, d_err);
    const int rc = sgic::check_launch("jpeg_scan_kernel");
    if (rc) return rc;
  }
  jpeg_idct_kernel<<<dim3(cdiv(max_blocks, 64), B), 64, 0, st>>>(d_work_params, d_coef, d_work_quant, d_planes, max_blocks);
  int rc = sgic::check_launch("jpeg_idct_kernel");
  if (rc) return rc;
  const long px = (long)H * W;
  jpeg_color_kernel<<<dim3((unsigned)min((px + 255) / 256, 4096L), B), 256, 0, st>>>(d_work_params, d_planes, d_out, H, W);
  return sgic::check_launch("jpeg_color_kernel");
}
