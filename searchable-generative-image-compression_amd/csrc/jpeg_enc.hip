// JPEG encode of a batch of B equal-geometry RGB u8 images (include/sgic.h): the entropy-coded bytes of the file that Pillow /
// libjpeg-turbo writes for the same pixels, quantisation tables and sampling layout, byte for byte.  Integer arithmetic only (jccolor,
// jcsample without smoothing, jfdctint islow, division by 8 q with rounding); DESIGN.md section 13 has the definition.  Three calls, one
// chain.  A call's mode says which tables code the file and which scans it has:
//   sgic_jpeg_encode_batch       ANNEX_K      save(...): one sequential scan, the Annex K Huffman tables
//   sgic_jpeg_encode_opt_batch   FITTED       save(..., optimize=True): one sequential scan, tables fitted to the image
//   sgic_jpeg_encode_prog_batch  PROGRESSIVE  save(..., progressive=True): the ten scans of libjpeg's jpeg_simple_progression, every
//                                             scan with tables fitted to it (section 13.3)
// The coefficients are made once; then every scan of the script runs the same passes over its own blocks, every pass parallel in
// 8 x 8 blocks or in bytes (send_block<K> says what a block sends in a scan of kind K; hist, bits and pack are its three sinks):
//   coef    one thread per coded block: colour, downsampling, edge replication, DCT, quantisation -> i16 coefficients in zigzag order
//   (AC scans only: flags, link, runs, next, round find the blocks that lead an end-of-band run; listed where they begin)
//   hist    fitted tables: one thread per block: the symbols its codes would use, counted in LDS, then added to the image's histograms
//   tables  fitted tables: one wavefront per (image, table): libjpeg's jpeg_gen_optimal_table -> code words, BITS and HUFFVAL
//   bits    one thread per block: its code length; a workgroup scan leaves offsets within 256 blocks and the sum of the 256
//   scan    one workgroup per image: exclusive scan of those sums (used again for the stuffing counts)
//   pack    one thread per block: its codes go to the zeroed bit stream; blocks share at most their first and last word, which take an
//           integer atomicOr (order-free, so two runs give the same bytes), words in between are plain stores
//   count   one workgroup per 4 KiB of the stream: the 0xFF bytes (the 1-bit padding of the last byte included)
//   emit    the same split: bytes move to their place in the slot behind the scans before them, a 0x00 follows every 0xFF; a
//           sequential file then gets FF D9; every scan writes its length, the last one the error word (two kernels: the
//           sequential file's and the progressive scan's)
#include <type_traits>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_GRID_Y = 32768;
constexpr int CHUNK_WORDS = NT * 4;        // words of the bit stream that a workgroup of count / emit takes at a time
constexpr int MAX_CHUNK_GRID = 1024;
constexpr int HUFF_BYTES = 272;            // BITS (16) and HUFFVAL (256, zeros after the table's symbols)

// The kinds of scan.  A sequential scan codes whole blocks (coefficients 0 .. 63, no end-of-band runs) in the MCU order of coef, dummy
// blocks included; the two DC kinds run over the same blocks; an AC scan runs over its component's raster without dummy blocks.
constexpr int K_SEQ = 0, K_DC_FIRST = 1, K_DC_REFINE = 2, K_AC_FIRST = 3, K_AC_REFINE = 4;
// Where bits and pack take the code words from: the Annex K tables (staged once per workgroup), the image's own (staged for every
// image of the loop), none (a DC refinement scan sends raw bits only)
constexpr int T_ANNEX_K = 0, T_IMAGE = 1, T_NONE = 2;
constexpr int NSCAN = 10;                 // scans of a progressive file
constexpr int EOBRUN_MAX = 0x7FFF;
constexpr unsigned CORR_BITS = 937;       // libjpeg's MAX_CORR_BITS - DCTSIZE2 + 1: a run is cut once its correction bits pass this
constexpr int EOBRUN_BITS = 16 + 14;      // the symbol and its extra bits
// The bits of a block in a scan at the most.  Sequential, in whole words: 20 + 63 * 26 = 1658 bits with the Annex K tables; with
// fitted tables any code may have 16 bits, so 16 + 11 + 63 * (16 + 10) = 1665.  Progressive: a DC difference of at most 11 bits; a
// refinement bit; in a first scan (10 - Al)-bit values behind 16-bit codes; in a refinement scan a code, a sign and no correction
// bit per coefficient at the most, three ZRL at the most
constexpr unsigned seq_bits(bool fitted) { return fitted ? 53 * 32 : 52 * 32; }
constexpr unsigned dc_first_bits() { return 16 + 11; }
constexpr unsigned ac_first_bits(int ss, int se, int al) { return (unsigned)(se - ss + 1) * (16 + 10 - al) + EOBRUN_BITS; }
constexpr unsigned ac_refine_bits(int ss, int se) { return (unsigned)(se - ss + 1) * 17 + 3 * 16 + EOBRUN_BITS; }
constexpr unsigned MAX_SCAN_BITS = ac_first_bits(1, 63, 1);       // the largest of the ten scans: chroma, 1 .. 63 at Al = 1
constexpr size_t MAX_SLOT_BYTES = 0x7fffffff;      // an image's slot, which d_len and cap count in 31 bits

// What a call's tables and scans are.  max_blocks: bit offsets within a scan of an image are 32-bit, so the coded blocks of an image
// times the largest per-block bound stay below 2^32.  limits, work, slots: the texts of its refusals
struct Mode {
  unsigned max_blocks;
  bool fitted, progressive;
  const char *limits, *work, *slots;
};
#define JPEG_ENC_GEOMETRY "1 <= B, 1 <= H, W <= 16384, subsampling 0, 1 or 2, at most "
constexpr Mode ANNEX_K{2581110, false, false, JPEG_ENC_GEOMETRY "2581110 coded blocks per image",
                       "the workspace is smaller than sgic_jpeg_encode_work_bytes says", "the slots are smaller than sgic_jpeg_encode_cap says"};
constexpr Mode FITTED{2579559, true, false, JPEG_ENC_GEOMETRY "2579559 coded blocks per image",
                      "the workspace is smaller than sgic_jpeg_encode_opt_work_bytes says",
                      "the slots are smaller than sgic_jpeg_encode_opt_cap says"};
constexpr Mode PROGRESSIVE{2675992, true, true, JPEG_ENC_GEOMETRY "2675992 coded blocks per image and a slot below 2^31 bytes",
                           "the workspace is smaller than sgic_jpeg_encode_prog_work_bytes says",
                           "the slots are smaller than sgic_jpeg_encode_prog_cap says"};
static_assert((unsigned long long)ANNEX_K.max_blocks * seq_bits(false) < (1ull << 32) && (unsigned long long)FITTED.max_blocks * 1665 < (1ull << 32) &&
              1665 <= seq_bits(true), "32-bit bit offsets within a sequential image");
static_assert(MAX_SCAN_BITS == 1605 && ac_first_bits(6, 63, 2) < MAX_SCAN_BITS && ac_refine_bits(1, 63) == 1149, "per-block bounds");
static_assert((unsigned long long)PROGRESSIVE.max_blocks * MAX_SCAN_BITS < (1ull << 32) &&
              (unsigned long long)(PROGRESSIVE.max_blocks + 1) * MAX_SCAN_BITS >= (1ull << 32), "32-bit bit offsets within a scan of an image");
static_assert((CORR_BITS + 1 + 62) / 63 == 15, "a segment that the correction bits cut holds at least 15 blocks");

constexpr int ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.3: BITS and HUFFVAL of the four typical tables
constexpr unsigned char DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// code << 8 | length by symbol: DC luma, DC chroma (12 each), AC luma, AC chroma (256 each; 0 where the table has no such symbol)
constexpr int TAB_DC = 0, TAB_AC = 24, TAB_WORDS = 24 + 512;
struct HuffTabs {
  uint32_t w[TAB_WORDS];
};

constexpr void fill_codes(uint32_t *dst, const unsigned char *bits, const unsigned char *vals) {
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) dst[vals[k++]] = (code++ << 8) | (unsigned)len;
    code <<= 1;
  }
}

constexpr HuffTabs make_tabs() {
  HuffTabs t{};
  fill_codes(t.w + TAB_DC, DC_LUMA_BITS, DC_VALS);
  fill_codes(t.w + TAB_DC + 12, DC_CHROMA_BITS, DC_VALS);
  fill_codes(t.w + TAB_AC, AC_LUMA_BITS, AC_LUMA_VALS);
  fill_codes(t.w + TAB_AC + 256, AC_CHROMA_BITS, AC_CHROMA_VALS);
  return t;
}

__constant__ HuffTabs kTabs = make_tabs();

struct EPlan {
  int B, H, W;
  int hs, vs;        // luma sampling factors; chroma is 1 x 1
  int mx, my;        // MCUs across and down
  int wb, hb;        // luma blocks that are not dummy blocks: ceil(W / 8) x ceil(H / 8)
  int ny, bpm;       // luma blocks and all blocks of an MCU
  int nblk;          // coded blocks of an image, dummy blocks included
  int nchunk;        // workgroups of NT blocks per image
  int nbchunk;       // CHUNK_WORDS pieces of an image's worst-case bit stream in its largest scan
};

struct Scan {
  int kind;
  int comp;          // AC scans: the component
  int ss, se, al;
  int tab;           // AC scans: the table's place in the table layout
  int slot;          // progressive: the scan's first table in d_huff / d_nval
  int ntab, tw[2];   // progressive: its tables and the wavefronts of jpeg_enc_tables_kernel that build them (0 DC 0, 1 AC 0, 2 DC 1, 3 AC 1)
  int n;             // blocks of the scan per image
  int nchunk;        // workgroups of NT blocks
  int rounds;
  unsigned bound;    // bits of a block at the most
  int nbchunk;
  size_t words;      // u32 words of one image's bit stream in this scan (a multiple of 4, one spare word for the last flush)
};

// The workspace as typed arrays, in their order in d_work; the arrays of other modes are empty.  Everything from zero to ffsum is
// zeroed by one memset: the byte positions of the scans in the slots (progressive), the histograms (fitted tables; zeroed again
// for every later scan), the bit streams of all scans
struct Work {
  int16_t *coef;
  uint16_t *qt;
  uint32_t *local, *csum, *tabs;
  uint8_t *blk, *mark;
  uint16_t *cnt;
  uint32_t *re, *pre, *next;      // next: two arrays of B x nblk
  int32_t *clast, *cfirst;
  uint32_t *ctb;
  uint8_t *huff4;                 // what jpeg_enc_tables_kernel writes for the progressive scan at hand
  int32_t *nval4;
  uint8_t *zero;
  unsigned long long *pos;
  uint32_t *hist, *bits[NSCAN], *ffsum, *tot;
};

struct Plan {
  EPlan e;
  int nscan;
  Scan scan[NSCAN];
  Work w;
  size_t bytes, cap;
};

// The plan of a call in mode m: the geometry, the script of scans (one sequential scan, or the ten of libjpeg's
// jpeg_simple_progression) and the workspace carved from d_work (null where only the sizes are asked for).  false: outside the
// mode's limits
bool make_plan(const Mode &m, int B, int H, int W, int sub, uint8_t *d_work, Plan *pl) {
  if (B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || sub < 0 || sub > 2) return false;
  EPlan &p = pl->e;
  p.B = B; p.H = H; p.W = W;
  p.hs = sub == 0 ? 1 : 2;
  p.vs = sub == 2 ? 2 : 1;
  p.mx = (W + 8 * p.hs - 1) / (8 * p.hs);
  p.my = (H + 8 * p.vs - 1) / (8 * p.vs);
  p.wb = (W + 7) / 8;
  p.hb = (H + 7) / 8;
  p.ny = p.hs * p.vs;
  p.bpm = p.ny + 2;
  const size_t nblk = (size_t)p.mx * p.my * p.bpm;
  if (nblk > m.max_blocks) return false;
  p.nblk = (int)nblk;
  p.nchunk = (int)((nblk + NT - 1) / NT);
  pl->nscan = m.progressive ? NSCAN : 1;
  // (kind, component, Ss, Se, Al, first table)
  const int sequential[6] = {K_SEQ, 0, 0, 63, 0, 0};
  const int progression[NSCAN][6] = {{K_DC_FIRST, 0, 0, 0, 1, 0},  {K_AC_FIRST, 0, 1, 5, 2, 2},   {K_AC_FIRST, 2, 1, 63, 1, 3},
                                     {K_AC_FIRST, 1, 1, 63, 1, 4}, {K_AC_FIRST, 0, 6, 63, 2, 5},  {K_AC_REFINE, 0, 1, 63, 1, 6},
                                     {K_DC_REFINE, 0, 0, 0, 0, 0}, {K_AC_REFINE, 2, 1, 63, 0, 7}, {K_AC_REFINE, 1, 1, 63, 0, 8},
                                     {K_AC_REFINE, 0, 1, 63, 0, 9}};
  pl->cap = 0;
  p.nbchunk = 0;
  for (int s = 0; s < pl->nscan; ++s) {
    const int *script = m.progressive ? progression[s] : sequential;
    Scan &sc = pl->scan[s];
    sc.kind = script[0]; sc.comp = script[1]; sc.ss = script[2]; sc.se = script[3]; sc.al = script[4]; sc.slot = script[5];
    sc.tab = TAB_AC + (sc.comp ? 256 : 0);
    // a sequential scan's four tables are written where the caller reads them; a progressive scan's move to their slots
    sc.ntab = sc.kind == K_DC_FIRST ? 2 : sc.kind >= K_AC_FIRST ? 1 : 0;
    sc.tw[0] = sc.kind == K_DC_FIRST ? 0 : sc.comp ? 3 : 1;
    sc.tw[1] = 2;
    sc.n = sc.kind < K_AC_FIRST ? p.nblk : sc.comp ? p.mx * p.my : p.wb * p.hb;
    sc.nchunk = (sc.n + NT - 1) / NT;
    sc.rounds = 0;
    if (sc.kind == K_AC_REFINE) {
      int k = 0;
      while (((size_t)15 << k) < (size_t)sc.n) ++k;
      sc.rounds = k + 1;
    }
    sc.bound = sc.kind == K_SEQ ? seq_bits(m.fitted) : sc.kind == K_DC_FIRST ? dc_first_bits() : sc.kind == K_DC_REFINE ? 1
               : sc.kind == K_AC_FIRST ? ac_first_bits(sc.ss, sc.se, sc.al) : ac_refine_bits(sc.ss, sc.se);
    sc.words = (((size_t)sc.n * sc.bound + 31) / 32 + 1 + 3) & ~(size_t)3;
    sc.nbchunk = (int)((sc.words + CHUNK_WORDS - 1) / CHUNK_WORDS);
    if (sc.nbchunk > p.nbchunk) p.nbchunk = sc.nbchunk;
    // every byte of a stream may be 0xFF and take a stuffed zero; a sequential file ends with FF D9
    pl->cap += sc.kind == K_SEQ ? (size_t)sc.n * (sc.bound / 4) + 2 : sc.words * 8;
  }
  if (pl->cap > MAX_SLOT_BYTES) return false;      // lengths and the caller's cap are 31-bit
  // every array starts on a multiple of 16 bytes; n: its elements per image
  size_t o = 0;
  auto take = [&o, d_work, B](auto *&array, size_t n) {
    array = reinterpret_cast<std::remove_reference_t<decltype(array)>>((uintptr_t)d_work + o);
    o += ((size_t)B * n * sizeof(*array) + 15) & ~(size_t)15;
  };
  const size_t fitted = m.fitted ? 1 : 0, runs = m.progressive ? 1 : 0;
  Work &w = pl->w;
  take(w.coef, nblk * 64);
  take(w.qt, 128);
  take(w.local, nblk);
  take(w.csum, p.nchunk);
  take(w.tabs, fitted * TAB_WORDS);
  take(w.blk, runs * nblk);
  take(w.mark, runs * nblk);
  take(w.cnt, runs * nblk);
  take(w.re, runs * nblk);
  take(w.pre, runs * (nblk + 1));
  take(w.next, runs * 2 * nblk);
  take(w.clast, runs * p.nchunk);
  take(w.cfirst, runs * p.nchunk);
  take(w.ctb, runs * p.nchunk);
  take(w.huff4, runs * 4 * HUFF_BYTES);
  take(w.nval4, runs * 4);
  w.zero = reinterpret_cast<uint8_t *>((uintptr_t)d_work + o);
  take(w.pos, runs * (NSCAN + 1));
  take(w.hist, fitted * TAB_WORDS);
  for (int s = 0; s < pl->nscan; ++s) take(w.bits[s], pl->scan[s].words);
  take(w.ffsum, p.nbchunk);
  take(w.tot, 2);
  pl->bytes = o;
  return true;
}

// block t of an image's scan -> component (0 luma, 1 Cb, 2 Cr) and block coordinates within the component; false for a dummy block
__device__ __forceinline__ bool block_of(const EPlan &p, int t, int &comp, int &bx, int &by) {
  const int mcu = t / p.bpm, k = t - mcu * p.bpm;
  const int my = mcu / p.mx, mx = mcu - my * p.mx;
  if (k < p.ny) {
    const int dy = k / p.hs, dx = k - dy * p.hs;
    comp = 0;
    bx = mx * p.hs + dx;
    by = my * p.vs + dy;
    return bx < p.wb && by < p.hb;
  }
  comp = 1 + k - p.ny;
  bx = mx;
  by = my;
  return true;
}

// one jfdctint pass over eight values: the row pass keeps 2 extra bits, the column pass removes them and the factor 8 stays
template <bool FIRST>
__device__ __forceinline__ void fdct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7) {
  constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d0 = (t10 + t11) << 2;
    d4 = (t10 - t11) << 2;
  } else {
    d0 = (t10 + t11 + 2) >> 2;
    d4 = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + R) >> N;
  d6 = (z1 - t12 * 15137 + R) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (a4 + z1 + z3 + R) >> N;
  d5 = (a5 + z2 + z4 + R) >> N;
  d3 = (a6 + z2 + z3 + R) >> N;
  d1 = (a7 + z1 + z4 + R) >> N;
}

__global__ __launch_bounds__(NT) void jpeg_enc_coef_kernel(const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ qt,
                                                           int16_t *__restrict__ coef, EPlan p) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= p.nblk) return;
  int comp, bx, by;
  if (!block_of(p, t, comp, bx, by)) return;
  // jccolor: 16 fractional bits
  const int kr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
  const int kg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
  const int kb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
  const int ka = comp == 0 ? 32768 : (128 << 16) + 32767;
  const int hsub = comp ? p.hs : 1, vsub = comp ? p.vs : 1;
  const int rows = (p.H + vsub - 1) / vsub;        // rows of the component that come from the image
  const int H = p.H, W = p.W;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const uint8_t *im = rgb + (size_t)img * H * W * 3;
    int ws[64];
    if (hsub * vsub == 1) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint8_t *row = im + (size_t)min(by * 8 + r, H - 1) * W * 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint8_t *px = row + min(bx * 8 + c, W - 1) * 3;
          ws[r * 8 + c] = ((kr * px[0] + kg * px[1] + kb * px[2] + ka) >> 16) - 128;
        }
      }
    } else {
      // 2 x 1 and 2 x 2 as one form: a row taken twice doubles the sum and the bias, and (2 s + 2 b) >> 2 == (s + b) >> 1
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int cy = min(by * 8 + r, rows - 1);
        const uint8_t *row0 = im + (size_t)min(cy * vsub, H - 1) * W * 3;
        const uint8_t *row1 = im + (size_t)min(cy * vsub + vsub - 1, H - 1) * W * 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int x0 = min((bx * 8 + c) * 2, W - 1) * 3, x1 = min((bx * 8 + c) * 2 + 1, W - 1) * 3;
          const int s = ((kr * row0[x0] + kg * row0[x0 + 1] + kb * row0[x0 + 2] + ka) >> 16) +
                        ((kr * row0[x1] + kg * row0[x1 + 1] + kb * row0[x1 + 2] + ka) >> 16) +
                        ((kr * row1[x0] + kg * row1[x0 + 1] + kb * row1[x0 + 2] + ka) >> 16) +
                        ((kr * row1[x1] + kg * row1[x1 + 1] + kb * row1[x1 + 2] + ka) >> 16);
          const int bias = vsub == 2 ? 1 + (c & 1) : 2 * (c & 1);
          ws[r * 8 + c] = ((s + bias) >> 2) - 128;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
      fdct8<true>(ws[r * 8], ws[r * 8 + 1], ws[r * 8 + 2], ws[r * 8 + 3], ws[r * 8 + 4], ws[r * 8 + 5], ws[r * 8 + 6], ws[r * 8 + 7]);
#pragma unroll
    for (int c = 0; c < 8; ++c)
      fdct8<false>(ws[c], ws[8 + c], ws[16 + c], ws[24 + c], ws[32 + c], ws[40 + c], ws[48 + c], ws[56 + c]);
    const uint16_t *q = qt + ((size_t)img * 2 + (comp ? 1 : 0)) * 64;
#pragma unroll
    for (int n = 0; n < 64; ++n) {
      const unsigned d = 8u * q[n];
      const int v = ws[n];
      const unsigned m = ((unsigned)abs(v) + (d >> 1)) / d;
      ws[n] = v < 0 ? -(int)m : (int)m;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(coef + ((size_t)img * p.nblk + t) * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint4 o;
      o.x = (unsigned)(ws[ZIGZAG[8 * j]] & 0xffff) | ((unsigned)ws[ZIGZAG[8 * j + 1]] << 16);
      o.y = (unsigned)(ws[ZIGZAG[8 * j + 2]] & 0xffff) | ((unsigned)ws[ZIGZAG[8 * j + 3]] << 16);
      o.z = (unsigned)(ws[ZIGZAG[8 * j + 4]] & 0xffff) | ((unsigned)ws[ZIGZAG[8 * j + 5]] << 16);
      o.w = (unsigned)(ws[ZIGZAG[8 * j + 6]] & 0xffff) | ((unsigned)ws[ZIGZAG[8 * j + 7]] << 16);
      dst[j] = o;
    }
  }
}

// the DC that block t's difference is taken from: the last block of its component before it in the scan that is no dummy block
// (a dummy block repeats the DC before it, so it passes that value on)
__device__ __forceinline__ int dc_before(const EPlan &p, const int16_t *__restrict__ coef, int t) {
  int mcu = t / p.bpm, k = t - mcu * p.bpm;
  if (k >= p.ny) return mcu ? coef[(size_t)(t - p.bpm) * 64] : 0;
  if (--k < 0) {
    if (mcu == 0) return 0;
    --mcu;
    k = p.ny - 1;
  }
  for (; k > 0; --k) {     // block 0 of an MCU is never a dummy block
    int comp, bx, by;
    if (block_of(p, mcu * p.bpm + k, comp, bx, by)) break;
  }
  return coef[(size_t)(mcu * p.bpm + k) * 64];
}

// A sink takes the symbols of a block from code_block: sym(i, extra, nb) is the symbol at word i of the table layout (TAB_DC / TAB_AC)
// followed by nb extra bits.
// The progressive walks also send bits that no symbol leads: raw(v, n), the low n <= 63 bits of v.
struct CountSink {
  const uint32_t *tab;
  unsigned bits;
  __device__ __forceinline__ void sym(int i, unsigned, int nb) { bits += (tab[i] & 0xff) + (unsigned)nb; }
  __device__ __forceinline__ void raw(unsigned long long, int n) { bits += (unsigned)n; }
};

// counts symbols instead of bits: hist is a workgroup's histogram in LDS, in the table layout
struct HistSink {
  unsigned *hist;
  __device__ __forceinline__ void sym(int i, unsigned, int) { atomicAdd(&hist[i], 1u); }
  __device__ __forceinline__ void raw(unsigned long long, int) {}
};

// MSB first: bit i of the stream is bit 31 - i % 32 of word i / 32
struct PackSink {
  const uint32_t *tab;
  uint32_t *words;
  unsigned wi;
  unsigned long long acc;
  int n;
  bool shared;      // the next word to leave may hold bits of the block before this one
  __device__ __forceinline__ void put(unsigned code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t w = (uint32_t)(acc >> n);
      if (shared) {
        atomicOr(&words[wi], w);
        shared = false;
      } else {
        words[wi] = w;
      }
      ++wi;
      acc &= (1ull << n) - 1;
    }
  }
  __device__ __forceinline__ void sym(int i, unsigned extra, int nb) {
    const uint32_t e = tab[i];
    put(((e >> 8) << nb) | extra, (int)(e & 0xff) + nb);
  }
  __device__ __forceinline__ void raw(unsigned long long v, int nb) {
    if (nb > 32) {
      put((unsigned)(v >> 32), nb - 32);
      put((unsigned)v, 32);
    } else if (nb) {
      put((unsigned)v, nb);
    }
  }
};

// for the walks of the AC run passes, which only look at what a block would send
struct NullSink {
  __device__ __forceinline__ void sym(int, unsigned, int) {}
  __device__ __forceinline__ void raw(unsigned long long, int) {}
};

// a block's 64 coefficients in zigzag order: 8 x uint4 of i16 pairs
__device__ __forceinline__ void load_block(uint4 (&c)[8], const int16_t *__restrict__ ci, int t) {
  const uint4 *src = reinterpret_cast<const uint4 *>(ci + (size_t)t * 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = src[j];
}

// coefficient k (a constant under unrolling) of a block in c
__device__ __forceinline__ int coef_of(const uint4 (&c)[8], int k) {
  const unsigned w = (k & 7) < 2 ? c[k >> 3].x : (k & 7) < 4 ? c[k >> 3].y : (k & 7) < 6 ? c[k >> 3].z : c[k >> 3].w;
  return (int)(short)((k & 1) ? (w >> 16) : (w & 0xffff));
}

// the symbols of one block of a sequential scan
template <typename Sink>
__device__ __forceinline__ void code_block(Sink &sink, const uint4 (&c)[8], int pred, int chroma) {
  const int dc = TAB_DC + 12 * chroma, ac = TAB_AC + 256 * chroma;
  const int diff = coef_of(c, 0) - pred;
  {
    const int nb = min(32 - __clz(abs(diff)), 11);
    sink.sym(dc + nb, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
  }
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int v = coef_of(c, k);
    if (v == 0) {
      ++run;
    } else {
      for (; run > 15; run -= 16) sink.sym(ac + 0xF0, 0, 0);
      const int nb = min(32 - __clz(abs(v)), 15);
      sink.sym(ac + ((run << 4) | nb), (unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), nb);
      run = 0;
    }
  }
  if (run) sink.sym(ac, 0, 0);
}

// the tables go to LDS: the Annex K ones, or (T_IMAGE) those that the tables pass has written for an image
template <int T>
__device__ __forceinline__ void stage_tabs(uint32_t *tab, const uint32_t *__restrict__ src) {
  for (int i = threadIdx.x; i < TAB_WORDS; i += NT) tab[i] = T == T_IMAGE ? src[i] : kTabs.w[i];
  __syncthreads();
}

// exclusive scan of one value per thread over the workgroup; *total: the sum.  red: NT / 64 words of LDS
__device__ __forceinline__ unsigned wg_exclusive_scan(unsigned v, unsigned *red, unsigned *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const unsigned s = red[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

// One workgroup per image: v[img][0 .. n) becomes its exclusive scan and tot[img * 2 + slot] the sum.  With from_bits, n is the
// number of CHUNK_WORDS pieces that hold the tot[img * 2] bits of the image (the pieces that the count pass has written).
__global__ __launch_bounds__(NT) void jpeg_enc_scan_kernel(uint32_t *__restrict__ v, int stride, int n, uint32_t *__restrict__ tot,
                                                           int slot, int from_bits, int B) {
  __shared__ unsigned red[NT / 64];
  for (int img = blockIdx.x; img < B; img += gridDim.x) {
    uint32_t *a = v + (size_t)img * stride;
    int cnt = n;
    if (from_bits) {
      const unsigned nbytes = (tot[(size_t)img * 2] >> 3) + ((tot[(size_t)img * 2] & 7) ? 1 : 0);
      cnt = (int)((nbytes + CHUNK_WORDS * 4 - 1) / (CHUNK_WORDS * 4));
    }
    unsigned carry = 0;
    for (int base = 0; base < cnt; base += NT) {
      const int i = base + threadIdx.x;
      const unsigned x = i < cnt ? a[i] : 0;
      unsigned total;
      const unsigned off = wg_exclusive_scan(x, red, &total);
      if (i < cnt) a[i] = carry + off;
      carry += total;
    }
    if (threadIdx.x == 0) tot[(size_t)img * 2 + slot] = carry;
  }
}

// key of a symbol for the two smallest counts: the lower count wins, on equal counts the larger symbol; no count: the largest key
__device__ __forceinline__ unsigned long long merge_key(unsigned count, int sym) {
  return count ? ((unsigned long long)count << 9) | (unsigned)(256 - sym) : ~0ull;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int d) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// the two smallest keys of the wave from every lane's two smallest (k1 <= k2), in every lane: one butterfly for c1 and c2 together
__device__ __forceinline__ void wave_min2(unsigned long long &k1, unsigned long long &k2) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o1 = shfl_xor_u64(k1, d), o2 = shfl_xor_u64(k2, d);
    const unsigned long long hi = k1 < o1 ? o1 : k1;
    k1 = min_u64(k1, o1);
    k2 = min_u64(hi, min_u64(k2, o2));
  }
}

constexpr int MAX_CLEN = 32;        // libjpeg's bound, where it ends with an error: a longer code needs counts in Fibonacci proportions
                                    // that sum past 9.2 million in one table.  Here the image's error word becomes 2.

// One wavefront per (image, table), the four tables of an image in one workgroup in the header's order DC0, AC0, DC1, AC1:
// jpeg_gen_optimal_table.  Lane l holds symbols l, l + 64, ..., l + 256 (the pseudo-symbol 256 with count 1 keeps the all-ones code
// free).  Every merge takes c1 and c2 from one wave reduction of the two smallest keys; a tree id per symbol makes it "size += 1, tree = c1" for the symbols
// of both trees.  The sizes go to LDS, where lane 0 counts them, limits the lengths to 16 and orders HUFFVAL; all lanes write out.
// tabs (B, TAB_WORDS): code << 8 | length per symbol, 0 for a symbol without code; huff (B, 4, HUFF_BYTES); nval (B, 4).
__global__ __launch_bounds__(NT) void jpeg_enc_tables_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ tabs,
                                                             uint8_t *__restrict__ huff, int32_t *__restrict__ nval, int B) {
  __shared__ uint8_t s_size[4][260];
  __shared__ uint8_t s_val[4][256];
  __shared__ uint32_t s_word[4][256];
  __shared__ int s_bits[4][MAX_CLEN + 2];
  __shared__ int s_start[4][MAX_CLEN + 2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nsym = (w & 1) ? 256 : 12;
  const int off = (w & 1) ? TAB_AC + 256 * (w >> 1) : TAB_DC + 12 * (w >> 1);
  for (int img = blockIdx.x; img < B; img += gridDim.x) {
    const uint32_t *hi = hist + (size_t)img * TAB_WORDS + off;
    unsigned count[5];
    int size[5], tree[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int s = lane + 64 * j;
      count[j] = s < nsym ? hi[s] : s == 256 ? 1u : 0u;
      size[j] = 0;
      tree[j] = s;
    }
    for (;;) {
      unsigned long long k1 = ~0ull, k2 = ~0ull;      // keys of different symbols differ, so "c2 over the remaining symbols" is the second smallest
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const unsigned long long k = merge_key(count[j], lane + 64 * j);
        k2 = min_u64(k2, k < k1 ? k1 : k);
        k1 = min_u64(k1, k);
      }
      wave_min2(k1, k2);
      if (k2 == ~0ull) break;      // one tree is left
      const int c1 = 256 - (int)(k1 & 511), c2 = 256 - (int)(k2 & 511);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int s = lane + 64 * j;
        if (s == c1) count[j] += (unsigned)(k2 >> 9);
        if (s == c2) count[j] = 0;
        if (tree[j] == c1 || tree[j] == c2) {
          ++size[j];
          tree[j] = c1;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (lane + 64 * j <= 256) s_size[w][lane + 64 * j] = (uint8_t)size[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_word[w][lane + 64 * j] = 0;
      s_val[w][lane + 64 * j] = 0;
    }
    __syncthreads();
    if (lane == 0) {
      int *bits = s_bits[w], *start = s_start[w];
      for (int i = 0; i <= MAX_CLEN + 1; ++i) bits[i] = 0;
      for (int s = 0; s <= 256; ++s) ++bits[min((int)s_size[w][s], MAX_CLEN + 1)];
      // HUFFVAL: by unlimited size, then by symbol; the pseudo-symbol has no place in it
      int n = 0;
      for (int i = 1; i <= MAX_CLEN; ++i) {
        start[i] = n;
        n += bits[i] - (s_size[w][256] == i ? 1 : 0);
      }
      for (int s = 0; s < 256; ++s) {
        const int i = s_size[w][s];
        if (i >= 1 && i <= MAX_CLEN) s_val[w][start[i]++] = (uint8_t)s;
      }
      // a code longer than MAX_CLEN bits before limiting: libjpeg ends with an error, here the count becomes -1, which the emit
      // pass turns into the image's error word; the limiter and the codes are left out (their counts would no longer add up)
      const bool too_long = bits[MAX_CLEN + 1] > 0;
      if (!too_long) {
        for (int i = MAX_CLEN; i > 16; --i) {
          while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2;
            bits[i - 1] += 1;
            bits[j + 1] += 2;
            bits[j] -= 1;
          }
        }
        int i = 16;
        while (bits[i] == 0) --i;
        --bits[i];
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
          for (int m = 0; m < bits[len]; ++m) s_word[w][s_val[w][k++]] = (code++ << 8) | (unsigned)len;
          code <<= 1;
        }
      }
      nval[(size_t)img * 4 + w] = too_long ? -1 : n;
    }
    __syncthreads();
    uint32_t *to = tabs + (size_t)img * TAB_WORDS + off;
    uint8_t *hb = huff + ((size_t)img * 4 + w) * HUFF_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = lane + 64 * j;
      if (s < nsym) to[s] = s_word[w][s];
      hb[16 + s] = s_val[w][s];
    }
    if (lane < 16) hb[lane] = (uint8_t)s_bits[w][lane + 1];
    __syncthreads();      // the next image's sizes overwrite what the lanes have just read
  }
}

// the four words of the stream at word index wi (a multiple of 4 below the image's word count), with the 1-bits that pad the last
// byte.  Bytes past the stream's end are zero: the words were zeroed and only coded bits were set.
__device__ __forceinline__ uint4 padded_words(const uint32_t *__restrict__ words, unsigned wi, unsigned tbits) {
  uint4 w = *reinterpret_cast<const uint4 *>(words + wi);
  if (tbits & 7) {
    const unsigned last = tbits >> 3;      // the byte that holds the last bits
    if ((last >> 2) - wi < 4) {
      const unsigned m = ((1u << (8 - (tbits & 7))) - 1) << (24 - 8 * (last & 3));
      const unsigned j = (last >> 2) - wi;
      if (j == 0) w.x |= m; else if (j == 1) w.y |= m; else if (j == 2) w.z |= m; else w.w |= m;
    }
  }
  return w;
}

__device__ __forceinline__ unsigned count_ff(unsigned w) {
  return (unsigned)((w >> 24) == 0xff) + (unsigned)(((w >> 16) & 0xff) == 0xff) + (unsigned)(((w >> 8) & 0xff) == 0xff) +
         (unsigned)((w & 0xff) == 0xff);
}

// bits: a scan's streams, nwords per image
__global__ __launch_bounds__(NT) void jpeg_enc_count_kernel(const uint32_t *__restrict__ bits, size_t nwords, const uint32_t *__restrict__ tot,
                                                            uint32_t *__restrict__ ffsum, EPlan p) {
  __shared__ unsigned red[NT / 64];
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const unsigned tbits = tot[(size_t)img * 2];
    const unsigned nbytes = (tbits >> 3) + ((tbits & 7) ? 1 : 0);
    const uint32_t *words = bits + (size_t)img * nwords;
    for (unsigned c = blockIdx.x; (size_t)c * CHUNK_WORDS * 4 < nbytes; c += gridDim.x) {
      const unsigned wi = c * CHUNK_WORDS + threadIdx.x * 4;
      unsigned n = 0;
      if ((size_t)wi * 4 < nbytes) {
        const uint4 w = padded_words(words, wi, tbits);
        n = count_ff(w.x) + count_ff(w.y) + count_ff(w.z) + count_ff(w.w);
      }
      unsigned total;
      wg_exclusive_scan(n, red, &total);
      if (threadIdx.x == 0) ffsum[(size_t)img * p.nbchunk + c] = total;
    }
  }
}

// the workgroup's chunks of one stream (words, tbits bits in nbytes bytes) go to slot, stuffed; ffs: the stream's 0xFF counts in front
// of every chunk; bytes at cap and beyond are left out
__device__ __forceinline__ void emit_stuffed(const uint32_t *__restrict__ words, unsigned tbits, unsigned nbytes,
                                             const uint32_t *__restrict__ ffs, uint8_t *__restrict__ slot, size_t cap, unsigned *red) {
  for (unsigned c = blockIdx.x; (size_t)c * CHUNK_WORDS * 4 < nbytes; c += gridDim.x) {
    const unsigned wi = c * CHUNK_WORDS + threadIdx.x * 4;
    const bool live = (size_t)wi * 4 < nbytes;
    uint4 w = make_uint4(0, 0, 0, 0);
    unsigned n = 0;
    if (live) {
      w = padded_words(words, wi, tbits);
      n = count_ff(w.x) + count_ff(w.y) + count_ff(w.z) + count_ff(w.w);
    }
    unsigned total;
    const unsigned before = wg_exclusive_scan(n, red, &total);
    if (live) {
      size_t o = (size_t)wi * 4 + ffs[c] + before;
      const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if ((size_t)wi * 4 + j < nbytes) {
          const unsigned byte = (ww[j >> 2] >> (24 - 8 * (j & 3))) & 0xff;
          if (o < cap) slot[o] = (uint8_t)byte;
          ++o;
          if (byte == 0xff) {
            if (o < cap) slot[o] = 0;
            ++o;
          }
        }
      }
    }
  }
}

// The emit pass of a sequential file: its one scan lies at the slot's start, then FF D9, the length and the error word.  bits: the
// scan's streams, nwords per image.  One kernel for both kinds of file measured slower here (profiles/jpeg_enc_refactor.txt), so
// the two share emit_stuffed only.
__global__ __launch_bounds__(NT) void jpeg_enc_emit_kernel(const uint32_t *__restrict__ bits, size_t nwords, const uint32_t *__restrict__ tot,
                                                           const uint32_t *__restrict__ ffsum, uint8_t *__restrict__ out, size_t cap,
                                                           int32_t *__restrict__ lens, int32_t *__restrict__ err,
                                                           const int32_t *__restrict__ nval, EPlan p) {
  __shared__ unsigned red[NT / 64];
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const unsigned tbits = tot[(size_t)img * 2];
    const unsigned nbytes = (tbits >> 3) + ((tbits & 7) ? 1 : 0);
    uint8_t *slot = out + (size_t)img * cap;
    emit_stuffed(bits + (size_t)img * nwords, tbits, nbytes, ffsum + (size_t)img * p.nbchunk, slot, cap, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const size_t len = (size_t)nbytes + tot[(size_t)img * 2 + 1] + 2;
      const bool fits = len <= cap;
      if (fits) {
        slot[len - 2] = 0xff;
        slot[len - 1] = 0xd9;
      }
      // nval (fitted tables only): a table whose count is negative had a code that libjpeg refuses, so there is no file
      const bool coded = !nval || (nval[(size_t)img * 4] | nval[(size_t)img * 4 + 1] | nval[(size_t)img * 4 + 2] | nval[(size_t)img * 4 + 3]) >= 0;
      lens[img] = fits && coded ? (int32_t)len : 0;
      err[img] = !coded ? 2 : fits ? 0 : 1;
    }
  }
}

// The emit pass of a progressive scan: its stuffed bytes follow those of the scans before it in the image's slot: pos (NSCAN + 1, B)
// holds where every scan begins.  lens (B, NSCAN).  The scan's tables move from where jpeg_enc_tables_kernel left them (huff4, nval4:
// four per image) to their slots of huff (B, NSCAN, HUFF_BYTES) and nval (B, NSCAN).  The last scan also sets the error word: 2 if a
// table had a code that libjpeg refuses, 1 if the slot was too small; the image's lengths are then zero.
__global__ __launch_bounds__(NT) void jpeg_enc_prog_emit_kernel(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ tot,
                                                                const uint32_t *__restrict__ ffsum, uint8_t *__restrict__ out, size_t cap,
                                                                int32_t *__restrict__ lens, int32_t *__restrict__ err,
                                                                const uint8_t *__restrict__ huff4, const int32_t *__restrict__ nval4,
                                                                uint8_t *__restrict__ huff, int32_t *__restrict__ nval,
                                                                unsigned long long *__restrict__ pos, int scan, EPlan p, Scan s) {
  __shared__ unsigned red[NT / 64];
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const unsigned tbits = tot[(size_t)img * 2];
    const unsigned nbytes = (tbits >> 3) + ((tbits & 7) ? 1 : 0);
    const unsigned long long at = pos[(size_t)scan * p.B + img];
    const size_t room = at < cap ? cap - (size_t)at : 0;
    emit_stuffed(bits + (size_t)img * s.words, tbits, nbytes, ffsum + (size_t)img * p.nbchunk, out + (size_t)img * cap + (cap - room), room, red);
    if (blockIdx.x == 0) {
      for (int j = 0; j < s.ntab; ++j) {
        const uint8_t *src = huff4 + ((size_t)img * 4 + s.tw[j]) * HUFF_BYTES;
        uint8_t *dst = huff + ((size_t)img * NSCAN + s.slot + j) * HUFF_BYTES;
        for (int b = threadIdx.x; b < HUFF_BYTES; b += NT) dst[b] = src[b];
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      for (int j = 0; j < s.ntab; ++j) nval[(size_t)img * NSCAN + s.slot + j] = nval4[(size_t)img * 4 + s.tw[j]];
      const unsigned long long len = (unsigned long long)nbytes + tot[(size_t)img * 2 + 1], end = at + len;
      pos[(size_t)(scan + 1) * p.B + img] = end;
      lens[(size_t)img * NSCAN + scan] = (int32_t)len;
      if (scan == NSCAN - 1) {
        bool coded = true;
        for (int j = 0; j < NSCAN; ++j) coded = coded && nval[(size_t)img * NSCAN + j] >= 0;
        const bool fits = end <= cap;
        if (!fits || !coded)
          for (int j = 0; j < NSCAN; ++j) lens[(size_t)img * NSCAN + j] = 0;
        err[img] = !coded ? 2 : fits ? 0 : 1;
      }
    }
  }
}

// ---- what a block sends in a scan; the passes that find an AC scan's end-of-band runs ------------------------------------------------
// An AC scan's end-of-band runs span blocks, so three or more passes in front of its chain say which blocks lead an EOBRUN symbol:
//   flags  one thread per block: does it code a coefficient (nz), does it end in zeros or pending correction bits (tail), how many
//          correction bits trail it; per workgroup the last and the first nz block and the sum of those bits
//   link   one workgroup per image: the last nz block in front of every workgroup, the first one behind it, the bits in front of it
//   runs   one thread per block: the run it lies in (from the nz block in front of it to the one behind it).  First scans: the heads
//          are every 0x7FFF blocks from the run's start.  Refinement scans: prefix sums of the correction bits, the run starts
//   next   refinement: the head that follows if this block is one (binary search in the prefix sums: 0x7FFF blocks or 937 bits)
//   round  refinement: every marked head marks its successor, then next := next o next; ceil(log2(n / 15)) + 1 rounds mark all

// block i of a scan -> its place in coef
template <int K>
__device__ __forceinline__ int scan_block(const EPlan &p, const Scan &s, int i) {
  if (K < K_AC_FIRST) return i;
  if (s.comp) return i * p.bpm + p.ny + s.comp - 1;
  const int by = i / p.wb, bx = i - by * p.wb;
  return ((by / p.vs) * p.mx + bx / p.hs) * p.bpm + (by % p.vs) * p.hs + bx % p.hs;
}

// A first AC scan's symbols of one block without its EOBRUN: -> tail (the band ends in zeros); nz: a coefficient was coded
template <typename Sink>
__device__ __forceinline__ bool walk_ac_first(Sink &sink, const uint4 (&c)[8], const Scan &s, bool &nz) {
  int run = 0;
  nz = false;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    if (k < s.ss || k > s.se) continue;
    const int v = coef_of(c, k);
    const int a = abs(v) >> s.al;
    if (a == 0) {
      ++run;
      continue;
    }
    nz = true;
    for (; run > 15; run -= 16) sink.sym(s.tab + 0xF0, 0, 0);
    const int nb = 32 - __clz(a);
    sink.sym(s.tab + ((run << 4) | nb), (unsigned)(v < 0 ? ~a : a) & ((1u << nb) - 1), nb);
    run = 0;
  }
  return run > 0;
}

// A refinement AC scan's symbols of one block without its EOBRUN and without the nbr correction bits br that trail it:
// -> tail (zeros or correction bits are pending at the band's end); nz: a symbol was coded
template <typename Sink>
__device__ __forceinline__ bool walk_ac_refine(Sink &sink, const uint4 (&c)[8], const Scan &s, bool &nz, unsigned long long &br, int &nbr) {
  // one pass over the coefficients leaves four masks by position: non-zero, becomes non-zero in this scan, negative, correction bit
  unsigned long long nonzero = 0, one = 0, neg = 0, low = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    if (k < s.ss || k > s.se) continue;
    const int v = coef_of(c, k);
    const int a = abs(v) >> s.al;
    const unsigned long long bit = 1ull << k;
    if (a) nonzero |= bit;
    if (a == 1) one |= bit;
    if (v < 0) neg |= bit;
    if (a & 1) low |= bit;
  }
  const int eob = one ? 63 - __clzll(one) : 0;      // the last coefficient that becomes non-zero in this scan
  int run = 0;
  nz = false;
  br = 0;
  nbr = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    if (k < s.ss || k > s.se) continue;
    const unsigned long long bit = 1ull << k;
    if (!(nonzero & bit)) {
      ++run;
      continue;
    }
    while (run > 15 && k <= eob) {
      sink.sym(s.tab + 0xF0, 0, 0);
      sink.raw(br, nbr);
      run -= 16;
      br = 0;
      nbr = 0;
      nz = true;
    }
    if (!(one & bit)) {
      br = (br << 1) | ((low >> k) & 1);
      ++nbr;
      continue;
    }
    sink.sym(s.tab + ((run << 4) | 1), (neg & bit) ? 0u : 1u, 1);
    sink.raw(br, nbr);
    run = 0;
    br = 0;
    nbr = 0;
    nz = true;
  }
  return run > 0 || nbr > 0;
}

// Everything block i of a scan of kind K sends, in stream order.  Sequential: the whole block; a dummy block is a zero DC difference
// and EOB in the luma tables.  AC scans: the block's own symbols, the EOBRUN symbol if it heads a segment of head blocks, its
// trailing correction bits.  ci: the image's coefficients.
template <int K, typename Sink>
__device__ __forceinline__ void send_block(Sink &sink, const EPlan &p, const Scan &s, const int16_t *__restrict__ ci, int i, unsigned head) {
  const int t = scan_block<K>(p, s, i);
  if (K == K_SEQ) {
    int comp, bx, by;
    if (block_of(p, t, comp, bx, by)) {
      uint4 c[8];
      load_block(c, ci, t);
      code_block(sink, c, dc_before(p, ci, t), comp ? 1 : 0);
    } else {
      sink.sym(TAB_DC, 0, 0);
      sink.sym(TAB_AC, 0, 0);
    }
    return;
  }
  if (K == K_DC_FIRST || K == K_DC_REFINE) {
    int comp, bx, by;
    const bool real = block_of(p, t, comp, bx, by);
    const int before = dc_before(p, ci, t);
    if (K == K_DC_FIRST) {
      // a dummy block repeats the DC before it: difference 0 in the luma table
      const int diff = real ? ((int)ci[(size_t)t * 64] >> s.al) - (before >> s.al) : 0;
      const int nb = min(32 - __clz(abs(diff)), 11);
      sink.sym(TAB_DC + (real && comp ? 12 : 0) + nb, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
    } else {
      sink.raw((unsigned)(((real ? (int)ci[(size_t)t * 64] : before) >> s.al) & 1), 1);
    }
    return;
  }
  uint4 c[8];
  load_block(c, ci, t);
  bool nz;
  unsigned long long br = 0;
  int nbr = 0;
  if (K == K_AC_FIRST)
    walk_ac_first(sink, c, s, nz);
  else
    walk_ac_refine(sink, c, s, nz, br, nbr);
  if (head) {
    const int n = 31 - __clz(head);
    sink.sym(s.tab + (n << 4), head & ((1u << n) - 1), n);
  }
  if (K == K_AC_REFINE) sink.raw(br, nbr);
}

// blk (B, nblk): nz | tail << 1 | trailing correction bits << 2 of every block of the scan; clast, cfirst, ctb (B, p.nchunk): the
// workgroup's last nz block (-1: none), its first (s.n: none), the sum of its trailing bits
template <bool REFINE>
__global__ __launch_bounds__(NT) void jpeg_enc_prog_flags_kernel(const int16_t *__restrict__ coef, uint8_t *__restrict__ blk,
                                                                 int32_t *__restrict__ clast, int32_t *__restrict__ cfirst,
                                                                 uint32_t *__restrict__ ctb, EPlan p, Scan s) {
  __shared__ unsigned red[NT / 64];
  __shared__ int s_last, s_first;
  const int i = blockIdx.x * NT + threadIdx.x;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    if (threadIdx.x == 0) {
      s_last = -1;
      s_first = s.n;
    }
    __syncthreads();
    int nbr = 0;
    if (i < s.n) {
      uint4 c[8];
      load_block(c, coef + (size_t)img * p.nblk * 64, scan_block<K_AC_FIRST>(p, s, i));
      NullSink sink;
      bool nz, tail;
      unsigned long long br;
      if (REFINE)
        tail = walk_ac_refine(sink, c, s, nz, br, nbr);
      else
        tail = walk_ac_first(sink, c, s, nz);
      blk[(size_t)img * p.nblk + i] = (uint8_t)((nz ? 1 : 0) | (tail ? 2 : 0) | (nbr << 2));
      if (nz) {
        atomicMax(&s_last, i);
        atomicMin(&s_first, i);
      }
    }
    unsigned total;
    wg_exclusive_scan((unsigned)nbr, red, &total);      // its barriers also end the atomics above
    if (threadIdx.x == 0) {
      clast[(size_t)img * p.nchunk + blockIdx.x] = s_last;
      cfirst[(size_t)img * p.nchunk + blockIdx.x] = s_first;
      ctb[(size_t)img * p.nchunk + blockIdx.x] = total;
    }
    __syncthreads();
  }
}

// exclusive maximum scan of one value per thread over the workgroup, none standing for "no value"; *total: the maximum
__device__ __forceinline__ int wg_exclusive_max(int v, int none, int *red, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = max(inc, o);
  }
  const int prev = __shfl_up(inc, 1, 64);
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int before = none, all = none;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int r = red[w];
    if (w < wave) before = max(before, r);
    all = max(all, r);
  }
  __syncthreads();
  *total = all;
  return lane ? max(before, prev) : before;
}

// One workgroup per image, over the n workgroups of the flags pass: clast becomes the last nz block in front of the workgroup (-1),
// cfirst the first one behind it (nblocks), ctb the trailing bits in front of it
__global__ __launch_bounds__(NT) void jpeg_enc_prog_link_kernel(int32_t *__restrict__ clast, int32_t *__restrict__ cfirst,
                                                                uint32_t *__restrict__ ctb, int stride, int n, int nblocks, int B) {
  __shared__ unsigned red[NT / 64];
  __shared__ int redi[NT / 64];
  for (int img = blockIdx.x; img < B; img += gridDim.x) {
    int32_t *la = clast + (size_t)img * stride, *fi = cfirst + (size_t)img * stride;
    uint32_t *tb = ctb + (size_t)img * stride;
    int last = -1, first = -nblocks;      // first: the negated minimum, so that it is a maximum scan from the back
    unsigned bits = 0;
    for (int base = 0; base < n; base += NT) {
      const int i = base + threadIdx.x, j = n - 1 - i;
      const int x = i < n ? la[i] : -1, y = i < n ? -fi[j] : -nblocks;
      const unsigned z = i < n ? tb[i] : 0;
      int xt, yt;
      unsigned zt;
      const int xe = wg_exclusive_max(x, -1, redi, &xt), ye = wg_exclusive_max(y, -nblocks, redi, &yt);
      const unsigned ze = wg_exclusive_scan(z, red, &zt);
      if (i < n) {
        la[i] = max(last, xe);
        fi[j] = -max(first, ye);
        tb[i] = bits + ze;
      }
      last = max(last, xt);
      first = max(first, yt);
      bits += zt;
    }
  }
}

// One thread per block of an AC scan: the run it lies in.  mark: first scans, the block heads a segment; refinement scans, it starts a
// run.  cnt: first scans, the blocks from here to the segment's end.  re: refinement scans, the run's end (0: the block is in no run).
// pre (B, nblk + 1): refinement scans, the trailing bits in front of every block of the scan and their sum.
template <bool REFINE>
__global__ __launch_bounds__(NT) void jpeg_enc_prog_runs_kernel(const uint8_t *__restrict__ blk, const int32_t *__restrict__ clast,
                                                                const int32_t *__restrict__ cfirst, const uint32_t *__restrict__ ctb,
                                                                uint8_t *__restrict__ mark, uint16_t *__restrict__ cnt,
                                                                uint32_t *__restrict__ re, uint32_t *__restrict__ pre, EPlan p, Scan s) {
  __shared__ unsigned long long masks[NT / 64];
  __shared__ unsigned red[NT / 64];
  const int i = blockIdx.x * NT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const uint8_t *bi = blk + (size_t)img * p.nblk;
    const size_t cb = (size_t)img * p.nchunk + blockIdx.x;
    const unsigned f = i < s.n ? bi[i] : 0;
    const bool nz = f & 1;
    const unsigned long long mask = __ballot(nz);
    if (lane == 0) masks[wave] = mask;
    __syncthreads();
    // the last nz block at or in front of i, the first one behind i
    int last = clast[cb], next = cfirst[cb];
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      const unsigned long long m = masks[w];
      if (w < wave && m) last = blockIdx.x * NT + w * 64 + 63 - __clzll(m);
    }
#pragma unroll
    for (int w = NT / 64 - 1; w >= 0; --w) {
      const unsigned long long m = masks[w];
      if (w > wave && m) next = blockIdx.x * NT + w * 64 + __ffsll(m) - 1;
    }
    const unsigned long long upto = lane == 63 ? mask : mask & ((2ull << lane) - 1), behind = lane == 63 ? 0ull : mask >> (lane + 1);
    if (upto) last = blockIdx.x * NT + wave * 64 + 63 - __clzll(upto);
    if (behind) next = i + __ffsll(behind);
    // an nz block with a tail starts a run; other blocks follow the nz block in front of them, which starts their run if it has a tail
    const bool inrun = !nz || (f & 2);
    int start = i;
    if (!nz) start = last < 0 ? 0 : (bi[last] & 2) ? last : last + 1;
    if (REFINE) {
      unsigned total;
      const unsigned off = ctb[cb] + wg_exclusive_scan(f >> 2, red, &total);
      if (i < s.n) {
        uint32_t *pi = pre + (size_t)img * (p.nblk + 1);
        pi[i] = off;
        if (i == s.n - 1) pi[s.n] = off + (f >> 2);
        re[(size_t)img * p.nblk + i] = inrun ? (uint32_t)next : 0u;
        mark[(size_t)img * p.nblk + i] = inrun && start == i;
      }
    } else if (i < s.n) {
      mark[(size_t)img * p.nblk + i] = inrun && (i - start) % EOBRUN_MAX == 0;
      cnt[(size_t)img * p.nblk + i] = (uint16_t)min(EOBRUN_MAX, next - i);
    }
    __syncthreads();
  }
}

// Refinement scans, one thread per block in a run: the segment from it ends with the block that fills EOBRUN_MAX or takes the
// correction bits past CORR_BITS, at the run's end at the latest.  cnt: its blocks; next: the head behind it, s.n if the run ends.
__global__ __launch_bounds__(NT) void jpeg_enc_prog_next_kernel(const uint32_t *__restrict__ re, const uint32_t *__restrict__ pre,
                                                                uint16_t *__restrict__ cnt, uint32_t *__restrict__ next, EPlan p, Scan s) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= s.n) return;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const int end = (int)re[(size_t)img * p.nblk + i];
    int c = 0, nx = s.n;
    if (end) {
      const uint32_t *pi = pre + (size_t)img * (p.nblk + 1);
      const unsigned t0 = pi[i];
      int lo = i, hi = min(end, i + EOBRUN_MAX) - 1;       // the segment's last block lies in [lo, hi]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pi[mid + 1] - t0 > CORR_BITS) hi = mid; else lo = mid + 1;
      }
      c = lo + 1 - i;
      if (lo + 1 < end) nx = lo + 1;
    }
    cnt[(size_t)img * p.nblk + i] = (uint16_t)c;
    next[(size_t)img * p.nblk + i] = (uint32_t)nx;
  }
}

// One doubling round: a marked block marks the head `from` names, and to = from o from.  mark is read and written in the same
// launch without atomics: the only writes are byte stores of the constant 1, to bytes that are heads.  A mark that appears while the
// round runs is a head too, so it may or may not act in this round: the marks after the last round are the same.
__global__ __launch_bounds__(NT) void jpeg_enc_prog_round_kernel(const uint32_t *__restrict__ from, uint32_t *__restrict__ to,
                                                                 uint8_t *mark, EPlan p, Scan s) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= s.n) return;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    const size_t o = (size_t)img * p.nblk;
    const uint32_t nx = from[o + i];
    uint32_t nn = (uint32_t)s.n;
    if (nx < (uint32_t)s.n) {
      if (mark[o + i]) mark[o + nx] = 1;
      nn = from[o + nx];
    }
    to[o + i] = nn;
  }
}

// the blocks of the segment that block `at` of an AC scan heads; 0: it heads none.  The other kinds have no segments
template <int K>
__device__ __forceinline__ unsigned head_of(const uint8_t *__restrict__ mark, const uint16_t *__restrict__ cnt, size_t at) {
  if (K < K_AC_FIRST) return 0u;
  return mark[at] ? cnt[at] : 0u;
}

// ---- the chain of a scan: hist, tables, bits, scan, pack, count, scan, emit --------------------------------------------------------
// One thread per block of the scan counts the symbols that its codes use in the workgroup's histogram, which then joins the
// image's: hist (B, TAB_WORDS), zeroed by the call for this scan.  Integer atomics in LDS and in memory are order-free, so two runs
// give the same counts.
template <int K>
__global__ __launch_bounds__(NT) void jpeg_enc_hist_kernel(const int16_t *__restrict__ coef, const uint8_t *__restrict__ mark,
                                                           const uint16_t *__restrict__ cnt, uint32_t *__restrict__ hist, EPlan p, Scan s) {
  __shared__ unsigned h[TAB_WORDS];
  const int i = blockIdx.x * NT + threadIdx.x;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    for (int j = threadIdx.x; j < TAB_WORDS; j += NT) h[j] = 0;
    __syncthreads();
    if (i < s.n) {
      HistSink sink{h};
      send_block<K>(sink, p, s, coef + (size_t)img * p.nblk * 64, i, head_of<K>(mark, cnt, (size_t)img * p.nblk + i));
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TAB_WORDS; j += NT)
      if (h[j]) atomicAdd(&hist[(size_t)img * TAB_WORDS + j], h[j]);
    __syncthreads();
  }
}

// T: where the code words come from; T_IMAGE: tabs (B, TAB_WORDS)
template <int K, int T>
__global__ __launch_bounds__(NT) void jpeg_enc_bits_kernel(const int16_t *__restrict__ coef, const uint32_t *__restrict__ tabs,
                                                           const uint8_t *__restrict__ mark, const uint16_t *__restrict__ cnt,
                                                           uint32_t *__restrict__ local, uint32_t *__restrict__ csum, EPlan p, Scan s) {
  __shared__ uint32_t tab[TAB_WORDS];
  __shared__ unsigned red[NT / 64];
  if (T == T_ANNEX_K) stage_tabs<T>(tab, nullptr);
  const int i = blockIdx.x * NT + threadIdx.x;
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    if (T == T_IMAGE) stage_tabs<T>(tab, tabs + (size_t)img * TAB_WORDS);     // the scan below ends with a barrier, so nobody still reads tab
    CountSink sink{tab, 0};
    if (i < s.n) send_block<K>(sink, p, s, coef + (size_t)img * p.nblk * 64, i, head_of<K>(mark, cnt, (size_t)img * p.nblk + i));
    unsigned total;
    const unsigned off = wg_exclusive_scan(sink.bits, red, &total);
    if (i < s.n) local[(size_t)img * p.nblk + i] = off;
    if (threadIdx.x == 0) csum[(size_t)img * p.nchunk + blockIdx.x] = total;
  }
}

// bits: the scan's zeroed streams (B, s.words)
template <int K, int T>
__global__ __launch_bounds__(NT) void jpeg_enc_pack_kernel(const int16_t *__restrict__ coef, const uint32_t *__restrict__ tabs,
                                                           const uint8_t *__restrict__ mark, const uint16_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ local, const uint32_t *__restrict__ csum,
                                                           uint32_t *__restrict__ bits, EPlan p, Scan s) {
  __shared__ uint32_t tab[TAB_WORDS];
  if (T == T_ANNEX_K) stage_tabs<T>(tab, nullptr);
  const int i = blockIdx.x * NT + threadIdx.x;
  if (T != T_IMAGE && i >= s.n) return;      // with T_IMAGE every thread stays for the barriers of the image loop
  for (int img = blockIdx.y; img < p.B; img += gridDim.y) {
    if (T == T_IMAGE) {
      __syncthreads();                    // the image before this one has been coded from tab
      stage_tabs<T>(tab, tabs + (size_t)img * TAB_WORDS);
    }
    if (i >= s.n) continue;
    const unsigned pos = csum[(size_t)img * p.nchunk + blockIdx.x] + local[(size_t)img * p.nblk + i];
    // the bits of the word in front of this block count as zeros of the accumulator, so that whole words leave it
    PackSink sink{tab, bits + (size_t)img * s.words, pos >> 5, 0ull, (int)(pos & 31), true};
    send_block<K>(sink, p, s, coef + (size_t)img * p.nblk * 64, i, head_of<K>(mark, cnt, (size_t)img * p.nblk + i));
    if (sink.n) atomicOr(&sink.words[sink.wi], (uint32_t)(sink.acc << (32 - sink.n)));
  }
}

// the checks that the three batch calls share; d_huff and d_nval are required where the mode fits tables
int check_args(const char *name, const Mode &m, const Plan &pl, const uint8_t *d_rgb, const uint16_t *h_qt, const uint8_t *d_work,
               size_t work_bytes, const uint8_t *d_out, size_t cap, const int32_t *d_len, const int32_t *d_err, const uint8_t *d_huff,
               const int32_t *d_nval) {
  SGIC_REQUIRE_AS(name, d_rgb && h_qt && d_work && d_out && d_len && d_err && (!m.fitted || (d_huff && d_nval)), "null pointer");
  SGIC_REQUIRE_AS(name, ((uintptr_t)d_work & 15) == 0, "the workspace must be 16-byte aligned");
  SGIC_REQUIRE_AS(name, ((uintptr_t)h_qt & 1) == 0 && ((uintptr_t)d_len & 3) == 0 && ((uintptr_t)d_err & 3) == 0 &&
                            ((uintptr_t)d_huff & 3) == 0 && ((uintptr_t)d_nval & 3) == 0, "misaligned pointer");
  SGIC_REQUIRE_AS(name, work_bytes >= pl.bytes, m.work);
  SGIC_REQUIRE_AS(name, cap >= pl.cap && cap <= 0x7fffffff, m.slots);
  for (size_t i = 0; i < (size_t)pl.e.B * 128; ++i) SGIC_REQUIRE_AS(name, h_qt[i] >= 1 && h_qt[i] <= 255, "a quantisation table entry outside [1, 255]");
  return SGIC_OK;
}

// hist and tables (fitted tables only), bits, scan and pack of one scan.  The tables kernel always builds four tables per image: a
// progressive scan's symbols are counted where its layout has the table, the other histograms stay zero and give empty tables.
// huff, nval: where it leaves BITS, HUFFVAL and the symbol counts
template <int K, int T>
void launch_chain(const EPlan &p, const Scan &sc, dim3 grid, unsigned gy, const Work &w, uint8_t *huff, int32_t *nval, uint32_t *bits,
                  hipStream_t st) {
  if constexpr (T == T_IMAGE) {
    jpeg_enc_hist_kernel<K><<<grid, NT, 0, st>>>(w.coef, w.mark, w.cnt, w.hist, p, sc);
    jpeg_enc_tables_kernel<<<gy, NT, 0, st>>>(w.hist, w.tabs, huff, nval, p.B);
  }
  jpeg_enc_bits_kernel<K, T><<<grid, NT, 0, st>>>(w.coef, w.tabs, w.mark, w.cnt, w.local, w.csum, p, sc);
  jpeg_enc_scan_kernel<<<gy, NT, 0, st>>>(w.csum, p.nchunk, sc.nchunk, w.tot, 0, 0, p.B);
  jpeg_enc_pack_kernel<K, T><<<grid, NT, 0, st>>>(w.coef, w.tabs, w.mark, w.cnt, w.local, w.csum, bits, p, sc);
}

// The three batch calls: the plan of the mode, the checks, then the coefficients and the chain of every scan of the script
int encode(const char *name, const Mode &m, const uint8_t *d_rgb, int B, int H, int W, int sub, const uint16_t *h_qt, uint8_t *d_work,
           size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err, uint8_t *d_huff, int32_t *d_nval,
           sgic_stream_t stream) {
  Plan pl;
  SGIC_REQUIRE_AS(name, make_plan(m, B, H, W, sub, d_work, &pl), m.limits);
  if (const int rc = check_args(name, m, pl, d_rgb, h_qt, d_work, work_bytes, d_out, cap, d_len, d_err, d_huff, d_nval)) return rc;
  const EPlan &p = pl.e;
  const Work &w = pl.w;
  hipStream_t st = to_stream(stream);
  SGIC_HIP(hipMemcpyAsync(w.qt, h_qt, (size_t)B * 128 * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  SGIC_HIP(hipMemsetAsync(w.zero, 0, (size_t)(reinterpret_cast<uint8_t *>(w.ffsum) - w.zero), st));
  const unsigned gy = B < MAX_GRID_Y ? B : MAX_GRID_Y;
  jpeg_enc_coef_kernel<<<dim3(p.nchunk, gy), NT, 0, st>>>(d_rgb, w.qt, w.coef, p);
  // a sequential call's four tables are the caller's; a progressive scan's go to scratch, from where the emit pass moves them
  uint8_t *huff = m.progressive ? w.huff4 : d_huff;
  int32_t *nval = m.progressive ? w.nval4 : d_nval;
  for (int k = 0; k < pl.nscan; ++k) {
    const Scan &sc = pl.scan[k];
    const dim3 grid(sc.nchunk, gy), gbytes(sc.nbchunk < MAX_CHUNK_GRID ? sc.nbchunk : MAX_CHUNK_GRID, gy);
    if (k && sc.kind != K_DC_REFINE) SGIC_HIP(hipMemsetAsync(w.hist, 0, (size_t)B * TAB_WORDS * sizeof(uint32_t), st));
    uint32_t *bits = w.bits[k];
    if (sc.kind == K_AC_FIRST) {
      jpeg_enc_prog_flags_kernel<false><<<grid, NT, 0, st>>>(w.coef, w.blk, w.clast, w.cfirst, w.ctb, p, sc);
      jpeg_enc_prog_link_kernel<<<gy, NT, 0, st>>>(w.clast, w.cfirst, w.ctb, p.nchunk, sc.nchunk, sc.n, B);
      jpeg_enc_prog_runs_kernel<false><<<grid, NT, 0, st>>>(w.blk, w.clast, w.cfirst, w.ctb, w.mark, w.cnt, w.re, w.pre, p, sc);
    } else if (sc.kind == K_AC_REFINE) {
      jpeg_enc_prog_flags_kernel<true><<<grid, NT, 0, st>>>(w.coef, w.blk, w.clast, w.cfirst, w.ctb, p, sc);
      jpeg_enc_prog_link_kernel<<<gy, NT, 0, st>>>(w.clast, w.cfirst, w.ctb, p.nchunk, sc.nchunk, sc.n, B);
      jpeg_enc_prog_runs_kernel<true><<<grid, NT, 0, st>>>(w.blk, w.clast, w.cfirst, w.ctb, w.mark, w.cnt, w.re, w.pre, p, sc);
      jpeg_enc_prog_next_kernel<<<grid, NT, 0, st>>>(w.re, w.pre, w.cnt, w.next, p, sc);
      uint32_t *next[2] = {w.next, w.next + (size_t)B * p.nblk};
      for (int r = 0; r < sc.rounds; ++r) jpeg_enc_prog_round_kernel<<<grid, NT, 0, st>>>(next[r & 1], next[~r & 1], w.mark, p, sc);
    }
    switch (sc.kind) {
      case K_SEQ:
        if (m.fitted)
          launch_chain<K_SEQ, T_IMAGE>(p, sc, grid, gy, w, huff, nval, bits, st);
        else
          launch_chain<K_SEQ, T_ANNEX_K>(p, sc, grid, gy, w, huff, nval, bits, st);
        break;
      case K_DC_FIRST: launch_chain<K_DC_FIRST, T_IMAGE>(p, sc, grid, gy, w, huff, nval, bits, st); break;
      case K_DC_REFINE: launch_chain<K_DC_REFINE, T_NONE>(p, sc, grid, gy, w, huff, nval, bits, st); break;
      case K_AC_FIRST: launch_chain<K_AC_FIRST, T_IMAGE>(p, sc, grid, gy, w, huff, nval, bits, st); break;
      default: launch_chain<K_AC_REFINE, T_IMAGE>(p, sc, grid, gy, w, huff, nval, bits, st); break;
    }
    jpeg_enc_count_kernel<<<gbytes, NT, 0, st>>>(bits, sc.words, w.tot, w.ffsum, p);
    jpeg_enc_scan_kernel<<<gy, NT, 0, st>>>(w.ffsum, p.nbchunk, 0, w.tot, 1, 1, B);
    if (m.progressive)
      jpeg_enc_prog_emit_kernel<<<gbytes, NT, 0, st>>>(bits, w.tot, w.ffsum, d_out, cap, d_len, d_err, w.huff4, w.nval4, d_huff, d_nval, w.pos, k, p, sc);
    else
      jpeg_enc_emit_kernel<<<gbytes, NT, 0, st>>>(bits, sc.words, w.tot, w.ffsum, d_out, cap, d_len, d_err, d_nval, p);
  }
  return sgic::check_launch(name);
}

int plan_cap(const char *name, const Mode &m, int H, int W, int sub, size_t *cap) {
  SGIC_REQUIRE_AS(name, cap != nullptr, "null output");
  Plan pl;
  SGIC_REQUIRE_AS(name, make_plan(m, 1, H, W, sub, nullptr, &pl), m.limits);
  *cap = pl.cap;
  return SGIC_OK;
}

int plan_work_bytes(const char *name, const Mode &m, int B, int H, int W, int sub, size_t *bytes) {
  SGIC_REQUIRE_AS(name, bytes != nullptr, "null output");
  Plan pl;
  SGIC_REQUIRE_AS(name, make_plan(m, B, H, W, sub, nullptr, &pl), m.limits);
  *bytes = pl.bytes;
  return SGIC_OK;
}

}  // namespace

extern "C" int sgic_jpeg_encode_cap(int H, int W, int subsampling, size_t *cap) { return plan_cap(__func__, ANNEX_K, H, W, subsampling, cap); }

extern "C" int sgic_jpeg_encode_work_bytes(int B, int H, int W, int subsampling, size_t *bytes) {
  return plan_work_bytes(__func__, ANNEX_K, B, H, W, subsampling, bytes);
}

extern "C" int sgic_jpeg_encode_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt, uint8_t *d_work,
                                      size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err,
                                      sgic_stream_t stream) {
  return encode(__func__, ANNEX_K, d_rgb, B, H, W, subsampling, h_qt, d_work, work_bytes, d_out, cap, d_len, d_err, nullptr, nullptr, stream);
}

extern "C" int sgic_jpeg_encode_opt_cap(int H, int W, int subsampling, size_t *cap) { return plan_cap(__func__, FITTED, H, W, subsampling, cap); }

extern "C" int sgic_jpeg_encode_opt_work_bytes(int B, int H, int W, int subsampling, size_t *bytes) {
  return plan_work_bytes(__func__, FITTED, B, H, W, subsampling, bytes);
}

extern "C" int sgic_jpeg_encode_opt_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt,
                                          uint8_t *d_work, size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err,
                                          uint8_t *d_huff, int32_t *d_nval, sgic_stream_t stream) {
  return encode(__func__, FITTED, d_rgb, B, H, W, subsampling, h_qt, d_work, work_bytes, d_out, cap, d_len, d_err, d_huff, d_nval, stream);
}

extern "C" int sgic_jpeg_encode_prog_cap(int H, int W, int subsampling, size_t *cap) {
  return plan_cap(__func__, PROGRESSIVE, H, W, subsampling, cap);
}

extern "C" int sgic_jpeg_encode_prog_work_bytes(int B, int H, int W, int subsampling, size_t *bytes) {
  return plan_work_bytes(__func__, PROGRESSIVE, B, H, W, subsampling, bytes);
}

extern "C" int sgic_jpeg_encode_prog_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt,
                                           uint8_t *d_work, size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err,
                                           uint8_t *d_huff, int32_t *d_nval, sgic_stream_t stream) {
  return encode(__func__, PROGRESSIVE, d_rgb, B, H, W, subsampling, h_qt, d_work, work_bytes, d_out, cap, d_len, d_err, d_huff, d_nval, stream);
}
