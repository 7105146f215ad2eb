/*
 * sgic.h -- C ABI of libsgic.so, the MI355X (gfx950) hot path of the searchable generative image codec.
 *
 * Every entry point is `extern "C"`, takes plain pointers + sizes (no torch / pybind types), returns
 * 0 on success or a negative SGIC_E* code, never throws, and launches on the HIP stream it is given
 * (pass NULL for the default stream).  Pointers named d_* are DEVICE pointers (HBM); everything else is
 * host memory.  Handles are thread-compatible: one handle per thread/stream; the library has no mutable
 * process-global launch state (launch options travel per call in sgic_launch_opts).
 *
 * Each block below cites the reference interface (file:line under /root/reference/src) it replaces;
 * INTEGRATION.md shows the reference-side binding.
 */
#ifndef SGIC_H
#define SGIC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t *sgic_stream_t; /* == hipStream_t */

#define SGIC_OK 0
#define SGIC_EINVAL -1  /* bad argument / shape the kernel does not support */
#define SGIC_EHIP -2    /* a HIP runtime call failed (see sgic_last_error) */
#define SGIC_ENOSPC -3  /* output buffer too small */
#define SGIC_ENODEV -4  /* no gfx950 device visible */

const char *sgic_last_error(void);
int sgic_version(void);
/* number of visible HIP devices, or SGIC_ENODEV; does not create a context */
int sgic_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Entropy coder  (replaces entropy.MLCodec_rans / MLCodec_CXX: cpp/py_rans/py_rans.h:13-57,
 * cpp/py_rans/py_rans.cpp:22-221, cpp/rans/rans.cpp:71-187,280-362, cpp/ops/ops.cpp:24-82)
 * ------------------------------------------------------------------------------------------- */

/* MLCodec_CXX.pmf_to_quantized_cdf(pmf, precision) -> cdf[n+1]   (ops.cpp:24-82).  Host-side table
 * builder, runs once per process at update() time. */
int sgic_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf_out);

/* CDF group = what RansEncoder/RansDecoder.add_cdf registers (py_rans.cpp:47-76, rans.cpp:71-93,
 * 287-295).  cdf is (rows, cols) int32 row-major on the HOST; it is uploaded to HBM once. */
typedef struct sgic_cdf_table sgic_cdf_table;
int sgic_cdf_table_create(const int32_t *cdf, int rows, int cols, const int32_t *sizes, const int32_t *offsets,
                          sgic_cdf_table **out);
void sgic_cdf_table_destroy(sgic_cdf_table *t);

/* Batched RansEncoder.{reset, encode_with_indexes x K, flush, get_encoded_stream} for B independent
 * images (py_rans.cpp:22-45,85-136; rans.cpp:101-187).  d_sym/d_idx: (B, n_per_img) int16, for each
 * image the concatenation of all encode_with_indexes calls in call order; idx < 0 => symbol skipped.
 * Stream b is written END-ALIGNED inside its slot: bytes d_out[b*cap + d_off[b] .. b*cap + cap),
 * d_len[b] = cap - d_off[b]; byte 0 of the stream is the 0x01 single-stream flag.  d_err[b] != 0 if
 * the slot was too small (SGIC_ENOSPC) or an index was out of range (SGIC_EINVAL). */
int sgic_rans_encode_batch(const sgic_cdf_table *t, const int16_t *d_sym, const int16_t *d_idx, int B,
                           int n_per_img, uint8_t *d_out, int cap, int32_t *d_off, int32_t *d_len,
                           int32_t *d_err, sgic_stream_t stream);

/* RansDecoder.set_stream for B images (py_rans.cpp:150-185, rans.cpp:280-285).  Streams are
 * (B, cap) with d_off/d_len as produced above (or d_off = 0 for front-aligned uploads).
 * d_state: (B, 4) uint32 cursor {x, pos, err, _}.  err: 0, 1 = the stream ended too soon, 2 = not a header this
 * coder writes (a multi-stream flag byte, or a state below the coder's lower bound 2^23, from which decoding need
 * not end), 3 = an index past the table's rows (set by decode).  Once set it stays, and decode writes zeros. */
int sgic_rans_decode_init_batch(const uint8_t *d_streams, int cap, const int32_t *d_off, const int32_t *d_len,
                                int B, uint32_t *d_state, sgic_stream_t stream);
/* RansDecoder.decode_stream (rans.cpp:303-362): continues from the cursor.  Image b reads its indexes at
 * d_idx + b*idx_stride (n int16) and writes symbols at d_sym_out + b*out_stride (0 where idx<0), so a
 * step slice of a (B,4,n) buffer can be addressed in place.  Reads past the end of a stream are
 * bounds-checked: the state's err word is set instead of over-reading like the reference. */
int sgic_rans_decode_batch(const sgic_cdf_table *t, const uint8_t *d_streams, int cap, const int32_t *d_off,
                           const int32_t *d_len, int B, uint32_t *d_state, const int16_t *d_idx, int n,
                           int idx_stride, int16_t *d_sym_out, int out_stride, sgic_stream_t stream);

/* z-branch: torchac.encode_float_cdf / decode_float_cdf with the uniform 4096-symbol cdf
 * (models/codec_sq_fixbpp.py:841-846,863-864,886-887) == 12-bit MSB-first packing + "01" terminator.
 * d_idx: (B, n) int32 indices in [0,4096); d_out: (B, sgic_pack12_size(n)) bytes. */
size_t sgic_pack12_size(size_t n);
int sgic_pack12_batch(const int32_t *d_idx, int B, int n, uint8_t *d_out, sgic_stream_t stream);
int sgic_unpack12_batch(const uint8_t *d_in, int B, int n, int32_t *d_idx, sgic_stream_t stream);

/* One step k (0..3) of the 4-step masked quantiser fused with build_indexes
 * (entropy/compression_model.py:224-239,296-366; entropy/entropy_models.py:355-362,66-69).
 * Layout NHWC: d_y (B*HW, 64) already divided by clamp_min(q_step,0.5); d_scales/d_means rows of
 * ld_sm floats; d_yhat (B*HW rows, ld_yhat floats): the active (channel,pos) entries get y_q + mean.
 * d_sym/d_idx: (B, 4, 16, H, W) int16, step k slice written.  thr < 0 disables force-zero/skip. */
int sgic_quant_step(const float *d_y, const float *d_scales, const float *d_means, int ld_sm, float *d_yhat,
                    int ld_yhat, int B, int H, int W, int C, int k, float thr, int16_t *d_sym, int16_t *d_idx,
                    sgic_stream_t stream);
/* GaussianEncoder.build_indexes on a flat array (entropy/entropy_models.py:355-362); thr < 0: no skip marking. */
int sgic_scale_to_index(const float *d_scales, long n, float thr, int16_t *d_idx, sgic_stream_t stream);
/* Decoder twins (compression_model.py:377-418): indexes from scales for step k, and
 * y_hat[active] = sym + mean after the symbols were decoded. */
int sgic_index_step(const float *d_scales, int ld_sm, int B, int H, int W, int C, int k, float thr,
                    int16_t *d_idx, sgic_stream_t stream);
/* Decision margins of sgic_index_step for step k (robust decoding of streams written by another fp32 implementation):
 * d_margin (B,4,C/4,H,W) float = distance of each coded sigma, in index steps, to the nearest boundary of build_indexes
 * (a bin edge or the skip threshold; entropy_models.py:355-362), d_alt = the index on the other side of that boundary. */
int sgic_index_margins(const float *d_scales, int ld_sm, int B, int H, int W, int C, int k, float thr, float *d_margin,
                       int16_t *d_alt, sgic_stream_t stream);
int sgic_dequant_step(const int16_t *d_sym, const float *d_means, int ld_sm, float *d_yhat, int ld_yhat, int B,
                      int H, int W, int C, int k, sgic_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Transform kernels (fp32, row-major "token x channel" = NHWC activations).  They replace the stock
 * ATen ops under the reference's nn.Modules; reference call sites are cited per function.
 * ------------------------------------------------------------------------------------------- */
#define SGIC_ACT_NONE 0
#define SGIC_ACT_GELU 1  /* exact erf GELU (nn.GELU default) */
#define SGIC_ACT_SILU 2
#define SGIC_ACT_TANH 3
#define SGIC_ACT_LRELU 4 /* LeakyReLU(0.01) */

/* Launch options of the GEMM-family and attention entry points.  Passed per call (NULL = defaults): the library keeps
 * NO process-global launch state, so two threads / streams can launch with different options concurrently.
 *   tile_mode (sgic_gemm_f32 / sgic_gemm_batched_f32 / sgic_conv3x3_f32): 0 = built-in heuristic, 1 = 128x128,
 *     2 = 128x64 workgroup tiles (double-buffered LDS), 3 / 4 = the same tiles with a single LDS buffer (3-4 workgroups
 *     per CU), 5..8 = 1..4 with a start-up stagger of the co-resident workgroups, 9 / 10 = MIXED: whole rounds of
 *     128x128 tiles for the bulk of the rows + 64x64 tiles for the remaining rows in the same launch (2 / 1 LDS
 *     buffers), 11 = persistent 128x128 (2 resident workgroups per CU walk the tile list), 12 = persistent MIXED,
 *     13 / 14 = 64x64 tiles as their own launch (2 / 1 buffers; small-M GEMMs), 15 = latency kernel for under-filled
 *     launches (32x32 tiles of 16x16x4-MFMA blocks: 4x shorter dependent chains, 4x the workgroups; needs K % 64 == 0,
 *     otherwise runs as 13).  Results are bitwise identical for
 *     every choice (the k order is fixed by K alone); the host autotuner (sgic_amd.ops) picks per shape and persists
 *     its picks.
 *   attn_mode (sgic_attention_f32): low 3 bits: 0 = built-in choice, 1..6 = K/V ring depth x start-up stagger, 7 = three query
 *     row blocks per workgroup with a unit's row blocks padded to a multiple of three (three workgroups per CU: two whole rounds
 *     for L = 289 at batch 32) (results bitwise identical for every choice); +8: S^T = K Q^T as a bf16x3 split product on the bf16
 *     matrix pipe (fp32-accurate, the arithmetic of sgic_gemm_split3_f32; differs from the fp32-MFMA variant in the last bits,
 *     identical across 1..7).
 *   profiler: non-NULL and open => the launch is dispatched with its own (start, stop) event pair (hipExtLaunchKernel:
 *     timestamps taken by the dispatch itself, no extra packets on the stream). */
typedef struct sgic_profiler sgic_profiler;
typedef struct sgic_launch_opts {
  int tile_mode;
  int attn_mode;
  sgic_profiler *profiler;
  int w_packed;   /* split GEMM / convolution: d_Wplanes is in the slice-major layout of sgic_split3_pack_f32 */
  int a_packed;   /* split GEMM with d_A == NULL: d_Aplanes is slice-major [3][K / 32][M][32] -- what sgic_layernorm_split3_f32,
                     sgic_attention_split3_f32, a GEMM's d_Cplanes output and sgic_split3_pack_f32 write; 0 = row-major [3][M][K]
                     (sgic_split3_f32) */
} sgic_launch_opts;

/* Profile window for the roofline figure of bench.py.  One profiler per launching thread.  begin() opens a window,
 * every launch that carries the profiler in its opts is timed, end() closes the window and returns the duration in
 * milliseconds of each launch in launch order (at most cap of them; *n_out = launches seen). */
int sgic_profiler_create(sgic_profiler **out);
void sgic_profiler_destroy(sgic_profiler *p);
int sgic_profiler_begin(sgic_profiler *p, int max_launches);
int sgic_profiler_end(sgic_profiler *p, float *ms_out, int cap, int *n_out);

/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + R[M,N]   -- nn.Linear / 1x1 Conv2d / im2col'd convs
 * (titok/blocks.py:37-64, blocks/swin_transformer.py:30-39,86,92, models/cross_blocks.py:55-68,
 * blocks/conv_blocks.py:63-67, blocks/dcvc.py:17-23,42-43).  fp32-input MFMA (exact fp32), fixed k
 * order => batch-invariant.  K, lda, ldw multiples of 4; A, W 16-byte aligned; bias/R optional.
 * Row maps row(m) = (m / seg) * seg_stride + m % seg (seg = 0: identity) let A be read from / C be
 * written to a token slice [:, a:b] of an (n, L, C) buffer in place (models/cross_blocks.py:87-94). */
int sgic_gemm_f32(const float *d_A, int lda, const float *d_W, int ldw, const float *d_bias, const float *d_R,
                  int ldr, float *d_C, int ldc, int M, int N, int K, int act, int a_seg, int a_seg_stride,
                  int c_seg, int c_seg_stride, const sgic_launch_opts *opts, sgic_stream_t stream);

/* Row LayerNorm, biased variance, eps inside sqrt, optional fused SiLU (act = SGIC_ACT_SILU); rows of x
 * and y addressed through the same kind of segment map (titok/blocks.py:36,42,
 * blocks/swin_transformer.py:135,142, blocks/conv_blocks.py:62, models/cross_blocks.py:62,67). */
int sgic_layernorm_f32(const float *d_x, int ldx, int xseg, int xseg_stride, const float *d_gamma,
                       const float *d_beta, float *d_y, int ldy, int yseg, int yseg_stride, int M, int C, float eps,
                       int act, sgic_stream_t stream);

/* softmax(scale * Q K^T + bias) V for 64-wide heads; q/k/v/out are row-strided "token x (heads*64)"
 * matrices, head h at column h*64.  Sequence s, token t lives in row d_rowmap[s*L+t] (null: s*L+t) --
 * the Swin cyclic shift + window partition is such a map (blocks/swin_transformer.py:94-128).
 * d_bias: (nvar, L, L) additive (relative-position table + -inf shift masks), variant per sequence in
 * d_biasvar (null: 0).  nn.MultiheadAttention (titok/blocks.py:50-54) is the rowmap = bias = null case. */
int sgic_attention_f32(const float *d_q, int ldq, const float *d_k, int ldk, const float *d_v, int ldv,
                       float *d_out, int ldo, int L, int nseq, int nheads, const int32_t *d_rowmap,
                       const float *d_bias, const int32_t *d_biasvar, float scale, const sgic_launch_opts *opts,
                       sgic_stream_t stream);
/* The same attention for the query tokens q_tok0 .. q_tok0 + Lq - 1 of every sequence only (a last layer whose other rows nobody
 * reads).  K / V keep the full row space (row s*L + t); query token t lives at row s*Lq + (t - q_tok0) of d_q and of d_out.
 * q_tok0 % 32 == 0, and the window ends at L or on a multiple of 32: the kernel works on 32-row query blocks (plus the ragged
 * rows of L % 32 in {1, 2}), and exactly the blocks inside the window run, each as in the full launch -- every output row is
 * bitwise what sgic_attention_f32 writes for that token.  d_rowmap must be NULL. */
int sgic_attention_window_f32(const float *d_q, int ldq, const float *d_k, int ldk, const float *d_v, int ldv,
                              float *d_out, int ldo, int L, int nseq, int nheads, const int32_t *d_rowmap,
                              const float *d_bias, const int32_t *d_biasvar, float scale, int q_tok0, int Lq,
                              const sgic_launch_opts *opts, sgic_stream_t stream);
/* nblocks runs of block_elems contiguous floats, run i copied from d_src + i*src_stride to d_dst + i*dst_stride (element
 * strides): an exact device-to-device copy of the rows that sgic_attention_window_f32's caller keeps. */
int sgic_copy_blocks_f32(const float *d_src, long src_stride, float *d_dst, long dst_stride, long block_elems, int nblocks,
                         sgic_stream_t stream);

/* im2col of non-overlapping PxP patches of an NCHW image with x*mul+add fused; patch rows in plain
 * (b,gy,gx) order or 16x16-tile-major (tile16) order (codec_sq_fixbpp.py:855,119; titok/blocks.py:98-100). */
int sgic_im2col_patch(const float *d_x, int B, int C, int H, int W, int P, float mul, float add, int tile16,
                      float *d_out, sgic_stream_t stream);
/* [cls+pos0 ; emb+pos ; lat+latpos] token assembly (codec_sq_fixbpp.py:127-138). */
int sgic_assemble_tokens(const float *d_emb, const float *d_cls, const float *d_pos, const float *d_lat,
                         const float *d_latpos, int N, int P, int T, int D, float *d_out, sgic_stream_t stream);
/* out[n*oseg+l,:] = in[n*iseg+l,:] + vec[l,:]  (models/cross_blocks.py:82-84); vec may be null. */
int sgic_add_rows_bcast(const float *d_in, int ldi, int iseg, const float *d_vec, float *d_out, int ldo, int oseg,
                        int Nn, int Lr, int D, sgic_stream_t stream);
/* depthwise kxk conv, NHWC, weights [k*k][C], optional per-channel prescale (blocks/conv_blocks.py:74-75,
 * blocks/dcvc.py:21,35). */
int sgic_dwconv_nhwc(const float *d_x, const float *d_w, const float *d_bias, const float *d_prescale, float *d_y,
                     int B, int H, int W, int C, int k, int tile16, sgic_stream_t stream);
/* im2col of the 2x2/s2 conv in feat_out (codec_sq_fixbpp.py:90): out[(b,y/2,x/2)][(ky*2+kx)*C+c]. */
int sgic_im2col_2x2(const float *d_x, int B, int H, int W, int C, int tile16, float *d_out, sgic_stream_t stream);
/* ConvFFN3 gate (blocks/dcvc.py:50-53). */
int sgic_gated_lrelu(const float *d_x, float *d_out, int M, int C2, sgic_stream_t stream);
/* y = x * v (mode 0), x / max(v, 0.5) (mode 1) or x * max(v, 0.5) (mode 2), v row m % vrows (sq_bottleneck.py:111,117;
 * compression_model.py:325-326,355). */
int sgic_colop(const float *d_x, int ldx, const float *d_v, int ldv, int vrows, float *d_y, int ldy, int M, int C,
               int mode, sgic_stream_t stream);
/* out[n][t][c] = in[n*in_seq_stride + c*T + t]  ("fake 2-D" reshape, codec_sq_fixbpp.py:175-177). */
int sgic_fake2d_transpose(const float *d_in, long in_seq_stride, float *d_out, int N, int T, int D,
                          sgic_stream_t stream);
/* l2-normalised nearest-code search (titok/quantizer.py:46-61). */
int sgic_vq_argmin(const float *d_z, int ldz, const float *d_codebook, int ncodes, int dim, int M, int l2norm,
                   int32_t *d_idx, sgic_stream_t stream);
/* (CLIP preprocessing: sgic_clip_preprocess_ragged / sgic_clip_preprocess_u8canvas below.) */
/* unit-normalise rows + u8 quantise (compress.py:73,77). */
int sgic_l2norm_u8(const float *d_x, int ldx, int M, int D, float *d_unit, uint8_t *d_q, sgic_stream_t stream);

/* ---- fp32-accurate GEMM on the bf16 matrix pipe ("bf16x3" operand split; csrc/gemm_split.hip) -------------------
 * Same contract as sgic_gemm_f32 (the nn.Linear / 1x1 Conv2d call sites cited there), computed as six bf16 MFMAs per
 * 16 k over operands pre-split into three bf16 planes, x = x1 + x2 + x3 exactly.  Error vs an fp64 reference is at the
 * level of (measured: slightly below) a plain fp32 fmaf chain; results are bitwise independent of M, of the tile mode
 * and of the batch (fixed arithmetic order per output element), but NOT bitwise equal to sgic_gemm_f32's.
 * sgic_split3_f32: x[rows, cols] fp32 (row map as A of sgic_gemm_f32) -> d_planes [3][rows][cols] bf16 bit patterns;
 *   cols % 8 == 0.  Weights are split once at load time.
 * sgic_gemm_split3_f32: d_A != NULL: A is split into the caller's workspace d_Aplanes (3*M*K uint16) first;
 *   d_A == NULL: d_Aplanes already holds the planes.  K % 32 == 0.
 *   d_Cplanes != NULL: the result is written as slice-major planes [3][N / 32][M][32] (the next GEMM's A operand with
 *   opts->a_packed = 1) instead of d_C; N % 32 == 0.
 *   opts->tile_mode: 0 = heuristic, 1 = 128x256, 2 = 128x128, 3 = 64x64, 4 = 32x32 (the latency kernel for
 *   under-filled launches), 5 = 64x128 (two workgroups per CU) workgroup tiles, 6 / 7 = 1 / 2 for the rows that
 *   fill whole rounds of the 256 CUs + 5 for the remaining rows (two launches), 8 / 9 = the same with 4 for the remaining rows,
 *   10 / 11 = 1 / 2 as a persistent launch (one resident workgroup per CU walks the tile list), 12 / 13 = 8 / 9 with the
 *   whole rounds walked persistently, 14 / 15 = 256x128 tiles (plain / persistent), 16 / 17 = 2 / 11 with LDS-DMA staging,
 *   18-25 = the ring kernel's small tiles (32x32 ... 80x64: single-image sized launches), 26 / 27 = 8 / 12 with the ring kernel's
 *   80x64 tiles for the remaining rows, 28 / 29 = 128x192 tiles (plain / persistent; N = 768: 8192 rows = one whole round), 30 = 256x256 tiles
 *   (W single-buffered in LDS), 31 = 30 for the rows that fill whole rounds + 1 for the rest, 32 = 160x256 tiles (M = 9 248 x
 *   N = 1024: 232 tiles, one round).  26 takes ONE launch of 32 instead when the product is not a convolution, 128x256 tiles need
 *   more than one round of the 256 CUs and 160x256 tiles fit in one; 27 never does.
 *   The 128x256 and 256x128 tiles (1, 10, 14, 15 and the whole-round part of 6, 8, 12) stage their operands by LDS-DMA
 *   (global_load_lds: no register pass, no ds_write), the other tiles through registers; all modes are bitwise identical. */
int sgic_split3_f32(const float *d_x, int ld, int rows, int cols, int seg, int seg_stride, uint16_t *d_planes,
                    sgic_stream_t stream);
/* planes of an operand [rows][cols = K] in the slice-major layout [3][K / 32][rows][32] (opts->w_packed / a_packed = 1 at the
 * consuming call): a 16-row piece of a 32-k slice is 1 KiB of consecutive bytes (whole cache lines) for the LDS-DMA staging.  K % 32 == 0. */
int sgic_split3_pack_f32(const float *d_x, int ld, int rows, int cols, uint16_t *d_planes, sgic_stream_t stream);
int sgic_gemm_split3_f32(const float *d_A, int lda, int a_seg, int a_seg_stride, uint16_t *d_Aplanes,
                         const uint16_t *d_Wplanes, const float *d_bias, const float *d_R, int ldr, float *d_C, int ldc,
                         uint16_t *d_Cplanes, int M, int N, int K, int act, int c_seg, int c_seg_stride,
                         const sgic_launch_opts *opts, sgic_stream_t stream);
/* What tile_mode does with an M x N product (conv != 0: as sgic_conv3x3_split3_f32 with M = B H W, N = Cout) -- the very function the
 * dispatcher runs; host only, no GPU call.  *tile_m x *tile_n: the nominal workgroup tile of the first launch; *split_row: the row
 * at which a second launch starts (0: there is one launch); *tail_mode: the single-launch mode of that second launch (0: none). */
int sgic_gemm_split3_plan(int M, int N, int conv, int tile_mode, int *tile_m, int *tile_n, int *split_row, int *tail_mode);
/* sgic_conv3x3_f32 as an implicit split GEMM: d_in_planes = bf16x3 planes of the zero-halo NHWC input, [3][B (H+2) (W+2)][Cin]
 * (sgic_split3_f32 over the halo buffer's rows; opts->a_packed = 0) or slice-major [3][Cin / 32][B (H+2) (W+2)][32]
 * (sgic_split3_pack_f32, sgic_groupnorm_nhwc_split3, sgic_halo_copy_split3; a_packed = 1); d_Wplanes = planes [3][Cout][9 Cin]
 * (or slice-major, w_packed = 1).  Cin % 32 == 0. */
int sgic_conv3x3_split3_f32(const uint16_t *d_in_planes, const uint16_t *d_Wplanes, const float *d_bias, const float *d_R,
                            int ldr, float *d_out, int ldc, int B, int H, int W, int Cin, int Cout, int act,
                            const sgic_launch_opts *opts, sgic_stream_t stream);
/* sgic_groupnorm_nhwc / sgic_halo_copy writing the interior of a zero-halo slice-major bf16x3 planes buffer
 * [3][C / 32][B (H+2) (W+2)][32] -- the input of sgic_conv3x3_split3_f32 with a_packed = 1 -- directly (no fp32 halo buffer, no
 * split pass).  C % 32 == 0. */
int sgic_groupnorm_nhwc_split3(const float *d_x, const float *d_gamma, const float *d_beta, int B, int H, int W, int C,
                               int groups, float eps, int swish, double *d_ws, float *d_stats, uint16_t *d_halo_planes,
                               sgic_stream_t stream);
int sgic_halo_copy_split3(const float *d_in, int B, int H, int W, int C, int upsample2x, int tile16, uint16_t *d_halo_planes,
                          sgic_stream_t stream);
/* sgic_attention_f32 with the output written as slice-major bf16x3 planes [3][nheads*2][rows][32] (rows = the row space of d_rowmap,
 * >= nseq*L): the A operand of the out-projection when that runs as a split GEMM. */
int sgic_attention_split3_f32(const float *d_q, int ldq, const float *d_k, int ldk, const float *d_v, int ldv,
                              uint16_t *d_out_planes, long rows, int L, int nseq, int nheads, const int32_t *d_rowmap,
                              const float *d_bias, const int32_t *d_biasvar, float scale, const sgic_launch_opts *opts,
                              sgic_stream_t stream);
/* sgic_attention_window_f32 with the planes output of sgic_attention_split3_f32 (rows >= nseq*Lq). */
int sgic_attention_window_split3_f32(const float *d_q, int ldq, const float *d_k, int ldk, const float *d_v, int ldv,
                                     uint16_t *d_out_planes, long rows, int L, int nseq, int nheads, const int32_t *d_rowmap,
                                     const float *d_bias, const int32_t *d_biasvar, float scale, int q_tok0, int Lq,
                                     const sgic_launch_opts *opts, sgic_stream_t stream);
/* nn.LayerNorm (call sites as sgic_layernorm_f32) whose only consumer is a split GEMM: the normalised rows are written
 * directly as slice-major bf16x3 planes [3][C / 32][M][32] (dense rows), so no fp32 copy and no separate split pass.  C % 256 == 0, C <= 2048. */
int sgic_layernorm_split3_f32(const float *d_x, int ldx, int xseg, int xseg_stride, const float *d_gamma,
                              const float *d_beta, uint16_t *d_planes, int M, int C, float eps, int act,
                              sgic_stream_t stream);

/* Batched GEMM (element strides, 0 = shared operand) -- VQGAN AttnBlock single-head attention as
 * S_b = Q_b K_b^T, O_b = P_b V_b (taming/modules/diffusionmodules/model.py:168-192). */
int sgic_gemm_batched_f32(const float *d_A, int lda, long strideA, const float *d_W, int ldw, long strideW,
                          const float *d_bias, const float *d_R, int ldr, long strideR, float *d_C, int ldc,
                          long strideC, int M, int N, int K, int act, int batch, const sgic_launch_opts *opts,
                          sgic_stream_t stream);
/* 3x3/s1/p1 Conv2d as an implicit GEMM on the matrix cores over a zero-halo NHWC input [B,H+2,W+2,Cin]
 * (Cin % 32 == 0); weights [Cout][(ky,kx,cin)]; fused bias/activation/residual (model.py:38-137,436-537). */
int sgic_conv3x3_f32(const float *d_in_halo, const float *d_W, const float *d_bias, const float *d_R, int ldr,
                     float *d_out, int ldc, int B, int H, int W, int Cin, int Cout, int act, const sgic_launch_opts *opts,
                     sgic_stream_t stream);
/* GroupNorm(groups, eps) on NHWC + optional swish; output plain or into the interior of a zero-halo buffer.
 * d_ws: B*64*C*2 doubles, d_stats: B*groups*2 floats (model.py:34-35,117-131). */
int sgic_groupnorm_nhwc(const float *d_x, const float *d_gamma, const float *d_beta, int B, int H, int W, int C,
                        int groups, float eps, int swish, int halo_out, double *d_ws, float *d_stats, float *d_y,
                        sgic_stream_t stream);
/* copy (optionally nearest-2x upsampled, optionally from tile-major rows) into the interior of a zero-halo
 * buffer [B, OH+2, OW+2, C] (Upsample, model.py:49-53). */
int sgic_halo_copy(const float *d_in, int B, int H, int W, int C, int upsample2x, int tile16, float *d_out,
                   sgic_stream_t stream);
/* y = softmax(scale * x) over rows of length L (model.py:181-183; codec_sq_fixbpp.py:660-661). */
int sgic_softmax_rows(const float *d_x, float *d_y, long M, int L, float scale, sgic_stream_t stream);
/* PixelShuffle(2) of a plain [(b,y,x), 4C] map into tile-major [(b,2y+i,2x+j), C] (codec_sq_fixbpp.py:203-207). */
int sgic_pixel_shuffle2_tm16(const float *d_in, int B, int H, int W, int C, float *d_out, sgic_stream_t stream);
/* decoder tokens [cls+pos0 ; mask+pos ; emb+latpos] (codec_sq_fixbpp.py:258-267). */
int sgic_assemble_dec_tokens(const float *d_emb, const float *d_cls, const float *d_mask, const float *d_pos,
                             const float *d_latpos, int N, int P, int T, int D, float *d_out, sgic_stream_t stream);
/* z_hat rows: codebook[idx] l2-normalised, zero-padded to ld floats (codec_sq_fixbpp.py:889-892). */
int sgic_codebook_gather_norm(const int32_t *d_idx, const float *d_codebook, int M, int dim, int ld, float *d_out,
                              sgic_stream_t stream);
/* x_hat [(b,y,x), ld>=3] -> clamp(-1,1) -> NCHW (codec_sq_fixbpp.py:901). */
int sgic_nhwc3_to_nchw_clamp(const float *d_in, int ld, int B, int H, int W, float *d_out, sgic_stream_t stream);

/* exact top-k per row, descending, ties -> lower index (IndexFlatIP.search, search.py:113-120); d_scores
 * (nq, n) = sgic_gemm_f32(queries, database) and is consumed (taken entries become NaN). */
int sgic_topk_rows(float *d_scores, int nq, int n, int k, float *d_out_scores, int32_t *d_out_idx, sgic_stream_t stream);

/* Fused exact search over u8 CLIP codes (sgic_amd/search.py CodeIndex): i8 MFMA inner products and top-k in one kernel; the
 * (nq, n) score matrix never exists.  d_q (nq, D) and d_db (n, D) are u8 codes, 16-byte aligned; D % 64 == 0, D <= 4096, k <= 128,
 * k <= n, anything else is SGIC_EINVAL (the caller keeps the fp32 path).  With a = c - 128, S = sum a_q a_d, s_x = sum a_x the
 * int32 N = 4 S + 2 s_q + 2 s_d + D equals sum (2 c_q - 255)(2 c_d - 255) exactly; d_rq / d_rdb hold r_x = float32(1 / sqrt(
 * float64(sum (2 c_x - 255)^2))), computed on the host (search.code_rnorm).  Ranking key = float32(N) * r_d, order: key
 * descending, equal keys -> lower database index; reported score = key * r_q.  No float add, sqrt or division runs on the
 * device, so numpy reproduces every bit.  The database is cut into contiguous ascending splits (splits <= 0: chosen so that the
 * grid covers the chip; > 0: an upper bound the caller asks for); with more than one split each (query, split) writes its k best
 * to d_work and a merge kernel orders them.  sgic_search_codes_u8_work_bytes (host-only, takes no stream) returns the split count
 * actually used and the workspace size, nq * splits * k * 8 bytes (0 for one split). */
int sgic_search_codes_u8_work_bytes(int nq, int n, int D, int k, int splits, int *splits_used, size_t *bytes);
int sgic_search_codes_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D, int k,
                         int splits, uint8_t *d_work, size_t work_bytes, float *d_out_scores, int32_t *d_out_idx,
                         sgic_stream_t stream);

/* The same search with fp32 queries (text / image vectors, CodeIndex.search_vectors): d_q (nq, D) fp32, 16-byte aligned, against
 * the u8 codes d_db (n, D) and their d_rdb.  D % 64 == 0, D <= 2048 (three query planes in LDS), k <= 128, k <= n, anything
 * else is SGIC_EINVAL (the caller keeps the fp32 path).  The query goes to fixed point: Q_j = clamp(rint(q_j * 2^22), -2^22,
 * +2^22) as an integer (round to nearest even; a NaN coordinate gives 0), then to balanced base-256 digits
 *   d0 = ((Q + 128) & 255) - 128, Q' = (Q - d0) >> 8, d1 = ((Q' + 128) & 255) - 128, d2 = (Q' - d1) >> 8,
 * so Q = 65536 d2 + 256 d1 + d0 with d0, d1 in [-128, 127] and d2 in [-64, 64], three i8 planes.  With a_d = c_d - 128 and
 * v_d = 2 c_d - 255 = 2 a_d + 1: S_p = sum_j d_p,j a_d,j (i8 MFMA, |S_p| <= 2^14 D, exact in int32) and, combined in int64,
 *   M = sum_j Q_j v_d,j = 2 (65536 S_2 + 256 S_1 + S_0) + sum_j Q_j,   |M| <= 2^22 * 255 * D.
 * Ranking key = float32(M) * r_d (one RNE int64 -> fp32 conversion, one fp32 multiply), order: key descending, equal keys ->
 * lower database index; reported score = key * 2^-22 (exact).  For finite |q_j| <= 1 the score is within 2^-23 sqrt(D) + 2^-22
 * of the fp64 q . v_d / |v_d| (query rounding of at most 2^-23 per coordinate times |v|_1 / |v| <= sqrt(D); three fp32
 * roundings).  Splits, workspace (nq * splits * k * 8 bytes, 0 for one split) and the merge are those of the u8 entry;
 * sgic_search_codes_f32q_work_bytes is host-only and takes no stream. */
int sgic_search_codes_f32q_work_bytes(int nq, int n, int D, int k, int splits, int *splits_used, size_t *bytes);
int sgic_search_codes_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D, int k, int splits,
                           uint8_t *d_work, size_t work_bytes, float *d_out_scores, int32_t *d_out_idx, sgic_stream_t stream);

/* Threshold (range) search over the same u8 codes (CodeIndex.range_search / duplicate_pairs): every pair (q, d) whose
 *   score = (float32(N) * r_d) * r_q   (N, r as above: the bits sgic_search_codes_u8 reports)
 * satisfies score >= threshold in fp32 is a hit.  Hits are appended, in no particular order, to d_out_q / d_out_d / d_out_score
 * (`capacity` entries each) through the 64-bit counter *d_count, which the CALLER zeroes: the call adds the full number of hits to
 * it and stores an entry only at a position < capacity, so the count is exact after an overflow and nothing past `capacity` is
 * written (retry with `count` entries; the predicate is deterministic).  capacity = 0 with null arrays is a count-only call.
 * self_join = 1: d_q is d_db, d_rq is d_rdb, nq == n; only pairs d > q are emitted and the database tiles wholly at or below a
 * query tile's diagonal are not computed.  d_q / d_db 16-byte aligned, d_count 8-byte aligned; D % 64 == 0, D <= 4096; the
 * threshold finite; `splits` as in sgic_search_codes_u8; anything else is SGIC_EINVAL.  No workspace. */
int sgic_search_range_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D,
                         float threshold, int self_join, int splits, long long capacity, uint64_t *d_count, int32_t *d_out_q,
                         int32_t *d_out_d, float *d_out_score, sgic_stream_t stream);

/* The threshold search with fp32 queries (text / image vectors, CodeIndex.range_search_vectors): d_q (nq, D) fp32 against the u8
 * codes d_db (n, D) and their d_rdb.  The query goes to 2^-22 fixed point and three balanced base-256 digit planes exactly as in
 * sgic_search_codes_f32q (Q, d0, d1, d2, S_p and the int64 M = 2 (65536 S_2 + 256 S_1 + S_0) + sum_j Q_j are those of its comment;
 * a NaN coordinate gives 0), and a pair (q, d) is a hit iff
 *   score = (float32(M) * r_d) * 2^-22 >= threshold   (fp32, in that order: the bits sgic_search_codes_f32q reports)
 * No float add, root or division runs on the device.  Hits are appended, in no particular order, to d_out_q / d_out_d /
 * d_out_score (`capacity` entries each) through the 64-bit counter *d_count, which the CALLER zeroes.  Overflow contract, as in
 * sgic_search_range_u8: the call adds the full number of hits to the counter and stores an entry only at a position < capacity, so
 * the count is exact after an overflow and nothing past `capacity` is written (retry with `count` entries; the predicate is
 * deterministic).  capacity = 0 with null arrays is a count-only call.  There is no self-join.  d_q / d_db 16-byte aligned,
 * d_count 8-byte aligned; D % 64 == 0, D <= 2048 (three query planes in LDS); the threshold finite; `splits` as in
 * sgic_search_codes_u8; anything else is SGIC_EINVAL.  No workspace. */
int sgic_search_range_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D, float threshold,
                           int splits, long long capacity, uint64_t *d_count, int32_t *d_out_q, int32_t *d_out_d,
                           float *d_out_score, sgic_stream_t stream);

/* Rank of a target row (CodeIndex.rank / rank_vectors, search.py recall): for query q and database row t = d_target[q], with the
 * ranking key of sgic_search_codes_u8 (float32(N) * r_d), resp. of sgic_search_codes_f32q (float32(M) * r_d),
 *   d_rank[q]  = #{ d in [0, n) : key(q, d) > key(q, t)  or  (key(q, d) == key(q, t) and d < t) }
 *   d_score[q] = key(q, t) * r_q, resp. key(q, t) * 2^-22: the fp32 bits the top-k entry point reports for the pair,
 * so d_rank is the position of t in the full ordering the top-k search truncates at k: for every k, d_rank[q] < k exactly when t is
 * among the k results, and then out_idx[q][d_rank[q]] == t and out_scores[q][d_rank[q]] has the bits of d_score[q].  A pre-pass
 * computes the target's integer N / M in plain integer code (it is exact, so it is the scan's integer) and takes it through the
 * scan's one conversion and one multiply; the scan keeps integer counters and combines them with integer adds only (registers,
 * shuffles, LDS, one 32-bit atomic add per query and workgroup), so two runs give equal bits.  No candidate buffers, no merge.
 * d_target (nq) int32 is read on the DEVICE: the call cannot refuse a target outside [0, n), it clamps it into the range for the
 * loads and the outputs of that query then describe the clamped row.  Callers check the range first (ops.search_codes_rank does).
 * d_q, d_rq, d_db, d_rdb, D and `splits` as in sgic_search_codes_u8 / _f32q (D % 64 == 0; D <= 4096, fp32 queries D <= 2048);
 * d_work: 4-byte aligned, sgic_search_rank_work_bytes bytes (host-only, takes no stream: nq * 4, the target keys).  A null
 * pointer, nq < 1, n < 1, a bad D, splits > 2048, a misaligned pointer or a workspace that is too small is SGIC_EINVAL before any
 * launch: the outputs stay untouched. */
int sgic_search_rank_work_bytes(int nq, size_t *bytes);
int sgic_search_rank_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, const int32_t *d_target,
                        int nq, int n, int D, int splits, uint8_t *d_work, size_t work_bytes, int32_t *d_rank, float *d_score,
                        sgic_stream_t stream);
int sgic_search_rank_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, const int32_t *d_target, int nq, int n, int D,
                          int splits, uint8_t *d_work, size_t work_bytes, int32_t *d_rank, float *d_score, sgic_stream_t stream);

/* Clustering over the same u8 codes (CodeIndex.assign / kmeans): for every database row the best of K fp32 centroids.  d_cent
 * (K, D) fp32 rows of norm <= 1 and d_db (n, D) u8, both 16-byte aligned.  The centroid goes to 2^-22 fixed point and three balanced
 * base-256 digit planes exactly as the query of sgic_search_codes_f32q (Q, d0, d1, d2, S_p and the int64
 * M = 2 (65536 S_2 + 256 S_1 + S_0) + sum_j Q_j are those of its comment; a NaN coordinate gives 0).  For every row d:
 *   d_out_c[d] = the centroid with the largest M(c, d), equal M -> the lower centroid index;   d_out_M[d] = that M.
 * r_d > 0 is common to all centroids of a row, so the order of M is the order of the scores; the device runs no float compare, add,
 * root or division, and the caller derives score = (float32(M) * r_d) * 2^-22, the bits sgic_search_codes_f32q reports for that
 * (vector, row) pair.  A pre-pass writes the planes in MFMA fragment order and sum Q per centroid into d_work (16-byte aligned;
 * sgic_assign_codes_f32c_work_bytes, host-only, takes no stream: 16 ceil(K / 16) (3 D + 8) bytes).  D % 64 == 0, D <= 2048,
 * 1 <= K <= 65536, n >= 1; anything else, a null or misaligned pointer or a workspace that is too small is SGIC_EINVAL. */
int sgic_assign_codes_f32c_work_bytes(int K, int D, size_t *bytes);
int sgic_assign_codes_f32c(const float *d_cent, const uint8_t *d_db, int K, int n, int D, uint8_t *d_work, size_t work_bytes,
                           int32_t *d_out_c, int64_t *d_out_M, sgic_stream_t stream);

/* The exact integer sums of a partition of the codes: d_sums[c][j] += sum over the rows d of cluster c of (2 d_db[d][j] - 255),
 * d_counts[c] += the number of those rows (both int64; the CALLER zeroes them).  The caller passes the partition sorted by cluster:
 * d_order (n) int64, a permutation of the rows, and d_sorted_assign (n) int32, the cluster of row d_order[i], ascending.  A cluster
 * id outside [0, K) or a row outside [0, n) is skipped, never written.  Integer adds only (int32 registers, LDS, one 64-bit
 * atomic add per coordinate and run): the result is exact and does not depend on the schedule.  D % 16 == 0, D <= 4096; d_db
 * 16-byte aligned; anything else is SGIC_EINVAL. */
int sgic_cluster_sums_u8(const uint8_t *d_db, const int64_t *d_order, const int32_t *d_sorted_assign, int n, int D, int K,
                         int64_t *d_sums, int64_t *d_counts, sgic_stream_t stream);

/* Rate-distortion measurement of B pairs of u8 images (quality.measure, evaluate.py; the arithmetic of the reference's
 * taming/modules/losses/quality.py: PSNR and pytorch_msssim.MS_SSIM(data_range=1.0)).  d_a (original) and d_b (reconstruction) are
 * (B, H, W, 3) interleaved RGB.  d_sse[b][c] = sum (a - b)^2 over the plane, int64, exact (integer adds only; zeroed here).
 * d_levels[b][c][s] = {mean ssim, mean cs} of level s = 0..4 in fp64: level 0 is the u8 values, level s + 1 the 2 x 2 SUM of level s
 * with stride 2 starting at -(H_s % 2), -(W_s % 2), cells outside the plane 0 (avg_pool2d(2, padding = size % 2) without the
 * division: u16 numerators over 255 * 4^s, kept in d_work for both images); the window is g_i = exp(-(i - 5)^2 / 4.5) / sum, 11
 * taps, valid filtering, rows then columns; mu = F(X), s1 = F(XX) - mu1^2, s2 = F(YY) - mu2^2, s12 = F(XY) - mu1 mu2 with the
 * products formed exactly from the integers; cs = (2 s12 + 9e-4) / (s1 + s2 + 9e-4), ssim = (2 mu1 mu2 + 1e-4) / (mu1^2 + mu2^2 +
 * 1e-4) cs; each averaged over the (H_s - 10) x (W_s - 10) map.  A workgroup reduces its tile, the tiles' sums are added in a fixed
 * order (no float atomics): the same input gives the same bits.  The caller combines the levels (relu, weights, channel mean).
 * d_work: 16-byte aligned, at least the *bytes sgic_quality_u8_work_bytes returns (host-only, takes no stream).  1 <= B <= 65536,
 * 160 < H, W <= 16384; anything else, a null pointer, a misaligned or too small workspace is SGIC_EINVAL before any launch. */
int sgic_quality_u8_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_quality_u8(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, uint8_t *d_work, size_t work_bytes,
                    int64_t *d_sse, double *d_levels, sgic_stream_t stream);

/* The block sums of NIQE for B u8 images (niqe.Niqe, evaluate.py --niqe_params).  d_img is (B, H, W, 3)
 * interleaved RGB; nbh = H / 96, nbw = W / 96 (integer division) and the top-left 96 nbh x 96 nbw pixels are used.  Luma
 * Y = 16 + round_half_even((65481 R + 128553 G + 24966 B) / 255000) in integers; the half-size plane is MATLAB's imresize(Y, 0.5)
 * as int32 numerators over 65536 (taps [-3 -9 29 111 111 29 -9 -3] / 256 along each axis, symmetric extension); both are kept in
 * d_work.  Per scale and pixel, over the 7 x 7 window with replicated borders and centre value c: the ten class sums
 * s_k = sum (x - c) and q_k = sum (x - c)^2 (class (a, b), 0 <= a <= b <= 3, by {|di|, |dj|}; exact integers),
 * m = sum_k w_k s_k, v = sum_k w_k q_k in ascending class order with separate multiply and add, sigma = sqrt(|v - m m|),
 * mscn = (0 - m) / (sigma + 1).  h_weights: HOST array of the ten class weights w_k = g[3 + a] g[3 + b] of the normalised 7-tap
 * Gaussian of sigma 7 / 6 (niqe.window_weights), each in (0, 1); they travel as kernel arguments.
 * d_stats[b][ih][iw][scale][map][5] (fp64): for block (ih, iw) of 96 x 96 (scale 0) or 48 x 48 (scale 1) samples and the maps
 * n, n roll(n, (0,1)), n roll(n, (1,0)), n roll(n, (1,1)), n roll(n, (1,-1)) (circular inside the block): the count of samples < 0,
 * the count > 0, the sum of squares of each kind, and the sum of |.|.  d_sharp[b][ih][iw]: the mean of sigma over the scale-0 block.
 * Three launches whatever B is; reductions in a fixed order, no float atomics: the same input gives the same bits.
 * d_work: 16-byte aligned, at least the *bytes sgic_niqe_u8_work_bytes returns (host-only, takes no stream).  1 <= B <= 65536,
 * 96 <= H, W <= 16384; anything else, a null pointer, a misaligned or too small workspace is SGIC_EINVAL before any launch. */
int sgic_niqe_u8_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_niqe_u8(const uint8_t *d_img, int B, int H, int W, const double *h_weights, uint8_t *d_work, size_t work_bytes,
                 double *d_stats, double *d_sharp, sgic_stream_t stream);

/* The hand-crafted full-reference measures of evaluate.py --hvs (quality.measure_hvs), all on fp64 luma and
 * all in fp64.  sgic_hvs_luma_u8: d_img (B, H, W, 3) interleaved RGB -> d_y (B, H, W), Y = (0.299 R + 0.587 G) + 0.114 B on the
 * 0..255 scale, unrounded, one multiply or add per written operation.  The three measures take the luma planes of the originals
 * (d_ya) and of the reconstructions (d_yb).  Each reduces a tile (block group) in a workgroup and combines the partials of one image
 * in a fixed order (no float atomics): the same image gives the same bits whatever batch it comes in.
 *
 * sgic_hvs_vifp: pixel-domain VIF with sigma_n^2 = 2.  Scales s = 1..4 with the N x N window N = 2^(5 - s) + 1 (17, 9, 5, 3),
 * g_i = exp(-(i - N / 2)^2 / (2 (N / 5)^2)) / sum along each axis; for s > 1 both planes are first filtered with that window (valid
 * support) and every second row and column is kept, starting at 0 (planes kept in d_work).  At every scale, with the same window
 * and valid support: mu1, mu2, s1 = E[xx] - mu1^2, s2 = E[yy] - mu2^2, s12 = E[xy] - mu1 mu2; then with eps = 1e-10, in this
 * order: s1, s2 < 0 -> 0; g = s12 / (s1 + eps), sv = s2 - g s12; s1 < eps: g = 0, sv = s2, s1 = 0; s2 < eps: g = 0, sv = 0;
 * g < 0: sv = s2, g = 0; sv <= eps: sv = eps.  d_out[b] = {sum log10(1 + g^2 s1 / (sv + 2)), sum log10(1 + s1 / 2)} over all
 * scales and samples; the caller divides.  41 <= H, W: below that scale 4 has no sample.
 *
 * sgic_hvs_gmsd: the 2 x 2 mean of Y at every second row and column starting at 0 (samples past the plane count 0: MATLAB's
 * conv2(Y, ones(2) / 4, 'same') then (1:2:end, 1:2:end)), Prewitt gradients [[1, 0, -1]] x 3 / 3 and its transpose with zero
 * padding, m = sqrt(gx^2 + gy^2), GMS = (2 m1 m2 + 170) / (m1^2 + m2^2 + 170); d_out[b] = the population standard deviation of
 * the GMS map, from per-tile (count, mean, sum of squared deviations from the tile's mean) merged pairwise in a fixed order.
 *
 * sgic_hvs_psnr: non-overlapping 8 x 8 blocks from the top left (partial blocks ignored), orthonormal DCT-II D of both blocks.
 * h_q: HOST array, the 64 steps of a quantisation table in natural order, each in 1..255 (T.81 Annex K.1 luminance for the
 * published measure); MaskCof = (10 / Q)^2, CSFCof = 2.5735088 (10 / Q).  Per image's block: m = sum over the 63 AC coefficients
 * of D^2 MaskCof; vari(X) = the unbiased variance of X times its element count; pop = vari(block), and where that is not 0,
 * pop = (sum of vari over the four 4 x 4 quadrants) / pop; mask = sqrt(m pop) / 32, the larger of the two images' masks.
 * u = |Da - Db|; with masking every AC coefficient has u = 0 where u < mask / MaskCof and u - mask / MaskCof elsewhere; the
 * block's error is sum (u CSFCof)^2.  d_out[b] = {sum of the block errors without masking (PSNR-HVS), with masking (PSNR-HVS-M)};
 * the caller divides by 64 (H / 8) (W / 8) and takes 10 log10(255^2 / .).  8 <= H, W.
 *
 * d_work: 16-byte aligned, at least the *bytes the measure's _work_bytes call returns (host-only, takes no stream).
 * 1 <= B <= 65536, H, W <= 16384; anything else, a null pointer, a misaligned or too small workspace is SGIC_EINVAL before any
 * launch. */
int sgic_hvs_luma_u8(const uint8_t *d_img, int B, int H, int W, double *d_y, sgic_stream_t stream);
int sgic_hvs_vifp_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_hvs_vifp(const double *d_ya, const double *d_yb, int B, int H, int W, uint8_t *d_work, size_t work_bytes, double *d_out,
                  sgic_stream_t stream);
int sgic_hvs_gmsd_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_hvs_gmsd(const double *d_ya, const double *d_yb, int B, int H, int W, uint8_t *d_work, size_t work_bytes, double *d_out,
                  sgic_stream_t stream);
int sgic_hvs_psnr_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_hvs_psnr(const double *d_ya, const double *d_yb, int B, int H, int W, const int *h_q, uint8_t *d_work, size_t work_bytes,
                  double *d_out, sgic_stream_t stream);

/* FSIM and FSIMc of evaluate.py --fsim (quality.fsim; DESIGN.md section 21 holds the definition), all in fp64.
 *
 * sgic_fsim_planes_u8: d_img (B, H, W, 3) interleaved RGB -> d_out (B, 3, h, w), the reduced Y, I, Q planes: Y = (0.299 R + 0.587 G)
 * + 0.114 B, I = (0.596 R - 0.274 G) - 0.322 B, Q = (0.211 R - 0.523 G) + 0.312 B, unrounded; with F = max(1, floor(min(H, W) /
 * 256 + 0.5)), h = ceil(H / F), w = ceil(W / F), sample (i, j) is the sum over input rows i F + F / 2 - F + 1 .. i F + F / 2 and the
 * same columns (samples outside count 0), added row by row from the lowest offset, divided by F F.
 *
 * sgic_fsim_phasecong: d_planes (B, h, w) -> d_pc (B, h, w), the phase congruency map of every plane (four scales, four
 * orientations, log-Gabor filters built on the device, the 2-D transforms as dense DFT passes with twiddles from a table indexed by
 * (j k) mod n, the noise threshold from the exact median of |EO_0|^2 by a radix select); a plane with max == min gives 0
 * everywhere and no transform runs.  2 <= h, w <= 2048.  Planes are transformed in chunks, so the workspace stays near 512 MiB
 * (one plane's scratch, 368 h w bytes, where that is more).
 *
 * sgic_fsim: d_a (originals), d_b (reconstructions) (B, H, W, 3) -> d_fsim[B], d_fsimc[B]: the reduced planes, the PC maps of
 * both Y planes, Scharr gradient magnitudes, and sum(Spc Sg PCm) / sum(PCm) without and with the chroma term.  Tile partials are
 * combined per pair in a fixed order (no float atomics): a pair gives the same bits whatever batch and slot it comes in.  Where
 * sum(PCm) is 0 both values are 1 if the reduced planes of the two images are equal, else 0.  2 <= H, W and max(h, w) <= 2048.
 *
 * d_work: 16-byte aligned, at least the *bytes the _work_bytes call returns (host-only, takes no stream).  1 <= B <= 65536,
 * H, W <= 16384; anything else, a null pointer, a misaligned or too small workspace is SGIC_EINVAL before any launch. */
int sgic_fsim_planes_u8(const uint8_t *d_img, int B, int H, int W, double *d_out, sgic_stream_t stream);
int sgic_fsim_phasecong_work_bytes(int B, int h, int w, size_t *bytes);
int sgic_fsim_phasecong(const double *d_planes, int B, int h, int w, uint8_t *d_work, size_t work_bytes, double *d_pc,
                        sgic_stream_t stream);
int sgic_fsim_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_fsim(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, uint8_t *d_work, size_t work_bytes, double *d_fsim,
              double *d_fsimc, sgic_stream_t stream);

/* LPIPS with the VGG16 trunk (lpips.LpipsVGG, evaluate.py --lpips_ckpt; the reference's taming/modules/losses/lpips.py): the
 * memory-bound glue around sgic_conv3x3_split3_f32, which runs the thirteen convolutions.  All planes are slice-major (a_packed = 1).
 *
 * sgic_lpips_input_split3: d_img (B, H, W, 3) u8 -> the interior of the zero-halo planes [3][1][total_images (H+2) (W+2)][32] of
 * images image_offset .. image_offset + B - 1 (two calls fill one buffer with both sides of the pairs).  Per channel c, each step one
 * IEEE fp32 operation: x = float(u) / 255 * 2 - 1; y = (x - shift_c) / scale_c with shift = (-.030, -.088, -.188), scale = (.458,
 * .448, .450).  Channels 3..31 are written as zero; the border is not written.
 *
 * sgic_relu_pool_halo_split3: d_in (B H W, C) fp32 -> relu -> (pool2x2: max over 2 x 2, stride 2, an odd last row / column dropped)
 * -> the interior of the planes [3][C / 32][B (H'+2) (W'+2)][32]; only the interior is written (the sgic_halo_copy_split3 contract).
 *
 * sgic_lpips_head: d_feat (2 B H W, C) fp32 BEFORE relu, image pair b = rows of image b and of image B + b; d_w (C).  With f =
 * relu(feat), n = sqrt(sum_c f_c^2), u = f * (1 / (n + 1e-10)): d_d[b] = mean over pixels of sum_c w_c (u_a - u_b)^2, in fp64 (an
 * all-zero pixel gives u = 0).  One partial per workgroup in d_work, added in a fixed order by a last kernel: no float atomics, the
 * same input gives the same bits.  d_work: at least the *bytes sgic_lpips_head_work_bytes returns (host-only, takes no stream).
 *
 * SGIC_EINVAL before any launch: a null pointer, B < 1 (head: B > 65535), H or W < 1, C % 32 != 0, a buffer that is not 16-byte
 * aligned, image slots outside total_images, a pool of fewer than two rows or columns, a workspace that is too small. */
int sgic_lpips_input_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset, uint16_t *d_halo_planes,
                            sgic_stream_t stream);
int sgic_relu_pool_halo_split3(const float *d_in, int B, int H, int W, int C, int pool2x2, uint16_t *d_halo_planes,
                               sgic_stream_t stream);
int sgic_lpips_head_work_bytes(int B, int H, int W, size_t *bytes);
int sgic_lpips_head(const float *d_feat, const float *d_w, int B, int H, int W, int C, uint8_t *d_work, size_t work_bytes,
                    double *d_d, sgic_stream_t stream);

/* DISTS with the VGG16 trunk (dists.DistsVGG, evaluate.py --dists_ckpt; DISTS_pytorch / piq.DISTS): the
 * memory-bound glue around sgic_conv3x3_split3_f32, which runs the same thirteen convolutions as for LPIPS.  All planes are slice-major
 * (a_packed = 1) with a zero halo; only the interior is written (the sgic_halo_copy_split3 contract).
 *
 * sgic_dists_input_split3: as sgic_lpips_input_split3 with another input layer.  Per channel c, each step one IEEE fp32 operation:
 * x = float(u) / 255; y = (x - mean_c) / std_c with mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225).
 *
 * sgic_dists_moments_u8 (tap 0): d_a, d_b (B, H, W, 3) u8 -> d_sums (B, 3, 5) int64 = (sum a, sum b, sum a^2, sum b^2, sum a b) over
 * the pixels of every pair and channel, exact (the entry clears d_sums first; 64-bit integer adds).
 *
 * sgic_relu_l2pool_halo_split3: d_in (B H W, C) fp32 BEFORE relu -> relu -> square -> the window g = (1, 2, 1) x (1, 2, 1) / 16 (the
 * normalised 3x3 Hanning window) at stride 2 with zero padding 1 -> + 1e-12 -> sqrt -> the interior of the planes [3][C / 32][B (H'+2)
 * (W'+2)][32], H' = (H + 1) / 2, W' = (W + 1) / 2.  fp32, the nine terms added in row-major order of the window, first to last.
 *
 * sgic_dists_moments: d_feat (2 B H W, C) fp32 BEFORE relu, pair b = rows of image b and of image B + b -> d_sums (B, 5, C) fp64 = (sum
 * x, sum y, sum x^2, sum y^2, sum x y) over the pixels, x = relu of the first side, y of the second; the products are exact in fp64.
 * A workgroup writes one partial per channel into d_work, a second kernel adds the partials in a fixed order: no float atomics, the
 * same input gives the same bits.  d_work: at least the *bytes sgic_dists_moments_work_bytes returns (host-only, takes no stream).
 *
 * sgic_dists_head: d_sums (B, 5, C) of sgic_dists_moments, d_alpha, d_beta (C) fp32 -> d_terms (B, 2) fp64 = (sum_c alpha_c (1 - S1_c),
 * sum_c beta_c (1 - S2_c)) with n = H W, mu = sum / n, var_x = sum x^2 / n - mu_x mu_x, cov = sum x y / n - mu_x mu_y (one expression, so
 * x == y gives exactly 0 for both), S1 = (2 mu_x mu_y + 1e-6) / (mu_x^2 + mu_y^2 + 1e-6), S2 = (2 cov + 1e-6) / (var_x + var_y + 1e-6).
 * The channels are added in a fixed order.
 *
 * SGIC_EINVAL before any launch: a null pointer, B < 1 (B > 65535 where pairs are grid rows), H or W < 1, C % 32 != 0 (moments: C >
 * 1024), a misaligned buffer (16 bytes for planes, features and workspace, 8 for int64 / fp64), image slots outside total_images, a
 * workspace that is too small. */
int sgic_dists_input_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset, uint16_t *d_halo_planes,
                            sgic_stream_t stream);
int sgic_dists_moments_u8(const uint8_t *d_a, const uint8_t *d_b, int B, int H, int W, int64_t *d_sums, sgic_stream_t stream);
int sgic_relu_l2pool_halo_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_halo_planes, sgic_stream_t stream);
int sgic_dists_moments_work_bytes(int B, int H, int W, int C, size_t *bytes);
int sgic_dists_moments(const float *d_feat, int B, int H, int W, int C, uint8_t *d_work, size_t work_bytes, double *d_sums,
                       sgic_stream_t stream);
int sgic_dists_head(const double *d_sums, const float *d_alpha, const float *d_beta, int B, int H, int W, int C, double *d_terms,
                    sgic_stream_t stream);

/* LPIPS with the AlexNet trunk (lpips_alex.LpipsAlex, evaluate.py --lpips_alex_ckpt; lpips.LPIPS(net="alex")):
 * the producers of the operands that the 3x3 path cannot take.  All planes are slice-major bf16x3 (a_packed = 1).
 *
 * sgic_lpips_alex_conv1_patches_split3: d_img (B, H, W, 3) u8 -> rows image_offset h1 w1 .. of the A operand [3][12][total_images h1
 * w1][32] of the 11x11 / stride 4 / pad 2 convolution as a GEMM, h1 = (H - 7) / 4 + 1, w1 = (W - 7) / 4 + 1.  Row (img, oy, ox),
 * column k = (ky 11 + kx) 3 + c, k < 363: the input layer of sgic_lpips_input_split3 at pixel (4 oy - 2 + ky, 4 ox - 2 + kx), 0 when
 * that pixel is outside the image; columns 363..383 are 0.  Two calls fill one buffer with both sides of the pairs; the rows of
 * other images are not touched.
 *
 * sgic_relu_maxpool3_patches5_split3: d_in (B H W, C) fp32 BEFORE relu -> relu -> max over 3 x 3, stride 2, no padding, floor, to PH
 * x PW (PH = (H - 3) / 2 + 1) -> the A operand [3][25 C / 32][B PH PW][32] of the 5x5 / pad 2 convolution as a GEMM: column k = (ky 5
 * + kx) C + c of row (b, oy, ox) is the pooled value at (oy + ky - 2, ox + kx - 2), 0 outside the pooled map.  Every element is
 * written.
 *
 * sgic_relu_maxpool3_halo_split3: the same relu and pool -> the interior of the zero-halo planes [3][C / 32][B (PH+2) (PW+2)][32], the
 * input of sgic_conv3x3_split3_f32; only the interior is written (the sgic_halo_copy_split3 contract).
 *
 * SGIC_EINVAL before any launch: a null pointer, B < 1, H or W < 7 (the pools: < 3), C % 32 != 0, a buffer that is not 16-byte
 * aligned (the u8 image may sit anywhere), image slots outside total_images, 2^31 or more rows. */
int sgic_lpips_alex_conv1_patches_split3(const uint8_t *d_img, int B, int H, int W, int total_images, int image_offset,
                                         uint16_t *d_planes, sgic_stream_t stream);
int sgic_relu_maxpool3_patches5_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_planes, sgic_stream_t stream);
int sgic_relu_maxpool3_halo_split3(const float *d_in, int B, int H, int W, int C, uint16_t *d_halo_planes, sgic_stream_t stream);

/* FID and KID (fid.InceptionFID, evaluate.py --fid_ckpt; pytorch-fid's InceptionV3 at pool3).  Every convolution
 * of the graph is sgic_gemm_split3_f32 over the planes that sgic_patches_split3 writes (slice-major bf16x3, a_packed = 1); every
 * activation is stored BEFORE its ReLU and its consumers apply it on read.
 *
 * sgic_fid_resize299: d_canvas (B, H, W, 3) u8 and n descriptors (image, y0, x0, h, w), int32, once on the host (h_desc: checked here)
 * and once on the device (d_desc: read by the kernel; the same values) -> d_out (n, 299, 299, 3) fp32: x = u / 255, the h x w window
 * at (y0, x0) of the image resized bilinearly to 299 x 299 with src = max((dst + 0.5) in / 299 - 0.5, 0) (the position exactly, in
 * integers: floor and remainder of ((2 dst + 1) in - 299) / 598), the neighbour clamped to in - 1, within rows first, then between
 * rows, with weights (1 - lambda, lambda); then 2 x - 1.
 *
 * sgic_patches_split3: d_in fp32 NHWC rows of leading dimension ld, columns col0 .. col0 + C - 1 (a slice of a concat buffer) ->
 * relu when `relu` -> the kh x kw patches at stride (sh, sw) with zero padding (ph, pw), OH = (H + 2 ph - kh) / sh + 1, as the A
 * operand [3][Kp / 32][B OH OW][32], Kp = ceil(kh kw C / 32) 32: column k = (ky kw + kx) C + c of row (b, oy, ox) is the input at
 * (oy sh - ph + ky, ox sw - pw + kx), 0 outside the map and for k >= kh kw C.  Every element is written.  Any C >= 1; C % 8 == 0 with
 * ld % 4 == 0, col0 % 4 == 0 and a 16-byte aligned d_in takes the vector path.  kh = kw = 1: relu + pack.
 *
 * sgic_relu_maxpool3s2 / sgic_relu_avgpool3s1p1 / sgic_relu_maxpool3s1p1: d_in (B H W, C) fp32 -> relu -> max over 3 x 3 at stride
 * 2 without padding (floor) / the mean over the taps of a 3 x 3 window at stride 1, padding 1, that lie inside the map (summed in
 * row-major order in fp32, divided once by their number) / max over the same window -> fp32 rows of leading dimension ldo at column
 * co (a slice of a concat buffer).  C % 4 == 0, ldo % 4 == 0, co % 4 == 0.
 *
 * sgic_relu_mean_rows: d_in (B R, C) fp32 -> d_out (B, C): (relu(row 0) + relu(row 1) + ... + relu(row R - 1), one fp32 accumulator,
 * in that order) / R.  The order does not depend on B.
 *
 * sgic_gram_f64: d_c[i][j] (n x m, leading dimension ldc, fp64) = sum_k A[ia[i]][k] B[ib[j]][k], k = 0 .. K - 1 in order in one fp64
 * accumulator per element, from fp32 rows (leading dimensions lda, ldb).  d_ia / d_ib: int32 row indices on the device or NULL (row
 * i itself); an index outside [0, rows_a) (resp. rows_b) reads as a row of zeros, never memory.
 *
 * SGIC_EINVAL before any launch: a null pointer, an empty extent, planes or pool buffers that are not 16-byte aligned, a descriptor
 * outside the canvas, a column slice outside its leading dimension, 2^31 or more rows. */
int sgic_fid_resize299(const uint8_t *d_canvas, int B, int H, int W, const int32_t *h_desc, const int32_t *d_desc, int n, float *d_out,
                       sgic_stream_t stream);
int sgic_patches_split3(const float *d_in, int ld, int col0, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                        int relu, uint16_t *d_planes, sgic_stream_t stream);
int sgic_relu_maxpool3s2(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream);
int sgic_relu_avgpool3s1p1(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream);
int sgic_relu_maxpool3s1p1(const float *d_in, int B, int H, int W, int C, float *d_out, int ldo, int co, sgic_stream_t stream);
int sgic_relu_mean_rows(const float *d_in, int B, int R, int C, float *d_out, sgic_stream_t stream);
int sgic_gram_f64(const float *d_a, long lda, const int32_t *d_ia, int rows_a, int n, const float *d_b, long ldb, const int32_t *d_ib,
                  int rows_b, int m, int K, double *d_c, long ldc, sgic_stream_t stream);

/* F.pad(x, (pl, pr, pt, pb), mode="replicate") on (BC, H, W) fp32 planes -> (BC, H+pt+pb, W+pl+pr)
 * (compress.py:258-261: every image is padded to a multiple of 256 before the encoder). */
int sgic_pad_replicate(const float *d_in, float *d_out, int BC, int H, int W, int pl, int pr, int pt, int pb,
                       sgic_stream_t stream);

/* Image ingest: decoded RGB u8 HWC (B, H, W, 3) on the device -> `transforms.ToTensor()(img) * 2.0 - 1.0` (compress.py:
 * 151-168) -> NCHW fp32 with F.pad(mode="replicate") fused (compress.py:258-261); out is (B, 3, H+pt+pb, W+pl+pr).
 * Bit-identical to the torch ops (one IEEE division, multiply, subtract per sample). */
int sgic_u8hwc_to_f32chw_pad(const uint8_t *d_in, float *d_out, int B, int H, int W, int pl, int pr, int pt, int pb,
                             sgic_stream_t stream);

/* Ragged batches: images of different sizes that pad to one geometry share a batch (sgic_amd/ingest.py pad_to).  The per-image
 * geometry is a HOST array, validated on the host and handed to the kernels as launch arguments (32 images per launch).
 *
 * Ragged ingest: d_in is a u8 canvas (B, Hc, Wc, 3) with image b at its top left, extent h_hw[2b] x h_hw[2b+1] (host int32, B x 2;
 * 1 <= h <= min(Hc, OH), 1 <= w <= min(Wc, OW)) -> d_out (B, 3, OH, OW) fp32: ToTensor, *2-1 and replicate padding from the
 * image's OWN right / bottom edge.  Bit-identical per image to sgic_u8hwc_to_f32chw_pad(pl = pt = 0) on that image alone. */
int sgic_u8canvas_to_f32chw_pad(const uint8_t *d_in, const int32_t *h_hw, float *d_out, int B, int Hc, int Wc, int OH, int OW,
                                sgic_stream_t stream);
/* Pillow's bicubic tables of an in_size -> out_size resample built on the device, in double precision in the operation order of
 * Pillow's precompute_coeffs (sgic_amd/clip.py pil_coeffs): d_bounds (out_size x 2 int32: first input index, count), d_kk
 * (out_size x ksize 22-bit fixed-point int32, zero past the count); ksize = ceil(2 * max(in_size / out_size, 1)) * 2 + 1 (checked). */
int sgic_clip_resize_coeffs(int in_size, int out_size, int ksize, int32_t *d_bounds, int32_t *d_kk, sgic_stream_t stream);
/* CLIP preprocessing of an fp32 batch, bit-exact with ToPILImage -> PIL bicubic antialias resize -> centre crop -> ToTensor ->
 * Normalize (compress.py:70-71): u8 = trunc((clamp(x, -1, 1) * 0.5 + 0.5) * 255), Pillow's two 8-bit passes with its 22-bit
 * fixed-point coefficients, (v / 255 - mean) / std.  Image b is the top-left H x W region of d_x[b] (element strides: img_stride
 * between images, ch_stride between channels, ldx between rows, 1 between columns), with its own resize geometry
 * h_geo[6b .. 6b+5] = (H, W, OH, OW, top, left) (host int32, B x 6; sgic_amd/clip.py resize_geometry; H, W <= 65535, OH, OW < 2^30)
 * -> d_out (B, 3, S, S).  An image's bits do not depend on the rest of the batch.  The coefficient tables are built on the device.
 * The horizontal pass covers the S cropped columns of the source rows the vertical pass reads -- bounds_v[top].first up to
 * bounds_v[top + S - 1].first + count -- and leaves them as a 3 x rows x S u8 intermediate, rows: a bound of that window computed
 * on the host from the geometry alone (<= H).  d_work: a device workspace (16-byte aligned) of at least the *bytes
 * sgic_clip_preprocess_ragged_workspace returns (host-only, takes no stream); per image, in batch order: bounds_h (OW x 2 int32),
 * kk_h (OW x ksize_h), bounds_v (OH x 2), kk_v (OH x ksize_v), the planar u8 image (3 x H x W) and the intermediate (3 x rows x S),
 * each 16-byte aligned. */
int sgic_clip_preprocess_ragged_workspace(int B, const int32_t *h_geo, int S, size_t *bytes);
int sgic_clip_preprocess_ragged(const float *d_x, long img_stride, long ch_stride, int ldx, int B, const int32_t *h_geo, int S,
                                const float *mean3, const float *std3, uint8_t *d_work, size_t work_bytes, float *d_out,
                                sgic_stream_t stream);
/* CLIP preprocessing straight from the u8 canvas of the ingest: d_canvas (B, Hc, Wc, 3) interleaved RGB, image b its top-left H x W
 * region with h_geo[6b .. 6b+5] = (H, W, OH, OW, top, left) as above (H <= Hc, W <= Wc; bytes of the canvas outside an image are
 * never read) -> d_out (B, 3, S, S) fp32.  The bytes are resampled as they are -- bit-identical to Pillow's
 * `Image.fromarray(u8).resize((OW, OH), BICUBIC)`, centre crop, / 255, (v - mean) / std -- where the fp32 entry point above first
 * truncates `(x * 0.5 + 0.5) * 255` back to u8.  There is no fp32 image and no planar u8 copy: the horizontal pass reads the canvas;
 * tables, row window, intermediate and vertical pass are those of the fp32 entry point (the same kernels).  d_work: a device
 * workspace (16-byte aligned) of at least the *bytes sgic_clip_preprocess_u8canvas_workspace returns (host-only, takes no stream);
 * per image, in batch order: the four tables and the intermediate (3 x rows x S u8) as above, each 16-byte aligned. */
int sgic_clip_preprocess_u8canvas_workspace(int B, const int32_t *h_geo, int S, size_t *bytes);
int sgic_clip_preprocess_u8canvas(const uint8_t *d_canvas, int Hc, int Wc, int B, const int32_t *h_geo, int S, const float *mean3,
                                  const float *std3, uint8_t *d_work, size_t work_bytes, float *d_out, sgic_stream_t stream);

/* Baseline JPEG decode of a batch of B equal-geometry files to RGB u8 HWC (B, H, W, 3) on the device -- the pixel decode inside
 * the reference's Test_Dataset (`Image.open(path).convert("RGB")`, compress.py:151-168), bit-exact with Pillow / libjpeg-turbo's
 * default decoder (islow IDCT, fancy chroma upsampling, jdcolor tables).  The host parses markers and strips byte stuffing
 * (sgic_amd/jpeg.py); Huffman decoding, IDCT, upsampling and colour conversion run here.  d_params: B x 64 int32 descriptors,
 * d_scan: cleaned entropy-coded segments (each padded to a multiple of 2048 B), d_tabs: B x 4 lookup tables of 1424 B,
 * d_segs: restart-interval byte offsets, d_quant: u16 tables in natural order -- these five may be device memory or PINNED host
 * memory (the kernels then pull the compressed bytes over PCIe themselves and no H2D copy exists); d_work_params (B x 64 int32),
 * d_work_quant (B x 256 u16), d_coef, d_planes: device workspaces; d_err[b]: 0 ok / 1 invalid code / 2 missing restart segment /
 * 3 the scan ended before the last MCU (more bytes consumed than its unpadded length, d_params[b][14]). */
int sgic_jpeg_decode_batch(const int32_t *d_params, const uint8_t *d_scan, const uint8_t *d_tabs, const int32_t *d_segs,
                           const uint16_t *d_quant, int32_t *d_work_params, uint16_t *d_work_quant, int16_t *d_coef,
                           uint8_t *d_planes, uint8_t *d_out, int32_t *d_err, int B, int H, int W, int max_blocks,
                           sgic_stream_t stream);

/* Multi-scan JPEG decode (progressive Huffman, T.81 Annex G; multi-scan sequential; baseline files as one scan each, so mixed
 * batches decode together) of a batch of B equal-geometry files to RGB u8 HWC (B, H, W, 3), bit-exact with Pillow / libjpeg-turbo
 * for files it takes (the host refuses those on which libjpeg would run block smoothing).  The host parses every scan and strips
 * byte stuffing (sgic_amd/jpeg.py ScanJpegBatch); d_descs: 32-int32 scan descriptors sorted by dependency level -- level l is
 * [h_level_start[l], h_level_start[l + 1]) of the HOST array h_level_start (nlevels + 1 entries), one launch per level, one wave per
 * scan; d_tabs: the batch's deduplicated Huffman lookup-table pool.  d_coef (total_blocks * 64 int16) is zeroed here.  Other
 * arguments as sgic_jpeg_decode_batch; d_err[b]: 0 ok / 1 invalid code / 2 missing restart segment / 3 coefficient past its band, or
 * the scan ended before its last unit (more bytes consumed than its unpadded length, descriptor slot 29). */
int sgic_jpeg_decode_scans_batch(const int32_t *d_params, const int32_t *d_descs, const uint8_t *d_scan, const uint8_t *d_tabs,
                                 const int32_t *d_segs, const uint16_t *d_quant, int32_t *d_work_params, uint16_t *d_work_quant,
                                 int16_t *d_coef, uint8_t *d_planes, uint8_t *d_out, int32_t *d_err, int B, int H, int W,
                                 long total_blocks, int max_blocks, const int32_t *h_level_start, int nlevels,
                                 sgic_stream_t stream);

/* Baseline JPEG encode of a batch of B equal-geometry images on the device: d_rgb (B, H, W, 3) u8 interleaved RGB -> for image b
 * the entropy-coded segment followed by FF D9 in d_out[b * cap .. b * cap + d_len[b]), the very bytes that Pillow / libjpeg-turbo's
 * `save(format="JPEG", quality, subsampling)` writes after its SOS header for the same pixels and tables (jccolor, jcsample without
 * smoothing, jfdctint islow, the Annex K Huffman tables, no restart markers).  The header is the host's (sgic_amd/jpeg_enc.py).
 * subsampling: Pillow's 0 (4:4:4), 1 (4:2:2), 2 (4:2:0).  h_qt: HOST array (B, 2, 64) u16, luma and chroma quantisation table of
 * every image in natural order, entries in [1, 255]; checked here and uploaded on the stream.  Limits: 1 <= H, W <= 16384 and at
 * most 2581110 coded 8 x 8 blocks per image (dummy blocks of partial MCUs included), so that a bit offset within an image fits 32
 * bits; offsets across images are 64-bit.  cap: bytes per slot, at least sgic_jpeg_encode_cap's (416 per coded block + 2: the
 * largest code of a block is 208 bytes, doubled for byte stuffing) and below 2^31.  d_work: a device workspace (16-byte aligned) of
 * at least sgic_jpeg_encode_work_bytes.  d_err[b] != 0 and d_len[b] = 0 if a slot was too small (with the computed cap it is not).
 * Every bad argument is SGIC_EINVAL before anything is launched.  The two helpers are host-only and take no stream. */
int sgic_jpeg_encode_cap(int H, int W, int subsampling, size_t *cap);
int sgic_jpeg_encode_work_bytes(int B, int H, int W, int subsampling, size_t *bytes);
int sgic_jpeg_encode_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt, uint8_t *d_work,
                           size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err, sgic_stream_t stream);

/* The same with optimised Huffman tables: the bytes that `save(format="JPEG", quality, subsampling, optimize=True)` writes after its
 * SOS header.  Per image the symbols of the scan are counted (dummy blocks included) and libjpeg's jpeg_gen_optimal_table makes the
 * four tables from the counts, all on the device.  d_huff (B, 4, 272) u8, 4-byte aligned: BITS (16 bytes) and HUFFVAL (256 bytes,
 * zeros past the table's symbols) of image b's tables in the header's order DC0, AC0, DC1, AC1; d_nval (B, 4) int32: the number of
 * HUFFVAL entries of each, so a DHT segment is 2 + 2 + 1 + 16 + d_nval bytes.  The host writes the header from them.  A fitted code
 * may be 16 bits long for any symbol, so a block can take 16 + 11 + 63 * 26 = 1665 bits: cap is at least sgic_jpeg_encode_opt_cap's
 * (424 per coded block + 2), the workspace sgic_jpeg_encode_opt_work_bytes', and an image has at most 2579559 coded blocks.  Every
 * other argument, the refusals (also for a null or misaligned d_huff or d_nval) and the overflow contract are those of
 * sgic_jpeg_encode_batch.  Where a code would be longer than 32 bits before the length limiter (libjpeg ends with an error there; it
 * takes counts in Fibonacci proportions that sum past 9.2 million in one table), d_err[b] = 2, d_len[b] = 0 and that table's d_nval
 * entry is -1. */
int sgic_jpeg_encode_opt_cap(int H, int W, int subsampling, size_t *cap);
int sgic_jpeg_encode_opt_work_bytes(int B, int H, int W, int subsampling, size_t *bytes);
int sgic_jpeg_encode_opt_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt, uint8_t *d_work,
                               size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err, uint8_t *d_huff,
                               int32_t *d_nval, sgic_stream_t stream);

/* The progressive file: what `save(format="JPEG", quality, subsampling, progressive=True)` writes, scan by scan.  The coefficients are
 * those of the calls above; they are coded in the ten scans of libjpeg's jpeg_simple_progression -- (Y Cb Cr, 0-0, Al 1), (Y, 1-5, Al 2),
 * (Cr, 1-63, Al 1), (Cb, 1-63, Al 1), (Y, 6-63, Al 2), (Y, 1-63, Ah 2 Al 1), (Y Cb Cr, 0-0, Ah 1 Al 0), (Cr, 1-63, Ah 1 Al 0), (Cb, the same),
 * (Y, the same) -- every scan with Huffman tables fitted to its own symbols, all on the device.  Image b's ten entropy-coded
 * segments (each padded with 1-bits to a byte and stuffed on its own, no markers between them, no EOI) lie back to back from
 * d_out[b * cap]; d_len (B, 10) int32 holds their lengths.  d_huff (B, 10, 272) u8 and d_nval (B, 10) int32 are BITS, HUFFVAL and
 * the HUFFVAL counts of the ten tables in file order: DC 0 and DC 1 of the first scan, then the AC table of scans 2, 3, 4, 5, 6, 8, 9,
 * 10 (the seventh scan sends raw bits).  The host places SOF2, the DHT and SOS segments and EOI (sgic_amd/jpeg_enc.py).  A block takes
 * at most 27 bits in the first scan, 1 in the seventh, (Se - Ss + 1) * (26 - Al) + 30 in a first AC scan (30: an EOBRUN symbol and its
 * extra bits) and 63 * 17 + 48 + 30 = 1149 in a refinement scan; the largest, 1605, sets the limit of 2675992 coded blocks per
 * image, so that a bit offset within a scan of an image fits 32 bits.  sgic_jpeg_encode_prog_cap is the sum over the scans of
 * twice their largest stream (for 4:2:0 about 880 bytes per coded block).  It must stay below 2^31 as well: a geometry whose slot
 * would be larger is refused by all three calls, which binds before the block limit at 4:2:2 and 4:2:0 (the largest accepted
 * width at H = 10240 is 8032 and 10144; at 4:4:4 the block limit binds first).  d_err (B): 1 where the slot was too small, 2 where a
 * code of some table would pass 32 bits before limiting (that table's d_nval entry is -1); the image's ten lengths are then 0.
 * Every other argument and the refusals are those of sgic_jpeg_encode_opt_batch. */
int sgic_jpeg_encode_prog_cap(int H, int W, int subsampling, size_t *cap);
int sgic_jpeg_encode_prog_work_bytes(int B, int H, int W, int subsampling, size_t *bytes);
int sgic_jpeg_encode_prog_batch(const uint8_t *d_rgb, int B, int H, int W, int subsampling, const uint16_t *h_qt, uint8_t *d_work,
                                size_t work_bytes, uint8_t *d_out, size_t cap, int32_t *d_len, int32_t *d_err, uint8_t *d_huff,
                                int32_t *d_nval, sgic_stream_t stream);

/* Image.resize for u8 RGB on the device: d_in (B, H, W, 3) -> d_out (B, OH, OW, 3), both contiguous, one geometry per call: the bytes
 * of Pillow's `Image.fromarray(x).resize((OW, OH), filter)` (default box, reducing_gap=None; ImagingResample for 8-bit images).
 * filter: 2 = bicubic, 1 = Lanczos (this ABI's codes; Pillow numbers Image.BICUBIC 3).  Per axis the tables are precompute_coeffs' (22-bit fixed point after
 * normalisation); the horizontal pass runs first and writes u8 (accumulator from 1 << 21, >> 22, clamped), the vertical pass runs the
 * same over that intermediate.  The tables are made on the host inside the call (Lanczos needs the host libm's sin to give Pillow's
 * bits) and uploaded on the stream.  d_work: a device workspace, 16-byte aligned, of at least sgic_resize_u8_work_bytes (host-only,
 * takes no stream; 0 for a geometry the call refuses).  SGIC_EINVAL before any launch, the output untouched, for: B < 1; H, W, OH or
 * OW outside [1, 16384]; a filter other than 1 or 2; a null pointer; a workspace that is misaligned or too small.
 * sgic_resize_u8_coeffs (host-only, takes no stream): the tables of one axis as the call makes them, into HOST arrays h_bounds
 * (out_size x 2: first input index, count) and h_kk (out_size x ksize, zero past the count); ksize =
 * ceil(support * max(in_size / out_size, 1)) * 2 + 1 with support 2 (bicubic) or 3 (Lanczos), checked. */
size_t sgic_resize_u8_work_bytes(int B, int H, int W, int OH, int OW, int filter);
int sgic_resize_u8_coeffs(int in_size, int out_size, int filter, int ksize, int32_t *h_bounds, int32_t *h_kk);
int sgic_resize_u8_batch(const uint8_t *d_in, int B, int H, int W, uint8_t *d_out, int OH, int OW, int filter, uint8_t *d_work,
                         size_t work_bytes, sgic_stream_t stream);

/* CLIP text tower front end: out[b*L+l,:] = table[ids[b,l],:] + pos[l,:] (open_clip CLIP.encode_text, reached from
 * search.py:93-97; ids outside [0,vocab) are clamped).  D multiple of 4. */
int sgic_embed_tokens(const int32_t *d_ids, const float *d_table, const float *d_pos, float *d_out, int B, int L, int D,
                      int vocab, sgic_stream_t stream);
/* CLIP text pooling: out[b,:] = x[b*L + argmax_l ids[b,l], :] (first maximum = the EOT token, the largest BPE id). */
int sgic_gather_eot_rows(const int32_t *d_ids, const float *d_x, int ldx, float *d_out, int B, int L, int D,
                         sgic_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
