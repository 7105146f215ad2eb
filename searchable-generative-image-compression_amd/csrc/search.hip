// Fused exact search over u8 CLIP codes (sgic_amd/search.py CodeIndex): i8 MFMA inner products + top-k in one kernel,
// no score matrix.  With a = c - 128 (i8), S = sum a_q a_d and s_x = sum a_x, the integer
//   N(q, d) = 4 S + 2 s_q + 2 s_d + D  ==  sum (2 c_q - 255)(2 c_d - 255)
// is exact in int32 for D <= 4096.  Ranking key = float(N) * r_d (one RNE conversion, one fp32 multiply), reported score =
// key * r_q; r = 1 / sqrt(sum (2c - 255)^2) comes from the host, the GPU does no sqrt, division or float add, so every bit is
// reproducible in numpy.  Order: key descending, equal keys -> lower database index (IndexFlatIP, topk_rows_kernel).
//
// Grid = (query tiles of 16*QF) x (contiguous ascending database splits).  A workgroup is 4 waves; the query tile sits in LDS
// already in MFMA fragment order, each wave streams its own 16-row database tile from global memory as 16-byte fragments
// (lane l: row l & 15, bytes 64 step + 16 (l >> 4) + j -- the SAME k mapping as the query fragments).  C layout: rows are
// queries (4 (l >> 4) + reg), columns database rows (l & 15).  Candidates that beat the query's running k-th best go to a
// per-query LDS buffer of k + 64 entries (one block iteration adds at most 64 per query); a full buffer is pruned to the best k
// by rank and raises the threshold.  The threshold only moves at block-wide sync points, after which every later candidate has a
// higher index than everything kept, so a strict `>` implements the tie rule.
//
// fp32 queries against the same codes (F32Query, CodeIndex.search_vectors).  The query goes to fixed point,
// Q = clamp(rint(q 2^22), -2^22, 2^22) (NaN -> 0), and is cut into balanced base-256 digits Q = 65536 d2 + 256 d1 + d0 with
// d0, d1 in [-128, 127], d2 in [-64, 64]: three i8 planes, each laid out in LDS exactly like the u8 query tile, quantised in the
// kernel's prologue.  One database fragment feeds three MFMAs, S_p = sum d_p a_d, and
//   M = 2 (65536 S_2 + 256 S_1 + S_0) + sum Q  ==  sum Q (2 c_d - 255)
// in int64 (|M| <= 2^22 255 D needs 41 bits at D = 2048).  Key = float(M) * r_d, score = key * 2^-22 (exact); the candidate
// buffers, pruning, splits and the merge are those of the u8 queries.  D <= 2048: three planes of a 16-query tile plus the
// candidate buffers at k = 128 take 120 KiB of the CU's 160 KiB of LDS, D = 4096 would not fit.
//
// The two query types (U8Query, F32Query) own the prologue, the step loop and the integer of a score; what happens to a score is
// one of three kernels, each compiled for both: search_topk_kernel (candidate buffers), search_range_kernel (append to a list) and
// search_rank_kernel (count the rows that come before one given target row).
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kMaxK = 128;
constexpr int kCandPerIter = 64;   // 4 waves x 16 database rows
constexpr int kMaxSplits = 2048;
constexpr int kLdsBigTile = 80 * 1024;   // the wide query tile is used only while two workgroups still fit a CU

__device__ __forceinline__ bool beats(float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// one wave: keep the best min(c, k) of the c buffered candidates of one query, sorted by (key desc, index asc), in slots 0..;
// c <= k + 64 <= 192, so a lane owns at most 3 entries
__device__ __forceinline__ void prune_wave(float *kq, int *iq, int c, int k, int lane, int *cntp, float *thrp) {
  float ke[3];
  int ie[3], rk[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const int e = lane + 64 * m;
    ke[m] = e < c ? kq[e] : -INFINITY;
    ie[m] = e < c ? iq[e] : 0x7fffffff;
    rk[m] = 0;
  }
  for (int j = 0; j < c; j++) {
    const float kj = kq[j];
    const int ij = iq[j];
#pragma unroll
    for (int m = 0; m < 3; m++) rk[m] += beats(kj, ij, ke[m], ie[m]) ? 1 : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int m = 0; m < 3; m++) {
    if (lane + 64 * m < c && rk[m] < k) {
      kq[rk[m]] = ke[m];
      iq[rk[m]] = ie[m];
      if (rk[m] == k - 1) *thrp = ke[m];
    }
  }
  if (lane == 0) *cntp = c < k ? c : k;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned sum_bytes16(const uint4 &v, unsigned acc) {
  acc = __builtin_amdgcn_sad_u8(v.x, 0u, acc);
  acc = __builtin_amdgcn_sad_u8(v.y, 0u, acc);
  acc = __builtin_amdgcn_sad_u8(v.z, 0u, acc);
  return __builtin_amdgcn_sad_u8(v.w, 0u, acc);
}

__device__ __forceinline__ v4i to_i8x16(const uint4 &v) {   // sixteen u8 codes c -> c - 128 as i8
  v4i r;
  r.x = (int)(v.x ^ 0x80808080u);
  r.y = (int)(v.y ^ 0x80808080u);
  r.z = (int)(v.z ^ 0x80808080u);
  r.w = (int)(v.w ^ 0x80808080u);
  return r;
}

constexpr float kQScale = 4194304.0f;   // 2^22: 2^23 would push the top digit to 128 at q = 1
constexpr int kMaxDimF32Q = 2048;

// sixteen fp32 query coordinates -> fixed point -> one 16-byte fragment per digit plane (byte j = coordinate j); returns sum Q
__device__ __forceinline__ int quantise16(const float4 *__restrict__ src, v4i &p0, v4i &p1, v4i &p2) {
  int sum = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const float4 v = src[w];
    const float x[4] = {v.x, v.y, v.z, v.w};
    unsigned w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      float t = x[b] * kQScale;
      t = t == t ? t : 0.0f;
      const int Q = (int)rintf(fminf(fmaxf(t, -kQScale), kQScale));
      const int d0 = ((Q + 128) & 255) - 128, Q1 = (Q - d0) >> 8;
      const int d1 = ((Q1 + 128) & 255) - 128, d2 = (Q1 - d1) >> 8;
      sum += Q;
      w0 |= (unsigned)(d0 & 255) << (8 * b);
      w1 |= (unsigned)(d1 & 255) << (8 * b);
      w2 |= (unsigned)(d2 & 255) << (8 * b);
    }
    p0[w] = (int)w0;
    p1[w] = (int)w1;
    p2[w] = (int)w2;
  }
  return sum;
}

// sixteen fp32 coordinates of one row -> its fragment in each of the three digit planes (`plane` fragments apart), and into sum Q
__device__ __forceinline__ void stage_f32_fragment(const float *__restrict__ src, v4i *dst, int plane, unsigned long long *sum) {
  v4i p0, p1, p2;
  const int s = quantise16(reinterpret_cast<const float4 *>(src), p0, p1, p2);
  atomicAdd(sum, (unsigned long long)(long long)s);
  dst[0] = p0;
  dst[plane] = p1;
  dst[2 * plane] = p2;
}

// What differs between the query types.  LDS of a tile of QT = 16 QF queries: kPlanes planes of [QF][steps][64 lanes] fragments
// and one Sum per query.  stage() fills both (query rows >= nq repeat row nq - 1), term() is a lane's share of a query's Sum,
// accumulate() adds the steps of this lane's database row (bp: its first fragment) into acc and returns the row's own term,
// key() is the ranking key of (fragment f, register r), scale() takes a key to the reported score.
struct U8Query {
  typedef uint8_t T;
  typedef int Sum;    // s_q + 128 D, the byte sum
  typedef int Term;   // 2 s_q + D
  static constexpr int kPlanes = 1, kWideQF = 4;
  static constexpr bool kSelfJoin = true;

  template <int QF>
  static __device__ __forceinline__ void stage(const T *__restrict__ q, int nq, int qbase, int D, int tid, v4i *A, Sum *sq) {
    const int steps = D >> 6;
    if (tid < 16 * QF) sq[tid] = 0;
    __syncthreads();
    for (int i = tid; i < QF * steps * 64; i += 256) {   // one 16-byte fragment per (query fragment, step, lane)
      const int ln = i & 63, t = i >> 6;
      const int step = t % steps, f = t / steps;
      const int row = f * 16 + (ln & 15);
      int qi = qbase + row;
      qi = qi < nq ? qi : nq - 1;
      const uint4 v = *reinterpret_cast<const uint4 *>(q + (size_t)qi * D + 64 * step + 16 * (ln >> 4));
      atomicAdd(&sq[row], (int)sum_bytes16(v, 0u));
      A[i] = to_i8x16(v);
    }
    __syncthreads();
  }

  static __device__ __forceinline__ Term term(const Sum *sq, int ql, int D) { return 2 * (sq[ql] - 128 * D) + D; }

  template <int QF, int U>
  static __device__ __forceinline__ int accumulate(const v4i *A, const uint4 *bp, int D, int lane, v4i (&acc)[kPlanes][QF]) {
    const int steps = D >> 6;
    unsigned ssum = 0;
    for (int s0 = 0; s0 < steps; s0 += U) {   // U divides steps; the U loads of a round are issued together
      uint4 bv[U];
#pragma unroll
      for (int u = 0; u < U; u++) bv[u] = bp[(s0 + u) * 4];
#pragma unroll
      for (int u = 0; u < U; u++) {
        ssum = sum_bytes16(bv[u], ssum);
        const v4i b = to_i8x16(bv[u]);
#pragma unroll
        for (int f = 0; f < QF; f++)
          acc[0][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[(f * steps + s0 + u) * 64 + lane], b, acc[0][f], 0, 0, 0);
      }
    }
    ssum += __shfl_xor(ssum, 16);
    ssum += __shfl_xor(ssum, 32);
    return 2 * ((int)ssum - 128 * D);   // 2 s_d
  }

  template <int QF>
  static __device__ __forceinline__ float key(const v4i (&acc)[kPlanes][QF], int f, int r, Term tq, int td, float rd) {
    const int N = 4 * acc[0][f][r] + tq + td;
    return (float)N * rd;
  }

  static __device__ __forceinline__ float scale(const float *__restrict__ r_q, int gq) { return r_q[gq]; }

  // a lane's share of N for one (query row, database row) pair in plain integer code: the 16-byte chunks lane, lane + 64, ...
  static __device__ __forceinline__ int pair(const T *__restrict__ q, const uint8_t *__restrict__ d, int D, int lane) {
    int s = 0;
    for (int c = lane; c < (D >> 4); c += 64) {
      const uint4 a = reinterpret_cast<const uint4 *>(q)[c], b = reinterpret_cast<const uint4 *>(d)[c];
      const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 16; j++)
        s += (2 * (int)((aw[j >> 2] >> (8 * (j & 3))) & 255u) - 255) * (2 * (int)((bw[j >> 2] >> (8 * (j & 3))) & 255u) - 255);
    }
    return s;
  }
};

// No byte sums of the database rows are needed (v_d = 2 a_d + 1 turns into the `+ sum Q` term), and no self-join: fp32 queries are
// not the database.
struct F32Query {
  typedef float T;
  typedef unsigned long long Sum;   // sum Q: up to 2^33 at D = 2048
  typedef long long Term;
  static constexpr int kPlanes = 3, kWideQF = 2;
  static constexpr bool kSelfJoin = false;

  template <int QF>
  static __device__ __forceinline__ void stage(const T *__restrict__ q, int nq, int qbase, int D, int tid, v4i *A, Sum *sq) {
    const int steps = D >> 6;
    const int plane = QF * steps * 64;   // fragments per digit plane
    if (tid < 16 * QF) sq[tid] = 0;
    __syncthreads();
    for (int i = tid; i < plane; i += 256) {   // sixteen coordinates -> one fragment in each plane per (query fragment, step, lane)
      const int ln = i & 63, t = i >> 6;
      const int step = t % steps, f = t / steps;
      const int row = f * 16 + (ln & 15);
      int qi = qbase + row;
      qi = qi < nq ? qi : nq - 1;
      stage_f32_fragment(q + (size_t)qi * D + 64 * step + 16 * (ln >> 4), A + i, plane, &sq[row]);
    }
    __syncthreads();
  }

  static __device__ __forceinline__ Term term(const Sum *sq, int ql, int) { return (long long)sq[ql]; }

  template <int QF, int U>
  static __device__ __forceinline__ int accumulate(const v4i *A, const uint4 *bp, int D, int lane, v4i (&acc)[kPlanes][QF]) {
    const int steps = D >> 6;
    const int plane = QF * steps * 64;
    for (int s0 = 0; s0 < steps; s0 += U) {   // U divides steps; the U loads of a round are issued together
      uint4 bv[U];
#pragma unroll
      for (int u = 0; u < U; u++) bv[u] = bp[(s0 + u) * 4];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const v4i b = to_i8x16(bv[u]);
#pragma unroll
        for (int p = 0; p < kPlanes; p++)
#pragma unroll
          for (int f = 0; f < QF; f++)
            acc[p][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[p * plane + (f * steps + s0 + u) * 64 + lane], b, acc[p][f], 0, 0, 0);
      }
    }
    return 0;
  }

  template <int QF>
  static __device__ __forceinline__ float key(const v4i (&acc)[kPlanes][QF], int f, int r, Term tq, int, float rd) {
    const long long M = 2 * (65536LL * acc[2][f][r] + 256LL * acc[1][f][r] + acc[0][f][r]) + tq;
    return (float)M * rd;
  }

  static __device__ __forceinline__ float scale(const float *__restrict__, int) { return 1.0f / kQScale; }

  // a lane's share of M for one (query row, database row) pair in plain integer code, from the digits quantise16 makes
  static __device__ __forceinline__ long long pair(const T *__restrict__ q, const uint8_t *__restrict__ d, int D, int lane) {
    long long m = 0;
    for (int c = lane; c < (D >> 4); c += 64) {
      v4i p0, p1, p2;
      const int sumq = quantise16(reinterpret_cast<const float4 *>(q + 16 * c), p0, p1, p2);
      const v4i b = to_i8x16(reinterpret_cast<const uint4 *>(d)[c]);
      int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int sh = 8 * (j & 3), a = (signed char)(b[j >> 2] >> sh);
        s0 += (signed char)(p0[j >> 2] >> sh) * a;
        s1 += (signed char)(p1[j >> 2] >> sh) * a;
        s2 += (signed char)(p2[j >> 2] >> sh) * a;
      }
      m += 2 * (65536LL * s2 + 256LL * s1 + s0) + sumq;
    }
    return m;
  }
};

// Top-k: r_q is read for u8 queries only (fp32 queries pass nullptr).  LDS: the query tile, the candidate buffers, then the sums.
template <class Query, int QF, int U>
__global__ __launch_bounds__(256) void search_topk_kernel(const typename Query::T *__restrict__ q, const float *__restrict__ r_q,
                                                          const uint8_t *__restrict__ db, const float *__restrict__ r_db, int nq,
                                                          int n, int D, int k, int rows_per_split, int splits, int final_out,
                                                          float *__restrict__ out_key, int *__restrict__ out_idx) {
  constexpr int QT = 16 * QF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int cap = k + kCandPerIter;
  v4i *A = reinterpret_cast<v4i *>(smem);
  float *keys = reinterpret_cast<float *>(smem + (size_t)Query::kPlanes * QT * D);
  int *idxs = reinterpret_cast<int *>(keys + QT * cap);
  int *cnt = idxs + QT * cap;
  float *thr = reinterpret_cast<float *>(cnt + QT);
  typename Query::Sum *sq = reinterpret_cast<typename Query::Sum *>(thr + QT);   // 8-byte aligned: every block before it is

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qbase = blockIdx.x * QT, split = blockIdx.y;

  if (tid < QT) {
    cnt[tid] = 0;
    thr[tid] = -INFINITY;
  }
  Query::template stage<QF>(q, nq, qbase, D, tid, A, sq);

  typename Query::Term tq[QF][4];
  float thr_r[QF][4];
#pragma unroll
  for (int f = 0; f < QF; f++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      tq[f][r] = Query::term(sq, f * 16 + 4 * (lane >> 4) + r, D);
      thr_r[f][r] = -INFINITY;
    }

  const int row0 = split * rows_per_split;
  const int row_end = (n - row0 < rows_per_split) ? n : row0 + rows_per_split;
  for (int base = row0; base < row_end; base += kCandPerIter) {
    const int my = base + wave * 16 + (lane & 15);
    v4i acc[Query::kPlanes][QF];   // zeroed here, not in accumulate(): through its reference that costs registers (an occupancy step)
#pragma unroll
    for (int p = 0; p < Query::kPlanes; p++)
#pragma unroll
      for (int f = 0; f < QF; f++) acc[p][f] = v4i{0, 0, 0, 0};
    const int myc = my < n ? my : n - 1;   // rows >= n are clamped for the loads and masked below
    const uint4 *bp = reinterpret_cast<const uint4 *>(db + (size_t)myc * D) + (lane >> 4);
    const int td = Query::template accumulate<QF, U>(A, bp, D, lane, acc);
    const float rd = r_db[myc];
    const bool valid = my < row_end;
    int any = 0;
#pragma unroll
    for (int f = 0; f < QF; f++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float key = Query::key(acc, f, r, tq[f][r], td, rd);
        if (valid && key > thr_r[f][r]) {
          const int ql = f * 16 + 4 * (lane >> 4) + r;
          const int pos = atomicAdd(&cnt[ql], 1);
          keys[ql * cap + pos] = key;
          idxs[ql * cap + pos] = my;
          any = 1;
        }
      }
    if (__syncthreads_or(any)) {
      for (int ql = wave; ql < QT; ql += 4) {
        const int c = cnt[ql];
        if (c > k) prune_wave(keys + ql * cap, idxs + ql * cap, c, k, lane, &cnt[ql], &thr[ql]);
      }
      __syncthreads();
#pragma unroll
      for (int f = 0; f < QF; f++)
#pragma unroll
        for (int r = 0; r < 4; r++) thr_r[f][r] = thr[f * 16 + 4 * (lane >> 4) + r];
    }
  }
  __syncthreads();
  for (int ql = wave; ql < QT; ql += 4) {
    const int gq = qbase + ql;
    if (gq >= nq) break;
    int c = cnt[ql];
    if (c > 0) prune_wave(keys + ql * cap, idxs + ql * cap, c, k, lane, &cnt[ql], &thr[ql]);
    c = c < k ? c : k;
    const float rq = final_out ? Query::scale(r_q, gq) : 1.0f;
    const size_t o = ((size_t)gq * splits + split) * k;
    for (int j = lane; j < k; j += 64) {
      const float key = j < c ? keys[ql * cap + j] : -INFINITY;
      out_key[o + j] = final_out ? key * rq : key;
      out_idx[o + j] = j < c ? idxs[ql * cap + j] : -1;
    }
  }
}

// per query: k-way selection over the splits' sorted lists (splits ascend in database index, so the index breaks ties)
__global__ __launch_bounds__(256) void search_merge_kernel(const float *__restrict__ ws_key, const int *__restrict__ ws_idx,
                                                           const float *__restrict__ r_q, float scale, int splits, int k,
                                                           float *__restrict__ out_s, int *__restrict__ out_i) {
  __shared__ unsigned short head[kMaxSplits];
  __shared__ float wk[4];
  __shared__ int wi[4], wsp[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t qo = (size_t)blockIdx.x * splits * k;
  const float rq = r_q ? r_q[blockIdx.x] : scale;   // u8 queries: their reciprocal norm; fp32 queries: the constant 2^-22
  for (int s = tid; s < splits; s += 256) head[s] = 0;
  __syncthreads();
  for (int j = 0; j < k; j++) {
    float bk = -INFINITY;
    int bi = 0x7fffffff, bs = -1;
    for (int s = tid; s < splits; s += 256) {
      const int h = head[s];
      if (h >= k) continue;
      const int idx = ws_idx[qo + (size_t)s * k + h];
      if (idx < 0) continue;
      const float key = ws_key[qo + (size_t)s * k + h];
      if (bs < 0 || beats(key, idx, bk, bi)) bk = key, bi = idx, bs = s;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const float ok = __shfl_xor(bk, m);
      const int oi = __shfl_xor(bi, m), os = __shfl_xor(bs, m);
      if (os >= 0 && (bs < 0 || beats(ok, oi, bk, bi))) bk = ok, bi = oi, bs = os;
    }
    if (lane == 0) wk[wave] = bk, wi[wave] = bi, wsp[wave] = bs;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; w++)
        if (wsp[w] >= 0 && (bs < 0 || beats(wk[w], wi[w], bk, bi))) bk = wk[w], bi = wi[w], bs = wsp[w];
      out_s[(size_t)blockIdx.x * k + j] = bs >= 0 ? bk * rq : -INFINITY;
      out_i[(size_t)blockIdx.x * k + j] = bs >= 0 ? bi : -1;
      if (bs >= 0) head[bs]++;
    }
    __syncthreads();
  }
}

// Threshold (range) search: search_topk_kernel's tiles and integer score, no top-k.  Every (query, database row) pair with
//   score = key * scale >= T      (fp32; the bits the top-k search reports: (float(N) * r_d) * r_q, (float(M) * r_d) * 2^-22)
// is appended to one global list (q, d, score) through one 64-bit counter.  A wave that has hits in a step takes one atomic add for
// all of them (ballots + lane ranks place the entries); a step without hits costs one wave-uniform branch.  The counter receives
// every hit, an entry is stored only at a position < capacity: the count stays exact after an overflow and nothing is written past
// capacity.  Query rows >= nq and database rows >= row_end are clamped for the loads and masked where entries are emitted.
// self_join (q == db, u8 queries only): only d > q is emitted, and the row loop starts at the first 64-row step that can hold a
// d > qbase, so the tiles wholly at or below the diagonal are never computed; the diagonal tile is masked per element.
// LDS holds the query tile and its sums only.
template <class Query, int QF, int U>
__global__ __launch_bounds__(256, 4) void search_range_kernel(const typename Query::T *__restrict__ q, const float *__restrict__ r_q,
                                                              const uint8_t *__restrict__ db, const float *__restrict__ r_db, int nq,
                                                              int n, int D, int rows_per_split, float threshold, int self_join,
                                                              unsigned long long capacity, unsigned long long *__restrict__ count,
                                                              int *__restrict__ out_q, int *__restrict__ out_d,
                                                              float *__restrict__ out_score) {
  constexpr int QT = 16 * QF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v4i *A = reinterpret_cast<v4i *>(smem);
  typename Query::Sum *sq = reinterpret_cast<typename Query::Sum *>(smem + (size_t)Query::kPlanes * QT * D);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qbase = blockIdx.x * QT, split = blockIdx.y;
  const bool sj = Query::kSelfJoin && self_join;
  int row0 = split * rows_per_split;
  const int row_end = (n - row0 < rows_per_split) ? n : row0 + rows_per_split;
  if (sj) {   // row0 is a multiple of 64, so is the step that holds qbase + 1
    const int first = (qbase + 1) & ~(kCandPerIter - 1);
    row0 = row0 > first ? row0 : first;
    if (row0 >= row_end) return;   // the whole split lies at or below the diagonal
  }

  Query::template stage<QF>(q, nq, qbase, D, tid, A, sq);

  typename Query::Term tq[QF][4];
  float rq[QF][4];
  const int gq0 = qbase + 4 * (lane >> 4);   // this lane's query of (f, r) is gq0 + 16 f + r
#pragma unroll
  for (int f = 0; f < QF; f++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gq = gq0 + 16 * f + r;
      tq[f][r] = Query::term(sq, f * 16 + 4 * (lane >> 4) + r, D);
      rq[f][r] = Query::scale(r_q, gq < nq ? gq : nq - 1);
    }

  for (int base = row0; base < row_end; base += kCandPerIter) {
    const int my = base + wave * 16 + (lane & 15);
    v4i acc[Query::kPlanes][QF];   // zeroed here, not in accumulate(): through its reference that costs registers (an occupancy step)
#pragma unroll
    for (int p = 0; p < Query::kPlanes; p++)
#pragma unroll
      for (int f = 0; f < QF; f++) acc[p][f] = v4i{0, 0, 0, 0};
    const int myc = my < n ? my : n - 1;   // rows >= n are clamped for the loads and masked below
    const uint4 *bp = reinterpret_cast<const uint4 *>(db + (size_t)myc * D) + (lane >> 4);
    const int td = Query::template accumulate<QF, U>(A, bp, D, lane, acc);
    const float rd = r_db[myc];
    const int qlim = sj ? my : nq;   // queries this lane may emit for: below nq, in a self-join (nq == n) below its own row
    const bool valid = my < row_end;
    float score[QF][4];
    unsigned hits = 0;   // bit 4 f + r
#pragma unroll
    for (int f = 0; f < QF; f++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        score[f][r] = Query::key(acc, f, r, tq[f][r], td, rd) * rq[f][r];
        const bool hit = valid && gq0 + 16 * f + r < qlim && score[f][r] >= threshold;
        hits |= hit ? 1u << (4 * f + r) : 0u;
      }
    if (__ballot(hits != 0) != 0ull) {   // rare: one atomic for all of this wave's hits of the step
      unsigned before[QF * 4];           // entries of (f, r) start this far into the wave's block (wave-uniform)
      unsigned total = 0;
#pragma unroll
      for (int m = 0; m < QF * 4; m++) {
        before[m] = total;
        total += (unsigned)__popcll(__ballot((hits >> m) & 1u));
      }
      unsigned long long start = 0;
      if (lane == 0) start = atomicAdd(count, (unsigned long long)total);
      start = __shfl(start, 0);
#pragma unroll
      for (int f = 0; f < QF; f++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int m = 4 * f + r;
          const unsigned long long mask = __ballot((hits >> m) & 1u);
          if ((hits >> m) & 1u) {
            const unsigned long long pos = start + before[m] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            if (pos < capacity) {
              out_q[pos] = gq0 + 16 * f + r;
              out_d[pos] = my;
              out_score[pos] = score[f][r];   // the value tested above
            }
          }
        }
    }
  }
}

// Rank of a target row: search_topk_kernel's tiles, integer score and tie rule, no candidates.  For query q with target row t
//   rank(q, t) = #{ d in [0, n) : beats(key(q, d), d, key(q, t), t) },
// the position of t in the full ordering the top-k search truncates at k.  search_rank_target_kernel (one wave per query) computes
// the pair's integer in plain integer code -- N and M are exact, so any route to them gives the same integer -- and takes it
// through the scan's float step (one conversion, one multiply): the key goes to the workspace, key * scale to d_score, and d_rank
// is zeroed.  search_rank_kernel then keeps one int32 counter per (fragment, register) in every lane over the whole scan of its
// split; at the end the sixteen lanes of a query are summed by shuffles, the four waves through LDS, and a workgroup with a
// non-zero count takes one global atomic add per query.  Integer adds only: the result does not depend on the schedule.  Targets
// are clamped into [0, n) for the loads (the callers refuse others); query rows >= nq and database rows >= row_end are clamped
// and masked as in the other sinks.  LDS: the query tile, its sums, one counter per query.
template <class Query>
__global__ __launch_bounds__(256) void search_rank_target_kernel(const typename Query::T *__restrict__ q, const float *__restrict__ r_q,
                                                                 const uint8_t *__restrict__ db, const float *__restrict__ r_db,
                                                                 const int *__restrict__ target, int nq, int n, int D,
                                                                 float *__restrict__ tkey, int *__restrict__ rank,
                                                                 float *__restrict__ score) {
  const int lane = threadIdx.x & 63, gq = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gq >= nq) return;
  int t = target[gq];
  t = t < 0 ? 0 : (t < n ? t : n - 1);
  auto N = Query::pair(q + (size_t)gq * D, db + (size_t)t * D, D, lane);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) N += __shfl_xor(N, m);
  if (lane == 0) {
    const float key = (float)N * r_db[t];
    tkey[gq] = key;
    rank[gq] = 0;
    score[gq] = key * Query::scale(r_q, gq);
  }
}

template <class Query, int QF, int U>
__global__ __launch_bounds__(256, 4) void search_rank_kernel(const typename Query::T *__restrict__ q, const uint8_t *__restrict__ db,
                                                             const float *__restrict__ r_db, const int *__restrict__ target,
                                                             const float *__restrict__ tkey, int nq, int n, int D, int rows_per_split,
                                                             int *__restrict__ rank) {
  constexpr int QT = 16 * QF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v4i *A = reinterpret_cast<v4i *>(smem);
  typename Query::Sum *sq = reinterpret_cast<typename Query::Sum *>(smem + (size_t)Query::kPlanes * QT * D);
  int *wcnt = reinterpret_cast<int *>(sq + QT);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qbase = blockIdx.x * QT, split = blockIdx.y;
  const int row0 = split * rows_per_split;
  const int row_end = (n - row0 < rows_per_split) ? n : row0 + rows_per_split;

  if (tid < QT) wcnt[tid] = 0;   // stage() has the barriers
  Query::template stage<QF>(q, nq, qbase, D, tid, A, sq);

  typename Query::Term tq[QF][4];
  float tk[QF][4];
  int tt[QF][4], cnt[QF][4];
  const int gq0 = qbase + 4 * (lane >> 4);   // this lane's query of (f, r) is gq0 + 16 f + r
#pragma unroll
  for (int f = 0; f < QF; f++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int gq = gq0 + 16 * f + r;
      gq = gq < nq ? gq : nq - 1;
      const int t = target[gq];
      tq[f][r] = Query::term(sq, f * 16 + 4 * (lane >> 4) + r, D);
      tk[f][r] = tkey[gq];
      tt[f][r] = t < 0 ? 0 : (t < n ? t : n - 1);
      cnt[f][r] = 0;
    }

  for (int base = row0; base < row_end; base += kCandPerIter) {
    const int my = base + wave * 16 + (lane & 15);
    v4i acc[Query::kPlanes][QF];   // zeroed here, not in accumulate(): through its reference that costs registers (an occupancy step)
#pragma unroll
    for (int p = 0; p < Query::kPlanes; p++)
#pragma unroll
      for (int f = 0; f < QF; f++) acc[p][f] = v4i{0, 0, 0, 0};
    const int myc = my < n ? my : n - 1;   // rows >= n are clamped for the loads and masked below
    const uint4 *bp = reinterpret_cast<const uint4 *>(db + (size_t)myc * D) + (lane >> 4);
    const int td = Query::template accumulate<QF, U>(A, bp, D, lane, acc);
    const float rd = r_db[myc];
    const bool valid = my < row_end;
#pragma unroll
    for (int f = 0; f < QF; f++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        cnt[f][r] += (valid && beats(Query::key(acc, f, r, tq[f][r], td, rd), my, tk[f][r], tt[f][r])) ? 1 : 0;
  }

#pragma unroll
  for (int f = 0; f < QF; f++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int c = cnt[f][r];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) c += __shfl_xor(c, m);   // the sixteen database columns of this query
      if ((lane & 15) == 0 && c) atomicAdd(&wcnt[f * 16 + 4 * (lane >> 4) + r], c);
    }
  __syncthreads();
  if (tid < QT && qbase + tid < nq && wcnt[tid]) atomicAdd(&rank[qbase + tid], wcnt[tid]);
}

struct Plan {
  int qf, qtiles, splits, rows_per_split;
  size_t lds, work_bytes;
};

// the query tile and its sums; with k > 0 the candidate buffers (k + 64 keys and indices), a count and a threshold per query
size_t lds_bytes(bool f32q, int qf, int D, int k) {
  const size_t query = f32q ? (size_t)F32Query::kPlanes * D + sizeof(F32Query::Sum) : (size_t)U8Query::kPlanes * D + sizeof(U8Query::Sum);
  return (size_t)16 * qf * (query + (k ? (size_t)(k + kCandPerIter) * 8 + 8 : 0));
}

// contiguous ascending database splits of whole 64-row steps, none empty; splits <= 0: cover the chip a few times over
void plan_splits(int n, int splits, Plan *p) {
  if (splits <= 0) {
    splits = (1024 + p->qtiles - 1) / p->qtiles;
    const int most = (n + 255) / 256;
    splits = splits < most ? splits : most;
  }
  const int tiles = (n + kCandPerIter - 1) / kCandPerIter;
  splits = splits < tiles ? splits : tiles;
  splits = splits < kMaxSplits ? splits : kMaxSplits;
  const int per = (n + splits - 1) / splits;
  p->rows_per_split = (per + kCandPerIter - 1) / kCandPerIter * kCandPerIter;
  p->splits = (n + p->rows_per_split - 1) / p->rows_per_split;
}

// k == 0: the plan of a threshold search (no candidate buffers, no workspace); the top-k entry points refuse it before they ask
int make_plan(int nq, int n, int D, int k, int splits, bool f32q, Plan *p) {
  SGIC_REQUIRE(nq > 0 && n > 0 && k >= 0 && k <= n, "sizes");
  SGIC_REQUIRE(k <= kMaxK, "the fused search keeps at most 128 results per query");
  SGIC_REQUIRE(D > 0 && D % 64 == 0 && D <= 4096, "D must be a multiple of 64, at most 4096 (int32 exactness)");
  SGIC_REQUIRE(!f32q || D <= kMaxDimF32Q, "fp32 queries: D at most 2048 (three query digit planes have to fit the LDS)");
  SGIC_REQUIRE(splits <= kMaxSplits, "splits");
  const int wide = f32q ? F32Query::kWideQF : U8Query::kWideQF;   // three planes: the wide tile is 32 queries, not 64
  p->qf = (nq > 16 && lds_bytes(f32q, wide, D, k) <= (size_t)kLdsBigTile) ? wide : 1;
  p->qtiles = (nq + 16 * p->qf - 1) / (16 * p->qf);
  plan_splits(n, splits, p);
  p->lds = lds_bytes(f32q, p->qf, D, k);
  p->work_bytes = p->splits > 1 ? (size_t)nq * p->splits * k * 8 : 0;
  return SGIC_OK;
}

template <auto Kernel, class... Args>
int launch(const Plan &p, const char *name, hipStream_t st, Args... args) {
  static bool lds_raised = false;   // beyond the default 64 KiB a kernel has to be allowed its dynamic LDS once (largest use: 120.25 KiB)
  if (p.lds > 60 * 1024 && !lds_raised) {
    SGIC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    lds_raised = true;
  }
  Kernel<<<dim3(p.qtiles, p.splits), 256, p.lds, st>>>(args...);
  return sgic::check_launch(name);
}

// f(QF, U) for the plan's tile (Query's wide tile or 16 queries) and eight 64-byte steps per round when D allows it, else one
template <class Query, class F>
int dispatch(const Plan &p, int D, F f) {
  constexpr std::integral_constant<int, Query::kWideQF> wide{};
  constexpr std::integral_constant<int, 1> one{};
  constexpr std::integral_constant<int, 8> eight{};
  const bool u8 = D % 512 == 0;
  return p.qf == wide ? (u8 ? f(wide, eight) : f(wide, one)) : (u8 ? f(one, eight) : f(one, one));
}

template <class Query>
int search_range(const Plan &p, const typename Query::T *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n,
                 int D, float threshold, int self_join, long long capacity, uint64_t *d_count, int32_t *d_out_q, int32_t *d_out_d,
                 float *d_out_score, sgic_stream_t stream) {
  return dispatch<Query>(p, D, [&](auto qf, auto u) {
    return launch<search_range_kernel<Query, qf, u>>(p, "search_range_kernel", to_stream(stream), d_q, d_rq, d_db, d_rdb, nq, n, D,
                                                    p.rows_per_split, threshold, self_join, (unsigned long long)capacity,
                                                    reinterpret_cast<unsigned long long *>(d_count), d_out_q, d_out_d, d_out_score);
  });
}

int topk_work_bytes(int nq, int n, int D, int k, int splits, bool f32q, int *splits_used, size_t *bytes) {
  SGIC_REQUIRE(k > 0, "sizes");
  Plan p;
  const int rc = make_plan(nq, n, D, k, splits, f32q, &p);
  if (rc != SGIC_OK) return rc;
  if (splits_used) *splits_used = p.splits;
  if (bytes) *bytes = p.work_bytes;
  return SGIC_OK;
}

// the search into the outputs, or with several splits into the workspace and the merge from there; d_rq: nullptr for fp32 queries
template <class Query>
int search_topk(const Plan &p, const typename Query::T *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n,
                int D, int k, uint8_t *d_work, float *d_out_scores, int32_t *d_out_idx, sgic_stream_t stream) {
  hipStream_t st = to_stream(stream);
  float *okey = d_out_scores;
  int *oidx = d_out_idx;
  if (p.splits > 1) {
    okey = reinterpret_cast<float *>(d_work);
    oidx = reinterpret_cast<int *>(d_work + (size_t)nq * p.splits * k * 4);
  }
  const int lrc = dispatch<Query>(p, D, [&](auto qf, auto u) {
    return launch<search_topk_kernel<Query, qf, u>>(p, "search_topk_kernel", st, d_q, d_rq, d_db, d_rdb, nq, n, D, k, p.rows_per_split,
                                                   p.splits, (int)(p.splits == 1), okey, oidx);
  });
  if (lrc != SGIC_OK) return lrc;
  if (p.splits > 1) {
    search_merge_kernel<<<nq, 256, 0, st>>>(okey, oidx, d_rq, 1.0f / kQScale, p.splits, k, d_out_scores, d_out_idx);
    return sgic::check_launch("search_merge_kernel");
  }
  return SGIC_OK;
}

// the pre-pass (target keys into the workspace, scores, zeroed ranks), then the scan
template <class Query>
int search_rank(int nq, int n, int D, int splits, bool f32q, const typename Query::T *d_q, const float *d_rq, const uint8_t *d_db,
                const float *d_rdb, const int32_t *d_target, uint8_t *d_work, size_t work_bytes, int32_t *d_rank, float *d_score,
                sgic_stream_t stream) {
  Plan p;
  const int rc = make_plan(nq, n, D, 0, splits, f32q, &p);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(d_q && (f32q || d_rq) && d_db && d_rdb && d_target && d_work && d_rank && d_score, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_q | (uintptr_t)d_db) % 16 == 0 && (uintptr_t)d_work % 4 == 0, "queries and codes must be 16-byte aligned");
  SGIC_REQUIRE(work_bytes >= (size_t)nq * 4, "workspace (sgic_search_rank_work_bytes)");
  p.lds += (size_t)16 * p.qf * sizeof(int);   // the per-query counters
  hipStream_t st = to_stream(stream);
  float *tkey = reinterpret_cast<float *>(d_work);
  search_rank_target_kernel<Query><<<cdiv((size_t)nq, 4), 256, 0, st>>>(d_q, d_rq, d_db, d_rdb, d_target, nq, n, D, tkey, d_rank, d_score);
  const int prc = sgic::check_launch("search_rank_target_kernel");
  if (prc != SGIC_OK) return prc;
  return dispatch<Query>(p, D, [&](auto qf, auto u) {
    return launch<search_rank_kernel<Query, qf, u>>(p, "search_rank_kernel", st, d_q, d_db, d_rdb, d_target, tkey, nq, n, D,
                                                   p.rows_per_split, d_rank);
  });
}

}  // namespace

extern "C" int sgic_search_rank_work_bytes(int nq, size_t *bytes) {
  SGIC_REQUIRE(nq > 0 && bytes, "sizes");
  *bytes = (size_t)nq * 4;   // one target key per query
  return SGIC_OK;
}

extern "C" int sgic_search_rank_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb,
                                   const int32_t *d_target, int nq, int n, int D, int splits, uint8_t *d_work, size_t work_bytes,
                                   int32_t *d_rank, float *d_score, sgic_stream_t stream) {
  return search_rank<U8Query>(nq, n, D, splits, false, d_q, d_rq, d_db, d_rdb, d_target, d_work, work_bytes, d_rank, d_score, stream);
}

extern "C" int sgic_search_rank_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, const int32_t *d_target, int nq, int n,
                                     int D, int splits, uint8_t *d_work, size_t work_bytes, int32_t *d_rank, float *d_score,
                                     sgic_stream_t stream) {
  return search_rank<F32Query>(nq, n, D, splits, true, d_q, nullptr, d_db, d_rdb, d_target, d_work, work_bytes, d_rank, d_score, stream);
}

extern "C" int sgic_search_range_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D, float threshold,
                                      int splits, long long capacity, uint64_t *d_count, int32_t *d_out_q, int32_t *d_out_d,
                                      float *d_out_score, sgic_stream_t stream) {
  Plan p;
  const int rc = make_plan(nq, n, D, 0, splits, true, &p);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(d_q && d_db && d_rdb && d_count, "null pointer");
  SGIC_REQUIRE(capacity >= 0 && (capacity == 0 || (d_out_q && d_out_d && d_out_score)), "capacity > 0 needs the three output arrays");
  SGIC_REQUIRE(((uintptr_t)d_q | (uintptr_t)d_db) % 16 == 0, "queries and codes must be 16-byte aligned");
  SGIC_REQUIRE((uintptr_t)d_count % 8 == 0, "the hit counter must be 8-byte aligned");
  SGIC_REQUIRE(isfinite(threshold), "the threshold must be finite");
  return search_range<F32Query>(p, d_q, nullptr, d_db, d_rdb, nq, n, D, threshold, 0, capacity, d_count, d_out_q, d_out_d, d_out_score,
                                stream);
}

extern "C" int sgic_search_range_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n,
                                    int D, float threshold, int self_join, int splits, long long capacity, uint64_t *d_count,
                                    int32_t *d_out_q, int32_t *d_out_d, float *d_out_score, sgic_stream_t stream) {
  Plan p;
  const int rc = make_plan(nq, n, D, 0, splits, false, &p);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(d_q && d_rq && d_db && d_rdb && d_count, "null pointer");
  SGIC_REQUIRE(capacity >= 0 && (capacity == 0 || (d_out_q && d_out_d && d_out_score)), "capacity > 0 needs the three output arrays");
  SGIC_REQUIRE(((uintptr_t)d_q | (uintptr_t)d_db) % 16 == 0, "codes must be 16-byte aligned");
  SGIC_REQUIRE((uintptr_t)d_count % 8 == 0, "the hit counter must be 8-byte aligned");
  SGIC_REQUIRE(isfinite(threshold), "the threshold must be finite");
  SGIC_REQUIRE(!self_join || nq == n, "self_join: the queries are the database (nq == n)");
  return search_range<U8Query>(p, d_q, d_rq, d_db, d_rdb, nq, n, D, threshold, self_join ? 1 : 0, capacity, d_count, d_out_q, d_out_d,
                               d_out_score, stream);
}

extern "C" int sgic_search_codes_u8_work_bytes(int nq, int n, int D, int k, int splits, int *splits_used, size_t *bytes) {
  return topk_work_bytes(nq, n, D, k, splits, false, splits_used, bytes);
}

extern "C" int sgic_search_codes_u8(const uint8_t *d_q, const float *d_rq, const uint8_t *d_db, const float *d_rdb, int nq, int n,
                                    int D, int k, int splits, uint8_t *d_work, size_t work_bytes, float *d_out_scores,
                                    int32_t *d_out_idx, sgic_stream_t stream) {
  SGIC_REQUIRE(k > 0, "sizes");
  Plan p;
  const int rc = make_plan(nq, n, D, k, splits, false, &p);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(d_q && d_rq && d_db && d_rdb && d_out_scores && d_out_idx, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_q | (uintptr_t)d_db | (uintptr_t)d_work) % 16 == 0, "codes and workspace must be 16-byte aligned");
  SGIC_REQUIRE(p.work_bytes == 0 || (d_work && work_bytes >= p.work_bytes), "workspace (sgic_search_codes_u8_work_bytes)");
  return search_topk<U8Query>(p, d_q, d_rq, d_db, d_rdb, nq, n, D, k, d_work, d_out_scores, d_out_idx, stream);
}

extern "C" int sgic_search_codes_f32q_work_bytes(int nq, int n, int D, int k, int splits, int *splits_used, size_t *bytes) {
  return topk_work_bytes(nq, n, D, k, splits, true, splits_used, bytes);
}

extern "C" int sgic_search_codes_f32q(const float *d_q, const uint8_t *d_db, const float *d_rdb, int nq, int n, int D, int k, int splits,
                                      uint8_t *d_work, size_t work_bytes, float *d_out_scores, int32_t *d_out_idx,
                                      sgic_stream_t stream) {
  SGIC_REQUIRE(k > 0, "sizes");
  Plan p;
  const int rc = make_plan(nq, n, D, k, splits, true, &p);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(d_q && d_db && d_rdb && d_out_scores && d_out_idx, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_q | (uintptr_t)d_db | (uintptr_t)d_work) % 16 == 0, "queries, codes and workspace must be 16-byte aligned");
  SGIC_REQUIRE(p.work_bytes == 0 || (d_work && work_bytes >= p.work_bytes), "workspace (sgic_search_codes_f32q_work_bytes)");
  return search_topk<F32Query>(p, d_q, nullptr, d_db, d_rdb, nq, n, D, k, d_work, d_out_scores, d_out_idx, stream);
}

// Clustering over the same codes (CodeIndex.assign / kmeans): for every database row the best of K fp32 centroids, and the exact
// integer sums of a partition.
//
// sgic_assign_codes_f32c.  M(c, d) is F32Query's integer: the centroid goes through quantise16 into three balanced
// base-256 digit planes, S_p = sum d_p (c_d - 128) comes from the i8 MFMA, M = 2 (65536 S_2 + 256 S_1 + S_0) + sum Q in int64.
// r_d > 0 is common to all centroids of a row, so the argmax runs on M itself: larger M, equal M -> lower centroid index.  No float
// compare, add, root or division; the caller derives the score (float32(M) * r_d) * 2^-22.
//   assign_prepare_kernel   one workgroup per tile of 16 centroids: the three planes in MFMA fragment order ([tile][plane][step][lane]
//                           16-byte fragments, lane l: centroid l & 15, coordinates 64 step + 16 (l >> 4) ..+15) and sum Q (int64) per
//                           centroid, into the workspace.  Slots >= K repeat centroid K - 1 and are masked by index below.
//   assign_codes_kernel     a workgroup of four waves owns 256 database rows, a wave four 16-row tiles.  REG (D = 512): a wave keeps
//                           its tiles' 32 fragments in registers for the whole kernel, so the codes are read from HBM once however
//                           large K is; otherwise the fragments are re-read (L2) per centroid tile.  Centroid tiles are staged in
//                           LDS `ct` at a time by straight 16-byte copies; one LDS fragment read feeds four MFMAs.  In C, rows are
//                           centroids (4 (l >> 4) + reg), columns database rows (l & 15): a lane sees its centroids in ascending
//                           order and keeps the best with a strict >; two cross-lane steps (xor 16, 32) with the full comparator
//                           finish a row.  Rows >= n are clamped for the loads and masked for the stores.  No atomics.
//
// sgic_cluster_sums_u8.  The caller sorts the rows by cluster (stable) and passes the order and the sorted cluster ids.  A workgroup
// takes 1024 consecutive sorted positions and walks them run by run (a run: one cluster's members inside the slice; its end is found
// by bisection of the sorted ids).  Thread (m, chunk) gathers the 16-byte chunk `chunk` of members m, m + ML, ... and adds the bytes
// in int32 registers (255 * 1024 < 2^31); the member lanes are summed through LDS and each coordinate takes one 64-bit atomicAdd of
// 2 sum c - 255 members.  Integer adds commute, so the result does not depend on the schedule.
namespace {

constexpr int kAssignR = 4;                      // 16-row database tiles per wave
constexpr int kAssignRows = 4 * 16 * kAssignR;   // database rows per workgroup
constexpr int kAssignMaxK = 65536;
constexpr int kAssignMaxCt = 8;                  // centroid tiles staged per round, at most
constexpr int kAssignStage = 6;                  // 16-byte fragments a thread has in flight while staging (one D = 512 tile: 6 per thread)
constexpr int kSumsSlice = 1024;                 // sorted positions per workgroup
constexpr int kSumsMaxDim = 4096;                // 256 threads x 16 bytes

__global__ __launch_bounds__(256) void assign_prepare_kernel(const float *__restrict__ cent, int K, int D, v4i *__restrict__ planes,
                                                             long long *__restrict__ sumq) {
  __shared__ unsigned long long sq[16];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int frags = (D >> 6) * 64;   // fragments per plane of one tile
  if (tid < 16) sq[tid] = 0;
  __syncthreads();
  v4i *dst = planes + (size_t)tile * 3 * frags;
  for (int i = tid; i < frags; i += 256) {   // sixteen coordinates -> one fragment in each plane per (step, lane)
    const int ln = i & 63, step = i >> 6;
    int ci = tile * 16 + (ln & 15);
    ci = ci < K ? ci : K - 1;
    stage_f32_fragment(cent + (size_t)ci * D + 64 * step + 16 * (ln >> 4), dst + i, frags, &sq[ln & 15]);
  }
  __syncthreads();
  if (tid < 16) sumq[tile * 16 + tid] = (long long)sq[tid];
}

template <bool REG>
__global__ __launch_bounds__(256, 2) void assign_codes_kernel(const v4i *__restrict__ planes, const long long *__restrict__ sumq,
                                                              const uint8_t *__restrict__ db, int K, int n, int D, int ct,
                                                              int *__restrict__ out_c, long long *__restrict__ out_M) {
  constexpr int R = kAssignR;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int steps = REG ? 8 : D >> 6;
  const int tiles = (K + 15) >> 4;
  const int tfrag = 3 * steps * 64;          // fragments per centroid tile
  v4i *A = reinterpret_cast<v4i *>(smem);   // [ct][3 planes][steps][64 lanes] fragments
  long long *sq = reinterpret_cast<long long *>(smem + (size_t)ct * tfrag * 16);   // [ct][16] sum Q

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * kAssignRows + wave * (16 * R) + (lane & 15);   // this lane's row of tile r: row0 + 16 r
  const uint4 *bp[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const long long row = row0 + 16 * r;
    bp[r] = reinterpret_cast<const uint4 *>(db + (size_t)(row < n ? row : n - 1) * D) + (lane >> 4);
  }
  v4i b[R][REG ? 8 : 1];
  if (REG) {
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int s = 0; s < 8; s++) b[r][s] = to_i8x16(bp[r][s * 4]);
  }
  long long best[R];
  int bidx[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    best[r] = (long long)0x8000000000000000ull;   // below every M; a lane without a live centroid keeps it and loses the reduction
    bidx[r] = 0x7fffffff;
  }

  for (int t0 = 0; t0 < tiles; t0 += ct) {
    const int nt = tiles - t0 < ct ? tiles - t0 : ct;
    __syncthreads();   // the previous round's fragments have been read
    const v4i *src = planes + (size_t)t0 * tfrag;
    for (int i0 = tid; i0 < nt * tfrag; i0 += 256 * kAssignStage) {   // kAssignStage loads in flight, then their LDS writes
      v4i f[kAssignStage];
#pragma unroll
      for (int u = 0; u < kAssignStage; u++) {
        const int i = i0 + 256 * u;
        f[u] = src[i < nt * tfrag ? i : i0];
      }
#pragma unroll
      for (int u = 0; u < kAssignStage; u++) {
        const int i = i0 + 256 * u;
        if (i < nt * tfrag) A[i] = f[u];
      }
    }
    if (tid < nt * 16) sq[tid] = sumq[t0 * 16 + tid];
    __syncthreads();
    for (int c = 0; c < nt; c++) {
      v4i acc[R][3];
#pragma unroll
      for (int r = 0; r < R; r++)
#pragma unroll
        for (int p = 0; p < 3; p++) acc[r][p] = v4i{0, 0, 0, 0};
      const v4i *Ac = A + c * tfrag + lane;
      if (REG) {
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
          for (int p = 0; p < 3; p++) {
            const v4i a = Ac[(p * 8 + s) * 64];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[r][s], acc[r][p], 0, 0, 0);
          }
      } else {
        for (int s = 0; s < steps; s++) {
#pragma unroll
          for (int r = 0; r < R; r++) b[r][0] = to_i8x16(bp[r][s * 4]);
#pragma unroll
          for (int p = 0; p < 3; p++) {
            const v4i a = Ac[(p * steps + s) * 64];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[r][0], acc[r][p], 0, 0, 0);
          }
        }
      }
      const int c0 = (t0 + c) * 16 + 4 * (lane >> 4);   // this lane's centroids of the tile: c0 + j, ascending
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const long long sj = sq[c * 16 + 4 * (lane >> 4) + j];
        if (c0 + j < K) {   // pad slots never win: masked by index, not by value
#pragma unroll
          for (int r = 0; r < R; r++) {
            const long long M = 2 * (65536LL * acc[r][2][j] + 256LL * acc[r][1][j] + acc[r][0][j]) + sj;
            if (M > best[r]) {
              best[r] = M;
              bidx[r] = c0 + j;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {   // the four lane groups of a column: larger M, else lower index
      const long long om = __shfl_xor(best[r], m);
      const int oi = __shfl_xor(bidx[r], m);
      if (om > best[r] || (om == best[r] && oi < bidx[r])) {
        best[r] = om;
        bidx[r] = oi;
      }
    }
    const long long row = row0 + 16 * r;
    if (lane < 16 && row < n) {
      out_c[row] = bidx[r];
      out_M[row] = best[r];
    }
  }
}

__global__ __launch_bounds__(256) void cluster_sums_kernel(const uint8_t *__restrict__ codes, const long long *__restrict__ order,
                                                           const int *__restrict__ sorted_assign, int n, int D, int K,
                                                           unsigned long long *__restrict__ sums, unsigned long long *__restrict__ counts) {
  __shared__ __attribute__((aligned(16))) int red[256 * 16];   // [member lane][D]
  const int tid = threadIdx.x;
  const int chunks = D >> 4;          // 16-byte chunks per row, at most 256
  const int ML = 256 / chunks;        // member lanes
  const int m = tid / chunks, ch = tid - m * chunks;
  long long p = (long long)blockIdx.x * kSumsSlice;
  const long long end = p + kSumsSlice < n ? p + kSumsSlice : n;
  while (p < end) {   // p, c, q are the same in every thread: the barriers below are taken by all
    const int c = sorted_assign[p];
    long long lo = p + 1, hi = end;   // the run's end: the first position after p whose id is not c
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (sorted_assign[mid] == c) lo = mid + 1; else hi = mid;
    }
    const long long q = lo;
    if (c >= 0 && c < K) {   // the caller has checked the ids; an id outside [0, K) is skipped, never written
      const int mlim = q - p < ML ? (int)(q - p) : ML;
      if (m < mlim) {
        unsigned acc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0;
        int members = 0;
        for (long long i = p + m; i < q; i += ML) {
          const long long row = order[i];
          if ((unsigned long long)row >= (unsigned long long)n) continue;
          const uint4 v = *reinterpret_cast<const uint4 *>(codes + (size_t)row * D + 16 * ch);
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 16; j++) acc[j] += (w[j >> 2] >> (8 * (j & 3))) & 255u;
          members++;
        }
        int4 *dst = reinterpret_cast<int4 *>(red + (size_t)m * D + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; j++)
          dst[j] = int4{2 * (int)acc[4 * j] - 255 * members, 2 * (int)acc[4 * j + 1] - 255 * members,
                        2 * (int)acc[4 * j + 2] - 255 * members, 2 * (int)acc[4 * j + 3] - 255 * members};
      }
      __syncthreads();
      for (int t = tid; t < D; t += 256) {
        int s = 0;
        for (int mm = 0; mm < mlim; mm++) s += red[mm * D + t];
        atomicAdd(&sums[(size_t)c * D + t], (unsigned long long)(long long)s);
      }
      if (tid == 0) atomicAdd(&counts[c], (unsigned long long)(q - p));
      __syncthreads();
    }
    p = q;
  }
}

int assign_work_bytes(int K, int D, size_t *bytes) {
  SGIC_REQUIRE(K >= 1 && K <= kAssignMaxK, "1 <= K <= 65536");
  SGIC_REQUIRE(D > 0 && D % 64 == 0 && D <= kMaxDimF32Q, "D must be a multiple of 64, at most 2048");
  const size_t kpad = ((size_t)K + 15) / 16 * 16;
  *bytes = kpad * ((size_t)3 * D + 8);   // three planes, then sum Q
  return SGIC_OK;
}

template <bool REG>
int launch_assign(size_t lds, unsigned blocks, const v4i *planes, const long long *sumq, const uint8_t *db, int K, int n, int D, int ct,
                  int *out_c, long long *out_M, hipStream_t st) {
  static bool lds_raised = false;   // largest use: one tile at D = 2048 -> 96.1 KiB
  if (lds > 60 * 1024 && !lds_raised) {
    SGIC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(assign_codes_kernel<REG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 128 * 1024));
    lds_raised = true;
  }
  assign_codes_kernel<REG><<<blocks, 256, lds, st>>>(planes, sumq, db, K, n, D, ct, out_c, out_M);
  return sgic::check_launch("assign_codes_kernel");
}

}  // namespace

extern "C" int sgic_assign_codes_f32c_work_bytes(int K, int D, size_t *bytes) {
  SGIC_REQUIRE(bytes, "null pointer");
  return assign_work_bytes(K, D, bytes);
}

extern "C" int sgic_assign_codes_f32c(const float *d_cent, const uint8_t *d_db, int K, int n, int D, uint8_t *d_work, size_t work_bytes,
                                      int32_t *d_out_c, int64_t *d_out_M, sgic_stream_t stream) {
  size_t need = 0;
  const int rc = assign_work_bytes(K, D, &need);
  if (rc != SGIC_OK) return rc;
  SGIC_REQUIRE(n >= 1, "sizes");
  SGIC_REQUIRE(d_cent && d_db && d_work && d_out_c && d_out_M, "null pointer");
  SGIC_REQUIRE(((uintptr_t)d_cent | (uintptr_t)d_db | (uintptr_t)d_work) % 16 == 0, "centroids, codes and workspace must be 16-byte aligned");
  SGIC_REQUIRE((uintptr_t)d_out_M % 8 == 0 && (uintptr_t)d_out_c % 4 == 0, "outputs must be aligned to their element size");
  SGIC_REQUIRE(work_bytes >= need, "workspace (sgic_assign_codes_f32c_work_bytes)");
  hipStream_t st = to_stream(stream);
  const int tiles = (K + 15) / 16;
  v4i *planes = reinterpret_cast<v4i *>(d_work);
  long long *sumq = reinterpret_cast<long long *>(d_work + (size_t)tiles * 16 * 3 * D);
  assign_prepare_kernel<<<tiles, 256, 0, st>>>(d_cent, K, D, planes, sumq);
  const int prc = sgic::check_launch("assign_prepare_kernel");
  if (prc != SGIC_OK) return prc;
  const size_t tile_bytes = (size_t)48 * D + 128;   // three planes of 16 centroids and their sum Q
  int ct = (int)((size_t)48 * 1024 / ((size_t)48 * D));   // about 48 KiB of planes per round
  ct = ct < 1 ? 1 : (ct > kAssignMaxCt ? kAssignMaxCt : ct);
  ct = ct < tiles ? ct : tiles;
  const size_t lds = ct * tile_bytes;
  const unsigned blocks = cdiv((size_t)n, kAssignRows);
  long long *oM = reinterpret_cast<long long *>(d_out_M);
  return D == 512 ? launch_assign<true>(lds, blocks, planes, sumq, d_db, K, n, D, ct, d_out_c, oM, st)
                  : launch_assign<false>(lds, blocks, planes, sumq, d_db, K, n, D, ct, d_out_c, oM, st);
}

extern "C" int sgic_cluster_sums_u8(const uint8_t *d_db, const int64_t *d_order, const int32_t *d_sorted_assign, int n, int D, int K,
                                    int64_t *d_sums, int64_t *d_counts, sgic_stream_t stream) {
  SGIC_REQUIRE(n >= 1 && K >= 1, "sizes");
  SGIC_REQUIRE(D > 0 && D % 16 == 0 && D <= kSumsMaxDim, "D must be a multiple of 16, at most 4096");
  SGIC_REQUIRE(d_db && d_order && d_sorted_assign && d_sums && d_counts, "null pointer");
  SGIC_REQUIRE((uintptr_t)d_db % 16 == 0, "codes must be 16-byte aligned");
  SGIC_REQUIRE(((uintptr_t)d_order | (uintptr_t)d_sums | (uintptr_t)d_counts) % 8 == 0 && (uintptr_t)d_sorted_assign % 4 == 0,
               "arrays must be aligned to their element size");
  cluster_sums_kernel<<<cdiv((size_t)n, kSumsSlice), 256, 0, to_stream(stream)>>>(
      d_db, reinterpret_cast<const long long *>(d_order), d_sorted_assign, n, D, K, reinterpret_cast<unsigned long long *>(d_sums),
      reinterpret_cast<unsigned long long *>(d_counts));
  return sgic::check_launch("cluster_sums_kernel");
}
