// softmax.hip -- the score of Bayesian softmax (multiclass logistic) regression
// (include/dsvgd.h, dsvgd_score_softmax): data rows xd_q in R^p with labels
// y_q in {0..C-1}, a particle x = [log alpha | vec(W)] with W (C x p, row-major),
//
//   z_qc = w_c . xd_q,  pi_qc = softmax_c(z_q.),  G_qc = 1[y_q = c] - pi_qc,
//   S[i, 1 + c p + k] = scale (wt sum_q G_qc xd_qk - alpha W_ck)
//   S[i, 0]           = scale (C p / 2 - alpha |W|^2 / 2 + a0 - b0 alpha)
//
// over the cyclic window of B rows that starts at *cursor % N, wt = N / B (the
// full-data score: the window of all N rows from row 0, wt = 1).  The rows
// are read where they lie, in exact f32; no input is split or scaled.
//
// Tile form (n > kSmxSmallRows): a workgroup of 4 waves scores 32 particles,
// the particle index the MFMA column as in logreg_window_kernel, and the four
// waves share the window's chunks of 32 rows between them (wave w takes chunks
// w, w + 4, ...; their partial sums meet in a fixed order at the end: the
// serial chain per wave is a quarter of the window, which is what lets a few
// thousand particles fill the machine).  Per chunk, staged through the wave's
// own LDS buffer with the next chunk's loads in flight under this chunk's
// MFMAs, a wave makes two passes over the classes:
//   A  Z_c^T = Xd W_c^T (v_mfma_f32_32x32x2_f32) for every class c, folded
//      into a running maximum and a running sum of exp(z - max) per (data
//      row, particle): all in one lane, no cross-lane traffic;
//   B  Z_c^T again for the classes of the own slab, G_c = 1[y = c] -
//      exp(z - max) / sum in registers, which IS the A operand of G_c Xd's
//      K-step j when the B operand takes row c_row(j, l) of the chunk
//      (logreg_window.hip's comment), accumulated into the slab's tiles.
// A tile is (class c, 32 columns of p); a slab (blockIdx.y) owns kSmxTiles
// consecutive tiles.  The two-pass softmax costs the logits of the slab's
// classes twice and needs 64 registers for them instead of 16 C.
// The weights are the B operand of Z^T: a lane reads its own particle's,
// four consecutive floats per 8 columns (the K order logreg_window.hip
// shares between A and B), from memory as they are needed.  p > kSmxPiece:
// the chunk's columns go through the buffer a piece at a time.
//
// Row form (n <= kSmxSmallRows, the sequential order's one-particle refresh):
// a workgroup per particle on the VALU, 64 rows of G at a time (a wave per
// row), then a thread per output column.
//
// Pads (rows past the window, columns past p, particles past n) are selected
// zeros, never products of data that was read.  Every sum runs in a fixed
// order, without atomics: the same bits on every call.
#include "common.hpp"

namespace dsvgd {

constexpr int kSmxMaxC = DSVGD_SOFTMAX_MAX_CLASSES;
constexpr int kSmxMaxD = 1024;
constexpr int kSmxRows = 32;          // particles per workgroup (the four waves share them)
constexpr int kSmxChunk = 32;         // window rows per chunk
constexpr int kSmxTiles = 16;         // 32 x 32 output tiles per slab
constexpr int kSmxPiece = 64;         // columns of a chunk staged at a time
constexpr int kSmxPitch = kSmxPiece + 8;   // rows 4 apart 32 banks apart
constexpr int kSmxBuf = kSmxChunk * kSmxPitch;    // floats per wave
constexpr int64_t kSmxSmallRows = 16;
constexpr int kSmxSmallChunk = 64;
constexpr int kSmxRed = 3 * 4 * 1024;   // the reduction: 4 tiles of 3 waves at a time
constexpr int kSmxLds = 4 * kSmxBuf > kSmxRed ? 4 * kSmxBuf : kSmxRed;

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int64_t smx_origin(const int64_t* cursor, int64_t N) {
  if (!cursor) return 0;
  int64_t org = *cursor % N;
  return org < 0 ? org + N : org;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void softmax_tile_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t n, int C, int p, const float* __restrict__ Xd,
    int64_t ldxd, const int32_t* __restrict__ y, int64_t N, const int64_t* __restrict__ cursor,
    int B, float wt, float a0, float b0, float scale, float* __restrict__ S, int64_t lds) {
  __shared__ __attribute__((aligned(16))) float buf[kSmxLds];
  __shared__ int sy[4][kSmxChunk];
  __shared__ float sa[kSmxRows];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * kSmxRows;
  const int64_t i = i0 + r;               // this lane's particle
  const bool live = i < n;
  const float* x = X + (live ? i : 0) * ldx;
  const int nkb = (p + 31) >> 5;          // tiles per class
  const int ntile = C * nkb;
  const int T0 = (int)blockIdx.y * kSmxTiles;
  const int nt = min(kSmxTiles, ntile - T0);
  const int npiece = (p + kSmxPiece - 1) / kSmxPiece;
  const int64_t org = smx_origin(cursor, N);
  const int nchunks = (B + kSmxChunk - 1) / kSmxChunk;
  const int rounds = (nchunks + 3) >> 2;
  float* mybuf = buf + w * kSmxBuf;

  // the label of row `lane` of chunk c, -1 past the window
  auto label = [&](int c) {
    const int q = c * kSmxChunk + r;
    int64_t row = org + q;
    if (row >= N) row -= N;
    const bool in = q < B;
    const int v = y[in ? row : org];
    return in ? v : -1;
  };
  // chunk c, piece pc: row j, column 64 pc + lane of the chunk (the loads from
  // addresses clamped into the window and the row; the masks are applied when
  // the values go to LDS: a pad is a selected zero)
  float stg[kSmxChunk];
  auto fetch = [&](int c, int pc) {
    const int cc = min(pc * kSmxPiece + lane, p - 1);
#pragma unroll
    for (int j = 0; j < kSmxChunk; ++j) {
      const int q = c * kSmxChunk + j;
      int64_t row = org + q;
      if (row >= N) row -= N;
      if (q >= B) row = org;
      stg[j] = Xd[row * ldxd + cc];
    }
  };
  auto put = [&](int c, int pc) {
    const bool cin = pc * kSmxPiece + lane < p;
#pragma unroll
    for (int j = 0; j < kSmxChunk; ++j)
      mybuf[j * kSmxPitch + lane] = (cin && c * kSmxChunk + j < B) ? stg[j] : 0.f;
  };
  int chunk = w;         // this wave's chunk of the round
  int staged = 0;        // the piece in the buffers (npiece > 1)
  auto ensure = [&](int pc) {
    if (npiece > 1 && staged != pc) {     // uniform over the workgroup
      __syncthreads();
      fetch(chunk, pc);
      put(chunk, pc);
      __syncthreads();
      staged = pc;
    }
  };
  // the weights of class c, columns 8 u + 4 h + e, zero past p and past n
  auto ldw = [&](int c, int u) {
    const int col = 8 * u + 4 * h;
    const float* wp = x + 1 + (int64_t)c * p;
    f32x4 v;
    if (col + 4 <= p) {
      v = *reinterpret_cast<const f32x4u*>(wp + col);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = wp[min(col + e, p - 1)];
        v[e] = col + e < p ? f : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = live ? v[e] : 0.f;
    return v;
  };
  // z0 + z1 = Z_c^T of the wave's chunk, two chains
  auto zmm = [&](int c, f32x16& z0, f32x16& z1) {
#pragma unroll
    for (int q = 0; q < 16; ++q) z0[q] = z1[q] = 0.f;
    for (int pc = 0; pc < npiece; ++pc) {
      ensure(pc);
      const int nu = (min(kSmxPiece, p - pc * kSmxPiece) + 7) >> 3;
      const int u0 = pc * (kSmxPiece / 8);
      // the piece's weights in flight together, then its MFMAs
      f32x4 wv[kSmxPiece / 8];
#pragma unroll
      for (int u = 0; u < kSmxPiece / 8; ++u)
        if (u < nu) wv[u] = ldw(c, u0 + u);
#pragma unroll
      for (int u = 0; u < kSmxPiece / 8; ++u) {
        if (u < nu) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(mybuf + r * kSmxPitch + 8 * u + 4 * h);
          z0 = mfma32(a[0], wv[u][0], z0);
          z1 = mfma32(a[1], wv[u][1], z1);
          z0 = mfma32(a[2], wv[u][2], z0);
          z1 = mfma32(a[3], wv[u][3], z1);
        }
      }
    }
  };

  f32x16 acc[kSmxTiles];
#pragma unroll
  for (int tt = 0; tt < kSmxTiles; ++tt)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[tt][q] = 0.f;

  if (w == 0 && h == 0) sa[r] = live ? expf(x[0]) : 0.f;
  int ynext = label(chunk);
  if (npiece == 1) {
    fetch(chunk, 0);
    put(chunk, 0);
  }
  const int cfirst = T0 / nkb, clast = (T0 + nt - 1) / nkb;
  for (int k = 0; k < rounds; ++k) {
    chunk = 4 * k + w;
    if (h == 0) sy[w][r] = ynext;
    __syncthreads();
    const bool more = k + 1 < rounds;
    if (more) {
      ynext = label(chunk + 4);
      if (npiece == 1) fetch(chunk + 4, 0);
    }
    staged = npiece == 1 ? 0 : -1;
    // pass A: the running maximum and sum of every (row, particle)
    f32x16 m, s;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      m[j] = -INFINITY;
      s[j] = 0.f;
    }
    for (int c = 0; c < C; ++c) {
      f32x16 z0, z1;
      zmm(c, z0, z1);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float z = z0[j] + z1[j];
        const float mn = fmaxf(m[j], z);
        s[j] = fmaf(s[j], __builtin_amdgcn_exp2f((m[j] - mn) * kLog2e),
                    __builtin_amdgcn_exp2f((z - mn) * kLog2e));
        m[j] = mn;
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = __builtin_amdgcn_rcpf(s[j]);
    // pass B: G_c of the slab's classes, and G_c Xd into the slab's tiles
    for (int c = cfirst; c <= clast; ++c) {
      f32x16 z0, z1;
      zmm(c, z0, z1);
      float g[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float pi = __builtin_amdgcn_exp2f(((z0[j] + z1[j]) - m[j]) * kLog2e) * s[j];
        const int yl = sy[w][c_row(j, lane)];
        g[j] = yl < 0 ? 0.f : (yl == c ? 1.f : 0.f) - pi;
      }
      const int tlo = max(c * nkb, T0) - T0, thi = min((c + 1) * nkb, T0 + nt) - T0;
#pragma unroll
      for (int tt = 0; tt < kSmxTiles; ++tt) {
        if (tt >= tlo && tt < thi) {
          const int kb = T0 + tt - c * nkb;
          ensure(kb / (kSmxPiece / 32));
          const float* col = mybuf + (kb % (kSmxPiece / 32)) * 32 + r;
#pragma unroll
          for (int j = 0; j < 16; ++j)
            acc[tt] = mfma32(g[j], col[c_row(j, lane) * kSmxPitch], acc[tt]);
        }
      }
    }
    __syncthreads();          // the buffers' and the labels' readers are done
    if (more && npiece == 1) put(chunk + 4, 0);
  }

  // the four waves' partial sums, ((w0 + w1) + w2) + w3, four tiles at a time
  __syncthreads();
#pragma unroll
  for (int g4 = 0; g4 < kSmxTiles / 4; ++g4) {
    if (4 * g4 >= nt) break;
    if (w > 0) {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int q = 0; q < 16; ++q)
          buf[(((w - 1) * 4 + tt) * 16 + q) * 64 + lane] = acc[4 * g4 + tt][q];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int ww = 0; ww < 3; ++ww)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int q = 0; q < 16; ++q)
            acc[4 * g4 + tt][q] += buf[((ww * 4 + tt) * 16 + q) * 64 + lane];
    }
    __syncthreads();
  }
  if (w != 0) return;

  // S[i][1 + c p + col] = scale (wt acc - a_i W_i[c][col]); register q: particle c_row(q, lane)
#pragma unroll
  for (int tt = 0; tt < kSmxTiles; ++tt) {
    if (tt >= nt) continue;
    const int T = T0 + tt, c = T / nkb, kb = T - c * nkb;
    const int col = 32 * kb + r;
    const int64_t off = 1 + (int64_t)c * p + min(col, p - 1);
    float xv[16];          // the tile's 16 loads in flight, then its stores
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t ii = i0 + c_row(q, lane);
      xv[q] = X[(ii < n ? ii : 0) * ldx + off];
    }
    if (col < p) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rr = c_row(q, lane);
        const int64_t ii = i0 + rr;
        if (ii < n) S[ii * lds + off] = scale * (wt * acc[tt][q] - sa[rr] * xv[q]);
      }
    }
  }
  if (blockIdx.y == 0) {
    // |W|^2: the half h sums entries h, h + 2, ..., then the two halves
    float w2 = 0.f;
    const int cp = C * p;
    for (int e = h; e < cp; e += 2) {
      const float v = x[1 + e];
      w2 = fmaf(v, v, w2);
    }
    w2 += __shfl_xor(w2, 32, 64);
    if (h == 0 && live) {
      const float a = sa[r];
      S[i * lds] = scale * (0.5f * (float)cp - 0.5f * a * w2 + a0 - b0 * a);
    }
  }
}

// softmax of the C logits every lane holds: z[c] <- pi_c (ascending sums)
__device__ __forceinline__ void smx_softmax(float (&z)[kSmxMaxC], int C) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < kSmxMaxC; ++c)
    if (c < C) m = fmaxf(m, z[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kSmxMaxC; ++c)
    if (c < C) {
      z[c] = expf(z[c] - m);
      s += z[c];
    }
#pragma unroll
  for (int c = 0; c < kSmxMaxC; ++c)
    if (c < C) z[c] = z[c] / s;
}

// one workgroup per particle (n <= kSmxSmallRows)
__global__ __launch_bounds__(256) void softmax_row_kernel(
    const float* __restrict__ X, int64_t ldx, int C, int p, const float* __restrict__ Xd,
    int64_t ldxd, const int32_t* __restrict__ y, int64_t N, const int64_t* __restrict__ cursor,
    int64_t B, float wt, float a0, float b0, float scale, float* __restrict__ S, int64_t lds) {
  __shared__ float sw[kSmxMaxD];
  __shared__ float g[kSmxSmallChunk * kSmxMaxC];
  __shared__ float red[4];
  const float* x = X + (int64_t)blockIdx.x * ldx;
  float* out = S + (int64_t)blockIdx.x * lds;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cp = C * p;
  const int64_t org = smx_origin(cursor, N);
  for (int e = tid; e < cp; e += 256) sw[e] = x[1 + e];
  int oc[4], ok[4];          // the class and the column of output entry tid + 256 u
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = min(tid + 256 * u, cp - 1);
    oc[u] = e / p;
    ok[u] = e - oc[u] * p;
  }
  __syncthreads();
  for (int64_t c0 = 0; c0 < B; c0 += kSmxSmallChunk) {
    const int cnt = (int)min((int64_t)kSmxSmallChunk, B - c0);
    for (int q = wv; q < cnt; q += 4) {
      int64_t row = org + c0 + q;
      if (row >= N) row -= N;
      const float* xq = Xd + row * ldxd;
      float z[kSmxMaxC];
#pragma unroll
      for (int c = 0; c < kSmxMaxC; ++c) z[c] = 0.f;
      for (int k = lane; k < p; k += 64) {
        const float v = xq[k];
#pragma unroll
        for (int c = 0; c < kSmxMaxC; ++c)
          if (c < C) z[c] = fmaf(v, sw[c * p + k], z[c]);
      }
#pragma unroll
      for (int c = 0; c < kSmxMaxC; ++c)
        if (c < C) z[c] = warp_sum(z[c]);
      smx_softmax(z, C);
      const int yq = y[row];
#pragma unroll
      for (int c = 0; c < kSmxMaxC; ++c)
        if (lane == c && c < C) g[q * kSmxMaxC + c] = (yq == c ? 1.f : 0.f) - z[c];
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      int64_t row = org + c0 + q;
      if (row >= N) row -= N;
      const float* xq = Xd + row * ldxd;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (tid + 256 * u < cp) acc[u] = fmaf(g[q * kSmxMaxC + oc[u]], xq[ok[u]], acc[u]);
    }
    __syncthreads();
  }
  const float a = expf(x[0]);
  float w2 = 0.f;
  for (int e = tid; e < cp; e += 256) w2 = fmaf(sw[e], sw[e], w2);
  w2 = warp_sum(w2);
  if (lane == 0) red[wv] = w2;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (tid + 256 * u < cp)
      out[1 + tid + 256 * u] = scale * (wt * acc[u] - a * sw[tid + 256 * u]);
  if (tid == 0)
    out[0] = scale * (0.5f * (float)cp - 0.5f * a * ((red[0] + red[1]) + (red[2] + red[3])) + a0 -
                      b0 * a);
}

// ---- predictive probabilities ------------------------------------------------
constexpr int kSmxPredBlocks = 64;   // most particle slices per test row

__host__ __device__ inline int smx_pred_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < kSmxPredBlocks ? b : kSmxPredBlocks);
}

// part[(q nblk + blk) C + c] = sum over the slice's particles of softmax_c(W_i xt_q):
// a thread per particle (slice blk: particles 256 (blk + nblk m) + tid), the
// same forward pass as the row form, then the block's sum in a fixed order
__global__ __launch_bounds__(256) void softmax_predict_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t n, int C, int p, const float* __restrict__ Xt,
    int64_t ldxt, float* __restrict__ part) {
  __shared__ float sx[kSmxMaxD];
  __shared__ float red[4][kSmxMaxC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nblk = gridDim.y, blk = blockIdx.y;
  const float* xt = Xt + (int64_t)blockIdx.x * ldxt;
  for (int k = tid; k < p; k += 256) sx[k] = xt[k];
  __syncthreads();
  float pr[kSmxMaxC];
#pragma unroll
  for (int c = 0; c < kSmxMaxC; ++c) pr[c] = 0.f;
  for (int64_t i = (int64_t)blk * 256 + tid; i < n; i += (int64_t)nblk * 256) {
    const float* wi = X + i * ldx + 1;
    float z[kSmxMaxC];
#pragma unroll
    for (int c = 0; c < kSmxMaxC; ++c) {
      z[c] = 0.f;
      if (c < C)
        for (int k = 0; k < p; ++k) z[c] = fmaf(sx[k], wi[c * p + k], z[c]);
    }
    smx_softmax(z, C);
#pragma unroll
    for (int c = 0; c < kSmxMaxC; ++c)
      if (c < C) pr[c] += z[c];
  }
#pragma unroll
  for (int c = 0; c < kSmxMaxC; ++c)
    if (c < C) {
      const float v = warp_sum(pr[c]);
      if (lane == 0) red[wv][c] = v;
    }
  __syncthreads();
  if (tid < C)
    part[((int64_t)blockIdx.x * nblk + blk) * C + tid] =
        (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(256) void softmax_predict_finish_kernel(
    const float* __restrict__ part, int nblk, int64_t Nt, int C, float inv_n, float* __restrict__ P,
    int64_t ldp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= Nt * C) return;
  const int64_t q = e / C;
  const int c = (int)(e - q * C);
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += part[(q * nblk + b) * C + c];
  P[q * ldp + c] = s * inv_n;
}

static int smx_check(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                     int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p) {
  DSVGD_REQUIRE(X && Xd && y, "null pointer");
  DSVGD_REQUIRE(C >= 2 && C <= kSmxMaxC, "softmax: 2 <= C <= DSVGD_SOFTMAX_MAX_CLASSES");
  DSVGD_REQUIRE(p >= 1 && p <= kSmxMaxD, "softmax: p >= 1");
  DSVGD_REQUIRE(d == 1 + C * p && d <= kSmxMaxD, "softmax: d = 1 + C p <= 1024");
  DSVGD_REQUIRE(n > 0 && N > 0 && ldx >= d && ldxd >= p, "sizes");
  return 0;
}

static int smx_score(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                     int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p, float a0,
                     float b0, float scale, const int64_t* cursor, int64_t B, float* S, int64_t lds,
                     bool force_row, void* stream) {
  DSVGD_REQUIRE(S, "null pointer");
  if (int rc = smx_check(X, ldx, n, d, Xd, ldxd, y, N, C, p)) return rc;
  DSVGD_REQUIRE(lds >= d, "sizes");
  DSVGD_REQUIRE(B >= 1 && B <= N, "softmax: the window needs 1 <= B <= N");
  DSVGD_REQUIRE(B <= ((int64_t)1 << 30), "softmax: more than 2^30 rows in one sum");
  const float wt = (float)((double)N / (double)B);
  hipStream_t s = (hipStream_t)stream;
  if (n <= kSmxSmallRows || force_row) {
    DSVGD_REQUIRE(n <= 0x7fffffff, "too many rows");
    hipLaunchKernelGGL(softmax_row_kernel, dim3((unsigned)n), dim3(256), 0, s, X, ldx, (int)C,
                       (int)p, Xd, ldxd, y, N, cursor, B, wt, a0, b0, scale, S, lds);
    return check_launch("softmax_row");
  }
  const int64_t tiles = (n + kSmxRows - 1) / kSmxRows;
  DSVGD_REQUIRE(tiles <= 0x7fffffff, "too many row tiles");
  const int ntile = (int)(C * ((p + 31) / 32));
  const int nslab = (ntile + kSmxTiles - 1) / kSmxTiles;
  hipLaunchKernelGGL(softmax_tile_kernel, dim3((unsigned)tiles, (unsigned)nslab), dim3(256), 0, s,
                     X, ldx, n, (int)C, (int)p, Xd, ldxd, y, N, cursor, (int)B, wt, a0, b0, scale, S,
                     lds);
  return check_launch("softmax_tile");
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int dsvgd_score_softmax(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                        int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p, float a0,
                        float b0, float scale, float* S, int64_t lds, void* stream) {
  return smx_score(X, ldx, n, d, Xd, ldxd, y, N, C, p, a0, b0, scale, nullptr, N, S, lds, false,
                   stream);
}

int dsvgd_score_softmax_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                               int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p,
                               float a0, float b0, float scale, const int64_t* cursor, int64_t B,
                               float* S, int64_t lds, void* stream) {
  DSVGD_REQUIRE(cursor, "null pointer");
  return smx_score(X, ldx, n, d, Xd, ldxd, y, N, C, p, a0, b0, scale, cursor, B, S, lds, false,
                   stream);
}

int dsvgd_score_softmax_rows(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                             int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p,
                             float a0, float b0, float scale, const int64_t* cursor, int64_t B,
                             float* S, int64_t lds, void* stream) {
  return smx_score(X, ldx, n, d, Xd, ldxd, y, N, C, p, a0, b0, scale, cursor, B, S, lds, true,
                   stream);
}

int64_t dsvgd_softmax_small_rows(void) { return kSmxSmallRows; }

size_t dsvgd_softmax_predict_workspace_bytes(int64_t n, int64_t Nt, int64_t C) {
  if (n < 1 || Nt < 1 || C < 1) return 0;
  return (size_t)Nt * (size_t)smx_pred_blocks(n) * (size_t)C * sizeof(float);
}

int dsvgd_softmax_predict(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xt,
                          int64_t ldxt, int64_t Nt, int64_t C, int64_t p, float* P, int64_t ldp,
                          void* workspace, void* stream) {
  DSVGD_REQUIRE(X && Xt && P && workspace, "null pointer");
  DSVGD_REQUIRE(C >= 2 && C <= kSmxMaxC, "softmax: 2 <= C <= DSVGD_SOFTMAX_MAX_CLASSES");
  DSVGD_REQUIRE(p >= 1 && d == 1 + C * p && d <= kSmxMaxD, "softmax: d = 1 + C p <= 1024");
  DSVGD_REQUIRE(n > 0 && Nt > 0 && Nt <= 0x7fffffff && ldx >= d && ldxt >= p && ldp >= C, "sizes");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = smx_pred_blocks(n);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(softmax_predict_kernel, dim3((unsigned)Nt, (unsigned)nblk), dim3(256), 0, s, X,
                     ldx, n, (int)C, (int)p, Xt, ldxt, part);
  if (int rc = check_launch("softmax_predict")) return rc;
  const int64_t blocks = (Nt * C + 255) / 256;
  hipLaunchKernelGGL(softmax_predict_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, s, part,
                     nblk, Nt, (int)C, (float)(1.0 / (double)n), P, ldp);
  return check_launch("softmax_predict_finish");
}

}  // extern "C"
