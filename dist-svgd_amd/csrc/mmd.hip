// mmd.hip -- the maximum mean discrepancy between two particle sets P (the
// first nf rows) and Q (the rest) of one pooled, packed set of n particles,
// from the distance matrix D the engine already holds ("MMD
// two-sample diagnostic").
//
// With k = exp(-D/h), or (1 + D/h)^beta for the inverse multiquadric,
//   rP_i = sum_{j < nf, j != i} k_ij,   rQ_i = sum_{j >= nf, j != i} k_ij
// are the one sweep over D below (the row sums of K split at column nf); the
// finish forms PP = sum_{i < nf} rP_i, PQ = sum_{i < nf} rQ_i, QQ =
// sum_{i >= nf} rQ_i in fp64, the V- and U-statistics and the witness
//   w_i = (rP_i + [i < nf]) / nf - (rQ_i + [i >= nf]) / (n - nf).
// The diagonal is never read (the Gram form does not give D_ii = 0 exactly):
// its terms k_ii = 1 enter as exact constants.
//
// Everything is deterministic: no float atomics, every partial has a slot of
// its own and every sum a fixed order.  The layouts, the slots and the
// traversal are those of ksd.hip.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace dsvgd {

constexpr int kMmdPanel = 2048;       // 128 rows x 16 columns of D, contiguous
constexpr int kMmdBlockTarget = 2048; // workgroups that fill 256 CUs 8 deep
constexpr int kMmdRowsPerBlock = 64;  // rows of one finish workgroup

template <int FAM>
__device__ __forceinline__ float mmd_k(float v, float scale, float beta) {
  if constexpr (FAM == kFamIMQ)
    return __builtin_amdgcn_exp2f(beta * __builtin_amdgcn_logf(fmaf(v, scale, 1.f)));
  else
    return __builtin_amdgcn_exp2f(v * scale);
}

// One panel's share of a thread: rows g0 (v0) and g0 + 64 (v1), four columns
// from j0.  EDGE = false: the panel lies inside the matrix, off the diagonal
// and in one class (pcls: its columns are all < nf) -- the four kernel values
// of a row are added, then sent to rP or rQ.  EDGE = true: entries with a row
// or column past the matrix (+inf pads) or on the diagonal contribute exactly
// 0, and every column picks its own class.  COLS: cv[0..3] = the two rows'
// values per column that belong to rP of the transposed entry (the stored
// row is < nf: pr0 / pr1), cv[4..7] = those that belong to rQ.
template <bool EDGE, bool COLS, int FAM>
__device__ __forceinline__ void mmd_panel(const f32x4 v0, const f32x4 v1, float scale, float beta,
                                          int g0, int j0, bool rv0, bool rv1, int n, int nf,
                                          bool pcls, bool pr0, bool pr1, float& p0, float& q0,
                                          float& p1, float& q1, float* cv) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float k0 = mmd_k<FAM>(v0[e], scale, beta);
    float k1 = mmd_k<FAM>(v1[e], scale, beta);
    if (EDGE) {
      const int j = j0 + e;
      k0 = (rv0 && j < n && j != g0) ? k0 : 0.f;
      k1 = (rv1 && j < n && j != g0 + 64) ? k1 : 0.f;
      const bool jp = j < nf;
      p0 += jp ? k0 : 0.f;
      q0 += jp ? 0.f : k0;
      p1 += jp ? k1 : 0.f;
      q1 += jp ? 0.f : k1;
    } else {
      s0 += k0;
      s1 += k1;
    }
    if (COLS) {
      cv[e] = (pr0 ? k0 : 0.f) + (pr1 ? k1 : 0.f);
      cv[4 + e] = (pr0 ? 0.f : k0) + (pr1 ? 0.f : k1);
    }
  }
  if (!EDGE) {
    p0 += pcls ? s0 : 0.f;
    q0 += pcls ? 0.f : s0;
    p1 += pcls ? s1 : 0.f;
    q1 += pcls ? 0.f : s1;
  }
}

// the four lanes that share a row hold its partial sums
__device__ __forceinline__ float mmd_quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

__device__ __forceinline__ double mmd_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Full panel layout: workgroup (I, z) walks the 16-column panels of row tile
// I in column slice z; thread t reads two 16-byte pieces per panel (rows t/4
// and t/4 + 64, columns 4 (t % 4) ..), a wave 1 KiB contiguous per load.
// P[z][0][i] = rP, P[z][1][i] = rQ of the slice.  No LDS.
template <int FAM>
__global__ __launch_bounds__(256) void mmd_rows_full_kernel(
    const float* __restrict__ D, int n_pad, int n, int nf,
    const dsvgd_select_state* __restrict__ st, int parts, float* __restrict__ P, float beta) {
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2;
  const int I = blockIdx.x, z = blockIdx.y;
  const int pcols = n_pad >> 4;
  const int c0 = (int)((int64_t)pcols * z / parts), c1 = (int)((int64_t)pcols * (z + 1) / parts);
  const float scale = FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e;
  const int i0 = I * 128 + r0;
  const bool rv0 = i0 < n, rv1 = i0 + 64 < n;
  const int gt = I * 128;                // the tile's first own column
  const bool row_edge = (I + 1) * 128 > n;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + (int64_t)I * pcols * (kMmdPanel / 4) + t;
  float p0 = 0.f, q0 = 0.f, p1 = 0.f, q1 = 0.f;
#pragma unroll 2
  for (int c = c0; c < c1; ++c) {
    const f32x4 v0 = Dp[(int64_t)c * (kMmdPanel / 4)];
    const f32x4 v1 = Dp[(int64_t)c * (kMmdPanel / 4) + 256];
    const int j0 = 16 * c + 4 * cq;
    const bool edge = row_edge || 16 * c + 16 > n || (16 * c + 15 >= gt && 16 * c <= gt + 127) ||
                      (16 * c < nf && 16 * c + 16 > nf);
    if (edge)
      mmd_panel<true, false, FAM>(v0, v1, scale, beta, i0, j0, rv0, rv1, n, nf, false, false,
                                  false, p0, q0, p1, q1, nullptr);
    else
      mmd_panel<false, false, FAM>(v0, v1, scale, beta, i0, j0, rv0, rv1, n, nf, 16 * c < nf,
                                   false, false, p0, q0, p1, q1, nullptr);
  }
  p0 = mmd_quad_sum(p0);
  p1 = mmd_quad_sum(p1);
  q0 = mmd_quad_sum(q0);
  q1 = mmd_quad_sum(q1);
  if (cq == 0) {
    float* Pz = P + (int64_t)z * 2 * n_pad;
    Pz[i0] = p0;
    Pz[i0 + 64] = p1;
    Pz[n_pad + i0] = q0;
    Pz[n_pad + i0 + 64] = q1;
  }
}

// Eight per-thread values (two quantities x four columns) summed over the 16
// lanes of a wave that hold the same columns (lane bits 2..5), each step
// trading half of what is left: 8 cross-lane moves instead of 32.  Returns,
// in every lane, the wave's sum of quantity (lane >> 2) & 1 for the column
// 2 ((lane >> 3) & 1) + ((lane >> 4) & 1) of the lane's quad.
__device__ __forceinline__ float mmd_col_reduce(const float* v, int lane) {
  const bool bA = lane & 4, bB = lane & 8, bC = lane & 16;
  float w[4], x[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float keep = bA ? v[k + 4] : v[k], send = bA ? v[k] : v[k + 4];
    w[k] = keep + __shfl_xor(send, 4, 64);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float keep = bB ? w[k + 2] : w[k], send = bB ? w[k] : w[k + 2];
    x[k] = keep + __shfl_xor(send, 8, 64);
  }
  const float keep = bC ? x[1] : x[0], send = bC ? x[0] : x[1];
  float y = keep + __shfl_xor(send, 16, 64);
  y += __shfl_xor(y, 32, 64);
  return y;
}

// Symmetric layout (only tiles (I, J >= I) stored): workgroup (I, z) walks
// slice z of the stored tiles of tile row I.  Row sums as above into slot z;
// an off-diagonal tile's column sums (the terms of the unwritten tile (J, I):
// k_ji for i in I, to rP_j where i < nf and to rQ_j otherwise -- a tile row
// that straddles nf feeds both) go to slot rparts + I at rows of J, one slot
// per stored tile row, summed by the finish for I < J in order.  The diagonal
// tile counts once, without its diagonal.
template <int FAM>
__global__ __launch_bounds__(256) void mmd_rows_sym_kernel(
    const float* __restrict__ D, int n_pad, int n, int nf,
    const dsvgd_select_state* __restrict__ st, int rparts, float* __restrict__ P, float beta) {
  __shared__ float red[4][2][128];
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2, lane = t & 63, wv = t >> 6;
  const int I = blockIdx.x, z = blockIdx.y;
  const int T = n_pad >> 7, pcols = n_pad >> 4, len = T - I;
  const int J0 = I + (int)((int64_t)len * z / rparts), J1 = I + (int)((int64_t)len * (z + 1) / rparts);
  const float scale = FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e;
  const int i0 = I * 128 + r0;
  const bool rv0 = i0 < n, rv1 = i0 + 64 < n;
  const bool pr0 = i0 < nf, pr1 = i0 + 64 < nf;
  const bool pads = n < n_pad;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + (int64_t)I * pcols * (kMmdPanel / 4) + t;
  float* Pc = P + (int64_t)(rparts + I) * 2 * n_pad;
  // the lane's result of mmd_col_reduce: quantity and column within a panel
  const int cqty = (lane >> 2) & 1;
  const int ccol = 4 * cq + 2 * ((lane >> 3) & 1) + ((lane >> 4) & 1);
  float p0 = 0.f, q0 = 0.f, p1 = 0.f, q1 = 0.f;
  for (int J = J0; J < J1; ++J) {
    const bool diag = J == I;
    const bool tedge = diag || (pads && (I == T - 1 || J == T - 1));
#pragma unroll 2
    for (int p = 0; p < 8; ++p) {
      const int c = J * 8 + p;
      const f32x4 v0 = Dp[(int64_t)c * (kMmdPanel / 4)];
      const f32x4 v1 = Dp[(int64_t)c * (kMmdPanel / 4) + 256];
      const int j0 = 16 * c + 4 * cq;
      const bool edge = tedge || (16 * c < nf && 16 * c + 16 > nf);
      float cv[8];
      if (edge)
        mmd_panel<true, true, FAM>(v0, v1, scale, beta, i0, j0, rv0, rv1, n, nf, false, pr0, pr1,
                                   p0, q0, p1, q1, cv);
      else
        mmd_panel<false, true, FAM>(v0, v1, scale, beta, i0, j0, rv0, rv1, n, nf, 16 * c < nf,
                                    pr0, pr1, p0, q0, p1, q1, cv);
      if (!diag) {  // block-uniform
        const float y = mmd_col_reduce(cv, lane);
        if (lane < 32) red[wv][cqty][16 * p + ccol] = y;
      }
    }
    if (!diag) {
      __syncthreads();
      const int qty = t >> 7, col = t & 127;
      const float s = ((red[0][qty][col] + red[1][qty][col]) + red[2][qty][col]) + red[3][qty][col];
      Pc[(int64_t)qty * n_pad + J * 128 + col] = s;
      __syncthreads();
    }
  }
  p0 = mmd_quad_sum(p0);
  p1 = mmd_quad_sum(p1);
  q0 = mmd_quad_sum(q0);
  q1 = mmd_quad_sum(q1);
  if (cq == 0) {
    float* Pz = P + (int64_t)z * 2 * n_pad;
    Pz[i0] = p0;
    Pz[i0 + 64] = p1;
    Pz[n_pad + i0] = q0;
    Pz[n_pad + i0 + 64] = q1;
  }
}

// rP_i, rQ_i and the witness for 64 rows per workgroup: wave w adds the slots
// w, w + 4, .. of 64 consecutive rows (coalesced, fp64), the four wave sums
// are added in order.  ws[3 blk + 0..2] = the workgroup's shares of PP, PQ,
// QQ in row order.
__global__ __launch_bounds__(256) void mmd_finish_kernel(const float* __restrict__ P, int n_pad,
                                                         int n, int nf, int sym, int parts,
                                                         float* __restrict__ rp,
                                                         float* __restrict__ rq,
                                                         float* __restrict__ witness,
                                                         double* __restrict__ ws) {
  __shared__ double shp[4][64], shq[4][64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ib = blockIdx.x * kMmdRowsPerBlock;
  const int i = ib + lane;
  {
    // symmetric layout: slots [0, rparts) the row sums, then one per stored
    // tile row I < this row's tile (the 64 rows share a tile)
    const int nslots = sym ? parts - (n_pad >> 7) + (ib >> 7) : parts;
    double p = 0.0, q = 0.0;
    if (i < n) {
#pragma unroll 4
      for (int sl = wv; sl < nslots; sl += 4) {
        const float* Ps = P + (int64_t)sl * 2 * n_pad;
        p += (double)Ps[i];
        q += (double)Ps[n_pad + i];
      }
    }
    shp[wv][lane] = p;
    shq[wv][lane] = q;
  }
  __syncthreads();
  if (t < 64) {
    const bool ok = i < n, first = i < nf;
    const double p = ((shp[0][t] + shp[1][t]) + shp[2][t]) + shp[3][t];
    const double q = ((shq[0][t] + shq[1][t]) + shq[2][t]) + shq[3][t];
    if (ok) {
      if (rp) rp[i] = (float)p;
      if (rq) rq[i] = (float)q;
      if (witness)
        witness[i] = (float)((p + (first ? 1.0 : 0.0)) / (double)nf -
                             (q + (first ? 0.0 : 1.0)) / (double)(n - nf));
    }
    const double pp = mmd_wave_sum_f64(ok && first ? p : 0.0);
    const double pq = mmd_wave_sum_f64(ok && first ? q : 0.0);
    const double qq = mmd_wave_sum_f64(ok && !first ? q : 0.0);
    if (t == 0) {
      double* w = ws + 3 * (int64_t)blockIdx.x;
      w[0] = pp;
      w[1] = pq;
      w[2] = qq;
    }
  }
}

// the second level: thread t adds the workgroup sums t, t + 256, .. in order,
// then a fixed halving tree; out = [PP, PQ, QQ, V, U]
__global__ __launch_bounds__(256) void mmd_reduce_kernel(const double* __restrict__ ws, int nb,
                                                         int n, int nf, double* __restrict__ out) {
  __shared__ double sh[3][256];
  const int t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int b = t; b < nb; b += 256) {
    s0 += ws[3 * (int64_t)b];
    s1 += ws[3 * (int64_t)b + 1];
    s2 += ws[3 * (int64_t)b + 2];
  }
  sh[0][t] = s0;
  sh[1][t] = s1;
  sh[2][t] = s2;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      sh[0][t] += sh[0][t + h];
      sh[1][t] += sh[1][t + h];
      sh[2][t] += sh[2][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double pp = sh[0][0], pq = sh[1][0], qq = sh[2][0];
    const double a = (double)nf, b = (double)(n - nf);
    out[0] = pp;
    out[1] = pq;
    out[2] = qq;
    out[3] = (pp + a) / (a * a) + (qq + b) / (b * b) - 2.0 * pq / (a * b);
    out[4] = (nf > 1 && n - nf > 1)
                 ? pp / (a * (a - 1.0)) + qq / (b * (b - 1.0)) - 2.0 * pq / (a * b)
                 : (double)NAN;
  }
}

// the largest pooled set whose indices and panel offsets the kernels hold in
// 32-bit ints (its D alone would be 4 TiB)
constexpr int64_t kMmdMaxN = 1 << 20;

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int64_t dsvgd_mmd_parts(int64_t n_total, int sym, int64_t force) {
  if (n_total <= 0 || n_total > kMmdMaxN) return 0;
  const int64_t T = roundup(n_total, 128) / 128;
  // full layout: at least eight panels (128 columns) per slice
  const int64_t rparts =
      force > 0 ? std::min<int64_t>(force, T)
                : std::max<int64_t>(1, std::min<int64_t>((kMmdBlockTarget + T - 1) / T, T));
  return sym ? rparts + T : rparts;
}

size_t dsvgd_mmd_workspace_doubles(int64_t n_total) {
  return n_total > 0 ? 3 * (size_t)((n_total + kMmdRowsPerBlock - 1) / kMmdRowsPerBlock) : 0;
}

int dsvgd_mmd_rows(const float* D, int64_t ldd, int64_t n_total, int64_t n_first,
                   const dsvgd_select_state* st, dsvgd_kernel kern, int sym, int64_t parts,
                   int64_t force, float* P, void* stream) {
  DSVGD_REQUIRE(kern_ok(kern), "kern: family RBF, or IMQ with beta in [-1, 0)");
  DSVGD_REQUIRE(D && st && P, "null pointer");
  DSVGD_REQUIRE(n_total >= 2 && n_total <= kMmdMaxN, "sizes: 2 <= n_total <= 2^20");
  DSVGD_REQUIRE(n_first >= 1 && n_first < n_total, "sizes: 1 <= n_first < n_total");
  const int64_t n_pad = roundup(n_total, 128), T = n_pad / 128;
  DSVGD_REQUIRE(ldd == n_pad, "ldd must equal roundup(n_total,128) (panel layout)");
  DSVGD_REQUIRE(((uintptr_t)D & 15) == 0 && ((uintptr_t)P & 3) == 0,
                "D must be 16-byte aligned, P 4-byte aligned");
  DSVGD_REQUIRE(parts > 0 && parts == dsvgd_mmd_parts(n_total, sym, force),
                "parts must be dsvgd_mmd_parts(n_total, sym, force)");
  hipStream_t s = (hipStream_t)stream;
  const bool imq = kern.family == DSVGD_KERNEL_IMQ;
  if (sym) {
    const int64_t rparts = parts - T;
    const dim3 grid((unsigned)T, (unsigned)rparts);
    if (imq)
      hipLaunchKernelGGL(mmd_rows_sym_kernel<kFamIMQ>, grid, dim3(256), 0, s, D, (int)n_pad,
                         (int)n_total, (int)n_first, st, (int)rparts, P, kern.beta);
    else
      hipLaunchKernelGGL(mmd_rows_sym_kernel<kFamRBF>, grid, dim3(256), 0, s, D, (int)n_pad,
                         (int)n_total, (int)n_first, st, (int)rparts, P, 0.f);
    return check_launch("mmd_rows_sym");
  }
  const dim3 grid((unsigned)T, (unsigned)parts);
  if (imq)
    hipLaunchKernelGGL(mmd_rows_full_kernel<kFamIMQ>, grid, dim3(256), 0, s, D, (int)n_pad,
                       (int)n_total, (int)n_first, st, (int)parts, P, kern.beta);
  else
    hipLaunchKernelGGL(mmd_rows_full_kernel<kFamRBF>, grid, dim3(256), 0, s, D, (int)n_pad,
                       (int)n_total, (int)n_first, st, (int)parts, P, 0.f);
  return check_launch("mmd_rows_full");
}

int dsvgd_mmd_finish(const float* P, int64_t n_total, int64_t n_first, int sym, int64_t parts,
                     int64_t force, float* rp, float* rq, float* witness, double* ws,
                     double* out, void* stream) {
  DSVGD_REQUIRE(P && ws && out, "null pointer");
  DSVGD_REQUIRE(n_total >= 2 && n_total <= kMmdMaxN, "sizes: 2 <= n_total <= 2^20");
  DSVGD_REQUIRE(n_first >= 1 && n_first < n_total, "sizes: 1 <= n_first < n_total");
  DSVGD_REQUIRE(parts > 0 && parts == dsvgd_mmd_parts(n_total, sym, force),
                "parts must be dsvgd_mmd_parts(n_total, sym, force)");
  DSVGD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0,
                "ws and out must be 8-byte aligned");
  DSVGD_REQUIRE(((uintptr_t)P & 3) == 0 && ((uintptr_t)rp & 3) == 0 && ((uintptr_t)rq & 3) == 0 &&
                    ((uintptr_t)witness & 3) == 0,
                "P, rp, rq and witness must be 4-byte aligned");
  const int64_t n_pad = roundup(n_total, 128);
  const int64_t nb = (n_total + kMmdRowsPerBlock - 1) / kMmdRowsPerBlock;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mmd_finish_kernel, dim3((unsigned)nb), dim3(256), 0, s, P, (int)n_pad,
                     (int)n_total, (int)n_first, sym ? 1 : 0, (int)parts, rp, rq, witness, ws);
  int rc = check_launch("mmd_finish");
  if (rc) return rc;
  hipLaunchKernelGGL(mmd_reduce_kernel, dim3(1), dim3(256), 0, s, ws, (int)nb, (int)n_total,
                     (int)n_first, out);
  return check_launch("mmd_reduce");
}

}  // extern "C"
