// ksd.hip -- the kernelized Stein discrepancy of the particles of one Jacobi
// step, from what the step left on the device ("KSD diagnostic").
//
// For k = exp(-|x - y|^2 / h) the Stein kernel is
//   u_ij = k_ij [ s_i.s_j + (2/h)(s_i - s_j).(x_i - x_j) + 2d/h - (4/h^2) D_ij ]
// and its off-diagonal row sum splits into pieces of the step:
//   t_i = s_i.KS_i + (2/h)[ r_i a_i - s_i.KXc_i - xc_i.KS_i + b_i ]
//         + (2d/h) r_i - (4/h^2) q_i,
//   a_j = s_j.xc_j,  b_i = sum_{j != i} k_ij a_j,  q_i = sum_{j != i} k_ij D_ij.
// KXc, KS, r are phi_mm's outputs; b and q are the one sweep over D below.
//
// For the inverse multiquadric k = u^beta, u = 1 + D/h (FAM = IMQ below), with
// F = u^beta, G' = u^(beta-1), H' = u^(beta-2), c1 = -2 beta/h, c2 = 4 beta
// (beta-1)/h^2:
//   u_ij = F s_i.s_j + c1 G' [(s_i - s_j).(x_i - x_j) + d] - c2 H' D_ij,
//   t_i = s_i.FS_i + c1 [rG_i a_i - s_i.G'Xc_i - xc_i.G'S_i + b_i + d rG_i] - c2 q_i,
//   b_i = sum_{j != i} G'_ij a_j,  q_i = sum_{j != i} H'_ij D_ij,  u_ii = |s_i|^2 + c1 d.
// FS comes from phi_mm's F run, G'Xc, G'S and rG from its G' run.
//
// Everything is deterministic: no float atomics, every partial has a slot of
// its own and every sum a fixed order.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace dsvgd {

constexpr int kKsdPanel = 2048;       // 128 rows x 16 columns of D, contiguous
constexpr int kKsdBlockTarget = 2048; // workgroups that fill 256 CUs 8 deep
constexpr int kKsdRowsPerBlock = 64;  // rows of one finish / direct workgroup
constexpr int kKsdDirectMaxD = 64;
constexpr int kKsdDirectJ = 32;       // columns staged per chunk (direct form)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a[j] = s_j . xc_j for j < n, 0 for n <= j < n_pad (fp64 dot, one wave per row)
__global__ __launch_bounds__(256) void ksd_a_kernel(const float* __restrict__ Y, int64_t ldy,
                                                    int64_t dp, int64_t d, int64_t n,
                                                    int64_t n_pad, float* __restrict__ a) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n_pad) return;
  double s = 0.0;
  if (j < n) {
    const float* y = Y + j * ldy;
    for (int64_t c = lane; c < d; c += 64) s += (double)y[c] * (double)y[dp + c];
  }
  s = wave_sum_f64(s);
  if (lane == 0) a[j] = (float)s;
}

// One panel's share of a thread: rows r0 (v0) and r0 + 64 (v1), four columns
// from j0.  q += k D, b += k a_j per row; COLS: cv[0..3] = the two rows' k D
// per column, cv[4..7] = their k a_i (the transposed tile's terms).  MASK:
// entries with a row or column past the matrix (+inf pads: exp(-inf) inf is
// NaN) or on the diagonal contribute exactly 0.
// FAM = IMQ: k -> G' = u^pw (pw = beta - 1, scale = 1/h) and k D -> H' D =
// u^(pw-1) D.
template <bool MASK, bool COLS, int FAM = kFamRBF>
__device__ __forceinline__ void ksd_panel(const f32x4 v0, const f32x4 v1, const f32x4 a4,
                                          float scale, int64_t g0, int64_t j0, bool rv0, bool rv1,
                                          int64_t n, float ai0, float ai1, float& q0, float& b0,
                                          float& q1, float& b1, float* cv, float pw = 0.f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float k0, k1, kd0, kd1;
    if constexpr (FAM == kFamIMQ) {
      const float l0 = __builtin_amdgcn_logf(fmaf(v0[e], scale, 1.f));
      const float l1 = __builtin_amdgcn_logf(fmaf(v1[e], scale, 1.f));
      k0 = __builtin_amdgcn_exp2f(pw * l0);
      k1 = __builtin_amdgcn_exp2f(pw * l1);
      kd0 = __builtin_amdgcn_exp2f((pw - 1.f) * l0) * v0[e];
      kd1 = __builtin_amdgcn_exp2f((pw - 1.f) * l1) * v1[e];
    } else {
      k0 = __builtin_amdgcn_exp2f(v0[e] * scale);
      k1 = __builtin_amdgcn_exp2f(v1[e] * scale);
      kd0 = k0 * v0[e];
      kd1 = k1 * v1[e];
    }
    if (MASK) {
      const int64_t j = j0 + e;
      const bool ok0 = rv0 && j < n && j != g0;
      const bool ok1 = rv1 && j < n && j != g0 + 64;
      k0 = ok0 ? k0 : 0.f;
      kd0 = ok0 ? kd0 : 0.f;
      k1 = ok1 ? k1 : 0.f;
      kd1 = ok1 ? kd1 : 0.f;
    }
    q0 += kd0;
    q1 += kd1;
    b0 = fmaf(k0, a4[e], b0);
    b1 = fmaf(k1, a4[e], b1);
    if (COLS) {
      cv[e] = kd0 + kd1;
      cv[4 + e] = fmaf(k0, ai0, k1 * ai1);
    }
  }
}

// the four lanes that share a row hold its partial sums
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// Full panel layout: workgroup (I, z) walks the 16-column panels of row tile
// I in column slice z; thread t reads two 16-byte pieces per panel (rows t/4
// and t/4 + 64, columns 4 (t % 4) ..), a wave 1 KiB contiguous per load.
// P[z][0][i] = q, P[z][1][i] = b of the slice.  No LDS.
template <int FAM = kFamRBF>
__global__ __launch_bounds__(256) void ksd_rows_full_kernel(
    const float* __restrict__ D, int64_t n_pad, const float* __restrict__ a, int64_t row0,
    int64_t m, int64_t n, const dsvgd_select_state* __restrict__ st, int parts,
    float* __restrict__ P, int64_t m_pad, float pw = 0.f) {
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2;
  const int64_t I = blockIdx.x;
  const int z = blockIdx.y;
  const int64_t pcols = n_pad >> 4;
  const int64_t c0 = pcols * z / parts, c1 = pcols * (z + 1) / parts;
  const float scale = FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e;
  const int64_t i0 = I * 128 + r0;
  const bool rv0 = i0 < m, rv1 = i0 + 64 < m;
  const int64_t g0 = row0 + i0;          // the row's own column
  const int64_t gt = row0 + I * 128;     // the tile's first own column
  const bool row_edge = (I + 1) * 128 > m;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + I * pcols * (kKsdPanel / 4) + t;
  float q0 = 0.f, b0 = 0.f, q1 = 0.f, b1 = 0.f;
#pragma unroll 2
  for (int64_t c = c0; c < c1; ++c) {
    const f32x4 v0 = Dp[c * (kKsdPanel / 4)];
    const f32x4 v1 = Dp[c * (kKsdPanel / 4) + 256];
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(a + 16 * c + 4 * cq);
    const int64_t j0 = 16 * c + 4 * cq;
    const bool edge = row_edge || 16 * c + 16 > n || (16 * c + 15 >= gt && 16 * c <= gt + 127);
    if (edge)
      ksd_panel<true, false, FAM>(v0, v1, a4, scale, g0, j0, rv0, rv1, n, 0.f, 0.f, q0, b0, q1, b1,
                                  nullptr, pw);
    else
      ksd_panel<false, false, FAM>(v0, v1, a4, scale, g0, j0, rv0, rv1, n, 0.f, 0.f, q0, b0, q1,
                                   b1, nullptr, pw);
  }
  q0 = quad_sum(q0);
  q1 = quad_sum(q1);
  b0 = quad_sum(b0);
  b1 = quad_sum(b1);
  if (cq == 0) {
    float* Pz = P + (int64_t)z * 2 * m_pad;
    Pz[i0] = q0;
    Pz[i0 + 64] = q1;
    Pz[m_pad + i0] = b0;
    Pz[m_pad + i0 + 64] = b1;
  }
}

// gate[0] = 1 if an owned row's kernel mass r_i = sum_z rowsum[z][i] is below
// tau (or NaN), else 0 (one workgroup; n = 1 has no off-diagonal terms: 0).
__global__ __launch_bounds__(256) void ksd_gate_kernel(const float* __restrict__ rowsum,
                                                       int splits, int64_t m, int64_t m_pad,
                                                       int64_t n, float tau,
                                                       float* __restrict__ gate) {
  __shared__ int flag;
  if (threadIdx.x == 0) flag = 0;
  __syncthreads();
  bool f = false;
  for (int64_t i = threadIdx.x; i < m; i += 256) {
    float r = 0.f;
    for (int z = 0; z < splits; ++z) r += rowsum[(int64_t)z * m_pad + i];
    f = f || !(r >= tau);
  }
  if (f && n > 1) flag = 1;  // (every writer stores the same value)
  __syncthreads();
  if (threadIdx.x == 0) gate[0] = flag ? 1.f : 0.f;
}

// Eight per-thread values (two quantities x four columns) summed over the 16
// lanes of a wave that hold the same columns (lane bits 2..5), each step
// trading half of what is left: 8 cross-lane moves instead of 32.  Returns,
// in every lane, the wave's sum of quantity (lane >> 2) & 1 for the column
// 2 ((lane >> 3) & 1) + ((lane >> 4) & 1) of the lane's quad.
__device__ __forceinline__ float ksd_col_reduce(const float* v, int lane) {
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
// weights a_i, i in I) go to slot rparts + I at rows of J -- one slot per
// stored tile row, summed by the finish for I < J in order.  The diagonal
// tile counts once, without its diagonal.
template <int FAM = kFamRBF>
__global__ __launch_bounds__(256) void ksd_rows_sym_kernel(
    const float* __restrict__ D, int64_t n_pad, const float* __restrict__ a, int64_t n,
    const dsvgd_select_state* __restrict__ st, int rparts, float* __restrict__ P, float pw = 0.f) {
  __shared__ float red[4][2][128];
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2, lane = t & 63, wv = t >> 6;
  const int64_t I = blockIdx.x;
  const int z = blockIdx.y;
  const int64_t T = n_pad >> 7, pcols = n_pad >> 4, len = T - I;
  const int64_t J0 = I + len * z / rparts, J1 = I + len * (z + 1) / rparts;
  const float scale = FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e;
  const int64_t i0 = I * 128 + r0;
  const bool rv0 = i0 < n, rv1 = i0 + 64 < n;
  const float ai0 = a[i0], ai1 = a[i0 + 64];
  const bool pads = n < n_pad;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + I * pcols * (kKsdPanel / 4) + t;
  float* Pc = P + (int64_t)(rparts + I) * 2 * n_pad;
  // the lane's result of ksd_col_reduce: quantity and column within a panel
  const int cqty = (lane >> 2) & 1;
  const int ccol = 4 * cq + 2 * ((lane >> 3) & 1) + ((lane >> 4) & 1);
  float q0 = 0.f, b0 = 0.f, q1 = 0.f, b1 = 0.f;
  for (int64_t J = J0; J < J1; ++J) {
    const bool diag = J == I;
    const bool edge = diag || (pads && (I == T - 1 || J == T - 1));
#pragma unroll 2
    for (int p = 0; p < 8; ++p) {
      const int64_t c = J * 8 + p;
      const f32x4 v0 = Dp[c * (kKsdPanel / 4)];
      const f32x4 v1 = Dp[c * (kKsdPanel / 4) + 256];
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(a + 16 * c + 4 * cq);
      const int64_t j0 = 16 * c + 4 * cq;
      float cv[8];
      if (edge)
        ksd_panel<true, true, FAM>(v0, v1, a4, scale, i0, j0, rv0, rv1, n, ai0, ai1, q0, b0, q1, b1,
                                   cv, pw);
      else
        ksd_panel<false, true, FAM>(v0, v1, a4, scale, i0, j0, rv0, rv1, n, ai0, ai1, q0, b0, q1,
                                    b1, cv, pw);
      if (!diag) {  // block-uniform
        const float y = ksd_col_reduce(cv, lane);
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
  q0 = quad_sum(q0);
  q1 = quad_sum(q1);
  b0 = quad_sum(b0);
  b1 = quad_sum(b1);
  if (cq == 0) {
    float* Pz = P + (int64_t)z * 2 * n_pad;
    Pz[i0] = q0;
    Pz[i0 + 64] = q1;
    Pz[n_pad + i0] = b0;
    Pz[n_pad + i0 + 64] = b1;
  }
}

// t_i, u_ii for 64 rows per workgroup.  First the rows' q and b: wave w adds
// the slots w, w + 4, .. of 64 consecutive rows (coalesced), the four wave
// sums are added in order.  Then one wave per row: the split-K slices summed
// in slice order in fp32 as phi_finish does, the five dot products in fp64.
// ws[2 blk], ws[2 blk + 1] = the workgroup's sums of t and u_ii in row order.
// FAM = IMQ: KY is the F run's [F Xc | F S], KG the G' run's [G' Xc | G' S]
// (row stride ldkg, the same slices), rowsum the G' run's rG.  KG, ldkg and
// beta arrive as one trailing KsdImqArgs that only the IMQ instantiation has
// (KA is empty for the RBF, whose argument block and code stay what they were).
struct KsdImqArgs {
  const float* KG;
  int64_t ldkg;
  float beta;
};
template <class... KA>
__device__ __forceinline__ KsdImqArgs ksd_imq_args(KA... ka) {
  if constexpr (sizeof...(KA) == 0)
    return KsdImqArgs{nullptr, 0, 0.f};
  else
    return (ka, ...);
}

template <int FAM = kFamRBF, class... KA>
__global__ __launch_bounds__(256) void ksd_finish_kernel(
    const float* __restrict__ KY, int64_t ldk, const float* __restrict__ rowsum, int splits,
    const float* __restrict__ Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0, int64_t m,
    int64_t m_pad, const dsvgd_select_state* __restrict__ st, int sym, int parts,
    const float* __restrict__ P, float* __restrict__ rows, double* __restrict__ ws, KA... ka) {
  static_assert(sizeof...(KA) == (FAM == kFamIMQ ? 1 : 0), "KsdImqArgs: the IMQ instantiation only");
  [[maybe_unused]] const KsdImqArgs ia = ksd_imq_args(ka...);
  [[maybe_unused]] const float* const KG = ia.KG;
  [[maybe_unused]] const int64_t ldkg = ia.ldkg;
  [[maybe_unused]] const float beta = ia.beta;
  __shared__ double shq[4][64], shb[4][64], sht[4][2];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t ib = (int64_t)blockIdx.x * kKsdRowsPerBlock;
  {
    // symmetric layout: slots [0, rparts) the row sums, then one per stored
    // tile row I < this row's tile (the 64 rows share a tile)
    const int nslots = sym ? parts - (int)(m_pad >> 7) + (int)(ib >> 7) : parts;
    const int64_t i = ib + lane;
    double q = 0.0, b = 0.0;
    if (i < m) {
#pragma unroll 4
      for (int sl = wv; sl < nslots; sl += 4) {
        const float* Ps = P + (int64_t)sl * 2 * m_pad;
        q += (double)Ps[i];
        b += (double)Ps[m_pad + i];
      }
    }
    shq[wv][lane] = q;
    shb[wv][lane] = b;
  }
  __syncthreads();
  // RBF: g = 2/h (and g^2 = 4/h^2 below); IMQ: c1 (and c2) in their places
  const double ih = (double)st->inv_h, g = FAM == kFamIMQ ? -2.0 * (double)beta * ih : 2.0 * ih;
  double wt = 0.0, wu = 0.0;
  for (int k = 0; k < 16; ++k) {
    const int rr = 16 * wv + k;
    const int64_t i = ib + rr;
    if (i >= m) break;  // wave-uniform
    const float* yi = Y + (row0 + i) * ldy;
    double sKS = 0.0, sKX = 0.0, xKS = 0.0, aa = 0.0, ss = 0.0;
    for (int64_t c = lane; c < d; c += 64) {
      float kx = 0.f, ks = 0.f, gs = 0.f;
      for (int zz = 0; zz < splits; ++zz) {
        const float* ky = KY + ((int64_t)zz * m + i) * ldk;
        if constexpr (FAM == kFamIMQ) {
          const float* kg = KG + ((int64_t)zz * m + i) * ldkg;
          kx += kg[c];
          gs += kg[dp + c];
        } else {
          kx += ky[c];
        }
        ks += ky[dp + c];
      }
      const double x = (double)yi[c], s = (double)yi[dp + c];
      sKS += s * (double)ks;
      sKX += s * (double)kx;
      if constexpr (FAM == kFamIMQ)
        xKS += x * (double)gs;
      else
        xKS += x * (double)ks;
      aa += s * x;
      ss += s * s;
    }
    sKS = wave_sum_f64(sKS);
    sKX = wave_sum_f64(sKX);
    xKS = wave_sum_f64(xKS);
    aa = wave_sum_f64(aa);
    ss = wave_sum_f64(ss);
    float r = 0.f;
    for (int zz = 0; zz < splits; ++zz) r += rowsum[(int64_t)zz * m_pad + i];
    const double q = ((shq[0][rr] + shq[1][rr]) + shq[2][rr]) + shq[3][rr];
    const double b = ((shb[0][rr] + shb[1][rr]) + shb[2][rr]) + shb[3][rr];
    const double rd = (double)r, dd = (double)d;
    double ti;
    if constexpr (FAM == kFamIMQ)
      ti = sKS + g * (rd * aa - sKX - xKS + b) + g * dd * rd -
           4.0 * (double)beta * ((double)beta - 1.0) * ih * ih * q;
    else
      ti = sKS + g * (rd * aa - sKX - xKS + b) + g * dd * rd - g * g * q;
    const double ui = ss + g * dd;
    if (lane == 0 && rows) rows[i] = (float)ti;
    wt += ti;
    wu += ui;
  }
  if (lane == 0) {
    sht[wv][0] = wt;
    sht[wv][1] = wu;
  }
  __syncthreads();
  if (t < 2) ws[2 * (int64_t)blockIdx.x + t] = ((sht[0][t] + sht[1][t]) + sht[2][t]) + sht[3][t];
}

// the second level: thread t adds the workgroup sums t, t + 256, .. in order,
// then a fixed halving tree; out = [off, diag, V, U]
__global__ __launch_bounds__(256) void ksd_reduce_kernel(const double* __restrict__ ws, int64_t nb,
                                                         int64_t n, double* __restrict__ out) {
  __shared__ double sh[2][256];
  const int t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t b = t; b < nb; b += 256) {
    s0 += ws[2 * b];
    s1 += ws[2 * b + 1];
  }
  sh[0][t] = s0;
  sh[1][t] = s1;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      sh[0][t] += sh[0][t + h];
      sh[1][t] += sh[1][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double off = sh[0][0], diag = sh[1][0], nn = (double)n;
    out[0] = off;
    out[1] = diag;
    out[2] = (off + diag) / (nn * nn);
    out[3] = n > 1 ? off / (nn * (nn - 1.0)) : (double)NAN;
  }
}

// d <= 64: t_i from explicit differences, straight from Y.  Workgroup: 64
// rows; thread (r, g) takes row r and the columns jj = g mod 4 of each staged
// chunk; the four partial sums of a row are added in g order.
template <int FAM = kFamRBF>
__global__ __launch_bounds__(256) void ksd_direct_kernel(
    const float* __restrict__ Y, int64_t ldy, int64_t dp, int d, int64_t row0, int64_t m,
    int64_t n, const dsvgd_select_state* __restrict__ st, float* __restrict__ rows,
    double* __restrict__ ws, float beta = 0.f) {
  __shared__ float xi[kKsdDirectMaxD * 64], si[kKsdDirectMaxD * 64];            // [c][r]
  __shared__ float xj[kKsdDirectJ * kKsdDirectMaxD], sj[kKsdDirectJ * kKsdDirectMaxD];  // [jj][c]
  __shared__ double part[4][64];
  const int t = threadIdx.x, r = t & 63, g = t >> 6;
  const int64_t ib = (int64_t)blockIdx.x * kKsdRowsPerBlock, i = ib + r;
  for (int e = t; e < 64 * d; e += 256) {
    const int c = e >> 6, rr = e & 63;
    const bool ok = ib + rr < m;
    const float* y = Y + (row0 + ib + rr) * ldy;
    xi[c * 64 + rr] = ok ? y[c] : 0.f;
    si[c * 64 + rr] = ok ? y[dp + c] : 0.f;
  }
  const float ihf = st->inv_h;
  const float scale = -ihf * kLog2e;
  // RBF: gg = 2/h; IMQ: c1, and c2 where the RBF has gg^2
  const double gg = FAM == kFamIMQ ? -2.0 * (double)beta * (double)ihf : 2.0 * (double)ihf;
  const double cst = gg * (double)d;
  const double c2 = 4.0 * (double)beta * ((double)beta - 1.0) * (double)ihf * (double)ihf;
  double acc = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += kKsdDirectJ) {
    __syncthreads();
    for (int e = t; e < kKsdDirectJ * d; e += 256) {
      const int jj = e / d, c = e - jj * d;
      const bool ok = j0 + jj < n;
      const float* y = Y + (j0 + jj) * ldy;
      xj[jj * kKsdDirectMaxD + c] = ok ? y[c] : 0.f;
      sj[jj * kKsdDirectMaxD + c] = ok ? y[dp + c] : 0.f;
    }
    __syncthreads();
    for (int jj = g; jj < kKsdDirectJ; jj += 4) {
      const int64_t j = j0 + jj;
      if (j >= n) break;
      float Dij = 0.f, ssum = 0.f, sd = 0.f;
      for (int c = 0; c < d; ++c) {
        const float x = xi[c * 64 + r], s = si[c * 64 + r];
        const float xo = xj[jj * kKsdDirectMaxD + c], so = sj[jj * kKsdDirectMaxD + c];
        const float dx = x - xo;
        Dij = fmaf(dx, dx, Dij);
        ssum = fmaf(s, so, ssum);
        sd = fmaf(s - so, dx, sd);
      }
      double u;
      if constexpr (FAM == kFamIMQ) {
        const float lg = __builtin_amdgcn_logf(fmaf(Dij, ihf, 1.f));
        const float f = __builtin_amdgcn_exp2f(beta * lg);
        const float gp = __builtin_amdgcn_exp2f((beta - 1.f) * lg);
        const float hp = __builtin_amdgcn_exp2f((beta - 2.f) * lg);
        u = (double)f * (double)ssum + (double)gp * (gg * (double)sd + cst) -
            c2 * (double)hp * (double)Dij;
      } else {
        const float k = __builtin_amdgcn_exp2f(Dij * scale);
        u = (double)k * ((double)ssum + gg * (double)sd + cst - gg * gg * (double)Dij);
      }
      if (j != row0 + i) acc += u;
    }
  }
  part[g][r] = acc;
  __syncthreads();
  if (t < 64) {
    const bool ok = i < m;
    const double ti = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    double ss = 0.0;
    for (int c = 0; c < d; ++c) ss += (double)si[c * 64 + t] * (double)si[c * 64 + t];
    if (ok && rows) rows[i] = (float)ti;
    const double st_ = wave_sum_f64(ok ? ti : 0.0);
    const double su = wave_sum_f64(ok ? ss + cst : 0.0);
    if (t == 0) {
      ws[2 * (int64_t)blockIdx.x] = st_;
      ws[2 * (int64_t)blockIdx.x + 1] = su;
    }
  }
}

static int64_t ksd_row_parts(int64_t tiles, int64_t cap) {
  return std::max<int64_t>(1, std::min<int64_t>((kKsdBlockTarget + tiles - 1) / tiles, cap));
}

static bool a16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int64_t dsvgd_ksd_parts(int64_t m, int64_t n, int sym) {
  if (m <= 0 || n <= 0) return 0;
  const int64_t n_pad = roundup(n, 128), m_pad = roundup(m, 128);
  if (sym) {
    const int64_t T = n_pad / 128;
    return ksd_row_parts(T, T) + T;
  }
  // at least eight panels (128 columns) per slice
  return ksd_row_parts(m_pad / 128, n_pad / 128);
}

size_t dsvgd_ksd_workspace_doubles(int64_t m) {
  return m > 0 ? 2 * (size_t)((m + kKsdRowsPerBlock - 1) / kKsdRowsPerBlock) : 0;
}

int dsvgd_ksd_gate(const float* rowsum, int64_t splits, int64_t m, int64_t n, float* gate,
                   void* stream) {
  DSVGD_REQUIRE(rowsum && gate, "null pointer");
  DSVGD_REQUIRE(m > 0 && n >= m, "sizes");
  DSVGD_REQUIRE(splits >= 1 && splits <= 1024, "splits must be in [1, 1024]");
  const float tau = (float)((double)n * 0x1p-20);
  hipLaunchKernelGGL(ksd_gate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rowsum,
                     (int)splits, m, roundup(m, 128), n, tau, gate);
  return check_launch("ksd_gate");
}

int dsvgd_ksd_rows(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t dp, int64_t d,
                   int64_t row0, int64_t m, int64_t n, const dsvgd_select_state* st, int sym,
                   int64_t parts, float* P, float* a, void* stream) {
  return dsvgd_ksd_rows_kern(D, ldd, Y, ldy, dp, d, row0, m, n, st, sym, parts, P, a, kRbfKern,
                             stream);
}

int dsvgd_ksd_rows_kern(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t dp,
                        int64_t d, int64_t row0, int64_t m, int64_t n,
                        const dsvgd_select_state* st, int sym, int64_t parts, float* P, float* a,
                        dsvgd_kernel kern, void* stream) {
  DSVGD_REQUIRE(kern_ok(kern), "kern: family RBF, or IMQ with beta in [-1, 0)");
  const bool imq = kern.family == DSVGD_KERNEL_IMQ;
  const float pw = kern.beta - 1.f;   // IMQ: the sweep's matrix is G' = u^(beta-1)
  DSVGD_REQUIRE(D && Y && st && P && a, "null pointer");
  DSVGD_REQUIRE(m > 0 && n > 0 && d > 0 && row0 >= 0 && row0 + m <= n, "sizes");
  const int64_t n_pad = roundup(n, 128), m_pad = roundup(m, 128);
  DSVGD_REQUIRE(ldd == n_pad, "ldd must equal roundup(n,128) (panel layout)");
  DSVGD_REQUIRE(dp >= d && ldy >= 2 * dp, "dp >= d and ldy >= 2 dp");
  DSVGD_REQUIRE(a16(D) && a16(a), "D and a must be 16-byte aligned");
  DSVGD_REQUIRE(!sym || (m == n && row0 == 0), "sym needs m == n and row0 == 0");
  DSVGD_REQUIRE(parts == dsvgd_ksd_parts(m, n, sym), "parts must be dsvgd_ksd_parts(m, n, sym)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ksd_a_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, s, Y, ldy, dp, d, n,
                     n_pad, a);
  int rc = check_launch("ksd_a");
  if (rc) return rc;
  if (sym) {
    const int64_t T = n_pad / 128, rparts = parts - T;
    if (imq)
      hipLaunchKernelGGL(ksd_rows_sym_kernel<kFamIMQ>, dim3((unsigned)T, (unsigned)rparts),
                         dim3(256), 0, s, D, n_pad, a, n, st, (int)rparts, P, pw);
    else
      hipLaunchKernelGGL(ksd_rows_sym_kernel<kFamRBF>, dim3((unsigned)T, (unsigned)rparts),
                         dim3(256), 0, s, D, n_pad, a, n, st, (int)rparts, P, 0.f);
    return check_launch("ksd_rows_sym");
  }
  const dim3 grid((unsigned)(m_pad / 128), (unsigned)parts);
  if (imq)
    hipLaunchKernelGGL(ksd_rows_full_kernel<kFamIMQ>, grid, dim3(256), 0, s, D, n_pad, a, row0, m,
                       n, st, (int)parts, P, m_pad, pw);
  else
    hipLaunchKernelGGL(ksd_rows_full_kernel<kFamRBF>, grid, dim3(256), 0, s, D, n_pad, a, row0, m,
                       n, st, (int)parts, P, m_pad, 0.f);
  return check_launch("ksd_rows_full");
}

int dsvgd_ksd_finish(const float* KY, int64_t ldk, const float* rowsum, int64_t splits,
                     const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0, int64_t m,
                     int64_t n, const dsvgd_select_state* st, int sym, int64_t parts,
                     const float* P, float* rows, double* ws, double* out, void* stream) {
  DSVGD_REQUIRE(KY && rowsum && Y && st && P && ws && out, "null pointer");
  DSVGD_REQUIRE(m > 0 && n > 0 && d > 0 && row0 >= 0 && row0 + m <= n, "sizes");
  DSVGD_REQUIRE(splits >= 1 && splits <= 1024, "splits must be in [1, 1024]");
  DSVGD_REQUIRE(dp >= d && ldk >= 2 * dp && ldy >= 2 * dp, "dp >= d, ldk >= 2 dp, ldy >= 2 dp");
  DSVGD_REQUIRE(!sym || (m == n && row0 == 0), "sym needs m == n and row0 == 0");
  DSVGD_REQUIRE(parts == dsvgd_ksd_parts(m, n, sym), "parts must be dsvgd_ksd_parts(m, n, sym)");
  DSVGD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0,
                "ws and out must be 8-byte aligned");
  const int64_t m_pad = roundup(m, 128);
  const int64_t nb = (m + kKsdRowsPerBlock - 1) / kKsdRowsPerBlock;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ksd_finish_kernel<kFamRBF>, dim3((unsigned)nb), dim3(256), 0, s, KY, ldk,
                     rowsum, (int)splits, Y, ldy, dp, d, row0, m, m_pad, st, sym ? 1 : 0,
                     (int)parts, P, rows, ws);
  int rc = check_launch("ksd_finish");
  if (rc) return rc;
  hipLaunchKernelGGL(ksd_reduce_kernel, dim3(1), dim3(256), 0, s, ws, nb, n, out);
  return check_launch("ksd_reduce");
}

int dsvgd_ksd_finish_imq(const float* KF, int64_t ldkf, const float* KG, int64_t ldkg,
                         const float* rowsum, int64_t splits, const float* Y, int64_t ldy,
                         int64_t dp, int64_t d, int64_t row0, int64_t m, int64_t n,
                         const dsvgd_select_state* st, dsvgd_kernel kern, int sym, int64_t parts,
                         const float* P, float* rows, double* ws, double* out, void* stream) {
  DSVGD_REQUIRE(KF && KG && rowsum && Y && st && P && ws && out, "null pointer");
  DSVGD_REQUIRE(kern.family == DSVGD_KERNEL_IMQ && kern_ok(kern),
                "kern: the IMQ family with beta in [-1, 0)");
  DSVGD_REQUIRE(m > 0 && n > 0 && d > 0 && row0 >= 0 && row0 + m <= n, "sizes");
  DSVGD_REQUIRE(splits >= 1 && splits <= 1024, "splits must be in [1, 1024]");
  DSVGD_REQUIRE(dp >= d && ldkf >= 2 * dp && ldkg >= 2 * dp && ldy >= 2 * dp,
                "dp >= d, ldkf, ldkg, ldy >= 2 dp");
  DSVGD_REQUIRE(!sym || (m == n && row0 == 0), "sym needs m == n and row0 == 0");
  DSVGD_REQUIRE(parts == dsvgd_ksd_parts(m, n, sym), "parts must be dsvgd_ksd_parts(m, n, sym)");
  DSVGD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0,
                "ws and out must be 8-byte aligned");
  const int64_t m_pad = roundup(m, 128);
  const int64_t nb = (m + kKsdRowsPerBlock - 1) / kKsdRowsPerBlock;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ksd_finish_kernel<kFamIMQ>, dim3((unsigned)nb), dim3(256), 0, s, KF, ldkf,
                     rowsum, (int)splits, Y, ldy, dp, d, row0, m, m_pad, st, sym ? 1 : 0,
                     (int)parts, P, rows, ws, KsdImqArgs{KG, ldkg, kern.beta});
  int rc = check_launch("ksd_finish(imq)");
  if (rc) return rc;
  hipLaunchKernelGGL(ksd_reduce_kernel, dim3(1), dim3(256), 0, s, ws, nb, n, out);
  return check_launch("ksd_reduce");
}

int dsvgd_ksd_direct(const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0, int64_t m,
                     int64_t n, const dsvgd_select_state* st, float* rows, double* ws, double* out,
                     void* stream) {
  return dsvgd_ksd_direct_kern(Y, ldy, dp, d, row0, m, n, st, rows, ws, out, kRbfKern, stream);
}

int dsvgd_ksd_direct_kern(const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0,
                          int64_t m, int64_t n, const dsvgd_select_state* st, float* rows,
                          double* ws, double* out, dsvgd_kernel kern, void* stream) {
  DSVGD_REQUIRE(kern_ok(kern), "kern: family RBF, or IMQ with beta in [-1, 0)");
  DSVGD_REQUIRE(Y && st && ws && out, "null pointer");
  DSVGD_REQUIRE(m > 0 && n > 0 && d > 0 && row0 >= 0 && row0 + m <= n, "sizes");
  DSVGD_REQUIRE(d <= kKsdDirectMaxD, "ksd_direct supports d <= 64");
  DSVGD_REQUIRE(dp >= d && ldy >= 2 * dp, "dp >= d and ldy >= 2 dp");
  DSVGD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0,
                "ws and out must be 8-byte aligned");
  const int64_t nb = (m + kKsdRowsPerBlock - 1) / kKsdRowsPerBlock;
  hipStream_t s = (hipStream_t)stream;
  if (kern.family == DSVGD_KERNEL_IMQ)
    hipLaunchKernelGGL(ksd_direct_kernel<kFamIMQ>, dim3((unsigned)nb), dim3(256), 0, s, Y, ldy, dp,
                       (int)d, row0, m, n, st, rows, ws, kern.beta);
  else
    hipLaunchKernelGGL(ksd_direct_kernel<kFamRBF>, dim3((unsigned)nb), dim3(256), 0, s, Y, ldy, dp,
                       (int)d, row0, m, n, st, rows, ws, 0.f);
  int rc = check_launch("ksd_direct");
  if (rc) return rc;
  hipLaunchKernelGGL(ksd_reduce_kernel, dim3(1), dim3(256), 0, s, ws, nb, n, out);
  return check_launch("ksd_reduce");
}

}  // extern "C"
