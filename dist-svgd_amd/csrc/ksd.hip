// ksd.hip -- the kernelized Stein discrepancy of the particles of one Jacobi
// step, from what the step left on the device ("KSD diagnostic").
//
// For k = exp(-|x - y|^2 / h) the Stein kernel is
//   u_ij = k_ij [ s_i.s_j + (2/h)(s_i - s_j).(x_i - x_j) + 2d/h - (4/h^2) D_ij ]
// and its off-diagonal row sum splits into pieces of the step:
//   t_i = s_i.KS_i + (2/h)[ r_i a_i - s_i.KXc_i - xc_i.KS_i + b_i ]
//         + (2d/h) r_i - (4/h^2) q_i,
//   a_j = s_j.xc_j,  b_i = sum_{j != i} k_ij a_j,  q_i = sum_{j != i} k_ij D_ij.
// KXc, KS, r are phi_mm's outputs; b and q are one sweep over D: the shared
// walker of dsweep.hpp with the payload below.
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
#include <cmath>

#include "dsweep.hpp"

namespace dsvgd {

constexpr int kKsdDirectMaxD = 64;
constexpr int kKsdDirectJ = 32;       // columns staged per chunk (direct form)

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

// The sweep's payload (dsweep.hpp): quantity 0 is q += k D, quantity 1 is
// b += k a_j, with a_j the panel's extra load; cv[0..3] = the two rows' k D
// per column, cv[4..7] = their k a_i (the transposed tile's terms, weights
// ai0, ai1 of the thread's rows).  Masked entries are exact zeros, not
// products: exp(-inf) inf is NaN.  FAM = IMQ: k -> G' = u^pw (pw = beta - 1,
// scale = 1/h) and k D -> H' D = u^(pw-1) D.
template <int FAM>
struct KsdPayload {
  using extra = f32x4;
  const float* a;
  float scale, pw, ai0, ai1;
  __device__ KsdPayload(const float* a_, const dsvgd_select_state* st, float pw_)
      : a(a_), scale(FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e), pw(pw_), ai0(0.f),
        ai1(0.f) {}
  __device__ void rows(int64_t i0) {
    ai0 = a[i0];
    ai1 = a[i0 + 64];
  }
  __device__ f32x4 load(int64_t c, int cq) const {
    return *reinterpret_cast<const f32x4*>(a + 16 * c + 4 * cq);
  }
  __device__ bool edge(int64_t) const { return false; }

  template <bool MASK, bool COLS>
  __device__ __forceinline__ void panel(const f32x4 v0, const f32x4 v1, const f32x4 a4, int64_t,
                                        int64_t g0, int64_t j0, bool rv0, bool rv1, int64_t n,
                                        float& q0, float& b0, float& q1, float& b1,
                                        float* cv) const {
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
};

// The sweep in the full panel layout (sweep_full): P[z][0][i] = q, P[z][1][i]
// = b of column slice z, for the rows [row0, row0 + m) of a row block.
template <int FAM = kFamRBF>
__global__ __launch_bounds__(256) void ksd_rows_full_kernel(
    const float* __restrict__ D, int64_t n_pad, const float* __restrict__ a, int64_t row0,
    int64_t m, int64_t n, const dsvgd_select_state* __restrict__ st, int parts,
    float* __restrict__ P, int64_t m_pad, float pw = 0.f) {
  KsdPayload<FAM> pl(a, st, pw);
  sweep_full(D, SweepGeom<int64_t>{n_pad, row0, m, n, m_pad}, parts, P, pl);
}

// ... and in the symmetric layout (sweep_sym): the column sums carry the
// weights a_i of the stored rows.
template <int FAM = kFamRBF>
__global__ __launch_bounds__(256) void ksd_rows_sym_kernel(
    const float* __restrict__ D, int64_t n_pad, const float* __restrict__ a, int64_t n,
    const dsvgd_select_state* __restrict__ st, int rparts, float* __restrict__ P, float pw = 0.f) {
  KsdPayload<FAM> pl(a, st, pw);
  sweep_sym(D, n_pad, n, rparts, P, pl);
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

// t_i, u_ii for 64 rows per workgroup.  First the rows' q and b from the
// sweep's slots (slot_sums).  Then one wave per row: the split-K slices summed
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
  const int64_t ib = (int64_t)blockIdx.x * kSweepRowsPerBlock;
  slot_sums(P, m_pad, m, ib, sym, parts, shq, shb);
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
    const double q = sum4(shq, rr), b = sum4(shb, rr);
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

// the second level (block_totals); out = [off, diag, V, U]
__global__ __launch_bounds__(256) void ksd_reduce_kernel(const double* __restrict__ ws, int64_t nb,
                                                         int64_t n, double* __restrict__ out) {
  double tot[2];
  block_totals<2>(ws, nb, tot);
  if (threadIdx.x == 0) {
    const double off = tot[0], diag = tot[1], nn = (double)n;
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
  const int64_t ib = (int64_t)blockIdx.x * kSweepRowsPerBlock, i = ib + r;
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

static bool a16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int64_t dsvgd_ksd_parts(int64_t m, int64_t n, int sym) {
  if (m <= 0 || n <= 0) return 0;
  const int64_t n_pad = roundup(n, 128), m_pad = roundup(m, 128);
  if (sym) {
    const int64_t T = n_pad / 128;
    return row_parts(T, T) + T;
  }
  // at least eight panels (128 columns) per slice
  return row_parts(m_pad / 128, n_pad / 128);
}

size_t dsvgd_ksd_workspace_doubles(int64_t m) {
  return m > 0 ? 2 * (size_t)((m + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock) : 0;
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
  const int64_t nb = (m + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock;
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
  const int64_t nb = (m + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock;
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
  const int64_t nb = (m + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock;
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
