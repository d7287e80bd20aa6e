// mmd.hip -- the maximum mean discrepancy between two particle sets P (the
// first nf rows) and Q (the rest) of one pooled, packed set of n particles,
// from the distance matrix D the engine already holds ("MMD
// two-sample diagnostic").
//
// With k = exp(-D/h), or (1 + D/h)^beta for the inverse multiquadric,
//   rP_i = sum_{j < nf, j != i} k_ij,   rQ_i = sum_{j >= nf, j != i} k_ij
// are one sweep over D (the row sums of K split at column nf): the shared
// walker of dsweep.hpp with the payload below.  The finish forms PP =
// sum_{i < nf} rP_i, PQ = sum_{i < nf} rQ_i, QQ = sum_{i >= nf} rQ_i in fp64,
// the V- and U-statistics and the witness
//   w_i = (rP_i + [i < nf]) / nf - (rQ_i + [i >= nf]) / (n - nf).
// The diagonal is never read (the Gram form does not give D_ii = 0 exactly):
// its terms k_ii = 1 enter as exact constants.
//
// Everything is deterministic: no float atomics, every partial has a slot of
// its own and every sum a fixed order.
#include <cmath>

#include "dsweep.hpp"

namespace dsvgd {

// The sweep's payload (dsweep.hpp): quantity 0 is rP, quantity 1 is rQ.
// Inside one class (EDGE = false; 16 c < nf: the panel's columns are all
// < nf) the four kernel values of a row are added, then sent to rP or rQ; a
// panel that the class boundary cuts is an edge, where every column picks its
// own class.  cv[0..3] = the two rows' values per column that belong to rP
// of the transposed entry (the stored row is < nf: pr0 / pr1), cv[4..7] =
// those that belong to rQ -- a tile row that straddles nf feeds both.
template <int FAM>
struct MmdPayload {
  struct extra {};
  float scale, beta;
  int nf;
  bool pr0, pr1;
  __device__ MmdPayload(const dsvgd_select_state* st, float beta_, int nf_)
      : scale(FAM == kFamIMQ ? st->inv_h : -st->inv_h * kLog2e), beta(beta_), nf(nf_), pr0(false),
        pr1(false) {}
  __device__ void rows(int i0) {
    pr0 = i0 < nf;
    pr1 = i0 + 64 < nf;
  }
  __device__ extra load(int, int) const { return {}; }
  __device__ bool edge(int c) const { return 16 * c < nf && 16 * c + 16 > nf; }
  __device__ __forceinline__ float k(float v) const {
    if constexpr (FAM == kFamIMQ)
      return __builtin_amdgcn_exp2f(beta * __builtin_amdgcn_logf(fmaf(v, scale, 1.f)));
    else
      return __builtin_amdgcn_exp2f(v * scale);
  }

  template <bool EDGE, bool COLS>
  __device__ __forceinline__ void panel(const f32x4 v0, const f32x4 v1, extra, int c, int g0,
                                        int j0, bool rv0, bool rv1, int n, float& p0, float& q0,
                                        float& p1, float& q1, float* cv) const {
    const bool pcls = 16 * c < nf;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float k0 = k(v0[e]);
      float k1 = k(v1[e]);
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
};

// The sweep in the full panel layout (sweep_full): P[z][0][i] = rP, P[z][1][i]
// = rQ of column slice z.
template <int FAM>
__global__ __launch_bounds__(256) void mmd_rows_full_kernel(
    const float* __restrict__ D, int n_pad, int n, int nf,
    const dsvgd_select_state* __restrict__ st, int parts, float* __restrict__ P, float beta) {
  MmdPayload<FAM> pl(st, beta, nf);
  sweep_full(D, SweepGeom<int>{n_pad, 0, n, n, n_pad}, parts, P, pl);
}

// ... and in the symmetric layout (sweep_sym): k_ji goes to rP_j where the
// stored row i < nf and to rQ_j otherwise.
template <int FAM>
__global__ __launch_bounds__(256) void mmd_rows_sym_kernel(
    const float* __restrict__ D, int n_pad, int n, int nf,
    const dsvgd_select_state* __restrict__ st, int rparts, float* __restrict__ P, float beta) {
  MmdPayload<FAM> pl(st, beta, nf);
  sweep_sym(D, n_pad, n, rparts, P, pl);
}

// rP_i, rQ_i from the sweep's slots (slot_sums) and the witness for 64 rows
// per workgroup.  ws[3 blk + 0..2] = the workgroup's shares of PP, PQ, QQ in
// row order.
__global__ __launch_bounds__(256) void mmd_finish_kernel(const float* __restrict__ P, int n_pad,
                                                         int n, int nf, int sym, int parts,
                                                         float* __restrict__ rp,
                                                         float* __restrict__ rq,
                                                         float* __restrict__ witness,
                                                         double* __restrict__ ws) {
  __shared__ double shp[4][64], shq[4][64];
  const int t = threadIdx.x;
  const int ib = blockIdx.x * kSweepRowsPerBlock;
  const int i = ib + (t & 63);
  slot_sums(P, n_pad, n, ib, sym, parts, shp, shq);
  if (t < 64) {
    const bool ok = i < n, first = i < nf;
    const double p = sum4(shp, t), q = sum4(shq, t);
    if (ok) {
      if (rp) rp[i] = (float)p;
      if (rq) rq[i] = (float)q;
      if (witness)
        witness[i] = (float)((p + (first ? 1.0 : 0.0)) / (double)nf -
                             (q + (first ? 0.0 : 1.0)) / (double)(n - nf));
    }
    const double pp = wave_sum_f64(ok && first ? p : 0.0);
    const double pq = wave_sum_f64(ok && first ? q : 0.0);
    const double qq = wave_sum_f64(ok && !first ? q : 0.0);
    if (t == 0) {
      double* w = ws + 3 * (int64_t)blockIdx.x;
      w[0] = pp;
      w[1] = pq;
      w[2] = qq;
    }
  }
}

// the second level (block_totals); out = [PP, PQ, QQ, V, U]
__global__ __launch_bounds__(256) void mmd_reduce_kernel(const double* __restrict__ ws, int nb,
                                                         int n, int nf, double* __restrict__ out) {
  double tot[3];
  block_totals<3>(ws, nb, tot);
  if (threadIdx.x == 0) {
    const double pp = tot[0], pq = tot[1], qq = tot[2];
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
  const int64_t rparts = force > 0 ? std::min<int64_t>(force, T) : row_parts(T, T);
  return sym ? rparts + T : rparts;
}

size_t dsvgd_mmd_workspace_doubles(int64_t n_total) {
  return n_total > 0 ? 3 * (size_t)((n_total + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock) : 0;
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
  const int64_t nb = (n_total + kSweepRowsPerBlock - 1) / kSweepRowsPerBlock;
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
