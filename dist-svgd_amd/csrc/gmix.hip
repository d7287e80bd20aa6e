// gmix.hip -- the d-dimensional Gaussian-mixture target with diagonal
// precisions: its score and its evaluation twin (log density and most
// responsible component), in exact fp32 on the VALU.
//
//   p(x) = sum_k w~_k N(x; mu_k, diag(1/lam_k)),  c_k = log w~_k + 1/2 sum_c log lam_kc
//   q_ik = 1/2 sum_c lam_kc (x_ic - mu_kc)^2,  l_ik = c_k - q_ik,  r_ik = softmax_k(l_ik)
//   S_ic = sum_k r_ik lam_kc (mu_kc - x_ic),  log p(x_i) = logsumexp_k l_ik - d/2 log 2 pi
//
// A particle belongs to G = 2^lg lanes of one wave; lane g keeps R of its
// coordinates in registers, in 16-byte pieces: c = 4 (g + G j) + u, j < R / 4,
// u < 4 (x, the running sum of the score and the terms of the two components
// in flight: 4 R registers).  R = 4 for d <= 8, else 16; G is the least power of
// two with R G >= d, so a workgroup of 256 threads holds P = 256 / G particles
// and d <= 1024.  The components go by in ascending order in tiles of TK (mu,
// lam and c in LDS, 2 TK R G <= 8192 floats, shared by the P particles; four
// workgroups fit a CU, so one stages while the others compute).
//
// Per component, in the difference form (the expanded form cancels near a
// mode, where the score matters): t_c = lam_c (mu_c - x_c), q = sum t_c (mu_c
// - x_c) -- four running sums per lane, one per u, added as (0 + 1) + (2 + 3),
// then a butterfly over the G lanes -- and one step of the online softmax:
// with m the running maximum, one exponential exp(-|l - m|) rescales either
// the sums (a new maximum) or the term, so no exponent is ever taken without
// its maximum and K is unbounded.  No atomics, a fixed order over k and a
// fixed tree over c: the same bits on every call, and a particle's result
// depends neither on n, nor on its row, nor on the particles beside it.
#include "common.hpp"

namespace dsvgd {

constexpr int kGmixThreads = 256;
constexpr int kGmixMaxD = 1024;       // 16 coordinates x 64 lanes
constexpr int64_t kGmixMaxK = 1 << 30;  // the component index is an int
constexpr int kGmixTile = 4096;       // floats of mu (and of lam) per tile
constexpr int kGmixMaxTK = 32;        // components per tile at most
constexpr int kGmixStage = kGmixTile / kGmixThreads;  // tile elements per thread
constexpr int kGmixPair = 2;          // components in flight per lane

struct GmixShape {
  int R, lg, tk;  // coordinates per lane, log2 of the lanes per particle, components per tile
};

inline GmixShape gmix_shape(int d) {
  GmixShape s;
  s.R = d <= 8 ? 4 : 16;
  s.lg = 0;
  while ((s.R << s.lg) < d) ++s.lg;
  const int dpad = s.R << s.lg;
  s.tk = kGmixTile / dpad < kGmixMaxTK ? kGmixTile / dpad : kGmixMaxTK;
  return s;
}

// Components kk .. kk + NB - 1 of the tile in LDS (mrow, lrow: the lane's
// first piece of component 0) for one lane: the terms t_c = lam_c (mu_c - x_c)
// and q of each, then one step of the online softmax per component, in order.
template <int R, int NB, bool kAssign>
__device__ __forceinline__ void gmix_step(const float* mrow, const float* lrow, const float* cs,
                                          int kk, int k0, int lg, int lgd, const float (&x)[R],
                                          float (&acc)[R], float& m, float& den, float& best,
                                          int& arg) {
  constexpr int RQ = R / 4;
  float t[NB][R], q[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float qs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      const int at = ((kk + b) << lgd) + 4 * (j << lg);
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(mrow + at);
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lrow + at);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float df = m4[u] - x[4 * j + u];
        t[b][4 * j + u] = l4[u] * df;
        qs[u] = fmaf(t[b][4 * j + u], df, qs[u]);
      }
    }
    q[b] = (qs[0] + qs[1]) + (qs[2] + qs[3]);
  }
  for (int o = (1 << lg) >> 1; o > 0; o >>= 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b) q[b] += __shfl_xor(q[b], o, 64);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const float l = fmaf(-0.5f, q[b], cs[kk + b]);
    if (kAssign && l > best) {
      best = l;
      arg = k0 + kk + b;
    }
    // one exponential: of m - l on a new maximum (the sums shrink), of
    // l - m otherwise (the term does)
    const float dl = l - m;
    const float ex = expf(-fabsf(dl));
    const bool up = dl > 0.f;
    const float sc = up ? ex : 1.f, e = up ? 1.f : ex;
    m = up ? l : m;
    den = fmaf(den, sc, e);
    if (!kAssign) {
#pragma unroll
      for (int i = 0; i < R; ++i) acc[i] = fmaf(acc[i], sc, e * t[b][i]);
    }
  }
}

// kAssign: logp_out[i] = log p(x_i) and comp_out[i] = argmax_k l_ik (the
// lowest index on a tie; scale, S and lds unused); otherwise S[i] = scale *
// grad log p(x_i).
template <int R, bool kAssign>
__global__ __launch_bounds__(kGmixThreads) void gmix_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t n, int d, const float* __restrict__ mu,
    int64_t ldm, const float* __restrict__ lam, int64_t ldl, const float* __restrict__ cw, int K,
    int lg, int TK, float scale, float* __restrict__ S, int64_t lds, float* __restrict__ logp_out,
    int* __restrict__ comp_out) {
  constexpr int RQ = R / 4;
  constexpr int lgR = R == 4 ? 2 : 4;
  __shared__ __align__(16) float mus[kGmixTile];
  __shared__ __align__(16) float lams[kGmixTile];
  __shared__ float cs[kGmixMaxTK];
  const int tid = threadIdx.x;
  const int G = 1 << lg, lgd = lg + lgR, dpad = 1 << lgd;
  const int g = tid & (G - 1);
  const int64_t row = (int64_t)blockIdx.x * (kGmixThreads >> lg) + (tid >> lg);
  const bool live = row < n;
  const int tile = TK << lgd;  // <= kGmixTile

  float x[R], acc[R];
#pragma unroll
  for (int j = 0; j < RQ; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 4 * (g + (j << lg)) + u;
      x[4 * j + u] = (live && c < d) ? X[row * ldx + c] : 0.f;
      acc[4 * j + u] = 0.f;
    }
  float m = -3.402823466e38f, den = 0.f, best = -INFINITY;
  int arg = 0;

  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();  // the tile before this one has been used
    // the tile that starts at component k0, element tid + 256 u of it: zero
    // past d and past K (a padded coordinate adds 0 to q and gets no score).
    // Eight loads in flight, then their stores: every load reads an address
    // inside the arrays (the indices are clamped), so none waits on a branch.
    const int klast = K - k0 - 1;
#pragma unroll 1
    for (int u0 = 0; u0 < kGmixStage && tid + kGmixThreads * u0 < tile; u0 += 4) {
      float vm[4], vl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + kGmixThreads * (u0 + u);
        const int kk = e >> lgd, c = e & (dpad - 1);
        const int kr = k0 + (kk < klast ? kk : klast), cr = c < d ? c : d - 1;
        const bool in = c < d && kk <= klast;
        const float a = mu[(int64_t)kr * ldm + cr], b = lam[(int64_t)kr * ldl + cr];
        vm[u] = in ? a : 0.f;
        vl[u] = in ? b : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + kGmixThreads * (u0 + u);
        if (e < tile) {
          mus[e] = vm[u];
          lams[e] = vl[u];
        }
      }
    }
    if (tid < TK) cs[tid] = tid < K - k0 ? cw[k0 + tid] : 0.f;
    __syncthreads();

    // kGmixPair components at a time (their reads, sums and butterflies are
    // independent: latency), then a last odd one; each component's own
    // arithmetic, and the order of the updates, are the same either way
    const int tk = K - k0 < TK ? K - k0 : TK;
    int kk = 0;
    for (; kk + kGmixPair <= tk; kk += kGmixPair)
      gmix_step<R, kGmixPair, kAssign>(mus + 4 * g, lams + 4 * g, cs, kk, k0, lg, lgd, x, acc, m,
                                       den, best, arg);
    for (; kk < tk; ++kk)
      gmix_step<R, 1, kAssign>(mus + 4 * g, lams + 4 * g, cs, kk, k0, lg, lgd, x, acc, m, den,
                               best, arg);
  }

  if (kAssign) {
    if (live && g == 0) {
      logp_out[row] = (m + logf(den)) - 0.9189385332046727f * (float)d;
      comp_out[row] = arg;
    }
    return;
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < RQ; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 4 * (g + (j << lg)) + u;
      if (c < d) S[row * lds + c] = scale * (acc[4 * j + u] / den);
    }
}

template <bool kAssign>
static int gmix_launch(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                       int64_t ldm, const float* lam, int64_t ldl, const float* c, int64_t K,
                       float scale, float* S, int64_t lds, float* logp_out, int* comp_out,
                       void* stream) {
  const GmixShape s = gmix_shape((int)d);
  const int P = kGmixThreads >> s.lg;
  const dim3 grid((unsigned)((n + P - 1) / P)), block(kGmixThreads);
  if (s.R == 4)
    hipLaunchKernelGGL((gmix_kernel<4, kAssign>), grid, block, 0, (hipStream_t)stream, X, ldx, n,
                       (int)d, mu, ldm, lam, ldl, c, (int)K, s.lg, s.tk, scale, S, lds, logp_out,
                       comp_out);
  else
    hipLaunchKernelGGL((gmix_kernel<16, kAssign>), grid, block, 0, (hipStream_t)stream, X, ldx, n,
                       (int)d, mu, ldm, lam, ldl, c, (int)K, s.lg, s.tk, scale, S, lds, logp_out,
                       comp_out);
  return check_launch(kAssign ? "gmix_assign" : "score_gmix");
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int dsvgd_score_gmix(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                     int64_t ldm, const float* lam, int64_t ldl, const float* c, int64_t K,
                     float scale, float* S, int64_t lds, void* stream) {
  DSVGD_REQUIRE(X && mu && lam && c && S, "null pointer");
  DSVGD_REQUIRE(d >= 1 && d <= kGmixMaxD, "gmix: 1 <= d <= 1024");
  DSVGD_REQUIRE(K >= 1 && K <= kGmixMaxK, "gmix: 1 <= K <= 2^30");
  DSVGD_REQUIRE(n > 0 && n <= 0x7fffffff && ldx >= d && lds >= d && ldm >= d && ldl >= d, "sizes");
  return gmix_launch<false>(X, ldx, n, d, mu, ldm, lam, ldl, c, K, scale, S, lds, nullptr, nullptr,
                            stream);
}

int dsvgd_gmix_assign(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                      int64_t ldm, const float* lam, int64_t ldl, const float* c, int64_t K,
                      float* logp_out, int32_t* comp_out, void* stream) {
  DSVGD_REQUIRE(X && mu && lam && c && logp_out && comp_out, "null pointer");
  DSVGD_REQUIRE(d >= 1 && d <= kGmixMaxD, "gmix: 1 <= d <= 1024");
  DSVGD_REQUIRE(K >= 1 && K <= kGmixMaxK, "gmix: 1 <= K <= 2^30");
  DSVGD_REQUIRE(n > 0 && n <= 0x7fffffff && ldx >= d && ldm >= d && ldl >= d, "sizes");
  return gmix_launch<true>(X, ldx, n, d, mu, ldm, lam, ldl, c, K, 1.f, nullptr, 0, logp_out,
                           comp_out, stream);
}

}  // extern "C"
