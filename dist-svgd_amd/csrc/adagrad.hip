// adagrad.hip -- the AdaGrad-conditioned particle update of the Jacobi order
// (Liu & Wang's SVGD code: a moving average of the squared direction per
// entry of the moved rows).
//
//   G' = p^2                             where G < 0 (no history yet)
//   G' = alpha G + (1 - alpha) p^2       elsewhere
//   x += step p / (eps + sqrt(G'))
//
// p is the whole direction (phi, with the h * W2 rows already added by the
// finish kernels).  The first step is flagged in the data, not by a counter:
// a history entry below 0 cannot come out of the rule, the state starts
// filled with -1, and so a captured iteration replays correctly and a step
// depends on its inputs alone.  One thread per entry (or per four entries
// where d, the leading dimensions and the pointers allow 16-byte accesses);
// IEEE square root and division, so that the chain is eight roundings.
#include "common.hpp"

namespace dsvgd {

constexpr int kAdaThreads = 256;

__device__ __forceinline__ void adagrad_entry(float& x, float p, float& g, float step, float alpha,
                                              float beta, float eps) {
  const float p2 = __fmul_rn(p, p);
  const float gn = g < 0.f ? p2 : __fmaf_rn(alpha, g, __fmul_rn(beta, p2));
  const float den = __fadd_rn(eps, __fsqrt_rn(gn));
  const float q = __fdiv_rn(p, den);
  x = __fadd_rn(x, __fmul_rn(step, q));
  g = gn;
}

__global__ __launch_bounds__(kAdaThreads) void adagrad_kernel(
    float* __restrict__ X, int64_t ldx, const float* __restrict__ P, int64_t ldp,
    float* __restrict__ G, int64_t ldg, int64_t m, int d, float step, float alpha, float beta,
    float eps) {
  const int64_t e = (int64_t)blockIdx.x * kAdaThreads + threadIdx.x;
  if (e >= m * d) return;
  const int64_t i = e / d;
  const int c = (int)(e - i * d);
  float x = X[i * ldx + c], g = G[i * ldg + c];
  adagrad_entry(x, P[i * ldp + c], g, step, alpha, beta, eps);
  X[i * ldx + c] = x;
  G[i * ldg + c] = g;
}

// d % 4 == 0, every leading dimension % 4 == 0, 16-byte aligned pointers
__global__ __launch_bounds__(kAdaThreads) void adagrad_kernel_v4(
    float* __restrict__ X, int64_t ldx, const float* __restrict__ P, int64_t ldp,
    float* __restrict__ G, int64_t ldg, int64_t m, int dq, float step, float alpha, float beta,
    float eps) {
  const int64_t e = (int64_t)blockIdx.x * kAdaThreads + threadIdx.x;
  if (e >= m * dq) return;
  const int64_t i = e / dq;
  const int c = 4 * (int)(e - i * dq);
  f32x4 x = *reinterpret_cast<const f32x4*>(X + i * ldx + c);
  f32x4 g = *reinterpret_cast<const f32x4*>(G + i * ldg + c);
  const f32x4 p = *reinterpret_cast<const f32x4*>(P + i * ldp + c);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float xk = x[k], gk = g[k];
    adagrad_entry(xk, p[k], gk, step, alpha, beta, eps);
    x[k] = xk;
    g[k] = gk;
  }
  *reinterpret_cast<f32x4*>(X + i * ldx + c) = x;
  *reinterpret_cast<f32x4*>(G + i * ldg + c) = g;
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int dsvgd_adagrad_step(float* X, int64_t ldx, const float* phi, int64_t ldphi, float* G,
                       int64_t ldg, int64_t m, int64_t d, float step, float alpha, float eps,
                       void* stream) {
  DSVGD_REQUIRE(X && phi && G, "null pointer");
  DSVGD_REQUIRE(m > 0 && d > 0 && d <= 0x7fffffff, "adagrad: m, d > 0");
  DSVGD_REQUIRE(ldx >= d && ldphi >= d && ldg >= d, "adagrad: ldx, ldphi, ldg >= d");
  DSVGD_REQUIRE(alpha >= 0.f && alpha < 1.f, "adagrad: 0 <= alpha < 1");
  DSVGD_REQUIRE(eps > 0.f, "adagrad: eps > 0");
  auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool v4 = d % 4 == 0 && ldx % 4 == 0 && ldphi % 4 == 0 && ldg % 4 == 0 && a16(X) &&
                  a16(phi) && a16(G);
  const int64_t work = v4 ? m * (d / 4) : m * d;
  const int64_t blocks = (work + kAdaThreads - 1) / kAdaThreads;
  DSVGD_REQUIRE(blocks <= 0x7fffffff, "adagrad: m d too large for one launch");
  const float beta = 1.f - alpha;
  if (v4)
    hipLaunchKernelGGL(adagrad_kernel_v4, dim3((unsigned)blocks), dim3(kAdaThreads), 0,
                       (hipStream_t)stream, X, ldx, phi, ldphi, G, ldg, m, (int)(d / 4), step,
                       alpha, beta, eps);
  else
    hipLaunchKernelGGL(adagrad_kernel, dim3((unsigned)blocks), dim3(kAdaThreads), 0,
                       (hipStream_t)stream, X, ldx, phi, ldphi, G, ldg, m, (int)d, step, alpha,
                       beta, eps);
  return check_launch("adagrad_step");
}

}  // extern "C"
