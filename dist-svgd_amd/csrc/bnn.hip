// bnn.hip -- the Bayesian neural-network regression target (Liu & Wang's
// one-hidden-layer ReLU network with Gamma hyper-priors): its score and its
// predictions, in exact fp32 FMAs on the VALU.
//
//   x = [ vec(W1) (p x H row-major) | b1 (H) | w2 (H) | b2 | log g | log l ]
//   f(z) = w2 . relu(W1^T z + b1) + b2,  r_q = y_q - f(z_q),  th = x[:d-2]
//   log p = N/2 log g - g/2 sum r_q^2 + (d-2)/2 log l - l/2 |th|^2
//           + a0 log g - b0 g + a0 log l - b0 l
//
// One workgroup per particle.  Its weights sit in LDS; the data go by in
// chunks of 256 rows, re-read by every particle (from L2).  Per chunk:
//   stage : the chunk's rows z -> LDS (zero past N and past p)
//   P1    : one thread per row: a = W1^T z + b1 in blocks of 16 hidden units
//           (z as 16-byte reads, W1 as 16-byte broadcasts), relu(a) -> LDS,
//           f, r
//   P2    : thread (h, quarter): sum r relu(a) (d w2) and sum G (d b1) over a
//           quarter of the rows, G = r w2_h [a > 0] written over relu(a)
//   P4    : thread = a 4 x 4 tile of d W1: sum_q z_qk G_qh, one 16-byte read
//           of each per row; the tiles of a small net are spread over 2 or 4
//           row groups so that every wave has work
// The sums are kept in registers across the chunks and combined once, in a
// fixed order: no atomics, the same bits on every call, and a particle's
// score does not depend on n or on its row.
#include "common.hpp"

namespace dsvgd {

constexpr int kBnnRows = 256;  // rows per chunk = threads per workgroup
constexpr int kBnnMax = 64;    // largest p and H (16 KiB of W1)

struct BnnLayout {
  int p4, Hp, sz;  // p, H rounded up to 4; row stride of the staged z
  int w1, b1, w2, z, g, r, red, floats;  // offsets (floats)
};

// The z rows are read 16 bytes per lane by consecutive rows (P1): an odd
// number of 16-byte slots per row keeps the 16 lanes of a read group on 16
// different slots of the 64-bank row.
__host__ __device__ inline BnnLayout bnn_layout(int p, int H) {
  BnnLayout L;
  L.p4 = (p + 3) & ~3;
  L.Hp = (H + 3) & ~3;
  L.sz = L.p4 + (((L.p4 >> 2) & 1) ? 0 : 4);
  L.w1 = 0;
  L.b1 = L.w1 + L.p4 * L.Hp;
  L.w2 = L.b1 + L.Hp;
  L.z = L.w2 + L.Hp;
  L.g = L.z + kBnnRows * L.sz;
  L.r = L.g + kBnnRows * L.Hp;
  L.red = L.r + kBnnRows;
  L.floats = L.red + 16;
  return L;
}

// sum over the workgroup in a fixed order (the same value in every thread)
__device__ __forceinline__ float bnn_block_sum(float v, float* red) {
  v = warp_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// hidden units [hb, hb + 4 NJ) of one row: a, relu(a) (stored if kStore) and
// their share of f, added to f in unit order
template <int NJ, bool kStore>
__device__ __forceinline__ float bnn_forward_block(const float* W1s, const float* b1s,
                                                   const float* w2s, const float* zrow,
                                                   float* arow, int KQ, int Hp, int hb, float f) {
  f32x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kq = 0; kq < KQ; ++kq) {
    const f32x4 z4 = *reinterpret_cast<const f32x4*>(zrow + 4 * kq);
    const float* w = W1s + 4 * kq * Hp + hb;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + kk * Hp + 4 * j);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[j][c] = fmaf(z4[kk], w4[c], acc[j][c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(b1s + hb + 4 * j);
    const f32x4 v4 = *reinterpret_cast<const f32x4*>(w2s + hb + 4 * j);
    f32x4 u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a = acc[j][c] + b4[c];
      u[c] = a > 0.f ? a : 0.f;  // strict: relu'(0) = 0
      f = fmaf(v4[c], u[c], f);
    }
    if (kStore) *reinterpret_cast<f32x4*>(arow + hb + 4 * j) = u;
  }
  return f;
}

template <bool kStore>
__device__ __forceinline__ float bnn_forward_row(const float* W1s, const float* b1s,
                                                 const float* w2s, const float* zrow, float* arow,
                                                 int KQ, int Hp) {
  float f = 0.f;
  int hb = 0;
  for (; hb + 16 <= Hp; hb += 16)
    f = bnn_forward_block<4, kStore>(W1s, b1s, w2s, zrow, arow, KQ, Hp, hb, f);
  switch ((Hp - hb) >> 2) {
    case 3: f = bnn_forward_block<3, kStore>(W1s, b1s, w2s, zrow, arow, KQ, Hp, hb, f); break;
    case 2: f = bnn_forward_block<2, kStore>(W1s, b1s, w2s, zrow, arow, KQ, Hp, hb, f); break;
    case 1: f = bnn_forward_block<1, kStore>(W1s, b1s, w2s, zrow, arow, KQ, Hp, hb, f); break;
    default: break;
  }
  return f;
}

// kPredict: out[i][q] = f_i(z_q) (y, a0, b0, scale unused); otherwise out[i] =
// scale * grad log p(x_i).
// kWindow: the likelihood over the cyclic window of `cnt` rows that starts at
// row *cursor, rows (c + q) mod N for q < cnt, its terms weighted wt = N / cnt
// (the minibatch estimate); the prior terms count once.  Without it the
// origin is 0, the count N and the weight 1, and none of the three is read:
// the full-data kernels keep their code.
template <bool kPredict, bool kWindow>
__global__ __launch_bounds__(kBnnRows) void bnn_kernel(const float* __restrict__ X, int64_t ldx,
                                                       int d, const float* __restrict__ Z,
                                                       int64_t ldz, const float* __restrict__ y,
                                                       int64_t N, int p, int H, float a0, float b0,
                                                       float scale, float* __restrict__ out,
                                                       int64_t ldo,
                                                       const int64_t* __restrict__ cursor,
                                                       int64_t cnt, float wt) {
  extern __shared__ __align__(16) float bnn_smem[];
  const int tid = threadIdx.x;
  const float* x = X + (int64_t)blockIdx.x * ldx;
  float* o = out + (int64_t)blockIdx.x * ldo;
  const BnnLayout L = bnn_layout(p, H);
  const int p4 = L.p4, Hp = L.Hp, sz = L.sz, KQ = p4 >> 2, HQ = Hp >> 2;
  float* W1s = bnn_smem + L.w1;
  float* b1s = bnn_smem + L.b1;
  float* w2s = bnn_smem + L.w2;
  float* zs = bnn_smem + L.z;
  float* Gs = bnn_smem + L.g;
  float* rs = bnn_smem + L.r;
  float* red = bnn_smem + L.red;
  const int pH = p * H;

  // the weights, zero past p and past H (a padded unit has a = 0: no
  // relu, no G; a padded input meets a zero of z)
  for (int e = tid; e < p4 * Hp; e += kBnnRows) {
    const int k = e / Hp, h = e - k * Hp;
    W1s[e] = (k < p && h < H) ? x[k * H + h] : 0.f;
  }
  for (int h = tid; h < Hp; h += kBnnRows) {
    b1s[h] = h < H ? x[pH + h] : 0.f;
    w2s[h] = h < H ? x[pH + H + h] : 0.f;
  }
  for (int k = p; k < sz; ++k) zs[tid * sz + k] = 0.f;
  const float b2 = x[pH + 2 * H];

  // the tiles of d W1 over the workgroup: T tiles, the rows of a chunk split
  // over SG groups of GP threads
  const int T = KQ * HQ;
  const int GP = T <= 64 ? 64 : T <= 128 ? 128 : 256;
  const int SG = kBnnRows / GP;
  const int grp = tid / GP, t = tid - grp * GP;
  const int tkq = t / HQ, thq = t - tkq * HQ;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float acc_w2 = 0.f, acc_b1 = 0.f, sr = 0.f, srr = 0.f;
  const int sq0 = tid / p, sk0 = tid - sq0 * p, sdq = kBnnRows / p, sdk = kBnnRows - sdq * p;
  // the rows walked and the window's origin, brought into [0, N) whatever
  // the cursor holds
  const int64_t M = kWindow ? cnt : N;
  int64_t org = 0;
  if (kWindow) {
    org = *cursor % N;
    if (org < 0) org += N;
  }

  for (int64_t c0 = 0; c0 < M; c0 += kBnnRows) {
    // stage: consecutive threads take consecutive elements of the chunk, p
    // each (element tid + 256 j), eight loads in flight before their stores
    for (int j0 = 0, q = sq0, k = sk0; j0 < p; j0 += 8) {
      float v[8];
      int at[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool on = j0 + u < p;
        int64_t row = c0 + q;
        const bool in = on && row < M;
        if (kWindow) {
          row += org;
          if (row >= N) row -= N;
        }
        v[u] = in ? Z[row * ldz + k] : 0.f;
        at[u] = on ? q * sz + k : -1;
        q += sdq;
        k += sdk;
        if (k >= p) {
          k -= p;
          ++q;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (at[u] >= 0) zs[at[u]] = v[u];
    }
    __syncthreads();
    {  // P1
      int64_t row = c0 + tid;
      const bool in = row < M;
      if (kWindow) {
        row += org;
        if (row >= N) row -= N;
      }
      const float f =
          bnn_forward_row<!kPredict>(W1s, b1s, w2s, zs + tid * sz, Gs + tid * Hp, KQ, Hp) + b2;
      if (kPredict) {
        if (in) o[row] = f;
      } else {
        const float r = in ? y[row] - f : 0.f;
        rs[tid] = r;
        sr += r;
        srr = fmaf(r, r, srr);
      }
    }
    __syncthreads();
    if (kPredict) continue;
    {  // P2
      const int h = tid & 63, g = tid >> 6;
      if (h < Hp) {
        const float w2h = w2s[h];
        for (int q0 = 64 * g; q0 < 64 * g + 64; q0 += 8) {  // eight rows' reads, then their writes
          float u[8], r[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            u[i] = Gs[(q0 + i) * Hp + h];
            r[i] = rs[q0 + i];
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            acc_w2 = fmaf(r[i], u[i], acc_w2);
            u[i] = u[i] > 0.f ? r[i] * w2h : 0.f;
            acc_b1 += u[i];
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) Gs[(q0 + i) * Hp + h] = u[i];
        }
      }
    }
    __syncthreads();
    if (t < T) {  // P4
      const float* zp = zs + 4 * tkq;
      const float* gp = Gs + 4 * thq;
      for (int q0 = grp * GP; q0 < grp * GP + GP; q0 += 4) {  // four rows' reads in flight
        f32x4 z4[4], g4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          z4[u] = *reinterpret_cast<const f32x4*>(zp + (q0 + u) * sz);
          g4[u] = *reinterpret_cast<const f32x4*>(gp + (q0 + u) * Hp);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(z4[u][i], g4[u][c], acc[i][c]);
      }
    }
    __syncthreads();
  }
  if (kPredict) return;

  // |theta|^2, sum r, sum r^2
  float th = 0.f;
  for (int e = tid; e < d - 2; e += kBnnRows) th = fmaf(x[e], x[e], th);
  th = bnn_block_sum(th, red);
  sr = bnn_block_sum(sr, red);
  srr = bnn_block_sum(srr, red);
  const float lg = x[d - 2], ll = x[d - 1];
  const float gam = expf(lg), lam = expf(ll);
  // the likelihood's weight rides on gamma (gw) and on the count of the
  // log gamma entry (hn = wt cnt / 2); the priors read gam and lam
  const float gw = kWindow ? __fmul_rn(wt, gam) : gam;
  const float hn = kWindow ? __fmul_rn(wt, 0.5f * (float)cnt) : 0.5f * (float)N;

  // the partial sums: tiles over Gs (SG T 16 <= 256 Hp floats), d w2 and d b1
  // over zs (8 Hp <= 256 sz floats)
  if (t < T) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(Gs + (grp * T + t) * 16 + 4 * i) = acc[i];
  }
  if ((tid & 63) < Hp) {
    zs[(tid >> 6) * Hp + (tid & 63)] = acc_w2;
    zs[(4 + (tid >> 6)) * Hp + (tid & 63)] = acc_b1;
  }
  __syncthreads();
  for (int e = tid; e < pH; e += kBnnRows) {
    const int k = e / H, h = e - k * H;
    const int tile = (k >> 2) * HQ + (h >> 2), at = 4 * (k & 3) + (h & 3);
    float s = Gs[tile * 16 + at];
    for (int g = 1; g < SG; ++g) s += Gs[(g * T + tile) * 16 + at];
    o[e] = scale * fmaf(gw, s, -lam * W1s[k * Hp + h]);
  }
  for (int h = tid; h < H; h += kBnnRows) {
    const float sw = (zs[h] + zs[Hp + h]) + (zs[2 * Hp + h] + zs[3 * Hp + h]);
    const float sb = (zs[4 * Hp + h] + zs[5 * Hp + h]) + (zs[6 * Hp + h] + zs[7 * Hp + h]);
    o[pH + h] = scale * fmaf(gw, sb, -lam * b1s[h]);
    o[pH + H + h] = scale * fmaf(gw, sw, -lam * w2s[h]);
  }
  if (tid == 0) {
    o[pH + 2 * H] = scale * fmaf(gw, sr, -lam * b2);
    o[d - 2] = scale * (hn - 0.5f * gw * srr + a0 - b0 * gam);
    o[d - 1] = scale * (0.5f * (float)(d - 2) - 0.5f * lam * th + a0 - b0 * lam);
  }
}

template <bool kPredict, bool kWindow = false>
static int bnn_launch(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Z,
                      int64_t ldz, const float* y, int64_t N, int64_t p, int64_t H, float a0,
                      float b0, float scale, float* out, int64_t ldo, void* stream,
                      const int64_t* cursor = nullptr, int64_t cnt = 0, float wt = 1.f) {
  const BnnLayout L = bnn_layout((int)p, (int)H);
  const size_t smem = sizeof(float) * (size_t)L.floats;
  // once per process, for the largest net (so that no launch inside a graph
  // capture has to raise it): p = H = 64 takes 150 KiB
  static bool reserved_on[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail_arg("bnn: device");
  bool& reserved = reserved_on[dev];
  if (!reserved) {
    const void* fn = reinterpret_cast<const void*>(&bnn_kernel<kPredict, kWindow>);
    const int most = (int)sizeof(float) * bnn_layout(kBnnMax, kBnnMax).floats;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess)
      return fail_arg("bnn: cannot reserve the chunk's LDS");
    reserved = true;
  }
  hipLaunchKernelGGL((bnn_kernel<kPredict, kWindow>), dim3((unsigned)n), dim3(kBnnRows), smem,
                     (hipStream_t)stream, X, ldx, (int)d, Z, ldz, y, N, (int)p, (int)H, a0, b0,
                     scale, out, ldo, cursor, cnt, wt);
  return check_launch(kPredict ? "bnn_predict" : kWindow ? "score_bnn_window" : "score_bnn");
}

// c <- (c + B) mod N: one thread, so that the window moves inside a captured
// iteration (the origin lives on the device)
__global__ void bnn_window_advance_kernel(int64_t* cursor, int64_t B, int64_t N) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t c = *cursor % N;
  if (c < 0) c += N;
  *cursor = (c + B) % N;
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int dsvgd_score_bnn(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Z, int64_t ldz,
                    const float* y, int64_t N, int64_t p, int64_t H, float a0, float b0,
                    float scale, float* S, int64_t lds, void* stream) {
  DSVGD_REQUIRE(X && Z && y && S, "null pointer");
  DSVGD_REQUIRE(p >= 1 && p <= kBnnMax && H >= 1 && H <= kBnnMax,
                "bnn: 1 <= p <= 64 and 1 <= H <= 64");
  DSVGD_REQUIRE(d == H * (p + 2) + 3, "bnn: d must be H (p + 2) + 3");
  DSVGD_REQUIRE(n > 0 && n <= 0x7fffffff && N > 0 && ldx >= d && lds >= d && ldz >= p, "sizes");
  return bnn_launch<false>(X, ldx, n, d, Z, ldz, y, N, p, H, a0, b0, scale, S, lds, stream);
}

int dsvgd_score_bnn_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Z,
                           int64_t ldz, const float* y, int64_t N, int64_t p, int64_t H, float a0,
                           float b0, float scale, const int64_t* cursor, int64_t B, float* S,
                           int64_t lds, void* stream) {
  DSVGD_REQUIRE(X && Z && y && S && cursor, "null pointer");
  DSVGD_REQUIRE(p >= 1 && p <= kBnnMax && H >= 1 && H <= kBnnMax,
                "bnn: 1 <= p <= 64 and 1 <= H <= 64");
  DSVGD_REQUIRE(d == H * (p + 2) + 3, "bnn: d must be H (p + 2) + 3");
  DSVGD_REQUIRE(n > 0 && n <= 0x7fffffff && N > 0 && ldx >= d && lds >= d && ldz >= p, "sizes");
  DSVGD_REQUIRE(B >= 1 && B <= N, "bnn: the window needs 1 <= B <= N");
  const float wt = (float)((double)N / (double)B);
  return bnn_launch<false, true>(X, ldx, n, d, Z, ldz, y, N, p, H, a0, b0, scale, S, lds, stream,
                                 cursor, B, wt);
}

int dsvgd_window_advance(int64_t* cursor, int64_t B, int64_t N, void* stream) {
  DSVGD_REQUIRE(cursor, "null pointer");
  DSVGD_REQUIRE(N > 0 && B >= 1 && B <= N, "window: 1 <= B <= N");
  hipLaunchKernelGGL(bnn_window_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor,
                     B, N);
  return check_launch("window_advance");
}

int dsvgd_bnn_predict(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Zt,
                      int64_t ldz, int64_t Nt, int64_t p, int64_t H, float* F, int64_t ldf,
                      void* stream) {
  DSVGD_REQUIRE(X && Zt && F, "null pointer");
  DSVGD_REQUIRE(p >= 1 && p <= kBnnMax && H >= 1 && H <= kBnnMax,
                "bnn: 1 <= p <= 64 and 1 <= H <= 64");
  DSVGD_REQUIRE(d == H * (p + 2) + 3, "bnn: d must be H (p + 2) + 3");
  DSVGD_REQUIRE(n > 0 && n <= 0x7fffffff && Nt > 0 && ldx >= d && ldf >= Nt && ldz >= p, "sizes");
  return bnn_launch<true>(X, ldx, n, d, Zt, ldz, nullptr, Nt, p, H, 0.f, 0.f, 1.f, F, ldf, stream);
}

}  // extern "C"
