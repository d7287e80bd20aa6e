// logreg_window.hip -- the minibatch estimate of the logistic-regression score
// (logreg.hip's model, experiments/logreg.py:45-58): the likelihood over the
// cyclic window of B data rows that starts at row c = *cursor % N, rows
// (c + q) mod N for q < B, weighted N / B, and the prior once:
//
//   S[i, 1:] = scale ((N/B) sum_q g_iq xd_q - a_i w_i),  g_iq = t_q sigma(-t_q xd_q.w_i)
//   S[i, 0]  = scale (-a_i + p/2 - a_i |w_i|^2 / 2)
//
// A window is a few hundred rows: no data image prepared per data set pays
// for itself, so the rows are read where they lie, every call, in exact f32.
//
// Tile form (n > kWinSmallRows): a workgroup of 4 waves scores 128 particles,
// a wave 32 of them.  The wave keeps its particles' weights in registers as
// the B operand of Z^T = Xd' W^T (v_mfma_f32_32x32x2_f32; Xd' = t Xd, the
// labels folded into the rows as they are staged, rows past B zero) and the
// 32 x 256 block of G Xd' in accumulators (the weights come through LDS once,
// a row at a time from memory, each wave through its own quarter of the
// buffer).  The window goes by in chunks of 32 rows through LDS, the next
// chunk's loads in flight under this chunk's MFMAs.  Z^T's C layout puts
// particle l & 31 in lane l and data rows c_row(j, l) in its 16 registers:
// sigma(-z) of register j IS the A operand of G Xd's K-step j when the B
// operand takes row c_row(j, l) of the chunk, so G never leaves the
// registers.  K runs in a permuted order that A and B share (K-step 4u + e,
// half h <-> column 8u + 4h + e): a lane's weights and its LDS reads are then
// runs of four consecutive floats.
//
// p > 256: blockIdx.y owns a slab of 256 output columns; Z is summed over all
// the slabs (the weights reloaded per slab, one LDS buffer), then the own
// slab's rows are staged for G Xd'.
//
// Row form (n <= kWinSmallRows, the sequential order's one-particle refresh):
// a workgroup per particle, nothing staged: g of 256 rows at a time (a wave
// per row), then a thread per column.
//
// Every sum runs in a fixed order, without atomics: the same bits on every call.
#include "common.hpp"

namespace dsvgd {

constexpr int kWinRows = 128;       // particles per workgroup (32 per wave)
constexpr int kWinChunk = 32;       // window rows per chunk
constexpr int kWinSlab = 256;       // columns per slab
constexpr int kWinPitch = kWinSlab + 8;   // LDS row pitch (floats): rows 4 apart 32 banks apart
constexpr int kWinBuf = kWinChunk * kWinPitch;
constexpr int64_t kWinSmallRows = 16;
constexpr int kWinSmallChunk = 256;

__device__ __forceinline__ int64_t window_origin(const int64_t* cursor, int64_t N) {
  int64_t org = *cursor % N;
  return org < 0 ? org + N : org;
}

template <bool MULTI, bool FULLW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void logreg_window_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t n, int p, const float* __restrict__ Xd,
    int64_t ldxd, const float* __restrict__ tl, int64_t N, const int64_t* __restrict__ cursor,
    int B, float wt, float scale, float* __restrict__ S, int64_t lds) {
  __shared__ __attribute__((aligned(16))) float buf[(MULTI ? 1 : 4) * kWinBuf];
  __shared__ float sa[kWinRows];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t i = (int64_t)blockIdx.x * kWinRows + w * 32 + r;   // this lane's particle
  const bool live = i < n;
  const float* x = X + (live ? i : 0) * ldx;
  const int dp = (p + 31) & ~31;
  const int nslab = (dp + kWinSlab - 1) / kWinSlab;
  const int own = MULTI ? (int)blockIdx.y : 0;
  const int64_t org = window_origin(cursor, N);
  const int nchunks = (B + kWinChunk - 1) / kWinChunk;
  const int64_t i0 = (int64_t)blockIdx.x * kWinRows + w * 32;   // the wave's first particle
  // a slab's width; FULLW (p in 225 .. 256): a constant, so that the unrolled
  // loops below are straight-line code the scheduler can pipeline
  auto width = [&](int s) { return FULLW ? kWinSlab : min(kWinSlab, dp - s * kWinSlab); };

  // the weights of slab s: wf[u][e] = w_i[256 s + 8u + 4h + e], zero past p
  float wf[kWinSlab / 8][4];
  float w2 = 0.f;
  auto load_w = [&](int s, bool norm) {
    const int wid = width(s);
#pragma unroll
    for (int u = 0; u < kWinSlab / 8; ++u) {
      if (8 * u >= wid) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = s * kWinSlab + 8 * u + 4 * h + e;
        wf[u][e] = (live && c < p) ? x[1 + c] : 0.f;
        if (norm) w2 = fmaf(wf[u][e], wf[u][e], w2);
      }
    }
  };
  // chunk c, slab s: rows (t >> 5) + 8 jr, columns 256 s + 32 jc + (t & 31)
  // (the loads are issued back to back, from addresses clamped into the
  // window -- a pad row reads the window's first row; the label, the row and
  // column masks are applied when the values go to LDS: a pad is a selected
  // zero, never a product, so nothing outside the window reaches the result)
  float stg[4][kWinSlab / 32], stq[4];
  int sin = 0;           // bit jr: row jr of this thread lies in the window
  auto fetch = [&](int c, int s) {
    const int wid = width(s);
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      const int q = c * kWinChunk + (t >> 5) + 8 * jr;
      int64_t row = org + q;
      if (row >= N) row -= N;
      const bool in = q < B;
      if (!in) row = org;
      sin = in ? sin | (1 << jr) : sin & ~(1 << jr);
      stq[jr] = tl[row];
      const float* xr = Xd + row * ldxd;
#pragma unroll
      for (int jc = 0; jc < kWinSlab / 32; ++jc) {
        if (32 * jc >= wid) break;
        const int col = s * kWinSlab + 32 * jc + (t & 31);
        stg[jr][jc] = xr[min(col, p - 1)];
      }
    }
  };
  auto put = [&](float* dst, int s) {
    const int wid = width(s);
#pragma unroll
    for (int jr = 0; jr < 4; ++jr)
#pragma unroll
      for (int jc = 0; jc < kWinSlab / 32; ++jc) {
        if (32 * jc >= wid) break;
        const int col = s * kWinSlab + 32 * jc + (t & 31);
        dst[((t >> 5) + 8 * jr) * kWinPitch + 32 * jc + (t & 31)] =
            (col < p && ((sin >> jr) & 1)) ? stq[jr] * stg[jr][jc] : 0.f;
      }
  };
  // Z^T of the chunk in `src` over slab s's columns, two chains
  auto zmm = [&](const float* src, int s, f32x16& z0, f32x16& z1) {
    const int wid = width(s);
#pragma unroll
    for (int u = 0; u < kWinSlab / 8; ++u) {
      if (8 * u >= wid) break;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + r * kWinPitch + 8 * u + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f32x16& z = (e & 1) ? z1 : z0;
        z = mfma32(a[e], wf[u][e], z);
      }
    }
  };
  f32x16 acc[kWinSlab / 32];
#pragma unroll
  for (int ni = 0; ni < kWinSlab / 32; ++ni)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ni][q] = 0.f;
  const int ownw = width(own);
  // acc += G (chunk) . Xd' (chunk, own slab) with G = sigma(-z) from registers
  auto gxd = [&](const float* src, const f32x16& z0, const f32x16& z1) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float g =
          __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f((z0[j] + z1[j]) * kLog2e));
      const float* row = src + c_row(j, lane) * kWinPitch + r;
#pragma unroll
      for (int ni = 0; ni < kWinSlab / 32; ++ni) {
        if (32 * ni >= ownw) break;
        acc[ni] = mfma32(g, row[32 * ni], acc[ni]);
      }
    }
  };

  if (h == 0) sa[w * 32 + r] = live ? expf(x[0]) : 0.f;
  if (!MULTI) {
    // the wave's 32 x dp weights through its own quarter of the buffer: read
    // from memory a row at a time (a lane per column), then the fragments
    {
      float* wreg = buf + w * kWinBuf;
      const int wid = width(0);
      for (int r8 = 0; r8 < 32; r8 += 8) {      // 8 rows' loads in flight, then their stores
        float v[8][kWinSlab / 64];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          const int64_t ii = i0 + r8 + rr;
          const float* xr = X + (ii < n ? ii : 0) * ldx + 1;
#pragma unroll
          for (int k = 0; k < kWinSlab / 64; ++k) v[rr][k] = xr[min(lane + 64 * k, p - 1)];
        }
#pragma unroll
        for (int rr = 0; rr < 8; ++rr)
#pragma unroll
          for (int k = 0; k < kWinSlab / 64; ++k) {
            const int c = lane + 64 * k;
            if (c < wid)
              wreg[(r8 + rr) * kWinPitch + c] = (i0 + r8 + rr < n && c < p) ? v[rr][k] : 0.f;
          }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kWinSlab / 8; ++u) {
        if (8 * u >= wid) break;
        const f32x4 v = *reinterpret_cast<const f32x4*>(wreg + r * kWinPitch + 8 * u + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          wf[u][e] = v[e];
          w2 = fmaf(v[e], v[e], w2);
        }
      }
      __syncthreads();          // the quarters are the chunk ring from here on
    }
    fetch(0, 0);
    put(buf, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      const float* cur = buf + (c & 1) * kWinBuf;
      if (c + 1 < nchunks) fetch(c + 1, 0);
      f32x16 z0 = {}, z1 = {};
      zmm(cur, 0, z0, z1);
      gxd(cur, z0, z1);
      if (c + 1 < nchunks) put(buf + ((c + 1) & 1) * kWinBuf, 0);
      __syncthreads();
    }
  } else {
    for (int c = 0; c < nchunks; ++c) {
      f32x16 z0 = {}, z1 = {};
      for (int s = 0; s < nslab; ++s) {
        fetch(c, s);
        load_w(s, c == 0);
        __syncthreads();          // the buffer's readers are done
        put(buf, s);
        __syncthreads();
        zmm(buf, s, z0, z1);
      }
      fetch(c, own);
      __syncthreads();
      put(buf, own);
      __syncthreads();
      gxd(buf, z0, z1);
    }
    __syncthreads();
  }

  // S[i][1 + col] = scale (wt acc - a_i w_i[col]); acc register q: particle c_row(q, lane)
#pragma unroll
  for (int ni = 0; ni < kWinSlab / 32; ++ni) {
    if (32 * ni >= ownw) break;
    const int col = own * kWinSlab + 32 * ni + r;
    const int cc = min(col, p - 1);
    float xv[16];          // the tile's 16 loads in flight, then its stores
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t ii = i0 + c_row(q, lane);
      xv[q] = X[(ii < n ? ii : 0) * ldx + 1 + cc];
    }
    if (col < p) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rr = c_row(q, lane);
        const int64_t ii = i0 + rr;
        if (ii < n) S[ii * lds + 1 + col] = scale * (wt * acc[ni][q] - sa[w * 32 + rr] * xv[q]);
      }
    }
  }
  w2 += __shfl_xor(w2, 32, 64);
  if (own == 0 && h == 0 && live) {
    const float a = sa[w * 32 + r];
    S[i * lds] = scale * (-a + 0.5f * (float)p - 0.5f * a * w2);
  }
}

// one workgroup per particle (n <= kWinSmallRows)
__global__ __launch_bounds__(256) void logreg_window_row_kernel(
    const float* __restrict__ X, int64_t ldx, int p, const float* __restrict__ Xd, int64_t ldxd,
    const float* __restrict__ tl, int64_t N, const int64_t* __restrict__ cursor, int64_t B,
    float wt, float scale, float* __restrict__ S, int64_t lds) {
  __shared__ float g[kWinSmallChunk];
  __shared__ float red[4];
  const float* x = X + (int64_t)blockIdx.x * ldx;
  float* out = S + (int64_t)blockIdx.x * lds;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t org = window_origin(cursor, N);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t c0 = 0; c0 < B; c0 += kWinSmallChunk) {
    const int cnt = (int)min((int64_t)kWinSmallChunk, B - c0);
    for (int q = wv; q < cnt; q += 4) {
      int64_t row = org + c0 + q;
      if (row >= N) row -= N;
      const float* xq = Xd + row * ldxd;
      float z = 0.f;
      for (int c = lane; c < p; c += 64) z = fmaf(xq[c], x[1 + c], z);
      z = warp_sum(z);
      if (lane == 0) {
        const float tq = tl[row];
        g[q] = tq / (1.f + expf(tq * z));   // t sigma(-t z)
      }
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      int64_t row = org + c0 + q;
      if (row >= N) row -= N;
      const float* xq = Xd + row * ldxd;
      const float gq = g[q];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (tid + 256 * u < p) acc[u] = fmaf(gq, xq[tid + 256 * u], acc[u]);
    }
    __syncthreads();
  }
  const float a = expf(x[0]);
  float w2 = 0.f;
  for (int c = tid; c < p; c += 256) w2 = fmaf(x[1 + c], x[1 + c], w2);
  w2 = warp_sum(w2);
  if (lane == 0) red[wv] = w2;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (tid + 256 * u < p)
      out[1 + tid + 256 * u] = scale * (wt * acc[u] - a * x[1 + tid + 256 * u]);
  if (tid == 0)
    out[0] = scale * (-a + 0.5f * (float)p - 0.5f * a * ((red[0] + red[1]) + (red[2] + red[3])));
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

size_t dsvgd_logreg_window_workspace_bytes(int64_t n, int64_t B, int64_t p) {
  (void)n;
  (void)B;
  (void)p;
  return 0;   // the window is staged through LDS; G stays in registers
}

int dsvgd_score_logreg_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                              int64_t ldxd, const float* t, int64_t N, float scale, float* S,
                              int64_t lds, void* workspace, int engine, const int64_t* cursor,
                              int64_t B, void* stream) {
  (void)workspace;
  DSVGD_REQUIRE(X && Xd && t && S && cursor, "null pointer");
  DSVGD_REQUIRE(n > 0 && d >= 2 && N > 0 && ldx >= d && lds >= d && ldxd >= d - 1, "sizes");
  DSVGD_REQUIRE(d - 1 <= 1023, "logreg window: at most 1023 weights");
  DSVGD_REQUIRE(engine >= 0 && engine <= 2, "engine must be 0 (h2), 1 (x3) or 2 (f32)");
  DSVGD_REQUIRE(B >= 1 && B <= N, "logreg window: the window needs 1 <= B <= N");
  DSVGD_REQUIRE(B <= ((int64_t)1 << 30), "logreg window: B too large");
  const int p = (int)(d - 1);
  const float wt = (float)((double)N / (double)B);
  hipStream_t s = (hipStream_t)stream;
  if (n <= kWinSmallRows) {
    hipLaunchKernelGGL(logreg_window_row_kernel, dim3((unsigned)n), dim3(256), 0, s, X, ldx, p, Xd,
                       ldxd, t, N, cursor, B, wt, scale, S, lds);
    return check_launch("logreg_window_row");
  }
  const int64_t tiles = (n + kWinRows - 1) / kWinRows;
  DSVGD_REQUIRE(tiles <= 0x7fffffff, "too many row tiles");
  const int nslab = (int)((roundup(p, 32) + kWinSlab - 1) / kWinSlab);
  if (nslab == 1 && roundup(p, 32) == kWinSlab) {
    hipLaunchKernelGGL((logreg_window_kernel<false, true>), dim3((unsigned)tiles), dim3(256), 0, s,
                       X, ldx, n, p, Xd, ldxd, t, N, cursor, (int)B, wt, scale, S, lds);
  } else if (nslab == 1) {
    hipLaunchKernelGGL((logreg_window_kernel<false, false>), dim3((unsigned)tiles), dim3(256), 0, s,
                       X, ldx, n, p, Xd, ldxd, t, N, cursor, (int)B, wt, scale, S, lds);
  } else {
    hipLaunchKernelGGL((logreg_window_kernel<true, false>), dim3((unsigned)tiles, (unsigned)nslab),
                       dim3(256), 0, s, X, ldx, n, p, Xd, ldxd, t, N, cursor, (int)B, wt, scale, S,
                       lds);
  }
  return check_launch("logreg_window");
}

}  // extern "C"
