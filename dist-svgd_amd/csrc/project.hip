// project.hip -- the three dense products of projected SVGD (include/dsvgd.h,
// dsvgd_proj_*): with particles X (n x d), scores S and a basis Psi (d x r),
//
//   gram   H  = (1/n) sum_i g_i g_i^T,  g = S + X (add_x) or S          (d x d)
//   apply  Xr = X Psi,  Sr = S Psi                                     (n x r)
//   lift   X += step . Phir Psi^T  (and Phi_out = Phir Psi^T)          (n x d)
//
// All on v_mfma_f32_32x32x2_f32 in exact f32: no input is split or scaled, no
// atomics, every sum in a fixed order -- the same bits on every call.  Pads
// (rows past n, columns past d or r) are selected zeros, never products of
// data that was read; every address is clamped into its array.
//
// gram: a workgroup owns one 128 x 128 block (I, J >= I) of H and one slice of
// the particles; its four waves hold 2 x 2 tiles of 32 x 32 each (a wave whose
// tiles lie below the diagonal of a diagonal block computes nothing).  The
// particle index is the MFMA's K: lane l's A and B operands are both
// g[i + (l >> 5)][c + (l & 31)], read from a chunk of 32 particles that the
// workgroup forms (S + X) on load and keeps in LDS, the next chunk's loads in
// flight under this chunk's MFMAs.  The slices' partial blocks go to the
// workspace and a second kernel sums them in slice order, scales by 1/n and
// writes every entry of the upper triangle and its mirror image.
//
// apply: a workgroup owns 64 particles; wave w the 32 x r strip of Xr (w even)
// or Sr (w odd) of one half of them.  X and S go through LDS 64 columns at a
// time (read once), Psi is the B operand straight from memory.
//
// lift: a workgroup owns 64 particles, whose Phir rows stay in LDS; wave w
// walks the column tiles w, w + 4, .. of d with both halves' accumulators,
// Psi^T the B operand straight from memory.
#include <mutex>

#include "common.hpp"

namespace dsvgd {

constexpr int kProjMaxD = 1024;
constexpr int kProjMaxR = 256;

// ---- gram ---------------------------------------------------------------------
constexpr int kPgBlock = 128;            // columns of H per workgroup, each way
constexpr int kPgChunk = 32;             // particles per LDS chunk
constexpr int64_t kPgSliceRows = 256;    // the most particles that stay in one slice
constexpr int64_t kPgMaxChain = 8192;    // longest f32 chain of one accumulator
constexpr int64_t kPgGroups = 512;       // workgroups the slices aim to fill

__host__ __device__ inline int pg_blocks(int64_t d) { return (int)((d + kPgBlock - 1) / kPgBlock); }
__host__ __device__ inline int pg_pairs(int64_t d) {
  const int b = pg_blocks(d);
  return b * (b + 1) / 2;
}

// rows of a slice: whole chunks, so that only the last slice has a ragged one
static int64_t pg_slice_rows(int64_t n, int64_t d) {
  const int64_t by_rows = (n + kPgSliceRows - 1) / kPgSliceRows;
  const int64_t fill = kPgGroups / pg_pairs(d) > 0 ? kPgGroups / pg_pairs(d) : 1;
  const int64_t chain = (n + kPgMaxChain - 1) / kPgMaxChain;
  int64_t s = by_rows < fill ? by_rows : fill;
  if (s < chain) s = chain;
  return roundup((n + s - 1) / s, kPgChunk);
}

// the slices of n particles (none empty): one slice up to kPgSliceRows
// particles, then ceil(n / kPgSliceRows) of them until they fill the CUs, and
// never a chain longer than kPgMaxChain
static int64_t pg_slices(int64_t n, int64_t d) {
  if (n < 1 || d < 1 || d > kProjMaxD) return 0;
  const int64_t per = pg_slice_rows(n, d);
  return (n + per - 1) / per;
}

__global__ __launch_bounds__(256) void proj_gram_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ S, int64_t lds, int64_t n,
    int d, int add_x, int64_t rows_per_slice, float* __restrict__ ws) {
  __shared__ float ga[kPgChunk * kPgBlock];
  __shared__ float gb[kPgChunk * kPgBlock];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  // blockIdx.x -> (I, J), I <= J, row by row of the upper triangle
  const int nb = pg_blocks(d);
  int I = 0, rest = (int)blockIdx.x;
  while (rest >= nb - I) {
    rest -= nb - I;
    ++I;
  }
  const int J = I + rest;
  const bool diag = I == J;
  const int64_t lo = (int64_t)blockIdx.y * rows_per_slice;
  const int64_t hi = min(n, lo + rows_per_slice);
  const int nchunks = (int)((hi - lo + kPgChunk - 1) / kPgChunk);
  // thread t stages column t & 127 of rows (t >> 7) + 2 j of each panel
  const int sc = t & 127, sr = t >> 7;
  const int ca = I * kPgBlock + sc, cb = J * kPgBlock + sc;
  const bool ina = ca < d, inb = cb < d;
  const int cca = min(ca, d - 1), ccb = min(cb, d - 1);
  float sa[kPgChunk / 2], sb[kPgChunk / 2];
  auto fetch = [&](int c) {
    // (row offsets by addition, a row past the slice reads row 0: no 64-bit
    // multiply and no 64-bit compare per load)
    const int64_t i0 = lo + (int64_t)c * kPgChunk + sr;
    const int left = (int)min(hi - i0, (int64_t)kPgChunk);      // rows i0 + 2 j, 2 j < left
    int64_t os = i0 * lds, ox = i0 * ldx;
#pragma unroll
    for (int j = 0; j < kPgChunk / 2; ++j) {
      const bool in = 2 * j < left;
      const int64_t rs = in ? os : 0, rx = in ? ox : 0;
      float v = S[rs + cca];
      if (add_x) v += X[rx + cca];
      sa[j] = (ina && in) ? v : 0.f;
      if (!diag) {
        float u = S[rs + ccb];
        if (add_x) u += X[rx + ccb];
        sb[j] = (inb && in) ? u : 0.f;
      }
      os += 2 * lds;
      ox += 2 * ldx;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < kPgChunk / 2; ++j) {
      ga[(sr + 2 * j) * kPgBlock + sc] = sa[j];
      if (!diag) gb[(sr + 2 * j) * kPgBlock + sc] = sb[j];
    }
  };
  // wave w: tile rows 2 (w >> 1) + {0, 1}, tile columns 2 (w & 1) + {0, 1} of the block
  const int tr0 = 2 * (w >> 1), tc0 = 2 * (w & 1);
  const bool work = !(diag && tr0 > tc0);
  const float* pa = ga + tr0 * 32 + r;
  const float* pb = (diag ? ga : gb) + tc0 * 32 + r;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

  fetch(0);
  put();
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    if (more) fetch(c + 1);
    if (work) {
#pragma unroll
      for (int k = 0; k < kPgChunk; k += 2) {
        const int o = (k + h) * kPgBlock;
        const float a0 = pa[o], a1 = pa[o + 32], b0 = pb[o], b1 = pb[o + 32];
        acc[0][0] = mfma32(a0, b0, acc[0][0]);
        acc[0][1] = mfma32(a0, b1, acc[0][1]);
        acc[1][0] = mfma32(a1, b0, acc[1][0]);
        acc[1][1] = mfma32(a1, b1, acc[1][1]);
      }
    }
    __syncthreads();          // the chunk's readers are done
    if (more) put();
    __syncthreads();
  }
  if (!work) return;
  // the slice's block: ws[((slice pairs + pair) 128 + row) 128 + column]
  float* out = ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPgBlock * kPgBlock);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (diag && tr0 + a > tc0 + b) continue;      // a tile below the diagonal
#pragma unroll
      for (int q = 0; q < 16; ++q)
        out[((tr0 + a) * 32 + c_row(q, lane)) * kPgBlock + (tc0 + b) * 32 + r] = acc[a][b][q];
    }
}

// H[k][l] = H[l][k] = (1/n) sum over the slices, in slice order, k <= l
__global__ __launch_bounds__(256) void proj_gram_reduce_kernel(
    const float* __restrict__ ws, int d, int slices, float inv_n, float* __restrict__ H,
    int64_t ldh) {
  const int l = (int)blockIdx.x * 256 + threadIdx.x, k = (int)blockIdx.y;
  if (l >= d || k > l) return;
  const int nb = pg_blocks(d), I = k / kPgBlock, J = l / kPgBlock;
  const int pair = I * nb - I * (I - 1) / 2 + (J - I);
  const int64_t npairs = pg_pairs(d);
  const float* p = ws + ((int64_t)pair * kPgBlock + (k - I * kPgBlock)) * kPgBlock + (l - J * kPgBlock);
  const int64_t stride = npairs * (kPgBlock * kPgBlock);
  float s = 0.f;
  int z = 0;
  for (; z + 8 <= slices; z += 8) {     // eight loads in flight, added in slice order
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = p[(int64_t)(z + e) * stride];
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  }
  for (; z < slices; ++z) s += p[(int64_t)z * stride];
  s *= inv_n;
  H[(int64_t)k * ldh + l] = s;
  H[(int64_t)l * ldh + k] = s;
}

// ---- apply --------------------------------------------------------------------
constexpr int kPaRows = 64;               // particles per workgroup
constexpr int kPaPiece = 64;              // columns of X and S staged at a time
constexpr int kPaPitch = kPaPiece + 8;    // rows 4 apart 32 banks apart (ds_read_b128)

template <int NT>   // 32-column tiles of the r columns per wave
__global__ __launch_bounds__(256) void proj_apply_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ S, int64_t lds, int64_t n,
    int d, const float* __restrict__ Psi, int64_t ldpsi, int r, float* __restrict__ Xr,
    int64_t ldxr, float* __restrict__ Sr, int64_t ldsr) {
  __shared__ __attribute__((aligned(16))) float buf[2 * kPaRows * kPaPitch];   // [X | S]
  const int t = threadIdx.x, lane = t & 63, rr = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * kPaRows;
  const int npieces = (d + kPaPiece - 1) / kPaPiece;
  // thread t stages column t & 63 of rows (t >> 6) + 4 j of both arrays
  const int sc = t & 63, sr = t >> 6;
  float sx[kPaRows / 4], ss[kPaRows / 4];
  auto fetch = [&](int pc) {
    const int col = pc * kPaPiece + sc;
    const int cc = min(col, d - 1);
#pragma unroll
    for (int j = 0; j < kPaRows / 4; ++j) {
      const int64_t i = i0 + sr + 4 * j;
      const int64_t ic = i < n ? i : 0;
      const float a = X[ic * ldx + cc], b = S[ic * lds + cc];
      const bool in = col < d && i < n;
      sx[j] = in ? a : 0.f;
      ss[j] = in ? b : 0.f;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < kPaRows / 4; ++j) {
      buf[(sr + 4 * j) * kPaPitch + sc] = sx[j];
      buf[(kPaRows + sr + 4 * j) * kPaPitch + sc] = ss[j];
    }
  };
  // wave w: the array w & 1 (X, S), the row tile w >> 1
  const float* arow = buf + ((w & 1) * kPaRows + (w >> 1) * 32 + rr) * kPaPitch + 4 * h;
  f32x16 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ct][q] = 0.f;

  fetch(0);
  put();
  __syncthreads();
  for (int pc = 0; pc < npieces; ++pc) {
    const bool more = pc + 1 < npieces;
    if (more) fetch(pc + 1);
    const int nu = (min(kPaPiece, d - pc * kPaPiece) + 7) >> 3;
    for (int u = 0; u < nu; ++u) {
      // K order of the group: half h takes columns 8 u + 4 h + e, e = 0..3
      const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 8 * u);
      const int k0 = pc * kPaPiece + 8 * u + 4 * h;
      float b[NT][4];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 32 * ct + rr;
        const int cc = min(c, r - 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = Psi[(int64_t)min(k0 + e, d - 1) * ldpsi + cc];
          b[ct][e] = (k0 + e < d && c < r) ? v : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[ct] = mfma32(a[e], b[ct][e], acc[ct]);
    }
    __syncthreads();
    if (more) put();
    __syncthreads();
  }
  float* out = (w & 1) ? Sr : Xr;
  const int64_t ldo = (w & 1) ? ldsr : ldxr;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int c = 32 * ct + rr;
    if (c >= r) continue;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t i = i0 + (w >> 1) * 32 + c_row(q, lane);
      if (i < n) out[i * ldo + c] = acc[ct][q];
    }
  }
}

// ---- lift ---------------------------------------------------------------------
constexpr int kPlRows = 64;               // particles per workgroup

__host__ __device__ inline int pl_pitch(int r) { return ((r + 31) & ~31) + 8; }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void proj_lift_kernel(
    const float* __restrict__ Phir, int64_t ldphi, const float* __restrict__ Psi, int64_t ldpsi,
    int64_t n, int d, int r, float step, float* __restrict__ X, int64_t ldx,
    float* __restrict__ Phi_out, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) float pbuf[];   // kPlRows x pl_pitch(r)
  const int t = threadIdx.x, lane = t & 63, rr = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * kPlRows;
  const int pitch = pl_pitch(r), rp = pitch - 8;
  // the workgroup's rows of Phir, zero past r and past n
  for (int e = t; e < kPlRows * rp; e += 256) {
    const int row = e / rp, col = e - row * rp;
    const int64_t i = i0 + row;
    const float v = Phir[(i < n ? i : 0) * ldphi + min(col, r - 1)];
    pbuf[row * pitch + col] = (i < n && col < r) ? v : 0.f;
  }
  __syncthreads();
  const float* a0p = pbuf + rr * pitch + 4 * h;
  const float* a1p = a0p + 32 * pitch;
  const int nu = (r + 7) >> 3;
  const int ntiles = (d + 31) >> 5;
  for (int ct = w; ct < ntiles; ct += 4) {
    const int c = 32 * ct + rr;              // this lane's column of X: row c of Psi
    const float* prow = Psi + (int64_t)min(c, d - 1) * ldpsi;
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
    for (int u = 0; u < nu; ++u) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a0p + 8 * u);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(a1p + 8 * u);
      const int k0 = 8 * u + 4 * h;
      float b[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = prow[min(k0 + e, r - 1)];
        b[e] = (k0 + e < r && c < d) ? v : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = mfma32(a0[e], b[e], acc0);
        acc1 = mfma32(a1[e], b[e], acc1);
      }
    }
    if (c >= d) continue;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x16& acc = half ? acc1 : acc0;
      if (step != 0.f) {
        float xv[16];          // the tile's loads in flight, then its stores
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t i = i0 + 32 * half + c_row(q, lane);
          xv[q] = X[(i < n ? i : 0) * ldx + c];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t i = i0 + 32 * half + c_row(q, lane);
          if (i < n) X[i * ldx + c] = fmaf(step, acc[q], xv[q]);
        }
      }
      if (Phi_out) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t i = i0 + 32 * half + c_row(q, lane);
          if (i < n) Phi_out[i * ldo + c] = acc[q];
        }
      }
    }
  }
}

static int proj_sizes(int64_t n, int64_t d, int64_t r) {
  DSVGD_REQUIRE(n >= 1, "projection: n >= 1");
  DSVGD_REQUIRE(d >= 1 && d <= kProjMaxD, "projection: 1 <= d <= 1024");
  DSVGD_REQUIRE(r >= 1 && r <= d && r <= kProjMaxR, "projection: 1 <= r <= min(d, 256)");
  return 0;
}

}  // namespace dsvgd

using namespace dsvgd;

extern "C" {

int64_t dsvgd_proj_gram_slices(int64_t n, int64_t d) { return pg_slices(n, d); }

size_t dsvgd_proj_gram_workspace_bytes(int64_t n, int64_t d) {
  const int64_t s = pg_slices(n, d);
  if (s < 1) return 0;
  return (size_t)s * (size_t)pg_pairs(d) * kPgBlock * kPgBlock * sizeof(float);
}

int dsvgd_proj_gram(const float* X, int64_t ldx, const float* S, int64_t lds, int64_t n, int64_t d,
                    int add_x, void* workspace, float* H, int64_t ldh, void* stream) {
  DSVGD_REQUIRE(S && workspace && H && (X || !add_x), "null pointer");
  if (int rc = proj_sizes(n, d, 1)) return rc;
  DSVGD_REQUIRE(lds >= d && ldh >= d && (!add_x || ldx >= d), "sizes");
  const int64_t slices = pg_slices(n, d);
  DSVGD_REQUIRE(slices <= 65535, "projection: too many particles for one Gram");
  const int64_t per = pg_slice_rows(n, d);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(proj_gram_kernel, dim3((unsigned)pg_pairs(d), (unsigned)slices), dim3(256), 0,
                     s, X, ldx, S, lds, n, (int)d, add_x ? 1 : 0, per,
                     (float*)workspace);
  if (int rc = check_launch("proj_gram")) return rc;
  hipLaunchKernelGGL(proj_gram_reduce_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)d),
                     dim3(256), 0, s, (const float*)workspace, (int)d, (int)slices,
                     (float)(1.0 / (double)n), H, ldh);
  return check_launch("proj_gram_reduce");
}

int dsvgd_proj_apply(const float* X, int64_t ldx, const float* S, int64_t lds, int64_t n,
                     int64_t d, const float* Psi, int64_t ldpsi, int64_t r, float* Xr,
                     int64_t ldxr, float* Sr, int64_t ldsr, void* stream) {
  DSVGD_REQUIRE(X && S && Psi && Xr && Sr, "null pointer");
  if (int rc = proj_sizes(n, d, r)) return rc;
  DSVGD_REQUIRE(ldx >= d && lds >= d && ldpsi >= r && ldxr >= r && ldsr >= r, "sizes");
  const int64_t groups = (n + kPaRows - 1) / kPaRows;
  DSVGD_REQUIRE(groups <= 0x7fffffff, "too many row tiles");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)groups), block(256);
  const int nt = (int)((r + 31) / 32);
#define DSVGD_PROJ_APPLY(NT)                                                                     \
  hipLaunchKernelGGL(proj_apply_kernel<NT>, grid, block, 0, s, X, ldx, S, lds, n, (int)d, Psi,    \
                     ldpsi, (int)r, Xr, ldxr, Sr, ldsr)
  if (nt <= 1) DSVGD_PROJ_APPLY(1);
  else if (nt <= 2) DSVGD_PROJ_APPLY(2);
  else if (nt <= 4) DSVGD_PROJ_APPLY(4);
  else DSVGD_PROJ_APPLY(8);
#undef DSVGD_PROJ_APPLY
  return check_launch("proj_apply");
}

int dsvgd_proj_lift(const float* Phir, int64_t ldphi, const float* Psi, int64_t ldpsi, int64_t n,
                    int64_t d, int64_t r, float step, float* X, int64_t ldx, float* Phi_out,
                    int64_t ldo, void* stream) {
  DSVGD_REQUIRE(Phir && Psi && (X || step == 0.f), "null pointer");
  if (int rc = proj_sizes(n, d, r)) return rc;
  DSVGD_REQUIRE(ldphi >= r && ldpsi >= r && (step == 0.f || ldx >= d) && (!Phi_out || ldo >= d),
                "sizes");
  if (step == 0.f && !Phi_out) return 0;      // nothing to write
  const int64_t groups = (n + kPlRows - 1) / kPlRows;
  DSVGD_REQUIRE(groups <= 0x7fffffff, "too many row tiles");
  const size_t shmem = (size_t)kPlRows * pl_pitch((int)r) * sizeof(float);
  // once per process and device, for the widest basis (so that no launch inside
  // a graph capture has to raise it): r = 256 takes 66 KiB
  static std::once_flag reserve_once[64];
  static bool reserved_on[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail_arg("proj_lift: device");
  std::call_once(reserve_once[dev], [dev] {
    const int most = (int)sizeof(float) * kPlRows * pl_pitch(kProjMaxR);
    reserved_on[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(&proj_lift_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           most) == hipSuccess;
  });
  if (!reserved_on[dev]) return fail_arg("proj_lift: cannot reserve the rows' LDS");
  hipLaunchKernelGGL(proj_lift_kernel, dim3((unsigned)groups), dim3(256), shmem,
                     (hipStream_t)stream, Phir, ldphi, Psi, ldpsi, n, (int)d, (int)r, step, X, ldx,
                     Phi_out, ldo);
  return check_launch("proj_lift");
}

}  // extern "C"
