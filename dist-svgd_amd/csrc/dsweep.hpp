// dsweep.hpp -- the one traversal of the distance matrix D that the row-sum
// diagnostics share (ksd.hip, mmd.hip; DESIGN.md, "The D-sweep walker"): the
// walks of the full and of the symmetric panel layout over a payload, the
// finish kernels' slot summing and the second-level reduce.
//
// A walk owns the geometry (tile row I, slice z, pads, the diagonal), the two
// loads per panel, the edge / interior dispatch, the quad sums and the slots.
// A payload PL owns what differs between the diagnostics:
//   PL::extra                         what load() returns (an empty struct: none)
//   extra load(c, cq)                 the per-panel extra load of column quad cq
//   bool  edge(c)                     a further reason to mask panel c
//   void  rows(i0)                    the constants of rows i0, i0 + 64 that the
//                                     column sums need (symmetric walk only)
//   panel<EDGE, COLS>(v0, v1, x, c, g0, j0, rv0, rv1, n, s00, s01, s10, s11, cv)
// panel adds one panel's share of a thread -- rows g0 (v0) and g0 + 64 (v1),
// four columns from j0 -- into quantity 0 / 1 of the first row (s00, s01) and
// of the second (s10, s11).  EDGE: entries with a row (rv0, rv1) or a column
// (>= n) past the matrix (+inf pads) or on the diagonal contribute exactly 0.
// COLS: cv[0..3] = the four columns' sums of quantity 0 over the two rows for
// the transposed entries, cv[4..7] = those of quantity 1.
//
// Ix is the index type of a walk: int64_t where a row block of a large matrix
// is swept (KSD), int where n <= 2^20 lets every index but the offsets into D
// and P stay in 32 bits (MMD).  Everything is deterministic: every partial has
// a slot of its own and every sum a fixed order.
#pragma once

#include <algorithm>

#include "common.hpp"

namespace dsvgd {

constexpr int kSweepPanel = 2048;        // 128 rows x 16 columns of D, contiguous
constexpr int kSweepBlockTarget = 2048;  // workgroups that fill 256 CUs 8 deep
constexpr int kSweepRowsPerBlock = 64;   // rows of one finish / direct workgroup

// row slices per tile row: enough workgroups to reach the block target, at most cap
inline int64_t row_parts(int64_t tiles, int64_t cap) {
  return std::max<int64_t>(1, std::min<int64_t>((kSweepBlockTarget + tiles - 1) / tiles, cap));
}

// rows [row0, row0 + m) of an n-column matrix, padded to m_pad x n_pad
template <class Ix>
struct SweepGeom {
  Ix n_pad, row0, m, n, m_pad;
};

// the four lanes that share a row hold its partial sums
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// Eight per-thread values (two quantities x four columns) summed over the 16
// lanes of a wave that hold the same columns (lane bits 2..5), each step
// trading half of what is left: 8 cross-lane moves instead of 32.  Returns,
// in every lane, the wave's sum of quantity (lane >> 2) & 1 for the column
// 2 ((lane >> 3) & 1) + ((lane >> 4) & 1) of the lane's quad.
__device__ __forceinline__ float col_reduce8(const float* v, int lane) {
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

// slot z of P: P[z][0][i], P[z][1][i] = the two quantities of rows i0, i0 + 64
__device__ __forceinline__ void sweep_store(float* __restrict__ Pz, int64_t i0, int64_t m_pad,
                                            float s00, float s01, float s10, float s11) {
  s00 = quad_sum(s00);
  s10 = quad_sum(s10);
  s01 = quad_sum(s01);
  s11 = quad_sum(s11);
  if ((threadIdx.x & 3) == 0) {
    Pz[i0] = s00;
    Pz[i0 + 64] = s10;
    Pz[m_pad + i0] = s01;
    Pz[m_pad + i0 + 64] = s11;
  }
}

// Full panel layout: workgroup (I, z) walks the 16-column panels of row tile
// I in column slice z; thread t reads two 16-byte pieces per panel (rows t/4
// and t/4 + 64, columns 4 (t % 4) ..), a wave 1 KiB contiguous per load.
// Slot z of P takes the slice's row sums.  No LDS.
template <class Ix, class PL>
__device__ __forceinline__ void sweep_full(const float* __restrict__ D, const SweepGeom<Ix> g,
                                           int parts, float* __restrict__ P, PL& pl) {
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2;
  const Ix I = blockIdx.x;
  const int z = blockIdx.y;
  const Ix pcols = g.n_pad >> 4;
  const Ix c0 = (Ix)((int64_t)pcols * z / parts), c1 = (Ix)((int64_t)pcols * (z + 1) / parts);
  const Ix i0 = I * 128 + r0;
  const bool rv0 = i0 < g.m, rv1 = i0 + 64 < g.m;
  const Ix g0 = g.row0 + i0;        // the row's own column
  const Ix gt = g.row0 + I * 128;   // the tile's first own column
  const bool row_edge = (I + 1) * 128 > g.m;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + (int64_t)I * pcols * (kSweepPanel / 4) + t;
  float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
#pragma unroll 2
  for (Ix c = c0; c < c1; ++c) {
    const f32x4 v0 = Dp[(int64_t)c * (kSweepPanel / 4)];
    const f32x4 v1 = Dp[(int64_t)c * (kSweepPanel / 4) + 256];
    const typename PL::extra x = pl.load(c, cq);
    const Ix j0 = 16 * c + 4 * cq;
    const bool edge = row_edge || 16 * c + 16 > g.n || (16 * c + 15 >= gt && 16 * c <= gt + 127) ||
                      pl.edge(c);
    if (edge)
      pl.template panel<true, false>(v0, v1, x, c, g0, j0, rv0, rv1, g.n, s00, s01, s10, s11,
                                     nullptr);
    else
      pl.template panel<false, false>(v0, v1, x, c, g0, j0, rv0, rv1, g.n, s00, s01, s10, s11,
                                      nullptr);
  }
  sweep_store(P + (int64_t)z * 2 * g.m_pad, i0, g.m_pad, s00, s01, s10, s11);
}

// Symmetric layout (only tiles (I, J >= I) stored; m == n, row0 == 0):
// workgroup (I, z) walks slice z of the stored tiles of tile row I.  Row sums
// as above into slot z; an off-diagonal tile's column sums (the terms of the
// unwritten tile (J, I)) go to slot rparts + I at rows of J -- one slot per
// stored tile row, summed by the finish for I < J in order.  The diagonal
// tile counts once, without its diagonal.
template <class Ix, class PL>
__device__ __forceinline__ void sweep_sym(const float* __restrict__ D, Ix n_pad, Ix n, int rparts,
                                          float* __restrict__ P, PL& pl) {
  __shared__ float red[4][2][128];
  const int t = threadIdx.x, cq = t & 3, r0 = t >> 2, lane = t & 63, wv = t >> 6;
  const Ix I = blockIdx.x;
  const int z = blockIdx.y;
  const Ix T = n_pad >> 7, pcols = n_pad >> 4, len = T - I;
  const Ix J0 = I + (Ix)((int64_t)len * z / rparts), J1 = I + (Ix)((int64_t)len * (z + 1) / rparts);
  const Ix i0 = I * 128 + r0;
  const bool rv0 = i0 < n, rv1 = i0 + 64 < n;
  pl.rows(i0);
  const bool pads = n < n_pad;
  const f32x4* Dp = reinterpret_cast<const f32x4*>(D) + (int64_t)I * pcols * (kSweepPanel / 4) + t;
  float* Pc = P + (int64_t)(rparts + I) * 2 * n_pad;
  // the lane's result of col_reduce8: quantity and column within a panel
  const int cqty = (lane >> 2) & 1;
  const int ccol = 4 * cq + 2 * ((lane >> 3) & 1) + ((lane >> 4) & 1);
  float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
  for (Ix J = J0; J < J1; ++J) {
    const bool diag = J == I;
    const bool tedge = diag || (pads && (I == T - 1 || J == T - 1));
#pragma unroll 2
    for (int p = 0; p < 8; ++p) {
      const Ix c = J * 8 + p;
      const f32x4 v0 = Dp[(int64_t)c * (kSweepPanel / 4)];
      const f32x4 v1 = Dp[(int64_t)c * (kSweepPanel / 4) + 256];
      const typename PL::extra x = pl.load(c, cq);
      const Ix j0 = 16 * c + 4 * cq;
      const bool edge = tedge || pl.edge(c);
      float cv[8];
      if (edge)
        pl.template panel<true, true>(v0, v1, x, c, i0, j0, rv0, rv1, n, s00, s01, s10, s11, cv);
      else
        pl.template panel<false, true>(v0, v1, x, c, i0, j0, rv0, rv1, n, s00, s01, s10, s11, cv);
      if (!diag) {  // block-uniform
        const float y = col_reduce8(cv, lane);
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
  sweep_store(P + (int64_t)z * 2 * n_pad, i0, n_pad, s00, s01, s10, s11);
}

// The finish kernels' opening, for the 64 rows from ib of a workgroup: wave w
// adds the slots w, w + 4, .. of the rows (coalesced, fp64) into s0[w], s1[w];
// after it sum4(s0, r), sum4(s1, r) are row ib + r's two sums, the four wave
// sums added in order.  Symmetric layout: slots [0, rparts) the row sums, then
// one per stored tile row I < this row's tile (the 64 rows share a tile).
template <class Ix>
__device__ __forceinline__ void slot_sums(const float* __restrict__ P, Ix m_pad, Ix m, Ix ib,
                                          int sym, int parts, double (&s0)[4][64],
                                          double (&s1)[4][64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nslots = sym ? parts - (int)(m_pad >> 7) + (int)(ib >> 7) : parts;
  const Ix i = ib + lane;
  double a = 0.0, b = 0.0;
  if (i < m) {
#pragma unroll 4
    for (int sl = wv; sl < nslots; sl += 4) {
      const float* Ps = P + (int64_t)sl * 2 * m_pad;
      a += (double)Ps[i];
      b += (double)Ps[m_pad + i];
    }
  }
  s0[wv][lane] = a;
  s1[wv][lane] = b;
  __syncthreads();
}
__device__ __forceinline__ double sum4(const double (&s)[4][64], int r) {
  return ((s[0][r] + s[1][r]) + s[2][r]) + s[3][r];
}

// The second level, one workgroup: thread t adds the workgroups' sums t,
// t + 256, .. of each of the Q quantities in order, then a fixed halving
// tree; thread 0 returns with the totals in tot.
template <int Q, class Ix>
__device__ __forceinline__ void block_totals(const double* __restrict__ ws, Ix nb, double* tot) {
  __shared__ double sh[Q][256];
  const int t = threadIdx.x;
  double s[Q] = {};
  for (Ix b = t; b < nb; b += 256) {
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] += ws[Q * (int64_t)b + q];
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) sh[q][t] = s[q];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int q = 0; q < Q; ++q) sh[q][t] += sh[q][t + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) tot[q] = sh[q][0];
}

}  // namespace dsvgd
