// phi_w2.hpp -- the one-operand phi_mm (C = exp-fused K . W, W = S - (2/h) Xc
// over 256-column blocks of the FmtH2 image) on a 256-ROW x 256-column block:
// phi_w1's machinery (phi_w1.hpp: one wave per SIMD, B fragments straight
// from the image, the staged A image alone in LDS, branch-free K-steps) with
// the four waves as 2 x 2, each 128 x 128 (256 accumulators).
//
// Why: with one operand a 128-row block has only 24 MFMAs per wave per K-step
// behind which to hide the staging of its D entries (exp2, diagonal select,
// row sum, two-part split: n^2 entries whatever the operand's width).  Here a
// K-step keeps 48 MFMAs per wave and phi_w1's LDS fragment traffic per MFMA
// (each wave reads only its own 128 rows of the staged image); each thread
// stages 16 D entries per K-step (rows t / 2 and 128 + t / 2 of the block),
// and the image is walked by half as many row blocks.
//
// Rows: D has a_rows (a multiple of 128) rows, the block 256: a second half
// at or past a_rows loads through an empty buffer resource (zeros) and stores
// nothing.  Symmetric layout (DS 4): only tiles (I, J), J >= I, are stored,
// so the block's second half reads the eight K-steps under the first half's
// diagonal tile transposed, from tile (I, I + 1), while the first half is
// already on its plain ones: three phases (both transposed, mixed, both plain).
#pragma once
#include "phi_w1.hpp"

namespace dsvgd {

struct PhiW2 {
  static constexpr int kThreads = 256;
  static constexpr int BM = 256, BC = 256, BJ = 16, P = 2;
  static constexpr int SA = P * BM * 32;  // one stage's A image (16 KiB)
  static constexpr int kSmemBytes = 2 * SA;
};

// staging VALU placed after each of a K-step's first kW2Mf MFMAs
#ifndef DSVGD_W2_SGB
#define DSVGD_W2_SGB 6
#endif
#ifndef DSVGD_W2_MF
#define DSVGD_W2_MF 40
#endif
constexpr int kW2Sgb = DSVGD_W2_SGB, kW2Mf = DSVGD_W2_MF;

// DS 0: the full D layout (row block of m rows from row0, K range [kchunk z,
// +kchunk)); DS 4: the symmetric layout (m == n, row0 == 0), slice z of a row
// block walks its K range ascending.  xm: slices mapped to XCDs (phi_w1 xmap).
template <int DS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void phi_w2_kernel(
    const float* A, int64_t a_npad, int64_t a_rows, const _Float16* Wh, int64_t ldw, int64_t K,
    int64_t kchunk, const dsvgd_select_state* __restrict__ st, float* __restrict__ C, int64_t ldc,
    float* __restrict__ rowsum, int64_t m, int64_t row0, const float* __restrict__ colinv,
    const float* __restrict__ gate, int xm) {
  static_assert(DS == 0 || DS == 4, "DS: 0 (full layout) or 4 (symmetric, one launch)");
  if (gate && *gate != 0.f) return;  // the range guard handed the step to the fallback
  using F = FmtH2;
  using V8 = F::V8;
  constexpr int P = PhiW2::P, BM = PhiW2::BM;
  constexpr bool SYM = DS == 4;
  __shared__ __attribute__((aligned(16))) char smem[PhiW2::kSmemBytes + (SYM ? 8 * PhiW1::kScrBytes : 0)];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wc = w & 1;
  // block -> (column block, row block, slice); xm as phi_w1_kernel's
  const int64_t lid = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int64_t xu = (lid >> 3) * (8 / gridDim.z) + (lid & 7) / gridDim.z;
  const int64_t cbx = xm ? xu % gridDim.x : blockIdx.x;
  const int64_t by = xm ? xu / gridDim.x : blockIdx.y;
  const int64_t bz = xm ? (lid & 7) % gridDim.z : blockIdx.z;
  const int64_t i0 = by * BM;
  const int64_t c0 = cbx * PhiW2::BC + wc * 128;
  const int64_t kb0 = bz * kchunk, kend = min(K, kb0 + kchunk);
  const int ks0 = (int)(kb0 / PhiW2::BJ);
  const int nsteps = kend > kb0 ? (int)((kend - kb0) / PhiW2::BJ) : 0;
  C += bz * m * ldc;
  rowsum += bz * roundup128(m);
  const float scale = -st->inv_h * kLog2e;
  // the halves that exist (the first always does: i0 < a_rows)
  const bool live1 = i0 + 128 < a_rows;
  const int64_t pcols = a_npad >> 4;
  const __amdgpu_buffer_rsrc_t rD0 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(A + (i0 >> 7) * pcols * kPanelElems), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rD1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(A + ((i0 >> 7) + (live1 ? 1 : 0)) * pcols * kPanelElems), (short)0,
      live1 ? 0x7fffffff : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB =
      __builtin_amdgcn_make_buffer_rsrc((void*)(Wh + c0 * 16), (short)0, 0x7fffffff, 0x00020000);
  const int pstride = (int)(ldw * 32);
  const int vB = x3_off(r, h);
  const int vD = t * 32;
  const int srow = t >> 1, shalf = t & 1;
  const int aoff = x3_off(srow, shalf);   // (half 1: + 128 * 32, the same swizzle)
  auto diag0 = [&](int kfirst, int hb) {
    const int64_t dg = row0 + i0 + 128 * hb + srow - 8 * shalf - (int64_t)kfirst * PhiW2::BJ;
    return (int)max(min(dg, (int64_t)(1 << 30)), (int64_t)-(1 << 30));
  };

  f32x16 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mi][ni][q] = 0.f;
  float rs0 = 0.f, rs1 = 0.f;

  // transposed loads (phi_w1_kernel DS 1): lane (piece t >> 5, s = t & 31)
  // loads rows 16 piece + 8 (s & 1) .. +7 of column j0 + (s >> 1) of a half
  const int symI = (int)(i0 >> 7);
  const int vP = (t >> 5) * kPanelElems * 4 + (t & 31) * 32;
  float* const scr0 = reinterpret_cast<float*>(smem + PhiW2::kSmemBytes + w * PhiW1::kScrBytes);
  float* const scr1 = scr0 + 4 * (PhiW1::kScrBytes / 4);
  const int sw_off = ((lane & 31) >> 1) * PhiW1::kScrLd + 16 * (lane >> 5) + 8 * (lane & 1);
  const int sr_off = 8 * shalf * PhiW1::kScrLd + (lane >> 1);

  // one phase: nsteps K-steps from global K-step ks0; half hb transposed (TRh)
  // or plain; qd0 / qd1: the halves' diagonal offsets at the phase's first step
  auto phase = [&](auto TR0_, auto TR1_, const int ks0, const int nsteps, const int qd0,
                   const int qd1) {
    constexpr bool TR0 = decltype(TR0_)::value, TR1 = decltype(TR1_)::value;
    if (nsteps <= 0) return;
    V8 b[4][P];
    f32x4 dr[4][2][2];   // D values: K-step k in dr[k & 3][half], loaded 3 K-steps ahead
    f32x4 tr[2][2];      // transposed halves: K-step k + 1's values
    const int last = nsteps - 1;
    auto loadB = [&](int ni, int k) {
      const int soff = (ks0 + min(k, last)) * P * pstride;
#pragma unroll
      for (int p = 0; p < P; ++p)
        b[ni][p] = __builtin_bit_cast(V8, w1_load(rB, vB + ni * 1024, soff + p * pstride));
    };
    auto loadD = [&](f32x4 (&d)[2][2], int k) {
      const int64_t j0 = (int64_t)(ks0 + min(k, last)) * PhiW2::BJ;
      const int soff = (int)(j0 >> 4) * kPanelElems * 4;
      auto one = [&](auto TR_, int hb, f32x4 (&o)[2]) {
        if constexpr (decltype(TR_)::value) {
          const bool ok = hb == 0 || live1;
          const float* src = A + (((j0 >> 7) * pcols + (symI + (ok ? hb : 0)) * 8) * kPanelElems +
                                  (j0 & 127) * 16);
          const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc(
              (void*)src, (short)0, ok ? 0x7fffffff : 0, 0x00020000);
          o[0] = w1_load_nt(rT, vP, 0);
          o[1] = w1_load_nt(rT, vP + 16, 0);
        } else {
          o[0] = w1_load_nt(hb ? rD1 : rD0, vD, soff);
          o[1] = w1_load_nt(hb ? rD1 : rD0, vD + 16, soff);
        }
      };
      one(TR0_, 0, d[0]);
      one(TR1_, 1, d[1]);
    };
    auto transpose = [&](float* scr, const f32x4 (&d)[2], f32x4 (&o)[2]) {
      *reinterpret_cast<f32x4*>(scr + sw_off) = d[0];
      *reinterpret_cast<f32x4*>(scr + sw_off + 4) = d[1];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q >> 2][q & 3] = scr[sr_off + q * PhiW1::kScrLd];
    };
    // exp2 / diagonal / row sum / 2-part split of 8 values of one half -> stage
    auto stage = [&](char* st_, const f32x4 (&d)[2], int k, bool tr_, int qd0_, float& rs) {
      const int qd = max(min(qd0_ - k * PhiW2::BJ, 8), -1);
      float e[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float v = q < 4 ? d[0][q] : d[1][q - 4];
        const float x = __builtin_amdgcn_exp2f(fmaf(v, scale, F::kAScaleLog2));
        e[q] = (!tr_ && qd == q) ? 0.f : x;
      }
      const float s = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
      rs += k <= last ? s : 0.f;
      V8 p0, p1;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const _Float16 a0 = (_Float16)e[q];
        p0[q] = a0;
        p1[q] = (_Float16)(e[q] - (float)a0);
      }
      *reinterpret_cast<V8*>(st_ + aoff) = p0;
      *reinterpret_cast<V8*>(st_ + BM * 32 + aoff) = p1;
    };
    auto stage2 = [&](char* st_, const f32x4 (&d)[2][2], int k) {
      if constexpr (TR0) stage(st_, tr[0], k, true, qd0, rs0);
      else stage(st_, d[0], k, false, qd0, rs0);
      if constexpr (TR1) stage(st_ + 128 * 32, tr[1], k, true, qd1, rs1);
      else stage(st_ + 128 * 32, d[1], k, false, qd1, rs1);
    };
    auto barrier = []() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    // K-step k from stage cur: A(k+1) -> stage nxt; MFMAs column tile by
    // column tile, each tile's B reloaded for k+1; then D(k+3) (a transposed
    // half stages tr = K-step k+1 and transposes dt = D(k+2) into tr)
    auto step = [&](int k, const char* cur, char* nxt, const f32x4 (&ds_)[2][2],
                    f32x4 (&dl)[2][2], const f32x4 (&dt)[2][2]) {
      V8 a[4][P];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int p = 0; p < P; ++p)
          a[mi][p] = *reinterpret_cast<const V8*>(cur + p * BM * 32 +
                                                  x3_off(wr * 128 + mi * 32 + r, h));
      stage2(nxt, ds_, k + 1);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        // small terms first, as mfma_products
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi][ni] = mfma_fmt<F>(a[mi][1], b[ni][0], acc[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi][ni] = mfma_fmt<F>(a[mi][0], b[ni][1], acc[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi][ni] = mfma_fmt<F>(a[mi][0], b[ni][0], acc[mi][ni]);
        loadB(ni, k + 1);
      }
      if constexpr (TR0) transpose(scr0, dt[0], tr[0]);
      if constexpr (TR1) transpose(scr1, dt[1], tr[1]);
      // the schedule (cdna_hip_programming.md T19): the 8 A fragment reads,
      // then kW2Mf MFMAs each followed by up to kW2Sgb staging VALU, the four
      // stage stores, and the rest of the 48 MFMAs with the B loads (and a
      // transposed half's scratch traffic) among them
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
      for (int i = 0; i < kW2Mf; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, kW2Sgb, 0);
        if (i % 12 == 11) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 4, 0);
#pragma unroll
      for (int i = kW2Mf; i < 48; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i % 12 == 11) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
      }
      loadD(dl, k + 3);
    };

    // prologue: B(0), D(0..2); A(0) -> stage 0 (transposed halves: D(0), D(1))
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) loadB(ni, 0);
    loadD(dr[0], 0);
    loadD(dr[1], 1);
    loadD(dr[2], 2);
    if constexpr (TR0) transpose(scr0, dr[0][0], tr[0]);
    if constexpr (TR1) transpose(scr1, dr[0][1], tr[1]);
    stage2(smem, dr[0], 0);
    if constexpr (TR0) transpose(scr0, dr[1][0], tr[0]);
    if constexpr (TR1) transpose(scr1, dr[1][1], tr[1]);
    barrier();
    for (int k = 0; k < nsteps; k += 4) {
      step(k, smem, smem + PhiW2::SA, dr[1], dr[3], dr[2]);
      barrier();
      if (k + 1 >= nsteps) break;
      step(k + 1, smem + PhiW2::SA, smem, dr[2], dr[0], dr[3]);
      barrier();
      if (k + 2 >= nsteps) break;
      step(k + 2, smem, smem + PhiW2::SA, dr[3], dr[1], dr[0]);
      barrier();
      if (k + 3 >= nsteps) break;
      step(k + 3, smem + PhiW2::SA, smem, dr[0], dr[2], dr[1]);
      barrier();
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  if constexpr (SYM) {
    // transposed up to the block's first row, the mixed eight K-steps under
    // the first half's diagonal tile, then plain; each clipped to the slice
    const int kse = ks0 + nsteps;
    const int ka = min(max(ks0, (int)(i0 >> 4)), kse), kb = min(max(ks0, (int)(i0 >> 4) + 8), kse);
    phase(T_{}, T_{}, ks0, ka - ks0, 0, 0);
    phase(F_{}, T_{}, ka, kb - ka, diag0(ka, 0), 0);
    phase(F_{}, F_{}, kb, kse - kb, diag0(kb, 0), diag0(kb, 1));
  } else {
    phase(F_{}, F_{}, ks0, nsteps, diag0(ks0, 0), diag0(ks0, 1));
  }

  // epilogue: C = acc * colinv * 2^-15; row sums by column block 0
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int64_t col = c0 + ni * 32 + r;
      const float cs = colinv[col] * (1.f / F::kAScale);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = i0 + wr * 128 + mi * 32 + c_row(q, lane);
        if (row < m) C[row * ldc + col] = acc[mi][ni][q] * cs;
      }
    }
  {
    const float v0 = rs0 + __shfl_xor(rs0, 1, 64), v1 = rs1 + __shfl_xor(rs1, 1, 64);
    if (cbx == 0 && shalf == 0) {
      if (i0 + srow < m) rowsum[i0 + srow] = v0 * (1.f / F::kAScale);
      if (i0 + 128 + srow < m) rowsum[i0 + 128 + srow] = v1 * (1.f / F::kAScale);
    }
  }
}

}  // namespace dsvgd
