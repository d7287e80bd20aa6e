// gram_sr.hpp -- the FmtH2 distance Gram with the row strip's image resident
// in LDS ("strip-resident"), for padded depths of exactly 16 K-steps (d <= 256).
//
// gram_rs_kernel (gram_rs.hpp) pushes a strip's A image (128 rows x 256 k x
// two fp16 parts = 128 KiB, the same for every column tile the strip meets)
// through a 3 x 8 KiB LDS ring once per 128 x 256 unit -- a block-wide barrier
// per K-step, LDS-DMA pieces among the MFMAs -- and hands every accumulator
// to an epilogue wave through 128 KiB of LDS with two more barriers per tile.
// At d <= 256 the whole image of a strip fits in LDS, so here:
//   * one 512-thread block per CU takes one 128-row strip at a time, copies
//     its image (16 K-steps x 8 KiB, the swizzled per-K-step layout gram_w1 /
//     gram_rs read fragments from) into LDS once, between two barriers; no
//     block-wide barrier follows until the strip is finished;
//   * all eight waves are the same kind of wave.  A wave owns 128 x 64 tiles
//     (the strip against 64 columns, 128 accumulators) and takes every 8th
//     of the strip's kept column tiles, from the right end of the strip.  Per
//     tile: 16 K-steps of 24 MFMAs in gram_w1's fragment and product order
//     (D keeps its bits), A fragments from the resident image, B fragments by
//     its own direct loads one K-step ahead; then gram_w1's epilogue straight
//     from its own accumulators (D value, bracket accounting, permlane
//     pairing, 16-byte nt stores of whole panel lines);
//   * the two waves of a SIMD overlap only while one is in its MFMA phase and
//     the other in its epilogue, and started together they stay together:
//     waves 4-7 begin when their SIMD's first wave reaches K-step 8 of its
//     first tile (an LDS word per SIMD, polled with s_sleep; kStagger);
//   * the next tile's first B fragments are loaded at the last K-step, before
//     the epilogue, so the MFMA phase starts when the epilogue ends.
// Tiles that are not kept (below the diagonal of the symmetric layout, past
// the padded matrix) are never visited.
//
// The walk: block b (XCD-major: the CUs of one XCD hold adjacent strips and,
// walking from the right end in step, meet the column tiles in the same
// order) takes strip b from the front, then strip Tm - 1 - b from the back,
// then the next round: on the symmetric layout a front strip and its back
// strip together hold the same number of kept tiles for every block.
//
// Candidate slots keep the unit numbering of GramUnitWalk (slot_base + 4 L +
// w for unit L = (strip, column pair) and 64-column quarter w), so the host's
// slot count and the select passes are those of gram_rs / gram_w1; the block
// that takes a strip zeroes the counts of that strip's slots it does not
// visit.  The slots' content is the same set in another order.
//
// LDS (one array): 128 KiB image | 8 x 512 B column norms / scales | 8 x 3 KiB
// candidate stage (depth 12 per lane, flushed when a lane passes 4) | 4
// stagger words | 1 KiB row norms / scales = 160 832 B.  Registers: 128
// accumulators, 32 + 32 for two A fragment sets, 32 for a two-deep B ring
// (256, waves_per_eu 2; the row norms / scales stay in LDS: in registers
// through the MFMA phase they spilled inside the tile loop).
#pragma once
#include "gram_w1.hpp"

namespace dsvgd {

struct GramSR {
  static constexpr int kThreads = 512;
  static constexpr int BM = 128;
  static constexpr int kSteps = 16;                    // K-steps (padded depth 256)
  static constexpr int SA = 2 * BM * 32;               // one K-step of the strip's image (8 KiB)
  static constexpr int kColOff = kSteps * SA;          // per wave: [norm | 1/s][64 columns]
  static constexpr int kCandDepth = 12;
  static constexpr int kCandOff = kColOff + 8 * 2 * 64 * 4;
  static constexpr int kFlagOff = kCandOff + 8 * 64 * kCandDepth * 4;
  static constexpr int kRowOff = kFlagOff + 64;          // the strip's rows: [norm | 2/s][128]
  static constexpr int kSmemBytes = kRowOff + 2 * BM * 4;
  // flags (dsvgd_gram_set_rs 2 / 3 / 4)
  static constexpr int kStagger = 1;   // waves 4-7 start half a tile late
  static constexpr int kPrio = 2;      // priority 1 in the MFMA phase
};
static_assert(GramSR::kSmemBytes <= 160 * 1024, "gram_sr LDS");

// Strips [0, Tm) of the owned rows [row0, row0 + m) against the global column
// pairs [jp_off, jp_off + Tc) (256 columns each); SYM: upper-triangle tiles
// only, weight 2 off the diagonal.  G: the strips per group of the slot
// numbering (GramUnitWalk).
template <int smode, bool SYM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gram_sr_kernel(
    const _Float16* __restrict__ Yg, int64_t img_rows, const float* __restrict__ norms,
    const float* __restrict__ rsc, int64_t row0, int64_t m, int64_t n, int64_t n_pad,
    float* __restrict__ D, dsvgd_select_state* __restrict__ st, float* __restrict__ cand, int Tm,
    int Tc, int jp_off, int G, int64_t slot_base, int64_t ns_total, int flags) {
  using V8 = FmtH2::V8;
  constexpr bool kBr = smode == kSelBracket;
  __shared__ __attribute__((aligned(16))) char smem[GramSR::kSmemBytes];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int T = (int)(n_pad >> 7);  // 128-column tiles of the padded matrix
  const bool stagger = (flags & GramSR::kStagger) != 0, prio = (flags & GramSR::kPrio) != 0;

  SlotLayout sl(cand, ns_total, kBr ? st->cand_cap : 0);
  if (kBr) sl.publish(st, blockIdx.x);
  const GramUnitWalk walk(Tm, Tc, SYM, G);
  const int WG = walk.G;

  // blocks in XCD-major order: XCD x holds b = x U .. x U + U - 1
  const int nb = (int)gridDim.x, U = nb / kXcds;
  const int b = (int)blockIdx.x < U * kXcds ? (int)(blockIdx.x % kXcds) * U + (int)(blockIdx.x / kXcds)
                                            : (int)blockIdx.x;

  // the kept 64-column tiles of strip I: [c_lo, c_hi) (global index c: columns 64 c ..)
  const int c_hi = min((jp_off + Tc) * 4, 2 * T);
  auto c_lo_of = [&](int I) { return SYM ? max(2 * I, jp_off * 4) : jp_off * 4; };

  // the slots of strip I's units that no wave visits: empty counts
  auto zero_slots = [&](int I) {
    if constexpr (kBr) {
      const int g = I / WG;
      int64_t goff = 0;
      for (int gg = 0; gg < g; ++gg) goff += walk.count(gg);
      const int j0 = walk.j0(g), nj = Tc - j0;
      const int c_lo = c_lo_of(I);
      for (int idx = t; idx < nj * 4; idx += GramSR::kThreads) {
        const int w = idx & 3, c = (j0 + (idx >> 2) + jp_off) * 4 + w;
        const bool kept = I < Tm && c >= c_lo && c < c_hi;
        if (!kept) {
          const int64_t slot = slot_base + (goff + (int64_t)(idx >> 2) * WG + (I % WG)) * 4 + w;
          sl.cnt[slot] = 0u;
          sl.below[slot] = 0u;
        }
      }
    }
  };
  // phantom strips of the last group (numbered by the walk, no rows)
  for (int ph = Tm + b; ph < walk.ng * WG; ph += nb) zero_slots(ph);

  const int pstride = (int)(img_rows * 32);  // bytes of one part of one image K-step
  const int vB = x3_off(r, h);
  float* const colbase = reinterpret_cast<float*>(smem + GramSR::kColOff) + wv * 128;
  float* const cstage =
      reinterpret_cast<float*>(smem + GramSR::kCandOff) + wv * 64 * GramSR::kCandDepth;
  float* const rowtab = reinterpret_cast<float*>(smem + GramSR::kRowOff);
  volatile uint32_t* const sflag = reinterpret_cast<volatile uint32_t*>(smem + GramSR::kFlagOff);

  // the bracket is fixed for the launch
  uint32_t klo0 = 0x7FFFFFFFu, kspan0 = 0u;
  if constexpr (kBr) {
    const float blo = st->lo, bhi = st->hi;
    const bool ok = bhi >= blo && blo >= 0.f;  // as SlotWriterLdsT::begin
    klo0 = ok ? __float_as_uint(blo) : 0x7FFFFFFFu;
    kspan0 = ok ? __float_as_uint(bhi) - klo0 : 0u;
  }

  V8 af[2][4][2];
  V8 rb[2][2][2];  // [ring][bj][part]
  f32x16 acc[4][2];
  auto read_frags = [&](V8 (&a)[4][2], const char* st_) {
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        a[bi][p] = *reinterpret_cast<const V8*>(st_ + p * GramSR::BM * 32 + x3_off(32 * bi + r, h));
  };
  auto load_B = [&](int sb, int ks, int c) {  // K-step ks of column tile c
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(Yg + (int64_t)c * 64 * 16), (short)0, 0x7fffffff, 0x00020000);
    const int so = ks * 2 * pstride;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        rb[sb][bj][p] = __builtin_bit_cast(V8, gw1_load(rB, vB + bj * 1024, so + p * pstride));
  };

  for (int it = 0;; ++it) {
    const int k2 = it >> 1, back = it & 1;
    if (2 * k2 * nb >= Tm) break;
    const int I = __builtin_amdgcn_readfirstlane(back ? Tm - 1 - k2 * nb - b : k2 * nb + b);
    const bool mine = back ? I >= (k2 + 1) * nb : I <= Tm - 1 - k2 * nb;
    if (!mine) continue;  // block-uniform

    // ---- the strip: its image into LDS, its rows' data into registers ----
    __syncthreads();  // every wave is past its reads of the previous image
    {
      const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(Yg + (row0 + (int64_t)I * 128) * 16), (short)0, 0x7fffffff, 0x00020000);
      // thread t: 16-byte chunk t & 255 of part t >> 8 of every K-step
      const int p = t >> 8, ch = (t & 255) * 16, vA = ch + p * pstride;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = gw1_load(rA, vA, (half * 8 + k) * 2 * pstride);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          *reinterpret_cast<f32x4*>(smem + (half * 8 + k) * GramSR::SA + p * GramSR::BM * 32 + ch) =
              v[k];
      }
      if (t < 4) sflag[t] = 0u;
    }
    zero_slots(I);
    const int64_t gi0 = row0 + (int64_t)I * 128;
    // row norms (+inf: padding) and 2 / s_i, read per slice (the MFMA phase
    // has no registers to spare for them)
    if (t < GramSR::BM) {
      const int64_t il = (int64_t)I * 128 + t;  // row within the owned block
      const bool ok = il < m;
      rowtab[t] = ok ? norms[row0 + il] : INFINITY;
      rowtab[GramSR::BM + t] = 2.f * pow2_inv(ok ? rsc[row0 + il] : 1.f);
    }
    __syncthreads();  // the image has landed

    // ---- the wave's tiles: c_hi - 1 - wv, then every 8th down to c_lo ----
    const int c_lo = c_lo_of(I);
    int c = c_hi - 1 - wv;
    if (c < c_lo) continue;  // (wave-uniform; the barriers are at the strip's head)
    load_B(0, 0, c);
    if (stagger && wv >= 4) {
      // wave wv - 4 has a tile whenever this one has; bounded all the same
      for (int spin = 0; spin < 4096 && sflag[wv - 4] == 0u; ++spin) __builtin_amdgcn_s_sleep(8);
    }
    bool first = true;
    for (;;) {
      const int cn = c - 8;
      const bool has_next = cn >= c_lo;
      // the tile's column data (lane: column 64 c + lane), to LDS after the MFMAs
      const int64_t j = (int64_t)c * 64 + lane;
      const float pcn = j < n ? norms[j] : INFINITY;
      const float pcs = j < n ? rsc[j] : 1.f;
      read_frags(af[0], smem);
      if (prio) __builtin_amdgcn_s_setprio(1);
      // one K-step: 24 MFMAs in gram_w1's order (product p of block idx % 8,
      // consecutive MFMAs independent); the next step's B in the first
      // group, the next step's fragments at mid-step
      auto step = [&](auto K_) {
        constexpr int K = decltype(K_)::value;
        V8 (&a)[4][2] = af[K & 1];
#pragma unroll
        for (int grp = 0; grp < 8; ++grp) {
#pragma unroll
          for (int qq = 0; qq < 3; ++qq) {
            const int idx = 3 * grp + qq, p = idx / 8, bi = (idx % 8) >> 1, bj = idx & 1;
            const f32x16 cc = (p == 0 && K == 0) ? f32x16{} : acc[bi][bj];
            const V8 bx = rb[K & 1][bj][p == 1 ? 1 : 0];
            const V8 ax = a[bi][p == 0 ? 1 : 0];
            acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bx, ax, cc, 0, 0, 0);
          }
          if (grp == 0) {
            if constexpr (K + 1 < GramSR::kSteps)
              load_B((K + 1) & 1, K + 1, c);
            else
              load_B(0, 0, has_next ? cn : c);  // the next tile's first B, before the epilogue
          }
          if (grp == 3) {
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (K + 1 < GramSR::kSteps)
              read_frags(af[(K + 1) & 1], smem + (K + 1) * GramSR::SA);
            if constexpr (K == 8) {
              if (first && wv < 4) sflag[wv] = 1u;  // every lane stores the same word
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      };
#define DSVGD_GSR_STEP(KK) step(std::integral_constant<int, KK>{});
      DSVGD_GSR_STEP(0) DSVGD_GSR_STEP(1) DSVGD_GSR_STEP(2) DSVGD_GSR_STEP(3)
      DSVGD_GSR_STEP(4) DSVGD_GSR_STEP(5) DSVGD_GSR_STEP(6) DSVGD_GSR_STEP(7)
      DSVGD_GSR_STEP(8) DSVGD_GSR_STEP(9) DSVGD_GSR_STEP(10) DSVGD_GSR_STEP(11)
      DSVGD_GSR_STEP(12) DSVGD_GSR_STEP(13) DSVGD_GSR_STEP(14) DSVGD_GSR_STEP(15)
#undef DSVGD_GSR_STEP
      if (prio) __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);

      // ---- the epilogue, from the wave's own accumulators ----
      colbase[lane] = pcn;
      colbase[64 + lane] = pow2_inv(pcs);
      const int64_t gj0 = (int64_t)c * 64;
      const int Jt = c >> 1;
      float* dt = D + ((int64_t)I * (n_pad >> 4) + (int64_t)Jt * 8 + 4 * (c & 1)) * kPanelElems;
      const __amdgpu_buffer_rsrc_t rD =
          __builtin_amdgcn_make_buffer_rsrc((void*)dt, (short)0, 4 * kPanelElems * 4, 0x00020000);
      const bool ediag = gj0 + 64 > gi0 && gj0 < gi0 + 128;
      const bool ew2 = SYM && Jt != I;
      const int64_t J2 = (c >> 2) - jp_off;
      int64_t eslot = 0;
      GramSlotWriter<GramSR::kCandDepth> sw;
      if constexpr (kBr) {
        const int g = I / WG;
        int64_t goff = 0;
        for (int gg = 0; gg < g; ++gg) goff += walk.count(gg);
        eslot = slot_base + (goff + (J2 - walk.j0(g)) * WG + (I % WG)) * 4 + (c & 3);
        sw.klo = klo0;
        sw.kspan = kspan0;
        sw.dst = sl.data + eslot * sl.cap;
        sw.cap = (uint32_t)sl.cap;
        sw.stage = cstage + lane;
      }
      // slice SL: block (bi, bj) = (SL >> 2, (SL >> 1) & 1), register runs
      // g = 2 (SL & 1), + 1 -- gram_w1's slice() and store_slice()
      auto slice = [&](auto SL_) {
        constexpr int SL = decltype(SL_)::value;
        constexpr int bi = SL >> 2, bj = (SL >> 1) & 1;
        if constexpr (kBr) {
          // a slice stages at most 8 values per lane
          if (__ballot(sw.pos > (uint32_t)(GramSR::kCandDepth - 8)) != 0ull) sw.flush4();
        }
        const float nrv = rowtab[32 * bi + r], siv = rowtab[GramSR::BM + 32 * bi + r];
        f32x4 v[2];
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
          constexpr int g0 = 2 * (SL & 1);
          const int g = g0 + gg;
          const int co = 32 * bj + 4 * h + 8 * g;
          const f32x4 cnv = *reinterpret_cast<const f32x4*>(colbase + co);
          const f32x4 csv = *reinterpret_cast<const f32x4*>(colbase + 64 + co);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float a = acc[bi][bj][4 * g + e];
            v[gg][e] = fmaxf(0.f, (nrv + cnv[e]) - siv * (csv[e] * a));
            if constexpr (kBr) sw.add(v[gg][e]);
          }
        }
        if (!kBr && ediag) {
          // diagonal target: c_row(q) + 32 bj == tgv <=> i == j (padding rows: never)
          const int tgv = nrv != INFINITY ? (int)(gi0 - gj0) + 32 * bi + r - 4 * h : (1 << 30);
#pragma unroll
          for (int gg = 0; gg < 2; ++gg) {
            const int g = 2 * (SL & 1) + gg;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (tgv == e + 8 * g + 32 * bj) v[gg][e] = 0.f;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[0][e]),
                                                           __float_as_uint(v[1][e]), false, false);
          v[0][e] = __uint_as_float(sv[0]);
          v[1][e] = __uint_as_float(sv[1]);
        }
        const int vo = (32 * bi + (lane & 15)) * 64 + 16 * h + 32 * ((lane >> 4) & 1);
        constexpr int so = (2 * bj + (SL & 1)) * kPanelElems * 4;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[0]), rD, vo, so, 2);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[1]), rD, vo + 1024, so, 2);
        __builtin_amdgcn_sched_barrier(0);  // slice by slice: no 128 values live at once
      };
#define DSVGD_GSR_SLICE(KK) slice(std::integral_constant<int, KK>{});
      DSVGD_GSR_SLICE(0) DSVGD_GSR_SLICE(1) DSVGD_GSR_SLICE(2) DSVGD_GSR_SLICE(3)
      DSVGD_GSR_SLICE(4) DSVGD_GSR_SLICE(5) DSVGD_GSR_SLICE(6) DSVGD_GSR_SLICE(7)
      DSVGD_GSR_SLICE(8) DSVGD_GSR_SLICE(9) DSVGD_GSR_SLICE(10) DSVGD_GSR_SLICE(11)
      DSVGD_GSR_SLICE(12) DSVGD_GSR_SLICE(13) DSVGD_GSR_SLICE(14) DSVGD_GSR_SLICE(15)
#undef DSVGD_GSR_SLICE
      if constexpr (kBr) sw.finish_tile(sl, eslot, ew2);
      if (!has_next) break;
      c = cn;
      first = false;
    }
  }
}

}  // namespace dsvgd
