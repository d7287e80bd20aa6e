/*
 * dsvgd.h -- C ABI of libdsvgd_hip.so, the MI355X (gfx950) SVGD particle-update
 * engine behind the drop-in `dsvgd.Sampler` / `dsvgd.DistSampler` Python API.
 *
 * Conventions (every entry point):
 *   - plain pointers + int64 sizes; every float buffer is caller-owned DEVICE
 *     memory, row-major fp32, with an explicit leading dimension (elements);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only ENQUEUES work on it (no host sync, no allocation), so the whole
 *     SVGD step can be captured into a hipGraph;
 *   - return 0 on success, a negative DSVGD_E* code otherwise; the message is
 *     in dsvgd_last_error() (thread-local).  No C++ exception crosses the ABI.
 *
 * Padding contract ("padded shapes"): n_pad = roundup(n,128), m_pad =
 * roundup(m,128), dp = roundup(d,32); Y has >= n_pad+128 rows and ldy =
 * dsvgd_ldy(dp) columns; D is m_pad x n_pad (ldd >= n_pad).  The helpers
 * dsvgd_dp / dsvgd_ldy / dsvgd_pad128 compute these.
 *
 * The reference interface each call replaces is cited beside it
 * (paths relative to the Sandy4321/dist-svgd tree).
 */
#ifndef DSVGD_H_
#define DSVGD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSVGD_ABI_VERSION 4

enum {
  DSVGD_OK = 0,
  DSVGD_E_ARG = -1,    /* bad size / pointer / alignment                    */
  DSVGD_E_LAUNCH = -2, /* hipLaunchKernel (or a HIP runtime call) failed     */
  DSVGD_E_UNSUPPORTED = -3
};

/* number of histogram bins of one radix-select pass (11-bit digits) */
#define DSVGD_RADIX_BINS 2048
/* bracketed select: the candidate buffer (cand_cap floats) is split into one
 * fixed-capacity SLOT per wave of the distance launch, written without any
 * atomic or block barrier:
 *   cand[0 : nslots)            u32 slot_cnt   (entries in [lo,hi]; bit 31 =
 *                                               weight 2, a mirrored tile)
 *   cand[nslots : 2 nslots)     u32 slot_below (entries < lo, same weight)
 *   cand[2 nslots + s*slot_cap] the slot's values (slot_cap floats each)
 * with slot_cap = (cand_cap - 2 nslots) / nslots; a slot that fills up sets
 * `overflow` and the select falls back to the passes over D (still exact). */
#define DSVGD_SLOT_WEIGHT2 0x80000000u

/* Device-resident state of the median-bandwidth radix select.  Allocate
 * dsvgd_select_state_bytes() of device memory; the histogram is the first
 * member so a distributed caller can all-reduce it in place (int64 SUM), and
 * below_total / ncand_total / overflow are adjacent for one int64[3]
 * all-reduce (between dsvgd_bracket_totals and dsvgd_bracket_check). */
typedef struct dsvgd_select_state {
  uint64_t hist[DSVGD_RADIX_BINS]; /* per-pass counts (u64: n^2 may be 2^32)  */
  uint64_t k;                      /* rank still to find inside the prefix    */
  uint64_t n_total;                /* global particle count n (matrix n x n)  */
  uint32_t prefix;                 /* key bits fixed by the passes so far     */
  uint32_t passes_done;
  float median;                    /* k-th smallest squared distance          */
  float h;                         /* bandwidth  h = median / log(n)          */
  float inv_h;                     /* 1 / h (read by the phi kernels)         */
  uint32_t fallback;               /* bracketed: 1 = select over D itself     */
  uint64_t below_total;            /* bracketed: # entries < lo      } int64[3], */
  uint64_t ncand_total;            /* bracketed: # entries in [lo,hi] } all-     */
  uint64_t overflow;               /* bracketed: # overflowed slots  } reduced  */
  float lo, hi;                    /* bracketed: the sample bracket           */
  uint64_t cand_cap;               /* bracketed: candidate buffer floats      */
  uint64_t nslots;                 /* bracketed: slots of the last sqdist     */
  uint64_t slot_cap;               /* bracketed: floats per slot              */
} dsvgd_select_state;

/* select_mode of dsvgd_sqdist */
#define DSVGD_SEL_NONE 0    /* fixed bandwidth: distances only                 */
#define DSVGD_SEL_HIST 1    /* fused radix digit-1 histogram                   */
#define DSVGD_SEL_BRACKET 2 /* count < lo, compact [lo, hi] into candidates    */

/* ---- meta ------------------------------------------------------------- */
int dsvgd_abi_version(void);
const char* dsvgd_last_error(void);
size_t dsvgd_select_state_bytes(void);
int64_t dsvgd_pad128(int64_t n);
int64_t dsvgd_dp(int64_t d);   /* padded feature width: roundup(d, 32)     */
int64_t dsvgd_ldy(int64_t dp); /* row stride of Y = [Xc | S] (phi col tile) */

/* ---- particle preparation ---------------------------------------------- */
/* mean[c] = (1/n) sum_j X[j][c]  (deterministic two-level sum; `partial`
 * is workspace of dsvgd_colmean_workspace_floats(n, d) floats).
 * Centering is exact algebra for phi (sum_j k_ij (x_i - x_j) is translation
 * invariant) and keeps ||x||^2 - 2 x.y well conditioned. */
size_t dsvgd_colmean_workspace_floats(int64_t n, int64_t d);
int dsvgd_colmean(const float* X, int64_t ldx, int64_t n, int64_t d, float* partial, float* mean,
                  void* stream);
/* center[c] = the lower median of X[:, c] over min(n, 1024) evenly spaced rows
 * (row k n / m): the centre the engine packs against.  Robust where the mean
 * is not: one diverging particle moves the mean by its distance / n and every
 * other particle's |x|^2 + |y|^2 - 2 x.y (and r x - K X) cancellation with it. */
int dsvgd_colcenter(const float* X, int64_t ldx, int64_t n, int64_t d, float* center,
                    void* stream);

/* Y[j] = [X[j]-mean | score_scale*S[j]] zero padded to (rows_pad x ldy);
 * norms[j] = ||X[j]-mean||^2.  Replaces the per-pair operand gathering of
 * dsvgd/sampler.py:37-39 and dsvgd/distsampler.py:90-99.  S may be NULL
 * (S half left zero); X may be NULL (then only the S half of rows < n is
 * written: the scores arriving after the distance stage, mean/norms unused). */
int dsvgd_pack(const float* X, int64_t ldx, const float* S, int64_t lds, float score_scale,
               const float* mean, int64_t n, int64_t d, int64_t rows_pad, float* Y, int64_t ldy,
               float* norms, void* stream);
/* dsvgd_pack + the FmtH2 statistics of what it writes (ldy <=
 * dsvgd_pack_max_ldy() = 2048, i.e. d <= 1024): partial (uint32,
 * dsvgd_pack_blocks(rows_pad) x ldy column maxima) and gmax (4 words per
 * block: [4b] / [4b+1] the largest |entry| of the X half [0, dp) / of the
 * rest; [4b+2] / [4b+3] the smallest nonzero row max of each half over the
 * block's rows < n, +inf if none -- fp32 bit patterns), the input of
 * dsvgd_h2_scales -- the scales and the range guard without a second pass
 * over Y.  With X NULL only the S half's statistics are (re)written, so
 * pack(X) then pack(NULL, S) leaves those of the whole Y.  partial = gmax =
 * NULL: dsvgd_pack.  rowscale (nullable, rows_pad floats, with X): the FmtH2
 * power-of-two scale of each row's X half (largest magnitude -> [2^14,
 * 2^15); 1 for a zero row or a row >= n) -- the Gram's per-row image scales. */
int64_t dsvgd_pack_blocks(int64_t rows_pad);
int64_t dsvgd_pack_max_ldy(void);
int dsvgd_pack_h2(const float* X, int64_t ldx, const float* S, int64_t lds, float score_scale,
                  const float* mean, int64_t n, int64_t d, int64_t rows_pad, float* Y, int64_t ldy,
                  float* norms, uint32_t* partial, uint32_t* gmax, float* rowscale,
                  void* stream);

/* ---- pairwise squared distances ---------------------------------------- */
/* D[i][j] = ||y_i - y_j||^2 for the owned row block i in [row0, row0+m) of Y
 * against all j < n, y = the first d columns of Y (centred particles).
 * d <= 2: explicit differences on the VALU (exact like the reference);
 * d > 2: max(0, |y_i|^2 + |y_j|^2 - 2 y_i.y_j) on v_mfma_f32_32x32x2_f32,
 * upper-triangle tiles only when m == n and row0 == 0 (the transpose is
 * stored too).  D[i][i] = 0 exactly, pads = +inf, panel layout (ldd = n_pad).
 * select_mode (DSVGD_SEL_*): HIST accumulates radix digit 1 of the valid
 * entries into st->hist; BRACKET counts the entries < st->lo and writes the
 * entries in [st->lo, st->hi] into the wave slots of cand (layout above;
 * st->nslots / st->slot_cap are set by the launch).
 * Replaces torch.dist(x, y, p=2)**2 inside kernel(...) at
 * experiments/logreg.py:60-61 / experiments/gmm.py:23-24 as called per pair
 * from dsvgd/sampler.py:38 and dsvgd/distsampler.py:91-97. */
int dsvgd_sqdist(const float* Y, int64_t ldy, const float* norms, int64_t row0, int64_t m,
                 int64_t n, int64_t d, float* D, int64_t ldd, int select_mode,
                 dsvgd_select_state* st, float* cand, void* stream);
/* dsvgd_sqdist's explicit-difference kernel forced for any d <= 64 (the
 * precision studies of DESIGN.md 3; dsvgd_sqdist takes it for d <= 2). */
int dsvgd_sqdist_direct(const float* Y, int64_t ldy, const float* norms, int64_t row0, int64_t m,
                        int64_t n, int64_t d, float* D, int64_t ldd, int select_mode,
                        dsvgd_select_state* st, float* cand, void* stream);

/* ---- median bandwidth: exact radix select over the n x n distances ----- */
/* (absent in the reference, whose kernel bandwidth is fixed at h=1; the
 * median heuristic is pinned in SURVEY.md a18: lower median, k=(n^2-1)//2
 * over the full matrix incl. the diagonal, h = median / log n.)
 * select_init: k = k_rank if k_rank >= 0 else (n_total^2-1)/2, prefix 0. */
int dsvgd_select_init(dsvgd_select_state* st, int64_t n_total, int64_t k_rank, void* stream);
/* histogram of key digit `pass` (1: bits 31..21, 2: 20..10, 3: 9..0) of the
 * finite entries (pads +inf / NaN skipped) whose higher digits equal
 * st->prefix, over D[0:count) -- or, when cand != NULL and the bracket holds
 * (st->fallback == 0), over the local candidate slots instead.
 * sym_npad > 0: D is the symmetric layout dsvgd_sqdist_x3 writes with
 * layout = 1 (upper-triangle tiles only; count = sym_npad^2): off-diagonal
 * tiles count twice, lower tiles are skipped. */
int dsvgd_radix_hist(const float* D, int64_t count, const float* cand, int pass,
                     dsvgd_select_state* st, int64_t sym_npad, void* stream);
/* pick the bin holding rank k, fix its digit, clear hist; after pass 3
 * writes median, h = median/log(n_total) (1 if median == 0 or n == 1), inv_h. */
int dsvgd_radix_pick(dsvgd_select_state* st, int pass, void* stream);
/* bracketed select: out[p] = ||y_i - y_j||^2 for s pairs (i,j) drawn by a
 * seeded hash (identical on every rank for the same Y) ... */
int dsvgd_sample_sqdist(const float* Y, int64_t ldy, int64_t n, int64_t d, int64_t s,
                        uint64_t seed, float* out, void* stream);
/* ... whose k_lo-th / k_hi-th order statistics (two select states run over
 * `out`) become the bracket [lo, hi] of st (k = (n_total^2-1)/2) ... */
int dsvgd_bracket_init(dsvgd_select_state* st, int64_t n_total, const dsvgd_select_state* lo_st,
                       const dsvgd_select_state* hi_st, int64_t cand_cap, void* stream);
/* ... the same three steps (sample_sqdist into `sample`, both sample
 * selects, bracket_init of st) in seven launches: the two selects share each
 * sweep over the sample and one launch picks both digits.  lo_st / hi_st:
 * histograms zero on entry (as dsvgd_select_init or a previous call leave
 * them); they end as after the three passes.  s % 4 == 0, 16-byte aligned
 * sample, 0 <= k_lo <= k_hi < s. */
int dsvgd_sample_bracket(const float* Y, int64_t ldy, int64_t n, int64_t d, int64_t s,
                         uint64_t seed, int64_t k_lo, int64_t k_hi, float* sample,
                         dsvgd_select_state* lo_st, dsvgd_select_state* hi_st,
                         dsvgd_select_state* st, int64_t n_total, int64_t cand_cap,
                         void* stream);
/* dsvgd_sample_bracket in two parts (ABI 4): a rank's share of the sample --
 * dsvgd_sample_sqdist's pairs [p0, p1) of s, the same pairs and values --
 * and, once the shares are all-gathered into the whole sample, the selects
 * and the bracket (the last six launches of dsvgd_sample_bracket). */
int dsvgd_sample_sqdist_range(const float* Y, int64_t ldy, int64_t n, int64_t d, int64_t s,
                              uint64_t seed, int64_t p0, int64_t p1, float* out, void* stream);
int dsvgd_sample_bracket_select(const float* sample, int64_t s, int64_t k_lo, int64_t k_hi,
                                dsvgd_select_state* lo_st, dsvgd_select_state* hi_st,
                                dsvgd_select_state* st, int64_t n_total, int64_t cand_cap,
                                void* stream);
/* ... then, after dsvgd_sqdist(BRACKET): bracket_totals sums the slots into
 * below_total / ncand_total / overflow (a distributed caller all-reduces
 * those three int64), and bracket_check decides exactly: below <= k <
 * below + ncand and no slot overflowed -> k -= below, the passes read the
 * candidate slots; otherwise they read D (fallback). */
int dsvgd_bracket_totals(dsvgd_select_state* st, const float* cand, void* stream);
int dsvgd_bracket_check(dsvgd_select_state* st, void* stream);
/* fixed-bandwidth mode: st->h = h, st->inv_h = 1/h */
int dsvgd_set_bandwidth(dsvgd_select_state* st, float h, void* stream);

/* dsvgd_sqdist's Gram path (d > 2) on the split engine (fp32-accurate, see
 * dsvgd_phi_mm_x3): Yg = dsvgd_rowsplit(Y, ldy, n_pad, dp, n_pad + 256, dp, 0)
 * with dp = roundup(d, 32), n_pad = roundup(n, 128) (256 rows of zero slack
 * for the 256 x 256 tiles); same outputs and select
 * modes as dsvgd_sqdist.  layout 0: the full panel-layout D; layout 1 (m ==
 * n, row0 == 0 only) the SYMMETRIC LAYOUT: tiles (I, J) with J < I are not
 * written -- consumers read them transposed (dsvgd_phi_mm_x3 with sym = 1,
 * dsvgd_radix_hist with sym_npad).  Requires dp * (n_pad + 256) * 6 < 2^31. */
int dsvgd_sqdist_x3(const void* Yg, const float* norms, int64_t row0, int64_t m, int64_t n,
                    int64_t d, float* D, int64_t ldd, int select_mode, dsvgd_select_state* st,
                    float* cand, int layout, void* stream);

/* ---- phi: K.[Xc | S] on MFMA with the fused RBF exp -------------------- */
/* KY_z[i][:] = sum_{j in slice z, j != row0+i} exp(-D[i][j]/h) Y[j][:] and
 * rowsum_z[i] = the same sum of exp(-D[i][j]/h), for split-K slices z < splits
 * of the columns (h read from st on device; row0 = index of the block's first
 * row in the interacting set; the diagonal self term is added exactly by
 * dsvgd_phi_finish instead of being summed among ~n tiny terms).  KY holds splits x m rows (ldk >= ldy,
 * slice z at KY + z*m*ldk), rowsum splits x roundup(m,128) floats.
 * Replaces the inner loop of dsvgd/sampler.py:35-40 (_phi_hat) and
 * dsvgd/distsampler.py:84-101.  dsvgd_phi_splits gives a slice count that
 * fills the 256 CUs (>= 2 blocks per CU) for an m-row block.
 * Slice z covers the columns [z kchunk, min(n_pad, (z + 1) kchunk)), kchunk =
 * roundup(ceil(n_pad / splits), 16) (32 on the f32 engine).  `splits` is the
 * caller's: a slice past n_pad (z kchunk >= n_pad) is EMPTY and comes out as
 * exact zeros -- except in the symmetric layout's one-launch form
 * (dsvgd_phi_mm_h2 with sym = 1, ldy % 512 == 0, splits >= 2 under symrow 1,
 * and dsvgd_phi_mm_h2w with sym = 1), whose walk would step past n_pad there:
 * these refuse (splits - 1) kchunk >= n_pad with an error and launch nothing.
 * (The two-launch hybrid has no kchunk: it deals the 16-column K-steps out
 * round-robin, and a slice that gets none is exact zeros.) */
int64_t dsvgd_phi_splits(int64_t m, int64_t n, int64_t ldy);
/* The symmetric layout's phi_mm form (A/B switch, returns the previous
 * setting): 1 (default) = one launch, each row block's split-K slices walking
 * contiguous K ranges ascending, transposed K-steps first (phi_w1 DS 4);
 * 0 = two launches split at each row block's diagonal tile (DS 1 + DS 2). */
int dsvgd_phi_set_symrow(int on);
/* The one-kernel FmtH2 Gram units (dsvgd_sqdist_h2, dsvgd_sqdist_h2_parts):
 * 2 (default) = gram_sr_kernel where it applies -- the panel-layout D of
 * dsvgd_sqdist_h2 at a padded depth of 256 (16 K-steps), none / bracket
 * select: a block keeps its 128-row strip's whole image in LDS, every wave
 * computes 128 x 64 tiles and writes them out from its own accumulators, the
 * second wave of each SIMD starting half a tile late; gram_rs_kernel
 * everywhere else (deeper images, dsvgd_sqdist_h2_parts, dsvgd_w2_cost_h2).
 * 3, 4: the same without the stagger / without priority 1 in the MFMA phase
 * (A/B).
 * 1 = gram_rs_kernel, split roles -- four waves issue only the
 * MFMAs (and stage the strip image by LDS-DMA), four waves write the
 * previous tile's epilogue (D values, bracket accounting, stores) from an
 * LDS hand-off; 0 = gram_w1_kernel, one wave per SIMD with the epilogue
 * between its MFMAs.  Identical D and candidates.  5, 6, 7: timing probes of
 * the bracketed symmetric form only (5: no epilogue, 6: no MFMAs -- D wrong;
 * 7: epilogue waves at priority 1; 8: barrier clock stamps into the buffer
 * given to dsvgd_gram_debug_stamps; 9: the MFMA waves' B ring 4 deep).
 * Returns the previous setting. */
int dsvgd_gram_set_rs(int on);
/* The kernel the last launch of one-kernel Gram units ran on: 0
 * gram_w1_kernel, 1 gram_rs_kernel, 2 gram_sr_kernel.  dsvgd_sqdist_h2 and
 * dsvgd_sqdist_x3 reset it to -1 on entry, so -1 after one of them means the
 * call had no such units (roundup(d, 32) not a multiple of 256, the histogram
 * select: the 8-wave kernel).  For tests of the dispatch above. */
int dsvgd_gram_last_kernel(void);
/* CUs the persistent launches issued after this call leave free (returns
 * the previous; 0 = none): the pipelined Gauss-Seidel sweep sets it around
 * its side-stream passes so the walk (one workgroup, most of a CU's LDS)
 * finds a free CU beside them.  A launch-time host setting. */
int dsvgd_set_cu_reserve(int cus);
/* Strips per unit group of the split-role Gram's walk (A/B switch, returns
 * the previous setting): 8 (default) or 16.  Each group's strip images stay
 * in an XCD's L2 while every column pair's image streams past once. */
int dsvgd_gram_set_group(int g);
/* Probe 8 of dsvgd_gram_set_rs: int64 [8 blocks][8 waves][512] shader-clock
 * stamps, on arriving at and leaving each barrier (NULL: probe off). */
int dsvgd_gram_debug_stamps(void* buf);
/* The split-K slices of the symmetric layout's phi_mm (n x n, the engine's
 * KY / rowsum hold this many): dsvgd_phi_splits, or with the one-launch form
 * half as many while each fp32 chain stays within 2 x 16384 columns and the
 * launch has >= 512 blocks (n = 65536, d = 256: 2). */
int64_t dsvgd_phi_splits_sym(int64_t n, int64_t ldy);
/* Map a phi_mm launch's split-K slices to XCDs (A/B switch, returns the
 * previous mask): the blocks of one XCD then walk one K range and share its
 * Yx K-steps in their L2.  Bits: 1 = the symmetric layout's one-launch form
 * (default), 2 = the full layout / window launches, 4 = the pair split's
 * batched forward partials; grids of one column block whose slice count
 * divides 8 and whose block count 8 divides. */
int dsvgd_phi_set_xmap(int mask);
/* logreg's G . Xd on the FmtH2 engine with 256 output columns (p <= 255):
 * phi_w1's one-wave-per-SIMD shape in 128 x 256 blocks (1; measured slower)
 * or the 8-wave 256-row NN tile (0, default).  A/B switch; returns the
 * previous setting. */
int dsvgd_phi_set_gxd_w1(int on);
int dsvgd_phi_mm(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t row0,
                 int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits, float* KY,
                 int64_t ldk, float* rowsum, void* stream);
/* dsvgd_phi_mm gated on a device word: does nothing while *gate reads 0 --
 * the exact f32 fallback of dsvgd_phi_mm_h2 where the FmtX3 image does not
 * fit its 32-bit offsets (roundup(n,128) * ldy * 6 >= 2^31); full D layout
 * only (ABI 4). */
int dsvgd_phi_mm_gated(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t row0,
                       int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits,
                       float* KY, int64_t ldk, float* rowsum, const float* gate, void* stream);

/* phi_mm on the bf16 MFMA at fp32 accuracy (the default engine): both
 * operands split three ways into bf16 (v = v0 + v1 + v2 to ~2^-26 |v|) and
 * the six products a_i b_j with i + j <= 2 accumulated in fp32, so the
 * result carries fp32 GEMM rounding, not bf16's.  Same arguments, outputs,
 * split-K slices and diagonal rule as dsvgd_phi_mm; Yx = dsvgd_ysplit(Y)
 * (rows >= roundup(n, 128)).  Requires roundup(n,128) * ldy * 6 < 2^31.
 * sym = 1: D is dsvgd_sqdist_x3's symmetric layout (m == n, row0 == 0,
 * ldy % 256 == 0); a K-step in a column tile J < I is read from the stored
 * tile (J, I), transposed in LDS.  m16 = 1: the v_mfma_f32_16x16x32_bf16
 * form (ldy % 256 == 0), which needs Yx built with swz = 0; m16 = 0 needs
 * swz = 1.
 * dsvgd_ysplit: Yx[kstep][part][column][16] (bf16) from the first `rows`
 * rows of Y (rows a multiple of 16; dsvgd_ysplit_bytes(rows, ldy) bytes,
 * 16-byte aligned); swz = 1: 16-byte halves swapped on columns with bit 3
 * set (the 32x32x16 engines' image), swz = 0: unswizzled (16x16x32). */
int64_t dsvgd_ysplit_bytes(int64_t rows, int64_t ldy);
/* Row image for the split NT engine (Gram, logreg Z): img[kstep][part][row]
 * [16] (bf16) = the three parts of A[row][16 kstep + k] for row < rows_pad,
 * column < kpad (zero outside rows x cols); rows_pad, kpad multiples of 16;
 * dsvgd_rowsplit_bytes(rows_pad, kpad) bytes, 16-byte aligned; swz = 1:
 * 16-byte halves swapped on rows with bit 3 set (32x32x16 engines), swz = 0:
 * unswizzled (16x16x32 engines). */
int64_t dsvgd_rowsplit_bytes(int64_t rows_pad, int64_t kpad);
int dsvgd_rowsplit(const float* A, int64_t lda, int64_t rows, int64_t cols, int64_t rows_pad,
                   int64_t kpad, void* img, int swz, void* stream);
/* gate (nullable): the FmtH2 range-guard word of a dsvgd_h2_scales output
 * over all ldy columns (&scale[2 ldy + 2]): dsvgd_ysplit and dsvgd_phi_mm_x3
 * do nothing while it reads 0 -- the FmtX3 fallback of dsvgd_phi_mm_h2,
 * launched behind it on the same stream, so exactly one of the two writes KY
 * and rowsum without a host round trip (graph-capturable). */
int dsvgd_ysplit(const float* Y, int64_t ldy, int64_t rows, void* Yx, int swz, const float* gate,
                 void* stream);
int dsvgd_phi_mm_x3(const float* D, int64_t ldd, const void* Yx, int64_t ldy, int64_t row0,
                    int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits, float* KY,
                    int64_t ldk, float* rowsum, int sym, int m16, const float* gate, void* stream);

/* ---- FmtH2: the fp16 two-part split engine (the default) ---------------
 * An operand v enters the fp16 MFMA as s v = v0 + v1, v0 = f16(s v),
 * v1 = f16(s v - v0), s a power of two putting the operand's largest
 * magnitude in [2^14, 2^15); the products a0 b0 + a0 b1 + a1 b0 are exact in
 * fp32 and the dropped a1 b1 and split remainder are <= 2^-22 relative, below
 * the fp32 accumulation rounding of any of these GEMMs: fp32-level results
 * from half the MFMAs of the X3 engine (gemm_x3.hpp, h2.hip).  The scale
 * divides out exactly inside each kernel: outputs are unscaled fp32.
 *
 * The window: an entry keeps 22 significant bits only within 2^-16 of the
 * largest magnitude sharing its scale; below it, only 2^-38 of that largest
 * (absolute).  So the NT row images (the Gram's Xc, logreg's W) take one
 * scale per ROW (dsvgd_h2_rowscale / dsvgd_pack_h2's rowscale: no particle
 * sits in another's window), and the NN B operand (phi_mm's [Xc | S], one
 * scale per column) is guarded: dsvgd_h2_scales flags a step whose particles'
 * rows span more than 2^16 in a half of Y, and that step's phi_mm runs on the
 * FmtX3 engine instead (dsvgd_phi_mm_h2 / _x3 `gate`).
 *
 * dsvgd_h2_colscale: per column c of A (rows x cols), scale[c] = s_c and
 * scale[cols + c] = 1 / s_c; scale[2 cols] = t = min s_c over the nonzero
 * finite columns (1 if a column holds an inf / NaN, which then propagate),
 * scale[2 cols + 1] = 1 / t, scale[2 cols + 2] = 0 (no range guard).
 * scale: 2 cols + 3 floats; ws: dsvgd_h2_colscale_workspace_floats(rows,
 * cols) floats.  dsvgd_h2_colscale_guarded (ABI 4; the unfused d > 1024
 * path) also writes the RANGE GUARD of dsvgd_h2_scales for the halves
 * [0, dp) and [dp, cols) (a second pass over A's rows). */
size_t dsvgd_h2_colscale_workspace_floats(int64_t rows, int64_t cols);
int dsvgd_h2_colscale(const float* A, int64_t lda, int64_t rows, int64_t cols, float* ws,
                      float* scale, void* stream);
int dsvgd_h2_colscale_guarded(const float* A, int64_t lda, int64_t rows, int64_t cols, int64_t dp,
                              float* ws, float* scale, void* stream);
/* dsvgd_h2_colscale's output over Y's first cols columns (cols = dp: the X
 * half; cols = ldy: all of Y), bit-identical, from dsvgd_pack_h2's maxima
 * (nb = dsvgd_pack_blocks(rows_pad)); scale[2 cols + 2] = the RANGE GUARD:
 * 1.0 when the X half (or, cols = ldy, the S half) has its largest magnitude
 * more than 2^16 times its smallest nonzero row max, else 0.0. */
int dsvgd_h2_scales(const uint32_t* partial, const uint32_t* gmax, int64_t nb, int64_t ldy,
                    int64_t cols, int64_t dp, float* scale, void* stream);
/* fp16 images (dsvgd_h2_image_bytes(rows, cols) bytes, 16-byte aligned):
 * ysplit: Yh[kstep][part][column][16] of colscale[c] * Y[16 kstep + k][c]
 * (the NN engine's B operand, rows a multiple of 16); rowsplit:
 * img[kstep][part][row][16] of tscale[0] * A[row][16 kstep + k] (the NT
 * engine's operands, zero outside rows x cols).  16-byte halves swapped on
 * columns / rows with bit 3 set (32x32x16 fragment reads). */
int64_t dsvgd_h2_image_bytes(int64_t rows, int64_t cols);
int dsvgd_h2_ysplit(const float* Y, int64_t ldy, int64_t rows, const float* colscale, void* Yh,
                    void* stream);
int dsvgd_h2_rowsplit(const float* A, int64_t lda, int64_t rows, int64_t cols, int64_t rows_pad,
                      int64_t kpad, const float* tscale, void* img, void* stream);
/* the same image with one scale per row: rowscale[i] * A[row i] (rows < rows) */
int dsvgd_h2_rowsplit_rows(const float* A, int64_t lda, int64_t rows, int64_t cols,
                           int64_t rows_pad, int64_t kpad, const float* rowscale, void* img,
                           void* stream);
/* rows [row_begin, row_begin + nrows) of dsvgd_h2_rowsplit_rows's image only
 * (the same arguments; ABI 4: the wide Gauss-Seidel sweep re-splits the rows a
 * block moved). */
int dsvgd_h2_rowsplit_rows_range(const float* A, int64_t lda, int64_t rows, int64_t cols,
                                 int64_t rows_pad, int64_t kpad, const float* rscale, void* img,
                                 int64_t row_begin, int64_t nrows, void* stream);
/* rowscale[i] = the FmtH2 power-of-two scale of row i of A (rows x cols) and
 * rowinv[i] = 1 / rowscale[i] (nullable), for i < rows_pad (1 past rows) */
int dsvgd_h2_rowscale(const float* A, int64_t lda, int64_t rows, int64_t cols, int64_t rows_pad,
                      float* rowscale, float* rowinv, void* stream);
/* dsvgd_h2_rowscale (rowinv required) and dsvgd_h2_rowsplit_rows with those
 * scales in one pass over A: the same bits (round 5; the logreg W image) */
int dsvgd_h2_rowimage(const float* A, int64_t lda, int64_t rows, int64_t cols, int64_t rows_pad,
                      int64_t kpad, float* rowscale, float* rowinv, void* img, void* stream);
/* dsvgd_sqdist_x3 on the FmtH2 engine: Yg = dsvgd_h2_rowsplit_rows(Y, ldy,
 * n_pad, dp, n_pad + 256, dp, rowscale) with the per-row scales of Y's X half
 * (dsvgd_pack_h2's rowscale, or dsvgd_h2_rowscale; >= n_pad floats); same
 * outputs, select modes and layouts. */
int dsvgd_sqdist_h2(const void* Yg, const float* norms, int64_t row0, int64_t m, int64_t n,
                    int64_t d, float* D, int64_t ldd, int select_mode, dsvgd_select_state* st,
                    float* cand, int layout, const float* rowscale, void* stream);
/* ---- the reference's Gauss-Seidel order for 64 < d <= 1024 (ABI 4) -----
 * dsvgd/sampler.py:64-68 / distsampler.py:194-200 move row i with phi_i of the
 * CURRENT particles.  The wide blocked sweep takes B = dsvgd_gsw_block_rows(d, kind)
 * rows at a time: their interactions with every row not moved before them in
 * the block on the f32 engines (dsvgd_sqdist of the centred Y = [X - c | S]
 * rows [r0, r0 + B); dsvgd_gs_mask: D[i][r0 + j] = +inf for j < i, the pairs
 * the walk takes; dsvgd_phi_mm into split-K slices; dsvgd_phi_partial_reduce
 * -> Q = [K Xc | K S], Qr = K 1), then dsvgd_gsw_block_sweep walks the B rows
 * in order in one workgroup: phi_i = (Q_i + s_i + sum_{j<i} k(x_i, x_j')
 * (s_j' + (2/h)(x_i - x_j'))) / n (+ extra), X[i] += step phi_i, the score
 * refreshed (score_kind as dsvgd_gs_block_sweep, or 3: the logistic
 * regression score of logreg_small_kernel on nd data rows xd (ld ldxd, d - 1
 * features) with labels td, times score_scale -- experiments/logreg.py:45-58
 * re-run per pair by distsampler.py:97-99), Y's row and norms[] kept current
 * (centre c = center, the packing centre of Y).  Any d <= 1024 for kind 3. */
int64_t dsvgd_gsw_block_rows(int64_t d, int score_kind);  /* 0 if d > 1024 */
/* The walk's form for score_kind 0 .. 2 (A/B switch, returns the previous
 * setting): 1 (default) = the incremental walk (each moved row's pair terms
 * added to every later row of the block at once, two barriers per row,
 * nothing per row on the path but the row's own phi) for roundup(d, 32) <=
 * 1024 -- 1, 2 or 4 columns per thread up to 256, 512, 1024, blocks of at
 * most 64, 32, 16 rows (B <= 64 / columns per thread), about 132 KB of LDS
 * at every shape; 0 = the four-wave walk (distances and the column loop per
 * row).  Where the incremental walk's LDS cannot be reserved the call runs
 * the four-wave walk (no error). */
int dsvgd_gsw_set_inc(int on);
/* Timing probe of the walk (scripts/walk_probe.py; results are garbage while
 * set): bit 0 skips the next row's operand loads, bit 1 the distances, bit 2
 * the column loop.  Process-wide; returns the previous mask.  0 = normal. */
int dsvgd_gsw_debug(int mask);
int dsvgd_gs_mask(float* D, int64_t ldd, int64_t r0, int64_t B, void* stream);
/* D[i][c0 + j] = +inf for i < B (<= 1024), j < nc (panel layout): the
 * pipelined wide sweep (round 6) leaves the group walking beside a wide pass
 * out of that pass; dsvgd_gsw_group_corr adds its rows at their moved
 * positions afterwards. */
int dsvgd_gs_mask_cols(float* D, int64_t ldd, int64_t B, int64_t c0, int64_t nc, void* stream);
/* Test hook: one wave holds `stream` for ns nanoseconds (the pipelined
 * sweep's forced-overlap test). */
int dsvgd_debug_spin(int64_t ns, void* stream);
/* The grouped wide sweep (round 5): one wide pass for a group of blocks
 * (dsvgd_gs_mask over the whole group, B <= 1024), then after each block's
 * walk the group's later rows [r0, r0 + nr) gain that block's moved rows
 * [p0, p0 + pB): Q += k_ij (x_j' - c | s_j'), Qr += k_ij by explicit
 * differences, j in order (Q, Qr: the later rows' first entries).  pB <= 128
 * (round 6: a whole 128-row group in one launch, the pipelined sweep's
 * correction for the group walked beside its pass). */
int dsvgd_gsw_group_corr(const float* X, int64_t ldx, const float* S, int64_t lds,
                         const float* center, int64_t n, int64_t d, int64_t r0, int64_t nr,
                         int64_t p0, int64_t pB, const dsvgd_select_state* st, float* Q,
                         int64_t ldq, float* Qr, void* stream);
int dsvgd_gsw_block_sweep(float* X, int64_t ldx, float* S, int64_t lds, float* Y, int64_t ldy,
                          float* norms, const float* center, int64_t n, int64_t d, int64_t r0,
                          int64_t B, const dsvgd_select_state* st, float step, const float* Q,
                          int64_t ldq, const float* Qr, const float* extra, int64_t lde,
                          float* phi_out, int64_t ldphi, int score_kind, const float* mu,
                          const float* lam, float score_scale, const float* xd, int64_t ldxd,
                          const float* td, int64_t nd, void* stream);

/* ---- the pair-split layout of a DistSampler rank (ABI 4) ---
 * With the scores identical on every rank (all_scores, or replicated data),
 * the S ranks split the symmetric n x n matrix by BLOCK PAIRS: rank r
 * computes its diagonal square, the forward blocks (r, r+1) .. (r, r+S/2-1)
 * (mod S) and half of the antipodal pair {(r, r+S/2), (r+S/2, r)}; for each
 * block (r, c) it holds it sends the owner of c the partial K(r,c)^T Y_r
 * (dsvgd_phi_h2_transposed), and sums the partials it receives into its own
 * phi (dsvgd_phi_finish_parts).  Replaces the interaction loop of
 * dsvgd/distsampler.py:84-101 over the all-gathered particles (:152-170).
 *
 * dsvgd_sqdist_h2_parts: dsvgd_sqdist_h2 over a list of parts of the owned
 * row block [row0, row0 + m) (host array).  kind 0: a rectangle (rows
 * [row_off, +rows) of the block x global columns [col0, +cols)) whose
 * entries count twice in the median select when weight2 (the rank holds the
 * pair for both owners); kind 1: the block's diagonal square (row_off = 0,
 * rows = cols = m, col0 = row0; upper tiles + mirror stores); kind 2: a
 * rectangle computed only while *gate != 0 (the FmtH2 range guard: the
 * fallback phi_mm reads the whole row block), without select accounting.
 * select_mode 0 or 2 (bracket); dp % 256 == 0; row0, m multiples of 256;
 * col0, cols multiples of 256, row_off, rows of 128. */
typedef struct dsvgd_gram_part {
  int64_t row_off, rows, col0, cols;
  int32_t kind, weight2;
} dsvgd_gram_part;
int dsvgd_sqdist_h2_parts(const void* Yg, const float* norms, int64_t row0, int64_t m, int64_t n,
                          int64_t d, float* D, int64_t ldd, int select_mode,
                          dsvgd_select_state* st, float* cand, const dsvgd_gram_part* parts,
                          int nparts, const float* gate, const float* rowscale, void* stream);
/* dsvgd_radix_hist with a tile weight map instead of the symmetric rule:
 * the panel of D tile (I, J) (128 x 128, panel layout, m_pad x n_pad) counts
 * wmap[I * (n_pad / 128) + J] times (0: not an entry of this rank's share). */
int dsvgd_radix_hist_wmap(const float* D, int64_t m_pad, int64_t n_pad, const float* cand,
                          int pass, dsvgd_select_state* st, const uint8_t* wmap, void* stream);
/* phi_mm (FmtH2) of rows [row0, row0 + m) of the interacting set (D: their
 * panel rows) over a CYCLIC window of columns [col0, col0 + wlen) mod
 * n_pad, into `splits` split-K slices (KY + z m ldk, rowsum + z
 * roundup(m,128)); the diagonal j == row0 + i skipped as in dsvgd_phi_mm
 * wherever the window holds it, before or after the wrap (a row left of col0
 * meets its own column in the wrapped part).  col0, wlen multiples of 16.
 * gate / gate_on as dsvgd_phi_mm_h2 (run iff (*gate != 0) == gate_on). */
int dsvgd_phi_h2_window(const float* D, int64_t ldd, const void* Yh, int64_t ldy, int64_t row0,
                        int64_t m, int64_t n, int64_t col0, int64_t wlen,
                        const dsvgd_select_state* st, int64_t splits, float* KY, int64_t ldk,
                        float* rowsum, const float* colinv, const float* gate, int gate_on,
                        void* stream);
/* The transposed partial of a rectangle of D: D points at the rectangle's
 * first row (a 128-row panel row; its rows are interacting-set rows yrow0 ..
 * yrow0 + krows - 1), its columns [col0, col0 + mo) (col0 a multiple of
 * 128).  P_z[i][:] = sum_{j in slice z} exp(-D[j][col0 + i]/h) Y[yrow0 + j][:]
 * and rs_z[i] the same sum of the weights, for i < mo (KY layout: P + z mo
 * ldp, rs + z roundup(mo,128)).  krows a multiple of 16.  No diagonal rule:
 * a rectangle that holds entries j == col0 + i - yrow0 of D's diagonal sums
 * their k_ii like any other weight (the layout's rectangles are off-diagonal
 * blocks).  The same holds for the two batched forms below. */
int dsvgd_phi_h2_transposed(const float* D, int64_t ldd, const void* Yh, int64_t ldy,
                            int64_t yrow0, int64_t krows, int64_t col0, int64_t mo, int64_t n,
                            const dsvgd_select_state* st, int64_t splits, float* P, int64_t ldp,
                            float* rs, const float* colinv, const float* gate, int gate_on,
                            void* stream);
/* dsvgd_phi_h2_transposed for `count` whole m x m blocks of the owned rows'
 * D in one launch, no split-K: block q (< count) is D's column block (first +
 * q) mod nblocks (the forward blocks of a rank), its partial [m x ldp | m row
 * sums] written at P + q pstride. */
int dsvgd_phi_h2_transposed_blocks(const float* D, int64_t ldd, const void* Yh, int64_t ldy,
                                   int64_t yrow0, int64_t m, int64_t first, int64_t nblocks,
                                   int64_t count, int64_t n, const dsvgd_select_state* st,
                                   float* P, int64_t ldp, int64_t pstride, const float* colinv,
                                   const float* gate, int gate_on, void* stream);
/* dsvgd_phi_h2_transposed_blocks with each block's K range (its m rows of D)
 * split into zsplit slices (m a multiple of 16 zsplit), so that count x
 * m/128 x zsplit workgroups fill the CUs: slice z of block q written at
 * P + (z count + q) pstride (dsvgd_phi_partial_reduce_blocks sums them). */
int dsvgd_phi_h2_transposed_blocks_split(const float* D, int64_t ldd, const void* Yh, int64_t ldy,
                                         int64_t yrow0, int64_t m, int64_t first, int64_t nblocks,
                                         int64_t count, int64_t zsplit, int64_t n,
                                         const dsvgd_select_state* st, float* P, int64_t ldp,
                                         int64_t pstride, const float* colinv, const float* gate,
                                         int gate_on, void* stream);
/* For q < count: out + q ostride = sum over z < zsplit of the [rows x ldp |
 * row sums] partial at P + (z count + q) pstride (row sums at + rows ldp in,
 * + rows ldo out) -- the split forward blocks' messages.  The order of
 * dsvgd_phi_partial_reduce. */
int dsvgd_phi_partial_reduce_blocks(const float* P, int64_t ldp, int64_t pstride, int64_t zsplit,
                                    int64_t count, int64_t rows, int64_t cols, float* out,
                                    int64_t ldo, int64_t ostride, void* stream);
/* out[i][c] = sum_z P[z][i][c] (c < cols) and out_rs[i] = sum_z rs[z][i] (the
 * P / rs layout of dsvgd_phi_h2_transposed), in a fixed order: with G = the
 * slice count rounded up to a power of two, at most 16, group g < G sums the
 * slices g, g + G, g + 2 G, ... in that order from zero, and the G group sums
 * are then added in g order -- slice order up to 16 slices, interleaved
 * groups beyond. */
int dsvgd_phi_partial_reduce(const float* P, int64_t ldp, const float* rs, int64_t splits,
                             int64_t rows, int64_t cols, float* out, int64_t ldo, float* out_rs,
                             void* stream);
/* dsvgd_phi_finish over the own split-K slices plus `nparts` partials, each
 * adding ky[z][i - row_off][:] and rs[z][i - row_off] (z < splits) to rows
 * row_off <= i < row_off + rows, summed in list order after the own slices.
 * gate (nullable): while *gate != 0 the parts are skipped and the own slices
 * are `splits_fb` (the range guard's whole-row-block fallback). */
typedef struct dsvgd_phi_part {
  const float* ky;
  const float* rs;
  int64_t ldk, row_off, rows, splits;
} dsvgd_phi_part;
int dsvgd_phi_finish_parts(const float* KY, int64_t ldk, const float* rowsum, int64_t splits,
                           const float* Y, int64_t ldy, int64_t row0, int64_t m, int64_t d,
                           int64_t dp, const dsvgd_select_state* st, float inv_n, float step,
                           const float* extra, int64_t lde, float* phi, int64_t ldphi, float* X,
                           int64_t ldx, const dsvgd_phi_part* parts, int nparts,
                           const float* gate, int64_t splits_fb, void* stream);

/* dsvgd_phi_mm_x3 on the FmtH2 engine: Yh = dsvgd_h2_ysplit(Y, ldy, n_pad,
 * scale) and colinv = &scale[ldy] of a dsvgd_h2_colscale over all ldy
 * columns of Y; same outputs (unscaled), split-K slices, diagonal rule and
 * symmetric layout (sym needs ldy % 256 == 0).  Requires n_pad * ldy * 4 <
 * 2^31.  gate (nullable, &scale[2 ldy + 2]): does nothing while it reads
 * nonzero (the range guard hands the step to dsvgd_phi_mm_x3, or to
 * dsvgd_phi_mm_gated where no FmtX3 image fits). */
int dsvgd_phi_mm_h2(const float* D, int64_t ldd, const void* Yh, int64_t ldy, int64_t row0,
                    int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits, float* KY,
                    int64_t ldk, float* rowsum, int sym, const float* colinv, const float* gate,
                    void* stream);

/* phi[i] = inv_n * (s_i + KS[i] + (2/h) (rowsum[i] xc[i] - KXc[i])) with the
 * split-K partials summed in slice order (s_i: the self term k_ii s_i), plus
 * extra[i] if extra != NULL (the h * W2-gradient row of dsvgd_w2_grad:
 * delta = phi_hat + h W, dsvgd/distsampler.py:194-198), and, if X != NULL,
 * X[i] += step * phi[i] (the update of dsvgd/sampler.py:68 /
 * dsvgd/distsampler.py:200, Jacobi order).  phi and extra may be NULL. */
int dsvgd_phi_finish(const float* KY, int64_t ldk, const float* rowsum, int64_t splits,
                     const float* Y, int64_t ldy, int64_t row0, int64_t m, int64_t d, int64_t dp,
                     const dsvgd_select_state* st, float inv_n, float step, const float* extra,
                     int64_t lde, float* phi, int64_t ldphi, float* X, int64_t ldx,
                     void* stream);
/* Process-wide A/B switch (default 1): dsvgd_phi_finish takes four columns
 * per thread (16-byte accesses) when d, dp and every leading dimension are
 * multiples of 4 and every base is 16-byte aligned; 0 keeps one element per
 * thread.  Same bits.  Returns the previous setting. */
int dsvgd_phi_set_finish_vec(int on);

/* ---- phi_mm in the ONE-OPERAND form ---------------------------------------
 * K S - (2/h) K Xc = K W with W = S - (2/h) Xc, so
 *   phi_i = inv_n (s_i + (K W)_i + (2/h) r_i xc_i)
 * needs one dp-wide product instead of K [Xc | S] (2 dp wide): half the
 * MFMAs, half the B image and half the split-K partials, for the same staging
 * of K.  The form is a property of the caller (an engine picks it once); the
 * two-operand entry points above are unchanged.  Requires the fused scales
 * (dsvgd_pack_h2's maxima, ldy <= dsvgd_pack_max_ldy()) and dp % 256 == 0.
 *
 * dsvgd_h2_wscales (after the bandwidth is in `st`; t = 2 st->inv_h): the
 * power-of-two column scales of W in dsvgd_h2_colscale's layout over dp
 * columns (wscale: 2 dp + 3 floats), from the bound b_c = max|S_c| + t
 * max|Xc_c| (s_c b_c in [2^14, 2^15); at most one bit of the 22 lost), and
 * the RANGE GUARD wscale[2 dp + 2], at least as conservative as
 * dsvgd_h2_scales over all of Y: 1.0 when that guard fires (a half of Y
 * spans more than 2^16 between its largest magnitude and its smallest
 * nonzero row max), or when max(gS, t gX) > 2^16 min(rS, t rX) (g: a half's
 * largest magnitude, r: its smallest nonzero row max), else 0.0.
 * dsvgd_h2_wsplit: Wh[kstep][part][column][16] (dsvgd_h2_image_bytes(rows,
 * dp) bytes) of wscale[c] * fmaf(-t, Y[r][c], Y[r][dp + c]) -- dsvgd_h2_ysplit's
 * image over dp columns; Y's zero padding gives zero rows >= n, columns >= d.
 * dsvgd_phi_mm_h2w: dsvgd_phi_mm_h2's arguments with the W image, ldw = dp
 * (a multiple of 256) and colinv = &wscale[dp]; partials KW[splits][m][ldk]
 * (ldk >= dp) and the row sums as dsvgd_phi_mm_h2; the full layout with any
 * row block, or sym = 1 (m == n, row0 == 0) in one launch.  gate =
 * &wscale[2 dp + 2]: does nothing while it reads nonzero -- the caller runs
 * the two-operand FmtX3 fallback (dsvgd_ysplit + dsvgd_phi_mm_x3, or
 * dsvgd_phi_mm_gated) behind it on the same word.
 * dsvgd_phi_splits_w: the slice count (every fp32 chain within 16384
 * columns, at least two rounds of blocks per CU; m = n = 65536, dp = 256: 4).
 * dsvgd_phi_finish_w: dsvgd_phi_finish for this form.  *guard == 0: sums the
 * `splits` slices of KW (row stride ldk) and forms the phi above; nonzero:
 * dsvgd_phi_finish's formula, in its order, on the `splits_fb` two-operand
 * slices the fallback left in KY (row stride ldky >= 2 dp).  KW and KY may be
 * one buffer.  extra, phi, X as dsvgd_phi_finish. */
int dsvgd_h2_wscales(const uint32_t* partial, const uint32_t* gmax, int64_t nb, int64_t ldy,
                     int64_t dp, const dsvgd_select_state* st, float* wscale, void* stream);
int dsvgd_h2_wsplit(const float* Y, int64_t ldy, int64_t rows, int64_t dp,
                    const dsvgd_select_state* st, const float* wscale, void* Wh, void* stream);
int64_t dsvgd_phi_splits_w(int64_t m, int64_t n, int64_t dp);
int dsvgd_phi_mm_h2w(const float* D, int64_t ldd, const void* Wh, int64_t ldw, int64_t row0,
                     int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits, float* KW,
                     int64_t ldk, float* rowsum, int sym, const float* colinv, const float* gate,
                     void* stream);
int dsvgd_phi_finish_w(const float* KW, int64_t ldk, const float* rowsum, int64_t splits,
                       const float* KY, int64_t ldky, int64_t splits_fb, const float* Y,
                       int64_t ldy, int64_t row0, int64_t m, int64_t d, int64_t dp,
                       const dsvgd_select_state* st, const float* guard, float inv_n, float step,
                       const float* extra, int64_t lde, float* phi, int64_t ldphi, float* X,
                       int64_t ldx, void* stream);

/* d <= 64 (used for d <= 2): phi (and the optional X update) straight from the pairwise form
 * phi_i = inv_n sum_j k_ij (s_j + (2/h)(x_i - x_j)) on the VALU -- the
 * reference's own per-pair expression (dsvgd/sampler.py:38-40), which avoids
 * the r x - K X cancellation of the GEMM form at small d.  Replaces
 * dsvgd_phi_mm + dsvgd_phi_finish for small d (extra as in dsvgd_phi_finish).
 * partial (nullable, partial_floats long): scratch for split-J partial sums
 * (up to partial_floats / (m d) slices, summed in order by a second kernel),
 * which keeps the chip busy when m is small. */
int dsvgd_phi_direct(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t row0,
                     int64_t m, int64_t n, int64_t d, const dsvgd_select_state* st, float inv_n,
                     float step, const float* extra, int64_t lde, float* phi, int64_t ldphi,
                     float* X, int64_t ldx, float* partial, int64_t partial_floats,
                     void* stream);

/* Gauss-Seidel single-row update (reference order): for particle i, phi_i
 * from exact differences against the CURRENT X (rows < i already moved),
 * X[i] += step * phi_i.  Reproduces dsvgd/sampler.py:64-68 and
 * dsvgd/distsampler.py:194-200 one row at a time.  n_int interacting rows
 * start at X (row i is X + i*ldx).  extra (nullable, d floats) is added to
 * phi_i before the step (the row's h * W2 gradient, distsampler.py:196-198). */
int dsvgd_phi_row(float* X, int64_t ldx, const float* S, int64_t lds, int64_t n_int, int64_t d,
                  int64_t i, const dsvgd_select_state* st, float step, const float* extra,
                  float* phi_out, void* stream);
/* The same row update with the j range split over `blocks` workgroups (two
 * launches; partial: blocks x d floats of scratch), for large n_int.
 * dsvgd_phi_row_blocks(n, d) = the split to use (1: call dsvgd_phi_row). */
int64_t dsvgd_phi_row_blocks(int64_t n, int64_t d);
int dsvgd_phi_row_split(float* X, int64_t ldx, const float* S, int64_t lds, int64_t n, int64_t d,
                        int64_t i, const dsvgd_select_state* st, float step, const float* extra,
                        float* phi_out, float* partial, int64_t blocks, void* stream);

/* Blocked Gauss-Seidel sweep (the same reference order, d <= 64): rows
 * [r0, r0 + B), B <= dsvgd_gs_block_rows() = 64, of the interacting set X
 * (n x d).  gs_block_part: Q[i][c] = the raw sum over every j outside
 * [r0, r0 + i) of k(x_i, x_j) (s_j + (2/h)(x_i - x_j)) as the block starts,
 * computed as nsplit = dsvgd_gs_splits(n) j slices (partial: nsplit x B x d
 * floats of scratch) and summed in slice order (into partial[0 .. B d) when
 * B d nsplit > 16384, else by the sweep);
 * gs_block_sweep then walks the block in order in one wave: phi_i = (Q_i +
 * the terms of the block rows already moved, at their new positions) / n
 * [+ extra row i], X[r0+i] += step phi_i, and the moved particle's score
 * refreshed in S (score_kind 1: scale * (-lam (x - mu)), 2: the
 * experiments/gmm.py mixture per coordinate; 0: S left as is -- exchanged
 * scores are frozen for the step, distsampler.py:194-200).  Two or three launches
 * per 64 rows instead of two per row (dsvgd_phi_row_split).  nsplit, B, d of
 * the sweep: those of the gs_block_part call. */
int64_t dsvgd_gs_block_rows(void);
int64_t dsvgd_gs_splits(int64_t n);
int dsvgd_gs_block_part(const float* X, int64_t ldx, const float* S, int64_t lds, int64_t n,
                        int64_t d, int64_t r0, int64_t B, const dsvgd_select_state* st,
                        float* partial, int64_t nsplit, void* stream);
int dsvgd_gs_block_sweep(float* X, int64_t ldx, float* S, int64_t lds, int64_t n, int64_t d,
                         int64_t r0, int64_t B, const dsvgd_select_state* st, float step,
                         const float* partial, int64_t nsplit, const float* extra, int64_t lde,
                         float* phi_out, int64_t ldphi, int score_kind, const float* mu,
                         const float* lam, float score_scale, void* stream);

/* ---- W2 / JKO term (dsvgd/distsampler.py:103-129, used at :190-198) ---- */
/* The reference LP  min <P,C>, P >= 0, row sums 1/m, column sums 1/n  over
 * C_ij = ||x_i - y_j||^2 (x: m owned particles, y: n previous particles) has
 * an integral optimum when n = R m: an assignment of n slots (slot s belongs
 * to row s / R) to the n columns, each of mass 1/n.
 *
 * C[i][j] (m x n, ldc >= n) from explicit fp32 differences
 * (distsampler.py:107-114). */
int dsvgd_w2_cost(const float* X, int64_t ldx, int64_t m, const float* Y, int64_t ldy, int64_t n,
                  int64_t d, float* C, int64_t ldc, void* stream);
/* The same C on the FmtH2 split-role Gram (ABI 4, round 6): C_ij = |x_i -
 * c|^2 + |y_j - c|^2 - 2 (x_i - c).(y_j - c) (c: Y's robust centre,
 * dsvgd_colcenter) on the fp16 MFMAs, fp32-accurate per the FmtH2 bound
 * (|error| ~ 2^-21 (|x_i - c|^2 + |y_j - c|^2)), and every entry below
 * tau (|x_i - c|^2 + |y_j - c|^2) -- where that form cancels, e.g. a particle
 * and its own previous position -- recomputed from explicit fp32
 * differences in dsvgd_w2_cost's order (the same bits).  C needs
 * roundup(m, 128) rows and ldc >= roundup(n, 256) (16-byte aligned rows;
 * the padding is written); ws: dsvgd_w2_cost_h2_workspace_bytes, 256-byte
 * aligned.  d <= 1024.  cstat (NULL, or 2 device words): the largest entry
 * of C (float bits) and a non-finite flag, taken while C is written --
 * dsvgd_w2_assign_stat then skips its pass over C for them. */
/* A/B switch of dsvgd_w2_cost_h2's C stores (returns the previous): 1
 * (default) non-temporal, 0 the default cache policy. */
int dsvgd_w2_set_cost_nt(int on);

/* Process-wide A/B switch (default 1): dsvgd_w2_cost_h2 writes C in whole
 * 128-byte row lines (two slices' values traded between lane pairs); 0 writes
 * each slice's half lines as it goes.  Same C bits.  Returns the previous
 * setting. */
int dsvgd_w2_set_cost_lines(int on);
size_t dsvgd_w2_cost_h2_workspace_bytes(int64_t m, int64_t n, int64_t d);
int dsvgd_w2_cost_h2(const float* X, int64_t ldx, int64_t m, const float* Y, int64_t ldy,
                     int64_t n, int64_t d, float* C, int64_t ldc, void* ws, float tau,
                     uint32_t* cstat, void* stream);
/* Device workspace of dsvgd_w2_assign (32 n + 256 bytes). */
size_t dsvgd_w2_workspace_bytes(int64_t m, int64_t n);
/* assign[s] = column of slot s in an optimal plan (replaces scipy linprog,
 * distsampler.py:115-126): epsilon-scaling auction on the GPU, final
 * eps = max C * 2^-24 / n (within one fp32 ulp of max C of the optimum).
 * BLOCKS the calling thread (polls the device between batches of rounds);
 * fails with -3 after max_rounds.  rounds_out (host, nullable) gets the
 * number of bidding rounds.  warm_phases > 0: keep the prices left in `ws`
 * by the previous call on a nearby problem (SVGD's next step) and start
 * warm_phases epsilon phases above the final eps; 0: cold start. */
int dsvgd_w2_assign(const float* C, int64_t ldc, int64_t m, int64_t n, void* ws,
                    int64_t max_rounds, int warm_phases, int32_t* assign, int64_t* rounds_out,
                    void* stream);
/* dsvgd_w2_assign warm-started from the previous call on this workspace
 * (its prices) and that call's plan prev_assign (n slots): the first epsilon
 * is the previous plan's complementary-slackness violation under the new
 * costs / 64 (so a small SVGD step starts near eps_final, a large one high),
 * then the usual phases down to eps_final -- same optimality guarantee. */
int dsvgd_w2_assign_warm(const float* C, int64_t ldc, int64_t m, int64_t n, void* ws,
                         int64_t max_rounds, const int32_t* prev_assign, int32_t* assign,
                         int64_t* rounds_out, void* stream);
/* dsvgd_w2_assign (prev_assign NULL, warm_phases as there) or
 * dsvgd_w2_assign_warm (prev_assign set) with C's largest entry and
 * finiteness taken from cstat (dsvgd_w2_cost_h2's) instead of a pass over C
 * (round 6).  The same plan. */
int dsvgd_w2_assign_stat(const float* C, int64_t ldc, int64_t m, int64_t n, void* ws,
                         int64_t max_rounds, int warm_phases, const int32_t* prev_assign,
                         int32_t* assign, int64_t* rounds_out, const uint32_t* cstat,
                         void* stream);
/* Process-wide switch of the auction's phase keep (default 0): a new
 * epsilon phase, and dsvgd_w2_assign_warm's first phase with the previous
 * plan, keep every slot whose column still meets epsilon-complementary
 * slackness; 0 re-assigns every slot each phase.  Same optimality guarantee
 * either way.  Returns the previous setting. */
int dsvgd_w2_set_keep(int keep);
/* Process-wide epsilon divisor between the auction's phases (default 8;
 * accepted in [2, 1024], otherwise ignored).  Returns the previous value. */
double dsvgd_w2_set_theta(double theta);
/* The last dsvgd_w2_assign's phase tails on this host thread: out[0] bids,
 * out[1] full row scans among them, out[2..4] microseconds spent in the
 * cached bids, the scans (with their cache refill) and the resolves, out[5]
 * tails whose scan helpers did not answer in time (the solve then finishes
 * on the bid rounds, same plan) -- as of the last control readback.
 * Returns 6 (the length of out). */
int64_t dsvgd_w2_tail_stats(int64_t* out);
/* Process-wide test switch (default 0): the phase tail's scan helpers exit
 * at once, so every tail stalls and hands its phase back to the bid rounds.
 * Returns the previous setting. */
int dsvgd_w2_set_tail_debug(int nohelp);

/* Process-wide switch (default 1): an R = 1 warm start (prev_assign given,
 * keep off) takes the violation and its first round's row scans (best value,
 * its column, second value) in one pass over C, and the first round bids from
 * them; 0 runs the violation pass and a full-scan bid round (same bids, same
 * plan; A/B).  Returns the previous setting. */
int dsvgd_w2_set_fuse_first(int on);
/* Progress of this host thread's last dsvgd_w2_assign: out[3k..3k+2] =
 * (rounds, epsilon phase, unassigned slots) at the k-th control readback
 * (every 16 rounds); copies min(count, cap) triples, returns count. */
int64_t dsvgd_w2_trace(int64_t* out, int64_t cap);
/* G[i] = h * sum_j P_ij (x_i - y_j) = h/n * sum_{slots s of i} (x_i - y_assign[s])
 * (distsampler.py:128 scaled by the JKO step h of :198); pass G as `extra`
 * to dsvgd_phi_finish / dsvgd_phi_direct / dsvgd_phi_row. */
int dsvgd_w2_grad(const float* X, int64_t ldx, int64_t m, const float* Y, int64_t ldy, int64_t n,
                  int64_t d, const int32_t* assign, float h, float* G, int64_t ldg, void* stream);

/* ---- target scores grad log p (replace the autograd _dlogp calls) ------ */
/* S = scale * (-lam * (X - mu))      (synthetic Gaussian target)            */
int dsvgd_score_gaussian(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                         const float* lam, float scale, float* S, int64_t lds, void* stream);
/* S = scale * d/dx log(1/3 N(x;-2,1) + 1/3 N(x;2,1)), elementwise
 * (experiments/gmm.py:16-21) */
int dsvgd_score_gmm(const float* X, int64_t ldx, int64_t n, int64_t d, float scale, float* S,
                    int64_t lds, void* stream);
/* Bayesian logistic regression (experiments/logreg.py:45-58), x = [log a, w]:
 *   s_0 = scale*(-a + p/2 - a/2 |w|^2),  s_w = scale*(-a w + Xd^T (t * sigma(-t * Xd w)))
 * as two MFMA GEMMs (Z = W Xd^T with the sigmoid epilogue, G Xd); for
 * n <= 32 particles and N <= 8192 rows (the Gauss-Seidel order's
 * one-particle refresh) a single one-block-per-particle launch instead.
 * Xd: N x p data rows (ldxd), t: N labels (+-1).  Workspace:
 * dsvgd_logreg_workspace_bytes(n, N, p) (unused on the small path). */
/* The FmtH2 logistic-regression score as one fused kernel (1, default: Z,
 * sigma and G . Xd with G kept in registers; 224 < p <= 256 weights, the
 * bench's p = 255) or the two-GEMM path (0).  A/B switch; returns the previous
 * setting.  The prepared workspace holds both paths' data images. */
int dsvgd_logreg_set_fused(int on);
size_t dsvgd_logreg_workspace_bytes(int64_t n, int64_t N, int64_t p);
/* 1 where n particles, N data rows and p = d - 1 weights take the
 * one-block-per-particle path, n <= 32 and (p <= 32 or N <= 8192): no
 * workspace is read there, and dsvgd_logreg_prepare / _prepared / _prior
 * refuse the shape.  0 otherwise.  Host only (no device call). */
int dsvgd_logreg_small(int64_t n, int64_t N, int64_t p);
int dsvgd_score_logreg(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                       int64_t ldxd, const float* t, int64_t N, float scale, float* S, int64_t lds,
                       void* workspace, void* stream);
/* the same on a chosen GEMM engine: 0 = FmtH2 (what dsvgd_score_logreg
 * runs), 1 = FmtX3, 2 = the exact f32 MFMA engines (precision reference) */
int dsvgd_score_logreg_engine(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                              int64_t ldxd, const float* t, int64_t N, float scale, float* S,
                              int64_t lds, void* workspace, int engine, void* stream);
/* ... as two calls, for a data set scored at many particle sets (every SVGD
 * step): logreg_prepare writes the data-only part of the workspace (padded
 * Xd and t, Xd's FmtH2 scales and split images) once; score_logreg_prepared
 * then reads it every step (same n, N, d, engine and workspace).  Not for
 * the n <= 32 one-block path (EINVAL there: use dsvgd_score_logreg_engine). */
int dsvgd_logreg_prepare(const float* Xd, int64_t ldxd, const float* t, int64_t N, int64_t n,
                         int64_t d, void* workspace, int engine, void* stream);
int dsvgd_score_logreg_prepared(const float* X, int64_t ldx, int64_t n, int64_t d, int64_t N,
                                float scale, float* S, int64_t lds, void* workspace, int engine,
                                void* stream);

/* dsvgd_score_logreg_prepared with the prior weighted by prior_weight:
 * S = scale * (sum over the data - prior_weight * grad of the prior terms).
 * DistSampler's gathered-data all_scores mode scores its own particles over
 * every rank's data with prior_weight = S, which is what the reference's
 * all-reduce of S per-rank logp gradients sums to (distsampler.py:160-170:
 * each rank's logp carries the prior once).  prior_weight = 1 gives exactly
 * dsvgd_score_logreg_prepared's bits.  Replaces: the same call sites. */
int dsvgd_score_logreg_prior(const float* X, int64_t ldx, int64_t n, int64_t d, int64_t N,
                             float scale, float prior_weight, float* S, int64_t lds,
                             void* workspace, int engine, void* stream);

/* The minibatch estimate of the logistic-regression score: the likelihood
 * over the cyclic window of B data rows that starts at row c = *cursor, rows
 * (c + q) mod N for q < B, its terms weighted N / B, and the prior terms once;
 * scale applies to the sum:
 *   s_w = scale*((N/B) sum_q t_q sigma(-t_q xd_q.w) xd_q - a w),
 *   s_0 = scale*(-a + p/2 - a/2 |w|^2)            (dsvgd_score_logreg's)
 * cursor: one int64 in device memory, read by every workgroup (any value:
 * taken mod N), so that a captured iteration replays with a moving window --
 * the window rule of dsvgd_score_bnn_window; dsvgd_window_advance moves it.
 * The arguments of dsvgd_score_logreg_engine, then the cursor and B.  The
 * window's rows are read where they lie on every call (no prepared image):
 * exact fp32 on v_mfma_f32_32x32x2_f32, a workgroup per 128 particles, the
 * window through LDS in chunks of 32 rows, G in registers; p > 256 splits the
 * columns over workgroups; n <= 16 (the sequential order's one-particle
 * refresh) takes a workgroup per particle on the VALU.  Every sum in a fixed
 * order, no atomics: the same bits on every call.  `engine` is checked (0-2)
 * and otherwise unused -- every engine's window score is this fp32 kernel --
 * and `workspace` is not read (may be NULL):
 * dsvgd_logreg_window_workspace_bytes is 0 and exists for callers that size
 * every score workspace through a query.  Only enqueues work.  Any n >= 1,
 * 1 <= p = d - 1 <= 1023, 1 <= B <= N; ldx, lds >= d, ldxd >= p; S's pad
 * columns are left alone.  Replaces: the reference has no minibatch logp;
 * its users subsample inside a Python logp differentiated by autograd
 * (dsvgd/sampler.py:28-33 _dlogp; notes.md:10-34). */
size_t dsvgd_logreg_window_workspace_bytes(int64_t n, int64_t B, int64_t p);
int dsvgd_score_logreg_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                              int64_t ldxd, const float* t, int64_t N, float scale, float* S,
                              int64_t lds, void* workspace, int engine, const int64_t* cursor,
                              int64_t B, void* stream);

/* Posterior-predictive probability of the logistic-regression test set:
 * prob[q] = (1/n) sum_j sigma(xt_q . w_j), w_j = X[j][1:d] (no bias; alpha
 * unused) -- the ensemble mean of experiments/logreg_plots.py:42-50
 * (`_test_acc`), which the caller thresholds (prob > 0.5 vs t > 0) for the
 * test accuracy.  fp32 (the reference evaluates it in fp64 with numpy).
 * Xt: Nt x (d-1) row-major; workspace of
 * dsvgd_logreg_predict_workspace_bytes(n, Nt, d-1) bytes, 256-B aligned. */
size_t dsvgd_logreg_predict_workspace_bytes(int64_t n, int64_t Nt, int64_t p);
int dsvgd_logreg_predict(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xt,
                         int64_t ldxt, int64_t Nt, float* prob, void* workspace, void* stream);

/* Bayesian neural-network regression (Liu & Wang 2016: one hidden ReLU layer
 * of H units, Gamma(a0, b0) hyper-priors on the noise precision g and the
 * weight precision l, both carried as logs with the log-Jacobian):
 *   x = [vec(W1) (p x H row-major) | b1 (H) | w2 (H) | b2 | log g | log l],
 *   d = H (p + 2) + 3,  f(z) = w2 . relu(W1^T z + b1) + b2,  r_q = y_q - f(z_q),
 *   log p = N/2 log g - g/2 sum_q r_q^2 + (d-2)/2 log l - l/2 |x[:d-2]|^2
 *           + a0 log g - b0 g + a0 log l - b0 l.
 * S = scale * grad log p (the whole gradient, prior included; relu'(0) = 0)
 * for n particles over N data rows Z (N x p, ldz) with targets y, in exact
 * fp32 FMAs on the VALU: one workgroup per particle, the data in chunks of
 * 256 rows, every sum in a fixed order (the same bits on every call, and a
 * particle's score does not depend on n).  1 <= p, H <= 64; any n, N >= 1.
 * No workspace.  Absent in the reference: replaces a user logp of this model
 * differentiated by autograd (dsvgd/sampler.py:28-33 _dlogp). */
int dsvgd_score_bnn(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Z, int64_t ldz,
                    const float* y, int64_t N, int64_t p, int64_t H, float a0, float b0,
                    float scale, float* S, int64_t lds, void* stream);
/* The minibatch estimate of the same score (Liu & Wang's): the likelihood
 * over the cyclic window of B rows that starts at row c = *cursor, rows
 * (c + q) mod N for q < B, its terms weighted N / B -- the N/2 of the log g
 * entry included, which becomes (N/B) B/2 -- and the prior terms once; scale
 * applies to the sum.  cursor: one int64 in device memory, read by every
 * workgroup (any value: taken mod N), so that a captured iteration replays
 * with a moving window.  1 <= B <= N.  The same kernel as dsvgd_score_bnn
 * with a row origin, a row count and a likelihood weight; dsvgd_score_bnn
 * keeps its own instantiation and its bits. */
int dsvgd_score_bnn_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Z,
                           int64_t ldz, const float* y, int64_t N, int64_t p, int64_t H, float a0,
                           float b0, float scale, const int64_t* cursor, int64_t B, float* S,
                           int64_t lds, void* stream);
/* *cursor <- (*cursor + B) mod N on the device (one thread, ordinary loads
 * and stores), stream-ordered like every other entry point. */
int dsvgd_window_advance(int64_t* cursor, int64_t B, int64_t N, void* stream);
/* F[i][q] = f_i(zt_q): each particle's network at the Nt rows of Zt (F: n x
 * Nt, ldf >= Nt); the same forward pass as dsvgd_score_bnn.  Absent in the
 * reference: replaces evaluating the user's network per particle in torch. */
int dsvgd_bnn_predict(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Zt,
                      int64_t ldz, int64_t Nt, int64_t p, int64_t H, float* F, int64_t ldf,
                      void* stream);

/* ---- Gaussian mixture with diagonal precisions (csrc/gmix.hip) ------------
 *   p(x) = sum_k w~_k N(x; mu_k, diag(1/lam_k)),  w~ = w / sum(w)
 *   c_k  = log w~_k + 1/2 sum_c log lam_kc         (the caller's, from fp64)
 *   q_ik = 1/2 sum_c lam_kc (x_ic - mu_kc)^2,  l_ik = c_k - q_ik,
 *   r_ik = softmax_k(l_ik),  S_ic = sum_k r_ik lam_kc (mu_kc - x_ic),
 *   log p(x_i) = logsumexp_k l_ik - (d/2) log(2 pi).
 * mu, lam: K x d row-major (ldm, ldl >= d), c: K floats.  Exact fp32 in the
 * difference form lam (x - mu)^2; one pass over the components in ascending
 * order with a running maximum (no exponent is taken without it: a particle
 * far from every mode keeps a finite score), so K needs no workspace.  No
 * atomics: the same bits on every call, and a particle's result depends
 * neither on n nor on its row.  Any n >= 1, 1 <= K <= 2^30, 1 <= d <= 1024.
 * Replaces a user logp of this model under autograd (the reference's
 * experiments/gmm.py is the case K = 2, d = 1). */
int dsvgd_score_gmix(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                     int64_t ldm, const float* lam, int64_t ldl, const float* c, int64_t K,
                     float scale, float* S, int64_t lds, void* stream);
/* The same pass without the score: logp_out[i] = log p(x_i) (normalised) and
 * comp_out[i] = argmax_k l_ik, the most responsible component, the lowest
 * index on a tie (n floats, n int32). */
int dsvgd_gmix_assign(const float* X, int64_t ldx, int64_t n, int64_t d, const float* mu,
                      int64_t ldm, const float* lam, int64_t ldl, const float* c, int64_t K,
                      float* logp_out, int32_t* comp_out, void* stream);

/* ---- Bayesian softmax (multiclass logistic) regression (csrc/softmax.hip) --
 * Data rows xd_q in R^p (N x p, ldxd >= p) with labels y_q in {0..C-1} (int32);
 * no bias term: the caller appends a ones column, as for the logistic
 * regression.  A particle is x = [log a | vec(W)], W of shape C x p row-major,
 * d = 1 + C p.  Priors W_ck ~ N(0, 1/a) and a ~ Gamma(a0, b0), a carried as its
 * log with the log-Jacobian (dsvgd_score_bnn's convention, not
 * dsvgd_score_logreg's, which has none):
 *   z_qc  = w_c . xd_q,  pi_qc = softmax_c(z_q.),  a = exp(x_0),
 *   log p = sum_q [z_{q,y_q} - logsumexp_c z_qc] + (C p / 2) x_0 - (a/2) |W|^2
 *           + a0 x_0 - b0 a,
 *   d/dW_c = sum_q (1[y_q = c] - pi_qc) xd_q - a W_c,
 *   d/dx_0 = C p / 2 - (a/2) |W|^2 + a0 - b0 a.
 * S = scale * grad log p for n particles, in exact fp32 (no input is split or
 * scaled), the softmax with its maximum subtracted before any exponent.
 * n > 16: v_mfma_f32_32x32x2_f32 for both products, a workgroup of four waves
 * per 32 particles, the waves sharing the data rows in chunks of 32 through
 * LDS, the softmax lane-local in two passes over the classes, G in registers;
 * more than 16 output tiles (a class x 32 columns each) split over workgroups.
 * n <= 16 (the sequential order's one-particle refresh): a workgroup per
 * particle on the VALU.  The two forms need not agree bit for bit; within a
 * form every sum runs in a fixed order without atomics (the same bits on every
 * call) and a particle's score depends neither on its row nor on the other
 * particles.  No workspace, no allocation, no host sync: only enqueues work.
 * 2 <= C <= DSVGD_SOFTMAX_MAX_CLASSES, p >= 1, d = 1 + C p <= 1024, any n >= 1,
 * 1 <= N <= 2^30; ldx, lds >= d; S's pad columns are left alone.  Absent in
 * the reference: replaces a user logp of this model differentiated by autograd
 * (dsvgd/sampler.py:28-33 _dlogp). */
#define DSVGD_SOFTMAX_MAX_CLASSES 16
int dsvgd_score_softmax(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                        int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p, float a0,
                        float b0, float scale, float* S, int64_t lds, void* stream);
/* The minibatch estimate of the same score: the data sum over the cyclic
 * window of B rows that starts at row c = *cursor, rows (c + q) mod N for
 * q < B, weighted N / B, and the prior terms once; scale applies to the sum.
 * cursor: one int64 in device memory, read by every workgroup (any value:
 * taken mod N) -- the window rule of dsvgd_score_bnn_window;
 * dsvgd_window_advance moves it.  1 <= B <= N.  The same kernels as
 * dsvgd_score_softmax, which is the window of all N rows from row 0. */
int dsvgd_score_softmax_window(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                               int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p,
                               float a0, float b0, float scale, const int64_t* cursor, int64_t B,
                               float* S, int64_t lds, void* stream);
/* The same with the one-workgroup-per-particle form for every n (cursor may
 * be NULL: the window starts at row 0): what the tile form is timed against
 * (scripts/softmax_timing.py).  dsvgd_softmax_small_rows: the largest n the
 * two entry points above give to that form. */
int dsvgd_score_softmax_rows(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xd,
                             int64_t ldxd, const int32_t* y, int64_t N, int64_t C, int64_t p,
                             float a0, float b0, float scale, const int64_t* cursor, int64_t B,
                             float* S, int64_t lds, void* stream);
int64_t dsvgd_softmax_small_rows(void);
/* Posterior-predictive class probabilities of a test set:
 *   P[q][c] = (1/n) sum_i softmax_c(W_i xt_q),  W_i = X[i][1:d] (alpha unused),
 * P: Nt x C (ldp >= C), Xt: Nt x p (ldxt >= p).  fp32; the sum over the
 * particles in a fixed order (per-workgroup partial sums in the workspace,
 * then a finish kernel): the same bits on every call.  workspace of
 * dsvgd_softmax_predict_workspace_bytes(n, Nt, C) bytes. */
size_t dsvgd_softmax_predict_workspace_bytes(int64_t n, int64_t Nt, int64_t C);
int dsvgd_softmax_predict(const float* X, int64_t ldx, int64_t n, int64_t d, const float* Xt,
                          int64_t ldxt, int64_t Nt, int64_t C, int64_t p, float* P, int64_t ldp,
                          void* workspace, void* stream);

/* ---- AdaGrad-conditioned update of the Jacobi order (csrc/adagrad.hip) ----
 * Liu & Wang's rule, per entry of the m moved rows; p = phi (m x d, ldphi) is
 * the whole direction, the h * W2 rows included:
 *   G' = p^2                        where G < 0 (no history: the state starts
 *                                   filled with -1, and the rule never
 *                                   produces a negative entry),
 *   G' = alpha G + (1 - alpha) p^2  elsewhere,
 *   x += step p / (eps + sqrt(G')).
 * X (ldx >= d) and G (ldg >= d) are updated in place.  No iteration counter:
 * a step depends on its inputs alone, so a captured iteration replays
 * correctly.  IEEE sqrt and division (eight roundings from p to x); 16-byte
 * accesses where d, the leading dimensions and the pointers allow them.
 * 0 <= alpha < 1, eps > 0.  Absent in the reference, which takes fixed
 * steps (dsvgd/sampler.py:68). */
int dsvgd_adagrad_step(float* X, int64_t ldx, const float* phi, int64_t ldphi, float* G,
                       int64_t ldg, int64_t m, int64_t d, float step, float alpha, float eps,
                       void* stream);

/* ---- kernelized Stein discrepancy of a Jacobi step's particles ---------
 * (absent in the reference, whose only diagnostics are the test accuracy of
 * experiments/logreg_plots.py and the KDE plot of experiments/gmm_plots.py.)
 * For k = exp(-|x - y|^2 / h) the Stein kernel of the score s is
 *   u_ij = k_ij [s_i.s_j + (2/h)(s_i - s_j).(x_i - x_j) + 2d/h - (4/h^2) D_ij]
 * and t_i = sum_{j != i} u_ij splits into what a step leaves behind -- Y =
 * [Xc | S] (scores unscaled), D, the slices of KY = [K Xc | K S] and rowsum r,
 * h in st -- plus two weighted row sums over D:
 *   t_i = s_i.KS_i + (2/h)[r_i a_i - s_i.KXc_i - xc_i.KS_i + b_i]
 *         + (2d/h) r_i - (4/h^2) q_i,
 *   a_j = s_j.xc_j,  b_i = sum_{j != i} k_ij a_j,  q_i = sum_{j != i} k_ij D_ij,
 * and u_ii = |s_i|^2 + 2d/h.  No float atomics anywhere: the same inputs give
 * the same bits.
 *
 * dsvgd_ksd_rows: the one sweep over the owned block of D.  It first forms a
 * (workspace of roundup(n,128) floats, 16-byte aligned; pads zeroed) from Y
 * with a small kernel of its own, then writes the partials P: `parts` slots
 * of [q | b], 2 roundup(m,128) floats each, parts = dsvgd_ksd_parts(m, n,
 * sym).  Full panel layout (sym = 0; any row0, m <= n): slot z holds column
 * slice z's sums; pads (+inf) and the element j = row0 + i are masked.
 * Symmetric layout (sym = 1: m == n, row0 == 0, dsvgd_sqdist_{h2,x3} layout
 * 1): with T = roundup(n,128)/128 and rparts = parts - T, slot z < rparts
 * holds the row sums of slice z of each tile row's stored tiles (I, J >= I),
 * and slot rparts + I the COLUMN sums of the stored off-diagonal tiles of
 * tile row I, at the rows of J (the terms of the unwritten tile (J, I));
 * entries of slot rparts + I at rows of tiles J <= I are never written nor
 * read, a diagonal tile counts once without its diagonal, tiles J < I are
 * not read. */
int64_t dsvgd_ksd_parts(int64_t m, int64_t n, int sym);
int dsvgd_ksd_rows(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t dp, int64_t d,
                   int64_t row0, int64_t m, int64_t n, const dsvgd_select_state* st, int sym,
                   int64_t parts, float* P, float* a, void* stream);
/* t_i and u_ii of the owned rows from the `splits` slices of KY / rowsum
 * (summed in slice order like dsvgd_phi_finish; the dot products in fp64) and
 * the slots of P (in slot order); rows[i] = t_i (m floats, nullable); the
 * sums over the owned rows in fp64 in a fixed two-level order (ws:
 * dsvgd_ksd_workspace_doubles(m) doubles, one pair per 64 rows); out[0] =
 * sum_i t_i, out[1] = sum_i u_ii, out[2] = V = (out[0] + out[1]) / n^2,
 * out[3] = U = out[0] / (n (n - 1)) (NaN for n = 1).  For m < n only
 * out[0], out[1] and rows are meaningful (a row block's share). */
size_t dsvgd_ksd_workspace_doubles(int64_t m);
int dsvgd_ksd_finish(const float* KY, int64_t ldk, const float* rowsum, int64_t splits,
                     const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0, int64_t m,
                     int64_t n, const dsvgd_select_state* st, int sym, int64_t parts,
                     const float* P, float* rows, double* ws, double* out, void* stream);
/* The FmtH2 image of K (dsvgd_phi_mm_h2: fp16 pairs of 2^15 k) keeps an
 * absolute 2^-40 per entry, harmless to phi (measured against the self term
 * k_ii = 1) but not to a row of the KSD whose whole off-diagonal kernel mass
 * r_i is tiny -- an outlier, a diverging step, a collapsed bandwidth: a row's
 * KY error is up to n 2^-40 max|Y| against terms of size r_i.  gate[0]
 * (device float) = 1.0 if an owned row has r_i < n 2^-20 (that error above
 * ~1e-6 of the row's terms) or NaN, else 0.0; n = 1: 0.0.  The caller then
 * launches dsvgd_ysplit + dsvgd_phi_mm_x3 (or dsvgd_phi_mm_gated) with this
 * gate into the same KY / rowsum -- bf16 parts have fp32's exponent range --
 * before dsvgd_ksd_finish: nothing runs while the gate reads 0. */
int dsvgd_ksd_gate(const float* rowsum, int64_t splits, int64_t m, int64_t n, float* gate,
                   void* stream);
/* d <= 64 (used for d <= 2, beside dsvgd_phi_direct, which leaves no KY):
 * the same rows and out from explicit differences on the VALU, straight from
 * Y -- u_ij per pair with D_ij = |x_i - x_j|^2 recomputed; the r x - K X form
 * cancels at d = 1.  Same ws and second-level reduction as dsvgd_ksd_finish. */
int dsvgd_ksd_direct(const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0, int64_t m,
                     int64_t n, const dsvgd_select_state* st, float* rows, double* ws, double* out,
                     void* stream);

/* ---- a second radial kernel: the inverse multiquadric (IMQ) --------------
 * The reference takes any kernel(x, y) callable and differentiates it by
 * autograd per pair (dsvgd/sampler.py:7-40, dsvgd/distsampler.py:84-101).
 * Beside k = exp(-|x - y|^2 / h) the engine has
 *   k(x, y) = (1 + |x - y|^2 / h)^beta = u^beta,   -1 <= beta < 0,
 * the kernel recommended for the KSD above a handful of dimensions (Gorham &
 * Mackey 2017).  It is radial: the same D, the same bandwidth in `st`, the
 * same engines.  Its gradient is not a multiple of itself, so it takes two
 * kernel matrices: with F = u^beta, G' = u^(beta-1), c1 = -2 beta / h,
 *   phi_i = inv_n [ s_i + (F S)_i + c1 (rG_i xc_i - (G' Xc)_i) ],
 *   rG_i = sum_{j != i} G'_ij
 * (the diagonal is skipped in both products; its term is s_i).  All powers of
 * u lie in (0, 1] and the +inf pads of D map to 0, as exp(-D/h) does.
 *
 * A kernel is described on the host and passed BY VALUE to the entry points
 * below, each beside the one it extends (no process-wide setting).  Both
 * names reach one implementation: the plain name is the _kern call with the
 * RBF family (the same checks, error texts and launches). */
#define DSVGD_KERNEL_RBF 0 /* exp(-|x - y|^2 / h); beta is ignored          */
#define DSVGD_KERNEL_IMQ 1 /* (1 + |x - y|^2 / h)^beta, beta in [-1, 0)     */
typedef struct dsvgd_kernel {
  int32_t family;
  float beta;
} dsvgd_kernel;

/* dsvgd_phi_mm{,_gated,_x3,_h2} with the kernel `kern` fused into the A
 * operand.  IMQ stages ONE power of u, u^e 2^15 = exp2(e log2(fma(D, 1/h, 1))
 * + 15) (the FmtH2 A scale 2^15 as the RBF's; c1 is applied by the finish):
 * order 0: e = beta (F), order 1: e = beta - 1 (G'; IMQ only) -- e is a launch
 * argument, so both run the same code.  Same layouts, split-K slices,
 * diagonal rule, range-guard gates and limits as the call each one extends
 * (dsvgd_phi_mm_kern: gate == NULL is dsvgd_phi_mm, else dsvgd_phi_mm_gated).
 * An IMQ direction is two calls (order 0 and 1) into two KY / rowsum pairs,
 * then dsvgd_phi_finish_imq.  Replaces the kernel and its autograd gradient
 * in dsvgd/sampler.py:26-40 for an IMQ callable. */
int dsvgd_phi_mm_kern(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t row0,
                      int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits,
                      float* KY, int64_t ldk, float* rowsum, const float* gate,
                      dsvgd_kernel kern, int order, void* stream);
int dsvgd_phi_mm_x3_kern(const float* D, int64_t ldd, const void* Yx, int64_t ldy, int64_t row0,
                         int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits,
                         float* KY, int64_t ldk, float* rowsum, int sym, int m16,
                         const float* gate, dsvgd_kernel kern, int order, void* stream);
int dsvgd_phi_mm_h2_kern(const float* D, int64_t ldd, const void* Yh, int64_t ldy, int64_t row0,
                         int64_t m, int64_t n, const dsvgd_select_state* st, int64_t splits,
                         float* KY, int64_t ldk, float* rowsum, int sym, const float* colinv,
                         const float* gate, dsvgd_kernel kern, int order, void* stream);
/* dsvgd_phi_finish for the IMQ kernel: KF = the order-0 run's [F Xc | F S]
 * (only F S is read), KG = the order-1 run's [G' Xc | G' S] (only G' Xc) and
 * its row sums `rowsum` = rG, `splits` slices each, summed in slice order;
 * phi as above, extra / phi / X as dsvgd_phi_finish (the update of
 * dsvgd/sampler.py:68 / dsvgd/distsampler.py:200, Jacobi order). */
int dsvgd_phi_finish_imq(const float* KF, int64_t ldkf, const float* KG, int64_t ldkg,
                         const float* rowsum, int64_t splits, const float* Y, int64_t ldy,
                         int64_t row0, int64_t m, int64_t d, int64_t dp,
                         const dsvgd_select_state* st, dsvgd_kernel kern, float inv_n, float step,
                         const float* extra, int64_t lde, float* phi, int64_t ldphi, float* X,
                         int64_t ldx, void* stream);
/* dsvgd_phi_direct with a kernel: IMQ sums F_ij s_j + c1 G'_ij (x_i - x_j)
 * per pair (dsvgd/sampler.py:38-40 with an IMQ kernel). */
int dsvgd_phi_direct_kern(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t row0,
                          int64_t m, int64_t n, int64_t d, const dsvgd_select_state* st,
                          float inv_n, float step, const float* extra, int64_t lde, float* phi,
                          int64_t ldphi, float* X, int64_t ldx, float* partial,
                          int64_t partial_floats, dsvgd_kernel kern, void* stream);
/* dsvgd_phi_row / dsvgd_phi_row_split with a kernel (dsvgd/sampler.py:64-68
 * with an IMQ kernel): IMQ keeps a second per-column coefficient, F_j on s_j
 * and c1 G'_j on x_i - x_j (d <= 7808 for dsvgd_phi_row_kern; twice the rows'
 * LDS for the split form). */
int dsvgd_phi_row_kern(float* X, int64_t ldx, const float* S, int64_t lds, int64_t n_int,
                       int64_t d, int64_t i, const dsvgd_select_state* st, float step,
                       const float* extra, float* phi_out, dsvgd_kernel kern, void* stream);
int dsvgd_phi_row_split_kern(float* X, int64_t ldx, const float* S, int64_t lds, int64_t n,
                             int64_t d, int64_t i, const dsvgd_select_state* st, float step,
                             const float* extra, float* phi_out, float* partial, int64_t blocks,
                             dsvgd_kernel kern, void* stream);
/* The KSD with a kernel (absent in the reference, as above).  For the IMQ,
 * with H' = u^(beta-2) and c2 = 4 beta (beta - 1) / h^2,
 *   u_ij = F s_i.s_j + c1 G' [(s_i - s_j).(x_i - x_j) + d] - c2 H' D_ij,
 *   u_ii = |s_i|^2 + c1 d,
 *   t_i = s_i.FS_i + c1 [rG_i a_i - s_i.G'Xc_i - xc_i.G'S_i + b_i + d rG_i]
 *         - c2 q_i,   b_i = sum_{j != i} G'_ij a_j,  q_i = sum_{j != i} H'_ij D_ij.
 * dsvgd_ksd_rows_kern: dsvgd_ksd_rows' sweep, slots and layouts with these b
 * and q.  dsvgd_ksd_gate reads the G' run's row sums rG; its fallback reruns
 * both products on the gate.  dsvgd_ksd_finish_imq: dsvgd_ksd_finish from the
 * two runs' slices (KF: F S; KG: G' Xc and G' S; rowsum: rG).
 * dsvgd_ksd_direct_kern: dsvgd_ksd_direct per pair.  Deterministic as above. */
int dsvgd_ksd_rows_kern(const float* D, int64_t ldd, const float* Y, int64_t ldy, int64_t dp,
                        int64_t d, int64_t row0, int64_t m, int64_t n,
                        const dsvgd_select_state* st, int sym, int64_t parts, float* P, float* a,
                        dsvgd_kernel kern, void* stream);
int dsvgd_ksd_finish_imq(const float* KF, int64_t ldkf, const float* KG, int64_t ldkg,
                         const float* rowsum, int64_t splits, const float* Y, int64_t ldy,
                         int64_t dp, int64_t d, int64_t row0, int64_t m, int64_t n,
                         const dsvgd_select_state* st, dsvgd_kernel kern, int sym, int64_t parts,
                         const float* P, float* rows, double* ws, double* out, void* stream);
int dsvgd_ksd_direct_kern(const float* Y, int64_t ldy, int64_t dp, int64_t d, int64_t row0,
                          int64_t m, int64_t n, const dsvgd_select_state* st, float* rows,
                          double* ws, double* out, dsvgd_kernel kern, void* stream);

/* ---- maximum mean discrepancy between two particle sets (csrc/mmd.hip) ---
 * (absent in the reference.)  The pooled set Z = [P; Q] of N = n_first + m
 * particles is packed as one interacting set; D is its N x N distance matrix
 * (the whole matrix: full panel layout, or the symmetric layout of
 * dsvgd_sqdist_{h2,x3} layout 1), k the RBF or IMQ kernel at the bandwidth in
 * st.  With
 *   rP_i = sum_{j < n_first, j != i} k_ij,   rQ_i = sum_{j >= n_first, j != i} k_ij,
 *   PP = sum_{i < n_first} rP_i,  PQ = sum_{i < n_first} rQ_i,  QQ = sum_{i >= n_first} rQ_i,
 * and n = n_first, m = N - n_first:
 *   V = (PP + n)/n^2 + (QQ + m)/m^2 - 2 PQ/(n m)         (k_ii = 1 exactly)
 *   U = PP/(n (n-1)) + QQ/(m (m-1)) - 2 PQ/(n m)         (NaN if n = 1 or m = 1)
 *   witness_i = (rP_i + [i < n])/n - (rQ_i + [i >= n])/m.
 * The diagonal of D is never read.  No float atomics: every partial has a slot
 * of its own and every sum a fixed order, so two calls give the same bits.
 *
 * dsvgd_mmd_rows: the one sweep over D.  P: `parts` slots of [rP | rQ], 2
 * roundup(N,128) floats each, parts = dsvgd_mmd_parts(N, sym, force).  Full
 * layout: slot z holds column slice z's sums.  Symmetric layout, T =
 * roundup(N,128)/128, rparts = parts - T: slot z < rparts holds the row sums
 * of slice z of each tile row's stored tiles (I, J >= I); slot rparts + I the
 * column sums of the stored off-diagonal tiles of tile row I at the rows of J
 * (the terms of the unwritten tile (J, I), each sent to rP or rQ by the class
 * of its row i in I); entries of slot rparts + I at rows of tiles J <= I are
 * never written nor read.  Pads (+inf) and the diagonal contribute exactly 0.
 * dsvgd_mmd_parts: force <= 0: the slice count that fills the CUs (the rule
 * of dsvgd_ksd_parts); force > 0: min(force, roundup(N,128)/128) row / column
 * slices (tests: more than one slice on a small matrix, or one on a large).
 * dsvgd_mmd_finish: the slots summed in slot order (fp64); rp, rq, witness
 * (N floats each, nullable); ws: dsvgd_mmd_workspace_doubles(N) doubles (three
 * per 64 rows); out[0..4] = PP, PQ, QQ, V, U (fp64 sums in a fixed two-level
 * order). */
int64_t dsvgd_mmd_parts(int64_t n_total, int sym, int64_t force);
size_t dsvgd_mmd_workspace_doubles(int64_t n_total);
int dsvgd_mmd_rows(const float* D, int64_t ldd, int64_t n_total, int64_t n_first,
                   const dsvgd_select_state* st, dsvgd_kernel kern, int sym, int64_t parts,
                   int64_t force, float* P, void* stream);
int dsvgd_mmd_finish(const float* P, int64_t n_total, int64_t n_first, int sym, int64_t parts,
                     int64_t force, float* rp, float* rq, float* witness, double* ws,
                     double* out, void* stream);

/* ---- projected SVGD (csrc/project.hip) ---------------------------------------
 * The three dense products around an r-wide SVGD step in the subspace spanned
 * by the orthonormal columns of Psi (d x r, row-major, row stride ldpsi), for
 * n particles X and their scores S (row-major, row strides >= d):
 * 1 <= d <= 1024, 1 <= r <= min(d, 256), n >= 1.  All run on the exact f32
 * MFMA (v_mfma_f32_32x32x2_f32), without atomics and with every sum in a fixed
 * order: two calls give the same bits.
 *
 * dsvgd_proj_gram: H = (1/n) sum_i g_i g_i^T (d x d, row stride ldh), g_i =
 * S_i + X_i (add_x != 0; rounded to f32 once) or S_i (add_x == 0; X is not
 * read and may be null).  Only the tiles on and above the diagonal are
 * computed; every entry is written together with its mirror image, so H is
 * exactly symmetric.  The particles are split into dsvgd_proj_gram_slices(n, d)
 * slices of whole 32-row chunks (none empty; one slice up to 256 particles, no
 * accumulator chain longer than 8192), whose partial sums meet in slice order.
 * workspace: dsvgd_proj_gram_workspace_bytes(n, d) bytes.
 *
 * dsvgd_proj_apply: Xr = X Psi and Sr = S Psi (n x r) in one launch; X and S
 * are each read once.
 *
 * dsvgd_proj_lift: X += step . Phir Psi^T (Phir n x r); a non-null Phi_out
 * (n x d, row stride ldo) is set to Phir Psi^T.  step == 0: X is neither read
 * nor written (and may be null). */
int64_t dsvgd_proj_gram_slices(int64_t n, int64_t d);
size_t dsvgd_proj_gram_workspace_bytes(int64_t n, int64_t d);
int dsvgd_proj_gram(const float* X, int64_t ldx, const float* S, int64_t lds, int64_t n, int64_t d,
                    int add_x, void* workspace, float* H, int64_t ldh, void* stream);
int dsvgd_proj_apply(const float* X, int64_t ldx, const float* S, int64_t lds, int64_t n,
                     int64_t d, const float* Psi, int64_t ldpsi, int64_t r, float* Xr,
                     int64_t ldxr, float* Sr, int64_t ldsr, void* stream);
int dsvgd_proj_lift(const float* Phir, int64_t ldphi, const float* Psi, int64_t ldpsi, int64_t n,
                    int64_t d, int64_t r, float step, float* X, int64_t ldx, float* Phi_out,
                    int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSVGD_H_ */
