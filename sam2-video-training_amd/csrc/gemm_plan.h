// GEMM dispatch as one pure function: which kernel, which tiling, how many K splits, into which storage.
//
//   gemm_plan(problem, knobs, workspace_bytes) -> GemmPlan
//
// Plain host C++17: no HIP header, no globals, no launches, no memory touched -- it compiles with g++ and
// runs without a GPU (gemm_plan_host_check.cpp, tests/test_gemm_plan_host.py).  The launch side
// (gemm_bf16.hip s2h_gemm_bf16, gemm_wgrad.hip, gemm.hip) fills a GemmProblem from its pointers and
// pitches, calls gemm_plan once and switches on the result.
//
// Order of precedence for a bf16 GEMM (each step only with no forced tiling, knobs.cfg == 0):
//   1. K = 1 without epilogue                                   -> the outer-product kernel
//   2. tiny split-K (opt-in, no tiny_cfg), when the workspace holds it
//   3. fp32 output, K >= 512: the deterministic weight-gradient kernel, when the workspace holds one split
//   4. a tiling number: the forced one, else gemm_pick_cfg, then in this order tiny_cfg (M <= 128), the
//      4 x 1 wave grids (w41), the A-in-registers rule (areg), the per-class configuration
//   5. number < 0, or operands the LDS-DMA path cannot address    -> the register-staged kernel
//      A-in-registers number on a shape it cannot take, or an unknown number -> CFG_128
//   6. the generic split-K plan for the tile of 5.
// The cost model below is compared with strict `<` in double: do not build this header with -ffast-math or
// -march=native (a contraction into FMA could change a tie).
#ifndef S2H_GEMM_PLAN_H  // (an include guard: the header also compiles alone, where `#pragma once` warns)
#define S2H_GEMM_PLAN_H
#include <algorithm>
#include <cstdint>

// LDS-DMA tilings (s2h_gemm_config selects one for A/B measurements; 0 = automatic)
enum GemmCfg {
  CFG_AUTO = 0, CFG_64 = 1, CFG_128 = 2, CFG_128_NS3 = 3, CFG_256x128 = 4, CFG_256 = 5, CFG_128x256 = 6,
  CFG_128x64 = 7, CFG_64x128 = 8, CFG_64_NS3 = 9, CFG_64_K32_NS4 = 10, CFG_128x64_K32_NS3 = 11,
  CFG_128x64_K32_NS4 = 12, CFG_128x64_NS3 = 13, CFG_256x128_W4_K32_NS3 = 14, CFG_256x128_W4_K64 = 15,
  CFG_128_K32_NS3 = 16, CFG_256x64_W4_K32_NS3 = 17, CFG_64_NS4 = 18, CFG_64_K32_NS8 = 19,
  // 4 x 1 wave grids: every wave owns whole 64-column rows of the tile (128-B bf16 output rows)
  CFG_64_W41 = 20, CFG_128x64_W41 = 21, CFG_128x64_W41_K32_NS3 = 22, CFG_64_W41_NS4 = 23, CFG_128x64_W41_NS3 = 24,
  // full-row tiles (round 4): one workgroup owns 64 rows x the whole N <= 256 output width, the four
  // waves stacked along M (16 full rows each), the K ring 4 stages deep (K <= 256 in one round trip)
  CFG_64x256_W41_NS4 = 25, CFG_64x128_W41_NS4 = 26, CFG_64x256_W41_NS3 = 27, CFG_64x256_W41_K32_NS4 = 28,
  // short K (round 4): A in registers, only B through LDS (gemm16a_kernel), K <= 256
  CFG_64_AREG = 29, CFG_64x128_AREG = 30,
  CFG_REGS = 99
};

struct GemmTile {
  int BM, BN, WGM, WGN, NS, BK;
};

// the tile of a GemmCfg number 1..30 (the template arguments of its instantiation in gemm_cfg*.hip, which
// launch_glds checks against the plan); false: not a tiling number
inline bool gemm_cfg_tile(int cfg, GemmTile& t) {
  static const GemmTile tiles[31] = {
      {0, 0, 0, 0, 0, 0},        {64, 64, 2, 2, 2, 64},    {128, 128, 2, 2, 2, 64},  {128, 128, 2, 2, 3, 64},
      {256, 128, 4, 2, 2, 64},   {256, 256, 2, 4, 2, 64},  {128, 256, 2, 4, 2, 64},  {128, 64, 2, 2, 2, 64},
      {64, 128, 2, 2, 2, 64},    {64, 64, 2, 2, 3, 64},    {64, 64, 2, 2, 4, 32},    {128, 64, 2, 2, 3, 32},
      {128, 64, 2, 2, 4, 32},    {128, 64, 2, 2, 3, 64},   {256, 128, 2, 2, 3, 32},  {256, 128, 2, 2, 2, 64},
      {128, 128, 2, 2, 3, 32},   {256, 64, 4, 1, 3, 32},   {64, 64, 2, 2, 4, 64},    {64, 64, 2, 2, 8, 32},
      {64, 64, 4, 1, 2, 64},     {128, 64, 4, 1, 2, 64},   {128, 64, 4, 1, 3, 32},   {64, 64, 4, 1, 4, 64},
      {128, 64, 4, 1, 3, 64},    {64, 256, 4, 1, 4, 64},   {64, 128, 4, 1, 4, 64},   {64, 256, 4, 1, 3, 64},
      {64, 256, 4, 1, 4, 32},    {64, 64, 4, 1, 1, 64},    {64, 128, 4, 1, 1, 64}};
  if (cfg < 1 || cfg > 30) return false;
  t = tiles[cfg];
  return true;
}

// profiler tag of a GEMM tiling (include/sam2hip.h, s2h_prof_read_tags); bit 41: the deterministic
// weight-gradient kernel
inline int64_t gemm_tag(int BM, int BN, int WGM, int WGN, int NS, int BK, bool akc, bool bkc, bool regs, bool mx8,
                        bool areg = false) {
  return (int64_t)BM | ((int64_t)BN << 10) | ((int64_t)WGM << 20) | ((int64_t)WGN << 24) | ((int64_t)NS << 28) |
         ((int64_t)(BK / 32) << 32) | ((int64_t)akc << 36) | ((int64_t)bkc << 37) | ((int64_t)regs << 38) |
         ((int64_t)mx8 << 39) | ((int64_t)areg << 40);
}

// One GEMM call, as far as the dispatch looks at it.  C[b](m, n) over `batch` problems of M x N x K.
struct GemmProblem {
  int batch, M, N, K;
  // layout: each operand addressed through (row, k) strides, one of them 1
  bool a_kc, a_rc;  // A: K-contiguous (lda_k == 1) / row-contiguous (lda_m == 1)
  bool b_kc, b_rc;  // B: K-contiguous (ldb_k == 1) / row-contiguous (ldb_n == 1)
  bool f32_in;      // fp32 operands (and output): gemm.hip's own kernel
  bool f32_out;     // bf16 operands with an fp32 output
  // the epilogue ("plain" = none of these, beta 0 or 1)
  bool bias, R, X, cscale, dropout;
  int act;
  float beta;
  bool rowsum, rope;
  // alignment facts, computed by the caller from pointers and pitches
  int64_t lda, ldb;  // the pitch of each operand (elements): lda_m if a_kc else lda_k; ldb_n if b_kc else ldb_k
  bool a16, b16;     // base addresses 16-B aligned
  bool sa8, sb8;     // batch strides multiples of 8 elements
};

// Every setting of the dispatch, with its default.  One instance in the library (g_gemm_knobs,
// gemm_bf16.hip), written by the extern "C" setters.
struct GemmKnobs {
  int cfg = CFG_AUTO;  // forced tiling (s2h_gemm_config bits 0-7; < 0: the register-staged kernel)
  int dbg = 0;         // measurement-only ablations (s2h_gemm_config bits 8+, gemm16.h GemmArgs16::dbg)
  int tiny_cfg = CFG_AUTO;  // A/B knob: tiling of GEMMs with M <= 128 (s2h_gemm_tiny_config)
  // 4 x 1 wave grids instead of the 2 x 2 ones for bf16 outputs (1: every such GEMM, the default;
  // 2: only N >= 768; 0: off); bit-identical results.  In-step env A/B (tools/gpu_r3q.sh,
  // S2H_GEMM_W41 0 / 1 / 2, two rounds): 136.77 / 136.71, 136.98 / 137.05, 136.68 / 136.86 clip-frames/s
  int w41 = 1;
  // Short K that is not a whole number of 64-deep stages (Hiera's 112 / 224 channels, the V-fold's 72,
  // the memory encoder's 64 + 8 ...) on the A-in-registers tiling: no zero-filled tail stage, no
  // extra barrier, 5 workgroups per CU (tools/areg_bench.py, profiles/r04_v11_areg.log: 32768x224x224
  // 22.1 -> 17.2 us, 8192x448x112 9.3 -> 8.3, 13312x256x72 9.7 -> 8.4; at K = 128 / 256 the LDS-DMA
  // tilings stay ahead).  1 = on (default), 0 = off (A/B, S2H_GEMM_AREG)
  int areg = 1;
  // A/B knob (round 6): the tiling of one class of bf16-output GEMMs (gemm_class), 0 = the shape rules.
  // Defaults (round 6): classes 4 / 5 on the 128 x 64 4 x 1 LDS-DMA tiling with 32-deep stages, 3-deep ring
  // (cfg 22) instead of the A-in-registers kernel: in-step sweeps 47.59 / 47.52 -> 47.45 / 47.44 ms
  // (profiles/r06_v12_gemm_class4_sweep.log, r06_v13_gemm_class45_sweep.log); every other class keeps its rules.
  int class_cfg[6] = {0, 0, 0, 0, CFG_128x64_W41_K32_NS3, CFG_128x64_W41_K32_NS3};
  // tiny split-K (gemm_plan_tiny_splitk): measured neutral in-step (profiles/r06_v9_tiny_splitk_ab.log): opt-in
  int tiny_splitk = 0;
  // workgroups a split-K launch aims at (s2h_gemm_split_target)
  // (512 -- one round of two workgroups per CU -- won the hot-cache sweep, profiles/r03_v6_wgrad_sweep.log,
  // but lost inside the step, profiles/r03_v6_trace_diff.log: kept at 768)
  int split_target = 768;
  int f32_small = 1;   // A/B knob (s2h_gemm_f32_small): fp32 GEMMs of < 64 tiles on 32 x 32 tiles
  int wg_kmin = 4096;  // reductions at least this long take the deterministic kernel (0: it and the workspace off)
  // measurement override (s2h_wgrad_force): the weight-gradient tile (-1 = the cost model) and split count (0)
  int wg_force_tile = -1, wg_force_splits = 0;
};

enum GemmKind {
  GEMM_OUTER = 0,        // K = 1: gemm_outer_kernel
  GEMM_TINY_SPLITK = 1,  // one fp32 launch over S K chunks into the workspace + gemm_splitk_epi_kernel
  GEMM_WGRAD_DET = 2,    // gemm_wg_kernel + gemm_wg_reduce_kernel (gemm_wgrad.hip)
  GEMM_GLDS = 3,         // gemm16g_kernel, an LDS-DMA tiling
  GEMM_AREG = 4,         // gemm16a_kernel, A in registers
  GEMM_REGS = 5,         // gemm16_kernel, register-staged
  GEMM_F32 = 6           // gemm_kernel<float> (gemm.hip)
};

struct GemmPlan {
  int kind = GEMM_GLDS;
  int cfg = 0;  // GemmCfg number of the tiling (CFG_REGS for the register-staged kernel; 0: it has none)
  GemmTile tile = {0, 0, 0, 0, 0, 0};
  // K range k of split s: [s * kchunk, min(K, (s + 1) * kchunk)); tiny split-K: S = splits chunks of K / S
  int splits = 1, kchunk = 0;
  bool use_ws = false;   // the splits' partials go to the workspace, a second launch adds them in split order
  bool atomic = false;   // the splits add into C with float atomics (no workspace)
  bool zero_c = false;   // ... and C (beta 0) is zeroed first
  int64_t ws_floats = 0;  // workspace floats the launch needs
  // the weight-gradient kernel: its tile (gemm_wg_tile), the operand extents padded to 8, the reduce slices
  int wg_tile = -1, Md = 0, Nd = 0, sl = 0;
  int64_t tag = 0;  // profiler tag (0: none recorded)
};

// ------------------------------------------------------------------------------------------ eligibility
inline bool gemm_plain(const GemmProblem& p) {
  return p.f32_out && !p.bias && !p.R && !p.X && !p.cscale && !p.dropout && p.act == 0 &&
         (p.beta == 1.f || p.beta == 0.f);
}

// workspace bytes the deterministic reductions may use (s2h_det_ws_bytes): wg_kmin 0 switches them off
inline int64_t gemm_ws_usable(const GemmKnobs& k, int64_t ws_bytes) { return k.wg_kmin > 0 && ws_bytes > 0 ? ws_bytes : 0; }

// The LDS-DMA form's requirements (else the register-staged kernel runs): 16-B aligned bases, row
// strides and batch strides multiple of 8 elements, the contiguous extent of every operand a multiple
// of 8, per-batch operand extents addressed with 32-bit element offsets in GImg::dma
inline bool gemm_glds_ok(const GemmProblem& p) {
  const int aext = p.a_kc ? p.K : p.M, bext = p.b_kc ? p.K : p.N;  // contiguous extents
  const int64_t aspan = p.a_kc ? (int64_t)p.M * p.lda : (int64_t)p.K * p.lda;
  const int64_t bspan = p.b_kc ? (int64_t)p.N * p.ldb : (int64_t)p.K * p.ldb;
  return p.a16 && p.b16 && p.lda % 8 == 0 && p.ldb % 8 == 0 && aext % 8 == 0 && bext % 8 == 0 &&
         (p.batch == 1 || (p.sa8 && p.sb8)) && p.K > 0 && aspan < (1ll << 31) && bspan < (1ll << 31);
}

// gemm16a_kernel's requirements: K-contiguous A, K <= kmax, no split-K, no fused row sums
inline bool gemm_areg_ok(const GemmProblem& p, int kmax) {
  return p.a_kc && p.K <= kmax && p.K > 0 && !p.rowsum && p.a16 && p.lda % 8 == 0 && p.K % 8 == 0 && p.sa8;
}

// --------------------------------------------------------------------------------------- tiling by shape
// Tiling by shape.  rocprofv3 kernel traces of tools/gemm_one.py (tools/kt_gemm.sh,
// profiles/r01_v14_gemm_tilings.txt) and the per-shape table of a profiled training step
// (bench.py --kernel-table with S2H_GEMM_CFG forced to 1 / 7, profiles/r01_v14_gemm_cfg_step.txt):
//  * 128x64 (4 waves of 32x32, 24 KB per stage) wins where it still yields >= 1024 tiles --
//    13312x2048x256 35.7 us vs 38.2 (64^2) / 40.0 (128^2), 131072x448x112 70.1 vs 77.5 --
//    and on split-K weight gradients with >= 64 of its tiles (2048x256x13312: -17 %);
//  * 64^2 wins on the narrow outputs (N = 128..256 of 13312 rows, 416 tiles at 128x64: the
//    occupancy of the smaller tile hides the LDS-DMA latency) and on tiny weight gradients;
//  * 256^2 (8 waves) only pays on large square problems (4096^3: 146 us vs 170 for 128^2).
inline int gemm_pick_cfg(const GemmProblem& a) {
  const int batch = a.batch;
  // M <= 128 (decoder tokens, pooled heads): 64^2 tiles with a 4-deep ring -- the in-step env A/B
  // (tools/gpu_r3n.sh, S2H_GEMM_TINY_CFG 0 / 19 / 18, two rounds) measured 137.5 / 137.3 clip-frames/s
  // for the default rules, 136.9 / 137.0 for the 8-deep K32 ring and 137.8 / 138.0 for this one
  if (a.M <= 128) return CFG_64_NS4;
  const long t256 = (long)((a.M + 255) / 256) * ((a.N + 255) / 256) * batch;
  if (a.M >= 1024 && a.N >= 1024 && a.K >= 1024 && t256 >= 128) return CFG_256;
  const long t128x64 = (long)((a.M + 127) / 128) * ((a.N + 63) / 64) * batch;
  const bool split = a.f32_out && a.K >= 1024 && t128x64 < 512;  // gemm_plan_splits' split-K regime
  // deep K on large grids: 128x128 (tools/epi_bench.py: 93184x256x2048 175 -> 139 us; below
  // 512 of its tiles the 128x64 form stays ahead, e.g. 8192x448x1792 24 vs 29 us)
  const long t128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128) * batch;
  // >= 1024 tiles of 128^2 with K >= 256 on the frame-batched backward's row counts: 32-deep
  // stages, 3-deep ring (tools/gemm_cfg_sweep.py, profiles/r03_v4_gemm_cfg_sweep.log: dgrad
  // 93184x256x2048 215 -> 188 us, 93184x256x256 32.6 -> 29.3, 93184x2048x256 148 -> 142; the
  // 13312-row forward shapes won in isolation but lost inside the step: 13312x2048x256 with its
  // ReLU + dropout epilogue 50.7 -> 57.8 us per launch, profiles/r03_v5_kernel_table.txt)
  if (!split && a.M >= 32768 && a.K >= 256 && a.N >= 256 && t128 >= 1024) return CFG_128_K32_NS3;
  if (!split && a.K >= 1024 && t128 >= 512) return CFG_128;
  // shallow K (<= 256) on large grids: 32-deep stages, 3-deep ring (tools/epi_bench.py graph
  // replays: 131072x448x112 70 -> 58 us, 32768x672x224 35 -> 28, 93184x2048x256 222 -> 216;
  // below ~2k tiles or at K >= 448 the 64-deep 2-stage form stays ahead)
  // (tools/dgrad_bench.py: the same holds for narrow outputs up to K = 1024 -- dgrad 32768x224
  // over K = 672: 29.2 -> 24.4 us, 131072x112 over K = 448: 43.9 -> 40.3)
  if (!split && t128x64 >= 1024 && (a.K <= 256 ? t128x64 >= 2048 : (a.N <= 256 && a.K <= 1024)))
    return CFG_128x64_K32_NS3;
  if (split ? t128x64 >= 64 : t128x64 >= 1024) return CFG_128x64;
  return CFG_64;
}

// the 4 x 1 wave grid of a 2 x 2 tiling (knobs.w41)
inline int gemm_w41_of(int cfg) {
  switch (cfg) {
    case CFG_64: return CFG_64_W41;
    case CFG_128x64: return CFG_128x64_W41;
    case CFG_128x64_K32_NS3: return CFG_128x64_W41_K32_NS3;
    case CFG_64_NS4: return CFG_64_W41_NS4;
    case CFG_128x64_NS3: return CFG_128x64_W41_NS3;
    default: return cfg;
  }
}

// The classes of bf16-output GEMMs (M > 128) that knobs.class_cfg can move to another tiling; -1: none.
//   class 0: K >= 1024, N <= 512 (long reduction, narrow output: the memory-attention FFN linear2, the
//            memory fuser pwconv2, Hiera MLP fc2)
//   class 1: K <= 256, N <= 256, M >= 8192 (short reduction, narrow output: per-frame projections)
//   class 2: K <= 512, N >= 768 (wide output: FFN linear1, Hiera qkv / fc1)
//   class 3: 256 < K < 1024, N <= 512 (mid reduction, narrow output: Hiera proj)
//   class 4: K < 256 not a multiple of 64 (the A-in-registers domain), M >= 65536 (Hiera stage 1 at
//            112 channels: 131072 rows at 512^2)
//   class 5: the same with M < 65536 and K >= 128 (Hiera stage 2 at 224 channels)
inline int gemm_class(const GemmProblem& a) {
  if (a.f32_out || a.M <= 128) return -1;
  // (K < 128 with M < 65536 -- the V-fold out projection, 13312x256x72 -- stays on the A-in-registers
  // rule: 12.45 us there vs 14.21 on cfg 22, profiles/r06_v3 vs r06_v37 shape tables)
  if (a.K < 256 && a.K % 64 != 0) return a.M >= 65536 ? 4 : (a.K >= 128 ? 5 : -1);
  if (a.K >= 1024 && a.N <= 512) return 0;
  if (a.K <= 256 && a.N <= 256 && a.M >= 8192) return 1;
  if (a.K <= 512 && a.N >= 768) return 2;
  if (a.K > 256 && a.K < 1024 && a.N <= 512) return 3;
  return -1;
}

// the full-row tiling of s2h_linear_add_ln / s2h_linear_dgrad_ln_bwd (N = 128 or 256, gemm_cfg6.hip)
inline int gemm_full_row_cfg(int N, int K) {
  return N == 128 ? CFG_64x128_W41_NS4 : (K <= 256 ? CFG_64x256_W41_NS4 : CFG_64x256_W41_NS3);
}

// the register-staged kernel's tile edge (128^2 or 64^2)
inline int gemm_regs_tile(const GemmProblem& a) {
  const long t128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128) * a.batch;
  return (t128 >= 256 || (a.M >= 128 && a.N >= 128 && a.K >= 1024)) ? 128 : 64;
}

// the fp32 kernel's tile edge
inline int gemm_f32_tile(const GemmProblem& a, const GemmKnobs& k) {
  // Small problems: 64x64 tiles keep enough workgroups in flight on 256 CUs.
  const long tiles128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128) * a.batch;
  if (tiles128 >= 512) return 128;
  // fp32 problems of fewer than 64 tiles of 64^2 (the V-fold weight gradients dWo += G V^T, 256 x 256 x 72,
  // and dV = Wo^T G, 256 x 72 x 256, once per layer and step): 32 x 32 tiles, 4x the workgroups
  const long tiles64 = (long)((a.M + 63) / 64) * ((a.N + 63) / 64) * a.batch;
  if (k.f32_small && tiles64 < 64) return 32;
  return 64;
}

// ------------------------------------------------------------------------------------------ split plans
// split-K decision for a BM x BN tiling: K is split over workgroups when the output tile count cannot
// fill the 256 CUs, only on a plain fp32-output problem
inline void gemm_plan_splits(GemmPlan& pl, const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes, int BM, int BN) {
  const int batch = a.batch;
  const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * batch;
  pl.splits = 1;
  pl.kchunk = a.K;
  if (!(gemm_plain(a) && tiles < 512 && a.K >= 1024)) return;
  int s = (k.split_target + tiles - 1) / tiles;
  int maxs = a.K / 512;
  if (s > maxs) s = maxs;
  // up to 256 splits: the memory K / V projection weight gradients (256 x 64 over 374k rows)
  // have 2-4 output tiles, which 64 splits left at half a wave of workgroups
  if (s > 256) s = 256;
  // deterministic (round 6): the splits' partial tiles in the workspace, added in split order by
  // gemm_split_reduce_kernel -- the float atomics' arrival order made e.g. the hypernetwork-mask
  // gradient (104 batched 1 x 32 x 65536 products, mask_decoder.py) differ between identical runs.
  // As many splits as the workspace holds; none when it holds fewer than two.
  const int64_t per = (int64_t)batch * a.M * a.N + (a.rowsum ? (int64_t)batch * a.M : 0);
  const int64_t cap = (k.dbg & 32) ? 0 : gemm_ws_usable(k, ws_bytes) / 4;  // dbg 32: the atomic form (A/B)
  if (cap > 0 && s > 1 && (int64_t)s * per > cap) s = (int)std::min<int64_t>(s, cap / per);
  if (s <= 1) return;
  pl.kchunk = ((a.K + s - 1) / s + 63) / 64 * 64;
  pl.splits = (a.K + pl.kchunk - 1) / pl.kchunk;
  if (cap > 0) {
    pl.use_ws = true;
    pl.ws_floats = (int64_t)pl.splits * per;
  } else {
    pl.atomic = true;
    pl.zero_c = a.beta == 0.f;
  }
}

// Tiny-M long-K GEMMs with a bf16 output (M <= 128, K >= 1024, <= 16 output tiles of 64 x 64; round 6):
// the two-way decoder's token MLP second layer, 104 x 256 x 2048 (transformer.py:219-245, frame-batched
// forward per frame), ran as 8 workgroups of 32 K steps each (21 us, profiles/r06_v3_shape_table.txt).
// The K range is split over S batch entries of ONE fp32 launch into the weight-gradient workspace
// (no epilogue), then ONE launch adds the S partials in fixed order and runs the GEMM epilogue (bias,
// activation, dropout, residual, pre-activation store: epilogue4) -- deterministic, the fp32 sum rounded
// once.  Opt-in (S2H_GEMM_TINY_SPLITK=1, s2h_gemm_tiny_splitk): 47.73 / 47.81 ms per bench step against
// 47.63 / 47.83 for the one-launch tiling (in-call A/B) -- no gain, so the one-launch tiling stays.
inline bool gemm_plan_tiny_splitk(GemmPlan& pl, const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes) {
  if (!k.tiny_splitk || a.batch != 1 || a.f32_out || a.M > 128 || a.K < 1024 || !a.a_kc || !a.b_kc || a.rowsum || a.rope)
    return false;
  const int tiles = ((a.M + 63) / 64) * ((a.N + 63) / 64);
  if (tiles > 16) return false;
  int S = 16;
  while (S > 1 && (a.K % (64 * S) != 0 || tiles * S > 256)) S /= 2;
  if (S < 4 || a.K / S >= 1024) return false;  // (a K chunk of >= 1024 would be split again, into the same workspace)
  const int64_t need = (int64_t)S * a.M * a.N;
  if (need * 4 > gemm_ws_usable(k, ws_bytes)) return false;  // the workspace is too small (or off)
  GemmProblem b = a;  // the first launch: S batch entries of K / S each, batch stride K / S
  b.batch = S;
  b.K = a.K / S;
  b.sa8 = b.sb8 = b.K % 8 == 0;
  if (!gemm_glds_ok(b)) return false;
  pl.kind = GEMM_TINY_SPLITK;
  pl.cfg = CFG_64_NS4;
  gemm_cfg_tile(pl.cfg, pl.tile);
  pl.splits = S;
  pl.kchunk = b.K;
  pl.use_ws = true;
  pl.ws_floats = need;
  pl.tag = gemm_tag(64, 64, 2, 2, 4, 64, true, true, false, false);
  return true;
}

// the deterministic weight-gradient kernel's tiles: 0 256x256, 1 256x128, 2 128x256, 3 128x128, 4 256x64,
// 5 64x256, on 8 waves; `rate` the per-CU rate (TF/s) of the cost model
struct GemmWgTile {
  int BM, BN, WGM, WGN, NS;
  double rate;
};
inline const GemmWgTile& gemm_wg_tile(int i) {
  static const GemmWgTile t[6] = {{256, 256, 2, 4, 2, 4.2}, {256, 128, 4, 2, 2, 3.4}, {128, 256, 2, 4, 2, 3.4},
                                  {128, 128, 2, 4, 3, 2.4}, {256, 64, 4, 2, 3, 2.0},  {64, 256, 1, 8, 3, 2.0}};
  return t[i];
}

// Weight gradients over a long reduction (gemm_wgrad.hip): batch 1, both operands row-contiguous over the
// reduction, plain fp32 output.  false: not its case, or the workspace fits not even one split (the
// generic split path then runs).
inline bool gemm_plan_wgrad(GemmPlan& pl, const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes) {
  if (gemm_ws_usable(k, ws_bytes) <= 0 || a.batch != 1) return false;
  const bool plain = gemm_plain(a) && !a.rope;
  // every reduction the split-K path would split (gemm_plan_splits: < 512 tiles of 128 x 64, K >= 1024), and
  // every reduction of >= kmin rows
  const long t128x64 = (long)((a.M + 127) / 128) * ((a.N + 63) / 64);
  // round 6: also the mid-length reductions (512 <= K < 1024) of few output tiles -- the two-way decoder's
  // frame-batched weight gradients (832 token rows: 256 x 256, 256 x 2048, ...), which ran as 16-64
  // unsplit 64 x 64 workgroups of 13 K steps (~23 us each, profiles/r06_v3_shape_table.txt)
  const bool mid = a.K >= 512 && a.K < 1024 && t128x64 <= 64;
  if (!plain || (a.K < 1024 && !mid) || (a.K < k.wg_kmin && t128x64 >= 512)) return false;
  if (a.a_kc || !a.a_rc || a.b_kc || !a.b_rc || a.M < 16 || a.N < 64) return false;
  // operand extents rounded up to 8 inside the row pitch (the DMA moves 8-element pieces; the extra
  // rows / columns are read, never stored)
  const int Md = (a.M + 7) / 8 * 8, Nd = (a.N + 7) / 8 * 8;
  if (Md > a.lda || Nd > a.ldb || a.lda % 8 || a.ldb % 8 || !a.a16 || !a.b16) return false;
  if ((int64_t)a.K * a.lda >= (1ll << 31) - 8 || (int64_t)a.K * a.ldb >= (1ll << 31)) return false;
  // tile and split count from a cost model (one workgroup per CU): rounds of workgroups x (the
  // K chunk's MFMA work at the tile's measured rate + a fixed prologue / epilogue) + the partial tiles
  // written and read back once each.  Per-CU rates (TF/s) fitted to tools/wgrad_sweep.py
  // (profiles/r05_v2_wgrad_sweep.log: the model's pick within ~10 % of the best forced tile x split).
  int best = -1, best_s = 1;
  double best_t = 1e30;
  for (int c = 0; c < 6; ++c) {
    const int bm = gemm_wg_tile(c).BM, bn = gemm_wg_tile(c).BN;
    const long tiles = (long)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
    const int smax = std::max(1, std::min(256, a.K / (mid ? 128 : 512)));
    for (int sp = 1; sp <= smax; ++sp) {
      const long kchunk = ((a.K + sp - 1) / sp + 63) / 64 * 64;
      const long wgs = tiles * sp;
      const long rounds = (wgs + 255) / 256;
      const double t = rounds * (2.0 * bm * bn * kchunk / (gemm_wg_tile(c).rate * 1e6) + 2.5) +
                       (sp > 1 ? 2.0 * wgs * bm * bn * 4 / 4.5e6 : 0.0);  // us
      if (t < best_t) { best_t = t; best = c; best_s = sp; }
    }
  }
  if (k.wg_force_tile >= 0 && k.wg_force_tile < 6) best = k.wg_force_tile;
  if (k.wg_force_splits > 0) best_s = k.wg_force_splits;
  const GemmWgTile& t = gemm_wg_tile(best);
  const int ntm = (a.M + t.BM - 1) / t.BM, ntn = (a.N + t.BN - 1) / t.BN;
  const int tiles = ntm * ntn;
  int s = best_s < 1 ? 1 : best_s;
  // as many splits as the workspace holds
  const int64_t tile_bytes = (int64_t)t.BM * t.BN * 4;
  const int64_t rs_bytes = a.rowsum ? (int64_t)ntm * t.BM * 4 : 0;
  const int64_t fit = ws_bytes / ((int64_t)tiles * tile_bytes + rs_bytes);
  if (fit < 1) return false;
  if (s > fit) s = (int)fit;
  pl.kind = GEMM_WGRAD_DET;
  pl.cfg = 0;
  pl.tile = {t.BM, t.BN, t.WGM, t.WGN, t.NS, 64};
  pl.kchunk = ((a.K + s - 1) / s + 63) / 64 * 64;
  pl.splits = (a.K + pl.kchunk - 1) / pl.kchunk;
  pl.use_ws = true;
  pl.ws_floats = (int64_t)pl.splits * ((int64_t)tiles * t.BM * t.BN + (a.rowsum ? (int64_t)ntm * t.BM : 0));
  pl.wg_tile = best;
  pl.Md = Md;
  pl.Nd = Nd;
  // reduction: SL slices per slot so that about 2^17 threads (eight 16-B loads in flight each) read
  // the partials
  const int64_t slots = (int64_t)tiles * (t.BM * t.BN / 4);
  pl.sl = 1;
  while (pl.sl < 16 && slots * pl.sl < 131072 && pl.sl * 2 <= pl.splits) pl.sl *= 2;
  pl.tag = gemm_tag(t.BM, t.BN, t.WGM, t.WGN, t.NS, 64, false, false, false, false) | ((int64_t)1 << 41);
  return true;
}

// ------------------------------------------------------------------------------------------- the plans
// LDS-DMA tiling `cfg` (a number gemm_cfg_tile knows, not an A-in-registers one) with its split plan; the
// caller has checked gemm_glds_ok
inline GemmPlan gemm_plan_glds(const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes, int cfg) {
  GemmPlan pl;
  pl.kind = GEMM_GLDS;
  pl.cfg = cfg;
  gemm_cfg_tile(cfg, pl.tile);
  const GemmTile& t = pl.tile;
  gemm_plan_splits(pl, a, k, ws_bytes, t.BM, t.BN);
  pl.tag = gemm_tag(t.BM, t.BN, t.WGM, t.WGN, t.NS, t.BK, a.a_kc, a.b_kc, false, false);
  return pl;
}

// tiling number `cfg` on this problem, with the fallbacks of step 5
inline GemmPlan gemm_plan_tiled(const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes, int cfg) {
  GemmPlan pl;
  if (cfg < 0 || cfg == CFG_REGS || !gemm_glds_ok(a)) {  // register-staged (unaligned operands)
    const int bm = gemm_regs_tile(a);
    pl.kind = GEMM_REGS;
    pl.cfg = CFG_REGS;
    pl.tile = {bm, bm, 2, 2, 1, 64};
    gemm_plan_splits(pl, a, k, ws_bytes, bm, bm);
    pl.tag = gemm_tag(bm, bm, 2, 2, 1, 64, a.a_kc, a.b_kc, true, false);
    return pl;
  }
  if ((cfg == CFG_64_AREG || cfg == CFG_64x128_AREG) && gemm_areg_ok(a, 256)) {
    // (K <= 256: never in the split regime)
    pl.kind = GEMM_AREG;
    pl.cfg = cfg;
    gemm_cfg_tile(cfg, pl.tile);
    pl.kchunk = a.K;
    pl.tag = gemm_tag(64, pl.tile.BN, 4, 1, 1, 64, true, a.b_kc, false, false, true);
    return pl;
  }
  GemmTile t;
  // a forced A-in-registers tiling the shape cannot take, or no tiling's number: CFG_128
  if (cfg == CFG_64_AREG || cfg == CFG_64x128_AREG || !gemm_cfg_tile(cfg, t)) cfg = CFG_128;
  return gemm_plan_glds(a, k, ws_bytes, cfg);
}

inline GemmPlan gemm_plan(const GemmProblem& a, const GemmKnobs& k, int64_t ws_bytes) {
  GemmPlan pl;
  if (a.f32_in) {
    const int t = gemm_f32_tile(a, k);
    pl.kind = GEMM_F32;
    pl.tile = {t, t, 2, 2, 1, 32};
    pl.kchunk = a.K;
    return pl;
  }
  if (!k.cfg && a.K == 1 && a.beta == 0.f && !a.bias && !a.R && !a.X && !a.cscale && !a.dropout && a.act == 0 &&
      !a.rowsum && !a.rope) {
    pl.kind = GEMM_OUTER;
    pl.kchunk = a.K;
    return pl;
  }
  if (!k.cfg && !k.tiny_cfg && gemm_plan_tiny_splitk(pl, a, k, ws_bytes)) return pl;
  // long / mid-reduction weight gradients
  if (!k.cfg && a.f32_out && a.K >= 512 && gemm_plan_wgrad(pl, a, k, ws_bytes)) return pl;
  int cfg = k.cfg ? k.cfg : gemm_pick_cfg(a);
  if (!k.cfg) {
    if (k.tiny_cfg && a.M <= 128) cfg = k.tiny_cfg;
    if (k.w41 && !a.f32_out && (k.w41 == 1 || a.N >= 768)) cfg = gemm_w41_of(cfg);
    if (k.areg && a.K < 256 && a.K % 64 != 0 && !a.f32_out && a.M > 128 && gemm_areg_ok(a, 256)) cfg = CFG_64_AREG;
    const int cls = gemm_class(a);  // A/B override per GEMM class (s2h_gemm_class_config)
    if (cls >= 0 && k.class_cfg[cls]) cfg = k.class_cfg[cls];
  }
  return gemm_plan_tiled(a, k, ws_bytes, cfg);
}

#endif  // S2H_GEMM_PLAN_H
