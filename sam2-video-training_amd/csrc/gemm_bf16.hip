// bf16 GEMM launch side: gemm_plan.h decides (kernel, tiling, splits, storage), this file and gemm_cfg*.hip
// launch what the plan says (kernels in gemm_bf16.h, instantiated in gemm_cfg*.hip).
#include <utility>

#include "gemm_bf16.h"

// the library's one GemmKnobs instance; the setters below (and s2h_gemm_f32_small in gemm.hip, s2h_wgrad_force /
// s2h_wgrad_workspace in gemm_wgrad.hip) write it, gemm_plan reads it.  The s2h_gemm_* setters return the
// previous value.
GemmKnobs g_gemm_knobs;

extern "C" int s2h_gemm_config(int cfg) {  // cfg | dbg << 8 (cfg < 0: the register-staged kernel, dbg 0)
  const int prev = g_gemm_knobs.cfg | (g_gemm_knobs.dbg << 8);
  g_gemm_knobs.cfg = cfg < 0 ? cfg : (cfg & 0xff);
  g_gemm_knobs.dbg = cfg < 0 ? 0 : (cfg >> 8);
  return prev;
}
extern "C" int s2h_gemm_tiny_config(int cfg) { return std::exchange(g_gemm_knobs.tiny_cfg, cfg); }
extern "C" int s2h_gemm_split_target(int t) {
  return std::exchange(g_gemm_knobs.split_target, t > 0 ? t : g_gemm_knobs.split_target);
}
extern "C" int s2h_gemm_w41(int mode) { return std::exchange(g_gemm_knobs.w41, mode); }
extern "C" int s2h_gemm_areg(int mode) { return std::exchange(g_gemm_knobs.areg, mode); }
extern "C" int s2h_gemm_class_config(int cls, int cfg) {
  return cls < 0 || cls > 5 ? -1 : std::exchange(g_gemm_knobs.class_cfg[cls], cfg);
}
extern "C" int s2h_gemm_tiny_splitk(int mode) {
  return std::exchange(g_gemm_knobs.tiny_splitk, mode >= 0 ? mode : g_gemm_knobs.tiny_splitk);
}

// the second launch of a tiny split-K plan (gemm_plan.h gemm_plan_tiny_splitk): the S partials added in fixed
// order, then the GEMM epilogue
__global__ __launch_bounds__(256) void gemm_splitk_epi_kernel(GemmArgs16 p, const float* part, int S) {
  if (p.drop_p > 0.f) p.seed = s2h_seed(p.seed, p.seed_off);  // the device RNG offset, as every dropout site
  const int nq = (p.N + 3) / 4;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)p.M * nq) return;
  const int row = (int)(q / nq), col0 = (int)(q % nq) * 4;
  const int64_t MN = (int64_t)p.M * p.N;
  const float* pp = part + (int64_t)row * p.N + col0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (col0 + 4 <= p.N && (p.N & 3) == 0) {
    for (int sp = 0; sp < S; ++sp) {
      const float4 t = *(const float4*)(pp + sp * MN);
      v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
    }
  } else {
    for (int sp = 0; sp < S; ++sp)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col0 + e < p.N) v[e] += pp[sp * MN + e];
  }
  float bcol[4];
  load_bcol(p, col0, bcol);
  epilogue4(p, 0, row, col0, float4{v[0], v[1], v[2], v[3]}, bcol);
}

static int gemm_tiny_splitk(const GemmPlan& pl, const GemmArgs16& a, hipStream_t st) {
  const int S = pl.splits;
  float* ws = s2h_det_ws(pl.ws_floats * 4);
  GemmArgs16 b = {};
  b.M = a.M; b.N = a.N; b.K = a.K / S;
  b.A = a.A; b.lda_m = a.lda_m; b.lda_k = 1; b.sA = a.K / S;
  b.B = a.B; b.ldb_k = 1; b.ldb_n = a.ldb_n; b.sB = a.K / S;
  b.C = ws; b.ldc = a.N; b.sC = (int64_t)a.M * a.N;
  b.alpha = 1.f; b.beta = 0.f; b.out_f32 = 1;
  b.vecA = a.vecA; b.vecB = a.vecB;
  b.dbg = a.dbg;
  GemmPlan first = pl;  // S batch entries of one unsplit K chunk each
  first.splits = 1;
  first.use_ws = false;
  int rc = gemm_cfg_launch_1(first, b, S, st);
  if (rc != 0) return rc;
  GemmArgs16 e = a;
  e.splits = 1;
  e.kchunk = a.K;
  gemm_plan_vec(e, 1);
  const int64_t nq = (int64_t)a.M * ((a.N + 3) / 4);
  hipLaunchKernelGGL(gemm_splitk_epi_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, e, ws, S);
  return (int)hipGetLastError();
}

// The fixed-order sum of a split launch's partial tiles (gemm16.h, gemm_plan.h gemm_plan_splits): one thread per output
// element (then per rowsum element), eight independent chains over the splits (split q on chain q % 8,
// eight loads in flight) combined in a fixed tree -- the same sum for any timing of the split launch.
__global__ __launch_bounds__(256) void gemm_split_reduce_kernel(const float* part, int S, int64_t sX, int batch, int M,
                                                                int N, float* C, int64_t ldc, int64_t sC, int beta1,
                                                                float* rowsum) {
  const int64_t nc = (int64_t)batch * M * N, nr = rowsum ? (int64_t)batch * M : 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc + nr) return;
  const float* pp = i < nc ? part + i : part + S * sX + (i - nc);
  const int64_t stride = i < nc ? sX : nr;
  float ch[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int s = 0;
  for (; s + 8 <= S; s += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) ch[j] += pp[(s + j) * stride];
#pragma unroll
  for (int j = 0; j < 7; ++j)
    if (s + j < S) ch[j] += pp[(s + j) * stride];
  const float v = ((ch[0] + ch[1]) + (ch[2] + ch[3])) + ((ch[4] + ch[5]) + (ch[6] + ch[7]));
  if (i < nc) {
    const int64_t b = i / ((int64_t)M * N), r = (i / N) % M, c = i % N;
    float* o = C + b * sC + r * ldc + c;
    *o = beta1 ? *o + v : v;
  } else {
    rowsum[i - nc] += v;
  }
}

int s2h_gemm_split_reduce(const GemmArgs16& a, int batch, hipStream_t st) {
  const int64_t n = (int64_t)batch * a.M * a.N + (a.rowsum ? (int64_t)batch * a.M : 0);
  hipLaunchKernelGGL(gemm_split_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)a.X,
                     a.splits, a.sX, batch, a.M, a.N, (float*)a.C, a.ldc, a.sC, a.beta == 1.f ? 1 : 0, a.rowsum);
  return (int)hipGetLastError();
}

// K = 1 (an outer product, e.g. the hypernetwork-mask gradient dup[o] = g[o]^T h[o] over 104 frames x
// objects of 16384 x 32, frametape._hyper_bw): C = alpha * a b^T element-wise, 8 output columns per lane
// with one 16-B store.  The bf16 x bf16 product is exact in fp32 and rounded once, as the MFMA tile's
// single accumulation is -- the same bits as the tiled GEMM, which spent 134 us per launch on K-step
// prologue / tail zeroing for 109 MB of output.
__global__ __launch_bounds__(256) void gemm_outer_kernel(GemmArgs16 p, int batch) {
  const int ng = (p.N + 7) / 8;
  const int64_t total = (int64_t)batch * p.M * ng;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int gcol = (int)(i % ng);
    const int64_t r = i / ng;
    const int m = (int)(r % p.M), bz = (int)(r / p.M);
    const float av = p.alpha * (float)p.A[(int64_t)bz * p.sA + (int64_t)m * p.lda_m];
    const bf16* B = p.B + (int64_t)bz * p.sB;
    const int n0 = gcol * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = n0 + e < p.N ? av * (float)B[(int64_t)(n0 + e) * p.ldb_n] : 0.f;
    if (p.out_f32) {
      float* C = (float*)p.C + (int64_t)bz * p.sC + (int64_t)m * p.ldc + n0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (n0 + e < p.N) C[e] = v[e];
    } else {
      bf16* C = (bf16*)p.C + (int64_t)bz * p.sC + (int64_t)m * p.ldc + n0;
      bf16 t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = (bf16)v[e];
      if (n0 + 8 <= p.N && (((uintptr_t)C) & 15) == 0) {
        *(uint4*)C = *(const uint4*)t;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (n0 + e < p.N) C[e] = t[e];
      }
    }
  }
}
static int gemm_outer(const GemmArgs16& a, int batch, hipStream_t st) {
  const int64_t total = (int64_t)batch * a.M * ((a.N + 7) / 8);
  if (total <= 0) return 0;
  const int64_t blocks = std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(gemm_outer_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, batch);
  return (int)hipGetLastError();
}

int s2h_gemm_bf16(const GemmArgs16& in, int batch, hipStream_t st) {
  GemmArgs16 a = in;
  a.dbg = g_gemm_knobs.dbg;
  const GemmPlan pl = gemm_plan(gemm_problem(a, batch), g_gemm_knobs, s2h_ws_registered_bytes());
  switch (pl.kind) {
    case GEMM_OUTER: return gemm_outer(a, batch, st);
    case GEMM_TINY_SPLITK: return gemm_tiny_splitk(pl, a, st);
    case GEMM_WGRAD_DET: return s2h_gemm_wgrad_det(pl, a, st);
    case GEMM_REGS: return gemm_cfg_launch_regs(pl, a, batch, st);
    case GEMM_AREG: return gemm_cfg_launch_7(pl, a, batch, st);
    case GEMM_GLDS: break;
    default: return (int)hipErrorInvalidValue;
  }
  switch (pl.cfg) {  // the translation unit that instantiates the tiling
    case CFG_64: case CFG_64_NS3: case CFG_64_K32_NS4: case CFG_64x128: case CFG_64_NS4: case CFG_64_K32_NS8:
      return gemm_cfg_launch_1(pl, a, batch, st);
    case CFG_128x64: case CFG_128x64_K32_NS3: case CFG_128x64_K32_NS4: case CFG_128x64_NS3:
      return gemm_cfg_launch_2(pl, a, batch, st);
    case CFG_128: case CFG_128_NS3: case CFG_128_K32_NS3: case CFG_128x256:
      return gemm_cfg_launch_3(pl, a, batch, st);
    case CFG_256: case CFG_256x128: case CFG_256x128_W4_K32_NS3: case CFG_256x128_W4_K64: case CFG_256x64_W4_K32_NS3:
      return gemm_cfg_launch_4(pl, a, batch, st);
    case CFG_64_W41: case CFG_128x64_W41: case CFG_128x64_W41_K32_NS3: case CFG_64_W41_NS4: case CFG_128x64_W41_NS3:
      return gemm_cfg_launch_5(pl, a, batch, st);
    case CFG_64x256_W41_NS4: case CFG_64x128_W41_NS4: case CFG_64x256_W41_NS3: case CFG_64x256_W41_K32_NS4:
      return gemm_cfg_launch_6(pl, a, batch, st);
    default: return (int)hipErrorInvalidValue;
  }
}
