// GEMM tilings, translation unit 1 (see gemm_bf16.h)
#include "gemm_bf16.h"

int gemm_cfg_launch_1(const GemmPlan& pl, GemmArgs16& a, int batch, hipStream_t st) {
  switch (pl.cfg) {
    case CFG_64: return launch_glds<64, 64, 2, 2, 2>(pl, a, batch, st);
    case CFG_64_NS3: return launch_glds<64, 64, 2, 2, 3>(pl, a, batch, st);
    case CFG_64_K32_NS4: return launch_glds<64, 64, 2, 2, 4, 32>(pl, a, batch, st);
    case CFG_64x128: return launch_glds<64, 128, 2, 2, 2>(pl, a, batch, st);
    case CFG_64_NS4: return launch_glds<64, 64, 2, 2, 4>(pl, a, batch, st);
    case CFG_64_K32_NS8: return launch_glds<64, 64, 2, 2, 8, 32>(pl, a, batch, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// register-staged kernel (unaligned operands): 128^2 or 64^2 tiles (gemm_plan.h gemm_regs_tile)
int gemm_cfg_launch_regs(const GemmPlan& pl, GemmArgs16& a, int batch, hipStream_t st) {
  if (pl.tile.BM == 128) return launch16_regs<128, 128>(pl, a, batch, st);
  return launch16_regs<64, 64>(pl, a, batch, st);
}
