// Short-K tilings with A in registers (gemm_bf16.h gemm16a_kernel, CFG_64_AREG / CFG_64x128_AREG).
#include "gemm_bf16.h"

int gemm_cfg_launch_7(const GemmPlan& pl, GemmArgs16& a, int batch, hipStream_t st) {
  return pl.cfg == CFG_64_AREG ? launch_areg<64>(pl, a, batch, st) : launch_areg<128>(pl, a, batch, st);
}
