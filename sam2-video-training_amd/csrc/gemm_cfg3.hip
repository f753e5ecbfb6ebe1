// GEMM tilings, translation unit 3 (see gemm_bf16.h)
#include "gemm_bf16.h"

int gemm_cfg_launch_3(const GemmPlan& pl, GemmArgs16& a, int batch, hipStream_t st) {
  switch (pl.cfg) {
    case CFG_128: return launch_glds<128, 128, 2, 2, 2>(pl, a, batch, st);
    case CFG_128_NS3: return launch_glds<128, 128, 2, 2, 3>(pl, a, batch, st);
    case CFG_128_K32_NS3: return launch_glds<128, 128, 2, 2, 3, 32>(pl, a, batch, st);
    case CFG_128x256: return launch_glds<128, 256, 2, 4, 2>(pl, a, batch, st);
    default: return (int)hipErrorInvalidValue;
  }
}
