// The bilinear resampling rule (align_corners=False, PyTorch upsample_bilinear2d) of s2h_bilinear_fwd
// (elementwise.hip: bil_src and the four-tap expression of bilinear_fwd_kernel), restated for the fused mask
// export (rle.hip), whose thresholded values must equal s2h_bilinear_fwd's bit for bit.
//
// The roundings are spelled out here.  In elementwise.hip the expression
//   (1 - ly) * ((1 - lx) * x00 + lx * x01) + ly * ((1 - lx) * x10 + lx * x11)
// is left to the compiler's contraction, and bilinear_fwd_kernel is compiled to: (1 - lx) * x00 rounded,
// lx * x01 fused into the add (likewise the second row), ly * row1 rounded, (1 - ly) * row0 fused; and
// scale * (o + 0.5) - 0.5 as one fused multiply-add.  The same source inlined into the export kernel was
// contracted the other way round (lx * x01 rounded), so this copy turns contraction off and writes exactly
// those fused multiply-adds.  tests/test_rle_export_gpu.py compares the two kernels exactly; if a compiler
// change ever moves elementwise.hip's contraction, that test says so, and this file follows.
#pragma once
#include <hip/hip_runtime.h>

// source taps i0 <= i1 and the weight l1 of i1 for output index o of a resampling in -> out, scale = in / out
__device__ __forceinline__ void bil_src(int o, float scale, int in, int& i0, int& i1, float& l1) {
  float s = __builtin_fmaf(scale, o + 0.5f, -0.5f);
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// the four-tap value of plane xp (row stride wi)
__device__ __forceinline__ float bil_tap(const float* xp, int wi, int y0, int y1, int x0, int x1, float ly, float lx) {
#pragma clang fp contract(off)
  const float mx = 1.f - lx, my = 1.f - ly;
  const float r0 = __builtin_fmaf(lx, xp[y0 * wi + x1], mx * xp[y0 * wi + x0]);
  const float r1 = __builtin_fmaf(lx, xp[y1 * wi + x1], mx * xp[y1 * wi + x0]);
  return __builtin_fmaf(my, r0, ly * r1);
}
