// The optimizer step's arithmetic in one place (s2h_grad_norm / s2h_adamw, optim.hip): the clip pair from the
// summed squares, the scalars of one AdamW step and one element's update.  Plain functions that compile for the
// device and for the host: optim_host_check.cpp runs them element by element, and tests/optim_cases.py mirrors
// them operation for operation in numpy.  Every fp32 rounding is written out: a product that feeds an addition
// goes through oe_mul_rn (never contracted into an fma), every fused multiply-add is an explicit fmaf, division
// and sqrtf are the IEEE operations (no fast-math flag, fp32 denormals on).  The update is therefore fixed by
// this source, not by a compiler's contraction choice; host builds add -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OE_HD __host__ __device__ __forceinline__
#else
#define OE_HD inline
#endif

// a * b rounded once to fp32, also where the result feeds an addition or subtraction
// (device: hipcc contracts across __fmul_rn and across `#pragma clang fp contract(off)` once the function is
// inlined -- its -ffp-contract=fast fuses in the backend -- so the rounded product passes through an empty asm
// statement, which costs no instruction and hides the multiplication from the fusion)
OE_HD float oe_mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r = __fmul_rn(a, b);
  asm("" : "+v"(r));
  return r;
#else
  return a * b;
#endif
}

// out[0] = sqrt(sumsq) * grad_scale, the norm of the scaled gradient; out[1] = grad_scale * the clip coefficient
// min(1, max_norm / (norm + 1e-6)) of clip_grad_norm_ (1 if max_norm <= 0): the factor AdamW applies to the
// stored gradient.  A NaN norm gives a NaN factor (the comparison is false), an infinite one the factor 0.
OE_HD void oe_clip_pair(float sumsq, float max_norm, float grad_scale, float* out) {
  const float norm = oe_mul_rn(sqrtf(sumsq), grad_scale);
  out[0] = norm;
  float c = 1.f;
  if (max_norm > 0.f) {
    c = max_norm / (norm + 1e-6f);
    if (c > 1.f) c = 1.f;
  }
  out[1] = oe_mul_rn(c, grad_scale);
}

// The scalars of one step.  decay = 1 - lr * wd with the product exact (one rounding); torch forms
// float32(1 - lr * wd) from a double lr, so with the ABI's float lr the two differ by at most one fp32 neighbour.
OE_HD float oe_decay(float lr, float wd) { return fmaf(-lr, wd, 1.f); }
OE_HD float oe_w1(float beta1) { return 1.f - beta1; }
OE_HD float oe_omb2(float beta2) { return 1.f - beta2; }
// host side: the bias corrections in double, rounded once
inline float oe_step_size(float lr, float beta1, int step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  return (float)((double)lr / bc1);
}
inline float oe_bc2_sqrt(float beta2, int step) {
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return (float)sqrt(bc2);
}

// One element's AdamW update (torch.optim.AdamW, decoupled weight decay): gi = g * cf is rounded before it is
// used, as clip_grad_norm_ rounds it when it writes the clipped gradient back; m.lerp_(gi, w1);
// v = beta2 * v + omb2 * gi^2; p = p * decay - step_size * m / (sqrt(v) / bc2_sqrt + eps).
OE_HD void adamw_elem(float g, float& p, float& m, float& v, float cf, float decay, float w1, float beta2, float omb2,
                      float eps, float step_size, float bc2_sqrt) {
  const float gi = oe_mul_rn(g, cf);
  const float mi = fmaf(w1, gi - m, m);
  const float vi = fmaf(omb2, oe_mul_rn(gi, gi), oe_mul_rn(v, beta2));
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = fmaf(-step_size, mi / denom, oe_mul_rn(p, decay));
  m = mi;
  v = vi;
}
