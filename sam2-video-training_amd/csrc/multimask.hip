// The three-mask SAM heads of the video predictor (inference only; reference sam/mask_decoder.py:145-166,
// 227-234, 247-295 and sam2_base.py:380-428): every mask token's hypernetwork product in one pass over
// the upscaled embedding, the stability counts of the single-mask logits, and the per-object selection
// (best predicted IoU among tokens 1..K-1, or token 0 while it is stable) fused with the object-score
// gate, the cast to fp32 and the mask-token gather.  No float atomics: the counts are integers reduced
// in a fixed order, everything else is per-element.
#include "common.h"

namespace {

#define MM_GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

inline dim3 mm_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

inline bool mm_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// convt2_tail_kernel (elementwise.hip) with K hypernetwork rows per object: the same scatter + bias + add,
// GELU and roundings, the activation of a pixel computed once and K dot products taken from it, each
// summed in convt2_tail_kernel's order (a lane's 8 channels in sequence, then the pixel's CG lanes by
// xor 1, 2) -- so slice 0 equals s2h_convt2_tail's masks bit for bit.  pre / post are optional.
template <typename T, int CG, int K>
__global__ __launch_bounds__(256) void convt2_tail_k_kernel(int B, int H, int W, const T* Y, const float* bias,
                                                            const T* add, int add_bcast, const T* hyper, T* pre,
                                                            T* post, T* masks) {
  constexpr int V = 16 / sizeof(T);
  constexpr int Co = CG * V;
  const int64_t n = (int64_t)B * H * W * CG;
  MM_GRID_STRIDE(i, n) {  // (n is a multiple of CG: a pixel's CG lanes stay together)
    const int cg = (int)(i % CG);
    const int64_t p = i / CG;  // (b * H + y) * W + x
    const int x = (int)(p % W);
    const int64_t t = p / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    T e[4 * V];
    const uint4* yr = (const uint4*)(Y + p * 4 * Co + (int64_t)cg * V * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) *(uint4*)(e + u * V) = yr[u];
    float bv[V], hv[K][V];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      T hb[V];
      *(uint4*)hb = *(const uint4*)(hyper + ((int64_t)b * K + k) * Co + cg * V);
#pragma unroll
      for (int j = 0; j < V; ++j) hv[k][j] = to_f32(hb[j]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) bv[j] = bias ? bias[cg * V + j] : 0.f;
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      const int dy = sidx >> 1, dx = sidx & 1;
      const int64_t pix = ((int64_t)(2 * y + dy) * 2 * W + 2 * x + dx);  // within batch b
      const int64_t o = ((int64_t)b * 4 * H * W + pix) * Co + cg * V;
      float v[V];
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = to_f32(from_f32<T>(to_f32(e[4 * j + sidx]) + bv[j]));
      if (add) {
        T ad[V];
        *(uint4*)ad = *(const uint4*)(add + (add_bcast ? pix * Co + cg * V : o));
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] += to_f32(ad[j]);
      }
      T r[V], g[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        r[j] = from_f32<T>(v[j]);
        g[j] = from_f32<T>(gelu_erf(to_f32(r[j])) + 0.f);  // (+ 0: act_fwd's `* 1 + 0`, -0 -> +0)
      }
      if (pre) *(uint4*)(pre + o) = *(const uint4*)r;
      if (post) *(uint4*)(post + o) = *(const uint4*)g;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) dot += hv[k][j] * to_f32(g[j]);
#pragma unroll
        for (int m = 1; m < CG; m <<= 1) dot += __shfl_xor(dot, m, 64);
        if (cg == 0) masks[((int64_t)b * K + k) * 4 * H * W + pix] = from_f32<T>(dot);
      }
    }
  }
}

// counts[b] = (#{p: m[b][p] > delta}, #{p: m[b][p] > -delta}) on the stored value widened to fp32: one
// workgroup per object, per-thread integer counts, the wave by xor shuffles, the four waves summed in order
template <typename T>
__global__ __launch_bounds__(256) void stability_counts_kernel(int64_t P, const T* masks, int64_t ld, float delta,
                                                               int* counts) {
  __shared__ int sh[2][4];
  const int b = blockIdx.x;
  const T* m = masks + (int64_t)b * ld;
  int ci = 0, cu = 0;
  for (int64_t p = threadIdx.x; p < P; p += 256) {
    const float v = to_f32(m[p]);
    ci += v > delta ? 1 : 0;
    cu += v > -delta ? 1 : 0;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    ci += __shfl_xor(ci, s, 64);
    cu += __shfl_xor(cu, s, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = ci;
    sh[1][threadIdx.x >> 6] = cu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[2 * b] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    counts[2 * b + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

// One thread per (object, pixel); every thread of an object derives the same selection from the
// object's K IoU predictions (first maximum of 1..K-1, as torch.argmax) and, in the dynamic mode, its
// stability counts.  Pixel 0 writes the index and the IoU, pixels < C copy the mask token.
template <typename T>
__global__ __launch_bounds__(256) void multimask_select_kernel(int B, int K, int64_t P, int C, const T* masks,
                                                               const float* iou, const int* counts,
                                                               const float* score, const T* tok, int64_t ld_tok,
                                                               int mode, int tok_follow, float thresh, float fill,
                                                               int* idx, float* low, float* iou_out, T* tok_out,
                                                               float* multi_low) {
  const int64_t n = (int64_t)B * P;
  MM_GRID_STRIDE(i, n) {
    const int b = (int)(i / P);
    const int64_t p = i % P;
    const float* io = iou + (int64_t)b * K;
    int sel = 1;
    float bv = io[1];
    for (int k = 2; k < K; ++k) {
      if (io[k] > bv) {
        bv = io[k];
        sel = k;
      }
    }
    if (mode == 1) {
      const int ai = counts[2 * b], au = counts[2 * b + 1];
      const float s = au > 0 ? (float)ai / (float)au : 1.f;
      if (s >= thresh) sel = 0;
    }
    const bool on = score[b] > 0.f;
    const T* mb = masks + (int64_t)b * K * P;
    low[i] = on ? to_f32(mb[(int64_t)sel * P + p]) : fill;
    if (multi_low != nullptr) {
      for (int k = 1; k < K; ++k)
        multi_low[((int64_t)b * (K - 1) + (k - 1)) * P + p] = on ? to_f32(mb[(int64_t)k * P + p]) : fill;
    }
    if (p == 0) {
      idx[b] = sel;
      iou_out[b] = io[sel];
    }
    const int tk = (mode == 0 && tok_follow) ? sel : 0;
    for (int64_t c = p; c < C; c += P) tok_out[(int64_t)b * C + c] = tok[(int64_t)b * ld_tok + (int64_t)tk * C + c];
  }
}

}  // namespace

extern "C" int s2h_convt2_tail_k(int dt, int B, int H, int W, int Co, int K, const void* Y, const float* bias,
                                 const void* add, int add_bcast, const void* hyper, void* pre, void* post,
                                 void* masks, hipStream_t st) {
  if (dt != S2H_BF16 || Co != 32 || K != 4 || !Y || !hyper || !masks || !mm_al16(Y) || !mm_al16(hyper) ||
      (pre && !mm_al16(pre)) || (post && !mm_al16(post)) || (add && !mm_al16(add)))
    return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)B * H * W * 4;
  if (n <= 0) return 0;
  hipLaunchKernelGGL((convt2_tail_k_kernel<bf16, 4, 4>), mm_grid(n), dim3(256), 0, st, B, H, W, (const bf16*)Y, bias,
                     (const bf16*)add, add_bcast, (const bf16*)hyper, (bf16*)pre, (bf16*)post, (bf16*)masks);
  return (int)hipGetLastError();
}

extern "C" int s2h_stability_counts(int dt, int B, int64_t P, const void* masks, int64_t ld, float delta, int* counts,
                                    hipStream_t st) {
  if (B <= 0) return 0;
  if (P < 0 || P > 0x7fffffffLL || ld < P || !masks || !counts || (dt != S2H_BF16 && dt != S2H_F32))
    return (int)hipErrorInvalidValue;
  if (dt == S2H_BF16)
    hipLaunchKernelGGL(stability_counts_kernel<bf16>, dim3(B), dim3(256), 0, st, P, (const bf16*)masks, ld, delta,
                       counts);
  else
    hipLaunchKernelGGL(stability_counts_kernel<float>, dim3(B), dim3(256), 0, st, P, (const float*)masks, ld, delta,
                       counts);
  return (int)hipGetLastError();
}

extern "C" int s2h_multimask_select(int dt, int B, int K, int64_t P, int C, const void* masks, const float* iou,
                                    const int* counts, const float* score, const void* tok, int64_t ld_tok, int mode,
                                    int tok_follow, float thresh, float fill, int* idx, float* low, float* iou_out,
                                    void* tok_out, float* multi_low, hipStream_t st) {
  if (B <= 0) return 0;
  if (K < 2 || K > 8 || P <= 0 || C <= 0 || ld_tok < (int64_t)K * C || (mode != 0 && mode != 1) ||
      (mode == 1 && !counts) || !masks || !iou || !score || !tok || !idx || !low || !iou_out || !tok_out ||
      (dt != S2H_BF16 && dt != S2H_F32))
    return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)B * P;
  if (dt == S2H_BF16)
    hipLaunchKernelGGL(multimask_select_kernel<bf16>, mm_grid(n), dim3(256), 0, st, B, K, P, C, (const bf16*)masks, iou,
                       counts, score, (const bf16*)tok, ld_tok, mode, tok_follow, thresh, fill, idx, low, iou_out,
                       (bf16*)tok_out, multi_low);
  else
    hipLaunchKernelGGL(multimask_select_kernel<float>, mm_grid(n), dim3(256), 0, st, B, K, P, C, (const float*)masks,
                       iou, counts, score, (const float*)tok, ld_tok, mode, tok_follow, thresh, fill, idx, low,
                       iou_out, (float*)tok_out, multi_low);
  return (int)hipGetLastError();
}
