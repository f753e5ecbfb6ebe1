// Training visualisation on the device (reference utils/viz.py create_composite_visualization, drawn there with
// cv2 + matplotlib on host copies of the logits, frames and masks): the picture is viz_pixel.h, shared with
// viz_host_check.cpp; only finished uint8 composites leave the device.
//
// s2h_viz_pack: one lane per pixel thresholds the C category planes of its pixel into one uint64 word (bit c =
//   category c).  Lanes of a wave read 64 consecutive values of each plane: coalesced, every value read once.
// s2h_viz_compose: the n composites are one flat byte array of n 2H 2W 3 bytes; a pixel is 3 bytes, so a lane
//   takes four consecutive pixels of the flat array (n 4 H W is a multiple of 4) and stores them as three whole
//   dwords, 12-byte aligned -- a wave writes 768 contiguous bytes.  The four pixels may wrap over a row end
//   (odd W): each finds its own (frame, row, column).  The 3 x 3 neighbourhood of an overlay pixel is read
//   straight from the words through the caches, not from an LDS tile with a halo: a word is 8 bytes, the nine
//   reads of a lane fall on three rows its neighbours in the wave read as well (each word is fetched from L2 once
//   per row of lanes and served from L1 / TA for the other eight uses), the kernel's floor is the HBM traffic of
//   frames + words + output either way, and a tile would add a barrier, a halo of 2 (T + 1) / T^2 extra loads and
//   edge cases at panel borders for a launch that runs on one step in twenty.
// Both launches are stream-ordered, write every output byte exactly once, use no atomics and no host round trip;
// the launch count is two whatever the data holds.
#include "common.h"
#include "viz_pixel.h"

namespace {

constexpr int VZ_BLOCK = 256;

__global__ __launch_bounds__(VZ_BLOCK) void viz_pack_kernel(int C, int64_t hw, int64_t total, int kind,
                                                            const uint8_t* src, int64_t stride_bytes, uint64_t* words) {
  const int64_t i = (int64_t)blockIdx.x * VZ_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int64_t f = i / hw, p = i - f * hw;
  words[i] = vz_pack(kind, src + f * stride_bytes, C, hw, p);
}

__global__ __launch_bounds__(VZ_BLOCK) void viz_compose_kernel(VizArgs a, int64_t quads, uint32_t* out) {
  const int64_t q = (int64_t)blockIdx.x * VZ_BLOCK + threadIdx.x;
  if (q >= quads) return;
  const int W2 = 2 * a.W;
  const int64_t per = (int64_t)4 * a.H * a.W;  // pixels of one composite
  uint32_t px[4], d[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = 4 * q + k;
    const int f = (int)(i / per);
    const int64_t r = i - (int64_t)f * per;
    const int Y = (int)(r / W2);
    px[k] = vz_composite_pixel(a, f, Y, (int)(r - (int64_t)Y * W2));
  }
  vz_pack4(px, d);
  out[3 * q] = d[0];
  out[3 * q + 1] = d[1];
  out[3 * q + 2] = d[2];
}

}  // namespace

extern "C" int s2h_viz_pack(int n, int C, int H, int W, int kind, const void* src, int64_t frame_stride,
                            uint64_t* words, hipStream_t st) {
  if (vz_out_bytes(n, C, H, W) < 0 || (kind != VZ_MASK_U8 && kind != VZ_MASK_F32) || frame_stride < 0)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!src || !words) return (int)hipErrorInvalidValue;
  const int64_t hw = (int64_t)H * W, total = hw * n;  // (< 2^31 / 12)
  hipLaunchKernelGGL(viz_pack_kernel, dim3((unsigned)((total + VZ_BLOCK - 1) / VZ_BLOCK)), dim3(VZ_BLOCK), 0, st, C, hw,
                     total, kind, (const uint8_t*)src, frame_stride * (kind == VZ_MASK_F32 ? 4 : 1), words);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_viz_compose(int n, int C, int H, int W, int img_kind, const void* frames, int64_t frame_stride,
                               const void* frame0, const uint64_t* gt_words, const uint64_t* pred_words,
                               const uint64_t* prompt_words, const uint8_t* palette, int M, const int* markers,
                               uint8_t* out, hipStream_t st) {
  if (vz_out_bytes(n, C, H, W) < 0 || (img_kind != VZ_IMG_F32_CHW && img_kind != VZ_IMG_U8_HWC) || frame_stride < 0 ||
      M < 0 || M > VZ_MAX_MARKERS)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!frames || !frame0 || !gt_words || !pred_words || !palette || !out || (M > 0 && !markers) ||
      ((uintptr_t)out & 3))
    return (int)hipErrorInvalidValue;
  VizArgs a;
  a.n = n, a.H = H, a.W = W, a.img_kind = img_kind, a.frames = frames, a.frame_stride = frame_stride;
  a.frame0 = frame0, a.gt = gt_words, a.pred = pred_words, a.prompt = prompt_words, a.palette = palette;
  a.M = prompt_words ? 0 : M, a.markers = markers;
  const int64_t quads = (int64_t)n * H * W;  // n 2H 2W / 4
  hipLaunchKernelGGL(viz_compose_kernel, dim3((unsigned)((quads + VZ_BLOCK - 1) / VZ_BLOCK)), dim3(VZ_BLOCK), 0, st, a,
                     quads, reinterpret_cast<uint32_t*>(out));
  S2H_LAUNCH_CHECK();
}
