// 8-connected component labelling and hole filling of the video predictor's low-res mask logits (upstream
// sam2/utils/misc.py get_connected_components / fill_holes_in_mask_scores), entirely on the device: no
// flag is read back, the number of launches does not depend on the data.
//
// One thread per pixel, the N images laid end to end; a wave covers 64 consecutive pixels.
//   1. run labelling: two ballots give every foreground pixel the first pixel of its horizontal run inside
//      the wave's 64 pixels as parent (cc_run_start) -- the local labelling, in registers, no LDS;
//   2. merge: lane 0 joins its run to the one on its left, and every pixel owes at most two unions with the
//      row above (cc_merge_pixel); lock-free union-find with integer atomic min, roots = smallest index;
//   3. flatten + count: each pixel finds its root; the lanes of a wave that share a root add their number
//      to the root's counter with one integer atomic add;
//   4. broadcast: labels = root + 1 and the root's count, or the +-0.1 fill.
// Integer atomics only: the fixed point (root = smallest pixel index, count = component size) is unique,
// so the output is a pure function of the input.  Loop bounds: cc_uf.h.
#include "cc_uf.h"
#include "common.h"

namespace {

// L[i] = -1 off the foreground, else the in-image index of the first pixel of i's run within the wave;
// cnt[i] = 0
// (T = float: a score, cc_fg; T = uint8_t: a mask byte, foreground is != 0, or == 0 when not `positive`)
__device__ __forceinline__ bool cc_fg_of(float s, int positive) { return cc_fg(s, positive); }
__device__ __forceinline__ bool cc_fg_of(uint8_t s, int positive) { return (s != 0) == (positive != 0); }
template <typename T>
__global__ __launch_bounds__(256) void cc_init_kernel(int total, int HW, int W, const T* scores, int positive, int* L,
                                                      int* cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (the host checked total + 256 < 2^31)
  const int lane = threadIdx.x & 63;
  const bool in = i < total;
  const bool fg = in && cc_fg_of(scores[in ? i : 0], positive);
  const int q = in ? i % HW : 0;
  const int x = q % W;
  const uint64_t fgm = __ballot(fg);
  const bool link = fg && lane > 0 && x > 0 && ((fgm >> (lane - 1)) & 1ull);
  const uint64_t linkm = __ballot(link);
  if (!in) return;
  L[i] = fg ? q - (lane - cc_run_start(linkm, lane)) : -1;
  cnt[i] = 0;
}

__global__ __launch_bounds__(256) void cc_merge_kernel(int total, int H, int W, int* L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  if (L[i] < 0) return;  // (the sign of a slot never changes after cc_init_kernel)
  const int HW = H * W;
  const int q = i % HW;
  cc_merge_pixel(L + (i - q), H, W, q / W, q % W, (threadIdx.x & 63) == 0);
}

// L[i] = root of i; cnt[root] = size of the component.  Lanes of one wave with the same root (the usual
// case: a run) add once: the lowest pending lane is the leader, the lanes that match it retire together, so
// the loop runs once per distinct root in the wave, at most 64 times.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int total, int HW, int* L, int* cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < total;
  int g = -1;  // the root's index in the whole batch
  if (in && L[i] >= 0) {
    const int q = i % HW;
    int budget = HW;
    const int r = cc_find(L + (i - q), q, &budget);
    if (r != q) cc_min(L + i, r);  // (other threads may still walk through this slot: r is an ancestor)
    g = i - q + r;
  }
  bool todo = g >= 0;
  for (int it = 0; it < CC_WAVE; ++it) {
    const uint64_t pending = __ballot(todo);
    if (!pending) break;
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const int lg = __shfl(g, leader, CC_WAVE);
    const uint64_t same = __ballot(todo && g == lg);
    if ((threadIdx.x & 63) == leader) atomicAdd(cnt + lg, __popcll(same));
    if (g == lg) todo = false;
  }
}

__global__ __launch_bounds__(256) void cc_labels_kernel(int total, int HW, int* L, int* cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int r = L[i];
  if (r < 0) {
    L[i] = 0;  // (cnt[i] is 0 since cc_init_kernel)
    return;
  }
  const int q = i % HW;
  L[i] = r + 1;
  if (r != q) cnt[i] = cnt[i - q + r];  // only root slots are read, only other slots are written
}

// small = the pixel lies in a component of at most max_area pixels
__device__ __forceinline__ bool cc_small(int i, int HW, const int* L, const int* cnt, int max_area) {
  const int r = L[i];
  return r >= 0 && cnt[i - i % HW + r] <= max_area;
}
__global__ __launch_bounds__(256) void cc_fill_bg_kernel(int total, int HW, const float* scores, const int* L,
                                                         const int* cnt, int max_area, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  out[i] = cc_small(i, HW, L, cnt, max_area) ? 0.1f : scores[i];
}
__global__ __launch_bounds__(256) void cc_fill_fg_kernel(int total, int HW, const int* L, const int* cnt,
                                                         int max_area, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  if (cc_small(i, HW, L, cnt, max_area)) out[i] = -0.1f;
}

// N * H * W as int, or -1 when the sizes are outside what the kernels index
int cc_total(int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1 || (int64_t)H * W > CC_MAX_PIXELS) return -1;
  const int64_t t = (int64_t)N * H * W;
  return t + 256 > 0x7fffffffLL ? -1 : (int)t;
}

// steps 1-3: parents flattened to roots in L, component sizes in cnt at the roots
template <typename T>
void cc_roots(int total, int H, int W, const T* scores, int positive, int* L, int* cnt, hipStream_t st) {
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(cc_init_kernel<T>, grid, block, 0, st, total, H * W, W, scores, positive, L, cnt);
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, total, H, W, L);
  hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, st, total, H * W, L, cnt);
}

}  // namespace

extern "C" int s2h_cc_label(int N, int H, int W, const float* scores, int positive, int* labels, int* areas,
                            hipStream_t st) {
  const int total = cc_total(N, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!scores || !labels || !areas) return (int)hipErrorInvalidValue;
  cc_roots(total, H, W, scores, positive, labels, areas, st);
  hipLaunchKernelGGL(cc_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, H * W, labels,
                     areas);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_cc_label_u8(int N, int H, int W, const uint8_t* mask, int positive, int* labels, int* areas,
                               hipStream_t st) {
  const int total = cc_total(N, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!mask || !labels || !areas) return (int)hipErrorInvalidValue;
  cc_roots(total, H, W, mask, positive, labels, areas, st);
  hipLaunchKernelGGL(cc_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, H * W, labels,
                     areas);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_fill_holes(int N, int H, int W, const float* scores, int max_area, float* out, int* work,
                              hipStream_t st) {
  const int total = cc_total(N, H, W);
  if (total < 0 || max_area < 1) return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!scores || !out || !work || (const float*)out == scores) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  int* L = work;
  int* cnt = work + total;
  // holes: background components (<= 0) of the input
  cc_roots(total, H, W, scores, 0, L, cnt, st);
  hipLaunchKernelGGL(cc_fill_bg_kernel, grid, block, 0, st, total, H * W, scores, (const int*)L, (const int*)cnt,
                     max_area, out);
  // sprinkles: foreground components (> 0) of what the first pass left
  cc_roots(total, H, W, out, 1, L, cnt, st);
  hipLaunchKernelGGL(cc_fill_fg_kernel, grid, block, 0, st, total, H * W, (const int*)L, (const int*)cnt, max_area, out);
  S2H_LAUNCH_CHECK();
}
