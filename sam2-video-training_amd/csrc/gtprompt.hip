// Prompt generation from ground truth on the device (reference sam2_video/eval/inference.py:275-326 get_each_obj
// and eval/utils.py:95-153 mask_to_masks / mask_to_points): COCO RLE -> byte masks, rectangular dilation and
// erosion (the 10 x 10 closing), the kept components of a labelled image with their boxes and the sums the
// centre needs, and the pixel of a given rank inside or outside a component.  The labelling itself is cc.hip.
//
// One thread per pixel, the N images laid end to end, as in cc.hip; the per-pixel logic is gtprompt.h, which
// gtprompt_host_check.cpp runs on the host in the same decomposition.  Counting is ballot + popcount per wave
// of 64, block totals through LDS, prefix sums over the blocks in a second launch: no block waits for
// another one inside a launch.  Integer atomics only (min / max / add on int64): the result is a pure
// function of the input.  Every loop has a bound that does not depend on the data (gtprompt.h, and the
// comments below).
#include "gtprompt.h"
#include "common.h"

namespace {

// N * H * W as int, or -1 when the sizes are outside what the kernels index (as cc.hip's cc_total)
int gp_total(int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1 || (int64_t)H * W > GP_MAX_PIXELS) return -1;
  const int64_t t = (int64_t)N * H * W;
  return t + 256 > 0x7fffffffLL ? -1 : (int)t;
}

// exclusive prefix of v over the 256 threads of the block and the block's total; sh: 4 ints of LDS.
// The two barriers make sh reusable right after the call.
__device__ __forceinline__ int gp_block_scan(int v, int* total, int* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < GP_WAVE; o <<= 1) {
    const int t = __shfl_up(inc, o, GP_WAVE);
    if (lane >= o) inc += t;
  }
  if (lane == GP_WAVE - 1) sh[wave] = inc;
  __syncthreads();
  int woff = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < GP_BLOCK / GP_WAVE; ++w) {
    if (w < wave) woff += sh[w];
    tot += sh[w];
  }
  __syncthreads();
  *total = tot;
  return woff + inc - v;
}

// --------------------------------------------------------------------------------------------- RLE decode
__global__ __launch_bounds__(256) void gp_rle_decode_kernel(int total, int HW, int H, int W, const int* run_off,
                                                            const int* run_end, uint8_t* mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (the host checked total + 256 < 2^31)
  if (i >= total) return;
  const int a = i / HW, q = i % HW;
  const int y = q / W, x = q % W;
  const int o = run_off[a];
  const int n = run_off[a + 1] - o;
  mask[i] = (uint8_t)(gp_run_index(run_end + o, n < 0 ? 0 : n, x * H + y) & 1);
}

// --------------------------------------------------------------------------------------------- morphology
// one separable pass: along x (vertical 0) or along y (vertical 1)
__global__ __launch_bounds__(256) void gp_morph_pass_kernel(int total, int HW, int H, int W, const uint8_t* in, int op,
                                                            int lo, int hi, int vertical, uint8_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = i % HW;
  const int y = q / W, x = q % W;
  const uint8_t* img = in + (i - q);
  out[i] = vertical ? gp_morph_line(img + x, H, W, y, lo, hi, op) : gp_morph_line(img + y * W, W, 1, x, lo, hi, op);
}

// --------------------------------------------------------------------------------------------- components
// blk[image * nb + b] = kept roots among pixels [256 b, 256 b + 256) of the image
__global__ __launch_bounds__(256) void gp_comp_count_kernel(int HW, int nb, const int* labels, const int* areas,
                                                            int min_area, int* blk) {
  __shared__ int wc[GP_BLOCK / GP_WAVE];
  const int img = blockIdx.x / nb, b = blockIdx.x % nb;
  const int q = b * 256 + threadIdx.x;
  const bool in = q < HW;
  const int i = img * HW + (in ? q : 0);
  const bool kept = in && gp_kept_root(labels[i], areas[i], q, min_area);
  const uint64_t m = __ballot(kept);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = gp_popc(m);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// one block per image: blk -> its exclusive prefix within the image, hdr[2 image] = the image's count.
// ceil(nb / 256) <= 256 rounds (nb <= 2^24 / 256).
__global__ __launch_bounds__(256) void gp_comp_scan_kernel(int nb, int* blk, int* hdr) {
  __shared__ int sh[GP_BLOCK / GP_WAVE];
  int* row = blk + (int64_t)blockIdx.x * nb;
  int carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int c = c0 + threadIdx.x;
    const int v = c < nb ? row[c] : 0;
    int tot;
    const int ex = gp_block_scan(v, &tot, sh);
    if (c < nb) row[c] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) hdr[2 * blockIdx.x] = carry;
}

// one block: hdr[2 i + 1] = offset of image i, hdr[2 N] = total, hdr[2 N + 1] = 1 when an image has more
// than GP_MAX_INDEX kept components.  ceil(N / 256) rounds.
__global__ __launch_bounds__(256) void gp_comp_offsets_kernel(int N, int* hdr) {
  __shared__ int sh[GP_BLOCK / GP_WAVE];
  int carry = 0, over = 0;
  for (int c0 = 0; c0 < N; c0 += 256) {
    const int c = c0 + threadIdx.x;
    const int v = c < N ? hdr[2 * c] : 0;
    int tot;
    const int ex = gp_block_scan(v, &tot, sh);
    if (c < N) hdr[2 * c + 1] = carry + ex;
    carry += tot;
    over |= __syncthreads_or(v > GP_MAX_INDEX);
  }
  if (threadIdx.x == 0) {
    hdr[2 * N] = carry;
    hdr[2 * N + 1] = over ? 1 : 0;
  }
}

// rk[pixel] = the 1-based rank of the kept root at that pixel within its image, 0 elsewhere; the kept
// components' stats rows initialised (label, area, empty box, zero sums)
__global__ __launch_bounds__(256) void gp_comp_rank_kernel(int HW, int nb, int H, int W, const int* labels,
                                                           const int* areas, int min_area, const int* blk,
                                                           const int* hdr, int capacity, int* rk, int64_t* stats) {
  __shared__ int wc[GP_BLOCK / GP_WAVE];
  const int img = blockIdx.x / nb, b = blockIdx.x % nb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = b * 256 + threadIdx.x;
  const bool in = q < HW;
  const int i = img * HW + (in ? q : 0);
  const int label = labels[i], area = areas[i];
  const bool kept = in && gp_kept_root(label, area, q, min_area);
  const uint64_t m = __ballot(kept);
  if (lane == 0) wc[wave] = gp_popc(m);
  __syncthreads();
  if (!in) return;
  if (!kept) {
    rk[i] = 0;
    return;
  }
  int rank = blk[blockIdx.x] + gp_popc(gp_below(m, lane));
  for (int w = 0; w < GP_BLOCK / GP_WAVE; ++w)
    if (w < wave) rank += wc[w];
  rk[i] = rank + 1;
  const int64_t row = (int64_t)hdr[2 * img + 1] + rank;
  if (row >= capacity) return;
  int64_t* s = stats + row * GP_STATS;
  s[0] = label;
  s[1] = area;
  s[2] = W;
  s[3] = H;
  s[4] = -1;
  s[5] = -1;
  s[6] = 0;
  s[7] = 0;
  s[8] = 0;
}

__device__ __forceinline__ void gp_atomic_min(int64_t* p, int64_t v) {
  __hip_atomic_fetch_min((long long*)p, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gp_atomic_max(int64_t* p, int64_t v) {
  __hip_atomic_fetch_max((long long*)p, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gp_atomic_add(int64_t* p, int64_t v) {
  __hip_atomic_fetch_add((long long*)p, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// index image and the per-component box / selected-pixel sums.  The lanes of a wave that lie in the same
// component (the usual case: a run) reduce among themselves and their lowest lane issues the atomics, so
// the loop runs once per distinct component in the wave, at most 64 times (as cc_flatten_kernel).
__global__ __launch_bounds__(256) void gp_comp_stats_kernel(int total, int HW, int W, const int* labels, const int* rk,
                                                            const uint8_t* grid, const int* hdr, int capacity,
                                                            int64_t* stats, uint8_t* index) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int g = -1;  // the pixel's stats row
  int x = 0, y = 0;
  bool sel = false;
  if (i < total) {
    const int q = i % HW;
    const int l = labels[i];
    const int r = l > 0 && l <= HW ? rk[i - q + l - 1] : 0;
    index[i] = (uint8_t)(r > GP_MAX_INDEX ? GP_MAX_INDEX : r);
    if (r > 0) {
      const int64_t row = (int64_t)hdr[2 * (i / HW) + 1] + r - 1;
      if (row < capacity) g = (int)row;
      y = q / W;
      x = q % W;
      sel = !grid || grid[q] != 0;
    }
  }
  bool todo = g >= 0;
  for (int it = 0; it < GP_WAVE; ++it) {
    const uint64_t pending = __ballot(todo);
    if (!pending) break;
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const int lg = __shfl(g, leader, GP_WAVE);
    const bool mine = todo && g == lg;
    const uint64_t same = __ballot(mine);
    const int nsel = gp_popc(__ballot(mine && sel));
    // pixels of a wave are consecutive, so y is monotone over the lanes: the ends of `same` hold min and max
    const int ymin = __shfl(y, leader, GP_WAVE);
    const int ymax = __shfl(y, 63 - __clzll((long long)same), GP_WAVE);
    int xmin = mine ? x : 0x7fffffff, xmax = mine ? x : -1;
    int sx = mine && sel ? x : 0, sy = mine && sel ? y : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      xmin = min(xmin, __shfl_xor(xmin, o, GP_WAVE));
      xmax = max(xmax, __shfl_xor(xmax, o, GP_WAVE));
      sx += __shfl_xor(sx, o, GP_WAVE);
      sy += __shfl_xor(sy, o, GP_WAVE);
    }
    if (lane == leader) {
      int64_t* s = stats + (int64_t)lg * GP_STATS;
      gp_atomic_min(s + 2, xmin);
      gp_atomic_min(s + 3, ymin);
      gp_atomic_max(s + 4, xmax);
      gp_atomic_max(s + 5, ymax);
      if (nsel) {
        gp_atomic_add(s + 6, nsel);
        gp_atomic_add(s + 7, sx);
        gp_atomic_add(s + 8, sy);
      }
    }
    if (mine) todo = false;
  }
}

// --------------------------------------------------------------------------------------------- rank select
__device__ __forceinline__ bool gp_query_pixel(bool valid, int img, int HW, int p, const int* labels, int q_label,
                                               int neg, const uint8_t* grid) {
  return valid && p < HW && gp_selected(labels[(int64_t)img * HW + p], q_label, neg, grid, p);
}

// cnt[query * nchunk + c] = selected pixels of the query in chunk c (GP_CHUNK pixels of its image)
__global__ __launch_bounds__(256) void gp_rank_count_kernel(const int* q_img, const int* q_label, const int* q_neg,
                                                            int N, int HW, int nchunk, const int* labels,
                                                            const uint8_t* grid, int* cnt) {
  __shared__ int wc[GP_BLOCK / GP_WAVE];
  const int qi = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  const int img = q_img[qi], ql = q_label[qi], neg = q_neg[qi];
  const bool valid = img >= 0 && img < N;
  int acc = 0;  // (wave-uniform)
  for (int s = 0; s < GP_TILES; ++s) {
    const int p = c * GP_CHUNK + s * GP_BLOCK + threadIdx.x;
    acc += gp_popc(__ballot(gp_query_pixel(valid, img, HW, p, labels, ql, neg, grid)));
  }
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// one block per query: the chunk that holds the rank (prefix sums over the chunk counts, at most
// ceil(nchunk / 256) <= 16 chunks per thread), then the pixel inside it (GP_TILES tiles)
__global__ __launch_bounds__(256) void gp_rank_pick_kernel(const int* q_img, const int* q_label, const int* q_neg,
                                                           const int* q_rank, int N, int HW, int W, int nchunk,
                                                           const int* labels, const uint8_t* grid, const int* cnt,
                                                           int* xy, int* count) {
  __shared__ int sh[GP_BLOCK / GP_WAVE];
  __shared__ int pick[2];
  const int qi = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int img = q_img[qi], ql = q_label[qi], neg = q_neg[qi], rank = q_rank[qi];
  const bool valid = img >= 0 && img < N;
  const int* row = cnt + (int64_t)qi * nchunk;
  const int per = (nchunk + GP_BLOCK - 1) / GP_BLOCK;
  int local = 0;
  for (int j = 0; j < per; ++j) {
    const int c = threadIdx.x * per + j;
    if (c < nchunk) local += row[c];
  }
  if (threadIdx.x == 0) pick[0] = -1;
  int total;
  const int ex = gp_block_scan(local, &total, sh);  // (its barriers also order pick[0] = -1 before the writes below)
  if (rank >= ex && rank < ex + local) {            // exactly one thread when 0 <= rank < total
    int acc = ex;
    for (int j = 0; j < per; ++j) {
      const int c = threadIdx.x * per + j;
      const int v = c < nchunk ? row[c] : 0;
      if (rank < acc + v) {
        pick[0] = c;
        pick[1] = rank - acc;
        break;
      }
      acc += v;
    }
  }
  __syncthreads();
  const int chunk = pick[0], rem = pick[1];
  if (threadIdx.x == 0) count[qi] = total;
  if (chunk < 0) {  // (uniform over the block)
    if (threadIdx.x == 0) xy[2 * qi] = xy[2 * qi + 1] = -1;
    return;
  }
  int running = 0;
  for (int s = 0; s < GP_TILES; ++s) {
    const int p = chunk * GP_CHUNK + s * GP_BLOCK + threadIdx.x;
    const bool match = gp_query_pixel(valid, img, HW, p, labels, ql, neg, grid);
    const uint64_t m = __ballot(match);
    if (lane == 0) sh[wave] = gp_popc(m);
    __syncthreads();
    int pre = running + gp_popc(gp_below(m, lane)), tot = 0;
#pragma unroll
    for (int w = 0; w < GP_BLOCK / GP_WAVE; ++w) {
      if (w < wave) pre += sh[w];
      tot += sh[w];
    }
    if (match && pre == rem) {
      xy[2 * qi] = p % W;
      xy[2 * qi + 1] = p / W;
    }
    running += tot;
    __syncthreads();
  }
}

bool gp_reach_ok(int lo, int hi) { return lo >= -GP_MAX_REACH && lo <= 0 && hi >= 0 && hi <= GP_MAX_REACH; }

}  // namespace

extern "C" int s2h_rle_decode(int A, int H, int W, const int* run_off, const int* run_end, uint8_t* mask,
                              hipStream_t st) {
  const int total = gp_total(A, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!run_off || !run_end || !mask) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gp_rle_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, H * W, H, W,
                     run_off, run_end, mask);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_morph_rect(int N, int H, int W, const uint8_t* in, int op, int y_lo, int y_hi, int x_lo, int x_hi,
                              uint8_t* out, uint8_t* work, hipStream_t st) {
  const int total = gp_total(N, H, W);
  if (total < 0 || (op != 0 && op != 1) || !gp_reach_ok(y_lo, y_hi) || !gp_reach_ok(x_lo, x_hi))
    return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!in || !out || !work || out == in || work == in || work == out) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(gp_morph_pass_kernel, grid, block, 0, st, total, H * W, H, W, in, op, x_lo, x_hi, 0, work);
  hipLaunchKernelGGL(gp_morph_pass_kernel, grid, block, 0, st, total, H * W, H, W, (const uint8_t*)work, op, y_lo, y_hi,
                     1, out);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_cc_components(int N, int H, int W, const int* labels, const int* areas, int min_area,
                                 const uint8_t* grid, int capacity, int* hdr, int64_t* stats, uint8_t* index,
                                 int* work, hipStream_t st) {
  const int total = gp_total(N, H, W);
  if (total < 0 || capacity < 0 || !hdr) return (int)hipErrorInvalidValue;
  const int HW = H * W, nb = (HW + 255) / 256;
  if ((int64_t)N * nb > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (N > 0 && (!labels || !areas || !index || !work || (capacity > 0 && !stats))) return (int)hipErrorInvalidValue;
  int* rk = work;           // [N, H, W]
  int* blk = work + total;  // [N, nb]
  const dim3 block(256);
  if (N > 0) {
    hipLaunchKernelGGL(gp_comp_count_kernel, dim3((unsigned)(N * nb)), block, 0, st, HW, nb, labels, areas, min_area,
                       blk);
    hipLaunchKernelGGL(gp_comp_scan_kernel, dim3((unsigned)N), block, 0, st, nb, blk, hdr);
  }
  hipLaunchKernelGGL(gp_comp_offsets_kernel, dim3(1), block, 0, st, N, hdr);
  if (N > 0) {
    hipLaunchKernelGGL(gp_comp_rank_kernel, dim3((unsigned)(N * nb)), block, 0, st, HW, nb, H, W, labels, areas,
                       min_area, (const int*)blk, (const int*)hdr, capacity, rk, stats);
    hipLaunchKernelGGL(gp_comp_stats_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, st, total, HW, W, labels,
                       (const int*)rk, grid, (const int*)hdr, capacity, stats, index);
  }
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_mask_rank_select(int Q, const int* q_img, const int* q_label, const int* q_neg, const int* q_rank,
                                    int N, int H, int W, const int* labels, const uint8_t* grid, int* xy, int* count,
                                    int* work, hipStream_t st) {
  const int total = gp_total(N, H, W);
  if (total < 0 || Q < 0) return (int)hipErrorInvalidValue;
  if (Q == 0) return 0;
  const int HW = H * W, nchunk = (HW + GP_CHUNK - 1) / GP_CHUNK;
  if ((int64_t)Q * nchunk > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (!q_img || !q_label || !q_neg || !q_rank || !xy || !count || !work || (N > 0 && !labels))
    return (int)hipErrorInvalidValue;
  const dim3 block(256);
  hipLaunchKernelGGL(gp_rank_count_kernel, dim3((unsigned)(Q * nchunk)), block, 0, st, q_img, q_label, q_neg, N, HW,
                     nchunk, labels, grid, work);
  hipLaunchKernelGGL(gp_rank_pick_kernel, dim3((unsigned)Q), block, 0, st, q_img, q_label, q_neg, q_rank, N, HW, W,
                     nchunk, labels, grid, (const int*)work, xy, count);
  S2H_LAUNCH_CHECK();
}
