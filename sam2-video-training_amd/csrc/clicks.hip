// Correction clicks on the device (reference sam2_video/model/modeling/sam2_utils.py:202-323,
// sample_one_point_from_error_center and sample_random_points_from_errors): the exact squared Euclidean distance
// transform of byte masks, the click at the centre of the larger error region, and a uniformly drawn click in the
// error regions.  The reference copies two full-resolution masks per object to the host and runs
// cv2.distanceTransform twice; here nothing but the clicks leaves the device.
//
// Row pass: one workgroup per image row; a wave forms a 64-pixel region word with a ballot, the words of the row
// and their carries (the run of set pixels before and after each word) go through LDS, every lane takes its
// distance to the nearest clear pixel of the row from count-leading / count-trailing zeros (clicks.h) and stores
// it as uint16.  Column pass: one lane per pixel, lanes along x, rows y - d and y + d while d^2 can still
// improve: every global access is coalesced along x.  The centre entry forms FN and FP on the fly (a pixel is in
// at most one of them, so one tagged uint16 plane holds both), never writes D2, and reduces the argmax key
// (D2 << 32 | ~index) per workgroup and then over the workgroups' partials in a second launch.  The uniform
// entry counts per chunk, sums the chunks per object and picks by ballot + popcount rank inside the chunk, the
// structure of s2h_mask_rank_select.  Integer arithmetic only, no atomics at all: the results are pure functions
// of the inputs.  Every loop has a bound that does not depend on the data (clicks.h, and the comments below).
#include "clicks.h"
#include "common.h"

namespace {

// N * H * W as int, or -1 when the sizes are outside what the kernels index
int ck_total(int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1 || H > CK_MAX_SIDE || W > CK_MAX_SIDE || (int64_t)H * W > GP_MAX_PIXELS) return -1;
  const int64_t t = (int64_t)N * H * W;
  return t + 256 > 0x7fffffffLL ? -1 : (int)t;
}

// --------------------------------------------------------------------------------------------- row pass
// One workgroup per row (blockIdx.x = image * H + y).  a: the mask (fused 0) or gt (fused 1); b: pred or NULL.
// ceil(nw / 4) <= 16 words per wave, twice; the carries: nw <= 64 steps on one lane of each wave.
__global__ __launch_bounds__(256) void ck_row_kernel(int W, int nw, const uint8_t* a, const uint8_t* b, int fused,
                                                     uint16_t* hplane) {
  __shared__ uint64_t words[2][CK_MAX_WORDS];
  __shared__ int run_l[2][CK_MAX_WORDS], run_r[2][CK_MAX_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * W;
  for (int w = wave; w < nw; w += GP_BLOCK / GP_WAVE) {
    const int x = w * GP_WAVE + lane;
    const bool in = x < W;
    const bool g = in && a[row + x] != 0;
    const bool p = in && b && b[row + x] != 0;
    const uint64_t first = __ballot(fused ? ck_fn(g, p) : g);
    const uint64_t second = __ballot(fused && in && ck_fp(g, p));
    if (lane == 0) {
      words[0][w] = first;
      words[1][w] = second;
    }
  }
  __syncthreads();
  if (lane == 0) {  // wave 0, 1: the left carries of the two regions; wave 2, 3: the right carries
    if (wave < 2)
      ck_row_carry_left(words[wave], nw, run_l[wave]);
    else
      ck_row_carry_right(words[wave - 2], nw, run_r[wave - 2]);
  }
  __syncthreads();
  for (int w = wave; w < nw; w += GP_BLOCK / GP_WAVE) {
    const int x = w * GP_WAVE + lane;
    if (x < W)
      hplane[row + x] = ck_pack(ck_row_dist(words[0][w], lane, run_l[0][w], run_r[0][w]),
                                ck_row_dist(words[1][w], lane, run_l[1][w], run_r[1][w]));
  }
}

// --------------------------------------------------------------------------------------------- column pass
// one thread per pixel, the N images laid end to end (the host checked total + 256 < 2^31)
__global__ __launch_bounds__(256) void ck_col_store_kernel(int total, int HW, int H, int W, const uint16_t* hplane,
                                                           int* dist2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = i % HW;
  int tag;
  dist2[i] = ck_col_d2(hplane + (i - q), H, W, q / W, q % W, &tag);
}

__device__ __forceinline__ uint64_t ck_shfl_xor64(uint64_t v, int o) {
  const int lo = __shfl_xor((int)(uint32_t)v, o, GP_WAVE), hi = __shfl_xor((int)(uint32_t)(v >> 32), o, GP_WAVE);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// maxima of two keys over the 256 threads of the block, valid in thread 0; sh: 8 words of LDS
__device__ __forceinline__ void ck_block_max2(uint64_t& k0, uint64_t& k1, uint64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t0 = ck_shfl_xor64(k0, o), t1 = ck_shfl_xor64(k1, o);
    k0 = t0 > k0 ? t0 : k0;
    k1 = t1 > k1 ? t1 : k1;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[2 * wave] = k0;
    sh[2 * wave + 1] = k1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < GP_BLOCK / GP_WAVE; ++w) {
      k0 = sh[2 * w] > k0 ? sh[2 * w] : k0;
      k1 = sh[2 * w + 1] > k1 ? sh[2 * w + 1] : k1;
    }
  }
}

// part[(image * nb + b) * 2 + region] = the largest key among pixels [256 b, 256 b + 256) of the image; a pixel
// enters its own region with its D2 and the other one with 0, so an empty region's maximum is key(0, 0)
__global__ __launch_bounds__(256) void ck_col_key_kernel(int HW, int nb, int H, int W, const uint16_t* hplane,
                                                         uint64_t* part) {
  __shared__ uint64_t sh[2 * GP_BLOCK / GP_WAVE];
  const int img = blockIdx.x / nb, b = blockIdx.x % nb;
  const int q = b * 256 + threadIdx.x;
  uint64_t k0 = 0, k1 = 0;  // (below every real key: key(0, idx) has nonzero low bits for idx < 2^32 - 1)
  if (q < HW) {
    int tag;
    const int d2 = ck_col_d2(hplane + (int64_t)img * HW, H, W, q / W, q % W, &tag);
    k0 = ck_key(tag ? 0 : d2, q);
    k1 = ck_key(tag ? d2 : 0, q);
  }
  ck_block_max2(k0, k1, sh);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = k0;
    part[2 * (int64_t)blockIdx.x + 1] = k1;
  }
}

// one block per object: the partials in a fixed assignment (thread t takes b = t, t + 256, ...:
// ceil(nb / 256) <= 256 rounds), then the click
__global__ __launch_bounds__(256) void ck_center_pick_kernel(int nb, int W, const uint64_t* part, float* points,
                                                             int* labels, int* dmax) {
  __shared__ uint64_t sh[2 * GP_BLOCK / GP_WAVE];
  const uint64_t* row = part + 2 * (int64_t)blockIdx.x * nb;
  uint64_t k0 = 0, k1 = 0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    k0 = row[2 * b] > k0 ? row[2 * b] : k0;
    k1 = row[2 * b + 1] > k1 ? row[2 * b + 1] : k1;
  }
  ck_block_max2(k0, k1, sh);
  if (threadIdx.x == 0)
    ck_center_click(k0, k1, W, points + 2 * blockIdx.x, labels + blockIdx.x, dmax + 2 * blockIdx.x);
}

// --------------------------------------------------------------------------------------------- uniform click
// exclusive prefix of v over the 256 threads of the block and the block's total; sh: 4 ints of LDS.
// The two barriers make sh reusable right after the call.
__device__ __forceinline__ int ck_block_scan(int v, int* total, int* sh) {
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

// cnt[(object * nchunk + c) * 3 ..] = |FP|, |FN|, |~gt| inside chunk c (GP_CHUNK pixels of the object)
__global__ __launch_bounds__(256) void ck_uni_count_kernel(int HW, int nchunk, const uint8_t* gt, const uint8_t* pred,
                                                           int* cnt) {
  __shared__ int wc[3][GP_BLOCK / GP_WAVE];
  const int obj = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  const int64_t base = (int64_t)obj * HW;
  int a0 = 0, a1 = 0, a2 = 0;  // (wave-uniform)
  for (int s = 0; s < GP_TILES; ++s) {
    const int q = c * GP_CHUNK + s * GP_BLOCK + threadIdx.x;
    const bool in = q < HW;
    const bool g = in && gt[base + q] != 0;
    const bool p = in && pred && pred[base + q] != 0;
    a0 += gp_popc(__ballot(in && ck_fp(g, p)));
    a1 += gp_popc(__ballot(ck_fn(g, p)));
    a2 += gp_popc(__ballot(in && !g));
  }
  if ((threadIdx.x & 63) == 0) {
    wc[0][threadIdx.x >> 6] = a0;
    wc[1][threadIdx.x >> 6] = a1;
    wc[2][threadIdx.x >> 6] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int* w = wc[threadIdx.x];
    cnt[3 * (int64_t)blockIdx.x + threadIdx.x] = w[0] + w[1] + w[2] + w[3];
  }
}

// one block per object: tot[3 object ..] = the three sums over its chunks (thread t takes c = t, t + 256, ...:
// ceil(nchunk / 256) <= 16 rounds; integer sums, so the order does not matter), count = (|R0|, |R1|)
__global__ __launch_bounds__(256) void ck_uni_total_kernel(int nchunk, const int* cnt, int* tot, int* count) {
  __shared__ int sh[GP_BLOCK / GP_WAVE];
  const int* row = cnt + 3 * (int64_t)blockIdx.x * nchunk;
  int a[3] = {0, 0, 0};
  for (int c = threadIdx.x; c < nchunk; c += 256) {
    a[0] += row[3 * c];
    a[1] += row[3 * c + 1];
    a[2] += row[3 * c + 2];
  }
  int t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) ck_block_scan(a[k], &t[k], sh);
  if (threadIdx.x == 0) {
    const bool all_correct = t[0] + t[1] == 0;
    tot[3 * blockIdx.x] = t[0];
    tot[3 * blockIdx.x + 1] = t[1];
    tot[3 * blockIdx.x + 2] = t[2];
    count[2 * blockIdx.x] = all_correct ? t[2] : t[0];
    count[2 * blockIdx.x + 1] = t[1];
  }
}

// one block per click (blockIdx.x = object * P + click): the chunk that holds the rank (prefix sums over the
// chunks' union counts, at most ceil(nchunk / 256) <= 16 chunks per thread), then the pixel inside it (GP_TILES
// tiles)
__global__ __launch_bounds__(256) void ck_uni_pick_kernel(int P, int HW, int W, int nchunk, const uint8_t* gt,
                                                          const uint8_t* pred, const int64_t* r, const int* cnt,
                                                          const int* tot, float* points, int* labels) {
  __shared__ int sh[GP_BLOCK / GP_WAVE];
  __shared__ int pick[2];
  const int obj = blockIdx.x / P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)obj * HW;
  const bool all_correct = tot[3 * obj] + tot[3 * obj + 1] == 0;
  const int n = all_correct ? tot[3 * obj + 2] : tot[3 * obj] + tot[3 * obj + 1];
  if (n == 0) {  // (uniform over the block) nothing to draw from: gt covers the image and pred equals it
    if (threadIdx.x == 0) {
      points[2 * (int64_t)blockIdx.x] = points[2 * (int64_t)blockIdx.x + 1] = 0.f;
      labels[blockIdx.x] = 0;
    }
    return;
  }
  const int rank = ck_rank(r[blockIdx.x], n);
  const int* row = cnt + 3 * (int64_t)obj * nchunk;
  const int per = (nchunk + GP_BLOCK - 1) / GP_BLOCK;
  int local = 0;
  for (int j = 0; j < per; ++j) {
    const int c = threadIdx.x * per + j;
    if (c < nchunk) local += all_correct ? row[3 * c + 2] : row[3 * c] + row[3 * c + 1];
  }
  if (threadIdx.x == 0) pick[0] = -1;
  int total;
  const int ex = ck_block_scan(local, &total, sh);  // (its barriers also order pick[0] = -1 before the writes below)
  if (rank >= ex && rank < ex + local) {            // exactly one thread, as 0 <= rank < n = total
    int acc = ex;
    for (int j = 0; j < per; ++j) {
      const int c = threadIdx.x * per + j;
      const int v = c < nchunk ? (all_correct ? row[3 * c + 2] : row[3 * c] + row[3 * c + 1]) : 0;
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
  if (chunk < 0) return;  // (uniform over the block; not reached while cnt and tot come from the same masks)
  int running = 0;
  for (int s = 0; s < GP_TILES; ++s) {
    const int q = chunk * GP_CHUNK + s * GP_BLOCK + threadIdx.x;
    const bool in = q < HW;
    const bool g = in && gt[base + q] != 0;
    const bool p = in && pred && pred[base + q] != 0;
    const bool match = in && ck_union(g, p, all_correct);
    const uint64_t m = __ballot(match);
    if (lane == 0) sh[wave] = gp_popc(m);
    __syncthreads();
    int pre = running + gp_popc(gp_below(m, lane)), t = 0;
#pragma unroll
    for (int w = 0; w < GP_BLOCK / GP_WAVE; ++w) {
      if (w < wave) pre += sh[w];
      t += sh[w];
    }
    if (match && pre == rem) {
      points[2 * (int64_t)blockIdx.x] = (float)(q % W);
      points[2 * (int64_t)blockIdx.x + 1] = (float)(q / W);
      labels[blockIdx.x] = ck_fn(g, p) ? 1 : 0;
    }
    running += t;
    __syncthreads();
  }
}

}  // namespace

extern "C" int s2h_edt_sq(int N, int H, int W, const uint8_t* mask, int* dist2, void* work, hipStream_t st) {
  const int total = ck_total(N, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (!mask || !dist2 || !work) return (int)hipErrorInvalidValue;
  uint16_t* hplane = (uint16_t*)work;  // [N, H, W]
  hipLaunchKernelGGL(ck_row_kernel, dim3((unsigned)(N * H)), dim3(256), 0, st, W, (W + 63) / 64, mask,
                     (const uint8_t*)nullptr, 0, hplane);
  hipLaunchKernelGGL(ck_col_store_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, H * W, H, W,
                     (const uint16_t*)hplane, dist2);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_error_center_click(int B, int H, int W, const uint8_t* gt, const uint8_t* pred, float* points,
                                      int* labels, int* dmax, void* work, hipStream_t st) {
  const int total = ck_total(B, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!gt || !points || !labels || !dmax || !work) return (int)hipErrorInvalidValue;
  const int HW = H * W, nb = (HW + 255) / 256;
  if ((int64_t)B * nb > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  uint64_t* part = (uint64_t*)work;                        // [B, nb, 2]
  uint16_t* hplane = (uint16_t*)(part + 2 * (int64_t)B * nb);  // [B, H, W]
  hipLaunchKernelGGL(ck_row_kernel, dim3((unsigned)(B * H)), dim3(256), 0, st, W, (W + 63) / 64, gt, pred, 1, hplane);
  hipLaunchKernelGGL(ck_col_key_kernel, dim3((unsigned)(B * nb)), dim3(256), 0, st, HW, nb, H, W,
                     (const uint16_t*)hplane, part);
  hipLaunchKernelGGL(ck_center_pick_kernel, dim3((unsigned)B), dim3(256), 0, st, nb, W, (const uint64_t*)part, points,
                     labels, dmax);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_error_uniform_click(int B, int P, int H, int W, const uint8_t* gt, const uint8_t* pred,
                                       const int64_t* r, float* points, int* labels, int* count, int* work,
                                       hipStream_t st) {
  const int total = ck_total(B, H, W);
  if (total < 0 || P < 0 || (int64_t)B * P > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!gt || !count || !work || (P > 0 && (!r || !points || !labels))) return (int)hipErrorInvalidValue;
  const int HW = H * W, nchunk = (HW + GP_CHUNK - 1) / GP_CHUNK;
  if ((int64_t)B * nchunk * 3 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  int* cnt = work;                            // [B, nchunk, 3]
  int* tot = work + 3 * (int64_t)B * nchunk;  // [B, 3]
  const dim3 block(256);
  hipLaunchKernelGGL(ck_uni_count_kernel, dim3((unsigned)(B * nchunk)), block, 0, st, HW, nchunk, gt, pred, cnt);
  hipLaunchKernelGGL(ck_uni_total_kernel, dim3((unsigned)B), block, 0, st, nchunk, (const int*)cnt, tot, count);
  if (P > 0)
    hipLaunchKernelGGL(ck_uni_pick_kernel, dim3((unsigned)(B * P)), block, 0, st, P, HW, W, nchunk, gt, pred, r,
                       (const int*)cnt, (const int*)tot, points, labels);
  S2H_LAUNCH_CHECK();
}
