// Category-merged COCO RLE export of the video predictor's masks on the device (reference
// sam2_video/eval/inference.py:487-514 and :870-901: per object `(logits > 0).cpu()`, a sigmoid mean
// `.item()`, a host OR per category, pycocotools encode, mask_to_bbox).  Only run boundaries, six integers
// per category and one float per object are left for the host to copy.
//
// s2h_mask_export: one thread per video-resolution pixel in COLUMN-major order (y fastest), so the 64
//   lanes of a wave are the 64 bits of one word of the Fortran-order bit mask and the ballot is the stored
//   word.  Each thread evaluates the bilinear value of s2h_bilinear_fwd (bilinear_tap.h, the same inlined
//   expression) per object from the low-res planes, which stay in L1 / L2 (13 x 128^2 fp32 = 852 KB; a
//   wave touches 64 * hi / H + 2 input rows of one or two columns).  Nothing the size of [N, H, W] is
//   stored, so values are recomputed instead of kept: one pass for the per-pixel argmax (non-overlap only),
//   one over the objects for the sigmoid sums, one over the categories' object lists for the bits.
//   The sigmoid sums are reduced in a fixed order: butterfly within the wave, the four waves in order, one
//   partial per workgroup and object, then det_colsum (reduce_det.h).  No atomics.
// s2h_mask_export_cut: the same kernel body (a template flag) with foreground `value >= cut` for a tuned
//   threshold (eval/tune_threshold.py logit_cuts) and the per-object maximum value, reduced like the sums
//   (fmaxf per wave, workgroup, then over the workgroups).
// s2h_mask_sweep: the threshold sweep.  The same pixel mapping and values; per category the maximum over
//   its objects is binned against K cuts and counted per bin and ground-truth bit (sweep_hist.h): the wave's
//   ground-truth word is one load, a bin's pixels one ballot and two popcounts.  Integer adds only.
// s2h_rle_transitions: count / scan / emit over the words (rle_scan.h), 256 words per workgroup:
//   1. per word the popcount of its transition mask and its area / bounding box, reduced per workgroup;
//   2. one workgroup scans the workgroup counts (exclusive, over words then categories) and folds the
//      statistics per category in workgroup order -> the header;
//   3. every workgroup scans its 256 counts again and writes its positions behind its offset.
//   Integer arithmetic in a fixed order throughout: the output is a pure function of the bits.
// s2h_rle_pair_counts: the offline scoring's four counts per (image, category) group from the run boundaries
//   of its predicted and ground-truth annotations (pair_counts.h): a wave is one word of 64 column-major
//   positions, a lane searches its position in every annotation of a side, the two ballots are the words of
//   the OR-ed masks.  No mask is stored.  Integer adds (uint64 atomics, one per workgroup and count).
#include "bilinear_tap.h"
#include "common.h"
#include "pair_counts.h"
#include "reduce_det.h"
#include "rle_scan.h"
#include "sweep_hist.h"

namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// part[blockIdx.x][i] = (sum over the workgroup's pixels of sigmoid(final value of object i)) / (H W);
// bits[c][word] = OR over the objects of category c of (final value > 0)
// CUT (s2h_mask_export_cut): foreground is final value >= cut instead, and pmax[blockIdx.x][i] = the maximum
// over the workgroup's pixels of the final value of object i (fmaxf from -inf: NaN is skipped)
template <bool CUT>
__global__ __launch_bounds__(256) void mask_export_kernel(int N, int hi, int wi, int H, int W, const float* low,
                                                          int Ncat, const int* cat_off, const int* cat_obj,
                                                          int non_overlap, uint64_t* bits, int nw, float* part,
                                                          float cut, float* pmax) {
  __shared__ float red[2][4];
  __shared__ float redm[2][4];
  const int HW = H * W;
  const int j = blockIdx.x * 256 + threadIdx.x;  // (the host checked H W <= 2^24)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in = j < HW;
  const int jj = in ? j : HW - 1;  // lanes past the end compute the last pixel and contribute nothing
  const int x = jj / H, y = jj - x * H;
  const float sh = (float)hi / H, sw = (float)wi / W;
  int y0, y1, x0, x1;
  float ly, lx;
  bil_src(y, sh, hi, y0, y1, ly);
  bil_src(x, sw, wi, x0, x1, lx);
  const int64_t plane = (int64_t)hi * wi;

  // SAM2VideoPredictor._apply_non_overlapping_constraints: the object of the highest value keeps it (the
  // first index on a tie, as torch.argmax), every other object is clamped to <= -10
  int arg = -1;
  if (non_overlap && N > 0) {
    float best = bil_tap(low, wi, y0, y1, x0, x1, ly, lx);
    arg = 0;
    for (int i = 1; i < N; ++i) {
      const float v = bil_tap(low + i * plane, wi, y0, y1, x0, x1, ly, lx);
      if (v > best) {
        best = v;
        arg = i;
      }
    }
  }

  const float inv_n = 1.f / (float)HW;
  for (int i = 0; i < N; ++i) {
    float v = bil_tap(low + i * plane, wi, y0, y1, x0, x1, ly, lx);
    if (arg >= 0 && i != arg) v = fminf(v, -10.f);
    const float s = wave_sum_f(in ? 1.f / (1.f + expf(-v)) : 0.f);
    if (lane == 0) red[i & 1][wave] = s;
    if (CUT) {
      const float mx = wave_max_f(in ? v : -INFINITY);
      if (lane == 0) redm[i & 1][wave] = mx;
    }
    __syncthreads();  // (one barrier per object: iteration i + 2 rewrites red[i & 1] after the next barrier)
    if (threadIdx.x == 0) {
      part[(int64_t)blockIdx.x * N + i] = ((red[i & 1][0] + red[i & 1][1]) + (red[i & 1][2] + red[i & 1][3])) * inv_n;
      if (CUT)
        pmax[(int64_t)blockIdx.x * N + i] =
            fmaxf(fmaxf(redm[i & 1][0], redm[i & 1][1]), fmaxf(redm[i & 1][2], redm[i & 1][3]));
    }
  }

  const int word = j >> 6;  // the same for the 64 lanes of a wave
  for (int c = 0; c < Ncat; ++c) {
    const int k0 = cat_off[c];
    const int k1 = min(cat_off[c + 1], k0 + N);  // a category lists at most N objects: the loop is bounded
    bool fg = false;
    for (int k = k0; k < k1; ++k) {
      const int o = cat_obj[k];
      if ((unsigned)o >= (unsigned)N) continue;
      float v = bil_tap(low + o * plane, wi, y0, y1, x0, x1, ly, lx);
      if (arg >= 0 && o != arg) v = fminf(v, -10.f);
      fg = fg || (CUT ? v >= cut : v > 0.f);  // 0.0, -0.0 and NaN are background (CUT: NaN is, -0.0 >= 0.0)
    }
    const uint64_t m = __ballot(in && fg);  // bits past H W stay zero
    if (lane == 0 && word < nw) bits[(int64_t)c * nw + word] = m;
  }
}

// out[i] = max over the nr rows of pmax[r][i] (fmaxf: any order gives the same value); one workgroup per i
__global__ __launch_bounds__(256) void colmax_kernel(int nr, int N, const float* pmax, float* out) {
  __shared__ float red[4];
  const int i = blockIdx.x;
  float m = -INFINITY;
  for (int r = threadIdx.x; r < nr; r += 256) m = fmaxf(m, pmax[(int64_t)r * N + i]);
  m = wave_max_f(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[i] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// hist[c][g][b] += the workgroup's pixels of category c with ground-truth bit g whose merged value (the
// maximum over the category's objects of the final value, NaN skipped, -inf for no object) lies in bin b
// (sweep_hist.h).  The pixel mapping, the taps and the non-overlap clamp are mask_export_kernel's; a
// workgroup is SWEEP_BLOCK pixels = 16 words.  hist is zero on entry.
__global__ __launch_bounds__(SWEEP_BLOCK) void mask_sweep_kernel(int N, int hi, int wi, int H, int W, const float* low,
                                                                 int Ncat, const int* cat_off, const int* cat_obj,
                                                                 int non_overlap, int K, const float* cuts,
                                                                 const uint64_t* gt_bits, int nw, int* hist) {
  __shared__ int blk[2 * (SWEEP_MAX_K + 1)];
  __shared__ float scut[SWEEP_MAX_K];
  if ((int)threadIdx.x < K) scut[threadIdx.x] = cuts[threadIdx.x];
  if ((int)threadIdx.x < 2 * (K + 1)) blk[threadIdx.x] = 0;
  __syncthreads();
  const int HW = H * W;
  const int j = blockIdx.x * SWEEP_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = j < HW;
  const int jj = in ? j : HW - 1;
  const int x = jj / H, y = jj - x * H;
  const float sh = (float)hi / H, sw = (float)wi / W;
  int y0, y1, x0, x1;
  float ly, lx;
  bil_src(y, sh, hi, y0, y1, ly);
  bil_src(x, sw, wi, x0, x1, lx);
  const int64_t plane = (int64_t)hi * wi;

  int arg = -1;  // as mask_export_kernel
  if (non_overlap && N > 0) {
    float best = bil_tap(low, wi, y0, y1, x0, x1, ly, lx);
    arg = 0;
    for (int i = 1; i < N; ++i) {
      const float v = bil_tap(low + i * plane, wi, y0, y1, x0, x1, ly, lx);
      if (v > best) {
        best = v;
        arg = i;
      }
    }
  }

  const int word = j >> 6;  // the same for the 64 lanes of a wave
  const uint64_t valid = __ballot(in);
  for (int c = 0; c < Ncat; ++c) {
    const int k0 = cat_off[c];
    const int k1 = min(cat_off[c + 1], k0 + N);
    float m = -INFINITY;
    for (int k = k0; k < k1; ++k) {
      const int o = cat_obj[k];
      if ((unsigned)o >= (unsigned)N) continue;
      float v = bil_tap(low + o * plane, wi, y0, y1, x0, x1, ly, lx);
      if (arg >= 0 && o != arg) v = fminf(v, -10.f);
      m = fmaxf(m, v);  // (fmaxf returns the other operand for a NaN)
    }
    const int b = sweep_bin(m, scut, K);
    // one load per wave; a wave entirely past H W has valid == 0 and reads nothing
    const uint64_t gt = (gt_bits && valid) ? gt_bits[(int64_t)c * nw + word] : 0ull;
    for (int q = 0; q <= K; ++q) {
      const uint64_t sel = __ballot(in && b == q);
      if (sel && lane == 0) sweep_block_add(blk, K, q, sweep_word_counts(sel, gt));
    }
    __syncthreads();
    sweep_block_flush(hist + (int64_t)c * 2 * (K + 1), blk, K, threadIdx.x, SWEEP_BLOCK);
    __syncthreads();
  }
}

// the word of thread `tid` of workgroup f = c * nbw + b: tail-masked bits, transition mask, first pixel
struct RleWord {
  uint64_t w, t;
  int base;
};
__device__ __forceinline__ RleWord rle_load_word(const uint64_t* bits, int f, int nbw, int nw, int n) {
  const int c = f / nbw, b = f - c * nbw;
  const int wi = b * RLE_BLOCK_WORDS + threadIdx.x;
  RleWord r = {0ull, 0ull, 0};
  if (wi < nw) {
    const uint64_t* row = bits + (int64_t)c * nw;
    const uint64_t valid = rle_valid(wi, n);
    r.w = row[wi] & valid;
    r.t = rle_transitions(r.w, wi > 0 ? row[wi - 1] >> 63 : 0ull, valid);
    r.base = wi * 64;
  }
  return r;
}

// exclusive scan of v over the 256 threads (in thread order), *total = the sum; sh: 4 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  __syncthreads();  // (sh may still be read from the previous call)
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < wave) before += sh[q];
    all += sh[q];
  }
  *total = all;
  return before + incl - v;
}

// cnt[f] = transitions in workgroup f's 256 words; stats[f] = area and bounding box of those words
__global__ __launch_bounds__(RLE_BLOCK_WORDS) void rle_count_kernel(int nbw, int nw, int H, int W, const uint64_t* bits,
                                                                    int* cnt, int* stats) {
  __shared__ int red[4][6];
  const int f = blockIdx.x;
  const RleWord r = rle_load_word(bits, f, nbw, nw, H * W);
  const RleStats s = rle_word_stats(r.w, r.base, H, W);
  const int v[6] = {wave_sum_i(rle_popc(r.t)), wave_sum_i(s.area), wave_min_i(s.xmin),
                    wave_min_i(s.ymin),        wave_max_i(s.xmax), wave_max_i(s.ymax)};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) red[wave][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[f] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    int* o = stats + (int64_t)f * 5;
    o[0] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    o[1] = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
    o[2] = min(min(red[0][3], red[1][3]), min(red[2][3], red[3][3]));
    o[3] = max(max(red[0][4], red[1][4]), max(red[2][4], red[3][4]));
    o[4] = max(max(red[0][5], red[1][5]), max(red[2][5], red[3][5]));
  }
}

// one workgroup: off[f] = exclusive scan of cnt over all F = Ncat * nbw workgroups (words, then categories:
// the categories' positions lie back to back), then the header of every category
__global__ __launch_bounds__(256) void rle_scan_kernel(int Ncat, int nbw, int H, int W, const int* cnt,
                                                       const int* stats, int* off, int* hdr) {
  __shared__ int sh[4];
  const int F = Ncat * nbw;
  int run = 0;
  for (int base = 0; base < F; base += 256) {
    const int idx = base + threadIdx.x;
    int tot;
    const int e = block_excl_scan(idx < F ? cnt[idx] : 0, sh, &tot);
    if (idx < F) off[idx] = run + e;
    run += tot;
  }
  __threadfence_block();
  __syncthreads();  // off[] is read below by other threads of this workgroup
  for (int c = threadIdx.x; c < Ncat; c += 256) {
    const int o0 = off[c * nbw];
    const int o1 = c + 1 < Ncat ? off[(c + 1) * nbw] : run;
    RleStats s = rle_stats_empty(H, W);
    for (int b = 0; b < nbw; ++b) {
      const int* p = stats + (int64_t)(c * nbw + b) * 5;
      const RleStats q = {p[0], p[1], p[2], p[3], p[4]};
      s = rle_stats_join(s, q);
    }
    int* h = hdr + c * RLE_HDR;
    h[0] = o1 - o0;
    h[1] = o0;
    h[2] = s.area;
    h[3] = s.xmin;
    h[4] = s.ymin;
    h[5] = s.xmax;
    h[6] = s.ymax;
    h[7] = run;  // the capacity the call needs (the same in every category's header)
  }
}

__global__ __launch_bounds__(RLE_BLOCK_WORDS) void rle_emit_kernel(int nbw, int nw, int n, const uint64_t* bits,
                                                                   const int* off, int cap, int* trans) {
  __shared__ int sh[4];
  const int f = blockIdx.x;
  const RleWord r = rle_load_word(bits, f, nbw, nw, n);
  int tot;
  const int e = block_excl_scan(rle_popc(r.t), sh, &tot);
  rle_emit(r.t, r.base, trans, off[f] + e, cap);
}


// counts[g] += the counts of the PC_BLOCK / 64 words of workgroup b of group g (blockIdx.x = g * nbw + b);
// counts is zero on entry.  A group with no annotation on either side reads nothing.
__global__ __launch_bounds__(PC_BLOCK) void rle_pair_counts_kernel(int nbw, int HW, const int* dt_grp_off,
                                                                  const int* dt_run_off, const int* dt_run_end,
                                                                  const int* gt_grp_off, const int* gt_run_off,
                                                                  const int* gt_run_end, unsigned long long* counts) {
  __shared__ int red[PC_BLOCK / 64][4];
  const int g = blockIdx.x / nbw, b = blockIdx.x - g * nbw;
  const int d0 = dt_grp_off[g], d1 = dt_grp_off[g + 1], g0 = gt_grp_off[g], g1 = gt_grp_off[g + 1];
  if (d1 <= d0 && g1 <= g0) return;  // (the same for every thread of the workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pos = (b * (PC_BLOCK / 64) + wave) * 64 + lane;  // (the host checked G H W + 256 < 2^31)
  const bool in = pos < HW;
  const uint64_t p = __ballot(in && pc_side_bit(dt_run_off, dt_run_end, d0, d1, pos));
  const uint64_t q = __ballot(in && pc_side_bit(gt_run_off, gt_run_end, g0, g1, pos));
  if (lane == 0) {
    const PcCounts c = pc_word_counts(p, q);
    red[wave][0] = c.inter;
    red[wave][1] = c.uni;
    red[wave][2] = c.np;
    red[wave][3] = c.ng;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < PC_BLOCK / 64; ++w) v += red[w][threadIdx.x];
    if (v) atomicAdd(&counts[(int64_t)g * 4 + threadIdx.x], (unsigned long long)v);
  }
}

// ceil(H W / 64), or -1 when the sizes are outside what the kernels index (those of s2h_cc_label)
int rle_words(int Ncat, int H, int W) {
  if (Ncat < 0 || H < 1 || W < 1 || (int64_t)H * W > RLE_MAX_PIXELS) return -1;
  if ((int64_t)Ncat * H * W + 256 > 0x7fffffffLL) return -1;
  return (H * W + 63) / 64;
}

}  // namespace

extern "C" int s2h_mask_export(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                               const int* cat_obj, int non_overlap, uint64_t* bits, float* score, float* work,
                               hipStream_t st) {
  const int nw = rle_words(Ncat, H, W);
  if (nw < 0 || N < 0 || hi < 1 || wi < 1 || (int64_t)N * hi * wi > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (N == 0 && Ncat == 0) return 0;
  if ((N > 0 && (!low || !score || !work)) || (Ncat > 0 && (!bits || !cat_off || !cat_obj)))
    return (int)hipErrorInvalidValue;
  const int nb = (H * W + 255) / 256;
  hipLaunchKernelGGL(mask_export_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, N, hi, wi, H, W, low, Ncat,
                     cat_off, cat_obj, non_overlap, bits, nw, work, 0.f, (float*)nullptr);
  if (N > 0) det_colsum(1, nb, N, work, score, 0, st);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_mask_export_cut(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                                   const int* cat_obj, int non_overlap, float cut, uint64_t* bits, float* score,
                                   float* vmax, float* work, hipStream_t st) {
  const int nw = rle_words(Ncat, H, W);
  if (nw < 0 || N < 0 || hi < 1 || wi < 1 || (int64_t)N * hi * wi > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (N == 0 && Ncat == 0) return 0;
  if ((N > 0 && (!low || !score || !vmax || !work)) || (Ncat > 0 && (!bits || !cat_off || !cat_obj)))
    return (int)hipErrorInvalidValue;
  const int nb = (H * W + 255) / 256;
  float* pmax = work + (int64_t)nb * N;
  hipLaunchKernelGGL(mask_export_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, N, hi, wi, H, W, low, Ncat,
                     cat_off, cat_obj, non_overlap, bits, nw, work, cut, pmax);
  if (N > 0) {
    det_colsum(1, nb, N, work, score, 0, st);
    hipLaunchKernelGGL(colmax_kernel, dim3((unsigned)N), dim3(256), 0, st, nb, N, (const float*)pmax, vmax);
  }
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_mask_sweep(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                              const int* cat_obj, int non_overlap, int K, const float* cuts, const uint64_t* gt_bits,
                              int* hist, hipStream_t st) {
  const int nw = rle_words(Ncat, H, W);
  if (nw < 0 || N < 0 || hi < 1 || wi < 1 || (int64_t)N * hi * wi > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (K < 1 || K > SWEEP_MAX_K || !cuts) return (int)hipErrorInvalidValue;
  if (Ncat == 0) return 0;
  if (!hist || !cat_off || !cat_obj || (N > 0 && !low)) return (int)hipErrorInvalidValue;
  s2h_zero_f32((float*)hist, 1, (int64_t)Ncat * 2 * (K + 1), (int64_t)Ncat * 2 * (K + 1), st);  // (int 0 = 0.0f bits)
  const int nb = (H * W + SWEEP_BLOCK - 1) / SWEEP_BLOCK;
  hipLaunchKernelGGL(mask_sweep_kernel, dim3((unsigned)nb), dim3(SWEEP_BLOCK), 0, st, N, hi, wi, H, W, low, Ncat, cat_off,
                     cat_obj, non_overlap, K, cuts, gt_bits, nw, hist);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_rle_transitions(int Ncat, int H, int W, const uint64_t* bits, int capacity, int* hdr, int* trans,
                                   int* work, hipStream_t st) {
  const int nw = rle_words(Ncat, H, W);
  if (nw < 0 || capacity < 0) return (int)hipErrorInvalidValue;
  if (Ncat == 0) return 0;
  if (!bits || !hdr || !work || (capacity > 0 && !trans)) return (int)hipErrorInvalidValue;
  const int nbw = (nw + RLE_BLOCK_WORDS - 1) / RLE_BLOCK_WORDS;
  const int F = Ncat * nbw;  // (nbw <= 1024 and Ncat H W < 2^31: F fits)
  int* cnt = work;
  int* off = work + F;
  int* stats = work + 2 * (int64_t)F;
  hipLaunchKernelGGL(rle_count_kernel, dim3((unsigned)F), dim3(RLE_BLOCK_WORDS), 0, st, nbw, nw, H, W, bits, cnt, stats);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(256), 0, st, Ncat, nbw, H, W, (const int*)cnt, (const int*)stats,
                     off, hdr);
  hipLaunchKernelGGL(rle_emit_kernel, dim3((unsigned)F), dim3(RLE_BLOCK_WORDS), 0, st, nbw, nw, H * W, bits,
                     (const int*)off, capacity, trans);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_rle_pair_counts(int G, int H, int W, const int* dt_grp_off, const int* dt_run_off,
                                   const int* dt_run_end, const int* gt_grp_off, const int* gt_run_off,
                                   const int* gt_run_end, uint64_t* counts, hipStream_t st) {
  const int nw = rle_words(G, H, W);  // the limits of s2h_rle_decode, G in place of A
  if (nw < 0) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  // (run_end of a side may be NULL when that side has no annotation at all: it is never read then)
  if (!dt_grp_off || !dt_run_off || !gt_grp_off || !gt_run_off || !counts) return (int)hipErrorInvalidValue;
  s2h_zero_f32((float*)counts, 1, (int64_t)G * 8, (int64_t)G * 8, st);  // (uint64 0 = two 0.0f bit patterns)
  const int nbw = (nw + PC_BLOCK / 64 - 1) / (PC_BLOCK / 64);  // (G * nbw <= G H W / 256 + G < 2^31)
  hipLaunchKernelGGL(rle_pair_counts_kernel, dim3((unsigned)(G * nbw)), dim3(PC_BLOCK), 0, st, nbw, H * W, dt_grp_off,
                     dt_run_off, dt_run_end, gt_grp_off, gt_run_off, gt_run_end, (unsigned long long*)counts);
  S2H_LAUNCH_CHECK();
}
