// Bin index and histogram folding of the threshold sweep (s2h_mask_sweep, rle.hip) as plain functions that
// compile for the device and for the host: sweep_host_check.cpp runs the very same functions sequentially
// in the kernel's decomposition (workgroups of SWEEP_BLOCK pixels, waves of 64 = one ground-truth word), so
// the counting can be checked (and sanitized) without a GPU.
//
// A pixel of category c with merged value m falls into bin b = #{k : m >= cuts[k]}, 0 <= b <= K.  With
// non-decreasing cuts "the pixel counts at threshold k" is b > k, so the per-threshold pixel counts are
// suffix sums of the bins.  hist[c][g][b] counts the pixels of bin b whose ground-truth bit is g.
//
// Folding: per wave and bin one 64-bit selection mask (the ballot of "this lane is in bin b"), split by the
// ground-truth word into two popcounts; the waves add them into the workgroup's [2][K + 1] integers, the
// workgroup adds its non-zero entries into hist.  Integer additions only: the result does not depend on
// their order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SWEEP_HD __host__ __device__ __forceinline__
#else
#define SWEEP_HD inline
#endif

#define SWEEP_MAX_K 64     // cuts per call
#define SWEEP_BLOCK 1024   // pixels (threads) per workgroup: 16 waves = 16 words

SWEEP_HD int sweep_popc(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(w);
#else
  return __builtin_popcountll(w);
#endif
}

// b = #{k : m >= cuts[k]}; a NaN m (or cut) compares false.  K <= SWEEP_MAX_K steps.
SWEEP_HD int sweep_bin(float m, const float* cuts, int K) {
  int b = 0;
  for (int k = 0; k < K; ++k) b += m >= cuts[k] ? 1 : 0;
  return b;
}

// the bits of word `wi` that are pixels of a mask of n pixels (as rle_valid)
SWEEP_HD uint64_t sweep_valid(int wi, int n) {
  const int left = n - wi * 64;
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}

// one wave's pixels of one bin, split by the ground truth: sel = the lanes (bits) of the bin, already limited
// to the word's valid pixels, so whatever gt holds past H W is not counted
struct SweepPair {
  int bg, fg;
};
SWEEP_HD SweepPair sweep_word_counts(uint64_t sel, uint64_t gt) {
  SweepPair p = {sweep_popc(sel & ~gt), sweep_popc(sel & gt)};
  return p;
}

// add a wave's pair into the workgroup's counts blk[2][K + 1] (LDS on the device: several waves add at once)
SWEEP_HD void sweep_block_add(int* blk, int K, int b, SweepPair p) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (p.bg) atomicAdd(blk + b, p.bg);
  if (p.fg) atomicAdd(blk + (K + 1) + b, p.fg);
#else
  blk[b] += p.bg;
  blk[(K + 1) + b] += p.fg;
#endif
}

// "thread" tid of nthreads moves its share of the workgroup's counts into hist_c[2][K + 1] and clears them
// for the next category
SWEEP_HD void sweep_block_flush(int* hist_c, int* blk, int K, int tid, int nthreads) {
  for (int i = tid; i < 2 * (K + 1); i += nthreads) {
    const int v = blk[i];
    if (v) {
#if defined(__HIP_DEVICE_COMPILE__)
      atomicAdd(hist_c + i, v);
#else
      hist_c[i] += v;
#endif
      blk[i] = 0;
    }
  }
}
