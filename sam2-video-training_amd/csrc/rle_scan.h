// Word-level logic of the run-boundary extraction (rle.hip) as plain functions that compile for the device
// and for the host: rle_host_check.cpp runs the very same functions sequentially over the same blocks of
// words, so the transition logic can be checked (and sanitized) without a GPU.
//
// A mask of n = H * W pixels is bit-packed in column-major order: bit j % 64 of word j / 64 is pixel
// (y = j % H, x = j / H), ceil(n / 64) words.  A transition is a position j in [0, n) with m[j] != m[j - 1],
// m[-1] = 0: the COCO RLE run boundaries (counts = differences of [0, *transitions, n]).
//
// Loop bounds: rle_emit and rle_word_stats clear or skip at least one of a word's 64 bits per step.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RLE_HD __host__ __device__ __forceinline__
#else
#define RLE_HD inline
#endif

#define RLE_BLOCK_WORDS 256       // words per workgroup of the count and emit kernels, one per thread
#define RLE_MAX_PIXELS (1 << 24)  // per mask, as for s2h_cc_label
#define RLE_HDR 8                 // int32 per category: n_trans, offset, area, xmin, ymin, xmax, ymax, total needed

RLE_HD int rle_popc(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(w);
#else
  return __builtin_popcountll(w);
#endif
}
// index of the lowest / highest set bit of w != 0
RLE_HD int rle_low(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)w) - 1;
#else
  return __builtin_ctzll(w);
#endif
}
RLE_HD int rle_high(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)w);
#else
  return 63 - __builtin_clzll(w);
#endif
}

// bits lo .. hi - 1 of a word, 0 <= lo <= hi <= 64
RLE_HD uint64_t rle_span(int lo, int hi) {
  const uint64_t upto_hi = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
  const uint64_t upto_lo = lo >= 64 ? ~0ull : ((1ull << lo) - 1ull);
  return upto_hi & ~upto_lo;
}

// the bits of word `wi` that are pixels of a mask of n pixels (tail masking: the last word may be partial,
// and whatever its upper bits hold is not part of the mask)
RLE_HD uint64_t rle_valid(int wi, int n) {
  const int left = n - wi * 64;
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}

// transition mask of word w (already tail-masked): bit b set when pixel b differs from the pixel before it;
// carry = the last pixel of the previous word (0 for the first word)
RLE_HD uint64_t rle_transitions(uint64_t w, uint64_t carry, uint64_t valid) {
  return (w ^ ((w << 1) | (carry & 1ull))) & valid;
}

// write the positions base + b of the set bits b of t, ascending, to out[k], out[k + 1], ...; slots at or
// past cap are not written.  Returns the number of positions (written or not).
RLE_HD int rle_emit(uint64_t t, int base, int* out, int k, int cap) {
  int n = 0;
  while (t) {
    const int b = rle_low(t);
    t &= t - 1ull;
    if (k + n < cap) out[k + n] = base + b;
    ++n;
  }
  return n;
}

// area and the inclusive bounding box of a mask, folded over words: the neutral element is
// {0, W, H, -1, -1} (an empty mask keeps it)
struct RleStats {
  int area, xmin, ymin, xmax, ymax;
};
RLE_HD RleStats rle_stats_empty(int H, int W) {
  RleStats s = {0, W, H, -1, -1};
  return s;
}
RLE_HD RleStats rle_stats_join(RleStats a, RleStats b) {
  RleStats s = {a.area + b.area, a.xmin < b.xmin ? a.xmin : b.xmin, a.ymin < b.ymin ? a.ymin : b.ymin,
                a.xmax > b.xmax ? a.xmax : b.xmax, a.ymax > b.ymax ? a.ymax : b.ymax};
  return s;
}
// statistics of one tail-masked word whose bit 0 is column-major pixel `base`.  x = j / H rises with j, so
// the x range comes from the lowest and highest set bit; within one column y rises with j, so each column
// the word touches (at most 64) gives its y range from the lowest and highest set bit of its span.
RLE_HD RleStats rle_word_stats(uint64_t w, int base, int H, int W) {
  RleStats s = rle_stats_empty(H, W);
  if (!w) return s;
  s.area = rle_popc(w);
  s.xmin = (base + rle_low(w)) / H;
  s.xmax = (base + rle_high(w)) / H;
  for (int x = s.xmin; x <= s.xmax; ++x) {
    const int lo = x * H - base, hi = lo + H;  // the column's pixels, as bits of this word
    const uint64_t seg = w & rle_span(lo < 0 ? 0 : lo, hi > 64 ? 64 : hi);
    if (!seg) continue;
    const int y0 = base + rle_low(seg) - x * H, y1 = base + rle_high(seg) - x * H;
    if (y0 < s.ymin) s.ymin = y0;
    if (y1 > s.ymax) s.ymax = y1;
  }
  return s;
}
