// Clip loading on the device (preproc.hip): the per-element code of Pillow's fixed-point resample on uint8
// pixels and of the category masks read straight from COCO RLE run boundaries, as plain functions that compile
// for the device and for the host.  preproc_host_check.cpp runs them sequentially in the kernels'
// decomposition (one output element per thread), so the logic can be checked (and sanitized) without a GPU.
// Integer arithmetic only; every loop below is bounded by a table size, never by the data.
#pragma once
#include <stdint.h>

#include "gtprompt.h"  // gp_run_index: the run search s2h_rle_decode uses

#define RS_HD GP_HD
#define RS_BITS 22      // Pillow's PRECISION_BITS (32 - 8 - 2): coefficients are weights * 2^22
#define RS_MAX_TAPS 64  // taps per output sample (a bicubic down-scale by 15 still fits)
#define RS_MAX_SIDE 16384
#define RS_MAX_CATS 64  // categories: one bit each of the per-pixel set

// Pillow's clip8 of an accumulator that already holds the rounding term 1 << 21
RS_HD uint8_t rs_clip8(int acc) {
  const int v = acc >> RS_BITS;  // arithmetic shift, as Pillow's table lookup of in >> PRECISION_BITS
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// the tap window [lo, lo + n) of one output sample, restricted to the line [0, len) and to `ksize` taps: tables
// built by ops.resample_taps are inside already, a damaged table reads nothing outside the line
RS_HD int rs_window(int lo, int cnt, int ksize, int len, int* first) {
  int n = cnt < ksize ? cnt : ksize;
  if (n > RS_MAX_TAPS) n = RS_MAX_TAPS;
  int skip = lo < 0 ? -lo : 0;  // taps cut off in front
  if (skip > n) skip = n;
  const int a = lo + skip;      // >= 0 unless n == 0
  int m = n - skip;
  if (m > 0 && a > len - m) m = a < len ? len - a : 0;
  *first = skip;
  return m < 0 ? 0 : m;
}

// one output sample: px[(lo + k) * stride] weighted by coef[k], k in [0, cnt), rounded and clipped as Pillow's
// ImagingResampleHorizontal_8bpc / Vertical_8bpc do (int32 accumulator starting at 1 << 21)
RS_HD uint8_t rs_sample(const uint8_t* px, int64_t stride, int len, int lo, int cnt, const int* coef, int ksize) {
  int first;
  const int n = rs_window(lo, cnt, ksize, len, &first);
  int acc = 1 << (RS_BITS - 1);
  for (int k = 0; k < n; ++k) acc += (int)px[(int64_t)(lo + first + k) * stride] * coef[first + k];
  return rs_clip8(acc);
}

// the categories (bit n = category n) that cover the column-major position `pos` among the annotations
// [a0, a1) of one frame: annotation a is set there when the number of its run ends <= pos is odd
RS_HD uint64_t rs_cat_set(const int* run_off, const int* run_end, const int* ann_cat, int a0, int a1, int ncat,
                          int pos) {
  uint64_t set = 0;
  for (int a = a0; a < a1; ++a) {
    const int c = ann_cat[a];
    if (c < 0 || c >= ncat) continue;
    const int o = run_off[a], n = run_off[a + 1] - o;
    if (gp_run_index(run_end + o, n < 0 ? 0 : n, pos) & 1) set |= 1ull << c;
  }
  return set;
}
