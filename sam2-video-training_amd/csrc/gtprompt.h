// Prompt generation from ground truth (gtprompt.hip): the per-pixel logic of the RLE decoder, the rectangular
// morphology, the component listing and the rank selection as plain functions that compile for the device
// and for the host.  gtprompt_host_check.cpp runs the same functions sequentially in the kernels'
// decomposition (groups of 64 pixels, chunks of GP_CHUNK), so the logic can be checked (and sanitized) without
// a GPU.  Integer arithmetic only; every loop below has a bound that does not depend on the data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GP_HD __host__ __device__ __forceinline__
#else
#define GP_HD inline
#endif

#define GP_WAVE 64
#define GP_BLOCK 256
#define GP_MAX_PIXELS (1 << 24)  // per image, as for s2h_cc_label
#define GP_MAX_REACH 32          // a window reaches at most this far to either side
#define GP_STATS 9               // int64 per kept component: label, area, xmin, ymin, xmax, ymax, n_sel, sum x, sum y
#define GP_MAX_INDEX 255         // kept components per image the uint8 index image can name
#define GP_TILES 16              // rank selection: a chunk is GP_TILES tiles of GP_BLOCK pixels
#define GP_CHUNK (GP_TILES * GP_BLOCK)

// COCO RLE: ends[0 .. n) are the ascending cumulative sums of one annotation's counts.  -> the index k of
// the first ends[k] > pos, n when there is none; the pixel at column-major position pos is k & 1.
// Binary search: the interval halves every step, 32 steps cover any n < 2^31.
GP_HD int gp_run_index(const int* ends, int n, int pos) {
  int lo = 0, hi = n;  // the answer is in [lo, hi]
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ends[mid] > pos)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// One line of a separable rectangular dilation (op 0: OR) or erosion (op 1: AND): the taps p + d of a line
// of n elements `stride` apart, d in [lo, hi], restricted to 0 <= p + d < n.  lo <= 0 <= hi, so the tap d = 0
// is always inside.  At most hi - lo + 1 <= 2 GP_MAX_REACH + 1 steps.
GP_HD uint8_t gp_morph_line(const uint8_t* line, int n, int64_t stride, int p, int lo, int hi, int op) {
  const int a = p + lo < 0 ? 0 : p + lo;
  const int b = p + hi > n - 1 ? n - 1 : p + hi;
  bool acc = op != 0;
  for (int t = a; t <= b; ++t) {
    const bool v = line[(int64_t)t * stride] != 0;
    acc = op ? (acc && v) : (acc || v);
  }
  return acc ? 1 : 0;
}

// a kept component's root: pixel q of an image labelled by s2h_cc_label (labels = 1 + root index)
GP_HD bool gp_kept_root(int label, int area, int q, int min_area) { return label == q + 1 && area >= min_area; }

// the pixels a rank-select query counts: in (neg 0) or out of (neg 1) the component, and on the grid
GP_HD bool gp_selected(int label, int q_label, int neg, const uint8_t* grid, int q) {
  return ((label == q_label) != (neg != 0)) && (!grid || grid[q] != 0);
}

// bits of m below lane
GP_HD uint64_t gp_below(uint64_t m, int lane) { return m & ((1ull << lane) - 1ull); }

GP_HD int gp_popc(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}
