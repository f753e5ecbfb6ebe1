// Union-find with min-index roots for 8-connected component labelling (cc.hip), as plain functions that
// compile for the device and for the host: cc_host_check.cpp runs the very same find / union / neighbour
// logic sequentially, so the labelling can be checked (and sanitized) without a GPU.
//
// State of one H x W image: L[p] = -1 off the foreground, else the parent of pixel p (row-major index
// within the image).  Invariant kept by every writer: L[p] <= p.  A pixel with L[p] == p is a root; links
// only ever point to smaller indices, so the root of a finished component is its smallest pixel index --
// the canonical label, independent of scheduling.
//
// Loop bounds.  Every step of cc_find moves to a strictly smaller index, and every failed round of
// cc_union replaces one of its two nodes by a strictly smaller one, so a + b falls with every step and a
// union of a, b < n ends within 2n steps; cc_find and cc_union share one budget of that size.  The loops
// also stop on any value that breaks the invariant: a corrupted array yields a wrong label, never a spin.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

#define CC_WAVE 64
#define CC_MAX_PIXELS (1 << 24)  // per image: 2n + 2 budget steps stay far inside int

// relaxed load / min of a parent slot.  Device: agent scope, so that the waves of every XCD see each
// other's links while the merge kernel runs (a plain load could be served from a stale L2 line).
CC_HD int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
CC_HD int cc_min(int* p, int v) {  // returns the old value
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}

// foreground test of a score: > 0, or its complement <= 0 (NaN is in neither, as on the host path)
CC_HD bool cc_fg(float s, int positive) { return positive ? s > 0.f : s <= 0.f; }

// First lane of the horizontal run that `lane` belongs to inside its group of 64 consecutive pixels.
// link has bit l set when pixel l is foreground and joined to pixel l - 1 of the same group (same row,
// both foreground); bit 0 is never set.  The run start is the highest lane <= `lane` whose bit is clear.
CC_HD int cc_run_start(uint64_t link, int lane) {
  const uint64_t upto = lane >= 63 ? ~0ull : ((2ull << lane) - 1ull);
  const uint64_t clear = ~link & upto;  // bit 0 is in it
  int hi = 0;
  for (int s = 32; s > 0; s >>= 1)  // floor(log2(clear)), branch-light and the same on host and device
    if (clear >> (hi + s)) hi += s;
  return hi;
}

// root of x; *budget counts the steps left (shared with cc_union)
CC_HD int cc_find(const int* L, int x, int* budget) {
  while (*budget > 0) {
    const int p = cc_load(L + x);
    if (p >= x || p < 0) break;  // root (or a broken invariant: stop here)
    x = p;
    --*budget;
  }
  return x;
}

// join the sets of a and b (foreground pixels of one image of n pixels); lock-free: the larger root is
// hung under the smaller with an atomic min, and when another thread re-parented it first (the old value
// differs), the union goes on with that thread's parent, so no link is lost
CC_HD void cc_union(int* L, int a, int b, int n) {
  int budget = 2 * n + 2;
  while (budget-- > 0) {
    a = cc_find(L, a, &budget);
    b = cc_find(L, b, &budget);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = cc_min(L + b, a);
    if (old == b) return;
    b = old;  // old < b
  }
}

// All the unions pixel (y, x) of a foreground image owes, after the run labelling gave every pixel the
// first pixel of its in-group run as parent.  wave_first: the pixel is lane 0 of its group, so the run
// labelling could not see its left neighbour.
//
// Up-row links are thinned to what connectivity needs.  With W = left, N / NW / NE = the three pixels above:
//   N set:    NW and NE sit in N's run; p links to N unless W is set (W then reaches N by its own rules)
//   N clear:  p links to NE always, and to NW unless W is set (NW is W's N)
// By induction along a run from its left end, every foreground pixel ends up in the set of each of its
// foreground upper neighbours.
CC_HD void cc_merge_pixel(int* L, int H, int W, int y, int x, bool wave_first) {
  const int n = H * W;
  const int p = y * W + x;
  const bool w = x > 0 && cc_load(L + p - 1) >= 0;
  if (w && wave_first) cc_union(L, p, p - 1, n);
  if (y == 0) return;
  const int up = p - W;
  const bool nn = cc_load(L + up) >= 0;
  if (nn) {
    if (!w) cc_union(L, p, up, n);
    return;
  }
  if (!w && x > 0 && cc_load(L + up - 1) >= 0) cc_union(L, p, up - 1, n);
  if (x + 1 < W && cc_load(L + up + 1) >= 0) cc_union(L, p, up + 1, n);
}
