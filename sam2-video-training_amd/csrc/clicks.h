// Correction clicks from the error between ground truth and prediction (clicks.hip; reference
// sam2_video/model/modeling/sam2_utils.py:202-323): the exact squared Euclidean distance transform, the argmax
// key of the centre click and the rank of the uniform click as plain functions that compile for the device and
// for the host.  clicks_host_check.cpp runs the same functions sequentially in the kernels' decomposition (words
// of 64 pixels, blocks of 256, chunks of GP_CHUNK), so the logic can be checked (and sanitized) without a GPU.
// Integer arithmetic only; every loop below has a bound that does not depend on the data.
//
// D2(m)(y, x) = 0 where m is clear, else the minimum of (y - y')^2 + (x - x')^2 over the (y', x') in
// [-1, H] x [-1, W] that lie outside the image or where m is clear.  Separable: with h(y', x) the distance
// along row y' from x to the nearest clear position (-1 and W count as clear; 0 when (y', x) itself is clear,
// and on the rows -1 and H), D2(y, x) = min over y' of (y - y')^2 + h(y', x)^2.
#pragma once
#include "gtprompt.h"

#define CK_MAX_SIDE 4092   // H, W <= this: D2 <= (min(H, W) / 2 + 1)^2 < 2^22, where float32 sqrt is strictly increasing
#define CK_MAX_WORDS 64    // 64-pixel words per row: ceil(CK_MAX_SIDE / 64)
#define CK_TAG 0x8000      // the stored row distance of a pixel of the second region (FP) carries this bit
#define CK_HMASK 0x7fff    // h <= CK_MAX_SIDE / 2 + 1 fits below it

// the two error regions of a pixel: missed (FN, label 1) and wrongly predicted (FP, label 0)
GP_HD bool ck_fn(bool g, bool p) { return g && !p; }
GP_HD bool ck_fp(bool g, bool p) { return !g && p; }
// the pixels the uniform click draws from: the errors, or the background when there is no error at all
GP_HD bool ck_union(bool g, bool p, bool all_correct) { return all_correct ? !g : g != p; }

GP_HD int ck_clz(uint64_t m) { return __builtin_clzll(m); }  // m != 0
GP_HD int ck_ctz(uint64_t m) { return __builtin_ctzll(m); }  // m != 0

// set bits of a word counted down from bit 63 / up from bit 0 until the first clear one (64: all set)
GP_HD int ck_lead_ones(uint64_t word) { return ~word == 0 ? 64 : ck_clz(~word); }
GP_HD int ck_trail_ones(uint64_t word) { return ~word == 0 ? 64 : ck_ctz(~word); }

// The carries of one row of nw <= CK_MAX_WORDS region words (bit l of word w = pixel 64 w + l; bits past W are
// clear): run_l[w] = the set pixels that end right before word w, run_r[w] = those that start right after it.
// nw steps each.
GP_HD void ck_row_carry_left(const uint64_t* words, int nw, int* run_l) {
  int run = 0;
  for (int w = 0; w < nw; ++w) {
    run_l[w] = run;
    const int lead = ck_lead_ones(words[w]);
    run = lead == 64 ? run + 64 : lead;
  }
}
GP_HD void ck_row_carry_right(const uint64_t* words, int nw, int* run_r) {
  int run = 0;
  for (int w = nw - 1; w >= 0; --w) {
    run_r[w] = run;
    const int trail = ck_trail_ones(words[w]);
    run = trail == 64 ? run + 64 : trail;
  }
}

// h of the pixel at bit `lane` of `word`: the nearest clear position to the left is inside the word (the
// highest clear bit below the lane) or run_l pixels before it, to the right likewise; 0 for a clear pixel
GP_HD int ck_row_dist(uint64_t word, int lane, int run_l, int run_r) {
  if (!((word >> lane) & 1ull)) return 0;
  const uint64_t inv = ~word;
  const uint64_t lo = inv & ((2ull << lane) - 1ull);  // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
  const uint64_t hi = inv >> lane;
  const int dl = lo ? lane - (63 - ck_clz(lo)) : lane + 1 + run_l;
  const int dr = hi ? ck_ctz(hi) : 64 - lane + run_r;
  return dl < dr ? dl : dr;
}

// what the row pass stores per pixel: h, tagged with the region (0: the mask or FN, 1: FP; a pixel is in at
// most one of the two)
GP_HD uint16_t ck_pack(int h_first, int h_second) {
  return (uint16_t)(h_first ? h_first : (h_second ? (h_second | CK_TAG) : 0));
}

// D2 of pixel (y, x) in its own region from the stored row distances hp [H, W] of its image: rows y - d and
// y + d for d = 1, 2, ... while d^2 can still improve; a row whose pixel lies in the other region, or outside
// the image, contributes d^2.  *tag = the pixel's region bit.  Row -1 or row H is reached after at most
// min(y + 1, H - y) steps and ends the loop, so no row beyond them is read; at most H steps.
GP_HD int ck_col_d2(const uint16_t* hp, int H, int W, int y, int x, int* tag) {
  const int v = hp[(int64_t)y * W + x];
  const int h = v & CK_HMASK, t = v & CK_TAG;
  *tag = t ? 1 : 0;
  if (h == 0) return 0;
  int best = h * h;
  for (int d = 1; d <= H; ++d) {
    const int dd = d * d;
    if (dd >= best) break;
    int up = 0, dn = 0;
    if (y - d >= 0) {
      const int u = hp[(int64_t)(y - d) * W + x];
      up = (u & CK_TAG) == t ? (u & CK_HMASK) : 0;
    }
    if (y + d < H) {
      const int u = hp[(int64_t)(y + d) * W + x];
      dn = (u & CK_TAG) == t ? (u & CK_HMASK) : 0;
    }
    const int m = up < dn ? up : dn;
    if (dd + m * m < best) best = dd + m * m;
  }
  return best;
}

// argmax with the first index winning a tie = max over this key
GP_HD uint64_t ck_key(int d2, int idx) { return ((uint64_t)(uint32_t)d2 << 32) | (0xFFFFFFFFull - (uint32_t)idx); }
GP_HD int ck_key_d2(uint64_t key) { return (int)(key >> 32); }
GP_HD int ck_key_idx(uint64_t key) { return (int)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)); }

// the click of one object from the keys of its two regions: positive only when FN's maximum is strictly larger
GP_HD void ck_center_click(uint64_t key_fn, uint64_t key_fp, int W, float* point, int* label, int* dmax) {
  const int dn = ck_key_d2(key_fn), dp = ck_key_d2(key_fp);
  const int pos = dn > dp;
  const int idx = pos ? ck_key_idx(key_fn) : ck_key_idx(key_fp);
  point[0] = (float)(idx % W);
  point[1] = (float)(idx / W);
  *label = pos;
  dmax[0] = dn;
  dmax[1] = dp;
}

// the rank a 32-bit draw r picks among n <= 2^24 pixels: floor(r n / 2^32) < n
GP_HD int ck_rank(int64_t r, int n) { return (int)((((uint64_t)r & 0xFFFFFFFFull) * (uint64_t)n) >> 32); }
