// Index arithmetic of the dataset-preparation kernels (dataprep.hip) as plain functions that compile for the
// device and for the host: dataprep_host_check.cpp replays the kernels' decomposition with the very same
// functions, one workgroup and one lane after the other, so every tile and word index can be checked (and
// sanitized) without a GPU.
//
// A label image is [H, W] uint8, row-major.  A plane is the bit mask `label == class` (or `label != 0` for
// class -1) in the layout of rle_scan.h: bit j % 64 of word j / 64 is pixel (y = j % H, x = j / H),
// ceil(H W / 64) words, bits past H W zero.
//
// s2h_label_planes, staged form: a workgroup takes one frame and a band of DP_BAND = 64 columns.  The band's
// column-major positions start at 64 b H, a multiple of 64, so band b owns the words [b H, b H + words of the
// band): H whole words for a full band, ceil(cols H / 64) for the last one, whose last word is the plane's
// last.  No word is shared between workgroups.  The band's H x 64 bytes are staged in LDS as H rows of 16
// dwords; dword d of row r sits at r * 16 + (d ^ ((r >> 1) & 15)).  The word-building reads walk down a column
// (lane l = row r0 + l, one byte each): within 32 consecutive rows (r & 1, (r >> 1) & 15) takes 32 different
// values, so the 32 lanes of a half wave hit 32 different banks of the byte read's 32-bank rule.  The swizzle
// does what a padded row stride of 17 dwords would, in 64 instead of 68 bytes per row: 64 KB at H = 1024.
// Taller images than DP_STAGED_MAX_H take the direct form: one lane per column-major position, reading global
// memory (mask_export_kernel's mapping).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

#define DP_MAX_PIXELS (1 << 24)  // per image, as for s2h_rle_decode and s2h_rle_transitions
#define DP_BAND 64               // columns per workgroup of the staged form
#define DP_ROW_DWORDS 16         // a tile row: DP_BAND bytes
#define DP_STAGED_MAX_H 2048     // 128 KB of the 160 KB of LDS; taller images take the direct form
#define DP_BLOCK 256             // threads per workgroup of all three kernels
#define DP_HIST_LANE_BYTES 16    // consecutive bytes per lane and step of the histogram
#define DP_HIST_STEPS 4
#define DP_HIST_CHUNK (DP_BLOCK * DP_HIST_LANE_BYTES * DP_HIST_STEPS)  // bytes of one frame per workgroup

// total elements N * H * W, or -1 outside the limits (those of gp_total in gtprompt.hip)
DP_HD int64_t dp_total(int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1 || (int64_t)H * W > DP_MAX_PIXELS) return -1;
  const int64_t t = (int64_t)N * H * W;
  return t + 256 > 0x7fffffffLL ? -1 : t;
}

DP_HD int dp_words(int H, int W) { return (H * W + 63) / 64; }
DP_HD int dp_bands(int W) { return (W + DP_BAND - 1) / DP_BAND; }
DP_HD int dp_band_cols(int b, int W) {
  const int left = W - b * DP_BAND;
  return left >= DP_BAND ? DP_BAND : left;
}
DP_HD int dp_band_word0(int b, int H) { return b * H; }
DP_HD int dp_band_words(int b, int H, int W) { return (dp_band_cols(b, W) * H + 63) / 64; }
DP_HD bool dp_staged(int H) { return H <= DP_STAGED_MAX_H; }
DP_HD int dp_tile_dwords(int H) { return H * DP_ROW_DWORDS; }

// the tile's dword that holds columns 4 d .. 4 d + 3 of row r (0 <= d < 16), and the byte of column c
DP_HD int dp_tile_dword(int r, int d) { return r * DP_ROW_DWORDS + (d ^ ((r >> 1) & (DP_ROW_DWORDS - 1))); }
DP_HD int dp_tile_byte(int r, int c) { return dp_tile_dword(r, c >> 2) * 4 + (c & 3); }

// loading: item i of a band (0 <= i < 4 H) is the 16-byte segment `seg` of row `row`
DP_HD void dp_load_item(int i, int* row, int* seg) {
  *row = i >> 2;
  *seg = i & 3;
}

// lane `lane` of band word w (0 <= w < dp_band_words): the band-local position p = 64 w + lane is pixel
// (row p % H, band column p / H); false past the band's last pixel (the tail of the last word)
DP_HD bool dp_word_pos(int w, int lane, int H, int cols, int* row, int* col) {
  const int p = w * 64 + lane;
  if (p >= cols * H) return false;
  *col = p / H;
  *row = p - *col * H;
  return true;
}

// the plane bit of label byte v: class -1 = any nonzero byte
DP_HD bool dp_bit(int v, int cls) { return cls == -1 ? v != 0 : v == cls; }

// the planes of frame f, cut to [0, P): whatever frame_off holds, no plane outside the buffer is written
DP_HD void dp_frame_planes(const int* frame_off, int f, int P, int* p0, int* p1) {
  const int a = frame_off[f], b = frame_off[f + 1];
  *p0 = a < 0 ? 0 : a;
  *p1 = b > P ? P : b;
}

// histogram: workgroup chunk c of a frame covers bytes [c * DP_HIST_CHUNK, ...) of its H W; lane t's step s
// covers DP_HIST_LANE_BYTES bytes from the returned offset (which may lie at or past H W: nothing to do)
DP_HD int dp_hist_chunks(int HW) { return (HW + DP_HIST_CHUNK - 1) / DP_HIST_CHUNK; }
DP_HD int dp_hist_offset(int c, int s, int t) {
  return c * DP_HIST_CHUNK + (s * DP_BLOCK + t) * DP_HIST_LANE_BYTES;
}
