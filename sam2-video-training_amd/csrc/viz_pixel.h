// The training visualisation's picture in one place (s2h_viz_pack / s2h_viz_compose, viz.hip): one pixel of
// the packed category words and one pixel of the 2 x 2 composite.  Plain functions that compile for the device
// and for the host: viz_host_check.cpp runs them pixel after pixel, tests/viz_cases.py states the same picture
// independently in numpy / scipy.  Everything but the frame conversion is integer arithmetic.
//
// Composite of frame i, uint8 [2H, 2W, 3] (the reference's 2 x 2 order, utils/viz.py:92-235, no text):
//   top-left     frame i                      top-right     frame i + ground-truth overlay
//   bottom-left  frame 0 + prompts            bottom-right  frame i + prediction overlay
// Frame to uint8 (viz.py:46-54): u = trunc(min(max((double)x * std_c + mean_c, 0), 1) * 255), the product and
//   the sum rounded separately (numpy's float64 result); NaN gives 0.  uint8 RGB frames pass through.
// Mask bits: category c is set where its value is > 0.5 -- the reference's rule for the ground truth and for the
//   raw logits alike (`mask_array[c] > 0.5`); a uint8 / bool source is set where it is non-zero.
// Overlay panel: overlay = the colour of the highest set category (later categories overwrite in viz.py:104-109)
//   or 0; every pixel is out = (4 base + overlay + 2) / 5, cv2.addWeighted(base, 0.8, overlay, 0.2) -- pixels
//   without a mask are darkened too.  Then the contour band at full opacity: category c is on the band at p when
//   the 3 x 3 neighbourhood of p (positions outside the image ignored) holds both a pixel with c set and one
//   with c clear, OR(neigh) & ~AND(neigh) on the words; the highest band category gives the colour.
// Prompt panel: frame 0, then the markers in table order (later ones overwrite), clipped to the image; with a
//   mask prompt no markers but the overlay panel of the prompt words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VZ_HD __host__ __device__ __forceinline__
#else
#define VZ_HD inline
#endif

#define VZ_MAX_CAT 64
#define VZ_MAX_MARKERS 256
#define VZ_MARKER_INTS 8  // kind, x1, y1, x2, y2, r, g, b
enum VizMarker { VZ_DISC = 0, VZ_CROSS = 1, VZ_BOX = 2 };
enum VizImage { VZ_IMG_F32_CHW = 0, VZ_IMG_U8_HWC = 1 };
enum VizMask { VZ_MASK_U8 = 0, VZ_MASK_F32 = 1 };

// total bytes of n composites, or -1 beyond the limits (1 <= H, W; 1 <= C <= 64; n >= 0; n 2H 2W 3 < 2^31)
VZ_HD int64_t vz_out_bytes(int n, int C, int H, int W) {
  if (n < 0 || C < 1 || C > VZ_MAX_CAT || H < 1 || W < 1) return -1;
  const int64_t b = (int64_t)n * 12;
  if ((int64_t)H * W > 0x7FFFFFFFll / 12) return -1;
  const int64_t t = b * H * W;
  return t < 0x80000000ll ? t : -1;
}

// a * b rounded once to double where the result feeds an addition (hipcc's -ffp-contract=fast fuses in the
// backend even across __dmul_rn; the empty asm hides the product from it, as oe_mul_rn does.  Host builds add
// -ffp-contract=off)
VZ_HD double vz_mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __dmul_rn(a, b);
  asm("" : "+v"(r));
  return r;
#else
  return a * b;
#endif
}

// channel c of a normalised frame value -> uint8 (ImageNet mean / std as doubles, viz.py:48-54)
VZ_HD int vz_frame_u8(float x, int c) {
  const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406);
  const double std_ = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
  double v = vz_mul_rn((double)x, std_) + mean;
  v = v > 0.0 ? (v > 1.0 ? 1.0 : v) : 0.0;  // (NaN compares false: 0)
  return (int)(v * 255.0);
}

// r | g << 8 | b << 16 of pixel (y, x) of one frame
VZ_HD uint32_t vz_base(int kind, const void* frame, int H, int W, int y, int x) {
  const int64_t p = (int64_t)y * W + x;
  if (kind == VZ_IMG_U8_HWC) {
    const uint8_t* s = (const uint8_t*)frame + p * 3;
    return (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
  }
  const float* s = (const float*)frame;
  const int64_t hw = (int64_t)H * W;
  return (uint32_t)vz_frame_u8(s[p], 0) | (uint32_t)vz_frame_u8(s[hw + p], 1) << 8 |
         (uint32_t)vz_frame_u8(s[2 * hw + p], 2) << 16;
}

// the category word of pixel p of one frame: bit c = (mask[c][p] > 0.5); mask [C, H W] of the frame
VZ_HD uint64_t vz_pack(int kind, const void* mask, int C, int64_t hw, int64_t p) {
  uint64_t w = 0;
  if (kind == VZ_MASK_F32) {
    const float* s = (const float*)mask + p;
    for (int c = 0; c < C; ++c) w |= (uint64_t)(s[c * hw] > 0.5f) << c;
  } else {
    const uint8_t* s = (const uint8_t*)mask + p;
    for (int c = 0; c < C; ++c) w |= (uint64_t)(s[c * hw] != 0) << c;
  }
  return w;
}

VZ_HD int vz_top(uint64_t w) {  // index of the highest set bit, w != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)w);
#else
  return 63 - __builtin_clzll(w);
#endif
}

VZ_HD uint32_t vz_color(const uint8_t* palette, int c) {
  return (uint32_t)palette[3 * c] | (uint32_t)palette[3 * c + 1] << 8 | (uint32_t)palette[3 * c + 2] << 16;
}

VZ_HD uint32_t vz_blend(uint32_t base, uint32_t over) {  // per channel (4 base + overlay + 2) / 5
  uint32_t out = 0;
  for (int k = 0; k < 24; k += 8) out |= ((4u * ((base >> k) & 255u) + ((over >> k) & 255u) + 2u) / 5u) << k;
  return out;
}

// one pixel of an overlay panel; words [H W] = the category words of the panel's frame
VZ_HD uint32_t vz_overlay_pixel(uint32_t base, const uint64_t* words, const uint8_t* palette, int H, int W, int y,
                                int x) {
  uint64_t any = 0, all = ~0ull;
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W) continue;
      const uint64_t w = words[(int64_t)yy * W + xx];
      any |= w;
      all &= w;
    }
  }
  const uint64_t band = any & ~all;
  if (band) return vz_color(palette, vz_top(band));
  const uint64_t w = words[(int64_t)y * W + x];
  return vz_blend(base, w ? vz_color(palette, vz_top(w)) : 0u);
}

// marker m (VZ_MARKER_INTS int32) at pixel (y, x): true and its colour where it paints.
//   disc (label 1, cv2.circle radius 8 filled + a white ring): colour where dx^2 + dy^2 < 49, white where
//     49 <= dx^2 + dy^2 <= 81;
//   cross (label 0, drawMarker size 16 thickness 3): (|dx| <= 1 and |dy| <= 8) or (|dy| <= 1 and |dx| <= 8);
//   box (labels 2 / 3, rectangle thickness 2): x1 <= x <= x2, y1 <= y <= y2 and fewer than 2 pixels from one of
//     the four sides (min(x - x1, x2 - x, y - y1, y2 - y) < 2); an inverted box has no such pixel.
VZ_HD bool vz_marker(const int* m, int y, int x, uint32_t* rgb) {
  const uint32_t col = (uint32_t)(m[5] & 255) | (uint32_t)(m[6] & 255) << 8 | (uint32_t)(m[7] & 255) << 16;
  const int64_t dx = (int64_t)x - m[1], dy = (int64_t)y - m[2];
  if (m[0] == VZ_BOX) {
    const int64_t ex = (int64_t)m[3] - x, ey = (int64_t)m[4] - y;
    if (dx < 0 || dy < 0 || ex < 0 || ey < 0) return false;
    if (dx >= 2 && dy >= 2 && ex >= 2 && ey >= 2) return false;
    *rgb = col;
    return true;
  }
  const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  if (ax > 9 || ay > 9) return false;
  if (m[0] == VZ_DISC) {
    const int64_t d2 = ax * ax + ay * ay;
    if (d2 > 81) return false;
    *rgb = d2 < 49 ? col : 0xFFFFFFu;
    return true;
  }
  if (m[0] == VZ_CROSS && ((ax <= 1 && ay <= 8) || (ay <= 1 && ax <= 8))) {
    *rgb = col;
    return true;
  }
  return false;
}

struct VizArgs {
  int n, H, W;
  int img_kind;
  const void* frames;    // frame f at frames + f * frame_stride elements (float or byte)
  int64_t frame_stride;
  const void* frame0;    // the prompt panel's frame, same kind
  const uint64_t* gt;    // [n, H W]
  const uint64_t* pred;  // [n, H W]
  const uint64_t* prompt;  // [H W] (mask prompts) or null (markers)
  const uint8_t* palette;  // [C, 3]
  int M;
  const int* markers;  // [M, VZ_MARKER_INTS]
};

// pixel (Y, X) of composite f, 0 <= Y < 2H, 0 <= X < 2W
VZ_HD uint32_t vz_composite_pixel(const VizArgs& a, int f, int Y, int X) {
  const int H = a.H, W = a.W;
  const bool bottom = Y >= H, right = X >= W;
  const int y = bottom ? Y - H : Y, x = right ? X - W : X;
  const int64_t hw = (int64_t)H * W;
  if (bottom && !right) {
    const uint32_t base = vz_base(a.img_kind, a.frame0, H, W, y, x);
    if (a.prompt) return vz_overlay_pixel(base, a.prompt, a.palette, H, W, y, x);
    uint32_t out = base;
    for (int m = 0; m < a.M; ++m) vz_marker(a.markers + m * VZ_MARKER_INTS, y, x, &out);
    return out;
  }
  const int64_t esz = a.img_kind == VZ_IMG_U8_HWC ? 1 : 4;
  const uint32_t base = vz_base(a.img_kind, (const uint8_t*)a.frames + (int64_t)f * a.frame_stride * esz, H, W, y, x);
  if (!bottom && !right) return base;
  return vz_overlay_pixel(base, (bottom ? a.pred : a.gt) + (int64_t)f * hw, a.palette, H, W, y, x);
}

// the three dwords of four consecutive pixels (12 bytes of the flat output)
VZ_HD void vz_pack4(const uint32_t* px, uint32_t* d) {
  d[0] = px[0] | px[1] << 24;
  d[1] = px[1] >> 8 | px[2] << 16;
  d[2] = px[2] >> 16 | px[3] << 8;
}
