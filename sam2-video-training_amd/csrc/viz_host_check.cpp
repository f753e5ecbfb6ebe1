// Stand-alone host run of the visualisation picture (viz_pixel.h): the two launches of viz.hip in the same
// order, one pixel after the other instead of one lane per pixel (pack) or per four pixels (compose), over cases
// read from a file.  Built with plain g++ -ffp-contract=off (tests/test_viz_host.py; add
// -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   viz_host_check IN OUT
// IN: a sequence of cases, each 10 int32 {n, C, H, W, img_kind, gt_kind, pred_kind, prompt_kind (-1 = markers),
//     M, step} followed by
//       frames   ((n - 1) step + 1) frames of 3 H W float32 (img_kind 0) or H W 3 bytes (1); frame f of the case is
//                stored frame f * step (a frame stride of step frames),
//       frame0   one frame of the same kind,
//       gt       ((n - 1) step + 1) x C x H x W bytes (kind 0) or float32 (kind 1), pred the same in its kind,
//       prompt   C x H x W in its kind when prompt_kind >= 0,
//       palette  C x 3 bytes, markers M x 8 int32.
// OUT gets n x 2H x 2W x 3 bytes per case.  Sizes beyond the limits of s2h_viz_compose end the run with status 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "viz_pixel.h"

static bool rd(FILE* in, std::vector<uint8_t>& v, int64_t bytes) {
  v.resize((size_t)bytes + 8);  // (8 spare bytes keep data() aligned and non-null for an empty block)
  return fread(v.data(), 1, (size_t)bytes, in) == (size_t)bytes;
}

static void pack(int n, int C, int64_t hw, int kind, const std::vector<uint8_t>& src, int64_t stride_elems,
                 std::vector<uint64_t>& words) {
  const int64_t esz = kind == VZ_MASK_F32 ? 4 : 1;
  words.resize((size_t)(n * hw));
  for (int64_t i = 0; i < n * hw; ++i) {
    const int64_t f = i / hw, p = i - f * hw;
    words[(size_t)i] = vz_pack(kind, src.data() + f * stride_elems * esz, C, hw, p);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int h[10];
  while (fread(h, sizeof(int), 10, in) == 10) {
    const int n = h[0], C = h[1], H = h[2], W = h[3], img_kind = h[4], gt_kind = h[5], pred_kind = h[6];
    const int prompt_kind = h[7], M = h[8], step = h[9];
    const int64_t bytes = vz_out_bytes(n, C, H, W);
    if (bytes < 0 || n < 1 || M < 0 || M > VZ_MAX_MARKERS || step < 1 || step > 16 || (img_kind | 1) != 1 ||
        (gt_kind | 1) != 1 || (pred_kind | 1) != 1 || prompt_kind < -1 || prompt_kind > 1)
      return 3;
    const int64_t hw = (int64_t)H * W, stored = (int64_t)(n - 1) * step + 1;
    const int64_t fbytes = 3 * hw * (img_kind == VZ_IMG_U8_HWC ? 1 : 4);
    std::vector<uint8_t> frames, frame0, gt, pred, prompt, palette, markers;
    if (!rd(in, frames, stored * fbytes) || !rd(in, frame0, fbytes) ||
        !rd(in, gt, stored * C * hw * (gt_kind ? 4 : 1)) || !rd(in, pred, stored * C * hw * (pred_kind ? 4 : 1)) ||
        (prompt_kind >= 0 && !rd(in, prompt, C * hw * (prompt_kind ? 4 : 1))) || !rd(in, palette, 3 * C) ||
        !rd(in, markers, (int64_t)M * VZ_MARKER_INTS * 4))
      return 3;
    std::vector<uint64_t> gw, pw, qw;
    pack(n, C, hw, gt_kind, gt, step * C * hw, gw);
    pack(n, C, hw, pred_kind, pred, step * C * hw, pw);
    if (prompt_kind >= 0) pack(1, C, hw, prompt_kind, prompt, 0, qw);
    VizArgs a;
    a.n = n, a.H = H, a.W = W, a.img_kind = img_kind, a.frames = frames.data(), a.frame_stride = step * 3 * hw;
    a.frame0 = frame0.data(), a.gt = gw.data(), a.pred = pw.data(), a.prompt = prompt_kind >= 0 ? qw.data() : nullptr;
    a.palette = palette.data(), a.M = prompt_kind >= 0 ? 0 : M, a.markers = (const int*)markers.data();
    std::vector<uint32_t> o((size_t)(bytes / 4));
    const int W2 = 2 * W;
    const int64_t per = 4 * hw;
    for (int64_t q = 0; q < (int64_t)n * hw; ++q) {  // viz_compose_kernel, lane q
      uint32_t px[4];
      for (int k = 0; k < 4; ++k) {
        const int64_t i = 4 * q + k;
        const int f = (int)(i / per);
        const int64_t r = i - (int64_t)f * per;
        const int Y = (int)(r / W2);
        px[k] = vz_composite_pixel(a, f, Y, (int)(r - (int64_t)Y * W2));
      }
      vz_pack4(px, &o[(size_t)(3 * q)]);
    }
    if (fwrite(o.data(), 1, (size_t)bytes, out) != (size_t)bytes) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
