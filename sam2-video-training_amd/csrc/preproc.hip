// Clip loading on the device: what data/dataset.py load_image / resize_mask and predictor._load_frames do on the
// host after the JPEG decode.  s2h_resample_u8_norm is Pillow's two-pass fixed-point resample of uint8 RGB
// frames (horizontal pass, rounded to uint8, then vertical pass) with the crop and the normalisation fused;
// s2h_rle_catmasks reads the nearest-resized, cropped category masks straight from the COCO RLE run
// boundaries.  Both reproduce the host tensors bit for bit: integer arithmetic, the float stage is a table.
//
// One thread per output element, neighbouring threads on neighbouring bytes of a row; the per-element code is
// resample_u8.h, which preproc_host_check.cpp runs on the host in the same decomposition.  No atomics, no
// shared memory, every loop bounded by a table size (resample_u8.h).
#include "resample_u8.h"
#include "common.h"

namespace {

// a count of elements as int, or -1 when it does not leave 256 of headroom below 2^31
int pp_total(int64_t t) { return t < 0 || t + 256 > 0x7fffffffLL ? -1 : (int)t; }

// horizontal pass: src [F, H, W, 3] -> mid [F, nrows, Sw, 3], source rows [row0, row0 + nrows)
__global__ __launch_bounds__(256) void pp_resample_h_kernel(int total, int H, int W, const uint8_t* src, int Sw,
                                                            int kx, const int* x_min, const int* x_cnt,
                                                            const int* x_coef, int row0, int nrows, uint8_t* mid) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (the host checked total + 256 < 2^31)
  if (i >= total) return;
  const int c = i % 3, ox = (i / 3) % Sw;
  const int r = (i / (3 * Sw)) % nrows, f = i / (3 * Sw * nrows);
  const uint8_t* line = src + ((int64_t)(f * H + row0 + r) * W) * 3 + c;
  mid[i] = rs_sample(line, 3, W, x_min[ox], x_cnt[ox], x_coef + (int64_t)ox * kx, kx);
}

// vertical pass and the normalisation: mid -> out [F, 3, Sh, Sw] fp32 = lut[c][value]
__global__ __launch_bounds__(256) void pp_resample_v_kernel(int total, int Sw, int Sh, int ky, const int* y_min,
                                                            const int* y_cnt, const int* y_coef, int row0, int nrows,
                                                            const uint8_t* mid, const float* lut, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = i % Sw, oy = (i / Sw) % Sh;
  const int c = (i / (Sw * Sh)) % 3, f = i / (Sw * Sh * 3);
  const uint8_t* col = mid + ((int64_t)f * nrows * Sw + ox) * 3 + c;
  const uint8_t v = rs_sample(col, (int64_t)Sw * 3, nrows, y_min[oy] - row0, y_cnt[oy], y_coef + (int64_t)oy * ky, ky);
  out[i] = lut[c * 256 + v];
}

// one thread per (frame, output row, output column): the frame's annotations, then all N planes
__global__ __launch_bounds__(256) void pp_rle_catmasks_kernel(int total, int N, int H, int A, const int* run_off,
                                                              const int* run_end, const int* ann_cat,
                                                              const int* frame_off, int Sh, int Sw, const int* row_map,
                                                              const int* col_map, uint8_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int plane = Sh * Sw;
  const int x = i % Sw, y = (i / Sw) % Sh, f = i / plane;
  int a0 = frame_off[f], a1 = frame_off[f + 1];
  a0 = a0 < 0 ? 0 : a0;
  a1 = a1 > A ? A : a1;
  const uint64_t set = rs_cat_set(run_off, run_end, ann_cat, a0, a1, N, col_map[x] * H + row_map[y]);
  uint8_t* o = out + (int64_t)f * N * plane + (i - f * plane);
  for (int n = 0; n < N; ++n) o[(int64_t)n * plane] = (uint8_t)((set >> n) & 1);
}

bool pp_side_ok(int v) { return v >= 1 && v <= RS_MAX_SIDE; }

}  // namespace

extern "C" int s2h_resample_u8_norm(int F, int H, int W, const uint8_t* src, int Sw, int kx, const int* x_min,
                                    const int* x_cnt, const int* x_coef, int Sh, int ky, const int* y_min,
                                    const int* y_cnt, const int* y_coef, int row0, int nrows, const float* lut,
                                    uint8_t* scratch, float* out, hipStream_t st) {
  if (F < 0 || !pp_side_ok(H) || !pp_side_ok(W) || !pp_side_ok(Sh) || !pp_side_ok(Sw)) return (int)hipErrorInvalidValue;
  if (kx < 1 || kx > RS_MAX_TAPS || ky < 1 || ky > RS_MAX_TAPS) return (int)hipErrorInvalidValue;
  if (row0 < 0 || nrows < 1 || row0 > H - nrows) return (int)hipErrorInvalidValue;
  const int n_src = pp_total((int64_t)F * H * W * 3);
  const int n_mid = pp_total((int64_t)F * nrows * Sw * 3);
  const int n_out = pp_total((int64_t)F * 3 * Sh * Sw);
  if (n_src < 0 || n_mid < 0 || n_out < 0) return (int)hipErrorInvalidValue;
  if (F == 0) return 0;
  if (!src || !x_min || !x_cnt || !x_coef || !y_min || !y_cnt || !y_coef || !lut || !scratch || !out)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pp_resample_h_kernel, dim3((unsigned)((n_mid + 255) / 256)), dim3(256), 0, st, n_mid, H, W, src, Sw,
                     kx, x_min, x_cnt, x_coef, row0, nrows, scratch);
  hipLaunchKernelGGL(pp_resample_v_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, n_out, Sw, Sh, ky,
                     y_min, y_cnt, y_coef, row0, nrows, (const uint8_t*)scratch, lut, out);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_rle_catmasks(int F, int N, int H, int W, int A, const int* run_off, const int* run_end,
                                const int* ann_cat, const int* frame_off, int Sh, int Sw, const int* row_map,
                                const int* col_map, uint8_t* out, hipStream_t st) {
  if (F < 0 || N < 0 || N > RS_MAX_CATS || A < 0 || !pp_side_ok(H) || !pp_side_ok(W) || !pp_side_ok(Sh) ||
      !pp_side_ok(Sw))
    return (int)hipErrorInvalidValue;
  const int n_thr = pp_total((int64_t)F * Sh * Sw);
  if (n_thr < 0 || pp_total((int64_t)F * N * Sh * Sw) < 0 || pp_total((int64_t)H * W) < 0)
    return (int)hipErrorInvalidValue;
  if (n_thr == 0 || N == 0) return 0;
  if (!frame_off || !row_map || !col_map || !out || (A > 0 && (!run_off || !run_end || !ann_cat)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pp_rle_catmasks_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, st, n_thr, N, H, A,
                     run_off, run_end, ann_cat, frame_off, Sh, Sw, row_map, col_map, out);
  S2H_LAUNCH_CHECK();
}
