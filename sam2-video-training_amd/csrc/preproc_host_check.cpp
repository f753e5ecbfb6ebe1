// Stand-alone host run of the clip-loading kernels' logic (resample_u8.h): the steps of preproc.hip in the same
// order and the same decomposition -- one output element per thread index, the index split as the kernels split
// it -- one element after the other, over cases read from a file.  Built with plain g++
// (tests/test_preproc_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   preproc_host_check IN OUT
// IN: a sequence of cases, each 12 int32 {mode, ...} followed by the mode's arrays:
//   mode 0 resample  {0, F, H, W, Sw, kx, Sh, ky, row0, nrows}: src uint8 [F, H, W, 3], x_min, x_cnt int32 [Sw],
//          x_coef int32 [Sw, kx], y_min, y_cnt int32 [Sh], y_coef int32 [Sh, ky], lut fp32 [3, 256]
//          -> out fp32 [F, 3, Sh, Sw]
//   mode 1 catmasks  {1, F, N, H, W, A, R, Sh, Sw}: run_off int32 [A + 1], run_end int32 [R], ann_cat int32 [A],
//          frame_off int32 [F + 1], row_map int32 [Sh], col_map int32 [Sw] -> out uint8 [F, N, Sh, Sw]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_u8.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static void resample(int F, int H, int W, const uint8_t* src, int Sw, int kx, const int* x_min, const int* x_cnt,
                     const int* x_coef, int Sh, int ky, const int* y_min, const int* y_cnt, const int* y_coef, int row0,
                     int nrows, const float* lut, uint8_t* mid, float* out) {
  const int n_mid = F * nrows * Sw * 3, n_out = F * 3 * Sh * Sw;
  for (int i = 0; i < n_mid; ++i) {  // pp_resample_h_kernel
    const int c = i % 3, ox = (i / 3) % Sw;
    const int r = (i / (3 * Sw)) % nrows, f = i / (3 * Sw * nrows);
    const uint8_t* line = src + ((int64_t)(f * H + row0 + r) * W) * 3 + c;
    mid[i] = rs_sample(line, 3, W, x_min[ox], x_cnt[ox], x_coef + (int64_t)ox * kx, kx);
  }
  for (int i = 0; i < n_out; ++i) {  // pp_resample_v_kernel
    const int ox = i % Sw, oy = (i / Sw) % Sh;
    const int c = (i / (Sw * Sh)) % 3, f = i / (Sw * Sh * 3);
    const uint8_t* col = mid + ((int64_t)f * nrows * Sw + ox) * 3 + c;
    const uint8_t v =
        rs_sample(col, (int64_t)Sw * 3, nrows, y_min[oy] - row0, y_cnt[oy], y_coef + (int64_t)oy * ky, ky);
    out[i] = lut[c * 256 + v];
  }
}

static void catmasks(int F, int N, int H, int A, const int* run_off, const int* run_end, const int* ann_cat,
                     const int* frame_off, int Sh, int Sw, const int* row_map, const int* col_map, uint8_t* out) {
  const int plane = Sh * Sw;
  for (int i = 0; i < F * plane; ++i) {  // pp_rle_catmasks_kernel
    const int x = i % Sw, y = (i / Sw) % Sh, f = i / plane;
    int a0 = frame_off[f], a1 = frame_off[f + 1];
    a0 = a0 < 0 ? 0 : a0;
    a1 = a1 > A ? A : a1;
    const uint64_t set = rs_cat_set(run_off, run_end, ann_cat, a0, a1, N, col_map[x] * H + row_map[y]);
    uint8_t* o = out + (int64_t)f * N * plane + (i - f * plane);
    for (int n = 0; n < N; ++n) o[(int64_t)n * plane] = (uint8_t)((set >> n) & 1);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  int h[12];
  while (fread(h, sizeof(int), 12, in) == 12) {
    bool ok = true;
    if (h[0] == 0) {
      const int F = h[1], H = h[2], W = h[3], Sw = h[4], kx = h[5], Sh = h[6], ky = h[7], row0 = h[8], nrows = h[9];
      if (F < 0 || H < 1 || W < 1 || Sw < 1 || Sh < 1 || kx < 1 || kx > RS_MAX_TAPS || ky < 1 || ky > RS_MAX_TAPS ||
          row0 < 0 || nrows < 1 || row0 > H - nrows) {
        fprintf(stderr, "bad resample case\n");
        return 1;
      }
      std::vector<uint8_t> src, mid((size_t)F * nrows * Sw * 3);
      std::vector<int> xm, xc, xk, ym, yc, yk;
      std::vector<float> lut, res((size_t)F * 3 * Sh * Sw);
      ok = rd(in, src, (size_t)F * H * W * 3) && rd(in, xm, Sw) && rd(in, xc, Sw) && rd(in, xk, (size_t)Sw * kx) &&
           rd(in, ym, Sh) && rd(in, yc, Sh) && rd(in, yk, (size_t)Sh * ky) && rd(in, lut, 3 * 256);
      if (ok) {
        resample(F, H, W, src.data(), Sw, kx, xm.data(), xc.data(), xk.data(), Sh, ky, ym.data(), yc.data(), yk.data(),
                 row0, nrows, lut.data(), mid.data(), res.data());
        wr(out, res);
      }
    } else if (h[0] == 1) {
      const int F = h[1], N = h[2], H = h[3], W = h[4], A = h[5], R = h[6], Sh = h[7], Sw = h[8];
      if (F < 0 || N < 0 || N > RS_MAX_CATS || H < 1 || W < 1 || A < 0 || R < 0 || Sh < 1 || Sw < 1) {
        fprintf(stderr, "bad catmasks case\n");
        return 1;
      }
      std::vector<int> off, end, cat, foff, rows, cols;
      std::vector<uint8_t> res((size_t)F * N * Sh * Sw);
      ok = rd(in, off, (size_t)A + 1) && rd(in, end, R) && rd(in, cat, A) && rd(in, foff, (size_t)F + 1) &&
           rd(in, rows, Sh) && rd(in, cols, Sw);
      if (ok) {
        catmasks(F, N, H, A, off.data(), end.data(), cat.data(), foff.data(), Sh, Sw, rows.data(), cols.data(),
                 res.data());
        wr(out, res);
      }
    } else {
      fprintf(stderr, "unknown mode %d\n", h[0]);
      return 1;
    }
    if (!ok) {
      fprintf(stderr, "truncated case\n");
      return 1;
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 1;
}
