// Stand-alone host run of the correction-click kernels' logic (clicks.h): the steps of clicks.hip in the same
// order and the same decomposition -- rows cut into words of 64 pixels with their carries, blocks of 256 pixels
// whose key maxima are merged in a second step, chunks of GP_CHUNK for the rank -- one lane after the other
// instead of one thread per pixel, over cases read from a file.  Built with plain g++
// (tests/test_clicks_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   clicks_host_check IN OUT
// IN: a sequence of cases, each 6 int32 {mode, ...} followed by the mode's arrays:
//   mode 0 transform {0, N, H, W}: mask uint8 [N, H, W] -> dist2 int32 [N, H, W]
//   mode 1 centre    {1, B, H, W, has_pred}: gt uint8 [B, H, W], pred when has_pred
//          -> points float [B, 2], labels int32 [B], dmax int32 [B, 2]
//   mode 2 uniform   {2, B, H, W, has_pred, P}: gt, pred when has_pred, r int64 [B, P]
//          -> points float [B, P, 2], labels int32 [B, P], count int32 [B, 2]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clicks.h"

static const int WAVES = GP_BLOCK / GP_WAVE;

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// ck_row_kernel: every row of the rows x W pixels of a (mask) or of a = gt, b = pred (fused)
static void row_pass(int rows, int W, const uint8_t* a, const uint8_t* b, int fused, uint16_t* hplane) {
  const int nw = (W + GP_WAVE - 1) / GP_WAVE;
  std::vector<uint64_t> words[2] = {std::vector<uint64_t>(nw), std::vector<uint64_t>(nw)};
  std::vector<int> run_l[2] = {std::vector<int>(nw), std::vector<int>(nw)};
  std::vector<int> run_r[2] = {std::vector<int>(nw), std::vector<int>(nw)};
  for (int r = 0; r < rows; ++r) {
    const size_t row = (size_t)r * W;
    for (int w = 0; w < nw; ++w) {
      uint64_t first = 0, second = 0;  // the two ballots
      for (int lane = 0; lane < GP_WAVE; ++lane) {
        const int x = w * GP_WAVE + lane;
        const bool in = x < W;
        const bool g = in && a[row + x] != 0;
        const bool p = in && b && b[row + x] != 0;
        if (fused ? ck_fn(g, p) : g) first |= 1ull << lane;
        if (fused && in && ck_fp(g, p)) second |= 1ull << lane;
      }
      words[0][w] = first;
      words[1][w] = second;
    }
    for (int k = 0; k < 2; ++k) {
      ck_row_carry_left(words[k].data(), nw, run_l[k].data());
      ck_row_carry_right(words[k].data(), nw, run_r[k].data());
    }
    for (int w = 0; w < nw; ++w)
      for (int lane = 0; lane < GP_WAVE; ++lane) {
        const int x = w * GP_WAVE + lane;
        if (x < W)
          hplane[row + x] = ck_pack(ck_row_dist(words[0][w], lane, run_l[0][w], run_r[0][w]),
                                    ck_row_dist(words[1][w], lane, run_l[1][w], run_r[1][w]));
      }
  }
}

static void edt(int N, int H, int W, const uint8_t* mask, int* dist2) {
  const int HW = H * W, total = N * HW;
  std::vector<uint16_t> hplane(total);
  row_pass(N * H, W, mask, nullptr, 0, hplane.data());
  for (int i = 0; i < total; ++i) {  // ck_col_store_kernel
    const int q = i % HW;
    int tag;
    dist2[i] = ck_col_d2(hplane.data() + (i - q), H, W, q / W, q % W, &tag);
  }
}

static void center(int B, int H, int W, const uint8_t* gt, const uint8_t* pred, float* points, int* labels,
                   int* dmax) {
  const int HW = H * W, nb = (HW + GP_BLOCK - 1) / GP_BLOCK;
  std::vector<uint16_t> hplane((size_t)B * HW);
  std::vector<uint64_t> part((size_t)B * nb * 2);
  row_pass(B * H, W, gt, pred, 1, hplane.data());
  for (int img = 0; img < B; ++img)  // ck_col_key_kernel
    for (int b = 0; b < nb; ++b) {
      uint64_t k0 = 0, k1 = 0;
      for (int t = 0; t < GP_BLOCK; ++t) {
        const int q = b * GP_BLOCK + t;
        if (q >= HW) continue;
        int tag;
        const int d2 = ck_col_d2(hplane.data() + (size_t)img * HW, H, W, q / W, q % W, &tag);
        const uint64_t c0 = ck_key(tag ? 0 : d2, q), c1 = ck_key(tag ? d2 : 0, q);
        k0 = c0 > k0 ? c0 : k0;
        k1 = c1 > k1 ? c1 : k1;
      }
      part[2 * ((size_t)img * nb + b)] = k0;
      part[2 * ((size_t)img * nb + b) + 1] = k1;
    }
  for (int img = 0; img < B; ++img) {  // ck_center_pick_kernel
    uint64_t k0 = 0, k1 = 0;
    for (int b = 0; b < nb; ++b) {
      const uint64_t c0 = part[2 * ((size_t)img * nb + b)], c1 = part[2 * ((size_t)img * nb + b) + 1];
      k0 = c0 > k0 ? c0 : k0;
      k1 = c1 > k1 ? c1 : k1;
    }
    ck_center_click(k0, k1, W, points + 2 * img, labels + img, dmax + 2 * img);
  }
}

// the union ballots of one tile of 256 pixels: m[w] of its four waves; fn[w]: which of them are FN
static void tile_ballots(const uint8_t* gt, const uint8_t* pred, int HW, int q0, bool all_correct, uint64_t* m,
                         uint64_t* fn) {
  for (int w = 0; w < WAVES; ++w) {
    m[w] = fn[w] = 0;
    for (int lane = 0; lane < GP_WAVE; ++lane) {
      const int q = q0 + w * GP_WAVE + lane;
      const bool in = q < HW;
      const bool g = in && gt[q] != 0;
      const bool p = in && pred && pred[q] != 0;
      if (in && ck_union(g, p, all_correct)) m[w] |= 1ull << lane;
      if (ck_fn(g, p)) fn[w] |= 1ull << lane;
    }
  }
}

static void uniform(int B, int P, int H, int W, const uint8_t* gt, const uint8_t* pred, const int64_t* r,
                    float* points, int* labels, int* count) {
  const int HW = H * W, nchunk = (HW + GP_CHUNK - 1) / GP_CHUNK;
  std::vector<int> cnt((size_t)B * nchunk * 3, 0), tot((size_t)B * 3, 0);
  for (int obj = 0; obj < B; ++obj)  // ck_uni_count_kernel
    for (int c = 0; c < nchunk; ++c)
      for (int s = 0; s < GP_TILES; ++s)
        for (int w = 0; w < WAVES; ++w) {
          uint64_t b0 = 0, b1 = 0, b2 = 0;
          for (int lane = 0; lane < GP_WAVE; ++lane) {
            const int q = c * GP_CHUNK + s * GP_BLOCK + w * GP_WAVE + lane;
            const bool in = q < HW;
            const bool g = in && gt[(size_t)obj * HW + q] != 0;
            const bool p = in && pred && pred[(size_t)obj * HW + q] != 0;
            if (in && ck_fp(g, p)) b0 |= 1ull << lane;
            if (ck_fn(g, p)) b1 |= 1ull << lane;
            if (in && !g) b2 |= 1ull << lane;
          }
          int* o = cnt.data() + 3 * ((size_t)obj * nchunk + c);
          o[0] += gp_popc(b0);
          o[1] += gp_popc(b1);
          o[2] += gp_popc(b2);
        }
  for (int obj = 0; obj < B; ++obj) {  // ck_uni_total_kernel
    for (int c = 0; c < nchunk; ++c)
      for (int k = 0; k < 3; ++k) tot[3 * obj + k] += cnt[3 * ((size_t)obj * nchunk + c) + k];
    const bool all_correct = tot[3 * obj] + tot[3 * obj + 1] == 0;
    count[2 * obj] = all_correct ? tot[3 * obj + 2] : tot[3 * obj];
    count[2 * obj + 1] = tot[3 * obj + 1];
  }
  for (int i = 0; i < B * P; ++i) {  // ck_uni_pick_kernel
    const int obj = i / P;
    const uint8_t* g = gt + (size_t)obj * HW;
    const uint8_t* p = pred ? pred + (size_t)obj * HW : nullptr;
    const bool all_correct = tot[3 * obj] + tot[3 * obj + 1] == 0;
    const int n = all_correct ? tot[3 * obj + 2] : tot[3 * obj] + tot[3 * obj + 1];
    points[2 * i] = points[2 * i + 1] = -1.f;  // (shows a click that nothing wrote)
    labels[i] = -1;
    if (n == 0) {
      points[2 * i] = points[2 * i + 1] = 0.f;
      labels[i] = 0;
      continue;
    }
    const int rank = ck_rank(r[i], n);
    int chunk = -1, rem = 0, acc = 0;
    for (int c = 0; c < nchunk && chunk < 0; ++c) {
      const int* o = cnt.data() + 3 * ((size_t)obj * nchunk + c);
      const int v = all_correct ? o[2] : o[0] + o[1];
      if (rank < acc + v) {
        chunk = c;
        rem = rank - acc;
      }
      acc += v;
    }
    if (chunk < 0) continue;
    int running = 0;
    for (int s = 0; s < GP_TILES; ++s) {
      uint64_t m[WAVES], fn[WAVES];
      const int q0 = chunk * GP_CHUNK + s * GP_BLOCK;
      tile_ballots(g, p, HW, q0, all_correct, m, fn);
      int before = running;
      for (int w = 0; w < WAVES; ++w) {
        for (int lane = 0; lane < GP_WAVE; ++lane)
          if (((m[w] >> lane) & 1) && before + gp_popc(gp_below(m[w], lane)) == rem) {
            const int q = q0 + w * GP_WAVE + lane;
            points[2 * i] = (float)(q % W);
            points[2 * i + 1] = (float)(q / W);
            labels[i] = (int)((fn[w] >> lane) & 1);
          }
        before += gp_popc(m[w]);
      }
      running = before;
    }
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
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  int hdr[6];
  while (fread(hdr, sizeof(int), 6, in) == 6) {
    const int mode = hdr[0], N = hdr[1], H = hdr[2], W = hdr[3], has_pred = hdr[4], P = hdr[5];
    if (mode < 0 || mode > 2 || N < 0 || H < 1 || W < 1 || H > CK_MAX_SIDE || W > CK_MAX_SIDE || P < 0 ||
        (int64_t)H * W > GP_MAX_PIXELS || (int64_t)N * H * W > 0x7fffff00LL) {
      fprintf(stderr, "bad case header\n");
      return 1;
    }
    const size_t total = (size_t)N * H * W;
    std::vector<uint8_t> gt, pred;
    if (!rd(in, gt, total) || (mode > 0 && has_pred && !rd(in, pred, total))) {
      fprintf(stderr, "short input\n");
      return 1;
    }
    const uint8_t* pp = (mode > 0 && has_pred) ? pred.data() : nullptr;
    if (mode == 0) {
      std::vector<int> dist2(total);
      edt(N, H, W, gt.data(), dist2.data());
      wr(out, dist2);
    } else if (mode == 1) {
      std::vector<float> points((size_t)N * 2);
      std::vector<int> labels(N), dmax((size_t)N * 2);
      center(N, H, W, gt.data(), pp, points.data(), labels.data(), dmax.data());
      wr(out, points);
      wr(out, labels);
      wr(out, dmax);
    } else {
      std::vector<int64_t> r;
      if (!rd(in, r, (size_t)N * P)) {
        fprintf(stderr, "short input\n");
        return 1;
      }
      std::vector<float> points((size_t)N * P * 2);
      std::vector<int> labels((size_t)N * P), count((size_t)N * 2);
      uniform(N, P, H, W, gt.data(), pp, r.data(), points.data(), labels.data(), count.data());
      wr(out, points);
      wr(out, labels);
      wr(out, count);
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 1;
}
