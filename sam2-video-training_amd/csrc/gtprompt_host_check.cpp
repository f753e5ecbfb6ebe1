// Stand-alone host run of the prompt-generation kernels' logic (gtprompt.h): the steps of gtprompt.hip in the
// same order and the same decomposition -- waves of 64 pixels, blocks of 256, chunks of GP_CHUNK -- one lane
// after the other instead of one thread per pixel, over cases read from a file.  Built with plain g++
// (tests/test_gt_prompts_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   gtprompt_host_check IN OUT
// IN: a sequence of cases, each 9 int32 {mode, ...} followed by the mode's arrays:
//   mode 0 decode     {0, A, H, W, R}: run_off int32 [A + 1], run_end int32 [R]    -> mask uint8 [A, H, W]
//   mode 1 morphology {1, N, H, W, op, y_lo, y_hi, x_lo, x_hi}: in uint8 [N, H, W] -> out uint8 [N, H, W]
//   mode 2 components {2, N, H, W, min_area, has_grid, capacity}: labels, areas int32 [N, H, W], grid uint8 [H, W]
//          when has_grid -> hdr int32 [2 N + 2], stats int64 [capacity + 1, 9] (rows never written hold -7, the
//          extra row shows that nothing is written past the end), index uint8 [N, H, W]
//   mode 3 rank select {3, Q, N, H, W, has_grid}: q_img, q_label, q_neg, q_rank int32 [Q], labels int32 [N, H, W],
//          grid when has_grid -> xy int32 [Q, 2], count int32 [Q]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gtprompt.h"

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

static void decode(int A, int H, int W, const int* run_off, const int* run_end, uint8_t* mask) {
  const int HW = H * W;
  for (int i = 0; i < A * HW; ++i) {  // gp_rle_decode_kernel
    const int a = i / HW, q = i % HW, y = q / W, x = q % W;
    const int o = run_off[a], n = run_off[a + 1] - o;
    mask[i] = (uint8_t)(gp_run_index(run_end + o, n < 0 ? 0 : n, x * H + y) & 1);
  }
}

static void morph_pass(int N, int H, int W, const uint8_t* in, int op, int lo, int hi, int vertical, uint8_t* out) {
  const int HW = H * W;
  for (int i = 0; i < N * HW; ++i) {  // gp_morph_pass_kernel
    const int q = i % HW, y = q / W, x = q % W;
    const uint8_t* img = in + (i - q);
    out[i] = vertical ? gp_morph_line(img + x, H, W, y, lo, hi, op) : gp_morph_line(img + y * W, W, 1, x, lo, hi, op);
  }
}

// the kept-root ballots of one block: m[w] of its four waves
static void block_ballots(int img, int b, int HW, const int* labels, const int* areas, int min_area, uint64_t* m) {
  for (int w = 0; w < WAVES; ++w) {
    m[w] = 0;
    for (int lane = 0; lane < GP_WAVE; ++lane) {
      const int q = b * GP_BLOCK + w * GP_WAVE + lane;
      if (q < HW && gp_kept_root(labels[img * HW + q], areas[img * HW + q], q, min_area)) m[w] |= 1ull << lane;
    }
  }
}

static void components(int N, int H, int W, const int* labels, const int* areas, int min_area, const uint8_t* grid,
                       int capacity, int* hdr, int64_t* stats, uint8_t* index) {
  const int HW = H * W, nb = (HW + GP_BLOCK - 1) / GP_BLOCK, total = N * HW;
  std::vector<int> blk((size_t)N * nb), rk(total);
  uint64_t m[WAVES];
  for (int img = 0; img < N; ++img)  // gp_comp_count_kernel
    for (int b = 0; b < nb; ++b) {
      block_ballots(img, b, HW, labels, areas, min_area, m);
      blk[img * nb + b] = gp_popc(m[0]) + gp_popc(m[1]) + gp_popc(m[2]) + gp_popc(m[3]);
    }
  for (int img = 0; img < N; ++img) {  // gp_comp_scan_kernel
    int carry = 0;
    for (int b = 0; b < nb; ++b) {
      const int v = blk[img * nb + b];
      blk[img * nb + b] = carry;
      carry += v;
    }
    hdr[2 * img] = carry;
  }
  int carry = 0, over = 0;  // gp_comp_offsets_kernel
  for (int img = 0; img < N; ++img) {
    hdr[2 * img + 1] = carry;
    carry += hdr[2 * img];
    over |= hdr[2 * img] > GP_MAX_INDEX;
  }
  hdr[2 * N] = carry;
  hdr[2 * N + 1] = over;
  for (int img = 0; img < N; ++img)  // gp_comp_rank_kernel
    for (int b = 0; b < nb; ++b) {
      block_ballots(img, b, HW, labels, areas, min_area, m);
      for (int w = 0; w < WAVES; ++w)
        for (int lane = 0; lane < GP_WAVE; ++lane) {
          const int q = b * GP_BLOCK + w * GP_WAVE + lane;
          if (q >= HW) continue;
          const int i = img * HW + q;
          if (!((m[w] >> lane) & 1)) {
            rk[i] = 0;
            continue;
          }
          int rank = blk[img * nb + b] + gp_popc(gp_below(m[w], lane));
          for (int v = 0; v < w; ++v) rank += gp_popc(m[v]);
          rk[i] = rank + 1;
          const int64_t row = (int64_t)hdr[2 * img + 1] + rank;
          if (row >= capacity) continue;
          int64_t* s = stats + row * GP_STATS;
          s[0] = labels[i];
          s[1] = areas[i];
          s[2] = W;
          s[3] = H;
          s[4] = s[5] = -1;
          s[6] = s[7] = s[8] = 0;
        }
    }
  for (int base = 0; base < total; base += GP_WAVE) {  // gp_comp_stats_kernel, one wave
    int g[GP_WAVE], x[GP_WAVE], y[GP_WAVE];
    bool sel[GP_WAVE], todo[GP_WAVE];
    for (int lane = 0; lane < GP_WAVE; ++lane) {
      const int i = base + lane;
      g[lane] = -1;
      x[lane] = y[lane] = 0;
      sel[lane] = false;
      if (i < total) {
        const int q = i % HW, l = labels[i];
        const int r = l > 0 && l <= HW ? rk[i - q + l - 1] : 0;
        index[i] = (uint8_t)(r > GP_MAX_INDEX ? GP_MAX_INDEX : r);
        if (r > 0) {
          const int64_t row = (int64_t)hdr[2 * (i / HW) + 1] + r - 1;
          if (row < capacity) g[lane] = (int)row;
          y[lane] = q / W;
          x[lane] = q % W;
          sel[lane] = !grid || grid[q] != 0;
        }
      }
      todo[lane] = g[lane] >= 0;
    }
    for (int it = 0; it < GP_WAVE; ++it) {
      int leader = -1, last = -1;
      for (int lane = 0; lane < GP_WAVE && leader < 0; ++lane)
        if (todo[lane]) leader = lane;
      if (leader < 0) break;
      const int lg = g[leader];
      int nsel = 0, xmin = 0x7fffffff, xmax = -1, sx = 0, sy = 0;
      for (int lane = 0; lane < GP_WAVE; ++lane) {
        if (!(todo[lane] && g[lane] == lg)) continue;
        last = lane;
        if (x[lane] < xmin) xmin = x[lane];
        if (x[lane] > xmax) xmax = x[lane];
        if (sel[lane]) {
          ++nsel;
          sx += x[lane];
          sy += y[lane];
        }
        todo[lane] = false;
      }
      int64_t* s = stats + (int64_t)lg * GP_STATS;
      if (xmin < s[2]) s[2] = xmin;
      if (y[leader] < s[3]) s[3] = y[leader];  // (y is monotone over the lanes of one image)
      if (xmax > s[4]) s[4] = xmax;
      if (y[last] > s[5]) s[5] = y[last];
      s[6] += nsel;
      s[7] += sx;
      s[8] += sy;
    }
  }
}

static bool query_pixel(bool valid, int img, int HW, int p, const int* labels, int ql, int neg, const uint8_t* grid) {
  return valid && p < HW && gp_selected(labels[(int64_t)img * HW + p], ql, neg, grid, p);
}

static void rank_select(int Q, const int* q_img, const int* q_label, const int* q_neg, const int* q_rank, int N, int H,
                        int W, const int* labels, const uint8_t* grid, int* xy, int* count) {
  const int HW = H * W, nchunk = (HW + GP_CHUNK - 1) / GP_CHUNK;
  std::vector<int> cnt((size_t)Q * nchunk);
  for (int qi = 0; qi < Q; ++qi) {  // gp_rank_count_kernel
    const int img = q_img[qi];
    const bool valid = img >= 0 && img < N;
    for (int c = 0; c < nchunk; ++c) {
      int acc = 0;
      for (int t = 0; t < GP_CHUNK; ++t)
        acc += query_pixel(valid, img, HW, c * GP_CHUNK + t, labels, q_label[qi], q_neg[qi], grid);
      cnt[(size_t)qi * nchunk + c] = acc;
    }
  }
  for (int qi = 0; qi < Q; ++qi) {  // gp_rank_pick_kernel
    const int img = q_img[qi], ql = q_label[qi], neg = q_neg[qi], rank = q_rank[qi];
    const bool valid = img >= 0 && img < N;
    const int* row = cnt.data() + (size_t)qi * nchunk;
    const int per = (nchunk + GP_BLOCK - 1) / GP_BLOCK;
    int ex = 0, chunk = -1, rem = 0;
    for (int t = 0; t < GP_BLOCK; ++t) {  // thread t owns chunks [t per, t per + per)
      int local = 0;
      for (int j = 0; j < per; ++j)
        if (t * per + j < nchunk) local += row[t * per + j];
      if (rank >= ex && rank < ex + local) {
        int acc = ex;
        for (int j = 0; j < per; ++j) {
          const int c = t * per + j, v = c < nchunk ? row[c] : 0;
          if (rank < acc + v) {
            chunk = c;
            rem = rank - acc;
            break;
          }
          acc += v;
        }
      }
      ex += local;
    }
    count[qi] = ex;
    xy[2 * qi] = xy[2 * qi + 1] = -1;
    if (chunk < 0) continue;
    int running = 0;
    for (int s = 0; s < GP_TILES; ++s) {
      uint64_t m[WAVES];
      for (int w = 0; w < WAVES; ++w) {
        m[w] = 0;
        for (int lane = 0; lane < GP_WAVE; ++lane)
          if (query_pixel(valid, img, HW, chunk * GP_CHUNK + s * GP_BLOCK + w * GP_WAVE + lane, labels, ql, neg, grid))
            m[w] |= 1ull << lane;
      }
      int woff = 0;
      for (int w = 0; w < WAVES; ++w) {
        for (int lane = 0; lane < GP_WAVE; ++lane) {
          const int p = chunk * GP_CHUNK + s * GP_BLOCK + w * GP_WAVE + lane;
          if (((m[w] >> lane) & 1) && running + woff + gp_popc(gp_below(m[w], lane)) == rem) {
            xy[2 * qi] = p % W;
            xy[2 * qi + 1] = p / W;
          }
        }
        woff += gp_popc(m[w]);
      }
      running += woff;
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int h[9];
  while (fread(h, sizeof(int), 9, in) == 9) {
    const int mode = h[0];
    if (mode == 0) {
      const int A = h[1], H = h[2], W = h[3], R = h[4];
      if (A < 0 || H < 1 || W < 1 || R < 0 || (long long)H * W > GP_MAX_PIXELS || (long long)A * H * W > (1 << 28)) return 3;
      std::vector<int> off, end;
      if (!rd(in, off, (size_t)A + 1) || !rd(in, end, (size_t)R)) return 3;
      for (int a = 0; a < A; ++a)
        if (off[a] < 0 || off[a] > off[a + 1] || off[a + 1] > R) return 3;
      std::vector<uint8_t> mask((size_t)A * H * W);
      decode(A, H, W, off.data(), end.data(), mask.data());
      wr(out, mask);
    } else if (mode == 1) {
      const int N = h[1], H = h[2], W = h[3], op = h[4];
      if (N < 0 || H < 1 || W < 1 || (long long)H * W > GP_MAX_PIXELS || (long long)N * H * W > (1 << 28)) return 3;
      for (int k = 5; k < 9; k += 2)
        if (h[k] < -GP_MAX_REACH || h[k] > 0 || h[k + 1] < 0 || h[k + 1] > GP_MAX_REACH) return 3;
      std::vector<uint8_t> src, work((size_t)N * H * W), dst((size_t)N * H * W);
      if (!rd(in, src, (size_t)N * H * W)) return 3;
      morph_pass(N, H, W, src.data(), op, h[7], h[8], 0, work.data());   // s2h_morph_rect: along x, then along y
      morph_pass(N, H, W, work.data(), op, h[5], h[6], 1, dst.data());
      wr(out, dst);
    } else if (mode == 2) {
      const int N = h[1], H = h[2], W = h[3], min_area = h[4], has_grid = h[5], capacity = h[6];
      if (N < 0 || H < 1 || W < 1 || capacity < 0 || (long long)H * W > GP_MAX_PIXELS || (long long)N * H * W > (1 << 28))
        return 3;
      std::vector<int> labels, areas, hdr((size_t)2 * N + 2);
      std::vector<uint8_t> grid, index((size_t)N * H * W);
      if (!rd(in, labels, (size_t)N * H * W) || !rd(in, areas, (size_t)N * H * W)) return 3;
      if (has_grid && !rd(in, grid, (size_t)H * W)) return 3;
      std::vector<int64_t> stats(((size_t)capacity + 1) * GP_STATS, -7);
      components(N, H, W, labels.data(), areas.data(), min_area, has_grid ? grid.data() : nullptr, capacity, hdr.data(),
                 stats.data(), index.data());
      wr(out, hdr);
      wr(out, stats);
      wr(out, index);
    } else if (mode == 3) {
      const int Q = h[1], N = h[2], H = h[3], W = h[4], has_grid = h[5];
      if (Q < 0 || N < 0 || H < 1 || W < 1 || (long long)H * W > GP_MAX_PIXELS || (long long)N * H * W > (1 << 28)) return 3;
      std::vector<int> qa[4], labels, xy((size_t)2 * Q), count((size_t)Q);
      for (auto& v : qa)
        if (!rd(in, v, (size_t)Q)) return 3;
      std::vector<uint8_t> grid;
      if (!rd(in, labels, (size_t)N * H * W)) return 3;
      if (has_grid && !rd(in, grid, (size_t)H * W)) return 3;
      rank_select(Q, qa[0].data(), qa[1].data(), qa[2].data(), qa[3].data(), N, H, W, labels.data(),
                  has_grid ? grid.data() : nullptr, xy.data(), count.data());
      wr(out, xy);
      wr(out, count);
    } else {
      return 3;
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
