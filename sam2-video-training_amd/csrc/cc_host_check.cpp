// Stand-alone host run of the connected-components union-find (cc_uf.h): the steps of cc.hip in the same
// order, one pixel after the other instead of one thread per pixel, over cases read from a file.  Built with
// plain g++ (tests/test_cc_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   cc_host_check IN OUT
// IN:  a sequence of cases, each 5 int32 {mode, N, H, W, arg} followed by N*H*W float32 scores.
//      mode 0: label, arg = positive      -> OUT gets N*H*W int32 labels, then N*H*W int32 areas
//      mode 1: fill holes, arg = max_area -> OUT gets N*H*W float32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cc_uf.h"

// steps 1-3 of cc.hip: run labelling over groups of 64 consecutive pixels, merge, flatten + count
static void roots(int N, int H, int W, const float* scores, int positive, int* L, int* cnt) {
  const int HW = H * W, total = N * HW;
  for (int base = 0; base < total; base += CC_WAVE) {
    uint64_t fgm = 0, linkm = 0;
    for (int lane = 0; lane < CC_WAVE && base + lane < total; ++lane)
      if (cc_fg(scores[base + lane], positive)) fgm |= 1ull << lane;
    for (int lane = 1; lane < CC_WAVE && base + lane < total; ++lane) {
      const int x = (base + lane) % HW % W;
      if (((fgm >> lane) & 1) && x > 0 && ((fgm >> (lane - 1)) & 1)) linkm |= 1ull << lane;
    }
    for (int lane = 0; lane < CC_WAVE && base + lane < total; ++lane) {
      const int i = base + lane, q = i % HW;
      L[i] = ((fgm >> lane) & 1) ? q - (lane - cc_run_start(linkm, lane)) : -1;
      cnt[i] = 0;
    }
  }
  for (int i = 0; i < total; ++i) {
    if (L[i] < 0) continue;
    const int q = i % HW;
    cc_merge_pixel(L + (i - q), H, W, q / W, q % W, i % CC_WAVE == 0);
  }
  for (int i = 0; i < total; ++i) {
    if (L[i] < 0) continue;
    const int q = i % HW;
    int budget = HW;
    const int r = cc_find(L + (i - q), q, &budget);
    if (r != q) cc_min(L + i, r);
    cnt[i - q + r] += 1;
  }
}

static bool small(int i, int HW, const int* L, const int* cnt, int max_area) {
  return L[i] >= 0 && cnt[i - i % HW + L[i]] <= max_area;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr[5];
  while (fread(hdr, sizeof(int), 5, in) == 5) {
    const int mode = hdr[0], N = hdr[1], H = hdr[2], W = hdr[3], arg = hdr[4];
    if (N < 0 || H < 1 || W < 1 || (long long)H * W > CC_MAX_PIXELS || (long long)N * H * W > (1 << 28)) return 3;
    const int HW = H * W, total = N * HW;
    std::vector<float> s(total), o(total);
    std::vector<int> L(total), cnt(total);
    if (fread(s.data(), sizeof(float), total, in) != (size_t)total) return 3;
    if (mode == 0) {
      roots(N, H, W, s.data(), arg, L.data(), cnt.data());
      for (int i = 0; i < total; ++i) {  // cc_labels_kernel
        const int r = L[i], q = i % HW;
        L[i] = r < 0 ? 0 : r + 1;
        if (r >= 0 && r != q) cnt[i] = cnt[i - q + r];
      }
      fwrite(L.data(), sizeof(int), total, out);
      fwrite(cnt.data(), sizeof(int), total, out);
    } else {
      roots(N, H, W, s.data(), 0, L.data(), cnt.data());
      for (int i = 0; i < total; ++i) o[i] = small(i, HW, L.data(), cnt.data(), arg) ? 0.1f : s[i];
      roots(N, H, W, o.data(), 1, L.data(), cnt.data());
      for (int i = 0; i < total; ++i)
        if (small(i, HW, L.data(), cnt.data(), arg)) o[i] = -0.1f;
      fwrite(o.data(), sizeof(float), total, out);
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
