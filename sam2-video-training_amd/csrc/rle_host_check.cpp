// Stand-alone host run of the run-boundary extraction (rle_scan.h): the three steps of s2h_rle_transitions
// in the same order and the same decomposition into workgroups of RLE_BLOCK_WORDS words, one word after the
// other instead of one thread per word, over cases read from a file.  Built with plain g++
// (tests/test_rle_export_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   rle_host_check IN OUT
// IN:  a sequence of cases, each 4 int32 {Ncat, H, W, capacity} followed by Ncat * ceil(H W / 64) uint64
//      words (the bit-packed column-major masks; bits past H W in a last word may hold anything).
// OUT: per case Ncat * RLE_HDR int32 of header, then min(total, capacity) int32 transition positions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rle_scan.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr4[4];
  while (fread(hdr4, sizeof(int), 4, in) == 4) {
    const int Ncat = hdr4[0], H = hdr4[1], W = hdr4[2], cap = hdr4[3];
    if (Ncat < 0 || H < 1 || W < 1 || cap < 0 || (long long)H * W > RLE_MAX_PIXELS ||
        (long long)Ncat * H * W > (1 << 28))
      return 3;
    const int n = H * W, nw = (n + 63) / 64, nbw = (nw + RLE_BLOCK_WORDS - 1) / RLE_BLOCK_WORDS, F = Ncat * nbw;
    std::vector<uint64_t> bits((size_t)Ncat * nw);
    if (!bits.empty() && fread(bits.data(), sizeof(uint64_t), bits.size(), in) != bits.size()) return 3;
    // the word of "thread" tid of workgroup f, as rle_load_word
    auto load = [&](int f, int tid, uint64_t* w, uint64_t* t, int* base) {
      const int c = f / nbw, b = f - c * nbw, wi = b * RLE_BLOCK_WORDS + tid;
      *w = *t = 0;
      *base = 0;
      if (wi >= nw) return;
      const uint64_t* row = bits.data() + (size_t)c * nw;
      const uint64_t valid = rle_valid(wi, n);
      *w = row[wi] & valid;
      *t = rle_transitions(*w, wi > 0 ? row[wi - 1] >> 63 : 0ull, valid);
      *base = wi * 64;
    };
    // 1. rle_count_kernel
    std::vector<int> cnt(F), off(F);
    std::vector<RleStats> stats(F);
    for (int f = 0; f < F; ++f) {
      cnt[f] = 0;
      stats[f] = rle_stats_empty(H, W);
      for (int tid = 0; tid < RLE_BLOCK_WORDS; ++tid) {
        uint64_t w, t;
        int base;
        load(f, tid, &w, &t, &base);
        cnt[f] += rle_popc(t);
        stats[f] = rle_stats_join(stats[f], rle_word_stats(w, base, H, W));
      }
    }
    // 2. rle_scan_kernel
    int run = 0;
    for (int f = 0; f < F; ++f) {
      off[f] = run;
      run += cnt[f];
    }
    std::vector<int> hdr((size_t)Ncat * RLE_HDR);
    for (int c = 0; c < Ncat; ++c) {
      const int o0 = off[c * nbw], o1 = c + 1 < Ncat ? off[(c + 1) * nbw] : run;
      RleStats s = rle_stats_empty(H, W);
      for (int b = 0; b < nbw; ++b) s = rle_stats_join(s, stats[c * nbw + b]);
      const int h[RLE_HDR] = {o1 - o0, o0, s.area, s.xmin, s.ymin, s.xmax, s.ymax, run};
      for (int q = 0; q < RLE_HDR; ++q) hdr[(size_t)c * RLE_HDR + q] = h[q];
    }
    // 3. rle_emit_kernel, into a buffer of exactly `capacity` slots (a sanitizer sees a write past it)
    std::vector<int> trans(cap);
    for (int f = 0; f < F; ++f) {
      int k = off[f];
      for (int tid = 0; tid < RLE_BLOCK_WORDS; ++tid) {
        uint64_t w, t;
        int base;
        load(f, tid, &w, &t, &base);
        k += rle_emit(t, base, trans.data(), k, cap);
      }
    }
    if (!hdr.empty()) fwrite(hdr.data(), sizeof(int), hdr.size(), out);
    if (run > 0 && cap > 0) fwrite(trans.data(), sizeof(int), run < cap ? run : cap, out);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
