// Stand-alone host run of the offline scoring's counting (pair_counts.h): the per-position search, the
// ballots and the per-word counts of rle_pair_counts_kernel (rle.hip) in the same decomposition -- one
// workgroup of PC_BLOCK / 64 words per (group, block), waves of 64 positions, the workgroup's sums added to
// the group's counts -- one lane after the other instead of one thread per position, over cases read from a
// file.  Built with plain g++ (tests/test_pair_counts_host.py; add -fsanitize=address,undefined for a
// sanitizer run), no GPU needed.
//
//   pair_counts_host_check IN OUT
// IN:  a sequence of cases, each 3 int32 {G, H, W}, then per side (predicted, ground truth): G + 1 int32
//      grp_off, grp_off[G] + 1 int32 run_off, run_off[last] int32 run_end.
// OUT: per case G * 4 uint64 of counts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pair_counts.h"

namespace {

struct Side {
  std::vector<int> grp_off, run_off, run_end;
};

bool read_ints(FILE* in, std::vector<int>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(int), n, in) == n;
}

// the layout the kernel trusts: ascending offsets from 0 (a sanitizer sees any access past the buffers)
bool read_side(FILE* in, int G, int HW, Side& s) {
  if (!read_ints(in, s.grp_off, (size_t)G + 1) || s.grp_off[0] != 0) return false;
  for (int g = 0; g < G; ++g)
    if (s.grp_off[g + 1] < s.grp_off[g]) return false;
  const int A = s.grp_off[G];
  if (!read_ints(in, s.run_off, (size_t)A + 1) || s.run_off[0] != 0) return false;
  for (int a = 0; a < A; ++a)
    if (s.run_off[a + 1] < s.run_off[a]) return false;
  if (!read_ints(in, s.run_end, (size_t)s.run_off[A])) return false;
  for (int e : s.run_end)
    if (e < 0 || e > HW) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr[3];
  while (fread(hdr, sizeof(int), 3, in) == 3) {
    const int G = hdr[0], H = hdr[1], W = hdr[2];
    if (G < 0 || H < 1 || W < 1 || (long long)H * W > GP_MAX_PIXELS || (long long)G * H * W + 256 > 0x7fffffffLL)
      return 3;
    const int HW = H * W, nw = (HW + 63) / 64, waves = PC_BLOCK / 64, nbw = (nw + waves - 1) / waves;
    Side dt, gt;
    if (!read_side(in, G, HW, dt) || !read_side(in, G, HW, gt)) return 3;
    std::vector<unsigned long long> counts((size_t)G * 4, 0ull);
    for (int blk = 0; blk < G * nbw; ++blk) {
      const int g = blk / nbw, b = blk - g * nbw;
      const int d0 = dt.grp_off[g], d1 = dt.grp_off[g + 1], g0 = gt.grp_off[g], g1 = gt.grp_off[g + 1];
      if (d1 <= d0 && g1 <= g0) continue;
      int red[PC_BLOCK / 64][4];
      for (int wave = 0; wave < waves; ++wave) {
        uint64_t p = 0, q = 0;  // the ballots
        for (int lane = 0; lane < 64; ++lane) {
          const int pos = (b * waves + wave) * 64 + lane;
          const bool inside = pos < HW;
          if (inside && pc_side_bit(dt.run_off.data(), dt.run_end.data(), d0, d1, pos)) p |= 1ull << lane;
          if (inside && pc_side_bit(gt.run_off.data(), gt.run_end.data(), g0, g1, pos)) q |= 1ull << lane;
        }
        if ((p | q) & ~pc_valid(b * waves + wave, HW)) return 5;  // a bit past the image
        const PcCounts c = pc_word_counts(p, q);
        red[wave][0] = c.inter;
        red[wave][1] = c.uni;
        red[wave][2] = c.np;
        red[wave][3] = c.ng;
      }
      for (int t = 0; t < 4; ++t) {
        int v = 0;
        for (int w = 0; w < waves; ++w) v += red[w][t];
        if (v) counts[(size_t)g * 4 + t] += (unsigned long long)v;
      }
    }
    if (!counts.empty()) fwrite(counts.data(), sizeof(unsigned long long), counts.size(), out);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
