// Stand-alone host run of the threshold sweep's counting (sweep_hist.h): the bin index and the per-wave and
// per-workgroup folding of mask_sweep_kernel (rle.hip) in the same decomposition -- workgroups of SWEEP_BLOCK
// pixels, waves of 64 pixels = one ground-truth word, categories one after the other through the same
// workgroup counts -- one lane after the other instead of one thread per pixel, over cases read from a file.
// Built with plain g++ (tests/test_threshold_sweep_host.py; add -fsanitize=address,undefined for a sanitizer
// run), no GPU needed.
//
//   sweep_host_check IN OUT
// IN:  a sequence of cases, each 5 int32 {Ncat, H, W, K, has_gt}, K fp32 cuts, Ncat * H W fp32 merged values
//      (per category, pixels in column-major order j = x * H + y) and, when has_gt, Ncat * ceil(H W / 64)
//      uint64 ground-truth words (bits past H W in a last word may hold anything).
// OUT: per case Ncat * 2 * (K + 1) int32 of histogram.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sweep_hist.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr5[5];
  while (fread(hdr5, sizeof(int), 5, in) == 5) {
    const int Ncat = hdr5[0], H = hdr5[1], W = hdr5[2], K = hdr5[3], has_gt = hdr5[4];
    if (Ncat < 0 || H < 1 || W < 1 || K < 1 || K > SWEEP_MAX_K || (long long)H * W > (1 << 24) ||
        (long long)Ncat * H * W > (1 << 28))
      return 3;
    const int n = H * W, nw = (n + 63) / 64, nb = (n + SWEEP_BLOCK - 1) / SWEEP_BLOCK;
    std::vector<float> cuts(K), m((size_t)Ncat * n);
    std::vector<uint64_t> gt(has_gt ? (size_t)Ncat * nw : 0);
    if (fread(cuts.data(), sizeof(float), K, in) != (size_t)K) return 3;
    if (!m.empty() && fread(m.data(), sizeof(float), m.size(), in) != m.size()) return 3;
    if (!gt.empty() && fread(gt.data(), sizeof(uint64_t), gt.size(), in) != gt.size()) return 3;
    // buffers of exactly the sizes the kernel indexes (a sanitizer sees an access past them)
    std::vector<int> hist((size_t)Ncat * 2 * (K + 1), 0), blk(2 * (K + 1), 0);
    for (int blockIdx = 0; blockIdx < nb; ++blockIdx) {
      for (int c = 0; c < Ncat; ++c) {
        for (int wave = 0; wave < SWEEP_BLOCK / 64; ++wave) {
          const int word = (blockIdx * SWEEP_BLOCK + wave * 64) >> 6;
          const uint64_t valid = sweep_valid(word, n);  // the ballot of "this lane is a pixel"
          const uint64_t g = (has_gt && valid) ? gt[(size_t)c * nw + word] : 0ull;
          for (int q = 0; q <= K; ++q) {
            uint64_t sel = 0;  // the ballot of "this lane is a pixel of bin q"
            for (int lane = 0; lane < 64; ++lane) {
              if (!((valid >> lane) & 1ull)) continue;
              const int j = word * 64 + lane;
              if (sweep_bin(m[(size_t)c * n + j], cuts.data(), K) == q) sel |= 1ull << lane;
            }
            if (sel) sweep_block_add(blk.data(), K, q, sweep_word_counts(sel, g));
          }
        }
        for (int tid = 0; tid < SWEEP_BLOCK; ++tid)
          sweep_block_flush(hist.data() + (size_t)c * 2 * (K + 1), blk.data(), K, tid, SWEEP_BLOCK);
      }
    }
    if (!hist.empty()) fwrite(hist.data(), sizeof(int), hist.size(), out);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
