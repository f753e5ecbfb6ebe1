// Offline scoring from COCO RLE runs (s2h_rle_pair_counts, rle.hip): per group -- one (image, category) pair --
// the counts |p & g|, |p | g|, |p|, |g| of the OR of its predicted and of its ground-truth annotations,
// straight from the run boundaries.  A wave of 64 lanes is one word of 64 column-major positions: a lane
// finds its position's bit in every annotation of a side by the binary search of s2h_rle_decode
// (gtprompt.h gp_run_index), the ballot of the lanes is the word of the OR-ed mask, and four popcounts of
// the two words are the word's contribution.  No mask is stored anywhere.  Plain functions that compile for
// the device and for the host: pair_counts_host_check.cpp runs them sequentially in the kernel's
// decomposition.  Integer arithmetic only; every loop has a bound that does not depend on the data.
#pragma once
#include "gtprompt.h"

#define PC_BLOCK 256                  // threads of a workgroup = PC_BLOCK / 64 words
#define PC_MAX_GROUP_ANNS (1 << 12)   // annotations per group and side that are read (the launcher's caller checks)

// the bit of column-major position pos in the OR of annotations [a0, a1): run_off / run_end as for
// s2h_rle_decode.  At most PC_MAX_GROUP_ANNS searches of at most 32 steps.
GP_HD bool pc_side_bit(const int* run_off, const int* run_end, int a0, int a1, int pos) {
  bool bit = false;
  for (int k = 0; k < PC_MAX_GROUP_ANNS && a0 + k < a1; ++k) {
    const int o = run_off[a0 + k];
    const int n = run_off[a0 + k + 1] - o;
    bit = bit || ((gp_run_index(run_end + o, n < 0 ? 0 : n, pos) & 1) != 0);
  }
  return bit;
}

// the positions of word `word` that lie inside the n positions of the image
GP_HD uint64_t pc_valid(int word, int n) {
  const int rest = n - word * 64;
  return rest >= 64 ? ~0ull : (rest <= 0 ? 0ull : (1ull << rest) - 1ull);
}

struct PcCounts {
  int inter, uni, np, ng;
};
// one word's counts from the ballots of the two sides
GP_HD PcCounts pc_word_counts(uint64_t p, uint64_t g) {
  const PcCounts c = {gp_popc(p & g), gp_popc(p | g), gp_popc(p), gp_popc(g)};
  return c;
}
