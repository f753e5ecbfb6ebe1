// Stand-alone host run of the dataset-preparation kernels' decomposition (dataprep.h): the histogram's chunks,
// lanes and steps, the staged transpose's bands, load items, swizzled tile and 64-word wave chunks, and the
// direct form's blocks -- label_hist_kernel, label_planes_staged_kernel and label_planes_direct_kernel of
// dataprep.hip, one workgroup after the other and one lane after the other instead of one thread each, over
// cases read from a file.  The tile and the outputs are allocated at exactly the size the kernels are given,
// so a sanitizer sees any index past them; every output word is counted, so a word written twice or never is
// an error.  Built with plain g++ (tests/test_dataprep_host.py; add -fsanitize=address,undefined for a
// sanitizer run), no GPU needed.
//
//   dataprep_host_check IN OUT
// IN:  a sequence of cases, each 4 int32 {F, H, W, P}, F * H * W label bytes, F + 1 int32 frame_off, P int32
//      plane_class.
// OUT: per case F * 256 int32 of histogram, then P * ceil(H W / 64) uint64 of plane words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dataprep.h"

namespace {

void hist_model(int F, int HW, const uint8_t* labels, std::vector<int>& hist) {
  const int nch = dp_hist_chunks(HW);
  for (long long blk = 0; blk < (long long)F * nch; ++blk) {
    const int f = (int)(blk / nch), c = (int)(blk - (long long)f * nch);
    const uint8_t* img = labels + (size_t)f * HW;
    int sh[256] = {0};
    for (int t = 0; t < DP_BLOCK; ++t)
      for (int s = 0; s < DP_HIST_STEPS; ++s) {
        const int o = dp_hist_offset(c, s, t);
        if (o >= HW) continue;
        const int n = HW - o < DP_HIST_LANE_BYTES ? HW - o : DP_HIST_LANE_BYTES;
        int cur = img[o], run = 0;
        for (int k = 0; k < n; ++k) {
          const int v = img[o + k];
          if (v != cur) {
            sh[cur] += run;
            cur = v;
            run = 0;
          }
          ++run;
        }
        sh[cur] += run;
      }
    for (int t = 0; t < 256; ++t)
      if (sh[t]) hist[(size_t)f * 256 + t] += sh[t];
  }
}

// returns 0, or 5 when a word is written outside its plane's row or not exactly once
int planes_model(int F, int H, int W, const uint8_t* labels, int P, const int* frame_off, const int* plane_class,
                 std::vector<uint64_t>& bits) {
  const int nw = dp_words(H, W), HW = H * W;
  std::vector<unsigned char> written(bits.size(), 0);
  std::vector<unsigned char> owned((size_t)P, 0);  // planes some frame lists
  auto store = [&](int p, int word, uint64_t m) {
    if (p < 0 || p >= P || word < 0 || word >= nw) return false;
    const size_t at = (size_t)p * nw + word;
    bits[at] = m;
    return ++written[at] == 1;
  };
  if (dp_staged(H)) {
    const int nb = dp_bands(W);
    std::vector<uint32_t> tile((size_t)dp_tile_dwords(H));  // the LDS the launch asks for
    for (long long blk = 0; blk < (long long)F * nb; ++blk) {
      const int f = (int)(blk / nb), b = (int)(blk - (long long)f * nb);
      int p0, p1;
      dp_frame_planes(frame_off, f, P, &p0, &p1);
      if (p1 <= p0) continue;
      for (int p = p0; p < p1; ++p) owned[p] = 1;
      const int cols = dp_band_cols(b, W);
      const uint8_t* img = labels + (size_t)f * HW + b * DP_BAND;
      for (int i = 0; i < 4 * H; ++i) {  // (thread i % DP_BLOCK, round i / DP_BLOCK)
        int r, seg;
        dp_load_item(i, &r, &seg);
        const int c0 = seg * 16;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < 16; ++k)
          if (c0 + k < cols) q[k >> 2] |= (uint32_t)img[(size_t)r * W + c0 + k] << (8 * (k & 3));
        for (int k = 0; k < 4; ++k) tile.at((size_t)dp_tile_dword(r, seg * 4 + k)) = q[k];
      }
      const uint8_t* t8 = reinterpret_cast<const uint8_t*>(tile.data());
      const size_t t8n = tile.size() * 4;
      const int nbw = dp_band_words(b, H, W), w0 = dp_band_word0(b, H);
      for (int wave = 0; wave < DP_BLOCK / 64; ++wave)
        for (int base = wave * 64; base < nbw; base += (DP_BLOCK / 64) * 64)
          for (int p = p0; p < p1; ++p) {
            const int cls = plane_class[p];
            for (int i = 0; i < 64; ++i) {  // word base + i: the ballot over the 64 lanes, kept by lane i
              uint64_t m = 0;
              for (int lane = 0; lane < 64; ++lane) {
                int r, c;
                if (base + i < nbw && dp_word_pos(base + i, lane, H, cols, &r, &c)) {
                  const size_t at = (size_t)dp_tile_byte(r, c);
                  if (at >= t8n) return 5;
                  if (dp_bit(t8[at], cls)) m |= 1ull << lane;
                }
              }
              const int w = base + i;  // (lane i's store)
              if (w < nbw && w0 + w < nw && !store(p, w0 + w, m)) return 5;
            }
          }
    }
  } else {
    const int nblk = (HW + DP_BLOCK - 1) / DP_BLOCK;
    for (long long blk = 0; blk < (long long)F * nblk; ++blk) {
      const int f = (int)(blk / nblk), bk = (int)(blk - (long long)f * nblk);
      int p0, p1;
      dp_frame_planes(frame_off, f, P, &p0, &p1);
      if (p1 <= p0) continue;
      for (int p = p0; p < p1; ++p) owned[p] = 1;
      for (int wave = 0; wave < DP_BLOCK / 64; ++wave)
        for (int p = p0; p < p1; ++p) {
          uint64_t m = 0;
          for (int lane = 0; lane < 64; ++lane) {
            const int j = bk * DP_BLOCK + wave * 64 + lane;
            const bool in = j < HW;
            const int jj = in ? j : HW - 1;
            const int x = jj / H, y = jj - x * H;
            const int v = labels[(size_t)f * HW + (size_t)y * W + x];
            if (in && dp_bit(v, plane_class[p])) m |= 1ull << lane;
          }
          const int word = (bk * DP_BLOCK + wave * 64) >> 6;
          if (word < nw && !store(p, word, m)) return 5;
        }
    }
  }
  for (int p = 0; p < P; ++p)
    for (int w = 0; w < nw; ++w)
      if (written[(size_t)p * nw + w] != owned[p]) return 5;
  // bits past H W are zero
  if (HW % 64)
    for (int p = 0; p < P; ++p)
      if (bits[(size_t)p * nw + nw - 1] >> (HW % 64)) return 5;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr[4];
  while (fread(hdr, sizeof(int), 4, in) == 4) {
    const int F = hdr[0], H = hdr[1], W = hdr[2], P = hdr[3];
    if (dp_total(F, H, W) < 0 || dp_total(P, H, W) < 0) return 3;
    const size_t n = (size_t)F * H * W;
    std::vector<uint8_t> labels(n);
    std::vector<int> frame_off((size_t)F + 1), plane_class((size_t)P);
    if (n && fread(labels.data(), 1, n, in) != n) return 3;
    if (fread(frame_off.data(), sizeof(int), frame_off.size(), in) != frame_off.size()) return 3;
    if (P && fread(plane_class.data(), sizeof(int), plane_class.size(), in) != plane_class.size()) return 3;
    // the layout the kernel is promised: CSR ascending from 0 to P
    if (frame_off[0] != 0 || frame_off[F] != P) return 3;
    for (int f = 0; f < F; ++f)
      if (frame_off[f + 1] < frame_off[f]) return 3;
    std::vector<int> hist((size_t)F * 256, 0);
    if (F) hist_model(F, H * W, labels.data(), hist);
    std::vector<uint64_t> bits((size_t)P * dp_words(H, W), 0ull);
    if (P) {
      const int rc = planes_model(F, H, W, labels.data(), P, frame_off.data(), plane_class.data(), bits);
      if (rc) return rc;
    }
    if (!hist.empty()) fwrite(hist.data(), sizeof(int), hist.size(), out);
    if (!bits.empty()) fwrite(bits.data(), sizeof(uint64_t), bits.size(), out);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
