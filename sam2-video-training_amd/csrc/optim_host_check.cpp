// Stand-alone host run of the optimizer step's arithmetic (optim_elem.h): the clip pair of norm_finalize_kernel
// from a given sum of squares, the scalars of s2h_adamw and adamw_elem on every element of adamw_kernel /
// adamw_vec_kernel (optim.hip), one element after the other instead of one thread per element, over cases read
// from a file.  Built with plain g++ -O2 -ffp-contract=off (tests/test_optim_host.py; add
// -fsanitize=address,undefined for a sanitizer run), no GPU needed.  fmaf, sqrtf and / are the host's IEEE
// operations, so the output is the update the header defines, bit for bit.
//
//   optim_host_check IN OUT
// IN:  a sequence of cases, each 2 int32 {n, step} and 8 float {lr, beta1, beta2, eps, wd, sumsq, max_norm,
//      grad_scale}, then p, g, m, v of n floats each.  max_norm < 0 stands for "no clip tensor" (factor 1).
// OUT: per case 2 float clip pair {norm, factor}, 5 float {step_size, bc2_sqrt, decay, w1, omb2}, then p, m, v of
//      n floats each and n uint16 of the bf16 shadow (round to nearest even; 0x7fc0 for a NaN).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_elem.h"

namespace {

const int kMaxN = 1 << 24;

bool read_floats(FILE* in, std::vector<float>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(float), n, in) == n;
}

template <typename T>
bool write_all(FILE* out, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), out) == v.size();
}

uint16_t bf16_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr[2];
  while (fread(hdr, sizeof(int), 2, in) == 2) {
    const int n = hdr[0], step = hdr[1];
    float sc[8];
    if (n < 0 || n > kMaxN || step < 1 || fread(sc, sizeof(float), 8, in) != 8) return 3;
    const float lr = sc[0], beta1 = sc[1], beta2 = sc[2], eps = sc[3], wd = sc[4], sumsq = sc[5], max_norm = sc[6],
                grad_scale = sc[7];
    std::vector<float> p, g, m, v;
    if (!read_floats(in, p, n) || !read_floats(in, g, n) || !read_floats(in, m, n) || !read_floats(in, v, n)) return 3;
    float clip[2] = {0.f, 1.f};
    if (max_norm >= 0.f) oe_clip_pair(sumsq, max_norm, grad_scale, clip);
    const float cf = clip[1];
    const float derived[5] = {oe_step_size(lr, beta1, step), oe_bc2_sqrt(beta2, step), oe_decay(lr, wd), oe_w1(beta1),
                              oe_omb2(beta2)};
    std::vector<uint16_t> shadow((size_t)n);
    for (int i = 0; i < n; ++i) {
      adamw_elem(g[i], p[i], m[i], v[i], cf, derived[2], derived[3], beta2, derived[4], eps, derived[0], derived[1]);
      shadow[i] = bf16_bits(p[i]);
    }
    if (fwrite(clip, sizeof(float), 2, out) != 2 || fwrite(derived, sizeof(float), 5, out) != 5) return 4;
    if (!write_all(out, p) || !write_all(out, m) || !write_all(out, v) || !write_all(out, shadow)) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
