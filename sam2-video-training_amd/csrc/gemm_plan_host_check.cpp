// Stand-alone host run of the GEMM dispatch (gemm_plan.h): one plan per case of a text file.  Built with plain
// g++ (tests/test_gemm_plan_host.py; add -fsanitize=address,undefined for a sanitizer run), no GPU needed.
//
//   gemm_plan_host_check IN OUT
// IN:  one case per line, whitespace-separated numbers:
//        the problem   batch M N K  a_kc a_rc b_kc b_rc  f32_in f32_out  bias R X cscale dropout act beta
//                      rowsum rope  lda ldb a16 b16 sa8 sb8                                          (25)
//        the knobs     cfg dbg tiny_cfg w41 areg class_cfg[0..5] tiny_splitk split_target f32_small
//                      wg_kmin wg_force_tile wg_force_splits                                         (17)
//        the registered workspace's bytes (0: none)                                                  (1)
// OUT: one plan per line:
//        kind cfg BM BN WGM WGN NS BK splits kchunk use_ws atomic zero_c ws_floats wg_tile Md Nd sl tag
// Exit status 3: a malformed line.
#include <cinttypes>
#include <cstdio>

#include "gemm_plan.h"

namespace {

bool read_flag(FILE* in, bool& v) {
  int t;
  if (fscanf(in, "%d", &t) != 1 || (t != 0 && t != 1)) return false;
  v = t != 0;
  return true;
}

// 1: a case was read, 0: end of file, -1: malformed
int read_case(FILE* in, GemmProblem& p, GemmKnobs& k, int64_t& ws_bytes) {
  const int first = fscanf(in, "%d", &p.batch);
  if (first == EOF) return 0;
  bool ok = first == 1 && fscanf(in, "%d %d %d", &p.M, &p.N, &p.K) == 3;
  ok = ok && read_flag(in, p.a_kc) && read_flag(in, p.a_rc) && read_flag(in, p.b_kc) && read_flag(in, p.b_rc);
  ok = ok && read_flag(in, p.f32_in) && read_flag(in, p.f32_out);
  ok = ok && read_flag(in, p.bias) && read_flag(in, p.R) && read_flag(in, p.X) && read_flag(in, p.cscale) &&
       read_flag(in, p.dropout);
  ok = ok && fscanf(in, "%d %f", &p.act, &p.beta) == 2 && read_flag(in, p.rowsum) && read_flag(in, p.rope);
  ok = ok && fscanf(in, "%" SCNd64 " %" SCNd64, &p.lda, &p.ldb) == 2;
  ok = ok && read_flag(in, p.a16) && read_flag(in, p.b16) && read_flag(in, p.sa8) && read_flag(in, p.sb8);
  ok = ok && fscanf(in, "%d %d %d %d %d", &k.cfg, &k.dbg, &k.tiny_cfg, &k.w41, &k.areg) == 5;
  for (int c = 0; ok && c < 6; ++c) ok = fscanf(in, "%d", &k.class_cfg[c]) == 1;
  ok = ok && fscanf(in, "%d %d %d %d %d %d", &k.tiny_splitk, &k.split_target, &k.f32_small, &k.wg_kmin,
                    &k.wg_force_tile, &k.wg_force_splits) == 6;
  ok = ok && fscanf(in, "%" SCNd64, &ws_bytes) == 1;
  // the callers' guarantees (s2h_gemm): positive extents, a positive split target, every pitch positive
  ok = ok && p.batch > 0 && p.M > 0 && p.N > 0 && p.K >= 0 && p.lda > 0 && p.ldb > 0 && k.split_target > 0 &&
       ws_bytes >= 0;
  return ok ? 1 : -1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  for (;;) {
    GemmProblem p = {};
    GemmKnobs k;
    int64_t ws_bytes = 0;
    const int rc = read_case(in, p, k, ws_bytes);
    if (rc == 0) break;
    if (rc < 0) return 3;
    const GemmPlan pl = gemm_plan(p, k, ws_bytes);
    const GemmTile& t = pl.tile;
    fprintf(out, "%d %d %d %d %d %d %d %d %d %d %d %d %d %" PRId64 " %d %d %d %d %" PRId64 "\n", pl.kind, pl.cfg, t.BM,
            t.BN, t.WGM, t.WGN, t.NS, t.BK, pl.splits, pl.kchunk, (int)pl.use_ws, (int)pl.atomic, (int)pl.zero_c,
            pl.ws_floats, pl.wg_tile, pl.Md, pl.Nd, pl.sl, pl.tag);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
