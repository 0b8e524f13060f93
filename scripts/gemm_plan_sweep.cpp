// Stand-alone host program: the GEMM selection (csrc/gemm_host.h gemm_select) and the work
// decode over the sweep of tests/test_gemm_plan_cpu.py, for a run under host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/gemm_plan_sweep.cpp -o gemm_plan_sweep && ./gemm_plan_sweep
// Needs no HIP runtime and no device.  Exit status 0: every plan of the sweep is well formed
// and covered exactly once; it prints the number of plans it checked.  A tool, not a test.
#include <cstdio>

#include "../deepspeech.pytorch_amd/csrc/gemm_host.h"

using namespace ds2;

int main() {
  const int mn[] = {1, 37, 128, 129, 256, 257, 300, 2400, 16032};
  const int ks[] = {1, 4, 31, 32, 36, 255, 256, 512, 1021, 1024, 1028, 5000, 16032};
  const int cus[] = {8, 64, 256, 304};
  const GemmSwitches sws[] = {{true, true}, {true, false}, {false, true}};
  long plans = 0, bad = 0;
  for (int m : mn)
    for (int n : mn)
      for (int k : ks)
        for (int batch : {1, 3})
          for (int cu : cus)
            for (int kind = 0; kind < 3; ++kind)
              for (const GemmSwitches& sw : sws)
                for (int aligned = 0; aligned < 2; ++aligned)
                  for (int wsl = 0; wsl < 3; ++wsl) {   // no workspace, 1 MB, unbounded
                    if (kind == 2 && batch != 1) continue;
                    GemmCall g{};
                    g.kind = kind;
                    g.m = m, g.n = n, g.k = k, g.batch = batch;
                    g.a = g.b = g.c = aligned ? 256 : 260;
                    g.bias = 0;
                    if (kind == 2) {
                      g.lda = g.ldb = (k + 7) / 8 * 8;
                      g.ldc = n;
                    } else if (aligned) {
                      g.lda = (k + 3) / 4 * 4, g.ldb = g.ldc = (n + 3) / 4 * 4;
                      g.stride_a = m * g.lda, g.stride_b = k * g.ldb, g.stride_c = m * g.ldc;
                    } else {
                      g.trans_a = g.trans_b = 1;
                      g.lda = m, g.ldb = k, g.ldc = n;
                      g.stride_a = (int64_t)m * k, g.stride_b = (int64_t)n * k;
                      g.stride_c = (int64_t)m * n;
                    }
                    g.have_ws = wsl > 0;
                    g.ws_bytes = wsl == 1 ? (size_t)1 << 20 : wsl == 2 ? (size_t)1 << 44 : 0;
                    const GemmChoice ch = gemm_select(g, sw, cu);
                    if (ch.status != DS2_OK) continue;
                    ++plans;
                    const GemmPlan& p = ch.p;
                    const bool ok =
                        ch.rung != DS2_GEMM_NONE && p.nsplit >= 1 &&
                        (int64_t)(p.nsplit - 1) * p.kchunk < k &&
                        k <= (int64_t)p.nsplit * p.kchunk && ch.ws_need <= g.ws_bytes &&
                        gemm_cover_defects(m, n, k, batch, p.bm, p.bn, p.main_wgs, p.tail_tile0,
                                           p.tail_tiles, p.nsplit, p.kchunk,
                                           static_cast<int>(ch.grid)) == 0;
                    if (!ok) {
                      ++bad;
                      std::fprintf(stderr, "bad plan: kind %d m %d n %d k %d batch %d cus %d\n",
                                   kind, m, n, k, batch, cu);
                    }
                  }
  std::printf("%ld plans checked, %ld bad\n", plans, bad);
  return bad == 0 ? 0 : 1;
}
