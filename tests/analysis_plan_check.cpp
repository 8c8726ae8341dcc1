// Stand-alone replay of the analysis calls' host-only plan arithmetic (csrc/tsamd_{loglik,scan,foldin,kin}_plan.h; no ROCm
// header, no GPU).  Reads one line per geometry from stdin -- a family name and its inputs -- and prints every field of the
// geometry and its *_bytes figures; the *_segments results go with the kinship geometries for each of the lengths below, and
// for the two sweeps, whose segments depend on the geometry through nseg_max alone, on `segs` lines of their own.  tests/test_analysis_plan_cpu.py
// compares the output with tests/golden/analysis_plan_parent.json, which tools/dump_analysis_plans.py recorded with this
// same program compiled against the headers of the commit named in the file.
//   loglik npad K cus test_chunk
//   scan   npad K trait cus test_chunk
//   foldin npad K n_locs cus test_segments
//   kin    m cus test_chunk test_segments
//   segs   nseg_max len
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "tsamd_foldin_plan.h"
#include "tsamd_kin_plan.h"
#include "tsamd_loglik_plan.h"
#include "tsamd_scan_plan.h"

using namespace tsamd;

// chunk lengths the kinship segments are printed for (the golden file's "lens")
static const uint32_t kLens[] = {1u, 7u, 8u, 9u, 150u, 70000u};

int main() {
  char line[256], family[16];
  while (fgets(line, sizeof line, stdin)) {
    uint32_t v[5] = {0, 0, 0, 0, 0};
    const int got = sscanf(line, "%15s %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, family, &v[0], &v[1], &v[2], &v[3], &v[4]);
    if (got == 5 && strcmp(family, "loglik") == 0) {
      const LoglikGeom g = loglik_geometry(v[0], v[1], v[2], v[3]);
      printf("%u %u %u %u %u %" PRIu64, g.ipt, g.tile_n, g.ntiles, g.nseg_max, g.chunk, loglik_scratch_bytes(g, v[0]));
    } else if (got == 6 && strcmp(family, "scan") == 0) {
      const ScanGeom g = scan_geometry(v[0], v[1], v[2] != 0u, v[3], v[4]);
      printf("%u %u %u %u %u %u %" PRIu64, g.ipt, g.tile_n, g.ntiles, g.values, g.nseg_max, g.chunk, scan_scratch_bytes(g));
    } else if (got == 6 && strcmp(family, "foldin") == 0) {
      const FoldinGeom g = foldin_geometry(v[0], v[1], v[2], v[3], v[4]);
      printf("%u %u %u %u %u %u %" PRIu64 " %" PRIu64, g.ipt, g.tile_n, g.ntiles, g.batch, g.nseg, g.seg_len, foldin_scratch_bytes(g, v[0], v[1]),
             foldin_scratch_bound(v[0], v[1]));
    } else if (got == 5 && strcmp(family, "kin") == 0) {
      const KinGeom g = kin_geometry(v[0], v[1], v[2], v[3]);
      printf("%u %u %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64, g.mpad, g.ntiles, g.npairs, g.nseg_max, g.pairs_per_launch, g.chunk,
             kin_rs_bytes(g), kin_part_bytes(g), kin_acc_bytes(g));
      for (uint32_t len : kLens) {
        const KinSegs s = kin_segments(g, len);
        printf(" %u %u %u", s.steps, s.nseg, s.seg_steps);
      }
    } else if (got == 3 && strcmp(family, "segs") == 0) {
      LoglikGeom gl = loglik_geometry(512, 1, 1, 0);
      ScanGeom gs = scan_geometry(512, 1, false, 1, 0);
      gl.nseg_max = gs.nseg_max = v[0];
      const LoglikSegs sl = loglik_segments(gl, v[1]);
      const ScanSegs ss = scan_segments(gs, v[1]);
      printf("%u %u %u %u", sl.nseg, sl.seg_len, ss.nseg, ss.seg_len);
    } else {
      fprintf(stderr, "bad input line (%d fields): %s", got, line);
      return 2;
    }
    printf("\n");
  }
  return 0;
}
