// Host build of the blocked band kernel's LDS layout and choice of form (openmcmc_amd/csrc/omc_band_common.h) for the CPU test suite.
//   hipcc -x hip --cuda-host-only -O2 -I include -I openmcmc_amd/csrc tests/native/band_layout_host.hip -o <exe>
// stdout, one record per line:
//   F NB NT MT WPE wmax wgs_per_cu                      every instantiation of k_band_blocked
//   M FAIL ZERO DUMP COUNTER MISC_SLOTS                 the named slots of misc
//   L w NB NT  W1 WS WP PS FBS  ring rring Ld P dv Us misc fwd_end  WB xs ms Sx Sm Lb Part dump diag bwd_end  bytes
//   S w n_terms n_chains forced  NB NT MT WPE           the selector's answer with 256 CUs (NB = 0: none fits)
#include <stdio.h>

#include "omc_band_common.h"

int main() {
#define PRINT_FORM(NB, NT, MT, WPE) \
  printf("F %d %d %d %d %d %d\n", NB, NT, MT, WPE, BandBlockedForm{NB, NT, MT, WPE}.wmax(), BandBlockedForm{NB, NT, MT, WPE}.wgs_per_cu());
  BAND_BLOCKED_FORMS(PRINT_FORM)
  printf("M %d %d %d %d %d\n", BandBlockedLds::FAIL, BandBlockedLds::ZERO, BandBlockedLds::DUMP, BandBlockedLds::COUNTER, BandBlockedLds::MISC_SLOTS);
  const int pairs[4][2] = {{16, 256}, {8, 256}, {8, 512}, {16, 512}};
  for (int w = 1; w <= 128; ++w)
    for (const auto& p : pairs) {
      const BandBlockedLds l(w, p[0], p[1]);
      printf("L %d %d %d  %d %d %d %d %d  %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d  %zu\n", w, p[0], p[1], l.W1, l.WS, l.WP, l.PS,
             l.FBS, l.ring, l.rring, l.Ld, l.P, l.dv, l.Us, l.misc, l.fwd_end, l.WB, l.xs, l.ms, l.Sx, l.Sm, l.Lb, l.Part, l.dump, l.diag,
             l.bwd_end, l.bytes());
    }
  const int chains[5] = {256, 257, 768, 769, 1024}, forced[5] = {0, 4, 8, 16, 512};
  for (int w = 0; w <= 129; ++w)
    for (int nt = 1; nt <= 4; ++nt)
      for (int c : chains)
        for (int f : forced) {
          const BandBlockedForm g = band_blocked_choose(w, nt, c, 256, f);
          printf("S %d %d %d %d  %d %d %d %d\n", w, nt, c, f, g.NB, g.NT, g.MT, g.WPE);
        }
  return 0;
}
