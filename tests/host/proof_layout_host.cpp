// Prints what sonic_amd/csrc/proof_layout.hpp and share_plan.hpp::share_line say, for tests/test_proof_layout_host.py: every named slot,
// evaluation, transcript and pair index, the evaluation -> slot owner map, the byte offset of every field proof_layout() writes, and
// the work line.  Plain g++, no HIP.
#include <stdio.h>
#include <vector>
#include "../../sonic_amd/csrc/share_plan.hpp"

using namespace sonic;

int main() {
  for (long Q : {1L, 2L, 5L}) {
    const ProofLayout L{Q};
    printf("Q %ld\n", Q);
    printf("count K %ld\ncount F %ld\ncount slots_total %ld\ncount transcript_len %ld\ncount n_pairs %ld\ncount proof_bytes %zu\n", L.K(), L.F(),
           L.slots_total(), L.transcript_len(), L.n_pairs(), L.proof_bytes());
    printf("slot R %ld\nslot T %ld\nslot Wa %ld\nslot Wb %ld\nslot Wt %ld\nslot Qv %ld\nslot C %ld\nside C_extra %ld\n", L.R, L.T, L.Wa, L.Wb, L.Wt, L.Qv(), L.C(), L.C_extra());
    printf("eval a %ld\neval b %ld\neval s %ld\n", L.a, L.b, L.s);
    printf("tr y %ld\ntr z %ld\ntr u %ld\ntr v %ld\ntr n_blinders %ld\n", L.y, L.z, L.u(), L.v(), L.n_blinders);
    printf("pair pY %ld\npair pZ %ld\npair pYZ %ld\npair pU %ld\npair pV %ld\n", L.pY, L.pZ, L.pYZ, L.pU, L.pV);
    for (long j = 0; j < Q; j++) {
      printf("slot S%ld %ld\nslot W%ld %ld\nslot Wp%ld %ld\nslot Qj%ld %ld\nside S_extra%ld %ld\n", j, L.S(j), j, L.W(j), j, L.Wp(j), j, L.Qj(j), j, L.S_extra(j));
      printf("eval s_j%ld %ld\neval sp_j%ld %ld\n", j, L.s_j(j), j, L.sp_j(j));
      printf("tr y_j%ld %ld\ntr z_j%ld %ld\npair pYj%ld %ld\npair pZj%ld %ld\n", j, L.y_j(j), j, L.z_j(j), j, L.pYj(j), j, L.pZj(j));
    }
    for (long i = 0; i < L.F(); i++) printf("owner %ld %ld\n", i, L.eval_owner_slot(i));
    // every input block of proof_layout() carries its kind and index; the output is then walked field by field
    std::vector<uint8_t> pts(96 * (size_t)L.K(), 0), frs(32 * (size_t)L.F(), 0), tr(32 * (size_t)L.transcript_len(), 0), out(L.proof_bytes(), 0);
    for (long i = 0; i < L.K(); i++) { pts[96 * i] = 'G'; pts[96 * i + 1] = (uint8_t)i; }
    for (long i = 0; i < L.F(); i++) { frs[32 * i] = 'F'; frs[32 * i + 1] = (uint8_t)i; }
    for (long i = 0; i < L.transcript_len(); i++) { tr[32 * i] = 'T'; tr[32 * i + 1] = (uint8_t)i; }
    proof_layout(Q, pts.data(), frs.data(), tr.data(), out.data());
    for (size_t at = 0; at < out.size(); at += out[at] == 'G' ? 96 : 32) printf("field %zu %c %d\n", at, out[at], (int)out[at + 1]);
    for (long n : {1L, 16L, 257L})
      for (int prepared = 0; prepared < 2; prepared++)
        for (const ShareItem& it : share_line(n, Q, prepared != 0)) printf("line %ld %d %d %ld\n", n, prepared, it.slot, it.terms);
  }
  return 0;
}
