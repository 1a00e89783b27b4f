// Host program of tests/test_decode_form.py: prints what dc_tts_amd/csrc/decode_form.h resolves.
//   no argument:   every input of the enumeration as "<packed form> <key>" (the order and the packing of tests/golden/decode_form_parent.txt), the line "team_u",
//                  then "<packed form> <key>" for B in (1, 8, 9, 16, 17, 32, 33) x merged form or not x DCTTS_XGROUP=2 or not
//   ten arguments: chain_tail xgroup xcone sync_values chain_wait prof_id xgroup_ok can_stream_wait_value capability_set B -> that form, one "name=value" per field
//   one argument:  an environment value of DCTTS_CHAIN_TAIL -> 1 if it names a form
#include <cstdio>
#include <cstdlib>

#include "../dc_tts_amd/csrc/decode_form.h"

static DecodeCaps caps(int set, int prof, bool ok, bool can) {      // 0 = the standard networks, 1 = a cone tail that is not 5 / 3 / 1, 2 = no 16-row packing of C_1's Q half
  DecodeCaps c;
  c.xgroup_ok = ok; c.can_stream_wait_value = can; c.prof_id = prof;
  c.std_cone_tail = set != 1; c.c1q_wp16 = set != 2;
  return c;
}
static DecodeKnobs knobs(int ct, int xg, int xc, int sv, int cw) {
  DecodeKnobs k;
  k.chain_tail = (ChainTail)ct; k.xgroup = xg; k.xcone = xc; k.sync_values = sv; k.chain_wait_inkernel = cw;
  return k;
}
static unsigned packed(const DecodeForm& f) {
  return (unsigned)f.counters | (unsigned)f.chain_signals_inkernel << 1 | (unsigned)f.chain_waits_inkernel << 2 | (unsigned)f.side_signals_inkernel << 3 | (unsigned)f.xgroup_on << 4 |
         (unsigned)f.xcone_on << 5 | (unsigned)f.xtail_on << 6 | (unsigned)f.xmlp_on << 7 | (unsigned)f.dec_merged << 8 | (unsigned)f.attn_fold << 9 | (unsigned)f.one_launch << 10 |
         (unsigned)f.side_fold << 11 | (unsigned)f.c1qw_on_chain << 12 | (unsigned)f.passengers << 13 | (unsigned)f.np << 14 | (unsigned)f.team_u << 17;
}

int main(int argc, char** argv) {
  if (argc == 2) { printf("%d\n", (int)chain_tail_known(atoi(argv[1]))); return 0; }
  if (argc == 11) {
    int a[10]; for (int i = 0; i < 10; ++i) a[i] = atoi(argv[i + 1]);
    const DecodeForm f = resolve_decode_form(knobs(a[0], a[1], a[2], a[3], a[4]), caps(a[8], a[5], a[6] != 0, a[7] != 0), a[9]);
    printf("counters=%d\nchain_signals_inkernel=%d\nchain_waits_inkernel=%d\nside_signals_inkernel=%d\nxgroup_on=%d\nxcone_on=%d\nxtail_on=%d\nxmlp_on=%d\ndec_merged=%d\nnp=%d\nteam_u=%d\n"
           "attn_fold=%d\none_launch=%d\nside_fold=%d\nc1qw_on_chain=%d\npassengers=%d\n", f.counters, f.chain_signals_inkernel, f.chain_waits_inkernel, f.side_signals_inkernel, f.xgroup_on,
           f.xcone_on, f.xtail_on, f.xmlp_on, f.dec_merged, f.np, f.team_u, f.attn_fold, f.one_launch, f.side_fold, f.c1qw_on_chain, f.passengers);
    return 0;
  }
  const int cts[6] = {0, 1, 2, 5, 6, 7};
  const int profs[3] = {-1, DCTTS_PROF_CHAIN_HC, DCTTS_PROF_BULK_GEMM};
  for (int ct : cts) for (int xg = 0; xg < 3; ++xg) for (int xc = 0; xc < 3; ++xc) for (int sv = 0; sv < 2; ++sv) for (int cw = 0; cw < 2; ++cw)
    for (int prof : profs) for (int ok = 0; ok < 2; ++ok) for (int can = 0; can < 2; ++can) for (int cs = 0; cs < 3; ++cs) {
      const DecodeForm f = resolve_decode_form(knobs(ct, xg, xc, sv, cw), caps(cs, prof, ok != 0, can != 0), 3);
      printf("%u %s\n", packed(f), f.key().c_str());
    }
  printf("team_u\n");
  const int Bs[7] = {1, 8, 9, 16, 17, 32, 33};
  for (int B : Bs) for (int merged = 0; merged < 2; ++merged) for (int four = 0; four < 2; ++four) {
    const DecodeForm f = resolve_decode_form(knobs(merged ? 2 : 5, four ? 2 : 1, 1, 1, 1), caps(0, -1, true, true), B);
    if (f.dec_merged != (merged != 0)) return 1;
    printf("%u %s\n", packed(f), f.key().c_str());
  }
  return 0;
}
