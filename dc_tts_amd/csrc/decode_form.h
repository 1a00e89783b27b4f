// decode_form.h -- which launch form a two-stream decode (decode_host.h: decode_v3) takes, stated in one place: what was asked for (DecodeKnobs), what this
// context and device can do (DecodeCaps), and the form that follows (DecodeForm, resolve_decode_form).  Host only: no HIP header, no context struct; a plain
// C++17 compiler builds it (tests/test_decode_form.py does).  The measurements behind every form are in DESIGN.md section 2 and DESIGN_HISTORY.md.
#pragma once

#include <string>

#include "../../include/dctts_hip_debug.h"      // DCTTS_PROF_*: two of the timing ids need the per-layer launches they look at

// How the chain runs a piece (DCTTS_CHAIN_TAIL; the numbers are the environment's).  3 and 4 were round-4 A/B forms: measured, documented, removed.
enum class ChainTail {
  MlpRows = 0,           // round 2: AudioDec's newest-row layers as xgroup_kernel, the seven k = 1 layers around the mel frame in mlp_rows_kernel (split by rows)
  XMlp = 1,              // ... the k = 1 layers in team form (xmlp_kernel); HC_5 .. HC_7 stay split between the chain's run and the side stream
  OneLaunch = 2,         // default: the whole chain piece as ONE launch (xchain_kernel) -- xtail_kernel's layers (AudioDec's FOUR newest-row layers HC_2 .. HC_5, then HC_6, HC_7
                         //   over the 3 / 1 cone rows they need, then the seven k = 1 layers), a team barrier, xgroup_kernel's AudioEnc run + attention + AudioDec C_1
  TailBehindXgroup = 5,  // the first round-4 form, three launches: HC_2 .. HC_4 as an xgroup_kernel launch, xtail_kernel (HC_5 .. HC_7 + the k = 1 layers), the AudioEnc run
  TwoLaunches = 6,       // round 4: the two parts of OneLaunch as launches of their own (xtail_kernel, xgroup_kernel); how the parts are timed alone
  OneLaunchNP3 = 7,      // OneLaunch with round 5's split of the cone: THREE newest-row layers in front, HC_5 .. HC_7 over 5 / 3 / 1 cone rows on the chain, the side stream stops behind HC_4
};
inline bool chain_tail_known(int v) { return v == 0 || v == 1 || v == 2 || v == 5 || v == 6 || v == 7; }

// What the user or the environment asked for (tools/README.md).  Persistent in the context; one decode may run on a modified copy (dctts_decode_safe_once).
struct DecodeKnobs {
  ChainTail chain_tail = ChainTail::OneLaunch;
  int xgroup = 1;                // DCTTS_XGROUP: runs of the chain's highway layers as one launch whose workgroups meet inside one XCD (xgroup_kernel.h); 0: one chain3_kernel launch per
                                 //   layer; 2: the team kernels with FOUR utterances per team and round whatever the batch (A/B, tests)
  int xcone = 1;                 // DCTTS_XCONE: the side stream's piece as ONE launch (xcone_kernel.h); 2: three (rowc1_kernel, rowhc2_kernel, xcone_kernel: rounds 3-4); 0: one per layer
  int sync_values = 1;           // DCTTS_SYNC_VALUES: the two streams meet through two counters; 0: through events (what rocprofv3 --pmc needs: read_env)
  int chain_wait_inkernel = 1;   // DCTTS_CHAIN_WAIT: waits and signals on those counters happen inside kernels; 0: hipStreamWaitValue32 / hipStreamWriteValue32 around the pieces
};

// What this context and device can do.  The geometry predicates are facts about the loaded networks (decode_host.h: decode_caps).
struct DecodeCaps {
  bool xgroup_ok = true;               // cleared when a decode reports that the team kernels' placement assumption (block b on XCD b % 8) does not hold here, or keeps timing out
  bool can_stream_wait_value = true;   // hipDeviceAttributeCanUseStreamWaitValue
  int prof_id = -1;                    // the kernel being timed (dctts_prof_enable), -1 = none
  bool std_cone_tail = true;           // AudioDec has 11 layers and HC_5 .. HC_7 emit 5 / 3 / 1 cone rows (what xtail_kernel is written for)
  bool hc2_presum = true;              // AudioDec HC_2 has the presum packing with tap offset -1 (rowhc2_kernel; xcone_kernel starts behind it)
  bool c1q_wp16 = true;                // the Q half of AudioDec C_1 has the 16-row packing (the attention + C_1 block behind the AudioEnc run)
  bool d256 = true;                    // hp.d == 256 (the same block)
  bool c1_has_cone = true;             // AudioDec C_1 has cone rows besides the newest: a rowc1 phase exists to poll the passengers' counter
  bool side_fold_rows_ok = true;       // C_1's older cone rows and HC_2's cone rows are at most 96 each (the two row phases of xcone_kernel)
};

// The resolved form of one decode: assigned by resolve_decode_form and nowhere else, read-only to everything below decode_v3's first lines.
struct DecodeForm {
  bool counters = false;                 // the streams meet through two counters (stream memory operations or in-kernel polls / stores), not events
  bool chain_signals_inkernel = false;   // the chain's counter is written by the first launch of the NEXT chain piece
  bool chain_waits_inkernel = false;     // ... which also polls the side stream's counter itself (no wait operation in front of the piece)
  bool side_signals_inkernel = false;    // the side stream's counter is written by xcone_kernel's last team, which polls the chain's at its end: no stream operation per frame
  bool xgroup_on = false;                // the chain's runs of highway layers are team launches (xgroup_kernel or the kernels that contain it); off: one chain3_kernel launch per layer
  bool xcone_on = false;                 // the tail of AudioDec's cone (HC_3 ..) on the side stream is one team launch (xcone_kernel); off: a GEMM + a row pass per layer
  bool xtail_on = false;                 // HC_5 .. HC_7 over their few cone rows and the k = 1 layers run on the chain as xtail_kernel (ChainTail >= 2)
  bool xmlp_on = false;                  // the k = 1 layers as xmlp_kernel (otherwise, without xtail_on: mlp_rows_kernel)
  bool dec_merged = false;               // AudioDec's newest-row layers run in FRONT of xtail_kernel's cone layers in the same launch (not TailBehindXgroup)
  int np = 3;                            // newest-row layers in that front: 4 = HC_2 .. HC_5 (xcone_kernel runs HC_3 .. HC_5's older rows), 3 = HC_2 .. HC_4 (rounds 4-5)
  int team_u = 4;                        // utterances per team and round: a batch of at most 8 / 16 is dealt one / two to a team so that all eight teams work (the merged forms
                                         //   only: all three team kernels know about it); bitwise the four-utterance form, which DCTTS_XGROUP=2 forces
  bool attn_fold = false;                // the newest row's attention + AudioDec C_1 run behind the AudioEnc run's last layer inside xgroup_kernel, not as two more launches
  bool one_launch = false;               // a chain piece is ONE launch (xchain_kernel): xtail_kernel's layers, a team barrier, the AudioEnc run + attention + C_1
  bool side_fold = false;                // rowc1 / rowhc2 are the first two phases of xcone_kernel's launch (round 5), not launches of their own
  bool c1qw_on_chain = false;            // the newest row of the C1Q . W2 cache is computed on the chain's stream (its input is the chain's own newest row), not in front of the cone work
  bool passengers = false;               // ... and, like AudioEnc's presums, by passenger workgroups of the chain's first launch: no launch of its own; rowc1 polls the row's counter

  // Everything a device table or a captured graph built for this form depends on: the table caches and the graph cache key on this plus their own geometry and pointers.
  std::string key() const {
    std::string s;
    for (int v : {(int)counters, (int)chain_signals_inkernel, (int)chain_waits_inkernel, (int)side_signals_inkernel, (int)xgroup_on, (int)xcone_on, (int)xtail_on, (int)xmlp_on,
                  (int)dec_merged, np, team_u, (int)attn_fold, (int)one_launch, (int)side_fold, (int)c1qw_on_chain, (int)passengers}) s += (char)('0' + v);
    return s;
  }
};

inline DecodeForm resolve_decode_form(const DecodeKnobs& k, const DecodeCaps& cap, int B) {
  const ChainTail ct = k.chain_tail;
  const bool merged = ct == ChainTail::OneLaunch || ct == ChainTail::TwoLaunches || ct == ChainTail::OneLaunchNP3;
  DecodeForm f;
  f.counters = k.sync_values != 0 && cap.can_stream_wait_value;
  f.chain_signals_inkernel = f.counters;
  f.chain_waits_inkernel = f.counters && k.chain_wait_inkernel != 0;
  f.xgroup_on = k.xgroup != 0 && cap.xgroup_ok && cap.prof_id != DCTTS_PROF_CHAIN_HC;                       // (that timing id looks at chain3_kernel launches)
  f.xcone_on = k.xcone != 0 && cap.xgroup_ok && cap.prof_id != DCTTS_PROF_BULK_GEMM && cap.hc2_presum;     // (... and that one at hbulk_kernel's)
  f.side_signals_inkernel = f.chain_waits_inkernel && f.xcone_on;
  f.xtail_on = f.xgroup_on && f.xcone_on && (merged || ct == ChainTail::TailBehindXgroup) && cap.std_cone_tail;
  f.xmlp_on = f.xgroup_on && ct != ChainTail::MlpRows && !f.xtail_on;
  f.dec_merged = f.xtail_on && merged;
  f.np = (f.dec_merged && ct != ChainTail::OneLaunchNP3) ? 4 : 3;
  f.team_u = (!f.dec_merged || k.xgroup == 2 || B > 16) ? 4 : (B > 8 ? 2 : 1);
  f.attn_fold = f.xgroup_on && ct != ChainTail::MlpRows && cap.d256 && cap.c1q_wp16;
  f.side_fold = k.xcone == 1 && f.side_signals_inkernel && cap.side_fold_rows_ok;                           // (needs the team kernel and its in-kernel stream meetings)
  f.c1qw_on_chain = f.counters && f.xcone_on;
  f.passengers = f.side_signals_inkernel && f.xgroup_on && cap.c1_has_cone;
  f.one_launch = f.dec_merged && ct != ChainTail::TwoLaunches && f.attn_fold && f.passengers;
  return f;
}
