"""dc_tts_amd/csrc/decode_form.h on the host: which launch form the two-stream decode takes for which knobs and capabilities.  The header includes no HIP header, so a
plain C++17 compiler builds the small program (tests/decode_form_test.cpp) that prints what it resolves."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("decode_form") / "decode_form_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "decode_form_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def enumeration(exe):
    """(forms, team): [(packed form, key)] of the 7 776 inputs and of the 28 batch-size rows; bits 17-19 of a packed form are team_u."""
    head, tail = subprocess.check_output([exe]).decode().split("team_u\n")
    rows = lambda text: [(int(a), b) for a, b in (line.split() for line in text.splitlines())]
    return rows(head), rows(tail)


# ---------------------------------------------------------------- a. the documented forms (tools/README.md), written by hand
FLAGS = ("counters", "chain_signals_inkernel", "chain_waits_inkernel", "side_signals_inkernel", "xgroup_on", "xcone_on", "xtail_on", "xmlp_on", "dec_merged", "attn_fold",
         "one_launch", "side_fold", "c1qw_on_chain", "passengers")
INKERNEL = {"counters", "chain_signals_inkernel", "chain_waits_inkernel", "side_signals_inkernel"}      # both stream meetings of a frame inside kernels
TEAMS = {"xgroup_on", "xcone_on"}
# name: (chain_tail, xgroup, xcone, sync_values, chain_wait, prof_id, xgroup_ok, can_stream_wait_value, capability set), the flags that are on, np, team_u at B = 3
DOCUMENTED = {
    # one launch per chain piece with four newest-row layers in front, one per side piece with the row phases folded in, presum GEMMs as passengers, in-kernel meetings
    "default": ((2, 1, 1, 1, 1, -1, 1, 1, 0),
                INKERNEL | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "one_launch", "side_fold", "c1qw_on_chain", "passengers"}, 4, 1),
    # events: no counter, so nothing polls in-kernel, no passengers (and so no one-launch piece), the side piece as three launches
    "DCTTS_SYNC_VALUES=0": ((2, 1, 1, 0, 1, -1, 1, 1, 0), TEAMS | {"xtail_on", "dec_merged", "attn_fold"}, 4, 1),
    "no stream-wait-value capability": ((2, 1, 1, 1, 1, -1, 1, 0, 0), TEAMS | {"xtail_on", "dec_merged", "attn_fold"}, 4, 1),
    # stream memory operations around the pieces: the chain's launch still writes its counter; the C1Q . W2 row in the chain's presum launch
    "DCTTS_CHAIN_WAIT=0": ((2, 1, 1, 1, 0, -1, 1, 1, 0),
                           {"counters", "chain_signals_inkernel"} | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "c1qw_on_chain"}, 4, 1),
    # one chain3_kernel launch per chain layer; the side stream keeps its team kernel
    "DCTTS_XGROUP=0": ((2, 0, 1, 1, 1, -1, 1, 1, 0), INKERNEL | {"xcone_on", "side_fold", "c1qw_on_chain"}, 3, 4),
    # one GEMM + row pass per cone layer: the chain falls back to xgroup_kernel runs + xmlp_kernel
    "DCTTS_XCONE=0": ((2, 1, 0, 1, 1, -1, 1, 1, 0), (INKERNEL - {"side_signals_inkernel"}) | {"xgroup_on", "xmlp_on", "attn_fold"}, 3, 4),
    "DCTTS_XCONE=2": ((2, 1, 2, 1, 1, -1, 1, 1, 0),
                      INKERNEL | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "one_launch", "c1qw_on_chain", "passengers"}, 4, 1),
    "DCTTS_XGROUP=0,DCTTS_XCONE=0": ((2, 0, 0, 1, 1, -1, 1, 1, 0), INKERNEL - {"side_signals_inkernel"}, 3, 4),
    "DCTTS_CHAIN_TAIL=0": ((0, 1, 1, 1, 1, -1, 1, 1, 0), INKERNEL | TEAMS | {"side_fold", "c1qw_on_chain", "passengers"}, 3, 4),
    "DCTTS_CHAIN_TAIL=1": ((1, 1, 1, 1, 1, -1, 1, 1, 0), INKERNEL | TEAMS | {"xmlp_on", "attn_fold", "side_fold", "c1qw_on_chain", "passengers"}, 3, 4),
    "DCTTS_CHAIN_TAIL=5": ((5, 1, 1, 1, 1, -1, 1, 1, 0), INKERNEL | TEAMS | {"xtail_on", "attn_fold", "side_fold", "c1qw_on_chain", "passengers"}, 3, 4),
    "DCTTS_CHAIN_TAIL=6": ((6, 1, 1, 1, 1, -1, 1, 1, 0),
                           INKERNEL | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "side_fold", "c1qw_on_chain", "passengers"}, 4, 1),
    "DCTTS_CHAIN_TAIL=6,DCTTS_XCONE=2": ((6, 1, 2, 1, 1, -1, 1, 1, 0),
                                         INKERNEL | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "c1qw_on_chain", "passengers"}, 4, 1),
    "DCTTS_CHAIN_TAIL=7": ((7, 1, 1, 1, 1, -1, 1, 1, 0),
                           INKERNEL | TEAMS | {"xtail_on", "dec_merged", "attn_fold", "one_launch", "side_fold", "c1qw_on_chain", "passengers"}, 3, 1),
    # one launch per layer, stream-operation meetings: nothing in it polls
    "safe-once": ((2, 0, 0, 1, 0, -1, 1, 1, 0), {"counters", "chain_signals_inkernel"}, 3, 4),
    "xgroup_ok false": ((2, 1, 1, 1, 1, -1, 0, 1, 0), INKERNEL - {"side_signals_inkernel"}, 3, 4),
}


@pytest.mark.parametrize("name", list(DOCUMENTED))
def test_documented_forms(exe, name):
    args, on, np_, team_u = DOCUMENTED[name]
    out = subprocess.check_output([exe] + [str(a) for a in args] + ["3"]).decode()
    got = {k: int(v) for k, v in (line.split("=") for line in out.splitlines())}
    want = {f: int(f in on) for f in FLAGS}
    want.update(np=np_, team_u=team_u)
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}


def test_retired_and_unknown_chain_tail_values_are_not_forms(exe):
    known = [v for v in range(-1, 10) if subprocess.check_output([exe, str(v)]).decode().strip() == "1"]
    assert known == [0, 1, 2, 5, 6, 7]


# ---------------------------------------------------------------- b. every input against the commit that introduced the header
def test_every_form_is_what_the_scattered_flags_gave(enumeration):
    """tests/golden/decode_form_parent.txt was recorded once from the flag assignments of the commit before decode_form.h (decode_v3's first 50 lines, team_u_for,
    v3_xcone_table's side_fold, read_env's rewrite of 7), copied over a stub context: 6 chain tails x 3 x 3 team-kernel knobs x 2 x 2 meeting knobs x 3 timing ids x
    xgroup_ok x stream-wait capability x 3 capability sets, then team_u over the batch sizes at which it changes.  side_pre and ae_pass_split were false in every row."""
    forms, team = enumeration
    lines = [l for l in open(os.path.join(HERE, "golden", "decode_form_parent.txt")).read().splitlines() if not l.startswith("#")]
    cut = lines.index("team_u")
    want_forms, want_team = [int(x) for x in lines[:cut]], [int(x) for x in lines[cut + 1:]]
    assert len(want_forms) == 6 * 3 * 3 * 2 * 2 * 3 * 2 * 2 * 3 == 7776 and len(want_team) == 7 * 2 * 2
    assert [p for p, _ in forms] == want_forms
    assert [p >> 17 for p, _ in team] == want_team


# ---------------------------------------------------------------- c. the key tells forms apart
def test_key_distinguishes_forms(enumeration):
    forms, team = enumeration
    by_key, by_form = {}, {}
    for packed, key in forms + team:
        by_key.setdefault(key, set()).add(packed)
        by_form.setdefault(packed, set()).add(key)
    assert len(by_form) > 40                                        # the enumeration reaches many forms ...
    assert all(len(v) == 1 for v in by_key.values())                # ... no two of them share a key ...
    assert all(len(v) == 1 for v in by_form.values())               # ... and a form has one key
