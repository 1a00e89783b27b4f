"""Every launch form of the layer launcher (run_conv in dc_tts_amd/csrc/dctts_api.hip), reached ON PURPOSE and by name, at the row counts where the form changes.

run_conv picks a form from the row count M = B * rows, the compute units n of the device and per-layer flags.  Each case below
  1. builds its shape from n, and asserts the properties that make the shape reach the form it is meant for;
  2. runs one layer (Engine.debug_layer);
  3. reads the census of the launch (Engine.conv_forms: output rows per form) and compares it with `expected_forms`, the table below -- written
     out here as a plain function of (layer flags, rows, n), NOT imported from the library;
  4. compares the output with the float64 oracle, the rows of each form separately, so that a failure names the kernel.
Tolerance: 2e-4 max-abs, the bound test_layer_vs_oracle holds these layers to with the same input distribution.

The shape builders are plain functions of n and are checked without a GPU (test_shape_builders) for n = 32 .. 304: a partitioned device reaches the same forms.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from dc_tts_amd.hyperparams import hp
from dc_tts_amd.layers import audiodec_layers, audioenc_layers, ssrn_layers, textenc_layers
from dc_tts_amd.weights import synthetic_text
from oracle import dctts_ref as O
from test_gpu_parity import _dev_index, dev, engine_for, maxabs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_LAYER = 2e-4

NETS = {"textenc": (textenc_layers, "Text2Mel/TextEnc", False), "audioenc": (audioenc_layers, "Text2Mel/AudioEnc", True),
        "audiodec": (audiodec_layers, "Text2Mel/AudioDec", True), "ssrn": (ssrn_layers, "SSRN", False)}

# what computes the rows a form is counted under (for the failure messages)
KERNEL = {"main": "hconv_kernel (whole 32-row items)",
          "xc": "hconv_kernel<XC = 1> (32 column tiles + the last column on the vector ALU)",
          "col_split": "hconv_kernel<RAW = 2> (quarter-column items) + hc_tail_finish_kernel",
          "hc_tap_tail": "hconv_kernel<RAW = 1> (32-row items x taps) + hc_tail_finish_kernel",
          "c_tap_tail": "hconv_kernel<RAW = 1> (32-row items x thirds of K) + c_tail_finish_kernel",
          "rows16": "16-row items", "split_bf16": "hconv_kernel<BF = 1>"}

_SSRN = ssrn_layers(hp)
_FIRST_D = [i for i, l in enumerate(_SSRN) if l.kind == "D"][0]
_FIRST_4T = [i for i, l in enumerate(_SSRN) if l.kind == "D"][1] + 1      # SSRN layers from here on run at 4T rows


# ---------------------------------------------------------------- the documented table: (layer flags, rows, n) -> output rows per form
def layer_flags(net, li):
    """The per-layer flags run_conv looks at, restated from the network definitions:
       col_split  every highway layer of TextEnc (512 channels);
       hc_tail    every three-tap highway layer of SSRN (512 or 1024 channels);
       c_tail     SSRN's k = 1 conv layers at 4T resolution (C_10, C_13 .. C_16);
       xc         SSRN's 1025-column layers (C_13 .. C_16);
       up         a transposed conv: two launches (even / odd output rows), 2 output rows per input row."""
    l = NETS[net][0](hp)[li]
    return {"col_split": net == "textenc" and l.kind == "HC",
            "hc_tail": net == "ssrn" and l.kind == "HC" and l.size == 3,
            "c_tail": net == "ssrn" and l.kind == "C" and li >= _FIRST_4T,
            "xc": net == "ssrn" and l.kind == "C" and l.cout == 1025,
            "up": l.kind == "D"}


def expected_forms(flags, rows, n):
    """Output rows per launch form for a layer of `rows` input rows on a device of n compute units (exact fp32 mode).
       * a column-split layer: all rows, always;
       * otherwise the rows are 32-row items; `full` = the items of the exact rounds of n, `left` = the rest (the last one may be ragged);
       * a layer with a tap / K-third tail whose 3 * left workgroups fit in two rounds (0 < 3 left <= 2 n) runs the `full` items on the main kernel and the
         left-over ROWS on the tail form; everything else runs all items on the main kernel (XC for the 1025-column layers)."""
    if flags["col_split"]:
        return {"col_split": rows}
    main = "xc" if flags["xc"] else "main"
    if flags["up"]:
        return {main: 2 * rows}
    tiles = (rows + 31) // 32
    full = (tiles // n) * n
    left = tiles - full
    if (flags["hc_tail"] or flags["c_tail"]) and left > 0 and 3 * left <= 2 * n:
        out = {"hc_tap_tail" if flags["hc_tail"] else "c_tap_tail": rows - 32 * full}
        if full:
            out[main] = 32 * full
        return out
    return {main: rows}


def form_row_ranges(forms, rows):
    """[(form, first output row, end)] of a layer without upsampling: the main kernel's rows come first, a tail form takes the rest."""
    out, at = [], 0
    for f in ("main", "xc", "col_split", "hc_tap_tail", "c_tap_tail"):
        if f in forms:
            out.append((f, at, at + forms[f])); at += forms[f]
    assert at == rows
    return out


# ---------------------------------------------------------------- shapes, as functions of the device's compute units
TINY = [(1, 1), (1, 31), (3, 11)]            # M = 1, 31, 33: one ragged item; one row short of an item; one item + one row, two batch boundaries inside the item


def threshold_shapes(n):
    """The two sides of 3 * left <= 2 n for a layer with a tail form, B = 1, each with a ragged last item (19 of its 32 rows)."""
    below, above = (2 * n) // 3, (2 * n) // 3 + 1
    assert 0 < 3 * below <= 2 * n < 3 * above and above < n        # both less than one round: full = 0, left = tiles
    return 32 * below - 13, 32 * above - 13


def round_plus_tail_shape(n):
    """(B, T): one exact round of n items + a tail of 18 .. 40 rows that is no multiple of 4 (the finishing kernels take 4 rows per block) and contains a batch boundary.
    T = 17 wherever a batch size with these properties exists (n = 256: B = 483); for the few n where none does (n = 80: 17 B - 2560 is 24 or 41) the next odd T."""
    for T in (17, 19, 21, 23):
        for B in range((32 * n + 18 + T - 1) // T, (32 * n + 40) // T + 1):
            tail = T * B - 32 * n
            boundary = ((32 * n + T - 1) // T) * T                   # first utterance start at or behind row 32 n
            if 18 <= tail <= 40 and tail % 4 != 0 and 32 * n <= boundary < T * B:
                return B, T
    raise AssertionError(f"no batch size for n = {n}")


def check_shape_properties(n):
    lo, hi = threshold_shapes(n)
    for rows, tail in ((lo, True), (hi, False)):
        tiles = (rows + 31) // 32
        assert rows % 32 == 19 and tiles < n and (3 * tiles <= 2 * n) == tail
    assert (hi + 31) // 32 - (lo + 31) // 32 == 1                    # ONE more item changes the form
    B, T = round_plus_tail_shape(n)
    rows, tail = B * T, B * T - 32 * n
    tiles = (rows + 31) // 32
    assert 18 <= tail <= 40 and tail % 4 and tiles // n == 1 and 0 < 3 * (tiles - n) <= 2 * n
    assert any(r % T == 0 for r in range(32 * n, rows))             # an utterance starts inside the tail ...
    assert (32 * n) % T != 0 or tail > T                             # ... and the tail holds rows of two utterances
    hc = {"col_split": False, "hc_tail": True, "c_tail": False, "xc": False, "up": False}
    cx = {"col_split": False, "hc_tail": False, "c_tail": True, "xc": True, "up": False}
    plain = {"col_split": False, "hc_tail": False, "c_tail": False, "xc": False, "up": False}
    assert expected_forms(hc, lo, n) == {"hc_tap_tail": lo} and expected_forms(hc, hi, n) == {"main": hi}
    assert expected_forms(cx, lo, n) == {"c_tap_tail": lo} and expected_forms(cx, hi, n) == {"xc": hi}
    assert expected_forms(hc, rows, n) == {"main": 32 * n, "hc_tap_tail": tail} and expected_forms(cx, rows, n) == {"xc": 32 * n, "c_tap_tail": tail}
    assert expected_forms(plain, rows, n) == {"main": rows}
    for B1, T1 in TINY:
        assert expected_forms(hc, B1 * T1, n) == {"hc_tap_tail": B1 * T1} and expected_forms(cx, B1 * T1, n) == {"c_tap_tail": B1 * T1}


def test_shape_builders():
    """No GPU: the shapes keep their properties on whole and partitioned devices; n = 256 gives the shapes of the MI355X (B = 483: 8211 rows, 19 in the tail,
    utterance 482 starts at row 8194)."""
    for n in (32, 64, 80, 256, 304):
        check_shape_properties(n)
    assert threshold_shapes(256) == (32 * 170 - 13, 32 * 171 - 13)
    assert round_plus_tail_shape(256) == (483, 17)


# ---------------------------------------------------------------- cases: one layer per kernel instantiation
def _dedup(net, lo=0, keep=lambda l: True):
    seen, out = set(), []
    layers = NETS[net][0](hp)
    for li in range(lo, len(layers)):
        l = layers[li]
        key = (l.kind, l.cin, l.cout, l.size, l.act)
        if l.kind == "E" or key in seen or not keep(l):
            continue
        seen.add(key)
        out.append(pytest.param(net, li, id=f"{net}-{l.scope}-{l.kind}{l.cin}to{l.cout}k{l.size}"))
    return out


SMALL_LAYERS = [c for net in NETS for c in _dedup(net)]
BIG_LAYERS = _dedup("ssrn", _FIRST_4T)                            # SSRN's layers with a tail form, the 1025-column ones among them (HC_8, C_10, HC_11, C_13, C_14, C_16)
SHORT_LAYERS = []
for _net in ("textenc", "audioenc", "audiodec"):
    _seen = set()
    for _li, _l in enumerate(NETS[_net][0](hp)):
        if _l.kind == "HC" and _l.rate >= 9 and _l.rate not in _seen:
            _seen.add(_l.rate)
            SHORT_LAYERS.append(pytest.param(_net, _li, id=f"{_net}-{_l.scope}-d{_l.rate}"))


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def oracle64(weights, net, li, x):
    """The layer in float64 (x: the float32 input the device got, or int32 ids for TextEnc's fused embed + C_2)."""
    fn, scope, causal = NETS[net]
    layers = fn(hp)
    l = layers[li]
    P = O._Scoped(weights, scope, np.float64)
    pad = "CAUSAL" if causal else "SAME"
    if net == "textenc" and li == 1:
        ref = O.conv1d(O.embed(x, P["embed_1/lookup_table"]), P, "C_2", act=O.relu)
    elif l.kind == "C":
        ref = O.conv1d(x.astype(np.float64), P, l.scope, padding=pad, act=O.relu if l.act == "relu" else None)
    elif l.kind == "HC":
        ref = O.hc(x.astype(np.float64), P, l.scope, rate=l.rate, padding=pad)
    else:
        ref = O.conv1d_transpose(x.astype(np.float64), P, l.scope)
    if net in ("audiodec", "ssrn") and li == len(layers) - 1:         # the network's sigmoid rides in the last layer's epilogue
        ref = O.sigmoid(ref)
    return ref


def make_input(net, li, B, T, seed):
    l = NETS[net][0](hp)[li]
    rng = np.random.default_rng(seed)
    if net == "textenc" and li == 1:
        return rng.integers(0, len(hp.vocab), (B, T)).astype(np.int32)
    return rng.standard_normal((B, T, l.cin)).astype(np.float32)


def run_layer(eng, net, li, x):
    layers = NETS[net][0](hp)
    l = layers[li]
    di = 0 if (net == "textenc" and li == 1) else _dev_index(layers, li, net)
    eng.conv_forms()                                                  # (clear)
    got = eng.debug_layer(net, di, dev(x), l.cout, upsample=2 if l.kind == "D" else 1).cpu().numpy()
    return got, {k: v for k, v in eng.conv_forms().items() if v}


def check_case(weights, net, li, B, T, seed, want_forms=None):
    """Census first (a wrong form is reported as such, not as a numeric error), then max-abs against the float64 oracle per form."""
    eng = engine_for(weights)
    n = n_cu()
    l = NETS[net][0](hp)[li]
    flags = layer_flags(net, li)
    expect = expected_forms(flags, B * T, n)
    if want_forms is not None:
        assert set(expect) == set(want_forms), f"the shape {B} x {T} does not reach {want_forms} on {n} compute units: {expect}"
    x = make_input(net, li, B, T, seed)
    got, forms = run_layer(eng, net, li, x)
    assert forms == expect, f"{net}/{l.scope} {B} x {T} on {n} CUs: launch forms {forms}, expected {expect}"
    ref = oracle64(weights, net, li, x)
    assert got.shape == ref.shape
    up = 2 if flags["up"] else 1
    g, r = got.reshape(B * T * up, -1), ref.reshape(B * T * up, -1)
    errs = {f: maxabs(g[a:b], r[a:b]) for f, a, b in form_row_ranges(forms, B * T * up)}
    print(f"{net}/{l.scope} {B} x {T}: " + ", ".join(f"{f} rows {forms[f]} max-abs {e:.2e}" for f, e in errs.items()))
    for f, e in errs.items():
        assert e < TOL_LAYER, f"{net}/{l.scope} {B} x {T}: {KERNEL[f]}: max-abs {e:.3e} over its {forms[f]} rows (all forms: {errs})"
    return x, got


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", TINY)
@pytest.mark.parametrize("net,li", SMALL_LAYERS)
def test_tiny_launches(weights, net, li, B, T):
    check_case(weights, net, li, B, T, seed=1000 + 37 * li + B * T)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 28])
@pytest.mark.parametrize("net,li", SHORT_LAYERS)
def test_sequences_shorter_than_the_dilation(weights, net, li, T):
    """B = 3, T = 5 / 28 under dilation 9 / 27, SAME (TextEnc: the column-split form) and CAUSAL (AudioEnc, AudioDec): the outer taps leave the utterance and must
    read zeros, not the neighbouring utterance -- utterance 1's output is bitwise the same whatever utterances 0 and 2 hold."""
    B = 3
    l = NETS[net][0](hp)[li]
    reach = 2 * l.rate if NETS[net][2] else l.rate
    assert T <= reach + 1 or l.rate == 9                             # (T = 28 under dilation 9 is the in-between case: some rows read pad, some the utterance)
    x, got = check_case(weights, net, li, B, T, seed=2000 + 37 * li + T, want_forms=["col_split"] if net == "textenc" else ["main"])
    y = x.copy()
    y[0] = 3.0 * x[2] + 1.0; y[2] = -2.0 * x[0] - 1.0
    got2, _ = run_layer(engine_for(weights), net, li, y)
    assert np.array_equal(got2[1], got[1]), f"{net}/{l.scope} T = {T}: utterance 1 changed with its neighbours (max-abs {maxabs(got2[1], got[1]):.3e})"
    assert not np.array_equal(got2[0], got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["tail", "main"])
@pytest.mark.parametrize("net,li", BIG_LAYERS)
def test_switch_between_tail_and_main(weights, net, li, side):
    """(2 n) // 3 items: all rows on the tap / K-third tail form (m_base = 0); one item more: all on the main kernel (XC for the 1025-column layers) as a
    partial round.  The last item is ragged on both sides."""
    lo, hi = threshold_shapes(n_cu())
    flags = layer_flags(net, li)
    want = ["hc_tap_tail" if flags["hc_tail"] else "c_tap_tail"] if side == "tail" else ["xc" if flags["xc"] else "main"]
    check_case(weights, net, li, 1, lo if side == "tail" else hi, seed=3000 + li, want_forms=want)


@pytest.mark.gpu
@pytest.mark.parametrize("net,li", BIG_LAYERS)
def test_round_plus_tail_across_a_batch_boundary(weights, net, li):
    """One exact round on the main / XC kernel + a tail (m_base = 32 n) of 18 .. 40 rows, no multiple of the finishing kernels' 4 rows per block, that holds the
    end of one utterance and the start of the next."""
    B, T = round_plus_tail_shape(n_cu())
    flags = layer_flags(net, li)
    check_case(weights, net, li, B, T, seed=4000 + li,
               want_forms=["xc" if flags["xc"] else "main", "hc_tap_tail" if flags["hc_tail"] else "c_tap_tail"])


@pytest.mark.gpu
def test_production_shapes_never_take_16_row_items(weights):
    """The census over SSRN at the suite's production geometries (test_ssrn, config 3's batch of 128 and its shards of 32) and over a ragged Text2Mel batch:
    every row is accounted for, and none is given to 16-row items."""
    eng = engine_for(weights)
    n = n_cu()
    rng = np.random.default_rng(5)
    eng.conv_forms()
    for B, T in ((2, 37), (32, hp.max_T), (128, hp.max_T)):
        eng.ssrn(dev(rng.random((B, T, hp.n_mels), dtype=np.float32)), want_logits=False)
        torch.cuda.synchronize()
        forms = eng.conv_forms()
        want = {}
        for li, l in enumerate(_SSRN):
            rows = B * T * (1 if li <= _FIRST_D else 2 if li < _FIRST_4T else 4)      # input rows: T up to D_4, 2T up to D_7, then 4T
            for f, r in expected_forms(layer_flags("ssrn", li), rows, n).items():
                want[f] = want.get(f, 0) + r
        print(f"SSRN {B} x {T} on {n} CUs:", {k: v for k, v in forms.items() if v})
        assert {k: v for k, v in forms.items() if v} == want and forms["rows16"] == 0
    Tm = 24
    e2 = engine_for(weights, max_T=Tm)
    e2.conv_forms()
    e2.text2mel(dev(synthetic_text(hp.replace(max_T=Tm), B=33, seed=404)))
    e2.synchronize()
    forms = e2.conv_forms()
    print(f"Text2Mel decode 33 x {Tm}:", {k: v for k, v in forms.items() if v})
    assert forms["rows16"] == 0 and forms["col_split"] == 33 * hp.max_N * 12 and forms["main"] > 0


# ---------------------------------------------------------------- DCTTS_PIECETIME reaches the decode
_PIECE_WORKER = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from dc_tts_amd.engine import Engine
from dc_tts_amd.hyperparams import hp
from dc_tts_amd.weights import synthetic_text, synthetic_weights
h = hp.replace(max_T=4)
eng = Engine(synthetic_weights(hp, seed=1234, perturb=True), h)
Y, mx = eng.text2mel(torch.from_numpy(synthetic_text(h, B=2, seed=7)).cuda())
eng.synchronize()
np.savez(sys.argv[2], Y=Y.cpu().numpy(), mx=mx.cpu().numpy())
print("PIECE_OK")
'''


@pytest.mark.gpu
def test_piecetime_knob_is_read_and_leaves_the_decode_alone(weights, tmp_path):
    """DCTTS_PIECETIME=0 in a fresh process (the knobs are read when a context is created): the decode (B = 2, T = 4) prints one timing line per frame of the
    window it ran to stderr (tools/README.md), and its outputs are bitwise those of a decode without the knob."""
    script = tmp_path / "piece.py"; script.write_text(_PIECE_WORKER)
    outp = str(tmp_path / "piece.npz")
    torch.cuda.synchronize()
    r = subprocess.run([sys.executable, str(script), ROOT, outp], capture_output=True, text=True, env=dict(os.environ, DCTTS_PIECETIME="0"), timeout=240)
    assert r.returncode == 0 and "PIECE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^\[dctts\] frame (\d+): chain piece ([0-9.]+) us, bulk piece ([0-9.]+) us", r.stderr, re.M)
    assert [int(f) for f, _, _ in lines] == [0, 1, 2, 3], r.stderr[-2000:]
    assert all(float(c) > 0 for _, c, _ in lines)
    h = hp.replace(max_T=4)
    eng = engine_for(weights, max_T=4)
    Y, mx = eng.text2mel(dev(synthetic_text(h, B=2, seed=7)))
    eng.synchronize()
    g = np.load(outp)
    np.testing.assert_array_equal(g["mx"], mx.cpu().numpy())
    np.testing.assert_array_equal(g["Y"], Y.cpu().numpy())
