"""The three-term split-bf16 contraction (dctts_set_split_bf16_terms(ctx, 3); hconv_kernel<BF = 2>): fp32-grade error on the bf16 matrix pipe.

x = hi + mid + lo exactly, six products accumulated in fp32 small terms first; what is dropped is <= ~2^-26 |x||w| per product, below one fp32 accumulate rounding.
So the form is held to the fp32 form's OWN error against the oracle, not only to the project's layer bound (the two-term form sits at 4-22 x the fp32 form's at these shapes).

The factor: 2 was the expectation (both errors are rounding noise of the same predicted size; the max over ~1e5 outputs fluctuates).  Measured e3 / e32 per class at these
shapes: TextEnc 0.85 .. 1.31, SSRN 0.91 .. 2.20 (C_14 2.20, HC_3 1.97, HC_11 1.93; DESIGN.md section 11 has the table) -- at 150 rows SSRN's fp32 form is the tap / K-third
row tail, which adds three separately accumulated partial sums and so carries about sqrt(3) less accumulated rounding than one chain over K; the three-term errors themselves
are the same 4 .. 6e-6 in both networks.  RATIO is therefore the worst measured ratio x 1.5 = 3.3 (the rule of the issue that asked for this form; never above 4)."""
import numpy as np
import pytest
import torch

from dc_tts_amd.engine import Engine
from dc_tts_amd.hyperparams import hp
from dc_tts_amd.layers import ssrn_layers, textenc_layers
from dc_tts_amd.weights import synthetic_text
from oracle import dctts_ref as O
from test_gpu_parity import CASES, TOL, _dev_index, dev, engine_for, maxabs

pytestmark = pytest.mark.gpu

RATIO = 3.3
_eng = {}


def engine_terms(weights, terms):
    if terms not in _eng:
        _eng[terms] = Engine(weights, hp, split_bf16=2, split_bf16_terms=terms)
    return _eng[terms]


@pytest.mark.parametrize("net,scope,causal,li", [c for c in CASES if c.values[0] in ("textenc", "ssrn")])
def test_three_term_layer_is_fp32_grade(weights, net, scope, causal, li):
    """Every layer shape class of TextEnc / SSRN at B = 2, T = 75 (150 rows: four whole 32-row items + a ragged one of 22, a batch boundary inside an item)."""
    layers = {"textenc": textenc_layers, "ssrn": ssrn_layers}[net](hp)
    l = layers[li]
    rng = np.random.default_rng(100 + li)
    B, T = 2, 75
    P = O._Scoped(weights, scope, np.float32)
    di = _dev_index(layers, li, net)
    if net == "textenc" and li == 1:
        ids = rng.integers(0, len(hp.vocab), (B, T)).astype(np.int32)
        ref = O.conv1d(O.embed(ids, P["embed_1/lookup_table"]), P, "C_2", act=O.relu)
        run = lambda e: e.debug_layer(net, 0, dev(ids), l.cout).cpu().numpy()
    else:
        x = rng.standard_normal((B, T, l.cin)).astype(np.float32)
        if l.kind == "C":
            ref = O.conv1d(x, P, l.scope, padding="SAME", act=O.relu if l.act == "relu" else None)
        elif l.kind == "HC":
            ref = O.hc(x, P, l.scope, rate=l.rate, padding="SAME")
        else:
            ref = O.conv1d_transpose(x, P, l.scope)
        run = lambda e: e.debug_layer(net, di, dev(x), l.cout, **({"upsample": 2} if l.kind == "D" else {})).cpu().numpy()
    if net == "ssrn" and li == len(layers) - 1:
        ref = O.sigmoid(ref)
    e3_, e2_ = engine_terms(weights, 3), engine_terms(weights, 2)
    e3_.set_split_bf16(0); got32 = run(e3_)
    e3_.set_split_bf16(2); got3 = run(e3_)
    e2_.set_split_bf16(2); got2 = run(e2_)
    e3, e2, e32 = maxabs(got3, ref), maxabs(got2, ref), maxabs(got32, ref)
    print(f"{net}/{l.scope}: three-term {e3:.2e}  two-term {e2:.2e}  fp32 {e32:.2e}  (e3 / e32 = {e3 / e32:.2f})")
    assert got3.shape == ref.shape and e3 < 2e-4, e3
    assert e3 <= RATIO * e32, (e3, e32)
    if l.cin >= 32:
        assert not np.array_equal(got3, got2) and e3 < e2, (e3, e2)


def test_three_term_pipeline(weights):
    """Level 1 leaves Text2Mel bit-identical, level 2 keeps the oracle's attention trajectory; Y and Z stay within 2 x the same engine's fp32 error."""
    h = hp.replace(max_T=50)
    eng = Engine(weights, h, split_bf16=2, split_bf16_terms=3)
    Lh = synthetic_text(h, B=4, seed=77)
    L = dev(Lh)
    res = []
    for level in (0, 1, 2):
        eng.set_split_bf16(level); res.append(eng.synthesize(L)); eng.synchronize()
    (Y0, Z0, m0), (Y1, Z1, m1), (Y2, Z2, m2) = res
    assert torch.equal(Y1, Y0) and torch.equal(m1, m0)
    Yr, Zr, traj = O.synthesize(Lh, {k: v.astype(np.float64) for k, v in weights.items()}, h, np.float64)
    np.testing.assert_array_equal(m2.cpu().numpy(), traj)
    errs = [(maxabs(Y.cpu().numpy(), Yr), maxabs(Z.cpu().numpy(), Zr)) for Y, Z, _ in res]
    print("three-term max-abs vs the float64 oracle (Y, Z) at level 0 / 1 / 2:", [(f"{a:.2e}", f"{b:.2e}") for a, b in errs])
    for ey, ez in errs:
        assert ey <= 2 * errs[0][0] and ez <= 2 * errs[0][1] and ey < TOL and ez < TOL, errs
    eng.close()


def test_terms_state(weights):
    eng, plain = engine_terms(weights, 2), engine_for(weights)      # plain: created without split_bf16, no packing of either form
    for call, arg in ((eng.set_split_bf16_terms, 1), (eng.set_split_bf16_terms, 4), (eng.set_split_bf16_terms, 3), (plain.set_split_bf16, 1),
                      (plain.set_split_bf16_terms, 3), (plain.set_split_bf16, 1)):
        with pytest.raises(Exception):
            call(arg)
    eng.set_split_bf16_terms(2); plain.set_split_bf16_terms(2); plain.set_split_bf16(0)
