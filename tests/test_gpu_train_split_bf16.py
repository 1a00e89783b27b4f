"""The training GEMM on the bf16 matrix pipe (dctts_train_set_split_bf16_terms(t, 3); gemm3_kernel): every contraction of the
training path from three exact bf16 terms per operand element, held to the fp32 form's OWN error against the float64 oracle on identical inputs
(one handle, switched between the forms).  Shapes and seeds are those of test_gpu_train.py; four cases are the large shapes of test_gpu_train_edges.py
(1035 and 1027 rows, a transposed convolution 128 -> 256, attention at T = 131, N = 181): multi-tile M / N and split-K over more than 1024 rows.

RATIO: e3 <= RATIO * e32 per output.  Both errors are fp32 accumulate rounding of the same predicted size (expectation: ratio <= 2); the rule of
tests/test_gpu_split_bf16_terms.py: worst measured e3 / e32 x 1.5, never above 4 (a two-term form sits at 4-22 x).  Measured (`-s` prints every ratio,
DESIGN.md section 10 has the table): worst 1.40 (conv1d_backward 256 -> 80, dx; attention dQ 1.39; 39 of the 43 outputs <= 1.10)  ->  RATIO = 2.1.
The 22 outputs of the four large cases: 0.52 .. 1.23 (worst: conv1d_backward 1024 -> 1025 at 1027 rows, gamma 1.23; hc_backward at 1035 rows, bias 1.12); none
above 1.40, so RATIO stays."""
import numpy as np
import pytest
import torch

from oracle import dctts_ref as O, train_ref as TR
from test_gpu_train import _compare, _small_weights, dev, maxabs, ops, rel  # noqa: F401  (ops: the module-scoped TrainOps fixture)

pytestmark = pytest.mark.gpu

RATIO = 2.1
f64 = lambda rng, *s, sd=1.0: rng.normal(0, sd, s).astype(np.float32).astype(np.float64)
w64 = lambda p: {n: v.astype(np.float32).astype(np.float64) for n, v in p.items()}


def hc_case(B, T, C, k, rate, padding, fwd=False):
    rng = np.random.default_rng(100 + C + rate)
    p = w64({"kernel": rng.normal(0, (k * C) ** -0.5, (k, C, 2 * C)), "bias": rng.normal(0, 0.1, 2 * C),
         "g1": 1 + rng.normal(0, 0.1, C), "b1": rng.normal(0, 0.1, C), "g2": 1 + rng.normal(0, 0.1, C), "b2": rng.normal(0, 0.1, C)})
    x, dy = f64(rng, B, T, C), f64(rng, B, T, C)
    pd = {n: dev(v) for n, v in p.items()}
    if fwd:
        return {"y": TR.hc_fwd(x, p, rate, padding)}, lambda o: {"y": o.hc_forward(dev(x), pd, rate=rate, padding=padding)}, ["y"]
    return TR.hc_bwd(x, p, dy, rate, padding), lambda o: o.hc_backward(dev(x), dev(dy), pd, rate=rate, padding=padding), ["dx", "kernel"]


def c_case(B, T, Cin, Cout, fwd=False, differ=("dx",)):
    rng = np.random.default_rng(200 + Cin + Cout)
    p = w64({"kernel": rng.normal(0, Cin ** -0.5, (1, Cin, Cout)), "bias": rng.normal(0, 0.1, Cout), "gamma": 1 + rng.normal(0, 0.1, Cout), "beta": rng.normal(0, 0.3, Cout)})
    x, dy = f64(rng, B, T, Cin), f64(rng, B, T, Cout)
    pd = {n: dev(v) for n, v in p.items()}
    pad = "causal" if Cout == 80 else "same"
    if fwd:
        return {"y": TR.c_fwd(x, p, 1, pad, None)}, lambda o: {"y": o.conv1d_forward(dev(x), pd, padding=pad)}, ["y"]
    return TR.c_bwd(x, p, dy, 1, pad, None), lambda o: o.conv1d_backward(dev(x), dev(dy), pd, padding=pad), list(differ)  # wgrad K = B T < 32 in the small cases


def d_case(B, T, C, Cout=None):
    Cout = Cout or C
    rng = np.random.default_rng(300 + C + (Cout != C) * Cout)
    p = w64({"kernel": rng.normal(0, (3 * C) ** -0.5, (1, 3, Cout, C)), "bias": rng.normal(0, 0.1, Cout), "gamma": 1 + rng.normal(0, 0.1, Cout), "beta": rng.normal(0, 0.3, Cout)})
    x, dy = f64(rng, B, T, C), f64(rng, B, 2 * T, Cout)
    return TR.d_bwd(x, p, dy), lambda o: o.conv1d_transpose_backward(dev(x), dev(dy), {n: dev(v) for n, v in p.items()}), ["dx", "kernel"]


def att_case(N, B=3, T=50):
    from dc_tts_amd.hyperparams import hp
    rng = np.random.default_rng(41)
    d = 256
    Q, K, V, dR, dAl = f64(rng, B, T, d), f64(rng, B, N, d), f64(rng, B, N, d), f64(rng, B, T, 2 * d), f64(rng, B, N, T)
    ref = dict(zip(("dQ", "dK", "dV"), TR.attention_bwd(Q, K, V, dR, dAl, d)))
    ref["R"], ref["al"], _ = O.Attention(Q, K, V, hp)
    def run(o):
        out = dict(zip(("dQ", "dK", "dV"), o.attention_backward(dev(Q), dev(K), dev(V), dev(dR), dev(dAl))))
        out["R"], out["al"] = o.attention_forward(dev(Q), dev(K), dev(V))
        return out
    return ref, run, ["dQ", "dK", "dV", "R"]


CASES = {"hc_r1": lambda: hc_case(2, 37, 256, 3, 1, "causal"), "hc_r27": lambda: hc_case(2, 64, 256, 3, 27, "causal"), "hc_1024": lambda: hc_case(1, 24, 1024, 3, 1, "same"),
         "c_80": lambda: c_case(2, 21, 256, 80), "c_1025": lambda: c_case(1, 12, 1024, 1025), "d_256": lambda: d_case(3, 16, 256), "att_37": lambda: att_case(37),
         "hc_fwd": lambda: hc_case(2, 37, 256, 3, 1, "causal", fwd=True), "c_fwd": lambda: c_case(2, 21, 256, 80, fwd=True),
         # the large shapes of test_gpu_train_edges.py: several 128-wide tiles along M and N, split-K over more than 1024 rows
         "hc_1035": lambda: hc_case(5, 207, 256, 3, 3, "causal"), "c_1025_1027": lambda: c_case(1, 1027, 1024, 1025, differ=("dx", "kernel")),
         "d_128_256": lambda: d_case(2, 19, 128, 256), "att_131_181": lambda: att_case(181, B=2, T=131)}
TOL = {"R": (maxabs, 1e-4), "al": (maxabs, 1e-5)}           # test_gpu_train.py's absolute bounds for the attention forward pass; everything else: rel < 2e-5


@pytest.mark.parametrize("case", list(CASES))
def test_three_term_gemm_is_fp32_grade(ops, case):
    ref, run, differ = CASES[case]()
    def both(terms):
        ops.set_split_bf16_terms(terms)
        a, b = run(ops), run(ops)
        torch.cuda.synchronize()
        for n in a:
            assert torch.equal(a[n], b[n]), f"{n}: terms = {terms} must be bitwise reproducible"
        return a
    g32, g3 = both(0), both(3)
    ops.set_split_bf16_terms(0)
    for n in g32:
        err, tol = TOL.get(n, (rel, 2e-5))
        e32, e3 = err(g32[n].cpu().numpy().astype(np.float64), ref[n]), err(g3[n].cpu().numpy().astype(np.float64), ref[n])
        print(f"{case:11s} {n:7s} e32 {e32:.2e} e3 {e3:.2e} ratio {e3 / e32:.2f}")
        assert e32 < tol, f"{n}: fp32 form {e32}"
        assert e3 <= RATIO * e32, f"{n}: three-term error {e3} against fp32 {e32}"
        assert n not in differ or not torch.equal(g32[n], g3[n]), f"{n}: the three-term kernel did not run"


def test_text2mel_gradients_three_terms(ops):
    """test_gpu_train.test_text2mel_training_gradients_end_to_end (B = 2, N = 12, T = 10) with every contraction in the three-term form."""
    from dc_tts_amd.hyperparams import hp
    from dc_tts_amd.layers import audiodec_layers, audioenc_layers, textenc_layers
    from dc_tts_amd.train import network_backward
    rng = np.random.default_rng(52)
    W = _small_weights(hp, 78)
    B, N, T, d = 2, 12, 10, hp.d
    ids = rng.integers(1, len(hp.vocab), (B, N)).astype(np.int32); ids[:, -2:] = 0
    mels = rng.uniform(0, 1, (B, T, hp.n_mels)).astype(np.float32).astype(np.float64)
    S = np.concatenate((np.zeros_like(mels[:, :1]), mels[:, :-1]), 1)
    te, ae, ad = textenc_layers(hp), audioenc_layers(hp), audiodec_layers(hp)
    KV, xs_te = TR.network_forward(te, W, "Text2Mel/TextEnc", ids, "same")
    K, V = KV[..., :d], KV[..., d:]
    Q, xs_ae = TR.network_forward(ae, W, "Text2Mel/AudioEnc", S, "causal")
    R, al, _ = O.Attention(Q, K, V, hp)
    logits, xs_ad = TR.network_forward(ad, W, "Text2Mel/AudioDec", R, "causal")
    Y = O.sigmoid(logits)
    lref, (dY, dlog, dA) = TR.text2mel_losses(Y, logits, mels, al, hp.max_N, hp.max_T)
    gref, ggpu = {}, {}
    dR, g = TR.network_backward(ad, W, "Text2Mel/AudioDec", xs_ad, dlog + dY * Y * (1 - Y), "causal"); gref.update(g)
    dQ, dK, dV = TR.attention_bwd(Q, K, V, dR, dA, d)
    _, g = TR.network_backward(ae, W, "Text2Mel/AudioEnc", xs_ae, dQ, "causal"); gref.update(g)
    _, g = TR.network_backward(te, W, "Text2Mel/TextEnc", xs_te, np.concatenate((dK, dV), -1), "same"); gref.update(g)
    Wd, Yd = {n: dev(v) for n, v in W.items() if n.startswith("Text2Mel/")}, dev(Y)
    to = lambda xs: [torch.from_numpy(x).cuda() if x.dtype == np.int32 else dev(x) for x in xs]
    ops.set_split_bf16_terms(3)
    losses, gY, glog, gA = ops.text2mel_losses(Yd, dev(logits), dev(mels), dev(al), hp.max_N, hp.max_T)
    gR, g = network_backward(ops, ad, Wd, "Text2Mel/AudioDec", to(xs_ad), glog + gY * Yd * (1 - Yd), "causal"); ggpu.update(g)
    gQ, gK, gV = ops.attention_backward(dev(Q), dev(K), dev(V), gR, gA)
    _, g = network_backward(ops, ae, Wd, "Text2Mel/AudioEnc", to(xs_ae), gQ, "causal"); ggpu.update(g)
    _, g = network_backward(ops, te, Wd, "Text2Mel/TextEnc", to(xs_te), torch.cat((gK, gV), -1).contiguous(), "same"); ggpu.update(g)
    torch.cuda.synchronize()
    ops.set_split_bf16_terms(0)
    np.testing.assert_allclose(losses.cpu().numpy(), lref, rtol=2e-5)
    assert len(gref) == len(Wd)
    _compare(ggpu, gref, 5e-4)


def test_terms_argument(ops):
    from dc_tts_amd.engine import DcttsError
    from dc_tts_amd.train import TrainOps
    for bad in (1, 2, 4):
        with pytest.raises(DcttsError):
            ops.set_split_bf16_terms(bad)
    _, run, _ = hc_case(2, 9, 256, 3, 3, "causal")
    o3 = TrainOps(split_bf16_terms=3)
    a3 = run(o3)
    o3.set_split_bf16_terms(0)
    o0 = TrainOps()
    a0, fresh = run(o3), run(o0)
    torch.cuda.synchronize()
    o3.close(); o0.close()
    assert not torch.equal(a3["dx"], a0["dx"])
    for n in fresh:
        assert torch.equal(a0[n], fresh[n]), f"{n}: 3 -> 0 must be the default form again, bit for bit"
