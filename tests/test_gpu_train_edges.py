"""The training kernels (include/dctts_train.h) against oracle/train_ref.py (float64) on the branches test_gpu_train.py's small shapes never
reach: the row kernels' stride past 1024 rows, the losses' stride past 1024 workgroups, a transposed convolution with Cin != Cout, SAME padding at
dilation 27, fewer rows than a workgroup has waves, attention beyond one GEMM tile, every forward block on its own, the tape's hit / out-of-step /
off branches, and a handle whose workspaces an earlier, larger call of another geometry has filled.

Bounds are the ones test_gpu_train.py already uses for the same kind of output: rel() < 2e-5 for the gradients of a single block (the float32 evaluation of
the oracle itself differs from float64 by at most 1.9e-6 in this measure at these row counts: a 10 x margin), max |error| < 1e-4 for a block's forward
output, 1e-5 for alignments, 1e-6 for the sign gradients of the L1 losses, rtol 2e-5 for a loss.  Inputs are rounded to fp32 and widened, so both sides
see the same numbers.  Each case's comment names the branch it reaches."""
import numpy as np
import pytest
import torch

from oracle import dctts_ref as O, train_ref as TR
from test_gpu_train import _small_weights, dev, maxabs, ops, rel  # noqa: F401  (ops: the module-scoped TrainOps fixture)

pytestmark = pytest.mark.gpu

r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
f64 = lambda rng, *s, sd=1.0: r32(rng.normal(0, sd, s))
up = lambda p: {n: dev(v) for n, v in p.items()}
HC_NAMES = ("dx", "kernel", "bias", "g1", "b1", "g2", "b2")
C_NAMES = ("dx", "kernel", "bias", "gamma", "beta")


def hc_params(rng, C, k):
    return {n: r32(v) for n, v in {"kernel": rng.normal(0, (k * C) ** -0.5, (k, C, 2 * C)), "bias": rng.normal(0, 0.1, 2 * C), "g1": 1 + rng.normal(0, 0.1, C),
                                   "b1": rng.normal(0, 0.1, C), "g2": 1 + rng.normal(0, 0.1, C), "b2": rng.normal(0, 0.1, C)}.items()}


def c_params(rng, Cin, Cout, k):
    return {n: r32(v) for n, v in {"kernel": rng.normal(0, (k * Cin) ** -0.5, (k, Cin, Cout)), "bias": rng.normal(0, 0.1, Cout),
                                   "gamma": 1 + rng.normal(0, 0.1, Cout), "beta": rng.normal(0, 0.3, Cout)}.items()}


def d_params(rng, Cin, Cout):
    return {n: r32(v) for n, v in {"kernel": rng.normal(0, (3 * Cin) ** -0.5, (1, 3, Cout, Cin)), "bias": rng.normal(0, 0.1, Cout),
                                   "gamma": 1 + rng.normal(0, 0.1, Cout), "beta": rng.normal(0, 0.3, Cout)}.items()}


def check_grads(got, ref, names, what=""):
    torch.cuda.synchronize()
    for n in names:
        e = rel(got[n].cpu().numpy().astype(np.float64), ref[n])
        assert e < 2e-5, f"{what}{n}: relative error {e}"


def check_fwd(y, ref, what=""):
    torch.cuda.synchronize()
    assert tuple(y.shape) == ref.shape, (what, tuple(y.shape), ref.shape)
    e = maxabs(y.cpu().numpy(), ref)
    assert e < 1e-4, f"{what}: max |error| {e}"


def hc_check(ops, seed, B, T, C, k, rate, padding, fwd=False):
    rng = np.random.default_rng(seed)
    p, x, dy = hc_params(rng, C, k), f64(rng, B, T, C), f64(rng, B, T, C)
    pd = up(p)
    if fwd:
        check_fwd(ops.hc_forward(dev(x), pd, rate=rate, padding=padding), TR.hc_fwd(x, p, rate, padding), "hc_forward")
    else:
        check_grads(ops.hc_backward(dev(x), dev(dy), pd, rate=rate, padding=padding), TR.hc_bwd(x, p, dy, rate, padding), HC_NAMES)


def c_check(ops, seed, B, T, Cin, Cout, k, rate, padding, act, fwd=False):
    rng = np.random.default_rng(seed)
    p, x, dy = c_params(rng, Cin, Cout, k), f64(rng, B, T, Cin), f64(rng, B, T, Cout)
    pd = up(p)
    if fwd:
        check_fwd(ops.conv1d_forward(dev(x), pd, rate=rate, padding=padding, act=act), TR.c_fwd(x, p, rate, padding, act), "conv1d_forward")
    else:
        check_grads(ops.conv1d_backward(dev(x), dev(dy), pd, rate=rate, padding=padding, act=act), TR.c_bwd(x, p, dy, rate, padding, act), C_NAMES)


# ------------------------------------------------------------------------------------------------ 1. row kernels past 1024 rows
# nblk = min(256, ceil(B T / 4)) workgroups of 4 waves: above 1024 rows a wave takes a second row (r += gridDim.x * 4) and a workgroup's column sums
# (part[blockIdx.x] -> colsum6_kernel / colsum3_kernel) hold more than one row group.  Row counts that are no multiple of 4: the last group is ragged.
@pytest.mark.parametrize("B,T,C,k,rate,padding", [
    (5, 207, 256, 3, 3, "causal"),     # 1035 rows, hc_bwd_rows_kernel<1>: rows > 1024: `r += gridDim.x * 4`; the stride crosses utterance boundaries (b = r / T)
    (3, 345, 512, 3, 27, "same"),      # 1035 rows, hc_bwd_rows_kernel<2>: the stride with h_off = x_off = 27 pad rows on both sides
    (1, 1029, 1024, 1, 1, "same"),     # 1029 rows, hc_bwd_rows_kernel<4>: the stride at k = 1 (no padding rows at all), one utterance
])
def test_hc_backward_past_the_row_cap(ops, B, T, C, k, rate, padding):
    hc_check(ops, 1100 + C + rate, B, T, C, k, rate, padding)


@pytest.mark.parametrize("B,T,Cin,Cout,k,rate,padding,act", [
    (5, 207, 80, 256, 1, 1, "causal", "relu"),      # 1035 rows, c_bwd_rows_kernel<1>: rows > 1024: `r += gridDim.x * 4`
    (3, 343, 256, 512, 3, 2, "same", "sigmoid"),    # 1029 rows, c_bwd_rows_kernel<2>: the stride with pad rows (k = 3, rate 2) and the sigmoid branch
    (1, 1026, 512, 1024, 1, 1, "same", None),       # 1026 rows, c_bwd_rows_kernel<4>
    (1, 1030, 256, 80, 1, 1, "causal", None),       # 1030 rows, c_bwd_rows_generic_kernel<2> (C <= 128): the stride over scalar lanes
    (1, 1027, 1024, 1025, 1, 1, "same", None),      # 1027 rows, c_bwd_rows_generic_kernel<17> with Cp = 1028 != C: the stride over rows of the padded width
])
def test_conv1d_backward_past_the_row_cap(ops, B, T, Cin, Cout, k, rate, padding, act):
    c_check(ops, 1200 + Cin + Cout, B, T, Cin, Cout, k, rate, padding, act)


def d_check(ops, seed, B, T, Cin, Cout, fwd):
    rng = np.random.default_rng(seed)
    p, x, dy = d_params(rng, Cin, Cout), f64(rng, B, T, Cin), f64(rng, B, 2 * T, Cout)
    pd = up(p)
    check_grads(ops.conv1d_transpose_backward(dev(x), dev(dy), pd), TR.d_bwd(x, p, dy), C_NAMES, "conv1d_transpose_backward ")
    if fwd:
        check_fwd(ops.conv1d_transpose_forward(dev(x), pd), TR.d_fwd(x, p), "conv1d_transpose_forward")


def test_conv1d_transpose_backward_past_the_row_cap(ops):
    d_check(ops, 1300, 1, 517, 512, 512, fwd=False)     # 2 T = 1034 output rows: launch_c_rows -> c_bwd_rows_kernel<2> with rows > 1024 and Tp = 2 (T + 1), h_off = 2


# ------------------------------------------------------------------------------------------------ 2. shapes and edges never compared
@pytest.mark.parametrize("B,T,Cin,Cout", [
    (2, 19, 128, 256),     # Cin != Cout: wsz = Cout * Cin, six strided GEMMs with lda = 2 Cout / Cin; the row part on c_bwd_rows_kernel<1>
    (2, 19, 256, 132),     # Cout no multiple of 128 and > 128: the row part on c_bwd_rows_generic_kernel<17>, a ragged N tile in every GEMM
])
def test_conv1d_transpose_unequal_widths(ops, B, T, Cin, Cout):
    d_check(ops, 1400 + Cin + Cout, B, T, Cin, Cout, fwd=True)


@pytest.mark.parametrize("Cin,Cout", [(130, 128), (128, 130), (128, 1092)])      # Cin & 3, Cout & 3, Cout > 1088
def test_conv1d_transpose_rejects_bad_widths(ops, Cin, Cout):
    from dc_tts_amd.engine import DcttsError
    z = lambda *s: torch.zeros(*s, device="cuda")
    p = {"kernel": z(1, 3, Cout, Cin), "bias": z(Cout), "gamma": z(Cout), "beta": z(Cout)}
    with pytest.raises(DcttsError):
        ops.conv1d_transpose_backward(z(1, 2, Cin), z(1, 4, Cout), p)
    with pytest.raises(DcttsError):
        ops.conv1d_transpose_forward(z(1, 2, Cin), p)


@pytest.mark.parametrize("B,T", [
    (2, 60),     # SAME, dilation 27 (TextEnc HC_7 / HC_11): pl = pr = 27, T > 27: the outer taps read the neighbouring utterance's padding and real rows
    (2, 12),     # T < 27: the outer taps read nothing but padding (Tp = 66 for 12 rows)
])
def test_hc_same_padding_at_dilation_27(ops, B, T):
    hc_check(ops, 1500 + T, B, T, 512, 3, 27, "same")
    hc_check(ops, 1500 + T, B, T, 512, 3, 27, "same", fwd=True)


def test_fewer_rows_than_waves(ops):
    hc_check(ops, 1601, 1, 1, 256, 3, 1, "causal")                 # B T = 1 < 4: one workgroup, three waves skip the row loop and still write their (zero) column sums
    hc_check(ops, 1602, 3, 1, 512, 3, 9, "same")                   # T = 1 with dilation 9: Tp = 19 rows per utterance for one real row, B T = 3
    c_check(ops, 1603, 1, 2, 256, 80, 1, 1, "causal", None)        # B T = 2 on c_bwd_rows_generic_kernel<2>


def test_attention_past_one_tile(ops):
    """T = 131, N = 181 (the workload: 210, 180): the batched GEMMs with M and N above one 128-wide tile, ragged second tiles, K = N = 181 contractions
    over a leading dimension Np = 184, K = T = 131 in the transposed products.  Bounds of test_attention_and_embed_backward_vs_oracle."""
    from dc_tts_amd.hyperparams import hp
    rng = np.random.default_rng(1700)
    B, T, N, d = 2, 131, 181, 256
    Q, K, V, dR, dAl = f64(rng, B, T, d), f64(rng, B, N, d), f64(rng, B, N, d), f64(rng, B, T, 2 * d), f64(rng, B, N, T)
    rQ, rK, rV = TR.attention_bwd(Q, K, V, dR, dAl, d)
    gQ, gK, gV = ops.attention_backward(dev(Q), dev(K), dev(V), dev(dR), dev(dAl))
    check_grads({"dQ": gQ, "dK": gK, "dV": gV}, {"dQ": rQ, "dK": rK, "dV": rV}, ("dQ", "dK", "dV"))
    Rr, alr, _ = O.Attention(Q, K, V, hp)
    Rg, alg = ops.attention_forward(dev(Q), dev(K), dev(V))
    torch.cuda.synchronize()
    assert tuple(Rg.shape) == (B, T, 2 * d) and tuple(alg.shape) == (B, N, T)
    eR, eA = maxabs(Rg.cpu().numpy(), Rr), maxabs(alg.cpu().numpy(), alr)
    assert eR < 1e-4 and eA < 1e-5, (eR, eA)
    colsum = alg.cpu().numpy().astype(np.float64).sum(axis=1)       # alignments = A^T: every decoder step's weights over the N characters
    assert np.abs(colsum - 1.0).max() < 1e-5, np.abs(colsum - 1.0).max()


@pytest.mark.parametrize("B,T,C,k,rate,padding", [
    (2, 37, 256, 3, 3, "causal"),      # hc_fwd_rows_kernel<1>
    (2, 41, 512, 3, 3, "same"),        # hc_fwd_rows_kernel<2>
    (1, 24, 1024, 3, 1, "same"),       # hc_fwd_rows_kernel<4>
])
def test_hc_forward_vs_oracle(ops, B, T, C, k, rate, padding):
    hc_check(ops, 1800 + C, B, T, C, k, rate, padding, fwd=True)


@pytest.mark.parametrize("B,T,Cin,Cout,k,rate,padding,act", [
    (2, 37, 80, 256, 1, 1, "causal", "relu"),       # c_fwd_rows_kernel, relu; Cin = 80
    (2, 21, 256, 80, 1, 1, "causal", None),         # C = 80: most of the 17 channel slots of a lane are empty
    (1, 12, 1024, 1025, 1, 1, "same", None),        # Cp = 1028 != C = 1025: rows of the padded width, the 17th slot holds one channel
    (1, 10, 1025, 1025, 1, 1, "same", "relu"),      # Cinp != Cin as well: pad_rows_generic_kernel and the zero-padded kernel copy
    (2, 33, 256, 256, 3, 2, "causal", "sigmoid"),   # k = 3, rate 2 and the sigmoid branch
])
def test_conv1d_forward_vs_oracle(ops, B, T, Cin, Cout, k, rate, padding, act):
    c_check(ops, 1900 + Cin + Cout, B, T, Cin, Cout, k, rate, padding, act, fwd=True)


def test_embed_forward_is_a_lookup(ops):
    rng = np.random.default_rng(2000)
    vocab, e = 32, 128
    table = rng.normal(0, 1, (vocab, e)).astype(np.float32)
    ids = rng.integers(0, vocab, (4, 60)).astype(np.int32)
    ids[0, :3] = 0; ids[1, 5] = vocab; ids[2, 7] = vocab + 9; ids[3, -1] = 2 ** 31 - 1          # row 0 reads zeros (modules.py:36-38); ids past the table read zeros
    want = np.where(((ids > 0) & (ids < vocab))[..., None], table[np.clip(ids, 0, vocab - 1)], np.float32(0))
    got = ops.embed_forward(torch.from_numpy(ids).cuda(), torch.from_numpy(table).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and np.abs(want).max() > 0


def test_sigmoid_over_the_whole_range(ops):
    rng = np.random.default_rng(2100)
    x = np.concatenate((np.linspace(-100, 100, 4001), rng.normal(0, 3, 5000), [-100.0, -88.0, -17.0, 0.0, 17.0, 88.0, 100.0])).astype(np.float32)
    y = ops.sigmoid(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.isfinite(y).all() and y.min() >= 0.0 and y.max() <= 1.0
    assert maxabs(y, 1.0 / (1.0 + np.exp(-x.astype(np.float64)))) < 1e-6


# ------------------------------------------------------------------------------------------------ 3. losses past the grid cap
# loss_blocks() = min(1024, ceil(n / 2048)): above 1024 * 2048 = 2 097 152 elements a thread of l1_bd_loss_kernel / att_loss_kernel takes a ninth element.
def test_ssrn_losses_past_the_grid_cap(ops):
    rng = np.random.default_rng(2200)
    shape = (1, 2052, 1025)                                         # 2 103 300 elements: 6 148 of them are reached only by the ninth trip of the loop
    n = int(np.prod(shape))
    logits = f64(rng, *shape, sd=2.0)
    Z = r32(1 / (1 + np.exp(-logits)))
    mags = r32(rng.uniform(0, 1, shape))
    idx = rng.choice(n, 4096, replace=False)                        # exact 0 / 1 targets, the tail of the array included
    idx[:64] = n - 1 - np.arange(64) * 96
    zero, one = idx[:2048], idx[2048:]
    mags.reshape(-1)[zero] = 0.0; mags.reshape(-1)[one] = 1.0
    Zf = Z.reshape(-1)
    Zf[zero[:24]] = 0.0; Zf[zero[24:48]] = 1.0                      # d = 0 (sign 0) and d = +1
    Zf[one[:24]] = 1.0; Zf[one[24:48]] = 0.0                        # d = 0 and d = -1
    (m1, m2), (dZ, dZl) = TR.ssrn_losses(Z, logits, mags)
    assert int((dZ == 0).sum()) >= 48
    ls, gZ, gZl = ops.ssrn_losses(dev(Z), dev(logits), dev(mags))
    torch.cuda.synchronize()
    print("ssrn losses", ls.cpu().numpy(), (m1, m2))
    np.testing.assert_allclose(ls.cpu().numpy(), [m1, m2], rtol=2e-5)
    gZ = gZ.cpu().numpy()
    assert rel(gZ, dZ) < 1e-6 and rel(gZl.cpu().numpy(), dZl) < 2e-5
    assert np.array_equal(gZ == 0, dZ == 0)


def test_text2mel_losses_past_the_grid_cap(ops):
    rng = np.random.default_rng(2300)
    B, T, M, N, max_N, max_T = 16, 730, 80, 180, 180, 210           # alignments: 2 102 400 elements, T > max_T: the crop branch (t < max_T) inside the strided loop
    logits = f64(rng, B, T, M, sd=2.0)
    Y = r32(1 / (1 + np.exp(-logits)))
    mels = r32(rng.uniform(0, 1, (B, T, M)))
    al = rng.uniform(0, 1, (B, N, T)); al /= al.sum(axis=1, keepdims=True); al = r32(al)
    (l1, l2, l3), (dY, dlog, dA) = TR.text2mel_losses(Y, logits, mels, al, max_N, max_T)
    losses, gY, glog, gA = ops.text2mel_losses(dev(Y), dev(logits), dev(mels), dev(al), max_N, max_T)
    torch.cuda.synchronize()
    print("text2mel losses", losses.cpu().numpy(), (l1, l2, l3))
    np.testing.assert_allclose(losses.cpu().numpy(), [l1, l2, l3], rtol=2e-5)
    gA = gA.cpu().numpy()
    assert rel(gY.cpu().numpy(), dY) < 1e-6 and rel(glog.cpu().numpy(), dlog) < 2e-5 and rel(gA, dA) < 2e-5
    assert not gA[:, :, max_T:].any() and gA[:, :, :max_T].any()    # train.py:93: what the crop drops gets no gradient


# ------------------------------------------------------------------------------------------------ 4. the tape
class _Layer:
    """One block with its parameters on both sides, its input from the oracle's forward pass and its output gradient from the oracle's reverse pass."""
    def __init__(self, kind, p, rate=1, act=None):
        self.kind, self.p, self.pd, self.rate, self.act = kind, p, up(p), rate, act
        self.names = HC_NAMES if kind == "hc" else C_NAMES

    def fwd_ref(self, x):
        return TR.hc_fwd(x, self.p, self.rate, "causal") if self.kind == "hc" else TR.c_fwd(x, self.p, self.rate, "causal", self.act)

    def bwd_ref(self, x, dy):
        return TR.hc_bwd(x, self.p, dy, self.rate, "causal") if self.kind == "hc" else TR.c_bwd(x, self.p, dy, self.rate, "causal", self.act)

    def fwd(self, ops, x):
        return ops.hc_forward(x, self.pd, rate=self.rate, padding="causal") if self.kind == "hc" else ops.conv1d_forward(x, self.pd, rate=self.rate, padding="causal", act=self.act)

    def bwd(self, ops, x, dy):
        if self.kind == "hc":
            return ops.hc_backward(x, dy, self.pd, rate=self.rate, padding="causal")
        return ops.conv1d_backward(x, dy, self.pd, rate=self.rate, padding="causal", act=self.act)


class _Chain:
    """Layers in forward order.  Every layer is compared on its own: its input is the oracle's (rounded to fp32), its dy the oracle's dx of the layer behind it
    (rounded to fp32), so the single-block bound applies to each.  The device tensors are made once: a tape entry is matched by the kernel's pointer."""
    def __init__(self, layers, x, dy_last):
        self.layers, self.x, self.dy, self.ref = layers, [], [None] * len(layers), [None] * len(layers)
        for L in layers:
            self.x.append(x)
            x = r32(L.fwd_ref(x))
        g = dy_last
        for i in reversed(range(len(layers))):
            self.dy[i] = g
            self.ref[i] = layers[i].bwd_ref(self.x[i], g)
            g = r32(self.ref[i]["dx"])
        self.xd, self.dyd = [dev(a) for a in self.x], [dev(a) for a in self.dy]

    def forward(self, ops):
        for L, x in zip(self.layers, self.xd):
            L.fwd(ops, x)

    def backward(self, ops, order):
        return {i: self.layers[i].bwd(ops, self.xd[i], self.dyd[i]) for i in order}

    def check(self, got, what):
        for i, g in got.items():
            check_grads(g, self.ref[i], self.layers[i].names, f"{what}, layer {i + 1}: ")


@pytest.fixture(scope="module")
def chain():
    """conv1d 80 -> 256 relu, hc 256 k = 3 rate 3, conv1d 256 -> 80, all causal, B, T = 2, 37: three distinct kernels; the 80-wide layer is kept on the tape at a
    padded width that equals its width (Chp == Ch = 80 is a multiple of 4) and read by the scalar-lane row kernel, the hc entry is 512 wide."""
    rng = np.random.default_rng(2400)
    layers = [_Layer("c", c_params(rng, 80, 256, 1), act="relu"), _Layer("hc", hc_params(rng, 256, 3), rate=3), _Layer("c", c_params(rng, 256, 80, 1))]
    return _Chain(layers, r32(rng.uniform(0, 1, (2, 37, 80))), f64(rng, 2, 37, 80))


@pytest.fixture(scope="module")
def wide():
    """conv1d 1024 -> 1025 at T = 12: `Chp != Ch` on the tape (the entry is R x 1028 floats, the backward pass reads it at that width)."""
    rng = np.random.default_rng(2500)
    return _Chain([_Layer("c", c_params(rng, 1024, 1025, 1))], f64(rng, 1, 12, 1024), f64(rng, 1, 12, 1025))


def _same(a, b, what):
    torch.cuda.synchronize()
    for i in a:
        for n in a[i]:
            assert torch.equal(a[i][n], b[i][n]), f"{what}, layer {i + 1}, {n}: the taped and the recomputed pre-norm tensor come from the same GEMM on the same inputs"


@pytest.mark.parametrize("which", ["chain", "wide"])
def test_tape_hit_path(ops, request, which):
    """tape(True), forward, backward in reverse order: every backward pass finds its entry on top (conv_prenorm's match branch: no GEMM, H from the entry)."""
    c = request.getfixturevalue(which)
    order = list(reversed(range(len(c.layers))))
    try:
        ops.tape(True)
        c.forward(ops)
        taped = c.backward(ops, order)
        c.check(taped, "tape hit")
        ops.tape(False)
        plain = c.backward(ops, order)
        c.check(plain, "tape off")
        _same(taped, plain, "hit against off")
    finally:
        ops.tape(False)


def test_tape_out_of_step(ops, chain):
    """conv_prenorm's mismatch branch: the entry on top belongs to another layer (or the same layer at another T): recompute, and tape_n = 0 keeps every later call
    of the step off the entries that are left."""
    try:
        for order in ([0, 1, 2], [2, 0, 1]):              # layer 1 first: nothing matches;  layer 3 hits, layer 1 meets layer 2's entry, layer 2 then finds the tape empty
            ops.tape(True)
            chain.forward(ops)
            chain.check(chain.backward(ops, order), f"backward order {order}")
        # the same kernel pointer, another T: the entry of the forward pass at T = 37 must not serve a backward pass at T = 29
        L, T2 = chain.layers[2], 29
        x2, dy2 = np.ascontiguousarray(chain.x[2][:, :T2]), np.ascontiguousarray(chain.dy[2][:, :T2])
        ops.tape(True)
        L.fwd(ops, chain.xd[2])
        check_grads(L.bwd(ops, dev(x2), dev(dy2)), L.bwd_ref(x2, dy2), L.names, "T = 29 after a taped forward pass at T = 37: ")
    finally:
        ops.tape(False)


def test_tape_does_not_grow_and_switches_off(chain, wide):
    """A second identical step reuses the entries of the first (reserve() on a TapeEntry of the same size); the entries are the padded pre-norm tensors
    (R = B (T + pl + pr) rows of Chp floats); after tape(False) a backward pass recomputes."""
    from dc_tts_amd.train import TrainOps
    o = TrainOps()
    try:
        def sweep(c):
            c.forward(o)
            return c.backward(o, list(reversed(range(len(c.layers)))))
        o.tape(False)
        sweep(chain); sweep(wide)                          # every workspace at its final size, nothing on the tape
        b0 = o.device_bytes()
        o.tape(True); sweep(chain); b1 = o.device_bytes()
        o.tape(True); got = sweep(chain); b2 = o.device_bytes()
        chain.check(got, "second taped step")
        assert b1 - b0 == 4 * (2 * 37 * 256 + 2 * (37 + 6) * 512 + 2 * 37 * 80), (b0, b1)     # k = 1: no pad rows; hc k = 3 rate 3 causal: pl = 6
        assert b2 == b1, (b1, b2)
        o.tape(True); sweep(wide); b3 = o.device_bytes()
        assert b3 == b2, (b2, b3)                          # the 1024 -> 1025 entry (12 rows x Chp = 1028 floats) fits the first entry's buffer (74 x 256): reused, not added
        o.tape(False)
        chain.check(chain.backward(o, [2, 1, 0]), "after tape(False)")
        assert o.device_bytes() == b3
    finally:
        o.close()


def test_train_graph_is_the_same_with_and_without_the_tape():
    """TrainGraph.loss_and_grads turns the tape on for every step; the same step with the tape kept off must give the same bits (losses and all 209 gradients)."""
    from dc_tts_amd.hyperparams import hp
    from dc_tts_amd.train import TrainGraph
    rng = np.random.default_rng(71)                       # the tiny Text2Mel batch of test_gpu_train.test_train_steps_vs_oracle
    W0 = _small_weights(hp, 80)
    B, N, T = 2, 12, 10
    ids = torch.from_numpy(rng.integers(1, len(hp.vocab), (B, N)).astype(np.int32)).cuda()
    mels = dev(rng.uniform(0, 1, (B, T, hp.n_mels)))
    g = TrainGraph(1, W0, hp, training=False)
    try:
        la, ga = g.loss_and_grads(ids, mels)
        tape = g.ops.tape
        g.ops.tape = lambda enable: tape(False)
        lb, gb = g.loss_and_grads(ids, mels)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and set(ga) == set(gb) and len(ga) == 209
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n
    finally:
        g.ops.close()


# ------------------------------------------------------------------------------------------------ 5. one handle, any history
def _history_case(name):
    rng = np.random.default_rng(2600)
    rnd = lambda *s: dev(rng.normal(0, 1, s))
    if name == "hc":
        p, x, dy = up(hc_params(rng, 256, 3)), rnd(2, 37, 256), rnd(2, 37, 256)
        return lambda o: o.hc_backward(x, dy, p, rate=1, padding="causal")
    if name == "conv1d":
        p, x, dy = up(c_params(rng, 256, 80, 1)), rnd(2, 21, 256), rnd(2, 21, 80)
        return lambda o: o.conv1d_backward(x, dy, p, padding="causal")
    p, x, dy = up(d_params(rng, 256, 256)), rnd(3, 16, 256), rnd(3, 32, 256)
    return lambda o: o.conv1d_transpose_backward(x, dy, p)


def _fill_workspaces(o):
    """Larger calls of other geometries on NaN inputs: every workspace (xp, Hp, dHp, dxp, part, wpart, wpad, att) is left full of NaN, so a single stale element
    read by a later call shows in its result even where it is multiplied by zero."""
    rng = np.random.default_rng(2700)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    o.hc_backward(nan(3, 345, 512), nan(3, 345, 512), up(hc_params(rng, 512, 3)), rate=27, padding="same")
    o.conv1d_backward(nan(1, 40, 1024), nan(1, 40, 1025), up(c_params(rng, 1024, 1025, 1)), padding="same")
    o.attention_backward(nan(2, 131, 256), nan(2, 181, 256), nan(2, 181, 256), nan(2, 131, 512), nan(2, 181, 131))


@pytest.mark.parametrize("name", ["hc", "conv1d", "transpose"])
def test_result_does_not_depend_on_the_handles_history(name):
    """reserve() grows a workspace and never clears it: a call must write every element it later reads."""
    from dc_tts_amd.train import TrainOps
    run = _history_case(name)
    fresh, used = TrainOps(), TrainOps()
    try:
        a = run(fresh)
        _fill_workspaces(used)
        b = run(used)
        torch.cuda.synchronize()
        for n in a:
            assert torch.isfinite(a[n]).all(), n
            assert torch.equal(a[n], b[n]), f"{name} {n}: differs on a handle that ran larger calls before"
    finally:
        fresh.close(); used.close()
