"""One training step of each network at the training batch (B = 32, T = 210, N = 180): wall time per step and the part of it the host
spends enqueueing (perf_counter around the calls, before the synchronize) -- says whether the step is launch/host-bound or GPU-bound.
--terms 0,3 times the fp32 and the three-term split-bf16 contractions (TrainGraph(split_bf16_terms=...)) in ONE run, alternating windows."""
import argparse, os, sys, time, torch
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', '/root/repo'))
from dc_tts_amd.hyperparams import hp
from dc_tts_amd.train import TrainGraph
from dc_tts_amd.weights import synthetic_weights
ap = argparse.ArgumentParser()
ap.add_argument("--terms", default="0", help="comma-separated forms to time in this run: 0 = fp32 MFMA, 3 = three-term split bf16")
forms = [int(v) for v in ap.parse_args().terms.split(",")]
B, T, N = 32, 210, 180
Wn = synthetic_weights(hp, seed=1)
ids = torch.randint(1, len(hp.vocab), (B, N), dtype=torch.int32, device="cuda")
for num, name in ((1, "Text2Mel"), (2, "SSRN")):
    batch = (ids, torch.rand(B, T, hp.n_mels, device="cuda")) if num == 1 else \
        (torch.rand(B, T, hp.n_mels, device="cuda"), torch.rand(B, 4 * T, hp.n_linear, device="cuda"))
    gs = {f: TrainGraph(num, Wn, hp, split_bf16_terms=f) for f in forms}
    for g in gs.values():
        for _ in range(2): g.train_op(*batch)
    torch.cuda.synchronize()
    n, best = 5, {}
    for rep in range(3):                                   # alternating windows of n steps; the best window of each form is reported
        for f, g in gs.items():
            t0 = time.perf_counter()
            for _ in range(n): g.train_op(*batch)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if f not in best or t2 - t0 < best[f][0]: best[f] = (t2 - t0, t1 - t0)
    for f, (tt, th) in best.items():
        print(f"{name} terms={f}: {1e3 * tt / n:.2f} ms/step, host enqueue {1e3 * th / n:.2f} ms/step, {B * n / tt:.0f} utterances/s"
              + (f", {tt / best[forms[0]][0]:.3f} x the terms={forms[0]} time" if f != forms[0] else ""))
    del gs
