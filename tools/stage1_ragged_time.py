"""What stage 1's ragged batches (`counts`: images with different numbers of points in one batch) cost and buy on one MI355X -> one
JSON line.

    python tools/stage1_ragged_time.py [--out profiles/stage1_ragged_time.json] [--images 32] [--steps 20] [--warmup 5] [--calls 200]

Synthetic images at 384x576, seeded weights.  Every figure is a host clock around work that ends in a device synchronise AND the HIP
events around the same window; alternated rounds, the median is reported with the spread.
  (a) pseudo-label forward (model.eval(), no_grad), images/s: one image per forward (what --generate_pseudo_label does without
      --ragged_batches) against B = 4 and 8 images per forward with counts, over a fixed, seeded list of point counts spanning 7 ... 900
      in list order; the padded-row share of the batches (rows computed and thrown away by the row-wise operators) beside it.
  (b) training step, Stage1Trainer.step at B = 4: counts (3, 3, 3, 3) dense, the same batch through the ragged path, counts (3, 4, 3, 6).
  (c) the self-attention kernels: cdetr_mha_fwd_lens / _bwd_lens at N = 4, L = 900 with lens all 900 against cdetr_mha_fwd / _bwd -- the
      cost of the bound itself -- and with the lens of a mixed batch, in the step's arithmetic (forward bf16x3, backward as ops selects).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 384, 576
DEV = "cuda:0"


def _build():
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    from oracle.weights import seeded_state_dict, stage1_schema
    args = get_args_parser_stage1().parse_args([])
    args.device = DEV
    model, crit, _ = stage1.build(args)
    model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True)
    model.to(DEV)
    return args, model, crit


def _window(fn, reps):
    """(wall seconds, event seconds) of `reps` calls of fn, both ending in a synchronise."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, e0.elapsed_time(e1) / 1e3


def _alternate(variants, reps, rounds=5):
    """Every variant timed `rounds` times in turn (A B C A B C ...): {name: {wall_ms, event_ms (medians per call), wall_ms_min, wall_ms_max}}."""
    seen = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            seen[k].append(_window(fn, reps))
    out = {}
    for k, v in seen.items():
        wall = [w / reps * 1e3 for w, _ in v]
        out[k] = {"wall_ms": round(statistics.median(wall), 4), "event_ms": round(statistics.median(e / reps * 1e3 for _, e in v), 4),
                  "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}
    return out


def point_counts(n, seed=7):
    """A fixed, seeded list of point counts spanning 7 ... 900 (log-uniform: FSC-147's counts are heavy-tailed), both ends included."""
    import numpy as np
    rng = np.random.RandomState(seed)
    c = np.exp(rng.uniform(np.log(7), np.log(900), size=n)).astype(int).tolist()
    c[0], c[-1] = 7, 900
    return c


def pseudo_label_forward(n_images):
    import torch
    from counting_detr_amd import stage1
    _, model, _ = _build()
    model.eval()
    counts = point_counts(n_images)
    g = torch.Generator().manual_seed(11)
    images = torch.randn(8, 3, H, W, generator=g).to(DEV)                     # (eight distinct images, cycled: the content does not matter)
    pts = [(torch.rand(c, 2, generator=g) * 0.9 + 0.05).to(DEV) for c in counts]

    def batches(B):
        out = []
        for i in range(0, n_images, B):
            cs = counts[i:i + B]
            p = torch.full((len(cs), max(cs), 2), 0.5, device=DEV)
            for b, c in enumerate(cs):
                p[b, :c] = pts[i + b]
            out.append((images[:len(cs)], p, torch.tensor(cs, dtype=torch.int32, device=DEV)))
        return out

    plans = {B: batches(B) for B in (4, 8)}

    def one_by_one():
        for i, p in enumerate(pts):
            stage1.generate_pseudo_boxes(model, images[i % 8:i % 8 + 1], p[None])

    def batched(B):
        def run():
            for im, p, c in plans[B]:
                stage1.generate_pseudo_boxes(model, im, p, c)
        return run

    variants = {"B1": one_by_one, "B4_ragged": batched(4), "B8_ragged": batched(8)}
    for fn in variants.values():                                              # warm-up: every shape of the timed window
        fn()
    res = _alternate(variants, 1, rounds=3)
    for k, v in res.items():
        v["img_s"] = round(n_images / (v["wall_ms"] / 1e3), 1)
    for B in (4, 8):
        rows = sum(p.shape[0] * p.shape[1] for _, p, _ in plans[B])
        res[f"B{B}_ragged"]["padded_row_share"] = round(1 - sum(counts) / rows, 4)
    return {"images": n_images, "point_counts": counts, **res}


def training_step(steps, warmup):
    import torch
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = _build()
    model.train()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    g = torch.Generator().manual_seed(5004)
    img = torch.randn(4, 3, H, W, generator=g).to(DEV)

    def batch(counts):
        n = max(counts)
        p, w = torch.rand(4, n, 2, generator=g) * 0.6 + 0.2, torch.rand(4, n, 2, generator=g) * 0.15 + 0.03
        for b, c in enumerate(counts):
            p[b, c:], w[b, c:] = 0.5, 0.0
        return p.to(DEV), w.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)

    p3, w3, c3 = batch((3, 3, 3, 3))
    p6, w6, c6 = batch((3, 4, 3, 6))
    variants = {"dense_3333": lambda: tr.step(img, p3, w3), "ragged_3333": lambda: tr.step(img, p3, w3, counts=c3),
                "ragged_3436": lambda: tr.step(img, p6, w6, counts=c6)}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    res = _alternate(variants, steps)
    for v in res.values():
        v["img_s"] = round(4 / (v["wall_ms"] / 1e3), 1)
    res["captures"] = tr.cache_stats["captures"]
    res["nonfinite_steps"] = tr.nonfinite_steps()
    return res


def attention_kernels(calls):
    import torch
    from counting_detr_amd import ops
    N, L, E, nh = 4, 900, 256, 8
    g = torch.Generator().manual_seed(3)
    qk, v, go = (torch.randn(N, L, w, generator=g).to(DEV) for w in (2 * E, E, E))
    full = torch.full((N,), L, dtype=torch.int32, device=DEV)
    mixed = torch.tensor([900, 37, 300, 7], dtype=torch.int32, device=DEV)
    o, lse = ops.mha_fwd_raw(qk, v, nh)
    fwd = {"dense": lambda: ops.mha_fwd_raw(qk, v, nh), "lens_full": lambda: ops.mha_fwd_raw(qk, v, nh, full),
           "lens_900_37_300_7": lambda: ops.mha_fwd_raw(qk, v, nh, mixed)}
    bwd = {"dense": lambda: ops.mha_bwd_raw(qk, v, o, go, lse, nh), "lens_full": lambda: ops.mha_bwd_raw(qk, v, o, go, lse, nh, full),
           "lens_900_37_300_7": lambda: ops.mha_bwd_raw(qk, v, o, go, lse, nh, mixed)}
    for fn in list(fwd.values()) + list(bwd.values()):
        for _ in range(10):
            fn()
    return {"N": N, "L": L, "calls_per_window": calls, "precision": ops.PRECISION, "bwd_precision": ops.bwd_precision() if ops.MHA_BWD_BF16 else ops.PRECISION,
            "note": "per call, output allocation included on both sides", "fwd": _alternate(fwd, calls), "bwd": _alternate(bwd, calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stage1_ragged_time.py measures on the GPU: none found")
    line = {"what": "stage-1 ragged batches: pseudo-label forward, training step, self-attention kernels", "size": [H, W],
            "device": torch.cuda.get_device_name(0),
            "c_attention_kernels": attention_kernels(a.calls), "b_training_step": training_step(a.steps, a.warmup),
            "a_pseudo_label_forward": pseudo_label_forward(a.images)}
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
