"""Generate tests/golden/g14_sgd_train.npz from the REAL 2nd-stage reference trained with --sgd (TEST INFRA, needs the reference tree; CPU only).

    python -m tools.gen_golden_sgd_train [--ref <checkout of the reference>/src/CountDETR_147_2nd_stage]

A2's model with oracle.weights.seeded_state_dict weights, A2's optimizer setup for --sgd (A2/main.py:157-189: the three lr groups,
torch.optim.SGD(lr, momentum 0.9, weight decay 1e-4), StepLR(lr_drop)) and its step (A2/engine.py: zero_grad, backward,
clip_grad_norm_(0.1), optimizer step) for three seeded batches (oracle.step.synthetic_batch, B=1, 384x576; never stored).
scheduler.step() runs once between the 2nd and the 3rd step with lr_drop = 1, so the third step runs at 0.1 lr: the lr drop is pinned
while the momentum buffer carries on unscaled.

The reference's lr 1e-4 with the 0.1 clip moves most parameters by less than one fp32 ulp, so the learning rate here is LR (backbone
LR_BACKBONE), recorded in the file; every sampled parameter delta is checked at generation to be >= MIN_ULPS ulps of its value.
Stored, data only:
  * per step: the losses, the weighted total, the clip's total norm (before clipping), the assignment's conditioning (`min_swap_gap`)
    and the L1 kink distance of the matched boxes (`min_l1_margin`);
  * after the last step, per parameter: the momentum buffer's norm (-1 = no state: the parameter never had a gradient);
  * for every trained parameter, the SAMPLE_K elements that moved most: flat index, value before the first step, value after the last,
    momentum buffer after the last.
Seeds 1401-1403 give gaps >= 1e-3 and L1 margins >= 1e-4 on every step (checked at generation).
Single-threaded CPU arithmetic, so that the committed file is reproducible bit for bit.
"""
import argparse
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g14_sgd_train.npz")

STEPS = ((384, 576, 11, 1401), (384, 576, 11, 1402), (384, 576, 11, 1403))     # (H, W, targets, seed) of the three B=1 batches
LR, LR_BACKBONE, WEIGHT_DECAY, MOMENTUM, MAX_NORM = 0.1, 0.05, 1e-4, 0.9, 0.1
DROP_AFTER = 2                 # scheduler.step() after this many steps (StepLR step_size 1: x0.1 from then on)
SAMPLE_K = 16
MIN_ULPS = 64
GAP_FLOOR, L1_FLOOR = 1e-3, 1e-4


def param_dicts(model, lr, lr_backbone, backbone_names=("backbone",), proj_names=(), proj_mult=0.1):
    """A2/main.py:157-183: [neither backbone nor linear_proj names | backbone names | linear_proj names], requires_grad only."""
    def has(n, keys):
        return any(k in n for k in keys)
    named = [(n, p) for n, p in model.named_parameters()]
    return [{"params": [p for n, p in named if not has(n, backbone_names) and not has(n, proj_names) and p.requires_grad], "lr": lr},
            {"params": [p for n, p in named if has(n, backbone_names) and p.requires_grad], "lr": lr_backbone},
            {"params": [p for n, p in named if has(n, proj_names) and p.requires_grad], "lr": lr * proj_mult}]


def batch(H, W, T, seed):
    from oracle.step import synthetic_batch
    return synthetic_batch(B=1, H=H, W=W, Ts=(T,), seed=seed)


def main():
    from oracle import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=G.REF, help="the reference's src/CountDETR_147_2nd_stage directory")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    G.install_stubs(a.ref)
    from models import build_model
    from oracle.gen_golden_full import swap_gap
    from oracle.weights import seeded_state_dict
    torch.manual_seed(0)
    model, crit, _ = build_model(G.ref_args())
    print(model.load_state_dict(seeded_state_dict(), strict=True))
    model.train()
    crit.train()
    opt = torch.optim.SGD(param_dicts(model, LR, LR_BACKBONE), lr=LR, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1)
    names = [n for n, _ in model.named_parameters()]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    d = {"steps": np.array(STEPS, dtype=np.int64), "param_names": np.array(names),
         "hyper": np.array([LR, LR_BACKBONE, WEIGHT_DECAY, MOMENTUM, MAX_NORM, DROP_AFTER], dtype=np.float64)}
    for s, (H, W, T, seed) in enumerate(STEPS):
        if s == DROP_AFTER:
            sched.step()
        images, rects, tg = batch(H, W, T, seed)
        out, _ = model(images, rects=rects)
        losses = crit(out, tg)
        wd = crit.weight_dict
        total = sum(losses[k] * wd[k] for k in losses if k in wd)
        opt.zero_grad()
        total.backward()
        tn = torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)
        idx = crit.matcher(out, tg)
        opt.step()
        gap = swap_gap(out, tg, idx, 0)
        margin = float((out["pred_boxes"][0][idx[0][0]].detach() - tg[0]["boxes"][idx[0][1]]).abs().min())
        assert gap >= GAP_FLOOR and margin >= L1_FLOOR, f"step {s}: swap gap {gap:.3e}, L1 margin {margin:.3e}: pick other seeds"
        for k, v in losses.items():
            G.put(d, f"s{s}/L_{k}", v)
        G.put(d, f"s{s}/loss_total", total)
        G.put(d, f"s{s}/grad_total_norm", tn)
        d[f"s{s}/min_swap_gap"] = np.array(gap)
        d[f"s{s}/min_l1_margin"] = np.array(margin)
        print(s, (H, W, T, seed), "lr", opt.param_groups[0]["lr"], {k: round(float(v), 6) for k, v in losses.items()}, "total", float(total.detach()),
              "norm", float(tn), "gap", gap, "l1 margin", margin, flush=True)
    bnorm, pidx, fidx, vb, va, vm = [], [], [], [], [], []
    for i, (n, p) in enumerate(model.named_parameters()):
        st = opt.state.get(p, {})
        buf = st.get("momentum_buffer")
        bnorm.append(float(buf.norm()) if buf is not None else -1.0)
        if buf is None:
            continue
        delta = (p.detach() - before[n]).reshape(-1).abs()
        k = min(SAMPLE_K, delta.numel())
        sel = torch.argsort(delta, descending=True, stable=True)[:k]
        ulp = torch.finfo(torch.float32).eps * before[n].reshape(-1)[sel].abs().clamp(min=torch.finfo(torch.float32).tiny)
        assert bool((delta[sel] >= MIN_ULPS * ulp).all()), f"{n}: sampled deltas of < {MIN_ULPS} ulps: raise LR"
        pidx += [i] * k
        fidx += sel.tolist()
        vb += before[n].reshape(-1)[sel].tolist()
        va += p.detach().reshape(-1)[sel].tolist()
        vm += buf.reshape(-1)[sel].tolist()
    d["buf_norms"] = np.array(bnorm)
    d["sample_pidx"] = np.array(pidx, dtype=np.int64)
    d["sample_fidx"] = np.array(fidx, dtype=np.int64)
    d["sample_before"] = np.array(vb, dtype=np.float32)
    d["sample_after"] = np.array(va, dtype=np.float32)
    d["sample_buf"] = np.array(vm, dtype=np.float32)
    np.savez_compressed(a.out, **d)
    print("wrote", a.out, len(d), "arrays,", len(pidx), "samples")


if __name__ == "__main__":
    main()
