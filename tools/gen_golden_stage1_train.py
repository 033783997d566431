"""Generate tests/golden/g12_stage1_train.npz from the REAL 1st-stage reference (TEST INFRA, needs the reference tree; CPU only).

    python -m tools.gen_golden_stage1_train --ref <checkout of the reference>/src/CountDETR_147_1st_stage

Two parts, data only in the output file:
  * training: A1's model (seeded weights, oracle.weights.stage1_schema), A1's optimizer setup (three lr groups over the parameters that
    require a gradient, AdamW(lr 1e-4, weight decay 1e-4), backbone lr 1e-5), its step (loss = sum_k loss_k * weight_dict[k],
    zero_grad, backward, clip_grad_norm_(0.1), AdamW) for STEPS seeded batches at FSC-147 sizes, 3 points each.  Per step: the two losses,
    the weighted total, the clip's total norm (before clipping) and the L1 kink distance min |pred_wh - tgt_whs| (a gradient bar is only well posed away
    from it); per-parameter norms of step 1's raw gradients (-1 = no gradient); after the last step, for every trained parameter, the SAMPLE_K
    elements that moved most (flat index, value before the first step, value after the last).  The batches are regenerated from their
    seeds on both sides (never stored).  Seeds 3100-3102 give a kink distance of >= 1e-3 on every step (checked at generation).
  * readers: A1/datasets/fscd_147.py's FSCD147_Exemplars and FSCD147_Points on tests/golden/fsc147_tiny (every split), with the
    pycocotools / torchvision.transforms stand-ins of oracle/gen_golden_data.py (neither package is installed where this runs).
Single-threaded CPU arithmetic, so that the committed file is reproducible bit for bit.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g12_stage1_train.npz")
DS = os.path.join(ROOT, "tests", "golden", "fsc147_tiny")

STEPS = ((384, 576, 3100), (384, 512, 3101), (384, 576, 3102))      # (H, W, seed) of the three batches
NPTS = 3
SAMPLE_K = 16
KINK_FLOOR = 1e-3


def batch(H, W, seed):
    """The seeded batch of one step: image [1,3,H,W], exemplar centres / sizes [1,3,2] (normalised)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(1, 3, H, W, generator=g)
    pts = torch.rand(1, NPTS, 2, generator=g) * 0.6 + 0.2
    whs = torch.rand(1, NPTS, 2, generator=g) * 0.15 + 0.03
    return img, pts, whs


def model_args():
    return argparse.Namespace(device="cpu", backbone="resnet50", dilation=True, lr_backbone=1e-5, masks=False, num_feature_levels=1,
                              hidden_dim=256, nheads=8, enc_layers=6, dec_layers=6, dim_feedforward=1024, dropout=0.0,
                              num_query_position=300, num_query_pattern=1, spatial_prior="defined", attention_type="RCDA",
                              frozen_weights=None)


def optimizer_groups(model, lr=1e-4, lr_backbone=1e-5, backbone_names=("backbone",), proj_names=(), proj_mult=0.1):
    """A1/main.py:164-201: [neither backbone nor linear_proj names | backbone names | linear_proj names], requires_grad only."""
    def has(n, keys):
        return any(k in n for k in keys)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return [{"params": [p for n, p in named if not has(n, backbone_names) and not has(n, proj_names)], "lr": lr},
            {"params": [p for n, p in named if has(n, backbone_names)], "lr": lr_backbone},
            {"params": [p for n, p in named if has(n, proj_names)], "lr": lr * proj_mult}]


def install(ref):
    from oracle import gen_golden as G
    from oracle import gen_golden_data as D
    D.install_stubs()                          # pycocotools + torchvision.transforms stand-ins
    tvt = sys.modules["torchvision.transforms"]
    G.install_stubs(ref)                       # the model's torchvision symbols (replaces the torchvision module object)
    sys.modules["torchvision"].transforms = tvt
    return G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's src/CountDETR_147_1st_stage directory")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    G = install(a.ref)
    from models import build_model
    from oracle.weights import seeded_state_dict, stage1_schema
    d = {}
    model, crit, _ = build_model(model_args())
    print(model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True))
    model.train()
    crit.train()
    opt = torch.optim.AdamW(optimizer_groups(model), lr=1e-4, weight_decay=1e-4)
    names = [n for n, _ in model.named_parameters()]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    d["steps"] = np.array(STEPS, dtype=np.int64)
    d["param_names"] = np.array(names)
    for s, (H, W, seed) in enumerate(STEPS):
        img, pts, whs = batch(H, W, seed)
        out = model(img, pts)
        losses = crit(out, {"points": pts, "whs": whs})
        total = sum(losses[k] * crit.weight_dict[k] for k in losses.keys() if k in crit.weight_dict)
        opt.zero_grad()
        total.backward()
        if s == 0:                             # raw gradients (before the clip rescales them in place)
            d["grad_norms"] = np.array([(p.grad.norm().item() if p.grad is not None else -1.0) for p in model.parameters()])
        tn = torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
        opt.step()
        kink = float((out["pred_wh"].detach() - whs).abs().min())
        assert kink >= KINK_FLOOR, f"step {s}: |pred_wh - tgt_whs| = {kink:.3e} is near the L1 kink: pick other seeds"
        for k, v in losses.items():
            G.put(d, f"s{s}/{k}", v)
        G.put(d, f"s{s}/loss_total", total)
        G.put(d, f"s{s}/grad_total_norm", tn)
        d[f"s{s}/min_l1_margin"] = np.array(kink)
        print(s, (H, W, seed), {k: float(v) for k, v in losses.items()}, "total", float(total), "norm", float(tn), "kink", kink)
    pidx, fidx, vb, va = [], [], [], []
    for i, (n, p) in enumerate(model.named_parameters()):
        if d["grad_norms"][i] < 0:
            continue
        delta = (p.detach() - before[n]).reshape(-1).abs()
        k = min(SAMPLE_K, delta.numel())
        idx = torch.argsort(delta, descending=True, stable=True)[:k]
        pidx += [i] * k
        fidx += idx.tolist()
        vb += before[n].reshape(-1)[idx].tolist()
        va += p.detach().reshape(-1)[idx].tolist()
    d["sample_pidx"] = np.array(pidx, dtype=np.int64)
    d["sample_fidx"] = np.array(fidx, dtype=np.int64)
    d["sample_before"] = np.array(vb, dtype=np.float32)
    d["sample_after"] = np.array(va, dtype=np.float32)
    # ---- the reference's 1st-stage readers on the tiny FSC-147 fixture
    from datasets import fscd_147 as R
    rargs = argparse.Namespace(data_path=DS, scale_factor=32)
    for split in ("train", "val", "test"):
        for tag, cls in (("ex", R.FSCD147_Exemplars), ("pts", R.FSCD147_Points)):
            ds = cls(rargs, split)
            d[f"{tag}_{split}/len"] = np.array(len(ds))
            for i in range(len(ds)):
                for k, v in ds[i].items():
                    d[f"{tag}_{split}{i}/{k}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    np.savez_compressed(a.out, **d)
    print("wrote", a.out, len(d), "arrays")


if __name__ == "__main__":
    main()
