"""Generate tests/golden/g13_attn_mha.npz from the REAL 2nd-stage reference built with --attention_type nn.MultiheadAttention (TEST INFRA,
needs the reference tree; CPU only).

    python -m tools.gen_golden_attn_mha [--ref <checkout of the reference>/src/CountDETR_147_2nd_stage]

Weights: oracle.weights.seeded_state_dict(attn_mha_schema(), heads="wide") -- the stage-2 schema with the encoder `self_attn.*` and the decoder
`cross_attn.*` input projections of nn.MultiheadAttention's shapes ([3E,E] / [3E]); the tests rebuild the same weights from this function.
Cases (inputs regenerated from their seeds with oracle.step on both sides, never stored):
  b1_384x576  one 384x576 image: 864 keys against 300 queries (Lk > Lq);
  b1_128x160  one 128x160 image: 80 keys against 300 queries (Lk < Lq);
  b2_pad      two images of different sizes (128x160, 96x128) padded into one batch: the attention runs over the padded positions too.
Stored per case, as in g10_full.npz: outputs, reference points, Hungarian indices, losses, the total gradient norm, per-parameter clipped
gradient norms (-1 = no gradient) and parameter sums after one AdamW step, and the conditioning of the assignment (`min_swap_gap`) and of
the L1 loss (`min_l1_margin`).  Plus the reference variant's state-dict keys and shapes (`state_dict_keys`, `state_dict_shapes`).
Single-threaded CPU arithmetic, so that the committed file is reproducible bit for bit.
"""
import argparse
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g13_attn_mha.npz")

CASES = {
    "b1_384x576": dict(sizes=[(384, 576)], Ts=(11,), seed=1301),
    "b1_128x160": dict(sizes=[(128, 160)], Ts=(7,), seed=1302),
    "b2_pad": dict(sizes=[(128, 160), (96, 128)], Ts=(7, 13), seed=1303),
}


def attn_mha_schema(**kw):
    """oracle.weights.model_schema(**kw) with nn.MultiheadAttention's input projections in the encoder self-attention and the decoder
    cross-attention (the RCDA ones are [5E,E] / [5E])."""
    from oracle.weights import model_schema
    out = []
    for name, shape, kind in model_schema(**kw):
        if (".self_attn.in_proj" in name and ".encoder_layers." in name) or ".cross_attn.in_proj" in name:
            shape = (3 * shape[0] // 5,) + tuple(shape[1:])
        out.append((name, shape, kind))
    return out


def make_inputs(c):
    from oracle.step import synthetic_batch, synthetic_images
    if len(c["sizes"]) == 1:
        H, W = c["sizes"][0]
        return synthetic_batch(B=1, H=H, W=W, Ts=c["Ts"], seed=c["seed"])
    return synthetic_images(c["sizes"], c["Ts"], c["seed"])


def run_case(G, name, c, d):
    from models import build_model
    from oracle.gen_golden_full import swap_gap
    from oracle.weights import seeded_state_dict
    model, crit, _ = build_model(G.ref_args(attention_type="nn.MultiheadAttention"))
    model.load_state_dict(seeded_state_dict(attn_mha_schema(), heads="wide"), strict=True)
    model.train(); crit.train()
    images, rects, tg = make_inputs(c)
    B = len(c["sizes"])
    out, ref = model(images, rects=rects)
    losses = crit(out, tg)
    wd = crit.weight_dict
    total = sum(losses[k] * wd[k] for k in losses if k in wd)
    opt = torch.optim.AdamW([{"params": [p for n, p in model.named_parameters() if "backbone" not in n and p.requires_grad], "lr": 1e-4},
                             {"params": [p for n, p in model.named_parameters() if "backbone" in n and p.requires_grad], "lr": 1e-5}],
                            lr=1e-4, weight_decay=1e-4)
    opt.zero_grad()
    total.backward()
    gn = torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
    gclip = np.array([(p.grad.norm().item() if p.grad is not None else -1.0) for n, p in model.named_parameters()])
    idx = crit.matcher(out, tg)
    opt.step()
    psum = np.array([p.detach().double().sum().item() for n, p in model.named_parameters()])
    G.put(d, f"{name}/sizes", np.array(c["sizes"]))
    G.put(d, f"{name}/Ts", np.array(c["Ts"]))
    G.put(d, f"{name}/seed", np.array(c["seed"]))
    for b in range(B):
        G.put(d, f"{name}/idx_i{b}", idx[b][0]); G.put(d, f"{name}/idx_j{b}", idx[b][1])
    for k in ("pred_logits", "pred_boxes", "pred_vars"):
        G.put(d, f"{name}/{k}", out[k])
    G.put(d, f"{name}/ref", ref)
    G.put(d, f"{name}/min_swap_gap", np.array([swap_gap(out, tg, idx, b) for b in range(B)]))
    G.put(d, f"{name}/min_l1_margin", np.array([float((out["pred_boxes"][b][idx[b][0]].detach() - tg[b]["boxes"][idx[b][1]]).abs().min())
                                                if len(idx[b][0]) else np.inf for b in range(B)]))
    for k, v in losses.items():
        G.put(d, f"{name}/L_{k}", v)
    G.put(d, f"{name}/loss_total", total)
    G.put(d, f"{name}/grad_total_norm", gn)
    G.put(d, f"{name}/param_names", np.array([n for n, p in model.named_parameters()]))
    G.put(d, f"{name}/grad_norms_clipped", gclip)
    G.put(d, f"{name}/param_sums_after_step", psum)
    print(name, {k: round(float(v), 6) for k, v in losses.items()}, "gn", float(gn), "gap", d[f"{name}/min_swap_gap"],
          "l1 margin", d[f"{name}/min_l1_margin"], flush=True)
    return model


def main():
    from oracle import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=G.REF, help="the reference's src/CountDETR_147_2nd_stage directory")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    G.install_stubs(a.ref)
    torch.manual_seed(0)
    d = {}
    model = None
    for name, c in CASES.items():
        model = run_case(G, name, c, d)
    sd = model.state_dict()
    d["state_dict_keys"] = np.array(list(sd.keys()))
    d["state_dict_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    np.savez_compressed(a.out, **d)
    print("wrote", a.out, len(d), "arrays")


if __name__ == "__main__":
    main()
