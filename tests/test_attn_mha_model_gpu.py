"""attention_type "nn.MultiheadAttention" end to end on the MI355X: parity with the real reference variant (tests/golden/g13_attn_mha.npz),
the trainer (eager step, cached graph step in both layouts, adapt_pos1d left alone), the inference engine, and main.py / infer.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["b1_384x576", "b1_128x160", "b2_pad"]


@pytest.fixture(params=[0, 1], ids=["fp32mfma", "bf16x3"])
def precision(request):
    from counting_detr_amd import ops
    old = ops.PRECISION
    ops.PRECISION = request.param
    yield request.param
    ops.PRECISION = old


def build(**kw):
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from oracle.weights import seeded_state_dict
    from tools.gen_golden_attn_mha import attn_mha_schema
    args = default_args(device=DEV, **kw)
    args.attention_type = "nn.MultiheadAttention"
    model, crit, _ = counting_detr_amd.build_model(args)
    model.load_state_dict(seeded_state_dict(attn_mha_schema(num_position=args.num_query_position), heads="wide"), strict=True)
    model.backbone.exemplar_mode = "reference"      # the golden vectors are the reference's: rects[0] for the whole batch
    return model.to(DEV), crit, args


def inputs(z, name):
    from tools.gen_golden_attn_mha import CASES as GEN, make_inputs
    images, rects, tg = make_inputs(GEN[name])
    assert np.array_equal(np.array(GEN[name]["sizes"]), z[f"{name}/sizes"])
    samples = images.to(DEV) if torch.is_tensor(images) else [i.to(DEV) for i in images]
    return samples, rects.to(DEV), [{k: v.to(DEV) for k, v in t.items()} for t in tg]


@pytest.mark.parametrize("name", CASES)
def test_forward_losses_grads_vs_reference(golden, name, precision):
    z = golden("g13_attn_mha.npz")
    samples, rects, tg = inputs(z, name)
    model, crit, _ = build()
    model.train()
    out, ref = model(samples, rects=rects)
    for k in ("pred_logits", "pred_boxes", "pred_vars"):
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), z[f"{name}/{k}"], rtol=1e-3, atol=1e-4, err_msg=k)
    np.testing.assert_allclose(ref.detach().cpu().numpy(), z[f"{name}/ref"], rtol=1e-6)
    idx = crit.matcher(out, tg)
    for b in range(len(tg)):
        assert z[f"{name}/min_swap_gap"][b] > 1e-3                 # well-posed: the assignment is far from a tie
        assert np.array_equal(idx[b][0].numpy(), z[f"{name}/idx_i{b}"])
        assert np.array_equal(idx[b][1].numpy(), z[f"{name}/idx_j{b}"])
    losses = crit(out, tg)
    for k in ("loss_ce", "loss_bbox", "loss_giou", "cardinality_error", "loss_variance", "class_error"):
        np.testing.assert_allclose(float(losses[k]), z[f"{name}/L_{k}"], rtol=1e-3, atol=1e-5, err_msg=k)
    total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
    total.backward()
    params = dict(model.named_parameters())
    grads = [p.grad for p in params.values() if p.grad is not None]
    tn = torch.norm(torch.stack([g.norm() for g in grads])).item()
    np.testing.assert_allclose(tn, z[f"{name}/grad_total_norm"], rtol=2e-3)
    coef = min(1.0, 0.1 / (tn + 1e-6))
    for n, r in zip((str(n) for n in z[f"{name}/param_names"]), z[f"{name}/grad_norms_clipped"]):
        p = params[n]
        if r < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
        else:
            np.testing.assert_allclose(p.grad.norm().item() * coef, r, rtol=1e-2, atol=1e-6, err_msg=n)


@pytest.mark.parametrize("name", CASES)
def test_train_step_matches_reference_adamw(golden, name, precision):
    from counting_detr_amd.engine import Trainer
    z = golden("g13_attn_mha.npz")
    samples, rects, tg = inputs(z, name)
    model, crit, args = build()
    model.train()
    tr = Trainer(model, crit, args, device=DEV)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if "adapt_pos1d" in n}
    out = tr.train_step(samples, rects, tg)
    np.testing.assert_allclose(float(out["grad_norm"]), z[f"{name}/grad_total_norm"], rtol=2e-3)
    params = dict(model.named_parameters())
    for n, s in zip((str(n) for n in z[f"{name}/param_names"]), z[f"{name}/param_sums_after_step"]):
        # tests/test_model_gpu.py's bar: a near-zero gradient whose sign flips under rounding moves the sum by 2 lr
        p = params[n]
        lr = 1e-5 if "backbone" in n else 1e-4
        np.testing.assert_allclose(p.detach().double().sum().item(), s, rtol=1e-4, atol=5e-3 + 0.02 * lr * p.numel(), err_msg=n)
    for n, b in before.items():          # no gradient in the reference: AdamW neither updates nor decays it
        assert torch.equal(params[n].detach(), b), n
    assert not any(k.startswith("transformer.adapt_pos1d") for k in tr.names)


def _batch(seed, B=2, H=128, W=160, Ts=(7, 13)):
    from oracle.step import synthetic_batch
    images, rects, targets = synthetic_batch(B=B, H=H, W=W, Ts=Ts, seed=seed)
    return images.to(DEV), rects.to(DEV), [{k: v.to(DEV) for k, v in t.items()} for t in targets]


@pytest.mark.parametrize("layout", ["chain", "single"])
def test_graph_step_equals_train_step(layout, monkeypatch):
    """Trainer.step (captured, cached graph) == Trainer.train_step from the same state on the same batch; then a second step of each, and
    adapt_pos1d untouched by both."""
    from counting_detr_amd.engine import Trainer
    monkeypatch.setenv("CDETR_GRAPH_LAYOUT", layout)
    batches = [_batch(0), _batch(1)]
    res, flat = [], []
    for use_graph in (False, True):
        model, crit, args = build(num_query_position=100)
        model.train()
        tr = Trainer(model, crit, args, device=DEV)
        p1d = {n: p.detach().clone() for n, p in model.named_parameters() if "adapt_pos1d" in n}
        outs = []
        for b in batches:
            o = tr.step(*b) if use_graph else tr.train_step(*b)
            outs.append({k: float(v) for k, v in o.items()})
        torch.cuda.synchronize()
        if use_graph:
            assert tr.cache_stats["captures"] == 1
        for n, p in model.named_parameters():
            if n in p1d:
                assert torch.equal(p.detach(), p1d[n]), n
        res.append(outs)
        flat.append(tr.flat_p.detach().clone())
    for a, b in zip(res[0], res[1]):
        for k in a:
            np.testing.assert_allclose(b[k], a[k], rtol=1e-4, atol=1e-6, err_msg=k)
    diff = (flat[0] - flat[1]).abs()          # atomic-order rounding of near-zero gradients: see test_model_gpu.py
    assert float(diff.max()) <= 4.1e-4 and float((diff > 2e-6).float().mean()) < 2e-3


def test_checkpoint_resume_optimizer_roundtrip():
    """Trainer.state_dict carries no optimizer state for adapt_pos1d; load_state_dict restores the moments and the next step matches."""
    from counting_detr_amd.engine import Trainer
    model, crit, args = build(num_query_position=100)
    tr = Trainer(model, crit, args, device=DEV)
    tr.train_step(*_batch(0))
    sd = tr.state_dict()
    order = [n for grp in tr._torch_param_order()[0] for n in grp]       # the state's indices: torch AdamW's parameter numbering
    assert {order[i] for i in sd["state"]} == set(tr.names)
    assert not any(order[i].startswith("transformer.adapt_pos1d.") for i in sd["state"])
    model2, crit2, _ = build(num_query_position=100)
    model2.load_state_dict(model.state_dict(), strict=True)
    tr2 = Trainer(model2, crit2, args, device=DEV)
    tr2.load_state_dict(sd)
    a = tr.train_step(*_batch(1))
    b = tr2.train_step(*_batch(1))
    for k in a:
        np.testing.assert_allclose(float(b[k]), float(a[k]), rtol=1e-5, atol=1e-7, err_msg=k)


def test_inference_engine_counts_equal_the_eager_rule():
    from counting_detr_amd.engine import InferenceEngine, count_objects
    model, _, _ = build(num_query_position=100)
    eng = InferenceEngine(model)
    for i, (H, W) in enumerate([(96, 128), (64, 96), (96, 128)]):
        images, rects, _ = _batch(40 + i, H=H, W=W, Ts=(1, 1))
        counts, keep, out, ref, prob = eng(images, rects)
        c0, k0, o0, r0 = count_objects(model, images, rects)
        assert torch.equal(counts, c0) and torch.equal(keep, k0)
        # the engine's forward GEMMs read pre-split weight images: rounding-level differences (measured 1.7e-5 on the logits at 96x128),
        # a decade above the RCDA engine's because six full self-attentions over every position compound them
        for k in ("pred_logits", "pred_boxes", "pred_vars"):
            np.testing.assert_allclose(out[k].cpu().numpy(), o0[k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    assert eng.stats["captures"] == 2 and eng.stats["calls"] == 3


def test_main_then_infer_cli(tmp_path):
    """main.py --synthetic --attention_type nn.MultiheadAttention trains one epoch and writes a checkpoint; infer.py runs the tiny FSC-147
    fixture from it.  Both in child processes under a time limit."""
    out = tmp_path / "run"
    common = ["--attention_type", "nn.MultiheadAttention", "--num_query_position", "100", "--device", DEV]
    subprocess.run([sys.executable, "main.py", "--synthetic", "--epochs", "1", "--steps_per_epoch", "2", "--images_per_gpu", "2",
                    "--synthetic_size", "128", "160", "-o", str(out)] + common, cwd=ROOT, check=True, timeout=600)
    ck = out / "detr_retrain.pth"
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["model"]["transformer.encoder_layers.0.self_attn.in_proj_weight"].shape == (768, 256)
    subprocess.run([sys.executable, "infer.py", "-dp", os.path.join(ROOT, "tests", "golden", "fsc147_tiny"), "--split", "val",
                    "--resume", str(ck), "-o", str(tmp_path / "inf")] + common, cwd=ROOT, check=True, timeout=600)
    assert (tmp_path / "inf" / "predictions_val.json").is_file()
