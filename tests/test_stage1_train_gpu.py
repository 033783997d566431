"""engine.Stage1Trainer (the 1st-stage step: fused BoundingBoxCriterion, flat clip + AdamW, graph-cached replay) and main_stage1.py:
  (a) three eager steps against the REAL reference's A1 optimizer run (tests/golden/g12_stage1_train.npz, tools/gen_golden_stage1_train.py);
  (b) graph-cached steps == stream-ordered steps from the same weights on the same batches (incl. a batch the graph was not captured with);
  (c) one capture per (image shape, points shape), replays after that;
  (d) what the optimizer must not touch (cls_embed, frozen stem / layer1, FrozenBN buffers) stays bit-identical;
  (e) / (f) main_stage1.py end to end in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TINY = os.path.join(HERE, "golden", "fsc147_tiny")


@pytest.fixture(params=[0, 1], ids=["fp32mfma", "bf16x3"])
def precision(request):
    from counting_detr_amd import ops
    old = ops.PRECISION
    ops.PRECISION = request.param
    yield request.param
    ops.PRECISION = old


def build(seed_weights=True, **kw):
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    from oracle.weights import seeded_state_dict, stage1_schema
    args = get_args_parser_stage1().parse_args([])
    args.device = DEV
    for k, v in kw.items():
        setattr(args, k, v)
    model, crit, _ = stage1.build(args)
    if seed_weights:
        model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True)
    model.to(DEV).train()
    return args, model, crit


def golden_batch(H, W, seed, npts=3):
    # the generator's batch rule (tools/gen_golden_stage1_train.batch), restated: the test must not import the generator's reference setup
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(1, 3, H, W, generator=g)
    pts = torch.rand(1, npts, 2, generator=g) * 0.6 + 0.2
    whs = torch.rand(1, npts, 2, generator=g) * 0.15 + 0.03
    return img.to(DEV), pts.to(DEV), whs.to(DEV)


def rand_batch(B, H, W, seed, npts=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, H, W, generator=g).to(DEV), (torch.rand(B, npts, 2, generator=g) * 0.6 + 0.2).to(DEV),
            (torch.rand(B, npts, 2, generator=g) * 0.15 + 0.03).to(DEV))


def test_eager_steps_match_reference_training(golden, precision):
    from counting_detr_amd.engine import Stage1Trainer
    z = golden("g12_stage1_train.npz")
    args, model, crit = build()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    assert crit.fused
    names = [str(n) for n in z["param_names"]]
    params = dict(model.named_parameters())
    for s, (H, W, seed) in enumerate(z["steps"].tolist()):
        img, pts, whs = golden_batch(H, W, seed)
        res = tr.train_step(img, pts, whs)
        # step 1 at the bars of stage 2's full-size tests; steps 2 and 3 start from weights that one / two AdamW updates moved: an update
        # is ~lr * sign(g) per element, so an element whose gradient is near zero can take the opposite sign under the bf16 backward and
        # move 2 lr away from the reference's -- measured 1.8e-3 on step 3's loss_wh (bf16x3 forward).  Those steps get 5x the bars.
        f = 1 if s == 0 else 5
        for k in ("loss_wh", "loss_giou"):
            np.testing.assert_allclose(float(res[k]), float(z[f"s{s}/{k}"]), rtol=1e-3 * f, atol=1e-5, err_msg=f"step {s} {k}")
        np.testing.assert_allclose(float(res["loss"]), float(z[f"s{s}/loss_total"]), rtol=1e-3 * f, err_msg=f"step {s} total")
        np.testing.assert_allclose(float(res["grad_norm"]), float(z[f"s{s}/grad_total_norm"]), rtol=2e-3 * f, err_msg=f"step {s} clip norm")
        if s == 0:
            tot = float(z["s0/grad_total_norm"])
            for n, r in zip(names, z["grad_norms"]):
                if r < 0:                                              # no gradient in the reference: none here either
                    assert params[n].grad is None or not params[n].requires_grad, n
                    continue
                np.testing.assert_allclose(params[n].grad.norm().item(), r, rtol=1e-2, atol=1e-6 * tot, err_msg=n)
    # post-AdamW: the sampled elements (largest movement in the reference).  Tight bar: within 3e-2 of their movement or -- stage 2's element
    # bar (tests/fullsize.check_param_samples: 0.05 lr per AdamW update) -- within 0.05 lr per step taken.  Each update moves an element by
    # ~lr * m / sqrt(v); where an element's gradient changes sign between steps that ratio is sensitive to the gradient's last digits, and
    # the bf16 backward's (plus the bf16x3 forward's, run to run) differ.  Measured: 0.011 lr worst over all 3844 elements with the fp32
    # forward; with the bf16x3 forward single elements 0.10 / 0.39 / 2.0 lr off in three runs (the last: one of three updates of a
    # LayerNorm weight whose gradient sits near zero took the other sign), 98.4 % of the elements within the tight bar.  So: fp32
    # forward -- every element within the tight bar; bf16x3 forward -- 97 % of them.
    pidx, fidx = z["sample_pidx"], z["sample_fidx"]
    before, after = z["sample_before"].astype(np.float64), z["sample_after"].astype(np.float64)
    tight, worst = 0, 0.0
    for k in range(len(pidx)):
        n = names[int(pidx[k])]
        lr = args.lr_backbone if "backbone" in n else args.lr
        v = float(params[n].detach().reshape(-1)[int(fidx[k])])
        d_ref, d = after[k] - before[k], v - before[k]
        err_lr = abs(d - d_ref) / lr
        worst = max(worst, err_lr)
        ok = abs(d - d_ref) <= 3e-2 * abs(d_ref) or err_lr <= 0.05 * len(z["steps"])
        assert ok or precision != 0, f"{n}[{int(fidx[k])}]: moved {d:.4e}, reference {d_ref:.4e}"
        tight += int(ok)
    print(f"post-AdamW: worst movement error {worst:.3f} lr, {tight} / {len(pidx)} elements within the tight bar")
    assert tight >= (1.0 if precision == 0 else 0.97) * len(pidx)


def _arena_state(tr):
    return [t.detach().cpu().clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state)]


def test_graph_steps_equal_stream_ordered_steps():
    """Stage1Trainer.step (graph cache) vs train_step (stream-ordered) from the SAME weights / moments on the same batches (as stage 2's
    test_cached_graph_steps_equal_eager_steps_on_varied_batches): losses and clip norm at rtol 1e-4 /
    atol 1e-6, every parameter's raw gradient to 1e-2 of its norm (the per-parameter bar of the reference comparisons: the captured step
    runs the weight gradients in other slices beside the data-gradient chain, so their fp32 sums of bf16 products round differently --
    measured 1.1e-3 on layer3.0.conv1.weight), updated parameters to the atomic-order noise of one AdamW step.  Batch 41 replays the graph captured on
    batch 40; 42 is another image size (its own capture); 43 replays the first graph again."""
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = build()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    params = dict(model.named_parameters())
    state = lambda: [t.detach().clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state)]      # noqa: E731
    for i, (B, H, W) in enumerate([(2, 384, 576), (2, 384, 576), (2, 384, 512), (2, 384, 576)]):
        img, pts, whs = rand_batch(B, H, W, 40 + i)
        saved = state()
        eo = {k: float(v) for k, v in tr.train_step(img, pts, whs).items()}
        g_eager = {n: params[n].grad.detach().clone() for n in tr.names}
        p_eager = tr.flat_p.detach().clone()
        for dst, src in zip((tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state), saved):
            dst.copy_(src)
        go = {k: float(v) for k, v in tr.step(img, pts, whs).items()}
        torch.cuda.synchronize()
        assert set(go) == set(eo) == {"loss_wh", "loss_giou", "loss", "grad_norm"}
        for k in eo:
            np.testing.assert_allclose(go[k], eo[k], rtol=1e-4, atol=1e-6, err_msg=f"step {i} {k}")
        tn = eo["grad_norm"]
        for n in tr.names:
            ge, gg = g_eager[n], params[n].grad
            err = float((gg - ge).norm())
            assert err <= 1e-2 * float(ge.norm()) + 1e-6 * tn, f"step {i} {n}: gradient differs by {err:.3e} (norm {float(ge.norm()):.3e})"
        diff = (tr.flat_p - p_eager).abs()
        assert float(diff.max()) <= 2.1e-4 and float((diff > 2e-6).float().mean()) < 2e-3, f"step {i}"
    assert tr.cache_stats == {"captures": 2, "steps": 4}
    assert sorted(e["replays"] for e in tr._cache.values()) == [1, 3]


def test_two_image_sizes_two_captures_then_replays():
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = build()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    for i, (H, W) in enumerate([(384, 576), (384, 512), (384, 576), (384, 512), (384, 576)]):
        tr.step(*rand_batch(1, H, W, 60 + i))
    assert tr.cache_stats == {"captures": 2, "steps": 5}
    tr.step(*rand_batch(1, 384, 576, 70, npts=4))                     # another points shape: its own capture
    assert tr.cache_stats == {"captures": 3, "steps": 6}
    assert tr.nonfinite_steps() == 0


def test_untrained_parameters_and_buffers_stay_bit_identical():
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = build()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    frozen = {n: p.detach().clone() for n, p in model.named_parameters()
              if n.startswith("transformer.cls_embed.") or n.startswith("backbone.body.conv1.") or n.startswith("backbone.body.layer1.")}
    assert any(n.startswith("transformer.cls_embed.") for n in frozen) and not any(n.startswith("transformer.cls_embed.") for n in tr.names)
    bufs = {n: b.detach().clone() for n, b in model.named_buffers()}
    trained = {n: p.detach().clone() for n, p in model.named_parameters() if n in tr.offsets}
    for i in range(3):
        tr.step(*rand_batch(1, 384, 512, 80 + i))
    tr.train_step(*rand_batch(1, 384, 512, 90))
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    for n, v in frozen.items():
        assert torch.equal(params[n].detach(), v), n
    for n, b in model.named_buffers():
        assert torch.equal(b.detach(), bufs[n]), n
    assert all(not torch.equal(params[n].detach(), v) for n, v in trained.items() if "layer4.2.conv3" in n or "bbox_embed" in n)
    # the optimizer's checkpoint entry: cls_embed is in the reference's parameter groups but has no state (no gradient ever)
    sd = tr.state_dict()
    groups, _ = tr._torch_param_order()
    order = [n for g in groups for n in g]
    idx = {n: i for i, n in enumerate(order)}
    assert idx["transformer.cls_embed.0.weight"] not in sd["state"] and idx["input_proj.0.0.weight"] in sd["state"]
    args2, model2, crit2 = build()
    tr2 = Stage1Trainer(model2, crit2, args2, device=DEV)
    tr2.load_state_dict(sd, tr.lr_scheduler_state_dict())
    assert torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq)
    assert float(tr2.opt_state[0]) == float(tr.opt_state[0]) == 4.0


def test_out_of_scope_configurations_raise():
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = build(sgd=True)
    with pytest.raises(NotImplementedError, match="sgd"):
        Stage1Trainer(model, crit, args, device=DEV)
    args, model, crit = build(seed_weights=False, num_query_pattern=3)
    with pytest.raises(ValueError, match="num_query_pattern"):
        Stage1Trainer(model, crit, args, device=DEV)


def _run(argv, timeout=900):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "main_stage1.py")] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_main_stage1_on_the_tiny_dataset(tmp_path):
    from counting_detr_amd import data
    from oracle.weights import seeded_state_dict, stage1_schema
    out = tmp_path / "out"
    out.mkdir()
    init = tmp_path / "init.pth"
    sd = seeded_state_dict(stage1_schema())
    sd["transformer.pattern.weight"] = torch.zeros(3, 256)            # a COCO Anchor-DETR key: filtered by --resume, as in A1
    torch.save({"model": sd}, init)
    common = ["--data_path", TINY, "--output_dir", str(out), "--num_workers", "0", "--print_freq", "1"]
    _run(common + ["--epochs", "1", "--resume", str(init)])
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "epoch", "args"} and ck["epoch"] == 0
    args, model, _ = build(seed_weights=False)
    model.load_state_dict(ck["model"], strict=True)
    log = [json.loads(line) for line in (out / "log.txt").read_text().splitlines()]
    assert len(log) == 1 and log[0]["epoch"] == 0 and np.isfinite(log[0]["train_loss"])
    txt = _run(common + ["--epochs", "2", "--auto_resume"])
    assert "continuing at epoch 1" in txt
    ck2 = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 1 and len((out / "log.txt").read_text().splitlines()) == 2
    txt = _run(common + ["--eval", "--resume", str(out / "checkpoint.pth")])
    val = json.loads(txt.split("validation:", 1)[1].strip().splitlines()[0])
    assert np.isfinite(val["loss"]) and val["batches"] == 2
    _run(common + ["--dataset_file", "fscd_147_point", "--generate_pseudo_label", "--resume", str(out / "checkpoint.pth")])
    for split in ("train", "val", "test"):
        assert (out / f"pseudo_bbox_{split}.json").is_file()
    # the hand-off: the 2nd stage's training reader opens the written labels (one box per annotated dot)
    root = tmp_path / "ds"
    (root / "annotations").mkdir(parents=True)
    (root / "annotations" / "pseudo_bbox_train.json").write_bytes((out / "pseudo_bbox_train.json").read_bytes())
    (root / "annotation_FSC147_384.json").write_bytes(open(os.path.join(TINY, "annotation_FSC147_384.json"), "rb").read())
    import argparse
    ds = data.FSC147Dataset(argparse.Namespace(data_path=str(root)))
    pts = data.FSC147PointsDataset(argparse.Namespace(data_path=TINY, scale_factor=32), "train")
    assert len(ds) == len(pts) == 2
    n_boxes = sum(len(ds.coco.getAnnIds([i])) for i in ds.images)
    assert n_boxes == sum(len(pts[i]["points"]) for i in range(len(pts)))
    assert [ds.coco.loadImgs([i])[0]["file_name"] for i in ds.images] == ["1.jpg", "2.jpg"]


def test_main_stage1_synthetic(tmp_path):
    txt = _run(["--synthetic", "--epochs", "1", "--steps_per_epoch", "4", "--print_freq", "2", "--output_dir", str(tmp_path)])
    log = json.loads((tmp_path / "log.txt").read_text().splitlines()[-1])
    for k in ("train_loss", "train_loss_wh", "train_loss_giou", "train_grad_norm"):
        assert np.isfinite(log[k]), (k, txt[-2000:])
    assert log["train_graph_steps"] == 4 and log["train_graph_captures"] == 1
