"""Stage 1 on batches whose images hold different numbers of points (`counts`), end to end:
  (a) AnchorDETRStage1(samples, points, counts) + BoundingBoxCriterion with counts against the CPU oracle run one image at a time on
      the image's own points: outputs of the valid rows, losses, per-parameter gradient norms;
  (b) Stage1Trainer.step(..., counts=) == train_step(..., counts=); two batches of one padded shape and different counts replay ONE
      captured graph, a dense batch takes its own;
  (c) stage1.write_pseudo_labels on a two-image batch == the two batch-1 files;
  (d) main_stage1.py --ragged_batches in a fresh child process: an epoch and the pseudo-label hand-off.
Needs an MI355X."""
import argparse
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
COUNTS = (3, 1, 5)


@pytest.fixture(params=[0, 1], ids=["fp32mfma", "bf16x3"])
def precision(request):
    from counting_detr_amd import ops
    old = ops.PRECISION
    ops.PRECISION = request.param
    yield request.param
    ops.PRECISION = old


def build(**kw):
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    from oracle.weights import seeded_state_dict, stage1_schema
    args = get_args_parser_stage1().parse_args([])
    args.device = DEV
    for k, v in kw.items():
        setattr(args, k, v)
    model, crit, _ = stage1.build(args)
    model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True)
    model.to(DEV).train()
    return args, model, crit


def ragged_batch(counts, H=64, W=96, seed=0):
    """(images [B,3,H,W], points / whs [B,N,2] padded with (0.5, 0.5) / 0, counts) on the host."""
    g = torch.Generator().manual_seed(seed)
    B, N = len(counts), max(counts)
    img = torch.randn(B, 3, H, W, generator=g)
    pts = torch.rand(B, N, 2, generator=g) * 0.6 + 0.2
    whs = torch.rand(B, N, 2, generator=g) * 0.15 + 0.03
    for b, c in enumerate(counts):
        pts[b, c:], whs[b, c:] = 0.5, 0.0
    return img, pts, whs, torch.tensor(counts, dtype=torch.int32)


@pytest.fixture(scope="module")
def oracle_run():
    """The CPU oracle, one image at a time on the image's own points, with autograd through its state dict: outputs per image, the
    losses over the concatenated pairs and every parameter's gradient norm.  Computed once for both arithmetic modes."""
    from counting_detr_amd import stage1
    from oracle.model import forward_stage1
    from oracle.weights import seeded_state_dict, stage1_schema
    img, pts, whs, _ = ragged_batch(COUNTS)
    sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in seeded_state_dict(stage1_schema()).items()}
    outs = [forward_stage1(img[b:b + 1], pts[b, :c], sd) for b, c in enumerate(COUNTS)]
    cat = lambda k: torch.cat([o[k] for o in outs], dim=1)      # noqa: E731
    crit = stage1.BoundingBoxCriterion()
    tgt = {"points": torch.cat([pts[b, :c] for b, c in enumerate(COUNTS)])[None], "whs": torch.cat([whs[b, :c] for b, c in enumerate(COUNTS)])[None]}
    ld, total = crit.forward_with_total({"pred_wh": cat("pred_wh")}, tgt)
    total.backward()
    norms = {k: float(v.grad.norm()) for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    return ([{k: v.detach().numpy() for k, v in o.items()} for o in outs], {k: float(v.detach()) for k, v in ld.items()}, norms)


def test_ragged_model_vs_cpu_oracle(oracle_run, precision):
    outs, losses, norms = oracle_run
    args, model, crit = build()
    img, pts, whs, counts = (t.to(DEV) for t in ragged_batch(COUNTS))
    out = model(img, pts, counts)
    for k in ("pred_logits", "pred_wh", "pred_points", "pred_boxes"):
        assert torch.isfinite(out[k]).all(), k                    # padded rows: don't-care values, but finite
    for b, c in enumerate(COUNTS):
        for k in ("pred_logits", "pred_wh", "pred_points"):
            np.testing.assert_allclose(out[k][b, :c].detach().cpu().numpy(), outs[b][k][0], rtol=1e-3, atol=1e-4, err_msg=f"image {b} {k}")
    tgt = {"points": pts, "whs": whs, "counts": counts}
    got = crit(out, tgt)                                          # the composition restricted to the valid pairs
    crit.fused = True
    fused, total = crit.forward_with_total(out, tgt)
    for k in ("loss_wh", "loss_giou"):
        print(k, float(got[k].detach()), float(fused[k].detach()), losses[k])
        np.testing.assert_allclose(float(got[k].detach()), losses[k], rtol=1e-3, err_msg=k)
        np.testing.assert_allclose(float(fused[k].detach()), losses[k], rtol=1e-3, err_msg=k + " (fused)")
    total.backward()
    tot = float(np.sqrt(sum(v * v for v in norms.values())))
    checked = 0
    for n, p in model.named_parameters():
        if n in norms and p.requires_grad:                        # (the oracle has no gradient for cls_embed; the frozen stem has none here)
            assert p.grad is not None, n
            np.testing.assert_allclose(p.grad.norm().item(), norms[n], rtol=1e-2, atol=1e-6 * tot, err_msg=n)
            checked += 1
    assert checked > 100, checked


def test_counts_need_one_pattern_and_defined_points():
    args, model, _ = build()
    img, pts, _, counts = (t.to(DEV) for t in ragged_batch(COUNTS))
    model.transformer.num_pattern = 3
    with pytest.raises(ValueError, match="num_query_pattern"):
        model(img, pts, counts)
    model.transformer.num_pattern = 1
    with pytest.raises(ValueError, match="int32"):
        model(img, pts, counts.long())


def _state(tr):
    return [t.detach().clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state)]


def test_ragged_graph_steps_equal_stream_ordered_steps_and_share_one_capture():
    from counting_detr_amd.engine import Stage1Trainer
    args, model, crit = build()
    tr = Stage1Trainer(model, crit, args, device=DEV)
    params = dict(model.named_parameters())
    for i, counts in enumerate([(3, 1, 5), (5, 5, 2)]):
        img, pts, whs, cn = (t.to(DEV) for t in ragged_batch(counts, seed=40 + i))
        saved = _state(tr)
        eo = {k: float(v) for k, v in tr.train_step(img, pts, whs, counts=cn).items()}
        g_eager = {n: params[n].grad.detach().clone() for n in tr.names}
        p_eager = tr.flat_p.detach().clone()
        for dst, src in zip((tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state), saved):
            dst.copy_(src)
        go = {k: float(v) for k, v in tr.step(img, pts, whs, counts=cn).items()}
        torch.cuda.synchronize()
        print(counts, eo, go)
        assert set(go) == set(eo) == {"loss_wh", "loss_giou", "loss", "grad_norm"}
        for k in eo:                                              # (the second batch REPLAYS the first one's graph: its losses are its own counts')
            np.testing.assert_allclose(go[k], eo[k], rtol=1e-4, atol=1e-6, err_msg=f"step {i} {k}")
        tn = eo["grad_norm"]
        for n in tr.names:
            ge, gg = g_eager[n], params[n].grad
            err = float((gg - ge).norm())
            assert err <= 1e-2 * float(ge.norm()) + 1e-6 * tn, f"step {i} {n}: gradient differs by {err:.3e} (norm {float(ge.norm()):.3e})"
        diff = (tr.flat_p - p_eager).abs()
        assert float(diff.max()) <= 2.1e-4 and float((diff > 2e-6).float().mean()) < 2e-3, f"step {i}"
        assert tr.cache_stats == {"captures": 1, "steps": i + 1}
    # the counts matter: the same padded tensors under other counts give another loss
    img, pts, whs, cn = (t.to(DEV) for t in ragged_batch((5, 5, 2), seed=41))
    saved = _state(tr)
    a = float(tr.step(img, pts, whs, counts=cn)["loss"])
    for dst, src in zip((tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state), saved):
        dst.copy_(src)
    b = float(tr.step(img, pts, whs, counts=torch.tensor((5, 1, 2), dtype=torch.int32, device=DEV))["loss"])
    assert a != b and tr.cache_stats["captures"] == 1
    # a dense batch of the same shapes: its own capture
    img, pts, whs, _ = (t.to(DEV) for t in ragged_batch((5, 5, 5), seed=43))
    out = tr.step(img, pts, whs)
    assert np.isfinite(float(out["loss"])) and tr.cache_stats["captures"] == 2
    # all counts == N through the ragged graph: today's dense batch
    for dst, src in zip((tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state), saved):
        dst.copy_(src)
    d = float(tr.step(img, pts, whs)["loss"])
    for dst, src in zip((tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.opt_state), saved):
        dst.copy_(src)
    r = float(tr.step(img, pts, whs, counts=torch.full((3,), 5, dtype=torch.int32, device=DEV))["loss"])
    np.testing.assert_allclose(r, d, rtol=1e-6)
    assert tr.cache_stats["captures"] == 2 and tr.nonfinite_steps() == 0
    with pytest.raises(ValueError, match="counts"):
        tr.train_step(img, pts, whs, counts=torch.ones(2, dtype=torch.int32))


def test_write_pseudo_labels_batched_equals_batch_one(tmp_path):
    from counting_detr_amd import stage1
    _, model, _ = build()
    g = torch.Generator().manual_seed(5)
    imgs = torch.randn(2, 3, 64, 96, generator=g)
    pts = [torch.rand(6, 2, generator=g) * 0.8 + 0.1, torch.rand(7, 2, generator=g) * 0.8 + 0.1]
    sizes, ids = [(384, 256), (480, 320)], [11, 12]
    padded = torch.full((2, 7, 2), 0.5)
    padded[0, :6], padded[1] = pts[0], pts[1]
    batched = [{"image": imgs, "points": padded, "counts": torch.tensor([6, 7], dtype=torch.int32),
                "orig_size": torch.tensor(sizes), "im_id": torch.tensor(ids)}]
    single = [{"image": imgs[b:b + 1], "points": pts[b][None], "orig_size": torch.tensor([sizes[b]]), "im_id": torch.tensor([ids[b]])}
              for b in range(2)]
    a = stage1.write_pseudo_labels(model, batched, "train", str(tmp_path / "batched"), device=DEV)
    b = stage1.write_pseudo_labels(model, single, "train", str(tmp_path / "single"), device=DEV)
    assert json.load(open(tmp_path / "batched" / "pseudo_bbox_train.json")) == a
    assert a["images"] == b["images"] and a["categories"] == b["categories"]
    assert [x["id"] for x in a["images"]] == [1, 2] and [x["file_name"] for x in a["images"]] == ["11.jpg", "12.jpg"]
    assert len(a["annotations"]) == len(b["annotations"]) == 13
    worst = 0
    for x, y in zip(a["annotations"], b["annotations"]):
        assert (x["id"], x["image_id"], x["category_id"], x["iscrowd"]) == (y["id"], y["image_id"], y["category_id"], y["iscrowd"])
        assert x["bbox"][:2] == y["bbox"][:2]                         # the given points
        worst = max([worst] + [abs(p - q) for p, q in zip(x["bbox"][2:], y["bbox"][2:])])
        # int() may flip on arithmetic noise: every integer within 1 of the batch-1 value
        assert all(abs(p - q) <= 1 for p, q in zip(x["bbox"], y["bbox"])), (x, y)
        assert abs(x["area"] - y["area"]) <= 1, (x, y)
    print("largest w / h difference (pixels):", worst)
    assert [x["image_id"] for x in a["annotations"]] == [1] * 6 + [2] * 7


def _run(argv, timeout=900):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "main_stage1.py")] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_main_stage1_ragged_batches_on_the_tiny_dataset(tmp_path):
    from counting_detr_amd import data
    from oracle.weights import seeded_state_dict, stage1_schema
    out = tmp_path / "out"
    out.mkdir()
    init = tmp_path / "init.pth"
    torch.save({"model": seeded_state_dict(stage1_schema())}, init)
    common = ["--data_path", TINY, "--output_dir", str(out), "--num_workers", "0", "--print_freq", "1", "--ragged_batches", "--batch_size", "2"]
    _run(common + ["--epochs", "1", "--resume", str(init)])
    log = [json.loads(line) for line in (out / "log.txt").read_text().splitlines()]
    assert len(log) == 1 and np.isfinite(log[0]["train_loss"]) and log[0]["train_graph_steps"] == 1
    _run(common + ["--dataset_file", "fscd_147_point", "--generate_pseudo_label", "--resume", str(out / "checkpoint.pth")])
    for split in ("train", "val", "test"):
        assert (out / f"pseudo_bbox_{split}.json").is_file()
    root = tmp_path / "ds"
    (root / "annotations").mkdir(parents=True)
    (root / "annotations" / "pseudo_bbox_train.json").write_bytes((out / "pseudo_bbox_train.json").read_bytes())
    (root / "annotation_FSC147_384.json").write_bytes(open(os.path.join(TINY, "annotation_FSC147_384.json"), "rb").read())
    ds = data.FSC147Dataset(argparse.Namespace(data_path=str(root)))
    pts = data.FSC147PointsDataset(argparse.Namespace(data_path=TINY, scale_factor=32), "train")
    assert len(ds) == len(pts) == 2
    n_boxes = sum(len(ds.coco.getAnnIds([i])) for i in ds.images)
    assert n_boxes == sum(len(pts[i]["points"]) for i in range(len(pts)))
    assert sorted(ds.coco.loadImgs([i])[0]["file_name"] for i in ds.images) == ["1.jpg", "2.jpg"]
