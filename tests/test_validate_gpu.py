"""Validation inside a training run on the tree of tests/validate_tree.py (four training images of two sizes, the five-image val split):
main.py / main_stage1.py --eval_every, --keep_best and engine.InferenceEngine(trainer=...), the engine that rides on a trainer's weight images.

  1  the in-training pass on the live weights gives the numbers and the predictions file of infer.py on the checkpoint written at that epoch:
     EQUAL, no tolerance (the same fp32 weights, the same image-refresh kernel, the same forward kernels) -- a pass on weight images one
     optimizer step old cannot, an AdamW step moves every output float;
  2  nothing is invalidated: the epoch after a pass captures no step graph, a second pass captures no forward graph -- and a plain
     InferenceEngine(model) beside a warmed trainer DOES clear the trainer's cache, which is why the riding form exists;
  3  the riding engine after sync() == a fresh engine on a copy of the weights, bit for bit; without sync() it is not; a rebuilt trainer mirror
     makes it drop its graphs and still agree;
  4  detr_retrain_best.pth is the epoch of the lowest logged test_loss, --auto_resume carries the best-so-far across the restart;
  5  the same for main_stage1.py (validation loss == --eval --resume on the checkpoint);
  6  without the flags: today's log keys, today's checkpoint keys, no *_best.pth.
A seeded network gives an image's queries nearly equal logits, so counts and AP are degenerate on this tree: the tests assert equality, not
quality.  `test_loss` is not a number infer.py prints: it is the criterion's weighted total of the pass's mean losses
(checkpoint.weighted_loss), compared with the same sum over infer.py's numbers.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import validate_tree as vt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
LOSS_KEYS = ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "loss_variance")
# --seed 2: the training loader's shuffle (seeded by --seed, batches of two) pairs images of ONE size in each of the first three epochs, with
# and without a validation pass between them (an evaluation loader's iterator draws from the same generator): both sizes meet in epoch 0
SEED = "2"


def _eq(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def _lines(path):
    return [json.loads(l) for l in open(path).read().strip().splitlines()]


def _argmin_first(vals):
    best = None
    for i, v in enumerate(vals):
        if v == v and (best is None or v < vals[best]):
            best = i
    return best


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return vt.write_tree(tmp_path_factory.mktemp("validate") / "ds")


def _stage2_argv(tree, out, *extra):
    return ["-dp", tree, "-o", str(out), "--images_per_gpu", "2", "--device", DEV, "--seed", SEED, *vt.MODEL_FLAGS, *extra]


@pytest.fixture(scope="module")
def run2(tree, tmp_path_factory):
    """main.py for two epochs with a pass after each, then infer.py on the checkpoint it left; everything the tests read, read NOW (item 4
    continues the run in the same directory)."""
    import infer as infer_mod
    import main as main_mod
    from counting_detr_amd.args import get_args_parser
    out = tmp_path_factory.mktemp("run2")
    val_flags = ["--device_detections", "--eval_batch_size", "2"]
    main_mod.main(get_args_parser().parse_args(_stage2_argv(tree, out, "--epochs", "2", "--eval_every", "1", "--keep_best", "loss", *val_flags)))
    lines = _lines(out / "detr_retrain.txt")
    pred_train = open(out / "predictions_val.json", "rb").read()
    last = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    best = torch.load(out / "detr_retrain_best.pth", map_location="cpu", weights_only=False)
    out_i = tmp_path_factory.mktemp("run2_infer")
    infer_mod.main(get_args_parser().parse_args(["-dp", tree, "-o", str(out_i), "--split", "val", "--resume", str(out / "detr_retrain.pth"), "--device", DEV,
                                                 *vt.MODEL_FLAGS, *val_flags]))
    metrics = json.loads(open(out_i / "results_val.txt").read())
    return {"out": out, "lines": lines, "pred_train": pred_train, "pred_infer": open(out_i / "predictions_val.json", "rb").read(), "infer": metrics,
            "last": last, "best": best, "best_mtime": os.stat(out / "detr_retrain_best.pth").st_mtime_ns}


# ---------------------------------------------------------------------------------------------------------------- 1, 2a
def test_live_weights_give_the_numbers_of_infer_on_the_checkpoint(run2):
    from counting_detr_amd import checkpoint as ck
    lines, m = run2["lines"], run2["infer"]
    assert [l["epoch"] for l in lines] == [0, 1]
    test = {k[len("test_"):]: v for k, v in lines[1].items() if k.startswith("test_")}
    print("in training", test)
    print("infer.py   ", m)
    assert set(test) == set(m) | {"loss"} and all(k in m for k in LOSS_KEYS + AP_KEYS + ("MAE", "RMSE", "NAE", "SRE", "images")) and m["images"] == 5
    for k, v in m.items():
        assert _eq(test[k], v), (k, test[k], v)
    weights = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_variance": 2.0}      # the parser's defaults (--no_aux_loss)
    assert _eq(test["loss"], ck.weighted_loss(m, weights)) and np.isfinite(test["loss"])
    assert run2["pred_train"] == run2["pred_infer"] and len(json.loads(run2["pred_train"])["images"]) == 5
    # the order of the line: train_*, test_*, epoch
    kinds = [k.split("_")[0] for k in lines[1]]
    n_train, n_test = kinds.count("train"), kinds.count("test")
    assert kinds == ["train"] * n_train + ["test"] * n_test + ["epoch"] and n_test == len(m) + 1
    # epoch 0 validated other weights: its pass differs (an optimizer epoch moves every float of the losses)
    assert lines[0]["test_loss"] != lines[1]["test_loss"] and lines[0]["test_loss_bbox"] != lines[1]["test_loss_bbox"]


def test_the_epoch_after_a_pass_captures_no_step_graph(run2):
    lines = run2["lines"]
    assert lines[0]["train_graph_captures"] == 2 and lines[0]["train_graph_steps"] == 2          # both sizes met (and captured) in epoch 0
    assert lines[1]["train_graph_captures"] == 0 and lines[1]["train_graph_steps"] == 2          # a validation pass ran between the two


# ---------------------------------------------------------------------------------------------------------------- in-process pieces
def _build(tree, out):
    import counting_detr_amd
    from counting_detr_amd.args import get_args_parser
    from counting_detr_amd.init import seeded_init_
    args = get_args_parser().parse_args(_stage2_argv(tree, out, "--device_detections", "--eval_batch_size", "2", "--eval_every", "1"))
    model, crit, _ = counting_detr_amd.build_model(args)
    seeded_init_(model)
    model.to(DEV).train()
    crit.train()
    return model, crit, args


def _batch(B, H, W, Ts, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g).to(DEV)
    rects = torch.tensor([[.10, .10, .20, .20], [.40, .40, .50, .55], [.70, .20, .80, .30]])[None].repeat(B, 1, 1).to(DEV)
    tg = []
    for b in range(B):
        box = torch.cat([torch.rand(Ts[b], 2, generator=g) * 0.8 + 0.1, torch.rand(Ts[b], 2, generator=g) * 0.10 + 0.02], 1)
        tg.append({"boxes": box.to(DEV), "labels": torch.zeros(Ts[b], dtype=torch.int64, device=DEV)})
    return images, rects, tg


def test_a_second_pass_captures_nothing_and_the_trainer_keeps_its_graphs(tree, tmp_path):
    import main as main_mod
    from counting_detr_amd.engine import InferenceEngine, Trainer
    model, crit, args = _build(tree, tmp_path)
    os.makedirs(args.output_dir, exist_ok=True)
    tr = Trainer(model, crit, args, device=DEV)
    batch = _batch(2, 64, 96, (5, 8), seed=1)
    tr.step(*batch)
    entries = [id(e) for e in tr._cache.values()]
    mirror = tr.mirror
    val = main_mod.Validator(tr, crit, args, torch.device(DEV))
    m1 = val.run(write_json=False)
    first = dict(val.engine.stats)
    assert first["captures"] == 3 and model.training and crit.training               # eval_split.BATCHES_AT_2: [2, 96x64] [1, 96x64] [2, 64x96]
    tr.step(*batch)
    m2 = val.run(write_json=False)
    assert val.engine.stats["captures"] == first["captures"] and val.engine.stats["calls"] == 2 * first["calls"] == 6
    assert m1["images"] == m2["images"] == 5 and m1["loss_bbox"] != m2["loss_bbox"]    # the second pass saw the step between the two
    assert not os.path.exists(os.path.join(args.output_dir, "predictions_val.json"))  # write_json=False
    assert tr.cache_stats == {"captures": 1, "steps": 2} and [id(e) for e in tr._cache.values()] == entries and tr.mirror is mirror
    assert val.engine.mirror is mirror
    # the parent's only way to evaluate between two epochs: a plain engine on the model being trained invalidates the folds, and with them
    # the trainer's captured steps and its weight mirror
    InferenceEngine(model)
    assert len(tr._cache) == 0 and tr._mirror_stale
    model.train()
    tr.step(*batch)
    assert tr.cache_stats == {"captures": 2, "steps": 3} and tr.mirror is not mirror


def test_riding_engine_equals_a_fresh_engine_after_sync_and_not_before(tree, tmp_path):
    import counting_detr_amd
    from counting_detr_amd import checkpoint as ck
    from counting_detr_amd.engine import InferenceEngine, Trainer
    model, crit, args = _build(tree, tmp_path)
    tr = Trainer(model, crit, args, device=DEV)
    assert tr._queries() == 100
    batch = _batch(2, 64, 96, (5, 8), seed=2)                          # two 96x64 images
    for _ in range(3):
        tr.step(*batch)
    image, rects, _ = _batch(1, 96, 64, (1,), seed=3)                 # one 64x96 image
    ride = InferenceEngine(model, trainer=tr)
    assert ride.arith[0] == tr.arith[0] and tr.cache_stats == {"captures": 1, "steps": 3} and len(tr._cache) == 1      # building it dropped nothing

    def run(engine):
        counts, keep, out, ref, prob = engine(image, rects)
        return [t.clone() for t in (out["pred_logits"], out["pred_boxes"], counts)]
    model.eval()
    stale = run(ride)                      # the images of the third step's forward: the weights BEFORE its optimizer update
    ride.sync()
    live = run(ride)
    assert ride.stats["captures"] == 1
    fresh_model, _, _ = counting_detr_amd.build_model(args)
    fresh_model.load_state_dict(model.state_dict(), strict=True)
    fresh_model.to(DEV)
    fresh = InferenceEngine(fresh_model)
    want = run(fresh)
    assert len(tr._cache) == 1 and tr.cache_stats["captures"] == 1    # (an engine on ANOTHER model touches nothing here)
    for name, a, b, c in zip(("pred_logits", "pred_boxes", "counts"), live, want, stale):
        assert torch.equal(a, b), name
        if name != "counts":
            assert not torch.equal(c, b), f"{name}: a pass without sync() ran on current weights?"
    # inside a step (the trainer's mirror scope armed) the engine refuses to run
    tr._arm_mirror()
    try:
        with pytest.raises(RuntimeError, match="armed"):
            ride(image, rects)
        with pytest.raises(RuntimeError, match="armed"):
            ride.sync()
    finally:
        tr._disarm_mirror()
    # the trainer rebuilds its mirror: the engine notices the new identity, drops its graphs, captures again and still agrees
    old = tr.mirror
    tr.clear_graph_cache()                 # (the trainer's own graphs go too: they hold the old mirror's addresses)
    ride.sync()
    again = run(ride)
    assert tr.mirror is not old and ride.mirror is tr.mirror and ride.stats["captures"] == 2
    # a real invalidation (what a checkpoint load does) reaches the riding engine through the model's owner list
    ck.invalidate_caches(model)
    assert len(ride._cache) == 0 and tr._mirror_stale
    ride.sync()
    once_more = run(ride)
    assert ride.stats["captures"] == 3
    for name, a, b, c in zip(("pred_logits", "pred_boxes", "counts"), again, once_more, want):
        assert torch.equal(a, c) and torch.equal(b, c), name
    model.train()
    tr.step(*batch)                        # and the trainer goes on (one re-capture after the real invalidation)
    assert tr.cache_stats == {"captures": 2, "steps": 4} and ride.mirror is tr.mirror


# ---------------------------------------------------------------------------------------------------------------- 4
def test_best_checkpoint_and_resume(run2, tree):
    import main as main_mod
    from counting_detr_amd.args import get_args_parser
    lines, out = run2["lines"], run2["out"]
    losses = [l["test_loss"] for l in lines]
    e_best = _argmin_first(losses)
    print("test_loss per epoch", losses)
    assert run2["best"]["epoch"] == e_best
    assert run2["best"]["best"] == {"metric": "loss", "value": losses[e_best], "epoch": e_best}
    assert run2["last"]["epoch"] == 1 and run2["last"]["best"] == run2["best"]["best"]
    assert set(run2["last"]) == {"model", "optimizer", "lr_scheduler", "epoch", "args", "best"}
    # continue to three epochs: the best-so-far comes back from the checkpoint
    main_mod.main(get_args_parser().parse_args(_stage2_argv(tree, out, "--epochs", "3", "--eval_every", "1", "--keep_best", "loss", "--auto_resume",
                                                            "--device_detections", "--eval_batch_size", "2")))
    lines3 = _lines(out / "detr_retrain.txt")
    assert [l["epoch"] for l in lines3] == [0, 1, 2]
    for before, after in zip(lines, lines3):          # the resumed run appended one line
        assert list(before) == list(after) and all(_eq(before[k], after[k]) for k in before)
    losses3 = [l["test_loss"] for l in lines3]
    e3 = _argmin_first(losses3)
    print("test_loss per epoch", losses3)
    best3 = torch.load(out / "detr_retrain_best.pth", map_location="cpu", weights_only=False)
    last3 = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    assert best3["epoch"] == e3 and best3["best"] == last3["best"] == {"metric": "loss", "value": losses3[e3], "epoch": e3} and last3["epoch"] == 2
    if e3 != 2:                            # epoch 2 did not improve: the file was left alone
        assert os.stat(out / "detr_retrain_best.pth").st_mtime_ns == run2["best_mtime"]
    else:
        assert losses3[2] < losses[e_best]


# ---------------------------------------------------------------------------------------------------------------- 5
def test_stage1_validates_between_epochs(tree, tmp_path, capsys):
    import main_stage1
    from counting_detr_amd.args import get_args_parser_stage1
    out = tmp_path / "s1"
    common = ["--data_path", tree, "--output_dir", str(out), "--num_workers", "0", "--device", DEV, "--num_query_position", "100"]
    main_stage1.main(get_args_parser_stage1().parse_args(common + ["--epochs", "2", "--eval_every", "1"]))
    lines = _lines(out / "log.txt")
    assert [l["epoch"] for l in lines] == [0, 1]
    for l in lines:
        assert [k for k in l if k.startswith("test_")] == ["test_loss", "test_loss_wh", "test_loss_giou"]
        assert list(l)[-2:] == ["epoch", "n_parameters"]
    assert lines[0]["train_graph_captures"] == 2 and lines[1]["train_graph_captures"] == 0 and lines[1]["train_graph_steps"] == 4
    capsys.readouterr()
    main_stage1.main(get_args_parser_stage1().parse_args(common + ["--eval", "--resume", str(out / "checkpoint.pth")]))
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("validation:")][-1]
    stats = json.loads(printed[len("validation:"):])
    print("in training", {k: v for k, v in lines[1].items() if k.startswith("test_")}, "--eval", stats)
    assert stats["batches"] == 5
    for k in ("loss", "loss_wh", "loss_giou"):
        assert lines[1]["test_" + k] == stats[k], k
    losses = [l["test_loss"] for l in lines]
    e_best = _argmin_first(losses)
    best = torch.load(out / "checkpoint_best.pth", map_location="cpu", weights_only=False)
    last = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert best["epoch"] == e_best and best["best"] == last["best"] == {"metric": "loss", "value": losses[e_best], "epoch": e_best}


# ---------------------------------------------------------------------------------------------------------------- 6
def test_off_means_off(tree, tmp_path):
    import main as main_mod
    from counting_detr_amd.args import get_args_parser
    out = tmp_path / "plain"
    main_mod.main(get_args_parser().parse_args(_stage2_argv(tree, out, "--epochs", "1")))
    (line,) = _lines(out / "detr_retrain.txt")
    assert set(line) == {"train_" + k for k in LOSS_KEYS + ("loss", "grad_norm", "ms_per_step", "graph_steps", "graph_captures")} | {"epoch"}
    assert list(line)[-1] == "epoch"
    assert sorted(os.listdir(out)) == ["detr_retrain.pth", "detr_retrain.txt"]
    ckpt = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    assert set(ckpt) == {"model", "optimizer", "lr_scheduler", "epoch", "args"}
