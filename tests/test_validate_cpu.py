"""Validation inside a training run (main.py / main_stage1.py --eval_every, --keep_best), the parts that need no GPU: the best-checkpoint
bookkeeping (checkpoint.BestKeeper), the two parsers' new flags, the epoch's log line (checkpoint.epoch_log_line), which epochs validate,
and the tree the GPU tests train on (tests/validate_tree.py)."""
import json
import math
import os

import pytest

from counting_detr_amd import checkpoint as ck
from counting_detr_amd.args import default_args, get_args_parser, get_args_parser_stage1

# default_args() before --eval_every / --keep_best existed: every other field stays what it was
DEFAULTS_BEFORE = {
    "data_path": "./FSC147/", "output_dir": "./outputs/anchor_detr", "test_split": "val", "lr": 0.0001, "lr_backbone_names": ["backbone"],
    "lr_backbone": 1e-05, "lr_linear_proj_names": [], "lr_linear_proj_mult": 0.1, "batch_size": 1, "weight_decay": 0.0001, "epochs": 30,
    "lr_drop": 20, "lr_drop_epochs": None, "clip_max_norm": 0.1, "sgd": False, "frozen_weights": None, "backbone": "resnet50", "dilation": True,
    "num_feature_levels": 1, "enc_layers": 6, "dec_layers": 6, "dim_feedforward": 1024, "hidden_dim": 256, "dropout": 0.0, "nheads": 8,
    "num_query_position": 300, "num_query_pattern": 1, "spatial_prior": "learned", "attention_type": "RCDA", "masks": False, "aux_loss": False,
    "cost_class": 2, "cost_bbox": 5, "cost_giou": 2, "mask_loss_coef": 1, "dice_loss_coef": 1, "cls_loss_coef": 2, "bbox_loss_coef": 5,
    "giou_loss_coef": 2, "focal_alpha": 0.25, "variance_loss_coef": 2, "device": "cuda", "seed": 42, "resume": "", "auto_resume": False,
    "start_epoch": 0, "eval": False, "num_workers": 2, "scale_factor": 32, "split": "val", "cache_mode": False, "ap_on_host": False,
    "device_detections": False, "eval_batch_size": 1, "dataset": "fsc147", "images_per_gpu": 2, "synthetic": False, "steps_per_epoch": 20,
    "synthetic_size": [800, 800], "pretrained_backbone": "", "resume_skip_mismatch": False, "resume_optimizer": False, "graph_cache": True,
    "graph_cache_size": 32, "graph_layout": "chain", "frozen_prefetch": True, "captured_allreduce": False, "bwd_precision": None,
    "exemplar_mode": "per_image", "device_preprocess": False}


# ---------------------------------------------------------------------------------------------------------------- BestKeeper
def test_lower_is_better_and_a_tie_keeps_the_earlier_epoch():
    for metric, key in (("mae", "MAE"), ("loss", "loss")):
        k = ck.BestKeeper(metric)
        assert k.state() == {"metric": metric, "value": None, "epoch": None}
        took = [k.update({key: v, "AP": 0.9}, e) for e, v in enumerate([3.0, 4.0, 2.5, 2.5, 2.75, 2.0])]
        assert took == [True, False, True, False, False, True]
        assert k.state() == {"metric": metric, "value": 2.0, "epoch": 5}
    k = ck.BestKeeper("mae")
    assert [k.update({"MAE": v}, e) for e, v in enumerate([1.5, 1.5, 1.5])] == [True, False, False] and k.epoch == 0


def test_higher_is_better_for_ap():
    k = ck.BestKeeper("ap", has_ground_truth=True)
    took = [k.update({"AP": v, "MAE": 100.0 - e}, e) for e, v in enumerate([0.25, 0.125, 0.25, 0.5, 0.375])]
    assert took == [True, False, False, True, False]
    assert k.state() == {"metric": "ap", "value": 0.5, "epoch": 3}
    assert ck.BestKeeper("ap").update({"AP": -1.0}, 0)            # COCOeval's "nothing to score" is a number: it is kept until a real one beats it


def test_nan_and_missing_numbers_never_become_best():
    k = ck.BestKeeper("loss")
    assert not k.update({"loss": float("nan")}, 0) and k.state()["value"] is None
    assert not k.update({"MAE": 1.0}, 1) and not k.update(None, 2) and not k.update({}, 3)
    assert k.update({"loss": 7.0}, 4)
    assert not k.update({"loss": float("nan")}, 5) and k.state() == {"metric": "loss", "value": 7.0, "epoch": 4}
    a = ck.BestKeeper("ap")
    assert not a.update({"AP": float("nan")}, 0) and a.update({"AP": 0.0}, 1) and not a.update({"AP": float("nan")}, 2)
    assert k.update({"loss": float("-inf")}, 6)                   # (an infinite loss is ordered, unlike NaN)


def test_state_round_trip_and_a_resumed_keeper_refuses_a_worse_value():
    k = ck.BestKeeper("mae")
    k.update({"MAE": 12.5}, 3)
    state = json.loads(json.dumps(k.state()))                     # what a checkpoint's "best" entry holds
    r = ck.BestKeeper("mae").load(state)
    assert r.state() == k.state() == {"metric": "mae", "value": 12.5, "epoch": 3}
    assert not r.update({"MAE": 13.0}, 4) and not r.update({"MAE": 12.5}, 5) and r.state() == state
    assert r.update({"MAE": 12.25}, 6) and r.state() == {"metric": "mae", "value": 12.25, "epoch": 6}
    h = ck.BestKeeper("ap").load({"metric": "ap", "value": 0.5, "epoch": 1})
    assert not h.update({"AP": 0.25}, 2) and h.update({"AP": 0.75}, 3)
    # an entry of another metric, an empty one or none at all: the keeper starts empty
    for other in (None, {}, {"metric": "loss", "value": 0.1, "epoch": 0}, {"metric": "mae", "value": None, "epoch": None}):
        e = ck.BestKeeper("mae").load(other)
        assert e.state() == {"metric": "mae", "value": None, "epoch": None} and e.update({"MAE": 99.0}, 0)


def test_keep_best_ap_without_ground_truth_raises_at_construction():
    with pytest.raises(ValueError, match="ground truth"):
        ck.BestKeeper("ap", has_ground_truth=False)
    ck.BestKeeper("mae", has_ground_truth=False)
    ck.BestKeeper("loss", has_ground_truth=False)
    with pytest.raises(ValueError):
        ck.BestKeeper("rmse")


# ---------------------------------------------------------------------------------------------------------------- parsers
def test_both_parsers_take_the_flags_and_default_to_off():
    a = get_args_parser().parse_args([])
    assert a.eval_every == 0 and a.keep_best == "mae"
    for choice in ("mae", "ap", "loss"):
        b = get_args_parser().parse_args(["--eval_every", "3", "--keep_best", choice])
        assert b.eval_every == 3 and b.keep_best == choice
    s = get_args_parser_stage1().parse_args([])
    assert s.eval_every == 0 and s.keep_best == "loss"
    s = get_args_parser_stage1().parse_args(["--eval_every", "2", "--keep_best", "loss"])
    assert s.eval_every == 2 and s.keep_best == "loss"
    for parser, bad in ((get_args_parser(), "rmse"), (get_args_parser_stage1(), "mae")):
        with pytest.raises(SystemExit):
            parser.parse_args(["--keep_best", bad])


def test_default_args_is_unchanged_in_every_other_field():
    d = vars(default_args())
    assert d.pop("eval_every") == 0 and d.pop("keep_best") == "mae"
    assert d == DEFAULTS_BEFORE


# ---------------------------------------------------------------------------------------------------------------- log line, schedule
def test_log_line_is_train_then_test_then_epoch():
    train = {"loss": 1.5, "loss_ce": 0.25, "graph_captures": 0}
    test = {"loss": 2.5, "MAE": 3.0, "images": 5, "AP": 0.125}
    line = ck.epoch_log_line(train, test, 7)
    assert list(line) == ["train_loss", "train_loss_ce", "train_graph_captures", "test_loss", "test_MAE", "test_images", "test_AP", "epoch"]
    assert line["train_loss"] == 1.5 and line["test_loss"] == 2.5 and line["test_AP"] == 0.125 and line["epoch"] == 7
    # no pass this epoch: the line main.py has always written
    assert ck.epoch_log_line(train, None, 7) == {**{f"train_{k}": v for k, v in train.items()}, "epoch": 7}
    assert list(ck.epoch_log_line(train, None, 7)) == ["train_loss", "train_loss_ce", "train_graph_captures", "epoch"]
    # main_stage1.py's extra field stays behind "epoch"
    s1 = ck.epoch_log_line({"loss": 1.0}, {"loss": 2.0, "loss_wh": 0.5, "loss_giou": 3.75}, 0, n_parameters=11)
    assert list(s1) == ["train_loss", "test_loss", "test_loss_wh", "test_loss_giou", "epoch", "n_parameters"]
    assert ck.epoch_log_line({"loss": 1.0}, None, 0, n_parameters=11) == {"train_loss": 1.0, "epoch": 0, "n_parameters": 11}
    assert not any(k.startswith("test_") for k in ck.epoch_log_line(train, None, 0))
    assert json.loads(json.dumps(line)) == line


def test_which_epochs_validate():
    assert [e for e in range(7) if ck.validation_due(e, 3, 7)] == [2, 5, 6]           # every third, and always the last
    assert [e for e in range(4) if ck.validation_due(e, 1, 4)] == [0, 1, 2, 3]
    assert [e for e in range(4) if ck.validation_due(e, 2, 4)] == [1, 3]
    assert [e for e in range(4) if ck.validation_due(e, 9, 4)] == [3]
    assert not any(ck.validation_due(e, 0, 4) for e in range(4))                      # off


def test_weighted_loss_is_the_criterions_total():
    wd = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_variance": 2.0, "loss_ce_0": 2.0}
    m = {"loss_ce": 0.5, "class_error": 40.0, "loss_bbox": 0.25, "loss_giou": 1.0, "loss_variance": -0.125, "MAE": 9.0}
    assert ck.weighted_loss(m, wd) == 2.0 * 0.5 + 5.0 * 0.25 + 2.0 * 1.0 + 2.0 * -0.125
    assert math.isnan(ck.weighted_loss({**m, "loss_giou": float("nan")}, wd))


# ---------------------------------------------------------------------------------------------------------------- the tree
def test_the_tree_feeds_every_reader(tmp_path):
    """tests/validate_tree.py: the stage-2 train reader, the stage-2 evaluation reader and the stage-1 readers of both splits open it, the
    training images resize to the two sizes in both orientations and hold 4-9 boxes."""
    import validate_tree as vt
    from counting_detr_amd import data
    root = vt.write_tree(tmp_path / "ds")
    args = get_args_parser().parse_args(["-dp", root] + vt.MODEL_FLAGS)
    train = data.build_dataset(args)
    assert len(train) == 4
    for i, (_, w, h, n) in enumerate(vt.TRAIN_IMAGES):
        s = train[i]
        assert tuple(s["image"].shape) == (3, vt.TRAIN_RESIZED[i][1], vt.TRAIN_RESIZED[i][0])
        assert s["boxes"].shape == (n, 4) and 4 <= n <= 9 and s["ex_rects"].shape == (3, 4)
        assert 0.0 < s["boxes"].min() and s["boxes"].max() < 1.0
    val = data.build_test_dataset(args, "val")
    assert len(val) == 5 and [len(val[i]["boxes"]) for i in range(5)] == [im[3] for im in vt.VAL_IMAGES]
    assert os.path.isfile(os.path.join(root, "instances_val.json"))
    a1 = get_args_parser_stage1().parse_args(["--data_path", root])
    assert len(data.build_dataset_stage1(a1, "train")) == 4 and len(data.build_dataset_stage1(a1, "val")) == 5
    assert data.build_dataset_stage1(a1, "train")[1]["points"].shape == (3, 2)
