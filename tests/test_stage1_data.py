"""1st-stage readers (data.FSC147ExemplarDataset / FSC147PointsDataset) against the REAL reference's FSCD147_Exemplars / FSCD147_Points
run on tests/golden/fsc147_tiny (arrays in tests/golden/g12_stage1_train.npz, tools/gen_golden_stage1_train.py), and collate_stage1."""
import argparse
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DS = os.path.join(HERE, "golden", "fsc147_tiny")


@pytest.fixture(scope="module")
def args():
    return argparse.Namespace(data_path=DS, scale_factor=32)


def _check(sample, z, prefix):
    keys = [k.split("/", 1)[1] for k in z.files if k.startswith(prefix + "/")]
    assert keys and sorted(keys) == sorted(sample.keys()), (sorted(keys), sorted(sample.keys()))
    for k in keys:
        ref = z[f"{prefix}/{k}"]
        got = sample[k].numpy() if torch.is_tensor(sample[k]) else np.asarray(sample[k])
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if ref.dtype.kind == "f":
            assert got.dtype == ref.dtype, (k, got.dtype, ref.dtype)
            tol = 1e-6 if k == "image" else 0.0
            np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=f"{prefix}/{k}")
        else:
            assert np.array_equal(got, ref), f"{prefix}/{k}"


@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_exemplar_reader_matches_reference(golden, args, split):
    from counting_detr_amd.data import FSC147ExemplarDataset
    z = golden("g12_stage1_train.npz")
    ds = FSC147ExemplarDataset(args, split)
    assert len(ds) == int(z[f"ex_{split}/len"])
    for i in range(len(ds)):
        s = ds[i]
        assert s["image"].shape[1] % 32 == 0 and s["image"].shape[2] % 32 == 0
        _check(s, z, f"ex_{split}{i}")


@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_points_reader_matches_reference(golden, args, split):
    from counting_detr_amd.data import FSC147PointsDataset
    z = golden("g12_stage1_train.npz")
    ds = FSC147PointsDataset(args, split)
    assert len(ds) == int(z[f"pts_{split}/len"])
    for i in range(len(ds)):
        _check(ds[i], z, f"pts_{split}{i}")


def test_collate_stage1_pads_and_masks_like_collate(args):
    from counting_detr_amd.data import FSC147ExemplarDataset, collate, collate_stage1
    ds = FSC147ExemplarDataset(args, "train")
    samples = [ds[0], ds[1]]
    b = collate_stage1(samples)
    # the 2nd-stage collate on the same images (its other fields stubbed) pads / masks identically
    ref = collate([{"image": s["image"], "ex_rects": np.zeros((3, 4), np.float32), "boxes": np.zeros((0, 4), np.float32),
                    "labels": np.zeros(0, np.int64), "orig_size": s["orig_size"]} for s in samples])
    assert torch.equal(b["image"], ref["image"]) and torch.equal(b["mask"], ref["mask"])
    assert b["image"].shape[2:] == (max(s["image"].shape[1] for s in samples), max(s["image"].shape[2] for s in samples))
    assert b["mask"][0].any() and not b["mask"][1].any()
    assert b["points"].shape == b["whs"].shape == (2, 3, 2) and b["points"].dtype == torch.float32
    for i, s in enumerate(samples):
        assert torch.equal(b["points"][i], torch.as_tensor(s["points"])) and torch.equal(b["whs"][i], torch.as_tensor(s["whs"]))
    assert b["orig_size"].tolist() == [list(s["orig_size"]) for s in samples]


def test_collate_stage1_rejects_unequal_counts(args):
    from counting_detr_amd.data import FSC147ExemplarDataset, FSC147PointsDataset, collate_stage1
    ds = FSC147ExemplarDataset(args, "train")
    s0, s1 = ds[0], dict(ds[1])
    s1["points"], s1["whs"] = s1["points"][:2], s1["whs"][:2]
    with pytest.raises(ValueError, match="different numbers of points"):
        collate_stage1([s0, s1])
    pts = FSC147PointsDataset(args, "train")                          # 6 and 7 dots: batch 1 only
    with pytest.raises(ValueError):
        collate_stage1([pts[0], pts[1]])
    one = collate_stage1([pts[1]])
    assert one["points"].shape == (1, len(pts[1]["points"]), 2) and one["im_id"].tolist() == [pts[1]["im_id"]]
