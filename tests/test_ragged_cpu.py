"""The host side of stage 1's ragged batches (no GPU): data.collate_stage1_ragged and the size-bucketed batch sampler on
tests/golden/fsc147_tiny, BoundingBoxCriterion(fused=False) with counts on the CPU, and the argument checks of the new entry points
(cdetr_mha_*_lens, cdetr_bbox_criterion_lens_*), which run before any launch."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from ragged_ref import criterion_closed_form, valid_rows

HERE = os.path.dirname(os.path.abspath(__file__))
DS = os.path.join(HERE, "golden", "fsc147_tiny")


@pytest.fixture(scope="module")
def args():
    return argparse.Namespace(data_path=DS, scale_factor=32)


def test_collate_stage1_ragged_pads_points_and_counts(args):
    from counting_detr_amd.data import FSC147PointsDataset, collate_stage1, collate_stage1_ragged
    ds = FSC147PointsDataset(args, "train")
    samples = [ds[i] for i in range(len(ds))]
    counts = [s["points"].shape[0] for s in samples]
    assert len(set(counts)) > 1, "the tiny split must mix point counts for this test to mean anything"
    b = collate_stage1_ragged(samples)
    B, N = len(samples), max(counts)
    assert b["points"].shape == (B, N, 2) and b["points"].dtype == torch.float32
    assert b["counts"].dtype == torch.int32 and b["counts"].tolist() == counts
    assert "whs" not in b and b["im_id"].tolist() == [s["im_id"] for s in samples]
    for i, s in enumerate(samples):
        assert torch.equal(b["points"][i, :counts[i]], torch.as_tensor(s["points"], dtype=torch.float32))
        assert bool((b["points"][i, counts[i]:] == 0.5).all())
    one = collate_stage1([samples[0]])                         # image / mask: collate_stage1's
    assert torch.equal(collate_stage1_ragged([samples[0]])["image"], one["image"])
    dense = collate_stage1(samples[:1] * 2)
    assert torch.equal(b["image"][0, :, :dense["image"].shape[2], :dense["image"].shape[3]], dense["image"][0])


def test_collate_stage1_ragged_whs_fill_and_equal_counts(args):
    from counting_detr_amd.data import FSC147ExemplarDataset, collate_stage1, collate_stage1_ragged
    ds = FSC147ExemplarDataset(args, "train")
    s0, s1 = ds[0], ds[1]
    dense, rag = collate_stage1([s0, s1]), collate_stage1_ragged([s0, s1])
    assert set(rag) == set(dense) | {"counts"}
    for k in dense:                                            # equal counts: collate_stage1's tensors plus counts
        assert torch.equal(rag[k], dense[k]), k
    assert rag["counts"].tolist() == [s0["points"].shape[0]] * 2
    short = dict(s1)
    short["points"], short["whs"] = s1["points"][:1], s1["whs"][:1]
    rag = collate_stage1_ragged([s0, short])
    n = s0["points"].shape[0]
    assert rag["counts"].tolist() == [n, 1] and rag["whs"].shape == (2, n, 2)
    assert bool((rag["whs"][1, 1:] == 0).all()) and bool((rag["points"][1, 1:] == 0.5).all())
    assert torch.equal(rag["whs"][1, :1], torch.as_tensor(short["whs"], dtype=torch.float32))
    empty = dict(s1)
    empty["points"], empty["whs"] = s1["points"][:0], s1["whs"][:0]
    with pytest.raises(ValueError, match="without points"):
        collate_stage1_ragged([s0, empty])


def test_collate_stage1_ragged_raw_carries_the_same_fields(args):
    from counting_detr_amd.data import FSC147PointsDataset, collate_stage1_ragged, collate_stage1_ragged_raw
    host = FSC147PointsDataset(args, "train")
    raw = FSC147PointsDataset(args, "train", raw=True)
    a = collate_stage1_ragged([host[0], host[1]])
    b = collate_stage1_ragged_raw([raw[0], raw[1]])
    assert set(b) == (set(a) - {"image", "mask"}) | {"raw"}
    for k in ("points", "counts", "orig_size", "im_id"):
        assert torch.equal(a[k], b[k]), k
    assert (b["raw"]["Hm"], b["raw"]["Wm"]) == tuple(a["image"].shape[2:])


@pytest.mark.parametrize("batch_size", [1, 2, 3])
def test_size_bucket_sampler(args, batch_size):
    from PIL import Image
    from counting_detr_amd.data import FSC147PointsDataset, SizeBucketBatchSampler
    ds = FSC147PointsDataset(args, "train")
    sampler = SizeBucketBatchSampler(ds, batch_size)
    batches = list(sampler)
    assert len(batches) == len(sampler) and batches == list(SizeBucketBatchSampler(ds, batch_size))      # deterministic
    assert sorted(i for b in batches for i in b) == list(range(len(ds)))                                 # every index exactly once

    def resized(i):
        w, h = Image.open(os.path.join(ds.im_dir, ds.data_split[i])).size
        return 32 * int(w / 32), 32 * int(h / 32)
    for b, size in zip(batches, sampler.sizes):
        assert 1 <= len(b) <= batch_size and b == sorted(b)                                              # dataset order within a size
        assert {resized(i) for i in b} == {size}
        assert all(tuple(ds[i]["image"].shape[1:]) == (size[1], size[0]) for i in b)                     # the reader's own rule
    with pytest.raises(ValueError):
        SizeBucketBatchSampler(ds, 0)


def _case(B=3, N=7, seed=31):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(B, N, 2, generator=g) * 0.8 + 0.1
    tw = torch.rand(B, N, 2, generator=g) * 0.3 + 0.01
    coord = torch.cat([torch.rand(B, N, 2, generator=g), tw * (torch.rand(B, N, 2, generator=g) + 0.5)], -1)
    return coord, pts, tw


def test_unfused_criterion_with_counts_on_the_cpu():
    from counting_detr_amd import stage1
    lens = [7, 1, 4]
    coord, pts, tw = _case()
    crit = stage1.BoundingBoxCriterion()
    valid = valid_rows(lens, 7)

    def run(coord, pts, tw):
        c = coord.clone().requires_grad_(True)
        ld, total = crit.forward_with_total({"pred_wh": c[..., 2:], "pred_boxes": c},
                                            {"points": pts, "whs": tw, "counts": torch.tensor(lens, dtype=torch.int32)})
        total.backward()
        return float(ld["loss_wh"].detach()), float(ld["loss_giou"].detach()), float(total.detach()), c.grad

    l_wh, l_gi, total, grad = run(coord, pts, tw)
    # the composition on the concatenated valid pairs, as a batch of one "image"
    cc = coord[valid][None].clone().requires_grad_(True)
    ld, tot = crit.forward_with_total({"pred_wh": cc[..., 2:], "pred_boxes": cc}, {"points": pts[valid][None], "whs": tw[valid][None]})
    tot.backward()
    assert (l_wh, l_gi, total) == (float(ld["loss_wh"].detach()), float(ld["loss_giou"].detach()), float(tot.detach()))
    assert torch.equal(grad[valid], cc.grad[0]) and float(grad[~valid].abs().sum()) == 0.0
    r_wh, r_gi, _, _ = criterion_closed_form(coord, pts, tw, lens)
    np.testing.assert_allclose([l_wh, l_gi], [r_wh, r_gi], rtol=1e-5)
    # padded values take no part: NaN there changes nothing
    coord2, pts2, tw2 = coord.clone(), pts.clone(), tw.clone()
    coord2[~valid], pts2[~valid], tw2[~valid] = float("nan"), float("nan"), float("nan")
    l2 = run(coord2, pts2, tw2)
    assert l2[:3] == (l_wh, l_gi, total) and torch.equal(l2[3], grad)
    # all counts == N: today's dense batch
    full = crit.forward_with_total({"pred_wh": coord[..., 2:]}, {"points": pts, "whs": tw, "counts": torch.full((3,), 7, dtype=torch.int32)})
    dense = crit.forward_with_total({"pred_wh": coord[..., 2:]}, {"points": pts, "whs": tw})
    assert float(full[1]) == float(dense[1])


def test_lens_entry_points_validate_before_launching():
    """Null pointers and bad sizes come back as an error code with cdetr_last_error set; nothing is launched (this runs without a GPU)."""
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    buf = ctypes.create_string_buffer(64)                     # 16-byte aligned host memory: never dereferenced by the checks
    p = (ctypes.addressof(buf) + 15) & ~15
    ok5, ok9 = [p] * 5, [p] * 9
    for k in range(5):
        a = list(ok5)
        a[k] = None
        assert L.cdetr_mha_fwd_lens(*a, 2, 5, 8, 0.17, 0, None) < 0 and b"cdetr_mha_fwd_lens" in L.cdetr_last_error()
    for k in range(9):
        a = list(ok9)
        a[k] = None
        assert L.cdetr_mha_bwd_lens(*a, 2, 5, 8, 0.17, 0, None) < 0 and b"cdetr_mha_bwd_lens" in L.cdetr_last_error()
    for N, Ln, nh in ((0, 5, 8), (2, 0, 8), (2, 5, 0), (-1, 5, 8)):
        assert L.cdetr_mha_fwd_lens(*ok5, N, Ln, nh, 0.17, 0, None) < 0 and b"bad sizes" in L.cdetr_last_error()
        assert L.cdetr_mha_bwd_lens(*ok9, N, Ln, nh, 0.17, 0, None) < 0 and b"bad sizes" in L.cdetr_last_error()
    assert L.cdetr_mha_fwd_lens(p + 4, p, p, p, p, 2, 5, 8, 0.17, 0, None) < 0 and b"aligned" in L.cdetr_last_error()
    # criterion: (pred_wh, stride, tgt_points, tgt_whs, lens, B, N, w_wh, w_giou, losses, g_wh, g_giou, stream)
    good = [p, 4, p, p, p, 3, 7, 1.0, 0.4, p, p, p, None]
    for k in (0, 2, 3, 4, 9, 10, 11):
        a = list(good)
        a[k] = None
        assert L.cdetr_bbox_criterion_lens_fwd(*a) < 0 and b"cdetr_bbox_criterion_lens_fwd" in L.cdetr_last_error()
    for k, bad in ((1, 1), (5, 0), (6, 0), (5, 1 << 20)):     # stride < 2, B = 0, N = 0, B * N beyond 2^28
        a = list(good)
        a[k] = bad
        if k == 5 and bad > 1:
            a[6] = 1 << 20
        assert L.cdetr_bbox_criterion_lens_fwd(*a) < 0 and b"bad sizes" in L.cdetr_last_error()
    # (g3, w_wh, w_giou, g_wh, g_giou, lens, d_coord, B, N, stream)
    good = [p, 1.0, 0.4, p, p, p, p, 3, 7, None]
    for k in (0, 3, 4, 5, 6):
        a = list(good)
        a[k] = None
        assert L.cdetr_bbox_criterion_lens_bwd(*a) < 0 and b"cdetr_bbox_criterion_lens_bwd" in L.cdetr_last_error()
    a = list(good)
    a[7] = 0
    assert L.cdetr_bbox_criterion_lens_bwd(*a) < 0 and b"bad sizes" in L.cdetr_last_error()
    a = list(good)
    a[6] = p + 4
    assert L.cdetr_bbox_criterion_lens_bwd(*a) < 0 and b"aligned" in L.cdetr_last_error()
