"""The host side of batched evaluation (no GPU): the --eval_batch_size flag, the size-bucketed batches of an evaluation split written into
tmp_path, SetCriterion.per_image's CPU composition against the reference's recorded batch-1 losses, and the boundary of the new entry point
(descriptor mirror, argument checks before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import eval_split as es


@pytest.fixture(scope="module")
def lib():
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    from counting_detr_amd import _ffi
    return _ffi.lib()


def make_criterion():
    from counting_detr_amd.anchor_detr import SetCriterion
    from counting_detr_amd.matcher import OriginalHungarianMatcher
    wd = {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2, "loss_variance": 2}
    return SetCriterion(1, OriginalHungarianMatcher(2, 5, 2), wd, ["labels", "boxes", "cardinality", "vars"], focal_alpha=0.25)


def test_eval_batch_size_flag_defaults_to_one():
    from counting_detr_amd.args import default_args, get_args_parser
    assert get_args_parser().parse_args([]).eval_batch_size == 1
    assert default_args().eval_batch_size == 1
    assert get_args_parser().parse_args(["--eval_batch_size", "16"]).eval_batch_size == 16


def test_size_buckets_of_an_evaluation_split(tmp_path):
    """Three images of one resized size and two of another at B = 2: three batches, one size each, the same on every pass -- from the sampler
    and from the loader infer.py builds with the flag."""
    import infer as infer_mod
    from counting_detr_amd import data
    from counting_detr_amd.args import default_args
    args = default_args()
    args.data_path, args.scale_factor, args.split, args.num_workers, args.eval_batch_size = es.write_split(tmp_path / "ds"), 32, "val", 0, 2
    ds = data.build_test_dataset(args, "val")
    assert len(ds) == 5
    sampler = data.SizeBucketBatchSampler(ds, 2)
    assert list(sampler) == es.BATCHES_AT_2 == list(sampler) == list(data.SizeBucketBatchSampler(ds, 2))
    assert sampler.sizes == [es.RESIZED[b[0]] for b in es.BATCHES_AT_2]
    for b, size in zip(sampler, sampler.sizes):
        assert {es.RESIZED[i] for i in b} == {size}
        assert all(tuple(ds[i]["image"].shape[1:]) == (size[1], size[0]) for i in b)
    dl, per_image = infer_mod.eval_loader(args, torch.device("cpu"))
    assert per_image
    for _ in range(2):                                     # every pass
        got = list(dl)
        assert [b["image_id"].tolist() for b in got] == [[i + 1 for i in b] for b in es.BATCHES_AT_2]
        for b, size in zip(got, sampler.sizes):
            assert tuple(b["image"].shape[2:]) == (size[1], size[0]) and not bool(b["mask"].any())      # one size: nothing is padded
    args.eval_batch_size = 1                               # the default: dataset order, one image each, the batched criterion
    dl1, per_image1 = infer_mod.eval_loader(args, torch.device("cpu"))
    assert not per_image1 and [b["image_id"].tolist() for b in dl1] == [[1], [2], [3], [4], [5]]
    args.eval_batch_size = 0
    with pytest.raises(ValueError):
        infer_mod.eval_loader(args, torch.device("cpu"))


@pytest.mark.parametrize("key", list(es.STACKS))
def test_per_image_cpu_reproduces_the_reference_batch_one_losses(golden, key):
    """Reference goldens of batch 1 stacked into one batch: entry b of every loss is case b's recorded value (rtol 1e-4, atol 1e-6 -- the bar of
    test_criterion_golden); target counts mix, some above Q."""
    outs, tgts, idx, want = es.load_stack(golden, key)
    outputs = {k: torch.from_numpy(v) for k, v in outs.items()}
    targets = [{"boxes": torch.from_numpy(t), "labels": torch.zeros(t.shape[0], dtype=torch.int64)} for t in tgts]
    got = make_criterion().per_image(outputs, targets, indices=[(torch.from_numpy(i), torch.from_numpy(j)) for i, j in idx])
    assert set(got) == set(es.LOSS_KEYS)
    for k in es.LOSS_KEYS:
        assert tuple(got[k].shape) == (len(tgts),)
        print(key, k, got[k].tolist(), want[k].tolist())
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=1e-4, atol=1e-6, equal_nan=True, err_msg=k)


def test_per_image_cpu_needs_indices():
    with pytest.raises(RuntimeError, match="indices"):
        make_criterion().per_image({"pred_logits": torch.zeros(1, 4, 2), "pred_boxes": torch.zeros(1, 4, 4), "pred_vars": torch.ones(1, 4, 2)},
                                   [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}])


def test_descriptor_mirrors_the_header_and_bad_arguments_launch_nothing(lib):
    from counting_detr_amd import _ffi
    names = abi_header.field_names("cdetr_criterion_eval_desc")
    assert names == [f[0] for f in _ffi.CriterionEvalDesc._fields_]
    assert not any(n.startswith("g_") or n == "num_boxes" for n in names)                 # forward only, the normaliser is formed in the kernel
    L = lib
    assert L.cdetr_abi_version() == 2
    assert L.cdetr_criterion_eval(None, None) < 0 and b"cdetr_criterion_eval" in L.cdetr_last_error()
    d = _ffi.CriterionEvalDesc()
    d.B, d.Q, d.C, d.Mmax = 65, 40, 2, 40                                                 # sizes pass (B > 64 is fine), the pointers are null
    assert L.cdetr_criterion_eval(ctypes.byref(d), None) < 0 and b"null pointer" in L.cdetr_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from counting_detr_amd import ops
        ops.criterion_eval(torch.zeros(1, 4, 2), torch.zeros(1, 4, 4), torch.ones(1, 4, 2), torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64),
                           ops.MatchPlan((0,), 4, "cpu"), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int64), 1, 0.25)
