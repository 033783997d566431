"""cdetr_criterion_eval (csrc/criterion_eval.hip) behind ops.criterion_eval and SetCriterion.per_image: every image of a batch gets the losses
the reference's SetCriterion returns for it ALONE.  Pinned to the reference's recorded batch-1 losses (goldens stacked into one batch), to the
existing fused kernel run on each image alone, and to its own CPU composition, all at the bar of test_criterion_golden (rtol 1e-4, atol
1e-6, equal_nan); reproducibility, the weighted total, B > 64 and graph replay under a capacity plan are exact comparisons."""
import numpy as np
import pytest
import torch

import eval_split as es

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-4, 1e-6
WD = {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2, "loss_variance": 2}


def make_criterion():
    from counting_detr_amd.anchor_detr import SetCriterion
    from counting_detr_amd.matcher import OriginalHungarianMatcher
    return SetCriterion(1, OriginalHungarianMatcher(2, 5, 2), WD, ["labels", "boxes", "cardinality", "vars"], focal_alpha=0.25)


def targets_of(boxes, dev=DEV):
    return [{"boxes": torch.as_tensor(t).reshape(-1, 4).to(dev), "labels": torch.zeros(len(t), dtype=torch.int64, device=dev)} for t in boxes]


def case(golden, name):
    """A golden case of B images -> (outputs on the device, [target boxes])."""
    z = golden("g45_matcher_criterion.npz")
    outs = {k: torch.from_numpy(z[f"{name}/{k}"]).to(DEV) for k in ("pred_logits", "pred_boxes", "pred_vars")}
    return outs, [torch.from_numpy(z[f"{name}/tgt{b}"]).reshape(-1, 4) for b in range(int(z[f"{name}/B"]))]


def rows_of(losses):
    return torch.stack([losses[k] for k in es.LOSS_KEYS], 1)


def count_calls(monkeypatch):
    from counting_detr_amd import ops
    calls = {"match_cost": 0, "lsap": 0, "criterion_eval": 0}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("key", list(es.STACKS))
def test_stacked_reference_goldens(golden, monkeypatch, key):
    """Row b == case b's recorded L_* after ONE device match and ONE launch; target counts mix (37 ... 3000, some above Q)."""
    outs, tgts, _, want = es.load_stack(golden, key)
    outputs = {k: torch.from_numpy(v).to(DEV) for k, v in outs.items()}
    crit = make_criterion()
    calls = count_calls(monkeypatch)
    got = crit.per_image(outputs, targets_of(tgts))
    assert calls == {"match_cost": 1, "lsap": 1, "criterion_eval": 1}
    assert list(got) == list(es.LOSS_KEYS) and tuple(crit.last_rows.shape) == (len(tgts), 7)
    assert torch.equal(rows_of(got), crit.last_rows[:, :6])
    for k in es.LOSS_KEYS:
        print(key, k, got[k].tolist(), want[k].tolist())
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=k)


def test_nan_of_a_negative_variance_stays_in_its_row(golden):
    outs, tgts, _, _ = es.load_stack(golden, "q300")
    outputs = {k: torch.from_numpy(v).to(DEV) for k, v in outs.items()}
    crit = make_criterion()
    before = crit.per_image(outputs, targets_of(tgts))
    before_rows = crit.last_rows.clone()
    q = int(crit.last_match[0][1, 0])                          # a matched query of image 1
    outputs["pred_vars"][1, q, 0] = -0.25
    after = crit.per_image(outputs, targets_of(tgts))
    assert bool(torch.isnan(after["loss_variance"][1])) and bool(torch.isnan(crit.last_rows[1, 6]))
    keep = [0, 2, 3]
    assert torch.equal(crit.last_rows[keep], before_rows[keep]) and not bool(torch.isnan(crit.last_rows[keep]).any())
    for k in es.LOSS_KEYS[:5]:
        assert torch.equal(after[k], before[k]), k


@pytest.mark.parametrize("name", ["b2_q40", "t0"])
def test_rows_against_the_training_kernel_on_each_image_alone(golden, name):
    """cdetr_criterion_fwd on image b as a batch of one is the per-image quantity by definition; `t0` has an image without targets
    (class_error 100, the box terms 0)."""
    outs, tgts = case(golden, name)
    crit = make_criterion()
    got = crit.per_image(outs, targets_of(tgts))
    for b in range(len(tgts)):
        alone = crit({k: v[b:b + 1] for k, v in outs.items()}, targets_of(tgts[b:b + 1]))
        assert crit.last_total is not None                     # the fused kernel ran
        for k in es.LOSS_KEYS:
            print(name, b, k, float(got[k][b]), float(alone[k]))
            np.testing.assert_allclose(float(got[k][b]), float(alone[k]), rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=f"{k} image {b}")
    if name == "t0":
        b = [len(t) for t in tgts].index(0)
        assert [float(got[k][b]) for k in ("class_error", "loss_bbox", "loss_giou", "loss_variance")] == [100.0, 0.0, 0.0, 0.0]


def test_more_than_64_images_and_reproducibility(golden):
    """B = 65 copies of one Q = 40 image: every row equals row 0 bit for bit (grid and offset indexing past the training kernel's limit);
    two runs are bit-equal; row 0 is the row of the image in a batch of one."""
    outs, tgts = case(golden, "b2_q40")
    crit = make_criterion()
    one = {k: v[1:2] for k, v in outs.items()}
    crit.per_image(one, targets_of(tgts[1:2]))
    single = crit.last_rows.clone()
    many = {k: v[1:2].repeat(65, 1, 1).contiguous() for k, v in outs.items()}
    crit.per_image(many, targets_of(tgts[1:2] * 65))
    first = crit.last_rows.clone()
    assert tuple(first.shape) == (65, 7) and not bool(torch.isnan(first).any())
    assert torch.equal(first, first[:1].expand(65, 7)) and torch.equal(first[:1], single)
    crit.per_image(many, targets_of(tgts[1:2] * 65))
    assert torch.equal(crit.last_rows, first)


def test_weighted_total_is_the_weighted_sum_of_the_row(golden):
    from counting_detr_amd import ops
    outs, tgts = case(golden, "b2_q40")
    crit = make_criterion()
    crit.per_image(outs, targets_of(tgts))
    rows = crit.last_rows.double().cpu().numpy()
    w = np.array([WD.get(k, 0.0) for k in es.LOSS_KEYS], dtype=np.float64)
    # six fp32 products summed in fp32, each possibly fused: a few ulps of the largest partial sum
    np.testing.assert_allclose(rows[:, 6], (rows[:, :6] * w).sum(1), rtol=1e-6, atol=0)
    idx_i, idx_j, plan = crit.last_match                       # without weights: the same six scalars, a total of 0
    t = torch.cat(tgts).to(DEV)
    bare = ops.criterion_eval(outs["pred_logits"], outs["pred_boxes"], outs["pred_vars"], t, torch.zeros(len(t), dtype=torch.int64, device=DEV), plan,
                              idx_i, idx_j, 1, 0.25)
    assert torch.equal(bare[:, :6], crit.last_rows[:, :6]) and bare[:, 6].tolist() == [0.0, 0.0]


def test_graph_replay_with_changed_counts_under_one_capacity_plan(golden):
    """Match + launch captured once over an ops.PackedTargets of capacity 16; other targets loaded, the graph replayed: the rows of a fresh
    call on those targets, bit for bit (the counts are read from device memory)."""
    from counting_detr_amd import ops
    outs, tgts = case(golden, "b2_q40")                        # 7 and 13 targets
    crit = make_criterion()
    B, Q = outs["pred_logits"].shape[:2]
    pk = ops.PackedTargets.with_capacity(B, Q, 16, DEV)
    static = torch.zeros((B, 7), device=DEV)
    pk.load(targets_of(tgts))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crit.per_image(outs, pk, out=static)                   # warm-up: the weight vector and every lazily built table exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh_a = static.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        crit.per_image(outs, pk, out=static)
    changed = [tgts[1][2:6], tgts[0][:0]]                      # 4 targets and none
    pk.load(targets_of(changed))
    g.replay()
    torch.cuda.synchronize()
    replayed = static.clone()
    crit.per_image(outs, targets_of(changed))
    assert torch.equal(replayed, crit.last_rows) and not torch.equal(replayed, fresh_a)
    assert replayed[1, 1].item() == 100.0 and replayed[1, 3:6].tolist() == [0.0, 0.0, 0.0]
    crit.per_image(outs, targets_of(tgts))                     # and the capacity plan's rows are the exact plan's
    assert torch.equal(fresh_a, crit.last_rows)


def test_per_image_on_the_device_agrees_with_its_cpu_composition(golden):
    outs, tgts = case(golden, "b2_q40")
    crit = make_criterion()
    got = crit.per_image(outs, targets_of(tgts))
    idx_i, idx_j, plan = crit.last_match
    indices = [(idx_i[b, :plan.M[b]].cpu(), idx_j[b, :plan.M[b]].cpu()) for b in range(plan.B)]
    ref = make_criterion().per_image({k: v.cpu() for k, v in outs.items()}, targets_of(tgts, "cpu"), indices=indices)
    assert set(ref) == set(got)
    for k in es.LOSS_KEYS:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k].numpy(), rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=k)
