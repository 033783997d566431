"""cdetr_criterion_fwd / _bwd (ops.CriterionFn), the tensor-op composition of SetCriterion, cdetr_criterion_eval (ops.criterion_eval,
SetCriterion.per_image), cdetr_match_cost and cdetr_lsap against fp64 at the cases of tests/criterion_edges_ref.py: GIoU ties and clamps at
0, sign(0), saturated logits, argmax ties, images without targets, T > Q, padded index slots, three classes, the dynamic-LDS launch sizes,
and the class cost's ill-conditioned band.  Every tensor is held to bar = min(the golden tests' bar, max(8 x floor, 2^-21)), floor being
the fp32 CPU oracle's own error against fp64 on that case (never a kernel's output); the gradients are taken one loss at a time, each under
its own scale.  Needs an MI355X.

Measured on an MI355X (`pytest -s` prints every figure; profiles/criterion_edges_floor_bar_measured.md lists them all).  Cells are
floor/bar/measured in units of 1e-8; the factor on the floor is 8 for every tensor (none had to be raised); class_error and
cardinality_error matched exactly everywhere.  Columns: the scalars, then d_logits, d_boxes, d_vars of one loss (dl, db, dv); the gradients
of the weighted total are in the profile.  ops.CriterionFn on the edge cases:

    case                           ce        bbox        giou         var       total       dl/ce     db/bbox     db/giou      db/var      dv/var
    identical                 10/79/3      1/48/1      3/48/3      3/48/3      3/48/3     10/84/8      4/48/4      9/71/9     2/48/11     9/75/12
    shared_edge                3/48/3      1/48/1      2/48/7      2/48/5      0/48/0   14/115/20      3/48/3   13/103/12     8/62/14     10/81/7
    concentric                9/71/10      1/48/1      0/48/0      1/48/7      6/51/1    22/173/9      1/48/1     8/66/11      6/48/5      7/55/8
    same_cx_w                  9/69/9      0/48/0     11/88/0      1/48/1      3/48/3    10/82/16      3/48/3     10/81/9      5/48/4    11/90/11
    disjoint                 13/101/3      0/48/8      0/48/0      3/48/3      9/71/5   18/148/18      5/48/5   13/101/14     3/48/12   12/100/14
    tiny                       2/48/8      3/48/4      2/48/9      2/48/2      2/48/2   14/114/14      1/48/1     11/90/4     12/92/2     8/65/11
    logit_sat                  4/48/4      4/48/4     10/83/6      9/72/2      1/48/1 115/917/115      2/48/2      7/56/9     10/81/8    10/80/10
    var_edges                  7/53/5      2/48/2      3/48/6      4/48/4      4/48/4    11/88/16      3/48/3     11/88/6    15/117/5     8/60/12
    t_gt_q                     0/48/0      0/48/0      2/48/2      1/48/1      2/48/2    10/84/14      0/48/0    12/100/6      5/48/6      8/61/8
    t_mixed                    1/48/5      4/48/6      4/48/4     11/91/1      1/48/1    11/88/20      1/48/1    13/103/7    10/79/22    10/79/10
    t_none                    3/48/11      0/48/0      0/48/0      0/48/0     3/48/11   21/167/14      0/48/0      0/48/0      0/48/0      0/48/0
    c3                        10/82/8      3/48/3      9/73/0      1/48/6     12/98/2   34/269/20      0/48/0     8/63/10     10/78/7      7/57/9

and at the launch-size edges (dynamic LDS bytes in brackets):

    case                           ce        bbox        giou         var       total       dl/ce     db/bbox     db/giou      db/var      dv/var
    b64_q24 (6144 B)           7/54/7      5/48/5     11/89/2      1/48/1      9/73/9   44/352/52      0/48/0      5/48/6      8/66/8    10/78/13
    b16_q800 (51200 B)        12/96/5      1/48/1      4/48/4      7/52/7    16/132/0   56/444/56      1/48/1      5/48/5      4/48/9    10/78/14
    b44_q900 (158400 B)        5/48/8      4/48/4      2/48/2      5/48/5      3/48/9   57/458/49      1/48/1      4/48/4      2/48/5    11/87/12
    b64_q624 (159744 B)        5/48/5      3/48/7      2/48/2      3/48/3      4/48/4   57/454/57      3/48/3      8/64/9     10/78/5   15/117/16

Largest measured / bar, ops.CriterionFn: 0.27 (t_mixed d_boxes/var: floor 9.8e-08, bar 7.9e-07, measured 2.2e-07).
Largest measured / bar, launch-size edges: 0.19 (b44_q900 (158400 B) total: floor 3.4e-08, bar 4.8e-07, measured 9.1e-08).
Largest measured / bar, tensor-op composition: 0.39 (shared_edge loss_ce: floor 3.0e-08, bar 4.8e-07, measured 1.9e-07).
Largest measured / bar, ops.criterion_eval rows: 0.22 (disjoint image 0 (T 5) loss_variance: floor 3.5e-08, bar 4.8e-07, measured 1.1e-07).
ops.match_cost: 0 of 13800 entries outside the +-2 ulp bracket (band up to 4.8 wide); 3459 entries differ from the fp32 CPU oracle, by at most
3.8e-06; against fp64 on the well-conditioned rows measured / bar <= 0.13 (floors 4e-8 ... 8e-8, bars 4.8e-7 ... 6.7e-7).
"""
import numpy as np
import pytest
import torch

import criterion_edges_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSSES = ["labels", "boxes", "cardinality", "vars"]
WD = {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2, "loss_variance": 2}
# factor on the floor per tensor (8 unless a reason is written beside it)
FACTORS = {}
case_param = pytest.mark.parametrize("name", R.CASES)
match_param = pytest.mark.parametrize("launch,table", R.MATCH_CASES, ids=[f"{a}-{b}" for a, b in R.MATCH_CASES])


def hold(tag, got, ref, floors, keys, exact=R.EXACT):
    """Every tensor of `keys` within its bar of fp64; prints measured / floor / bar; -> the bars."""
    failed, bars = [], {}
    for k in keys:
        name = "d_vars" if k.endswith("/vars") else k
        if k in exact:
            ok = float(got[k]) == ref[k]
            print(f"EDGE {tag} {k}: exact {float(got[k])!r} vs {ref[k]!r}")
            if not ok:
                failed.append(f"{k}: {float(got[k])!r} != {ref[k]!r}")
            continue
        e = R.err(name, got[k], ref[k])
        factor = FACTORS.get(k, R.FACTOR)
        bars[k] = R.bar(R.existing(k), floors[k], factor)
        print(f"EDGE {tag} {k}: floor {floors[k]:.2e} bar {bars[k]:.2e} measured {e:.2e} factor {factor:g}")
        if not e <= bars[k]:
            failed.append(f"{k}: {e:.3e} > {bars[k]:.3e}")
    assert not failed, tag + ": " + "; ".join(failed)
    return bars


def device_inputs(c, order=None):
    """The case on the device, its images in `order`: (logits, boxes, vars) leaves, packed targets, exact plan, padded indices."""
    from counting_detr_amd import ops
    sel = list(range(c.B)) if order is None else list(order)
    leaves = [t[sel].clone().to(DEV).requires_grad_(True) for t in (c.logits, c.boxes, c.vars)]
    tb = torch.cat([c.tgt_boxes[b] for b in sel]).reshape(-1, 4).to(DEV)
    tl = torch.cat([c.tgt_labels[b] for b in sel]).to(torch.int64).to(DEV)
    plan = ops.MatchPlan([c.sizes[b] for b in sel], c.Q, DEV)
    ii, jj = R.device_indices(c)
    return leaves, tb, tl, plan, ii[sel].contiguous().to(DEV), jj[sel].contiguous().to(DEV)


def run_fused(c):
    """ops.CriterionFn on the case -> dict of R.SCALARS + R.GRADS + d_total (one backward per loss: vec with a one-hot g6; then the total)."""
    from counting_detr_amd import ops
    leaves, tb, tl, plan, ii, jj = device_inputs(c)
    nb = torch.full((1,), max(float(sum(c.sizes)), 1.0), device=DEV)
    w6 = torch.tensor(R.W6, device=DEV)
    vec, tot = ops.CriterionFn.apply(*leaves, tb, tl, plan, ii, jj, nb, c.num_classes, R.ALPHA, w6)
    out = {k: vec[i].detach().cpu() for i, k in enumerate(R.ORDER6)}
    out["total"] = tot.detach().cpu()
    zero = {}
    for slot, names in ((0, ("d_logits/ce", None, None)), (3, (None, "d_boxes/bbox", None)), (4, (None, "d_boxes/giou", None)),
                        (5, (None, "d_boxes/var", "d_vars/var"))):
        g6 = torch.zeros(6, device=DEV)
        g6[slot] = 1.0
        grads = torch.autograd.grad(vec, leaves, grad_outputs=g6, retain_graph=True)
        for name, gr in zip(names, grads):
            if name:
                out[name] = gr.cpu()
            else:
                zero[slot] = zero.get(slot, 0.0) + float(gr.abs().sum())
    assert all(v == 0.0 for v in zero.values()), zero                      # a loss moves only its own inputs
    out["d_total"] = tuple(gr.cpu() for gr in torch.autograd.grad(tot, leaves))
    torch.cuda.synchronize()
    return out


class FixedMatcher:
    """Stand-in for the device matcher: the case's hand-made indices and a zero status."""

    def __init__(self, ii, jj):
        self.ii, self.jj = ii, jj

    def match_device(self, outputs, targets, plan=None, tgt_boxes=None, cost=None):
        return self.ii, self.jj, torch.zeros(self.ii.shape[0], dtype=torch.int32, device=self.ii.device), plan


def criterion_for(c, order=None):
    from counting_detr_amd.anchor_detr import SetCriterion
    sel = list(range(c.B)) if order is None else list(order)
    ii, jj = R.device_indices(c)
    crit = SetCriterion(c.num_classes, FixedMatcher(ii[sel].contiguous().to(DEV), jj[sel].contiguous().to(DEV)), WD, LOSSES, focal_alpha=R.ALPHA)
    targets = [{"boxes": c.tgt_boxes[b].to(DEV), "labels": c.tgt_labels[b].to(DEV)} for b in sel]
    return crit, targets


def run_composition(c):
    """SetCriterion.forward with fused = False (tensor ops on the device) -> the same dict as run_fused."""
    crit, targets = criterion_for(c)
    crit.fused = False
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in (c.logits, c.boxes, c.vars)]
    losses = crit(dict(zip(("pred_logits", "pred_boxes", "pred_vars"), leaves)), targets)
    assert crit.last_total is None
    out = {k: losses[k].detach().cpu() for k in R.ORDER6}
    total = sum(losses[k] * WD[k] for k in losses if k in WD)
    out["total"] = total.detach().cpu()
    for name, (loss, which) in R.GRAD_OF.items():
        gr, = torch.autograd.grad(losses[loss], leaves[which], retain_graph=True, allow_unused=True)
        out[name] = torch.zeros_like(leaves[which]).cpu() if gr is None else gr.cpu()
    gt = torch.autograd.grad(total, leaves, allow_unused=True)
    out["d_total"] = tuple(torch.zeros_like(x).cpu() if gr is None else gr.cpu() for x, gr in zip(leaves, gt))
    return out


def flat(res):
    out = dict(res)
    out["d_total/logits"], out["d_total/boxes"], out["d_total/vars"] = res["d_total"]
    return out


ALL_KEYS = R.SCALARS + R.GRADS + ("d_total/logits", "d_total/boxes", "d_total/vars")


@case_param
def test_fused_criterion_vs_fp64(name):
    c = R.case(name)
    got, ref = flat(run_fused(c)), flat(R.reference(c))
    hold(f"fused {name}", got, ref, R.floor(c), ALL_KEYS)
    rows = R.matched_rows(c)
    for k in R.GRADS[1:] + ("d_total/boxes", "d_total/vars"):              # unmatched queries: exactly 0
        assert float(got[k][~rows].abs().sum()) == 0.0, k
    again = flat(run_fused(c))
    for k in ALL_KEYS:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"


@case_param
def test_tensor_op_composition_vs_fp64_and_the_fused_kernel(name):
    c = R.case(name)
    got, ref = flat(run_composition(c)), flat(R.reference(c))
    # class_error and cardinality_error under the scalar bar here (floor 0, so 2^-21): torch's device mean multiplies by 1 / B where the
    # reference's CPU mean and the fused kernel divide by B, one ulp apart at B = 3
    bars = hold(f"composition {name}", got, ref, R.floor(c), ALL_KEYS, exact=())
    fused = flat(run_fused(c))
    failed = []
    for k, b in bars.items():
        e = R.err("d_vars" if k.endswith("/vars") else k, got[k], fused[k])
        print(f"EDGE composition-fused {name} {k}: {e:.2e} (2 x bar {2 * b:.2e})")
        if not e <= 2 * b:
            failed.append(f"{k}: {e:.3e} > {2 * b:.3e}")
    assert not failed, "; ".join(failed)


def eval_rows(c, order=None):
    from counting_detr_amd import ops
    leaves, tb, tl, plan, ii, jj = device_inputs(c, order)
    rows = ops.criterion_eval(*(x.detach() for x in leaves), tb, tl, plan, ii, jj, c.num_classes, R.ALPHA, torch.tensor(R.W6, device=DEV))
    torch.cuda.synchronize()
    return rows.cpu()


@case_param
def test_per_image_rows_vs_fp64_alone_and_batch_independence(name):
    c = R.case(name)
    rows = eval_rows(c)
    assert tuple(rows.shape) == (c.B, 7)
    for b in range(c.B):
        got = {k: rows[b, i] for i, k in enumerate(R.SCALARS)}
        hold(f"eval {name} image {b} (T {c.sizes[b]})", got, R.reference_per_image(c, b), R.floor_per_image(c, b), R.SCALARS)
        if c.sizes[b] == 0:
            assert rows[b, 1].item() == 100.0 and rows[b, 3:6].tolist() == [0.0, 0.0, 0.0]
    order = list(range(c.B))[::-1] if c.B > 1 else [0, 0, 0]               # other neighbours (or copies of itself): the same bits
    moved = eval_rows(c, order)
    for pos, b in enumerate(order):
        assert torch.equal(moved[pos], rows[b]), f"row of image {b} depends on its batch"
    crit, targets = criterion_for(c)
    outs = {k: v.to(DEV) for k, v in (("pred_logits", c.logits), ("pred_boxes", c.boxes), ("pred_vars", c.vars))}
    per = crit.per_image(outs, targets)
    assert torch.equal(crit.last_rows.cpu(), rows)
    for i, k in enumerate(R.ORDER6):
        assert torch.equal(per[k].cpu(), rows[:, i]), k


@pytest.mark.parametrize("B,Q", R.SIZE_CASES, ids=[f"b{B}_q{Q}" for B, Q in R.SIZE_CASES])
def test_fused_criterion_launch_size_edges(B, Q):
    """B = 64; the first B * Q * 4 past 48 KiB (dynamic LDS through hipFuncSetAttribute); the documented and the exact largest sizes."""
    c = R.size_case(B, Q)
    assert B <= 64 and B * Q * 4 <= 160 * 1024 - 4096
    got, ref = flat(run_fused(c)), flat(R.reference(c))
    hold(f"size b{B}_q{Q} ({B * Q * 4} B)", got, ref, R.floor(c), ALL_KEYS)
    rows = R.matched_rows(c)
    for k in R.GRADS[1:]:
        assert float(got[k][~rows].abs().sum()) == 0.0, k


@pytest.mark.parametrize("B,Q,msg", [(65, 24, "bad sizes"), (64, 625, "too large"), (44, 908, "too large")])
def test_fused_criterion_refuses_sizes_past_its_limits(B, Q, msg):
    from counting_detr_amd import ops
    assert B > 64 or B * Q * 4 > 160 * 1024 - 4096
    plan = ops.MatchPlan([1] * B, Q, DEV)
    z = torch.zeros((B, 1), dtype=torch.int64, device=DEV)
    args = (torch.zeros(B, Q, 2, device=DEV), torch.full((B, Q, 4), 0.5, device=DEV), torch.ones(B, Q, 2, device=DEV),
            torch.full((B, 4), 0.5, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV), plan, z, z.clone(),
            torch.full((1,), float(B), device=DEV), 1, R.ALPHA, torch.tensor(R.W6, device=DEV))
    with pytest.raises(RuntimeError, match=msg):
        ops.CriterionFn.apply(*args)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- match cost + assignment
def device_cost(mc, canary=None):
    """(flat cost on the CPU, plan) of ops.match_cost; with `canary`: the same launch into a canary-filled, 256 elements longer buffer."""
    from counting_detr_amd import ops
    from counting_detr_amd._ffi import check, lib, ptr, stream_ptr
    plan = ops.MatchPlan(list(mc.sizes), R.MATCH_Q, DEV)
    logits, boxes = mc.logits.to(DEV).contiguous(), mc.boxes.to(DEV).contiguous()
    tgt = torch.cat(mc.tgt).reshape(-1, 4).to(DEV).contiguous()
    if canary is None:
        cost = ops.match_cost(logits, boxes, tgt, plan)
    else:
        cost = torch.full((plan.cost_numel + 256,), canary, device=DEV, dtype=torch.float32)
        check(lib().cdetr_match_cost(ptr(logits), 2, ptr(boxes), ptr(tgt), ptr(plan.tgt_off), ptr(plan.cost_off), plan.B, plan.Q, 2.0, 5.0, 2.0,
                                     ptr(cost), stream_ptr()), "cdetr_match_cost")
    torch.cuda.synchronize()
    return cost, plan


@match_param
def test_match_cost_inside_the_bracket_and_vs_fp64(launch, table):
    mc = R.match_case(launch, table)
    cost, plan = device_cost(mc)
    flat_cost = cost.cpu()
    assert bool(torch.isfinite(flat_cost[:sum(R.MATCH_Q * t for t in mc.sizes)]).all())
    failed = []
    for b, T in enumerate(mc.sizes):
        blk = R.undo_layout(flat_cost, plan.cost_off_host, b, R.MATCH_Q, T)
        c32 = R.match_oracle(mc, b)
        lo, hi = R.match_bracket(mc, b)
        widen = R.EXISTING["cost"] * (1 + c32.abs())
        outside = (blk < lo - widen) | (blk > hi + widen)
        over = torch.maximum(lo - widen - blk, blk - hi - widen).clamp(min=0)
        print(f"EDGE cost {mc.name} image {b} T {T}: outside the +-2 ulp bracket {int(outside.sum())} of {blk.numel()}, by at most "
              f"{float(over.max()) if T else 0.0:.2e}; bracket up to {float((hi - lo).max()) if T else 0.0:.2e} wide; off the fp32 oracle by at most "
              f"{float((blk - c32).abs().max()) if T else 0.0:.2e} in {int((blk != c32).sum())} entries")
        if bool(outside.any()):
            q = int(outside.any(1).nonzero()[0])
            failed.append(f"image {b}: {int(outside.sum())} entries outside, first at logit {float(mc.logits[b, q, 0]):.3f}")
        fl = R.cost_floor(mc, b)
        e, bar = R.cost_err(mc, b, blk), R.bar(R.EXISTING["cost"], fl)
        print(f"EDGE cost {mc.name} image {b} fp64 on {int(R.well_rows(mc, b).sum())} rows: floor {fl:.2e} bar {bar:.2e} measured {e:.2e} factor 8")
        if not e <= bar:
            failed.append(f"image {b}: fp64 {e:.3e} > {bar:.3e}")
        q, q2 = mc.dup_q                                                   # identical predictions: identical rows, bit for bit
        assert torch.equal(blk[q], blk[q2])
        if b in mc.dup_t:
            assert torch.equal(blk[:, mc.dup_t[b][0]], blk[:, mc.dup_t[b][1]])
    assert not failed, "; ".join(failed)
    guarded, _ = device_cost(mc, canary=12345.0)                           # the T == 0 image and the last block write nothing outside their slots
    guarded = guarded.cpu()
    n = sum(R.MATCH_Q * t for t in mc.sizes)
    assert plan.cost_off_host[-1] == n and torch.equal(guarded[:n], flat_cost[:n])
    assert bool((guarded[n:] == 12345.0).all())
    for b, T in enumerate(mc.sizes):
        if T == 0:
            assert plan.cost_off_host[b] == plan.cost_off_host[b + 1]


@match_param
def test_lsap_on_the_device_cost_with_duplicate_targets(launch, table):
    from scipy.optimize import linear_sum_assignment
    from counting_detr_amd import ops
    from oracle import criterion as OC
    mc = R.match_case(launch, table)
    cost, plan = device_cost(mc)
    idx_i, idx_j, status = ops.lsap(cost, plan)
    torch.cuda.synchronize()
    assert status.tolist() == [0] * plan.B
    flat_cost, idx_i, idx_j = cost.cpu(), idx_i.cpu(), idx_j.cpu()
    oracle = OC.hungarian_match({"pred_logits": mc.logits, "pred_boxes": mc.boxes}, [{"boxes": t} for t in mc.tgt]) if table == "pinned" else None
    for b, T in enumerate(mc.sizes):
        m = min(R.MATCH_Q, T)
        if m == 0:
            continue
        blk = R.undo_layout(flat_cost, plan.cost_off_host, b, R.MATCH_Q, T).contiguous().numpy()
        ri, ci = linear_sum_assignment(blk)                                # the same downloaded bits
        assert np.array_equal(idx_i[b, :m].numpy(), ri) and np.array_equal(idx_j[b, :m].numpy(), ci), f"image {b}"
        if oracle is not None:                                             # decided by more than the bracket widths (the CPU test): the oracle's own
            want = R.canonical(oracle[b][0], oracle[b][1], mc.dup_q, mc.dup_t.get(b))
            assert R.canonical(ri, ci, mc.dup_q, mc.dup_t.get(b)) == want, f"image {b}"
