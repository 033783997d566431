"""The trainers' wiring around the fused optimizer kernels -- the arena's order, the per-element learning rates and their collapse to
(lr0, lr1, split), the StepLR factor, the parameters left out, the torch-layout checkpoint -- against clip_grad_norm_ + torch.optim.AdamW /
SGD + StepLR over the reference's own three parameter groups, on fp64 CPU clones of every parameter.  Needs an MI355X.

The network never runs: seeded gradients are written into the trainer's flat gradient arena (every p.grad is a view of it) and
`_optimizer_step()` is called.  Five free-running steps crossing one lr drop, then a checkpoint round trip and a sixth step.  Every
parameter is compared by name, over all of its elements: the displacement (p - p_start) / base lr and the optimizer state, as max |error|
of the parameter against bar x max |reference| of its learning-rate group, where the bar is 4 x the error of a float32 restatement of the
reference that runs beside it (optimizer_arenas.bar: the method of test_adamw_kernel_gpu.py; per group, because one ulp of p is ten times
as many lr in the backbone group).  An MI355X run, kernel / restatement, worst lr group: displacement after five steps 7.8e-5 / 1.3e-4
(lr 1e-2; 6.2e-3 / 6.2e-3 at the shipped lr 1e-4, where half an ulp of p is that share of five steps), exp_avg 3.1e-7 / 2.4e-7, exp_avg_sq
1.28e-5 / 1.34e-5 (the float cast of beta2, see test_adamw_kernel_gpu.py), SGD's momentum_buffer 1.4e-7 / 1.5e-7; the step after the
round trip 7.3e-4 / 1.2e-3 (lr 1e-2 x 0.1) and 5.9e-2 / 5.9e-2 (lr 1e-5 x 0.1 = 1e-6 a step).  The file takes 45 s, of which the CPU side
(torch's fp64 steps and the restatement over all 37.4 M elements) is nearly all: nothing is sampled.
"""
import copy
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from optimizer_arenas import adamw_ref32, bar, g

pytestmark = pytest.mark.gpu
DEV = "cuda"
MOMENTUM = 0.9
STEPS, LR_DROP = 5, 3                        # StepLR's factor is 1 for steps 1-3 and 0.1 from step 4 on
# gradient scales: the norm is scale sqrt(37.4 M) = 6100 scale, so clip_grad_norm_(0.1) is active at 3e-2 and inactive at 1e-5
SCALES = [3e-2, 1e-5, 3e-2, 1e-5, 3e-2, 1e-5]

GROUPINGS = {
    # the shipped arguments: [everything else | backbone], one change of lr at a multiple of 4 -> no table
    "shipped_groups": dict(),
    # a third group in the middle of the arena: lr | 0.1 lr | lr | lr_backbone -> the per-element table
    "three_groups": dict(lr_linear_proj_names=["decoder_layers.2."]),
    # one change of lr, at the first element of transformer.bbox_embed (behind transformer.cls_embed.0.bias, 2 elements: offset % 4 == 2)
    "odd_split": dict(lr_backbone_names=["backbone", "bbox_embed", "bbox_variance", "aggr_input_proj"]),
}
HYPER = {"shipped_hp": dict(), "visible_decay": dict(lr=1e-2, lr_backbone=1e-3, weight_decay=0.1)}


def build_stage2():
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from oracle.weights import model_schema, seeded_state_dict
    args = default_args(device=DEV)
    model, crit, _ = counting_detr_amd.build_model(args)
    model.load_state_dict(seeded_state_dict(model_schema()), strict=True)
    return model.to(DEV).train(), crit, args


def build_stage1():
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    from oracle.weights import seeded_state_dict, stage1_schema
    args = get_args_parser_stage1().parse_args([])
    args.device = DEV
    model, crit, _ = stage1.build(args)
    model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True)
    return model.to(DEV).train(), crit, args


class Pair:
    """Two copies of a model, built once per module (the network never runs; a trainer only re-homes the parameters in its arena), the
    seeded weights to start every case from, and the arguments to copy."""

    def __init__(self, build):
        (self.model, self.crit, self.args), (self.model2, self.crit2, _) = build(), build()
        self.start = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}

    def case_args(self, **kw):
        args = copy.copy(self.args)
        for k, v in kw.items():
            setattr(args, k, v)
        return args


@pytest.fixture(scope="module")
def stage2_pair():
    return Pair(build_stage2)


@pytest.fixture(scope="module")
def stage1_pair():
    return Pair(build_stage1)


def reference_groups(model, args):
    """The reference's optimizer groups (its main.py: param_dicts): names of [neither | lr_backbone_names | lr_linear_proj_names] over
    named_parameters(), requires_grad only, with lr, lr_backbone, lr * lr_linear_proj_mult."""
    def match(n, keys):
        return any(k in n for k in keys)
    named = [n for n, p in model.named_parameters() if p.requires_grad]
    return ([[n for n in named if not match(n, args.lr_backbone_names) and not match(n, args.lr_linear_proj_names)],
             [n for n in named if match(n, args.lr_backbone_names)],
             [n for n in named if match(n, args.lr_linear_proj_names)]],
            [args.lr, args.lr_backbone, args.lr * args.lr_linear_proj_mult])


def storage_perm(p):
    """The order of p's dimensions in memory, slowest first: a parameter occupies its slice of the arena in its own memory order, and the
    channels_last convolution weights' is not the order of reshape(-1)."""
    return sorted(range(p.dim()), key=lambda d: (-p.stride(d), d))


def in_storage_order(t, perm):
    return t.permute(perm).reshape(-1)


def from_storage_order(flat, shape, perm):
    return flat.view([shape[d] for d in perm]).permute([perm.index(d) for d in range(len(perm))])


class TorchSide:
    """fp64 CPU clones of the model's parameters under the reference's optimizer and scheduler."""

    def __init__(self, model, args, groups, lrs, sgd):
        self.args, self.names = args, [n for grp in groups for n in grp]
        params = dict(model.named_parameters())
        self.p = {n: torch.nn.Parameter(params[n].detach().double().cpu().clone()) for n in self.names}
        self.perm = {n: storage_perm(params[n]) for n in self.names}
        dicts = [{"params": [self.p[n] for n in grp], "lr": lr} for grp, lr in zip(groups, lrs)]
        if sgd:
            self.opt = torch.optim.SGD(dicts, lr=args.lr, momentum=MOMENTUM, weight_decay=args.weight_decay)
        else:
            self.opt = torch.optim.AdamW(dicts, lr=args.lr, weight_decay=args.weight_decay)
        self.sched = torch.optim.lr_scheduler.StepLR(self.opt, args.lr_drop)

    def step(self, grad_flat, offsets):
        """One step on the gradient arena's contents; parameters outside the arena have no gradient, as in the reference.  Returns
        clip_grad_norm_'s norm."""
        for n, p in self.p.items():
            p.grad = None
            if n in offsets:
                off, sz = offsets[n]
                p.grad = from_storage_order(grad_flat[off:off + sz].double(), p.shape, self.perm[n]).clone()
        tn = torch.nn.utils.clip_grad_norm_([p for p in self.p.values() if p.grad is not None], self.args.clip_max_norm)
        self.opt.step()
        return float(tn)

    def flat(self, offsets, total, key=None):
        """The parameters (key None) or one entry of the optimizer state in the arena's order, fp64 NumPy."""
        out = np.zeros(total, np.float64)
        for n, (off, sz) in offsets.items():
            t = self.p[n].detach() if key is None else self.opt.state[self.p[n]][key]
            out[off:off + sz] = in_storage_order(t, self.perm[n]).numpy()
        return out


def sgd_ref32(p, gr, buf, lr, s, max_norm, wd):
    """clip_grad_norm_ + torch.optim.SGD(momentum, dampening 0, coupled weight decay) in float32 NumPy, torch's operation order."""
    f = np.float32
    norm = f(np.sqrt(np.sum(gr * gr, dtype=np.float32)))
    coef = f(min(f(f(max_norm) / f(norm + f(1e-6))), f(1.0))) if max_norm > 0 else f(1.0)
    d = gr * coef + f(wd) * p
    buf = f(MOMENTUM) * buf + d
    return p - (lr * f(s)) * buf, buf


def compare(tag, names, offsets, group_of, triples, figures):
    """triples: (quantity, kernel, restatement, reference) flat fp64 arrays in the arena's order.  Per learning-rate group: the
    restatement's max error over the group's max |reference| gives the bar; every parameter's max |kernel - reference| over all of its
    elements is held to bar x that scale."""
    order = sorted(names, key=lambda n: offsets[n][0])
    starts = np.array([offsets[n][0] for n in order])
    grp = np.array([group_of[n] for n in order])
    for qname, k, y, r in triples:
        per_param = lambda x: np.maximum.reduceat(np.abs(x, out=x), starts)      # noqa: E731  (the arena is the parameters back to back)
        ek, ey, ar = per_param(k - r), per_param(y - r), per_param(r.copy())
        for gi in np.unique(grp):
            sel = grp == gi
            yerr, scale = float(ey[sel].max()), float(ar[sel].max()) + 1e-300
            assert yerr <= 0.1 * scale, f"{tag}: {qname}, lr group {gi}: ill-posed, float32 itself is {yerr / scale:.2e} off: no bar can be taken from it"
            figures.append(f"{tag} {qname} group {gi}: kernel {ek[sel].max() / scale:.2e} restatement {yerr / scale:.2e}")
            for n, e in zip(np.array(order)[sel], ek[sel]):
                assert e <= bar(yerr / scale) * scale, (f"{tag}: {qname} of {n} (lr group {gi}): max error {e / scale:.3e} of the group's scale, "
                                                        f"the float32 restatement {yerr / scale:.3e}, bar {bar(yerr / scale):.3e}")


def inject(tr, seed, scale):
    gr = torch.randn(tr.flat_g.numel(), generator=g(seed)) * scale
    tr.flat_g.copy_(gr.to(tr.flat_g.device))
    return gr


def run_case(pair, trainer_cls, sgd, grouping, hyper):
    from counting_detr_amd import engine
    kw = dict(GROUPINGS[grouping], **HYPER[hyper], lr_drop=LR_DROP, sgd=sgd)
    model, crit, args = pair.model, pair.crit, pair.case_args(**kw)
    model.load_state_dict(pair.start, strict=True)
    tr = getattr(engine, trainer_cls)(model, crit, args, device=DEV)
    total = tr.flat_p.numel()
    params = dict(model.named_parameters())

    # --- the arena: every trainable parameter the loss reaches, once, contiguous, a view of flat_p; the rest outside and untouched
    left_out = tuple(tr.unused_prefixes)
    expect_in = [n for n, p in params.items() if p.requires_grad and not n.startswith(left_out)]
    assert sorted(tr.offsets) == sorted(expect_in)
    if trainer_cls == "Stage1Trainer":
        assert any(n.startswith("transformer.cls_embed.") for n in params) and not any(n.startswith("transformer.cls_embed.") for n in tr.offsets)
    spans = sorted(tr.offsets.values())
    assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == total
    for n, (off, sz) in tr.offsets.items():
        assert params[n].numel() == sz and params[n].data_ptr() == tr.flat_p.data_ptr() + 4 * off, n
        assert params[n].grad.data_ptr() == tr.flat_g.data_ptr() + 4 * off and params[n].grad.stride() == params[n].stride(), n
        lin = in_storage_order(params[n].detach(), storage_perm(params[n]))      # dense: its elements in memory order ARE the slice
        assert lin.data_ptr() == params[n].data_ptr() and lin.is_contiguous(), n
    outside0 = {n: p.detach().clone() for n, p in params.items() if n not in tr.offsets}
    assert any(not p.requires_grad for p in params.values()) and any(n.startswith(left_out) for n in outside0)

    # --- the groups: the test's own, from the reference's rule; the trainer's must equal them
    groups, lrs = reference_groups(model, args)
    t_groups, t_lrs = tr._torch_param_order()
    assert t_groups == groups and list(t_lrs) == list(lrs)
    group_of = {n: gi for gi, grp in enumerate(groups) for n in grp}
    lr_el = np.zeros(total, np.float64)
    for n, (off, sz) in tr.offsets.items():
        lr_el[off:off + sz] = lrs[group_of[n]]
    change = np.flatnonzero(lr_el[1:] != lr_el[:-1]) + 1
    if grouping == "shipped_groups":
        first_bb = min(off for n, (off, sz) in tr.offsets.items() if "backbone" in n)
        assert tr._lr_two is not None and tr._lr_two[2] == first_bb == int(change[0]) and len(change) == 1
        assert tr._lr_two[0] == float(np.float32(args.lr)) and tr._lr_two[1] == float(np.float32(args.lr_backbone))
    elif grouping == "three_groups":
        assert tr._lr_two is None and len(change) == 3 and len(groups[2]) > 0
    else:
        assert tr._lr_two is None and len(change) == 1 and int(change[0]) % 4 != 0
    assert np.array_equal(tr.lr_vec.cpu().numpy(), lr_el.astype(np.float32))

    ref = TorchSide(model, args, groups, lrs, sgd)
    names = list(tr.offsets)
    p_start = tr.flat_p.cpu().numpy().astype(np.float64)
    lr32 = lr_el.astype(np.float32)
    yp = tr.flat_p.cpu().numpy().copy()                                  # the free-running float32 restatement
    ya, yb = np.zeros(total, np.float32), np.zeros(total, np.float32)
    figures = []
    wd, max_norm = args.weight_decay, args.clip_max_norm

    def yard_step(yp, ya, yb, gr, s, t):
        if sgd:
            p, buf = sgd_ref32(yp, gr, ya, lr32, s, max_norm, wd)
            return p, buf, yb
        p, m, v, _ = adamw_ref32(yp, gr, ya, yb, lr32, s, t, max_norm, wd)
        return p, m, v

    def state_triples(tr, ref, ya, yb):
        if sgd:
            return [("momentum_buffer", tr.momentum_buffer.cpu().numpy().astype(np.float64), ya, ref.flat(tr.offsets, total, "momentum_buffer"))]
        return [("exp_avg", tr.exp_avg.cpu().numpy().astype(np.float64), ya, ref.flat(tr.offsets, total, "exp_avg")),
                ("exp_avg_sq", tr.exp_avg_sq.cpu().numpy().astype(np.float64), yb, ref.flat(tr.offsets, total, "exp_avg_sq"))]

    pool = ThreadPoolExecutor(1)                                         # the restatement (NumPy, one thread) runs beside torch's fp64 step
    for i in range(STEPS):
        s = 0.1 ** (i // LR_DROP)
        gr = inject(tr, 1000 + i, SCALES[i])
        yard = pool.submit(yard_step, yp, ya, yb, gr.numpy(), np.float32(s), i + 1)
        tr._optimizer_step()
        torch.cuda.synchronize()
        tn = ref.step(gr, tr.offsets)
        yp, ya, yb = yard.result()
        st = tr.opt_state.cpu().tolist()
        assert st[0] == i + 1 and st[1] == float(np.float32(s)) and st[3] == 0.0 and abs(st[2] - tn) <= 1e-5 * tn, (i, st, tn)
        tr.lr_scheduler_step()
        ref.sched.step()
        if i == STEPS - 1:                                               # three steps at factor 1 and two at 0.1 behind it: everything, by name
            disp = lambda p: (np.asarray(p, np.float64) - p_start) / lr_el      # noqa: E731
            r = disp(ref.flat(tr.offsets, total))
            if not sgd:                                                  # an Adam term of at most 3 lr per step, plus the decay of the largest weight
                assert np.abs(r).max() <= (i + 1) * (3.0 + 2.0 * wd * np.abs(p_start).max()), "ill-posed: steps no Adam trajectory takes"
            compare(f"step {i + 1}", names, tr.offsets, group_of,
                    [("displacement", disp(tr.flat_p.cpu().numpy()), disp(yp), r)] + state_triples(tr, ref, ya, yb), figures)
    assert abs(float(tr.opt_state[1]) - 0.1) < 1e-8 and tr.epoch == STEPS

    # --- parameters outside the arena: bit-unchanged; no optimizer state for them
    for n, p0 in outside0.items():
        assert torch.equal(params[n].detach(), p0), n
    sd, ls = tr.state_dict(), tr.lr_scheduler_state_dict()
    flat_names = [n for grp in groups for n in grp]
    for idx, n in enumerate(flat_names):
        assert (idx in sd["state"]) == (n in tr.offsets), n

    # --- round trip: a fresh trainer and a real torch optimizer + StepLR load the checkpoint entries; a sixth step on all three
    model2 = pair.model2
    model2.load_state_dict(model.state_dict(), strict=True)
    tr2 = getattr(engine, trainer_cls)(model2, pair.crit2, pair.case_args(**kw), device=DEV)
    tr2.load_state_dict(sd, lr_scheduler=ls)
    assert torch.equal(tr2.flat_p, tr.flat_p) and tr2.epoch == tr.epoch
    ref2 = TorchSide(model, args, groups, lrs, sgd)                     # fp64 clones of the kernel's current parameters
    ref2.opt.load_state_dict(sd)
    ref2.sched.load_state_dict({k: v for k, v in ls.items() if k in ref2.sched.state_dict()})
    p5 = tr.flat_p.cpu().numpy().copy()
    if sgd:
        a5, b5 = tr.momentum_buffer.cpu().numpy().copy(), np.zeros(total, np.float32)
    else:
        a5, b5 = tr.exp_avg.cpu().numpy().copy(), tr.exp_avg_sq.cpu().numpy().copy()
    gr = inject(tr, 1000 + STEPS, SCALES[STEPS])
    s = 0.1 ** (STEPS // LR_DROP)
    yard = pool.submit(yard_step, p5, a5, b5, gr.numpy(), np.float32(s), STEPS + 1)
    tr2.flat_g.copy_(tr.flat_g)
    for t in (tr, tr2):
        t._optimizer_step()
    torch.cuda.synchronize()
    tn = ref2.step(gr, tr.offsets)
    assert torch.equal(tr2.flat_p, tr.flat_p)                            # the restored trainer takes the very same step
    if sgd:
        assert torch.equal(tr2.momentum_buffer, tr.momentum_buffer)
    else:
        assert torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq)
        assert float(tr2.opt_state[0]) == float(tr.opt_state[0]) == STEPS + 1
    assert float(tr2.opt_state[1]) == float(tr.opt_state[1]) and abs(float(tr2.opt_state[2]) - tn) <= 1e-5 * tn
    y6 = yard.result()
    pool.shutdown()
    upd = lambda p: (np.asarray(p, np.float64) - p5.astype(np.float64)) / (lr_el * s)      # noqa: E731
    compare("after the round trip", names, tr.offsets, group_of,
            [("update", upd(tr2.flat_p.cpu().numpy()), upd(y6[0]), upd(ref2.flat(tr.offsets, total)))] + state_triples(tr2, ref2, y6[1], y6[2]),
            figures)
    print("\nFIG " + "\nFIG ".join(figures))


# --sgd only with lr 1e-2: at the shipped lr 1e-4 a clipped gradient (0.1 / sqrt(37.4 M) = 1.6e-5 an element) moves p by 1e-9 a step, below
# one fp32 ulp of a 0.1 weight -- p stays put in float32, torch's float32 SGD included, and there is no displacement to compare
CASES = [("adamw", "shipped_groups", "shipped_hp"), ("adamw", "shipped_groups", "visible_decay"), ("adamw", "three_groups", "visible_decay"),
         ("adamw", "odd_split", "shipped_hp"), ("sgd", "shipped_groups", "visible_decay"), ("sgd", "three_groups", "visible_decay")]


@pytest.mark.parametrize("optimizer,grouping,hyper", CASES, ids=["-".join(c) for c in CASES])
def test_trainer_steps_equal_torch(stage2_pair, optimizer, grouping, hyper):
    run_case(stage2_pair, "Trainer", optimizer == "sgd", grouping, hyper)


def test_stage1_trainer_steps_equal_torch(stage1_pair):
    """The same for Stage1Trainer (AdamW only), three lr groups; transformer.cls_embed.* stays out of the arena, bit-unchanged and without
    optimizer state (run_case)."""
    run_case(stage1_pair, "Stage1Trainer", False, "three_groups", "visible_decay")
