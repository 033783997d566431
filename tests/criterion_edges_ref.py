"""Case tables, fp64 references, fp32 floors and mutants for the stage-2 loss path (csrc/matcher.hip match_cost_kernel, csrc/criterion.hip,
csrc/criterion_eval.hip) at the branches random inputs never reach.  No GPU needed; shared by tests/test_criterion_edges_cpu.py and
tests/test_criterion_edges_gpu.py.

  * Every box coordinate is dyadic (a multiple of 1/64, widths and heights >= 1/64), so cxcywh -> xyxy is exact in fp32 and in fp64 and a
    tie in one precision is a tie in the other; no box and no enclosing box has zero area.
  * CASES: named SetCriterion inputs with HAND-MADE matched indices (idx_i ascending per image, as the solver returns them), so the loss
    kernels are tested independently of the solver.  device_indices() pads slots m >= M_b with the valid but wrong pair (Q - 1, 0): a
    kernel that read them would give wrong numbers, not an out-of-bounds access.
  * reference / reference_per_image: oracle.criterion.set_criterion in fp64 on the case's indices (the whole batch / image b alone with
    num_boxes = max(T_b, 1), the contract of criterion_eval.hip); the gradients of each differentiable loss separately.
  * floor / floor_per_image: the same calls in fp32 on the CPU, measured against fp64.  bar(existing, floor) = min(existing, max(8 x floor,
    2^-21)): the kernel sums in another order (256 strided threads, a shuffle tree, four waves) and calls the device's expf / logf / log1pf,
    both a few ulp like the floor itself; 2^-21 covers exact dyadic cases whose floor is 0.  A bar never comes from a kernel's output.
  * err(): max|a - r| / max|r| per tensor; d_vars, whose entries span 1/v^2 over more than three decades, elementwise as
    max |a - r| / (|r| + 1e-6 max|r|).
  * closed_form(case, **switches): the losses and gradients restated in plain fp64 without autograd; each switch of MUTANTS turns on one
    plausible kernel mistake.  CATCHES lists which case and tensor tells each mutant from the right kernel.
  * MATCH_LAUNCHES / match_case: match-cost inputs (T < Q, T == Q, T > Q and T == 0 in one launch, duplicate targets and predictions) under
    three logit tables.  The class cost 0.75 p^2 (-log(1 - p + 1e-8)) is ill-conditioned in fp32 between logits ~2.4 and 20: there
    match_bracket() evaluates the fp32 oracle at p moved by +-2 ulp, which brackets any sigmoid within 2 ulp of torch's."""
import functools
from dataclasses import dataclass, field

import torch

from oracle import criterion as OC

SCALARS = ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "loss_variance", "total")
EXACT = ("class_error", "cardinality_error")                  # whole-number statistics: compared exactly
GRADS = ("d_logits/ce", "d_boxes/bbox", "d_boxes/giou", "d_boxes/var", "d_vars/var")
GRAD_OF = {"d_logits/ce": ("loss_ce", 0), "d_boxes/bbox": ("loss_bbox", 1), "d_boxes/giou": ("loss_giou", 1), "d_boxes/var": ("loss_variance", 1),
           "d_vars/var": ("loss_variance", 2)}               # tensor -> (loss, index into (logits, boxes, vars))
ORDER6 = SCALARS[:6]                                          # the kernel's vec
W6 = tuple(float(OC.WEIGHT_DICT.get(k, 0.0)) for k in ORDER6)
EXISTING = {"scalar": 1e-4, "grad": 2e-4, "cost": 2e-6}      # the bars of test_criterion_golden / test_match_cost_values
ALPHA = 0.25
FACTOR = 8.0
FLOOR_MIN = 2.0 ** -21


def g(seed):
    return torch.Generator().manual_seed(seed)


def u64(*rows):
    """Boxes given in units of 1/64 -> fp32 (exact)."""
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4) / 64.0


def rand_boxes(n, gen):
    """Dyadic cxcywh boxes inside the unit square: centres in [16, 48] / 64, sides in [2, 24] / 64."""
    c = torch.randint(16, 49, (n, 2), generator=gen)
    s = torch.randint(2, 25, (n, 2), generator=gen)
    return torch.cat([c, s], 1).float() / 64.0


# ----------------------------------------------------------------------------------------------------- criterion cases
@dataclass
class Case:
    name: str
    logits: torch.Tensor          # [B, Q, C] fp32
    boxes: torch.Tensor           # [B, Q, 4] fp32 cxcywh
    vars: torch.Tensor            # [B, Q, 2] fp32, positive
    tgt_boxes: list               # [T_b, 4] fp32 per image
    tgt_labels: list              # [T_b] int64 per image
    idx: list                     # (idx_i, idx_j) int64 per image, idx_i ascending, len = min(Q, T_b)
    num_classes: int = 1
    marks: dict = field(default_factory=dict)     # edge -> [(b, k)]: pair k of image b carries it (or (b, q) for query rows)

    @property
    def sizes(self):
        return tuple(int(t.shape[0]) for t in self.tgt_boxes)

    @property
    def B(self):
        return self.logits.shape[0]

    @property
    def Q(self):
        return self.logits.shape[1]

    def pair(self, b, k):
        """(predicted box, target box) of pair k of image b."""
        return self.boxes[b, self.idx[b][0][k]], self.tgt_boxes[b][self.idx[b][1][k]]

    def set_pair(self, b, k, pred, tgt, mark=None):
        self.boxes[b, self.idx[b][0][k]] = u64(pred)[0]
        self.tgt_boxes[b][self.idx[b][1][k]] = u64(tgt)[0]
        if mark:
            self.marks.setdefault(mark, []).append((b, k))

    def unmatched(self, b):
        m = set(self.idx[b][0].tolist())
        return [q for q in range(self.Q) if q not in m]


def base_case(name, B, Q, T, seed, C=2, num_classes=1, all_queries=False):
    gen = g(seed)
    logits = torch.randn(B, Q, C, generator=gen) * 1.5
    boxes = rand_boxes(B * Q, gen).reshape(B, Q, 4)
    pvars = 0.5 + torch.rand(B, Q, 2, generator=gen)
    tb = [rand_boxes(t, gen) for t in T]
    tl = [torch.randint(0, num_classes, (t,), generator=gen) for t in T]
    idx = []
    for t in T:
        m = min(Q, t)
        ii = torch.arange(Q) if (all_queries or m == Q) else torch.randperm(Q, generator=gen)[:m].sort().values
        idx.append((ii.to(torch.int64), torch.randperm(t, generator=gen)[:m].to(torch.int64)))
    return Case(name, logits, boxes, pvars, tb, tl, idx, num_classes)


SAT = (-100.0, -88.0, -30.0, -20.0, 0.0, 17.0, 20.0, 30.0, 88.0, 100.0)
TIES = ((2.0, 2.0), (-1.0, -1.0), (40.0, 40.0))
VAR_EDGES = (1.0, 0.01, 30.0, 0.05)


def _identical():
    c = base_case("identical", 1, 24, (7,), 101)
    for k, bx in enumerate(((32, 32, 16, 12), (20, 40, 6, 6), (45, 21, 3, 9))):
        c.set_pair(0, k, bx, bx, "identical")
    return c


def _shared_edge():
    c = base_case("shared_edge", 2, 24, (6, 5), 102)
    c.set_pair(0, 0, (38, 33, 12, 8), (24, 32, 16, 12), "touch_x")        # prediction starts where the target ends: x1 == u2
    c.set_pair(0, 1, (26, 33, 12, 8), (40, 32, 16, 12), "touch_x")        # prediction ends where the target starts: x2 == u1
    c.set_pair(1, 0, (33, 38, 8, 12), (32, 24, 12, 16), "touch_y")
    c.set_pair(1, 1, (33, 26, 8, 12), (32, 40, 12, 16), "touch_y")
    return c


def _concentric():
    c = base_case("concentric", 1, 40, (9,), 103)
    c.set_pair(0, 0, (32, 32, 10, 6), (32, 32, 24, 20), "concentric")     # prediction inside the target
    c.set_pair(0, 1, (30, 30, 20, 22), (30, 30, 6, 6), "concentric")      # target inside the prediction
    return c


def _same_cx_w():
    c = base_case("same_cx_w", 2, 40, (8, 3), 104)
    c.set_pair(0, 0, (32, 30, 12, 14), (32, 24, 12, 10), "same_cx_w")
    c.set_pair(1, 0, (20, 40, 6, 8), (20, 30, 6, 16), "same_cx_w")
    return c


def _disjoint():
    c = base_case("disjoint", 3, 24, (5, 4, 6), 105)
    c.set_pair(0, 0, (54, 54, 6, 6), (10, 10, 4, 4), "disjoint")
    c.set_pair(2, 0, (8, 56, 4, 8), (58, 6, 6, 4), "disjoint")
    return c


def _tiny():
    c = base_case("tiny", 2, 24, (6, 4), 106)
    c.set_pair(0, 0, (30, 30, 1, 1), (32, 32, 40, 36), "tiny")            # inside the target
    c.set_pair(0, 1, (61, 5, 1, 1), (30, 34, 36, 40), "tiny")             # outside it
    c.set_pair(1, 0, (32, 32, 40, 36), (30, 30, 1, 1), "tiny")            # a large prediction on a tiny target
    return c


def _logit_sat():
    c = base_case("logit_sat", 2, 40, (12, 11), 107)
    for k, x in enumerate(SAT):                                            # matched rows: class 0 (the target) / class 1 saturated
        c.logits[0, c.idx[0][0][k], 0] = x
        c.logits[1, c.idx[1][0][k], 1] = x
    for k, x in enumerate(SAT):                                            # unmatched rows: both classes
        c.logits[0, c.unmatched(0)[k]] = torch.tensor([x, SAT[(k + 3) % len(SAT)]])
    c.marks["sat_matched"] = [(0, k) for k in range(len(SAT))] + [(1, k) for k in range(len(SAT))]
    c.marks["sat_unmatched"] = [(0, q) for q in c.unmatched(0)[:len(SAT)]]
    c.marks["tie_matched"], c.marks["tie_unmatched"] = [], []
    for k, pair in enumerate(TIES[:2]):
        c.logits[0, c.idx[0][0][10 + k]] = torch.tensor(pair)
        c.marks["tie_matched"].append((0, 10 + k))
    c.logits[1, c.idx[1][0][10]] = torch.tensor(TIES[2])
    c.marks["tie_matched"].append((1, 10))
    for k, pair in enumerate(TIES):
        q = c.unmatched(1)[k]
        c.logits[1, q] = torch.tensor(pair)
        c.marks["tie_unmatched"].append((1, q))
    return c


def _var_edges():
    c = base_case("var_edges", 2, 24, (6, 5), 108)
    for b in range(2):
        for k in range(len(c.idx[b][0])):
            q = c.idx[b][0][k]
            c.vars[b, q, 0] = VAR_EDGES[(k + b) % 4]
            c.vars[b, q, 1] = VAR_EDGES[(k + b + 1) % 4]
    return c


def _t_gt_q():
    return base_case("t_gt_q", 2, 24, (29, 3), 109)


def _t_mixed():
    return base_case("t_mixed", 3, 24, (9, 0, 1), 110)


def _t_none():
    return base_case("t_none", 2, 24, (0, 0), 111)


def _c3():
    c = base_case("c3", 2, 40, (10, 7), 112, C=3, num_classes=3)
    c.tgt_labels[0][:3] = torch.tensor([0, 1, 2])
    return c


_BUILDERS = {f.__name__[1:]: f for f in (_identical, _shared_edge, _concentric, _same_cx_w, _disjoint, _tiny, _logit_sat, _var_edges, _t_gt_q,
                                         _t_mixed, _t_none, _c3)}
CASES = tuple(_BUILDERS)
# launch sizes of cdetr_criterion_fwd: the largest B; 51 200 B of dynamic LDS, the first size past 48 KiB; 158 400 B; and 159 744 B, exactly the
# 160 KiB - 4096 the argument check admits
SIZE_CASES = ((64, 24), (16, 800), (44, 900), (64, 624))


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case; tensors are shared between callers and must not be written."""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def size_case(B, Q):
    """Random dyadic inputs at a launch-size edge of cdetr_criterion_fwd; 0 ... 9 targets per image keep the reference small."""
    gen = g(1000 + B + Q)
    T = torch.randint(0, 10, (B,), generator=gen).tolist()
    T[0], T[-1] = 9, 5                                        # the first and the last image have pairs
    return base_case(f"size_b{B}_q{Q}", B, Q, tuple(T), 2000 + B + Q)


def device_indices(c):
    """(idx_i, idx_j) int64 [B, Mmax] as ops.lsap lays them out; slots m >= M_b hold the valid but wrong pair (Q - 1, 0)."""
    Mmax = max(max(len(i) for i, _ in c.idx), 1)
    ii = torch.full((c.B, Mmax), c.Q - 1, dtype=torch.int64)
    jj = torch.zeros((c.B, Mmax), dtype=torch.int64)
    for b, (i, j) in enumerate(c.idx):
        ii[b, :len(i)], jj[b, :len(j)] = i, j
    return ii, jj


def matched_rows(c):
    """bool [B, Q]: queries with a target."""
    m = torch.zeros(c.B, c.Q, dtype=torch.bool)
    for b, (i, _) in enumerate(c.idx):
        m[b, i] = True
    return m


# ----------------------------------------------------------------------------------------------------- references
def _run(c, dtype, images=None):
    """oracle.criterion.set_criterion on the case's indices in `dtype` -> dict of SCALARS (fp64 python floats) + GRADS (tensors of `dtype`)."""
    sel = list(range(c.B)) if images is None else list(images)
    ins = [t[sel].to(dtype).clone().requires_grad_(True) for t in (c.logits, c.boxes, c.vars)]
    outs = dict(zip(("pred_logits", "pred_boxes", "pred_vars"), ins))
    tg = [{"boxes": c.tgt_boxes[b].to(dtype), "labels": c.tgt_labels[b]} for b in sel]
    losses, _ = OC.set_criterion(outs, tg, indices=[c.idx[b] for b in sel], num_classes=c.num_classes)
    res = {k: float(losses[k].detach().double()) for k in ORDER6}
    total = OC.total_loss(losses)
    res["total"] = float(total.detach().double())
    for name, (loss, which) in GRAD_OF.items():
        gr, = torch.autograd.grad(losses[loss], ins[which], retain_graph=True, allow_unused=True)
        res[name] = torch.zeros_like(ins[which]) if gr is None else gr
    gt = torch.autograd.grad(total, ins, allow_unused=True)
    res["d_total"] = tuple(torch.zeros_like(i) if x is None else x for i, x in zip(ins, gt))
    return res


@functools.lru_cache(maxsize=None)
def _reference(name, images):
    return _run(_lookup(name), torch.float64, images)


@functools.lru_cache(maxsize=None)
def _fp32(name, images):
    return _run(_lookup(name), torch.float32, images)


def _lookup(name):
    if name.startswith("size_b"):
        B, Q = name[6:].split("_q")
        return size_case(int(B), int(Q))
    return case(name)


def reference(c):
    """fp64: the six scalars, the weighted total, one gradient tensor per differentiable loss and the gradients of the total."""
    return _reference(c.name, None)


def reference_per_image(c, b):
    """fp64 scalars of image b evaluated alone (num_boxes = max(T_b, 1), variance means over its own pairs)."""
    return _reference(c.name, (b,))


def err(name, a, r):
    """The error measure of tensor `name`: a scalar's relative error, max|a - r| / max|r| of a tensor, elementwise for d_vars.  A reference
    that is exactly 0 everywhere asks for exactly 0."""
    a, r = (x.detach().double().cpu() if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float64) for x in (a, r))
    assert a.shape == r.shape, (name, a.shape, r.shape)
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    scale = float(r.abs().max()) if r.numel() else 0.0
    diff = (a - r).abs()
    if scale == 0.0:
        return 0.0 if (a.numel() == 0 or float(diff.max()) == 0.0) else float("inf")
    if name.startswith("d_vars"):
        return float((diff / (r.abs() + 1e-6 * scale)).max())
    return float(diff.max()) / scale


def existing(name):
    return EXISTING["scalar"] if name in SCALARS else EXISTING["grad"]


def _floor(name, images):
    ref, low = _reference(name, images), _fp32(name, images)
    out = {k: err(k, low[k], ref[k]) for k in SCALARS + GRADS}
    for k, i in (("d_total/logits", 0), ("d_total/boxes", 1), ("d_total/vars", 2)):
        out[k] = err("d_vars" if i == 2 else k, low["d_total"][i], ref["d_total"][i])
    return out


def floor(c):
    """tensor -> error of the fp32 CPU oracle against fp64 on this case (whole batch)."""
    return _floor(c.name, None)


def floor_per_image(c, b):
    return _floor(c.name, (b,))


def bar(existing_bar, floor_value, factor=FACTOR):
    return min(existing_bar, max(factor * floor_value, FLOOR_MIN))


# ----------------------------------------------------------------------------------------------------- closed form + mutants
MUTANTS = {
    "tie_weight": dict(tie=1.0),                      # d max(a, b) / da = [a >= b]: a tie gets 1 (and 1 again from the other side) instead of 1/2
    "clamp_strict": dict(clamp_strict=True),          # clamp(min=0) passes its gradient at > 0 only
    "sign0": dict(sign0=1.0),                         # sign(0) = 1
    "argmax_last": dict(argmax_last=True),            # the LAST maximum wins a tie
    "var_mean_per_image": dict(var_mean_per_image=True),   # mean |dw| over the image's own pairs instead of the batch's
    "nb_from_pairs": dict(nb_from_pairs=True),        # num_boxes counted from the matched pairs instead of the targets
    "unmatched_class0": dict(unmatched_class0=True),  # an unmatched query gets class 0 instead of num_classes
}
# mutant -> (case, tensor) that tells it from the right kernel by more than ten bars (asserted by tests/test_criterion_edges_cpu.py)
CATCHES = {
    "tie_weight": (("same_cx_w", "d_boxes/giou"),),       # (identical boxes cannot: their GIoU gradient is 0 under any symmetric tie weight)
    "clamp_strict": (("shared_edge", "d_boxes/giou"),),
    "sign0": (("identical", "d_boxes/bbox"), ("concentric", "d_boxes/bbox"), ("var_edges", "d_vars/var")),
    "argmax_last": (("logit_sat", "cardinality_error"), ("logit_sat", "class_error")),
    "var_mean_per_image": (("var_edges", "d_vars/var"), ("disjoint", "loss_variance"), ("tiny", "d_vars/var"), ("t_mixed", "loss_variance")),
    "nb_from_pairs": (("t_gt_q", "loss_ce"), ("t_gt_q", "d_boxes/giou")),
    "unmatched_class0": (("t_none", "loss_ce"), ("c3", "d_logits/ce"), ("logit_sat", "loss_ce")),
}


def closed_form(c, tie=0.5, clamp_strict=False, sign0=0.0, argmax_last=False, var_mean_per_image=False, nb_from_pairs=False,
                unmatched_class0=False):
    """The losses and their gradients written out in fp64, no autograd; the switches are the MUTANTS."""
    f8 = torch.float64
    lg, bx, pv = c.logits.to(f8), c.boxes.to(f8), c.vars.to(f8)
    B, Q, C = lg.shape
    T = c.sizes
    bidx = torch.cat([torch.full_like(i, b) for b, (i, _) in enumerate(c.idx)])
    sidx = torch.cat([i for i, _ in c.idx])
    tb = torch.cat([c.tgt_boxes[b][j] for b, (_, j) in enumerate(c.idx)]).to(f8).reshape(-1, 4)
    tl = torch.cat([c.tgt_labels[b][j] for b, (_, j) in enumerate(c.idx)])
    K = int(bidx.numel())
    nb = max(float(K if nb_from_pairs else sum(T)), 1.0)

    def sgn(x):
        return torch.sign(x) + sign0 * (x == 0).to(f8)

    out = {}
    # ---- labels: focal loss over every (b, q, c); accuracy and cardinality
    tc = torch.full((B, Q), 0 if unmatched_class0 else c.num_classes, dtype=torch.int64)
    tc[bidx, sidx] = tl
    t = (torch.arange(C)[None, None, :] == tc[..., None]).to(f8)
    p = torch.sigmoid(lg)
    ce = lg.clamp(min=0) + torch.log1p(torch.exp(-lg.abs())) - lg * t
    pt = p * t + (1 - p) * (1 - t)
    m = 1 - pt
    at = ALPHA * t + (1 - ALPHA) * (1 - t)
    out["loss_ce"] = float((at * ce * m * m).sum() / nb)
    dpt = (2 * t - 1) * p * (1 - p)
    out["d_logits/ce"] = at * ((p - t) * m * m - ce * 2 * m * dpt) / nb
    top = lg == lg.amax(-1, keepdim=True)
    pos = torch.arange(C)[None, None, :].expand_as(lg)
    arg = torch.where(top, pos, torch.full_like(pos, -1)).amax(-1) if argmax_last else torch.where(top, pos, torch.full_like(pos, C)).amin(-1)
    # the two statistics of whole numbers in the reference's own fp32 steps (A2/util/misc.py:436-452, :199-211), so that they compare exactly
    out["class_error"] = float(100 - (arg[bidx, sidx] == tl).float().sum() * (100.0 / K)) if K else 100.0
    card = (arg != C - 1).sum(1).to(f8)
    out["cardinality_error"] = float((card.float() - torch.tensor(T, dtype=torch.float32)).abs().mean())
    # ---- boxes: L1 and GIoU on the matched pairs
    sb = bx[bidx, sidx]
    e = sb - tb
    out["loss_bbox"] = float(e.abs().sum() / nb)
    d_l1 = torch.zeros_like(bx)
    d_l1[bidx, sidx] = sgn(e) / nb
    out["d_boxes/bbox"] = d_l1
    x1, y1, x2, y2 = sb[:, 0] - 0.5 * sb[:, 2], sb[:, 1] - 0.5 * sb[:, 3], sb[:, 0] + 0.5 * sb[:, 2], sb[:, 1] + 0.5 * sb[:, 3]
    u1, v1, u2, v2 = tb[:, 0] - 0.5 * tb[:, 2], tb[:, 1] - 0.5 * tb[:, 3], tb[:, 0] + 0.5 * tb[:, 2], tb[:, 1] + 0.5 * tb[:, 3]
    a1, a2 = (x2 - x1) * (y2 - y1), (u2 - u1) * (v2 - v1)
    iw0, ih0 = torch.minimum(x2, u2) - torch.maximum(x1, u1), torch.minimum(y2, v2) - torch.maximum(y1, v1)
    iw, ih = iw0.clamp(min=0), ih0.clamp(min=0)
    inter = iw * ih
    uni = a1 + a2 - inter
    cw0, ch0 = torch.maximum(x2, u2) - torch.minimum(x1, u1), torch.maximum(y2, v2) - torch.minimum(y1, v1)
    cw, ch = cw0.clamp(min=0), ch0.clamp(min=0)
    area = cw * ch
    giou = inter / uni - (area - uni) / area
    out["loss_giou"] = float((1 - giou).sum() / nb)

    def first_wins(a, b):                             # d max(a, b) / da = d min(b, a) / db
        return (a > b).to(f8) + tie * (a == b).to(f8)

    def passes(x):
        return (x > 0).to(f8) if clamp_strict else (x >= 0).to(f8)

    # derivatives w.r.t. the prediction's (x1, y1, x2, y2) of: the intersection, the prediction's area, the enclosing area
    d_inter = (-passes(iw0) * first_wins(x1, u1) * ih, -passes(ih0) * first_wins(y1, v1) * iw,
               passes(iw0) * first_wins(u2, x2) * ih, passes(ih0) * first_wins(v2, y2) * iw)
    d_a1 = (-(y2 - y1), -(x2 - x1), (y2 - y1), (x2 - x1))
    d_area = (-passes(cw0) * first_wins(u1, x1) * ch, -passes(ch0) * first_wins(v1, y1) * cw,
              passes(cw0) * first_wins(x2, u2) * ch, passes(ch0) * first_wins(y2, v2) * cw)
    gx = []
    for di, da, dA in zip(d_inter, d_a1, d_area):
        du = da - di
        gx.append((di * uni - inter * du) / (uni * uni) + (du * area - uni * dA) / (area * area))     # giou = iou - 1 + union / area
    d_gi = torch.zeros_like(bx)
    d_gi[bidx, sidx] = -torch.stack([gx[0] + gx[2], gx[1] + gx[3], 0.5 * (gx[2] - gx[0]), 0.5 * (gx[3] - gx[1])], 1) / nb
    out["d_boxes/giou"] = d_gi
    # ---- variance loss: sum_k (mean_j |dw_j| / |v0_k| + |log v0_k| + the same for h) / nb
    d_vb, d_v = torch.zeros_like(bx), torch.zeros_like(pv)
    if K:
        v = pv[bidx, sidx]
        dev = e[:, 2:].abs()
        if var_mean_per_image:
            mean = torch.stack([dev[bidx == b].mean(0) if bool((bidx == b).any()) else dev.new_zeros(2) for b in range(B)])[bidx]     # [K, 2]
            cnt = torch.stack([(bidx == b).sum() for b in range(B)])[bidx].to(f8)[:, None]
            inv = torch.stack([(1 / v.abs())[bidx == b].sum(0) for b in range(B)])[bidx]
        else:
            mean, cnt, inv = dev.mean(0)[None, :].expand(K, 2), float(K), (1 / v.abs()).sum(0)[None, :].expand(K, 2)
        out["loss_variance"] = float((mean / v.abs() + v.log().abs()).sum() / nb)
        d_vb[bidx, sidx] = torch.cat([torch.zeros(K, 2, dtype=f8), sgn(e[:, 2:]) / cnt * inv / nb], 1)
        d_v[bidx, sidx] = (-mean * sgn(v) / (v * v) + sgn(v.log()) / v) / nb
    else:
        out["loss_variance"] = 0.0
    out["d_boxes/var"], out["d_vars/var"] = d_vb, d_v
    out["total"] = sum(w * out[k] for w, k in zip(W6, ORDER6))
    return out


# ----------------------------------------------------------------------------------------------------- match cost
MATCH_LAUNCHES = {"sizes": (17, 40, 45), "few": (1, 0, 12)}      # T < Q, T == Q, T > Q in one launch; one target, none, a dozen
MATCH_TABLES = ("pinned", "band", "golden_scale")
MATCH_Q = 40
PINNED_SAT = (20.0, -20.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
BAND = (4.5, 17.0)
EXACT_FROM = 20.0       # e^-20 < 2^-26: 1 + expf(-x) rounds to exactly 1 under any expf, so p == 1.0f and the class cost is deterministic
# Rows whose fp32 reference agrees with fp64 and are therefore ALSO compared with fp64: x <= 2 (1 - p >= 0.12 keeps its bits) and x >= 40
# (1 - p < 1e-17 vanishes beside the 1e-8 in both precisions).  Between them the reference's own fp32 is off: through the last bit of p up
# to 20, and from 20 on because fp32 has p == 1 while the true 1 - p (2e-9 at 20, 1e-13 at 30: 1.4e-5 of cost) still counts beside 1e-8.
# There the bracket alone holds.
WELL_BELOW, WELL_FROM = 2.0, 40.0


def well_rows(mc, b):
    x = mc.logits[b, :, 0]
    return (x <= WELL_BELOW) | (x >= WELL_FROM)


@dataclass
class MatchCase:
    name: str
    logits: torch.Tensor          # [B, Q, 2]
    boxes: torch.Tensor           # [B, Q, 4]
    tgt: list                     # [T_b, 4] per image
    dup_q: tuple                  # (q, q'): identical predictions (box and logits) in every image
    dup_t: dict                   # b -> (j, j'): identical targets of image b

    @property
    def sizes(self):
        return tuple(int(t.shape[0]) for t in self.tgt)


EDGE_PAIRS = (((32, 32, 16, 12), (32, 32, 16, 12)),           # identical
              ((38, 33, 12, 8), (24, 32, 16, 12)),            # shared edge in x
              ((32, 32, 10, 6), (32, 32, 24, 20)),            # concentric
              ((32, 30, 12, 14), (32, 24, 12, 10)),           # same cx and w
              ((54, 54, 6, 6), (10, 10, 4, 4)),               # disjoint
              ((30, 30, 1, 1), (32, 32, 40, 36)))             # tiny
DUP_Q = (7, MATCH_Q - 1)


@functools.lru_cache(maxsize=None)
def match_case(launch, table):
    T = MATCH_LAUNCHES[launch]
    B, Q = len(T), MATCH_Q
    gen = g(300 + len(launch))
    boxes = rand_boxes(B * Q, gen).reshape(B, Q, 4)
    tgt = [rand_boxes(t, gen) for t in T]
    dup_t = {}
    for b, t in enumerate(T):
        for k, (pr, tg) in enumerate(EDGE_PAIRS[:t]):         # query k and target k of every image form edge pair k
            boxes[b, k], tgt[b][k] = u64(pr)[0], u64(tg)[0]
        if t >= 9:
            tgt[b][t - 1] = tgt[b][8]
            dup_t[b] = (8, t - 1)
    lgen = g(400 + MATCH_TABLES.index(table))
    other = torch.randn(B, Q, generator=lgen)
    if table == "pinned":
        x = torch.rand(B, Q, generator=lgen) * 4 - 2
        for b in range(B):
            x[b, 10:10 + len(PINNED_SAT)] = torch.tensor(PINNED_SAT)
            x[b, 0] = EXACT_FROM                              # the identical pair with p == 1 exactly
    elif table == "band":
        x = torch.stack([torch.linspace(BAND[0], BAND[1], Q).roll(7 * b) for b in range(B)])
    else:
        x = torch.randn(B, Q, generator=lgen) * 3
    logits = torch.stack([x, other], -1)
    boxes[:, DUP_Q[1]], logits[:, DUP_Q[1]] = boxes[:, DUP_Q[0]], logits[:, DUP_Q[0]]
    return MatchCase(f"{launch}-{table}", logits, boxes, tgt, DUP_Q, dup_t)


MATCH_CASES = tuple((la, ta) for la in MATCH_LAUNCHES for ta in MATCH_TABLES)


def class_cost_of_p(p):
    """The class term of A2/models/matcher.py:231-235 on a given p (target id 0)."""
    neg = (1 - 0.25) * (p ** 2.0) * (-(1 - p + 1e-8).log())
    pos = 0.25 * ((1 - p) ** 2.0) * (-(p + 1e-8).log())
    return pos - neg


def cost_of_p(p, pred_boxes, tgt_boxes, w_class=2.0, w_bbox=5.0, w_giou=2.0):
    """oracle.criterion.match_cost with the sigmoid handed in: p [Q, C] (as the oracle forms it, so that torch takes the same vector code
    path) -> [Q, T], same expression and summation order."""
    cost_class = class_cost_of_p(p)[:, torch.zeros(tgt_boxes.shape[0], dtype=torch.int64)]
    cost_bbox = torch.cdist(pred_boxes, tgt_boxes, p=1)
    cost_giou = -OC.generalized_box_iou(OC.box_cxcywh_to_xyxy(pred_boxes), OC.box_cxcywh_to_xyxy(tgt_boxes))
    return w_bbox * cost_bbox + w_class * cost_class + w_giou * cost_giou


def match_oracle(mc, b, dtype=torch.float32):
    """[Q, T_b] cost block of image b from oracle.criterion.match_cost in `dtype`."""
    return OC.match_cost(mc.logits[b].to(dtype), mc.boxes[b].to(dtype), mc.tgt[b].to(dtype))


def moved(p, x, ulps):
    """p moved by `ulps` fp32 ulps (clamped to [0, 1]); not where x >= EXACT_FROM, where p is exactly 1 under any implementation."""
    q = p.clone()
    toward = torch.full_like(p, float("inf") if ulps > 0 else -float("inf"))
    for _ in range(abs(ulps)):
        q = torch.nextafter(q, toward)
    return torch.where(x >= EXACT_FROM, p, q.clamp(0.0, 1.0))


def match_bracket(mc, b):
    """(lo, hi) [Q, T_b] fp32: the fp32 oracle's cost at p - 2 ulp and p + 2 ulp.  The class cost falls monotonically in p, so the two bracket
    the cost under any sigmoid within 2 ulp of torch's; zero width from logit EXACT_FROM up."""
    x = mc.logits[b]
    p = x.sigmoid()
    ca = cost_of_p(moved(p, x, -2), mc.boxes[b], mc.tgt[b])
    cb = cost_of_p(moved(p, x, +2), mc.boxes[b], mc.tgt[b])
    return torch.minimum(ca, cb), torch.maximum(ca, cb)


def cost_err(mc, b, a):
    """max|a - r| / max|r| of a [Q, T_b] cost block against fp64 over the rows of well_rows()."""
    rows = well_rows(mc, b)
    r = match_oracle(mc, b, torch.float64)[rows]
    return err("cost", a[rows], r) if r.numel() else 0.0


def cost_floor(mc, b):
    return cost_err(mc, b, match_oracle(mc, b))


def undo_layout(flat, plan_off, b, Q, T):
    """The device cost block of image b as [Q, T] (the solver's layout puts the shorter side first)."""
    blk = flat[plan_off[b]: plan_off[b] + Q * T]
    return blk.view(T, Q).t() if T < Q else blk.view(Q, T)


def canonical(ii, jj, dup_q, dup_t):
    """A matching with duplicate predictions / targets mapped to their first copy: sorted (query, target) pairs."""
    rq = {dup_q[1]: dup_q[0]} if dup_q else {}
    rt = {dup_t[1]: dup_t[0]} if dup_t else {}
    return sorted((rq.get(int(i), int(i)), rt.get(int(j), int(j))) for i, j in zip(ii, jj))


def second_best_gap(cost, ii, jj, dup_q, dup_t, solver):
    """How much the best matching that is NOT the optimum up to duplicates costs more than the optimum (cost: float64 numpy [Q, T]).  Such a
    matching misses, for some optimal pair (i, j), every pair in copies(i) x copies(j): forbid that block, solve again, take the smallest."""
    best = cost[ii, jj].sum()
    copies_q = lambda i: list(dup_q) if (dup_q and i in dup_q) else [i]      # noqa: E731
    copies_t = lambda j: list(dup_t) if (dup_t and j in dup_t) else [j]      # noqa: E731
    big = float(abs(cost).sum()) + 1.0
    gap = float("inf")
    for i, j in zip(ii.tolist(), jj.tolist()):
        c2 = cost.copy()
        for a in copies_q(i):
            for d in copies_t(j):
                c2[a, d] = big
        r2, k2 = solver(c2)
        gap = min(gap, float(c2[r2, k2].sum() - best))
    return gap
