"""cdetr_adamw_step / cdetr_adamw_step2 (clip_grad_norm_ + torch.optim.AdamW in one pass: the kernel that writes the weights) against
torch's formula in fp64 and against torch.optim.AdamW itself.  Needs an MI355X.

What is compared: the update (p1 - p0) / (lr s) -- not p, where rtol 1e-6 on |p| ~ 0.1 hides a 1 % error of a 1e-4 step --, m and v, each
as max |error| over max |reference| of the tensor, and the state block exactly.  The update of the "eps slice" (elements with zero and
with 1e-9 ... 1e-6 gradients, where sqrt(v) / sqrt(bc2) is comparable to eps) is measured again on its own, over its own max |update|.

Every bar is 4 x the error that a float32 NumPy restatement of the *reference* (optimizer_arenas.adamw_ref32: torch's operation order,
every intermediate float32) makes against fp64 on the same inputs, floor 4 fp32 ulp; it is computed per case, from the inputs, never from
the kernel.  No bar was changed after the kernel was first measured.  Worst errors over the cases of a kind, kernel / restatement (the
kernel on an MI355X, first run; the restatement needs no GPU):

                                   update            m                 v                 eps-slice update
    one step, lr 1e-2 / 1e-3       4.2e-5 / 1.2e-4   3.0e-7 / 5.0e-7   1.30e-5 / 1.29e-5   5.3e-4 / 5.3e-4
    one step, lr 1e-4 / 1e-5       3.0e-3 / 3.0e-3   3.0e-7 / 5.0e-7   1.30e-5 / 1.29e-5   8.0e-2 / 8.0e-2
    lr_split edges (lr 1e-2)       4.4e-5 / 1.1e-4   1.3e-7 / 1.6e-7   5.1e-6 / 5.0e-6     5.3e-4 / 5.3e-4
    20 steps, each, lr 1e-2        2.2e-4 / 3.8e-4   2.2e-7 / 2.2e-7   1.28e-5 / 1.28e-5   2.8e-4 / 2.8e-4
    20 steps, each, lr 1e-4        1.9e-2 / 1.9e-2   2.2e-7 / 2.2e-7   1.28e-5 / 1.28e-5   2.7e-2 / 2.7e-2
    20 steps free-running          displacement 1.5e-5 / 2.2e-5 (lr 1e-2), 7.0e-4 / 7.0e-4 (lr 1e-4), m 2.1e-7 / 2.9e-7, v 1.28e-5 / 1.27e-5

The kernel sits at the restatement's level everywhere.  What sets the levels:
  * v, 1.3e-5 at every t: the float nearest 0.999 is 0.99900001287, so 1 - beta2 formed in float is 1.3e-5 off the 0.001 torch computes with;
    any fp32 AdamW handed beta2 as a float has it (the kernel forms `1.f - beta2`); the update inherits about half of it.
  * the update at the shipped learning rates: rounding p to fp32 (|p| up to 0.4: half an ulp is 1.5e-8) against a step of lr s = 5e-6
    (the 20 steps: 1e-6) -- 3e-3 (2e-2) of a step that no fp32 parameter can resolve; at lr 1e-2 it is 1e-4 and below.  The eps slice of the
    n = 7 case is two elements whose own update is 0.02 lr, hence its 8e-2 there.
  * m: 1 - beta1 formed in float (2.4e-7 off 0.1) and two roundings.
"""
import itertools

import numpy as np
import pytest
import torch

from optimizer_arenas import (BETA1, BETA2, DEV, EPS, Arenas, adam_state, adamw_ref32, adamw_ref64, bar, eps_slices, g, make_grad, relmax)

pytestmark = pytest.mark.gpu

HP = {"visible": (1e-2, 1e-3, 0.1),          # lr s wd = 5e-4: the decay term moves p by 0.1 |p| lr, far above every bar
      "shipped": (1e-4, 1e-5, 1e-4)}         # lr, lr_backbone, weight_decay of the product: 1 - lr s wd rounds to 1.0f (torch's fp32 path too)
SCALE = 0.5                                  # state[1], the StepLR factor, in the single-step cases
NS = [3, 7, 1030, 262147, 4194307]           # 3: tail only; 4194307 > 2048 blocks x 256 lanes x 4 floats: two grid-stride iterations + a tail
ENTRIES = [("step", "table"), ("step2", "table"), ("step2", "two")]
CLIPS = [0.1, 1e6, 0.0]                      # active (norm ~ 0.05 sqrt(n) for n >= 1030), inactive, off
COUNTS = [0, 1, 9, 999, 99999]               # state[0]: bias correction at t = 1, 2, 10, 1e3, 1e5
FULL = list(itertools.product(CLIPS, [1.0, 0.25], COUNTS))
# the grid-stride size costs seconds of fp64 per combination on the CPU: every clip mode, grad_div and count once
BIG = [(0.1, 1.0, 0), (1e6, 0.25, 9), (0.0, 1.0, 99999), (0.1, 0.25, 999), (1e6, 1.0, 1)]


def lr_table64(n, lr0, lr1):
    return torch.where(torch.arange(n) % 5 == 0, torch.tensor(lr1, dtype=torch.float64), torch.tensor(lr0, dtype=torch.float64))


def make_arenas(lr_form, n, hp, split=None):
    lr0, lr1, _ = HP[hp]
    if lr_form == "table":
        lr64 = lr_table64(n, lr0, lr1)
        return Arenas(n, lr_table=lr64.float(), adam=True), lr64
    a = Arenas(n, lr0=lr0, lr1=lr1, split=(n // 3) & ~3 if split is None else split, adam=True)
    return a, a.base_lr()


class Figures:
    """Worst kernel / restatement errors of one test, printed at its end (pytest -s, or the captured output of a failure)."""

    def __init__(self):
        self.w = {}

    def add(self, key, kernel, yard):
        k, y = self.w.get(key, (0.0, 0.0))
        self.w[key] = (max(k, kernel), max(y, yard))

    def __str__(self):
        return "  ".join(f"{k} {a:.2e}/{b:.2e}" for k, (a, b) in self.w.items())


def check(tag, fig, a, p0, ls, ref, yard, norm_ref, t_after, s, skipped=0.0, slice_idx=None, points=()):
    """The kernel's arenas `a` after a step from p0 against the reference's (p, m, v) `ref` (fp64 tensors), at bars measured by the float32
    restatement's `yard` (NumPy float32) on the same step.  ls: per-element lr s (fp64)."""
    p0 = p0.double()
    upd = lambda p1: ((torch.as_tensor(p1).double().cpu() - p0) / ls).numpy()      # noqa: E731
    u_ref, u_k, u_y = upd(ref[0]), upd(a.p), upd(yard[0])
    assert np.isfinite(u_k).all(), tag
    assert np.abs(u_ref).max() <= 4.0, f"{tag}: ill-posed input, reference update of {np.abs(u_ref).max():.1f} lr"
    todo = [("update", u_k, u_y, u_ref), ("m", a.m.cpu().numpy(), yard[1], ref[1].numpy()), ("v", a.v.cpu().numpy(), yard[2], ref[2].numpy())]
    if slice_idx is not None:
        i = slice_idx.numpy()
        todo.append(("eps-slice update", u_k[i], u_y[i], u_ref[i]))
    for name, k, y, r in todo:
        ek, ey = relmax(k, r), relmax(y, r)
        fig.add(name, ek, ey)
        assert ek <= bar(ey), f"{tag}: {name}: kernel {ek:.3e} against fp64, the float32 restatement {ey:.3e}, bar {bar(ey):.3e}"
    for i in points:                         # named elements (either side of lr_split), at the update's bar
        err = abs(u_k[i] - u_ref[i])
        assert err <= bar(relmax(u_y, u_ref)) * np.abs(u_ref).max(), f"{tag}: element {i}: update {u_k[i]:.6e}, reference {u_ref[i]:.6e}"
    st = a.state.cpu().tolist()
    assert st[0] == float(t_after) and st[1] == float(np.float32(s)) and st[3] == skipped, (tag, st)
    assert abs(st[2] - norm_ref) <= 1e-5 * norm_ref, (tag, st[2], norm_ref)
    return u_ref


def single_step(fig, entry, lr_form, n, hp, max_norm, grad_div, t0, split=None, points=()):
    _, _, wd = HP[hp]
    tag = f"{entry}/{lr_form} n={n} {hp} max_norm={max_norm} grad_div={grad_div} t={t0 + 1} split={split}"
    seed = n + 17 * t0 % 1000
    a, lr = make_arenas(lr_form, n, hp, split)
    zi, ti = eps_slices(n, seed)
    p0, m0, v0 = adam_state(n, seed, t0, lr, SCALE, max_norm, wd, grad_div, zi, ti)
    gr = make_grad(n, seed + 50, 0.05, max_norm, grad_div, zi, ti)
    a.load(p=p0, g=gr, m=m0, v=v0)
    a.state[0], a.state[1] = float(t0), SCALE
    a.step_adamw(entry, max_norm, wd, grad_div)
    args = (lr, SCALE, t0 + 1, max_norm)
    ref = adamw_ref64(p0.double(), gr.double(), m0.double(), v0.double(), *args, wd, grad_div)
    yard = adamw_ref32(p0.numpy(), gr.numpy(), m0.numpy(), v0.numpy(), lr.numpy().astype(np.float32), *args[1:], wd, grad_div)
    u_ref = check(tag, fig, a, p0, lr * SCALE, ref[:3], yard[:3], ref[3], t0 + 1, SCALE, slice_idx=torch.cat([zi, ti]), points=points)
    if t0 == 0:                              # zero gradient, zero moments: a zero Adam term, only the decay moves p
        assert float(a.m[zi.to(DEV)].abs().max()) == 0.0 and float(a.v[zi.to(DEV)].abs().max()) == 0.0, tag
    if hp == "visible":                      # the decay term is seen: without it the reference itself moves by far more than the bar
        nowd = adamw_ref64(p0.double(), gr.double(), m0.double(), v0.double(), *args, 0.0, grad_div)
        u0 = ((nowd[0] - p0.double()) / (lr * SCALE)).numpy()
        u_y = ((torch.from_numpy(yard[0]).double() - p0.double()) / (lr * SCALE)).numpy()
        assert relmax(u0, u_ref) > 10 * bar(relmax(u_y, u_ref)), f"{tag}: weight decay not visible: {relmax(u0, u_ref):.2e}"


@pytest.mark.parametrize("hp", list(HP))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("entry,lr_form", ENTRIES, ids=[f"{e}-{f}" for e, f in ENTRIES])
def test_adamw_step_vs_fp64(entry, lr_form, n, hp):
    """One step from a well-posed state, every clip mode x grad_div x step count (the grid-stride size: each of them once)."""
    fig = Figures()
    for max_norm, grad_div, t0 in (BIG if n > 2097152 else FULL):
        single_step(fig, entry, lr_form, n, hp, max_norm, grad_div, t0)
    print(f"\nFIG {entry}/{lr_form} n={n} {hp} kernel/restatement: {fig}")


def split_cases():
    out = []
    for n in NS:
        kinds = {"zero": 0, "mid": max(4, (n // 2) & ~3), "tail": n & ~3, "beyond": ((n + 3) & ~3) + 4}
        for k, s in kinds.items():
            if k == "mid" and not 0 < s < (n & ~3):
                continue
            out.append(pytest.param(n, s, id=f"{n}-{k}"))
    return out


@pytest.mark.parametrize("n,split", split_cases())
def test_lr_split_edges(n, split):
    """cdetr_adamw_step2 without a table: lr_split 0 (all lr1), a middle multiple of 4, n & ~3 (the float4 loop all lr0, the scalar tail --
    which reads lr_at, not lr4_at -- all lr1), >= n (all lr0).  lr0 = 10 lr1, so an element on the wrong side is a factor 10 (or 0.1) of
    its update; the elements at split - 1 and split are asserted by name."""
    fig = Figures()
    points = [i for i in (split - 1, split) if 0 <= i < n]
    single_step(fig, "step2", "two", n, "visible", 0.1, 1.0, 9, split=split, points=points)
    print(f"\nFIG split n={n} split={split} kernel/restatement: {fig}")


@pytest.mark.parametrize("hp", list(HP))
def test_twenty_steps_vs_torch_adamw(hp):
    """20 successive steps on fresh gradients (alternating scales: the clip is active on even steps, inactive on odd ones), two parameter
    groups [lr | lr_backbone], StepLR's factor dropping to 0.1 after step 12, clip_grad_norm_(0.1), against torch.optim.AdamW on fp64 CPU
    parameters.  Every step is compared on its own at the single-step bars: torch's parameters and state are loaded with the kernel's
    current p, m, v before it.  A second torch optimizer runs free; the kernel's distance from it after 20 steps is held to 4 x the
    free-running float32 restatement's."""
    lr0, lr1, wd = HP[hp]
    n, split, max_norm = 4099, 2048, 0.1
    a = Arenas(n, seed=5, lr0=lr0, lr1=lr1, split=split, adam=True)
    lr = a.base_lr()
    zi, ti = eps_slices(n, 5)
    p_init = torch.randn(n, generator=g(5)) * 0.1
    a.load(p=p_init)

    def torch_side():
        pa, pb = torch.nn.Parameter(p_init[:split].double().clone()), torch.nn.Parameter(p_init[split:].double().clone())
        opt = torch.optim.AdamW([{"params": [pa], "lr": lr0}, {"params": [pb], "lr": lr1}], lr=lr0, betas=(BETA1, BETA2), eps=EPS,
                                weight_decay=wd)
        return pa, pb, opt, torch.optim.lr_scheduler.StepLR(opt, 1)

    def torch_step(pa, pb, opt, gr):
        pa.grad, pb.grad = gr[:split].double().clone(), gr[split:].double().clone()
        tn = torch.nn.utils.clip_grad_norm_([pa, pb], max_norm)
        opt.step()
        cat = lambda k: torch.cat([opt.state[pa][k], opt.state[pb][k]])          # noqa: E731
        return (torch.cat([pa.detach(), pb.detach()]).clone(), cat("exp_avg").clone(), cat("exp_avg_sq").clone()), float(tn)

    pa, pb, opt, sched = torch_side()                       # compared step by step
    fa, fb, fopt, fsched = torch_side()                     # free-running
    yp, ym, yv = p_init.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)      # free-running float32 restatement
    fig, s = Figures(), 1.0
    for i in range(20):
        if i == 12:
            sched.step()
            fsched.step()
            a.state[1] = s = 0.1
        gr = make_grad(n, 100 + i, 1e-3 if i % 2 else 0.3, max_norm, 1.0, zi, ti)      # norm 0.064 < 0.1 on odd steps, 19 on even ones
        k_p, k_m, k_v = a.p.cpu().clone(), a.m.cpu().clone(), a.v.cpu().clone()
        if i:                                               # one step at a time: torch starts it from the kernel's own state
            for prm, sl in ((pa, slice(0, split)), (pb, slice(split, n))):
                prm.data.copy_(k_p[sl].double())
                opt.state[prm]["exp_avg"].copy_(k_m[sl].double())
                opt.state[prm]["exp_avg_sq"].copy_(k_v[sl].double())
        a.load(g=gr)
        a.step_adamw("step2", max_norm, wd)
        ref, tn = torch_step(pa, pb, opt, gr)
        yard = adamw_ref32(k_p.numpy(), gr.numpy(), k_m.numpy(), k_v.numpy(), lr.numpy().astype(np.float32), np.float32(s), i + 1, max_norm, wd)
        check(f"{hp} step {i}", fig, a, k_p, lr * s, ref, yard[:3], tn, i + 1, s, slice_idx=torch.cat([zi, ti]))
        free, _ = torch_step(fa, fb, fopt, gr)
        yp, ym, yv, _ = adamw_ref32(yp, gr.numpy(), ym, yv, lr.numpy().astype(np.float32), np.float32(s), i + 1, max_norm, wd)
    # free-running: the whole displacement in units of the base lr, and the moments
    disp = lambda p: ((torch.as_tensor(p).double().cpu() - p_init.double()) / lr).numpy()      # noqa: E731
    for name, k, y, r in (("displacement", disp(a.p), disp(yp), disp(free[0])), ("m", a.m.cpu().numpy(), ym, free[1].numpy()),
                          ("v", a.v.cpu().numpy(), yv, free[2].numpy())):
        ek, ey = relmax(k, r), relmax(y, r)
        fig.add("free " + name, ek, ey)
        assert ek <= bar(ey), f"{hp}: free-running {name}: kernel {ek:.3e}, the float32 restatement {ey:.3e}, bar {bar(ey):.3e}"
    print(f"\nFIG twenty steps {hp} kernel/restatement: {fig}")


NBIG = 4194307


@pytest.mark.parametrize("n,where", [(1031, 1031 - 2), (NBIG, (NBIG & ~3) - 2)], ids=["tail", "last_float4_grid_stride"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradient_skips_the_update(bad, n, where):
    """A NaN / Inf gradient (the kernel's documented branch: an ordinary value in an ordinary arena): p, m, v bit-unchanged, the step count
    unchanged, the skip latched in state[3], state[2] non-finite.  The next finite step runs with t = the unskipped count + 1: its bias
    corrections are checked against the reference (t = 5 here; t = 6, had the skipped step been counted, is 10 % off in bc1)."""
    lr0, lr1, wd = HP["visible"]
    a, lr = make_arenas("two", n, "visible", split=512)
    zi, ti = eps_slices(n, 9)
    p0, m0, v0 = adam_state(n, 9, 3, lr, 1.0, 0.1, wd, 1.0, zi, ti)
    a.load(p=p0, g=make_grad(n, 60, 0.05, 0.1, 1.0, zi, ti), m=m0, v=v0)
    a.state[0] = 3.0
    a.step_adamw("step2", 0.1, wd)                                   # a real step first: t = 4
    p1, m1, v1 = a.p.clone(), a.m.clone(), a.v.clone()
    gr = make_grad(n, 61, 0.05, 0.1, 1.0, zi, ti)
    a.load(g=gr)
    a.g[where] = bad                                                 # the skip must hold for every block, not just the one that reads it
    a.step_adamw("step2", 0.1, wd)
    assert torch.equal(a.p, p1) and torch.equal(a.m, m1) and torch.equal(a.v, v1)
    st = a.state.cpu().tolist()
    assert st[0] == 4.0 and st[1] == 1.0 and st[3] == 1.0 and not np.isfinite(st[2])
    a.load(g=gr)                                                     # the same gradient without the bad value
    a.step_adamw("step2", 0.1, wd)
    ref = adamw_ref64(p1.double().cpu(), gr.double(), m1.double().cpu(), v1.double().cpu(), lr, 1.0, 5, 0.1, wd)
    yard = adamw_ref32(p1.cpu().numpy(), gr.numpy(), m1.cpu().numpy(), v1.cpu().numpy(), lr.numpy().astype(np.float32), 1.0, 5, 0.1, wd)
    check(f"after the skipped step, n={n}", Figures(), a, p1.cpu(), lr, ref[:3], yard[:3], ref[3], 5, 1.0, skipped=1.0)


@pytest.mark.parametrize("n", [1030, NBIG])
def test_identical_arenas_stay_bit_identical(n):
    """Two arenas with the same contents, stepped separately, end with the same bits: data-parallel ranks hold the same reduced gradient
    and must not drift apart (the promise of sumsq_kernel's header for the clip coefficient, here for the whole update)."""
    lr0, lr1, wd = HP["visible"]
    zi, ti = eps_slices(n, 3)
    grads = [make_grad(n, 70 + i, 0.05, 0.1, 1.0, zi, ti) for i in range(3)]
    res = []
    for _ in range(2):
        a, _lr = make_arenas("two", n, "visible")
        a.load(p=torch.randn(n, generator=g(3)) * 0.1)
        for gr in grads:
            a.load(g=gr)
            a.step_adamw("step2", 0.1, wd)
        res.append((a.p.clone(), a.m.clone(), a.v.clone(), a.state.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert not torch.equal(res[0][0].cpu(), torch.randn(n, generator=g(3)) * 0.1)      # and the steps did run


def test_rejects_misaligned_arenas_odd_split_and_missing_table():
    from counting_detr_amd import _ffi
    L, st = _ffi.lib(), _ffi.stream_ptr()
    a = Arenas(64, seed=1, lr0=0.1, lr1=0.1, split=32, adam=True)
    P, G, M, V, S, ST = (t.data_ptr() for t in (a.p, a.g, a.m, a.v, a.sumsq, a.state))
    rc = L.cdetr_adamw_step2(P + 4, G, M, V, None, 0.1, 0.1, 32, 60, S, ST, 0.1, BETA1, BETA2, EPS, 0.0, 1.0, st)
    assert rc < 0 and b"cdetr_adamw_step2" in L.cdetr_last_error()
    rc = L.cdetr_adamw_step2(P, G, M, V, None, 0.1, 0.1, 30, 64, S, ST, 0.1, BETA1, BETA2, EPS, 0.0, 1.0, st)
    assert rc < 0 and b"lr_split" in L.cdetr_last_error()
    rc = L.cdetr_adamw_step(P, G, M, V, None, 64, S, ST, 0.1, BETA1, BETA2, EPS, 0.0, 1.0, st)
    assert rc < 0 and b"cdetr_adamw_step" in L.cdetr_last_error()
    tab = torch.full((64,), 0.1, device=DEV)
    rc = L.cdetr_adamw_step(P + 4, G, M, V, tab.data_ptr(), 60, S, ST, 0.1, BETA1, BETA2, EPS, 0.0, 1.0, st)
    assert rc < 0 and b"cdetr_adamw_step" in L.cdetr_last_error()
    torch.cuda.synchronize()
    assert a.state.cpu().tolist() == [0.0, 1.0, 0.0, 0.0]            # nothing was launched
