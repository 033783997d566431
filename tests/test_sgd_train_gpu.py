"""Stage-2 training with --sgd (engine.Trainer over cdetr_sgd_step) on the MI355X:
  (a) three eager steps against the REAL reference trained with --sgd (tests/golden/g14_sgd_train.npz, tools/gen_golden_sgd_train.py);
  (b) the cached graph step against the stream-ordered step, and the captured update against the stream-ordered one;
  (c) state_dict: a round trip into a fresh SGD trainer, torch.optim.SGD loading it and stepping like us, cross-optimizer loads raising;
  (d) main.py --synthetic --sgd end to end in fresh child processes, --auto_resume included."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, LR_BACKBONE = 0.1, 0.05          # the golden's learning rates: an update is many ulps of the weights it moves (the reference's 1e-4 is not)


def build(sgd=True, nq=300, **kw):
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from oracle.weights import model_schema, seeded_state_dict
    args = default_args(device=DEV, num_query_position=nq, sgd=sgd, lr=LR, lr_backbone=LR_BACKBONE, lr_drop=1, **kw)
    model, crit, _ = counting_detr_amd.build_model(args)
    model.load_state_dict(seeded_state_dict(model_schema(num_position=nq)), strict=True)
    model.backbone.exemplar_mode = "reference"
    return model.to(DEV).train(), crit, args


def dev_batch(B, H, W, Ts, seed):
    from oracle.step import synthetic_batch
    images, rects, targets = synthetic_batch(B=B, H=H, W=W, Ts=Ts, seed=seed)
    return images.to(DEV), rects.to(DEV), [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def test_eager_steps_match_reference_sgd_training(golden):
    from counting_detr_amd.engine import Trainer
    z = golden("g14_sgd_train.npz")
    lr, lr_bb, wd, mom, max_norm, drop_after = z["hyper"].tolist()
    assert (lr, lr_bb, wd, mom, max_norm) == (LR, LR_BACKBONE, 1e-4, 0.9, 0.1)
    model, crit, args = build()
    tr = Trainer(model, crit, args, device=DEV)
    assert tr.sgd and tr.exp_avg is None and tr.exp_avg_sq is None and tr._lr_two is not None
    names = [str(n) for n in z["param_names"]]
    params = dict(model.named_parameters())
    for s, (H, W, T, seed) in enumerate(z["steps"].tolist()):
        if s == int(drop_after):
            tr.lr_scheduler_step()              # StepLR(step_size 1): the third step at 0.1 lr, the buffer carried on unscaled
        assert float(z[f"s{s}/min_swap_gap"]) >= 1e-3 and float(z[f"s{s}/min_l1_margin"]) >= 1e-4     # well posed (checked at generation)
        res = tr.train_step(*dev_batch(1, H, W, (T,), seed))
        # step 1 at the bars of the stage-2 parity tests (tests/test_model_gpu.py); steps 2 and 3 start from weights that one / two updates
        # of lr 0.1 moved by up to ~1e-2 per element, carrying the bf16 backward's ~1e-2 error of the step-1 gradient into the forward:
        # 5x the bars.  (SGD, unlike AdamW, moves an element in proportion to its gradient, so no sign flip makes it jump.)
        f = 1 if s == 0 else 5
        for k in ("loss_ce", "loss_bbox", "loss_giou", "loss_variance"):
            np.testing.assert_allclose(float(res[k]), float(z[f"s{s}/L_{k}"]), rtol=1e-3 * f, atol=1e-5, err_msg=f"step {s} {k}")
        np.testing.assert_allclose(float(res["loss"]), float(z[f"s{s}/loss_total"]), rtol=1e-3 * f, err_msg=f"step {s} total")
        np.testing.assert_allclose(float(res["grad_norm"]), float(z[f"s{s}/grad_total_norm"]), rtol=2e-3 * f, err_msg=f"step {s} clip norm")
    assert tr.nonfinite_steps() == 0 and float(tr.opt_state[0]) == 3.0
    # momentum buffers: per-parameter norms (the sum of three clipped gradients, each within ~1e-2 per parameter under the bf16 backward,
    # tests/test_attn_mha_model_gpu.py's clipped-gradient bar); none for parameters the reference never gave a gradient
    buf = {n: tr._view_like(tr.momentum_buffer[off:off + sz], params[n]) for n, (off, sz) in tr.offsets.items()}
    worst = 0.0
    for n, r in zip(names, z["buf_norms"]):
        if r < 0:
            assert n not in tr.offsets, n
            continue
        got = float(buf[n].norm())
        worst = max(worst, abs(got - r) / max(r, 1e-12))
        np.testing.assert_allclose(got, r, rtol=2e-2, atol=1e-7, err_msg=n)
    # sampled elements (largest movement in the reference, >= 64 ulps each): the movement and the buffer within 5 % of the reference's,
    # or within 1 % of the parameter's largest sampled movement (an element whose three gradients nearly cancel)
    pidx, fidx = z["sample_pidx"], z["sample_fidx"]
    before, after, sbuf = (z[k].astype(np.float64) for k in ("sample_before", "sample_after", "sample_buf"))
    d_ref = after - before
    scale = {}
    for k in range(len(pidx)):
        scale[int(pidx[k])] = max(scale.get(int(pidx[k]), 0.0), abs(d_ref[k]))
    worst_d = worst_b = 0.0
    for k in range(len(pidx)):
        n = names[int(pidx[k])]
        i = int(fidx[k])
        d = float(params[n].detach().reshape(-1)[i]) - before[k]
        b = float(buf[n].reshape(-1)[i])
        sc = scale[int(pidx[k])]
        lr_n = LR_BACKBONE if "backbone" in n else LR
        worst_d = max(worst_d, abs(d - d_ref[k]) / sc)
        worst_b = max(worst_b, abs(b - sbuf[k]) * lr_n / sc)
        assert abs(d - d_ref[k]) <= 5e-2 * abs(d_ref[k]) + 1e-2 * sc, f"{n}[{i}]: moved {d:.4e}, reference {d_ref[k]:.4e}"
        assert abs(b - sbuf[k]) <= 5e-2 * abs(sbuf[k]) + 1e-2 * sc / lr_n, f"{n}[{i}]: buffer {b:.4e}, reference {sbuf[k]:.4e}"
    print(f"sgd parity: worst buffer-norm error {worst:.2e}; worst sampled movement / buffer error {worst_d:.2e} / {worst_b:.2e} of the "
          f"parameter's largest movement ({len(pidx)} elements)")


def test_graph_step_equals_train_step():
    """Trainer.step (captured, cached graph) vs Trainer.train_step from the same weights over three batches (the lr drop between 2 and 3).
    Two runs of the backward add split-K partial sums in different atomic orders, so gradients differ at rounding level; SGD moves an
    element in proportion to its gradient, so the parameters agree to rounding of lr * g."""
    from counting_detr_amd.engine import Trainer
    batches = [dev_batch(2, 128, 160, (7, 13), s) for s in range(3)]
    res, flat, bufs = [], [], []
    for use_graph in (False, True):
        model, crit, args = build(nq=100)
        tr = Trainer(model, crit, args, device=DEV)
        outs = []
        for s, b in enumerate(batches):
            if s == 2:
                tr.lr_scheduler_step()
            o = tr.step(*b) if use_graph else tr.train_step(*b)
            outs.append({k: float(v) for k, v in o.items()})
        torch.cuda.synchronize()
        if use_graph:
            assert tr.cache_stats["captures"] == 1
        res.append(outs)
        flat.append(tr.flat_p.detach().clone())
        bufs.append(tr.momentum_buffer.detach().clone())
    for a, b in zip(res[0], res[1]):
        for k in a:
            np.testing.assert_allclose(b[k], a[k], rtol=1e-4, atol=1e-6, err_msg=k)
    dp, db = (flat[0] - flat[1]).abs(), (bufs[0] - bufs[1]).abs()
    print(f"graph vs eager: max |dp| {float(dp.max()):.2e}, max |dbuf| {float(db.max()):.2e}")
    assert float(dp.max()) <= 1e-5 and float(db.max()) <= 1e-4


def test_captured_update_bit_identical_to_stream_ordered():
    """The SGD update replayed from a captured graph (state in device memory: step count, StepLR factor) == the stream-ordered update, bit
    for bit, over three steps from the same gradient arenas with the lr drop between the 2nd and the 3rd."""
    from counting_detr_amd.engine import Trainer
    trs = []
    for _ in range(2):
        model, crit, args = build(nq=100)
        trs.append(Trainer(model, crit, args, device=DEV))
    n = trs[0].flat_g.numel()
    grads = [(torch.randn(n, generator=torch.Generator().manual_seed(70 + s)) * 1e-3).to(DEV) for s in range(3)]
    eager, cap = trs
    s0 = torch.cuda.Stream()
    s0.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s0):
        with torch.cuda.graph(graph, stream=s0):
            cap._optimizer_step()
    torch.cuda.current_stream().wait_stream(s0)
    assert float(cap.opt_state[0]) == 0.0                       # captured, not run
    for s in range(3):
        if s == 2:
            eager.lr_scheduler_step()
            cap.lr_scheduler_step()
        eager.flat_g.copy_(grads[s])
        cap.flat_g.copy_(grads[s])
        eager._optimizer_step()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.flat_p, cap.flat_p) and torch.equal(eager.momentum_buffer, cap.momentum_buffer)
    assert torch.equal(eager.opt_state, cap.opt_state) and float(cap.opt_state[0]) == 3.0


def _param_groups(model, args, params=None):
    """A2/main.py:157-183's three groups over `params` (name -> tensor; default: the model's parameters)."""
    params = params or dict(model.named_parameters())
    bb = lambda n: any(k in n for k in args.lr_backbone_names)          # noqa: E731
    lp = lambda n: any(k in n for k in args.lr_linear_proj_names)       # noqa: E731
    named = [n for n, p in model.named_parameters() if p.requires_grad]
    return [{"params": [params[n] for n in named if not bb(n) and not lp(n)], "lr": args.lr},
            {"params": [params[n] for n in named if bb(n)], "lr": args.lr_backbone},
            {"params": [params[n] for n in named if lp(n)], "lr": args.lr * args.lr_linear_proj_mult}]


def test_state_dict_roundtrip_torch_sgd_and_cross_loads():
    from counting_detr_amd.engine import Trainer
    model, crit, args = build(nq=100)
    tr = Trainer(model, crit, args, device=DEV)
    sd0 = tr.state_dict()
    assert sd0["state"] == {} and all(pg["momentum"] == 0.9 and pg["nesterov"] is False and pg["dampening"] == 0 for pg in sd0["param_groups"])
    for s in range(2):
        tr.train_step(*dev_batch(2, 128, 160, (7, 13), s))
    tr.lr_scheduler_step()
    sd = tr.state_dict()
    buf0 = tr.momentum_buffer.clone()
    # the reference's torch 1.8 layout of the same state (no maximize / foreach / differentiable / fused keys); copies: torch's SGD below
    # steps the buffers it loads in place
    old = {"state": {i: {"momentum_buffer": v["momentum_buffer"].clone()} for i, v in sd["state"].items()},
           "param_groups": [{k: v for k, v in pg.items() if k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "initial_lr", "params")}
                            for pg in sd["param_groups"]]}
    # torch SGD's layout: momentum buffers only, none for parameters without a gradient (input_proj.*), the reference's numbering
    order = [n for g in tr._torch_param_order()[0] for n in g]
    assert sorted(sd["state"]) == [i for i, n in enumerate(order) if n in tr.offsets]
    assert all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    assert [pg["lr"] for pg in sd["param_groups"]] == pytest.approx([LR * 0.1, LR_BACKBONE * 0.1, LR * 0.1 * 0.1])
    # (1) round trip into a fresh SGD trainer: the same buffers and state, then a bit-identical update from the same gradient
    m2, c2, a2 = build(nq=100)
    m2.load_state_dict(model.state_dict())
    tr2 = Trainer(m2, c2, a2, device=DEV)
    tr2.load_state_dict(sd, tr.lr_scheduler_state_dict())
    assert torch.equal(tr2.momentum_buffer, tr.momentum_buffer) and torch.equal(tr2.flat_p, tr.flat_p)
    assert float(tr2.opt_state[1]) == float(tr.opt_state[1]) and tr2.epoch == tr.epoch
    grad = (torch.randn(tr.flat_g.numel(), generator=torch.Generator().manual_seed(3)) * 1e-3).to(DEV)
    # (2) the installed torch.optim.SGD loads the same entry and steps like us from that gradient (clip_grad_norm_(0.1) first)
    names = dict(model.named_parameters())
    cpu = {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in names.items()}
    opt = torch.optim.SGD(_param_groups(model, args, cpu), lr=LR, momentum=0.9, weight_decay=args.weight_decay)
    opt.load_state_dict(sd)
    for n, p in cpu.items():
        if n in tr.offsets:
            off, sz = tr.offsets[n]
            p.grad = tr._view_like(grad[off:off + sz], names[n]).detach().cpu().clone()
    torch.nn.utils.clip_grad_norm_([p for p in cpu.values() if p.grad is not None], 0.1)
    opt.step()
    for t in (tr, tr2):
        t.flat_g.copy_(grad)
        t._optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.flat_p, tr2.flat_p) and torch.equal(tr.momentum_buffer, tr2.momentum_buffer)
    worst = 0.0
    for n, p in cpu.items():
        if n not in tr.offsets:
            continue
        got = names[n].detach().cpu()
        worst = max(worst, float((got - p.detach()).abs().max()))
        np.testing.assert_allclose(got.numpy(), p.detach().numpy(), rtol=1e-5, atol=1e-7, err_msg=n)
        off, sz = tr.offsets[n]
        np.testing.assert_allclose(tr._view_like(tr.momentum_buffer[off:off + sz], names[n]).cpu().numpy(),
                                   opt.state[p]["momentum_buffer"].numpy(), rtol=1e-5, atol=1e-9, err_msg=n)
    print(f"torch.optim.SGD vs cdetr_sgd_step: worst |dp| {worst:.2e}")
    # (3) the reference's torch 1.8 layout loads too
    tr2.load_state_dict(old)
    assert torch.equal(tr2.momentum_buffer, buf0)
    # (4) cross-optimizer loads raise, naming both optimizers and pointing to a weights-only resume
    m3, c3, a3 = build(sgd=False, nq=100)
    tr_adam = Trainer(m3, c3, a3, device=DEV)
    with pytest.raises(RuntimeError, match=r"SGD.*AdamW.*weights only"):
        tr_adam.load_state_dict(sd)
    with pytest.raises(RuntimeError, match=r"AdamW.*SGD.*weights only"):
        tr2.load_state_dict(tr_adam.state_dict())


def test_adamw_trainer_unchanged_by_the_flag_default():
    """Args without the attribute (as tests build them) or with sgd False: the AdamW trainer, its two moment arenas and its layout."""
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import Trainer
    args = default_args(device=DEV, num_query_position=100)
    del args.sgd
    model, crit, _ = counting_detr_amd.build_model(args)
    tr = Trainer(model.to(DEV), crit, args, device=DEV)
    assert not tr.sgd and tr.optimizer_name == "AdamW" and tr.exp_avg is not None and tr.exp_avg_sq is not None
    assert not hasattr(tr, "momentum_buffer")
    assert "betas" in tr.state_dict()["param_groups"][0]


def test_main_sgd_checkpoint_and_auto_resume(tmp_path):
    """main.py --synthetic --sgd: two small epochs write a checkpoint whose optimizer entry torch.optim.SGD loads; --auto_resume continues
    from it (the SGD state restored, epoch 2 trained).  Child processes under a time limit."""
    import counting_detr_amd
    out = tmp_path / "run"
    common = [sys.executable, "main.py", "--synthetic", "--sgd", "--steps_per_epoch", "2", "--images_per_gpu", "1", "--synthetic_size", "128",
              "160", "--num_query_position", "100", "--device", DEV, "-o", str(out)]
    r = subprocess.run(common + ["--epochs", "2"], cwd=ROOT, check=True, timeout=600, capture_output=True, text=True)
    assert "optimizer: SGD" in r.stdout, r.stdout
    ck = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    sd = ck["optimizer"]
    assert ck["epoch"] == 1 and sd["state"] and all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    assert all(pg["momentum"] == 0.9 and "betas" not in pg for pg in sd["param_groups"])
    model, _, _ = counting_detr_amd.build_model(ck["args"])
    cpu = dict(model.named_parameters())
    opt = torch.optim.SGD(_param_groups(model, ck["args"], cpu), lr=ck["args"].lr, momentum=0.9)
    opt.load_state_dict(sd)
    assert all(opt.state[p]["momentum_buffer"].shape == p.shape for p in cpu.values() if p in opt.state)
    r = subprocess.run(common + ["--epochs", "3", "--auto_resume"], cwd=ROOT, check=True, timeout=600, capture_output=True, text=True)
    assert "continuing at epoch 2" in r.stdout, r.stdout
    ck2 = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 2 and set(ck2["optimizer"]["state"]) == set(sd["state"])
