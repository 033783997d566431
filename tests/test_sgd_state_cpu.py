"""--sgd's checkpoint layer without a GPU: engine.Trainer(sgd) writes torch.optim.SGD's state_dict layout (the reference's three groups and
numbering), the installed torch loads it, a fresh SGD trainer reads it back (and the reference's torch 1.8 layout), and loading the other
optimizer's state raises.  The trainer is built on the CPU; no update runs (that needs the HIP kernel: tests/test_sgd_train_gpu.py)."""
import pytest
import torch


def trainer(sgd, seed=0):
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import Trainer
    torch.manual_seed(seed)
    args = default_args(device="cpu", num_query_position=100, sgd=sgd, lr=0.1, lr_backbone=0.05, lr_drop=1)
    model, crit, _ = counting_detr_amd.build_model(args)
    return Trainer(model, crit, args, device="cpu")


@pytest.fixture(scope="module")
def stepped():
    """An SGD trainer with a (made-up) momentum buffer after two steps and one lr drop, and its state_dict."""
    tr = trainer(True)
    tr.momentum_buffer.copy_(torch.randn(tr.momentum_buffer.numel(), generator=torch.Generator().manual_seed(1)))
    tr.opt_state[0] = 2.0
    tr.lr_scheduler_step()
    return tr, tr.state_dict()


def test_sgd_trainer_arenas_and_fresh_layout():
    tr = trainer(True)
    assert tr.sgd and tr.optimizer_name == "SGD" and tr.exp_avg is None and tr.exp_avg_sq is None
    assert tr.momentum_buffer.shape == tr.flat_p.shape
    sd = tr.state_dict()
    assert sd["state"] == {}                                # torch: no state before the first step
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9).state_dict()["param_groups"][0]
    for pg in sd["param_groups"]:
        assert set(ref) | {"initial_lr"} == set(pg)
        assert (pg["momentum"], pg["dampening"], pg["nesterov"], pg["weight_decay"]) == (0.9, 0, False, 1e-4)


def test_sgd_state_dict_layout_and_torch_load(stepped):
    tr, sd = stepped
    groups, lrs = tr._torch_param_order()
    order = [n for g in groups for n in g]
    assert [len(pg["params"]) for pg in sd["param_groups"]] == [len(g) for g in groups]
    assert sorted(sd["state"]) == [i for i, n in enumerate(order) if n in tr.offsets]      # none for input_proj.* (never a gradient)
    assert any(n.startswith("input_proj.") for n in order) and len(sd["state"]) < len(order)
    params = dict(tr.model.named_parameters())
    for i, n in enumerate(order):
        if i in sd["state"]:
            off, sz = tr.offsets[n]
            assert set(sd["state"][i]) == {"momentum_buffer"}
            assert torch.equal(sd["state"][i]["momentum_buffer"], tr._view_like(tr.momentum_buffer[off:off + sz], params[n]))
    assert [pg["lr"] for pg in sd["param_groups"]] == pytest.approx([lr * 0.1 for lr in lrs])
    assert [pg["initial_lr"] for pg in sd["param_groups"]] == lrs
    cpu = {n: torch.nn.Parameter(p.detach().clone()) for n, p in params.items()}
    opt = torch.optim.SGD([{"params": [cpu[n] for n in g], "lr": lr} for g, lr in zip(groups, lrs)], lr=0.1, momentum=0.9, weight_decay=1e-4)
    opt.load_state_dict(sd)
    assert len(opt.state) == len(sd["state"])
    assert all(opt.state[cpu[n]]["momentum_buffer"].shape == cpu[n].shape for i, n in enumerate(order) if i in sd["state"])


def test_sgd_roundtrip_and_reference_layout(stepped):
    tr, sd = stepped
    tr2 = trainer(True, seed=5)
    tr2.load_state_dict(sd, tr.lr_scheduler_state_dict())
    assert torch.equal(tr2.momentum_buffer, tr.momentum_buffer)
    assert float(tr2.opt_state[1]) == float(tr.opt_state[1]) and tr2.epoch == 1 and float(tr2.opt_state[3]) == 0.0
    assert tr2.state_dict()["state"].keys() == sd["state"].keys()
    keep = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "initial_lr", "params")      # torch 1.8's SGD param_group keys
    old = {"state": sd["state"], "param_groups": [{k: v for k, v in pg.items() if k in keep} for pg in sd["param_groups"]]}
    tr3 = trainer(True, seed=6)
    tr3.load_state_dict(old)
    assert torch.equal(tr3.momentum_buffer, tr.momentum_buffer)


def test_cross_optimizer_loads_raise(stepped):
    _, sd = stepped
    adam = trainer(False)
    assert adam.optimizer_name == "AdamW" and not hasattr(adam, "momentum_buffer")
    with pytest.raises(RuntimeError, match=r"written by SGD, this trainer runs AdamW.*weights only"):
        adam.load_state_dict(sd)
    sgd = trainer(True)
    with pytest.raises(RuntimeError, match=r"written by AdamW, this trainer runs SGD.*weights only"):
        sgd.load_state_dict(adam.state_dict())
    round1 = {"names": adam.names, "exp_avg": adam.exp_avg, "exp_avg_sq": adam.exp_avg_sq, "state": adam.opt_state, "epoch": 0}
    with pytest.raises(RuntimeError, match=r"written by AdamW"):
        sgd.load_state_dict(round1)
