"""cdetr_sgd_step (clip_grad_norm_ + torch.optim.SGD(momentum, dampening 0, coupled weight decay) in one pass, --sgd) against fp64 math
and against torch.optim.SGD itself.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from optimizer_arenas import DEV, Arenas, g

pytestmark = pytest.mark.gpu


def ref_step(p, gr, buf, lr, max_norm, momentum, wd, grad_div):
    """The issue's formula in fp64: g' = g grad_div; coef = min(max_norm / (||g'|| + 1e-6), 1); d = g' coef + wd p; buf = m buf + d;
    p -= lr buf."""
    gq = gr * grad_div
    norm = float(gq.norm())
    coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
    d = gq * coef + wd * p
    buf = momentum * buf + d
    return p - lr * buf, buf, norm


# n not a multiple of 4 (scalar tail), both lr forms; clip active (norm ~ 0.05 sqrt(n) >> 0.1), inactive (max_norm 1e6) and off (<= 0);
# grad_div 1 / 0.25; weight decay on.  4194307 > 2048 blocks x 256 lanes x 4 floats: the grid-stride loop runs twice and the scalar tail follows it
@pytest.mark.parametrize("n", [7, 1030, 262147, 4194307])
@pytest.mark.parametrize("lr_form", ["table", "two"])
@pytest.mark.parametrize("max_norm", [0.1, 1e6, 0.0])
@pytest.mark.parametrize("grad_div", [1.0, 0.25])
def test_sgd_step_vs_fp64(n, lr_form, max_norm, grad_div):
    split = (n // 3) & ~3
    if lr_form == "table":
        tab = torch.where(torch.arange(n) % 5 == 0, torch.tensor(2e-2), torch.tensor(5e-2))
        a = Arenas(n, seed=n, lr_table=tab)
    else:
        a = Arenas(n, seed=n, lr0=5e-2, lr1=2e-2, split=split)
    a.buf.copy_((torch.randn(n, generator=g(n + 2)) * 0.01).to(DEV))      # a step with a live buffer (momentum term exercised)
    a.state[1] = 0.5                                                          # StepLR factor
    p0, g0, b0 = a.p.double().cpu(), a.g.double().cpu(), a.buf.double().cpu()
    a.step(max_norm, 0.9, 1e-2, grad_div)
    p1, b1, norm = ref_step(p0, g0, b0, a.base_lr() * 0.5, max_norm, 0.9, 1e-2, grad_div)
    # fp32 arithmetic of a handful of operations on O(1) values: ~1e-7 relative; the norm: a float sum of n squares
    np.testing.assert_allclose(a.buf.double().cpu().numpy(), b1.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(a.p.double().cpu().numpy(), p1.numpy(), rtol=1e-6, atol=1e-7)
    st = a.state.cpu().tolist()
    assert st[0] == 1.0 and st[1] == 0.5 and st[3] == 0.0
    assert abs(st[2] - norm) <= 1e-5 * norm


def test_five_steps_vs_torch_sgd():
    """Five successive steps with fresh gradients, the StepLR factor dropping to 0.1 after the 3rd, against torch.optim.SGD(momentum 0.9,
    weight decay) + clip_grad_norm_(0.1) in fp64 on the CPU over two parameter groups (the arena's [lr | lr_backbone] split)."""
    n, split = 4099, 2048
    a = Arenas(n, seed=5, lr0=0.1, lr1=0.05, split=split)
    w = torch.nn.Parameter(a.p.double().cpu())
    pa, pb = torch.nn.Parameter(w.data[:split].clone()), torch.nn.Parameter(w.data[split:].clone())
    opt = torch.optim.SGD([{"params": [pa], "lr": 0.1}, {"params": [pb], "lr": 0.05}], lr=0.1, momentum=0.9, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1)
    for s in range(5):
        if s == 3:
            sched.step()
            a.state[1] = 0.1
        gr = torch.randn(n, generator=g(100 + s)) * (0.02 if s % 2 else 0.3)      # clip active on even steps, inactive on odd ones
        a.g.copy_(gr.to(DEV))
        a.step(0.1, 0.9, 1e-4)
        pa.grad, pb.grad = gr[:split].double().clone(), gr[split:].double().clone()
        tn = torch.nn.utils.clip_grad_norm_([pa, pb], 0.1)
        opt.step()
        assert abs(float(a.state[2]) - float(tn)) <= 1e-5 * float(tn)
        ref_p = torch.cat([pa.detach(), pb.detach()])
        ref_b = torch.cat([opt.state[pa]["momentum_buffer"], opt.state[pb]["momentum_buffer"]])
        np.testing.assert_allclose(a.buf.double().cpu().numpy(), ref_b.numpy(), rtol=1e-5, atol=1e-8, err_msg=f"buf, step {s}")
        np.testing.assert_allclose(a.p.double().cpu().numpy(), ref_p.numpy(), rtol=1e-6, atol=1e-8, err_msg=f"p, step {s}")
    assert float(a.state[0]) == 5.0


def nonfinite_skip(bad, n, where):
    a = Arenas(n, seed=9, lr0=0.1, lr1=0.01, split=512)
    a.step(0.1, 0.9, 1e-4)                      # one real step first: a live buffer
    p0, b0 = a.p.clone(), a.buf.clone()
    a.g[where] = bad                            # the skip must hold for every block, not just the one that reads it
    a.step(0.1, 0.9, 1e-4)
    assert torch.equal(a.p, p0) and torch.equal(a.buf, b0)
    st = a.state.cpu().tolist()
    assert st[0] == 1.0 and st[3] == 1.0 and not np.isfinite(st[2])
    a.g[where] = 0.0
    a.step(0.1, 0.9, 1e-4)
    st = a.state.cpu().tolist()
    assert st[0] == 2.0 and st[3] == 1.0 and not torch.equal(a.p, p0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradient_skips_the_update(bad):
    """A NaN / Inf gradient: p and buf bit-unchanged, the step count unchanged, the skip latched in state[3]; the next finite step runs."""
    nonfinite_skip(bad, 1031, 1031 - 2)         # in the scalar tail


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradient_in_the_last_float4_of_the_grid_stride_case(bad):
    """The same with more elements than one pass of the grid covers (2048 blocks x 256 lanes x 4 floats): the value sits in the last float4,
    which the loop's second iteration reads."""
    n = 4194307
    nonfinite_skip(bad, n, (n & ~3) - 2)


def test_rejects_misaligned_arenas_and_odd_split():
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    a = Arenas(64, seed=1, lr0=0.1, lr1=0.1, split=32)
    rc = L.cdetr_sgd_step(a.p.data_ptr() + 4, a.g.data_ptr(), a.buf.data_ptr(), None, 0.1, 0.1, 32, 60, a.sumsq.data_ptr(), a.state.data_ptr(),
                          0.1, 0.9, 0.0, 1.0, _ffi.stream_ptr())
    assert rc < 0 and b"cdetr_sgd_step" in L.cdetr_last_error()
    rc = L.cdetr_sgd_step(a.p.data_ptr(), a.g.data_ptr(), a.buf.data_ptr(), None, 0.1, 0.1, 30, 64, a.sumsq.data_ptr(), a.state.data_ptr(),
                          0.1, 0.9, 0.0, 1.0, _ffi.stream_ptr())
    assert rc < 0 and b"lr_split" in L.cdetr_last_error()
