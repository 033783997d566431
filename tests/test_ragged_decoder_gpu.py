"""The decoder with a per-image query count (`lens`): ops.DecoderStackFn(..., lens) and the op-by-op TransformerDecoderLayer(..., lens=)
against the existing dense path run ONE IMAGE AT A TIME on the unpadded rows -- outputs of the valid rows, input gradients and every
parameter gradient (per-image gradients summed).  Built like test_hip_kernels.test_decoder_stack_fused_equals_unfused: 3 layers,
H x W = 9 x 14, random weights and inputs of unit scale.  Padded query rows hold finite junk (they run through the row-wise operators and
the cross-attention) and take no part in the loss.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, E = 9, 14, 256
CASES = [(3, 9, [9, 1, 5]), (3, 70, [70, 33, 64])]
# (forward code, backward code, output bar, gradient bar): test_decoder_stack_fused_equals_unfused's modes and bars
MODES = [(0, 1, 2e-5, 1e-4), (1, 1, 2e-5, 1e-4), (1, 3, 2e-5, 1.5e-2)]
NAMES = ("tgt", "qpos", "qx", "qy", "mem", "krm", "kcm")


def g(seed):
    return torch.Generator().manual_seed(seed)


def close(actual, ref, rtol, msg):
    """test_hip_kernels.close as that test calls it: err <= rtol * scale + 2e-5 * scale, scale = the reference's largest magnitude."""
    a, r = actual.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == r.shape, (a.shape, r.shape)
    assert torch.isfinite(a).all(), msg + " non-finite"
    scale = r.abs().max().item() + 1e-30
    err = (a - r).abs().max().item()
    assert err <= (rtol + 2e-5) * scale, f"{msg}: max err {err:.3e} vs scale {scale:.3e}"


def make(N, L):
    torch.manual_seed(3)
    from counting_detr_amd.transformer import TransformerDecoderLayer
    layers = [TransformerDecoderLayer(E, 1024, 8).to(DEV) for _ in range(3)]
    mk = lambda shape, seed: torch.randn(*shape, generator=g(seed))   # noqa: E731
    ins = [mk((N, L, E), 1), mk((N, L, E), 2), mk((N, L, E), 3), mk((N, L, E), 4), mk((N, H, W, E), 5), mk((N, W, E), 6), mk((N, H, E), 7)]
    mr = torch.zeros(N, W, dtype=torch.uint8); mr[1, W - 3:] = 1
    mc = torch.zeros(N, H, dtype=torch.uint8); mc[1, H - 2:] = 1
    gos = [torch.randn(N, L, E, generator=g(10 + i)) for i in range(3)]         # the loss: a random linear functional of the valid rows
    return layers, ins, mr.to(DEV), mc.to(DEV), gos


def param_grads(layers):
    return {f"{i}.{k}": p.grad.detach().double().cpu().clone() for i, layer in enumerate(layers) for k, p in layer.named_parameters()}


def yardstick(layers, ins, mr, mc, gos, lens):
    """The dense fused node, one image at a time on rows [:len]: valid outputs, input gradients (padded query rows 0), summed parameter
    gradients."""
    from counting_detr_amd import ops
    N, L = ins[0].shape[:2]
    outs = [torch.zeros(N, L, E, dtype=torch.float64) for _ in range(3)]
    gin = [torch.zeros(t.shape, dtype=torch.float64) for t in ins]
    gp = None
    for n, ln in enumerate(lens):
        for layer in layers:
            for p in layer.parameters():
                p.grad = None
        q = [t[n:n + 1, :ln].to(DEV).requires_grad_(True) for t in ins[:4]]
        m = [t[n:n + 1].to(DEV).requires_grad_(True) for t in ins[4:]]
        o = ops.DecoderStackFn.apply(*q, *m, mr[n:n + 1], mc[n:n + 1], layers, q[0])
        sum((o[i] * gos[i][n:n + 1, :ln].to(DEV)).sum() for i in range(3)).backward()
        for i in range(3):
            outs[i][n, :ln] = o[i][0].detach().double().cpu()
        for k in range(4):
            gin[k][n, :ln] = q[k].grad[0].double().cpu()
        for k in range(3):
            gin[4 + k][n] = m[k].grad[0].double().cpu()
        cur = param_grads(layers)
        gp = cur if gp is None else {k: gp[k] + cur[k] for k in gp}
    return outs, gin, gp


def ragged(layers, ins, mr, mc, gos, lens, fused):
    from counting_detr_amd import ops
    for layer in layers:
        for p in layer.parameters():
            p.grad = None
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    t = [x.to(DEV).requires_grad_(True) for x in ins]
    if fused:
        o = ops.DecoderStackFn.apply(*t, mr, mc, layers, t[0], None, None, ln)
    else:
        o, x = [], t[0]
        for layer in layers:
            x = layer(x, t[1], t[2], t[3], t[4], t[5], t[6], mr, mc, lens=ln)
            o.append(x)
    valid = (torch.arange(ins[0].shape[1])[None, :] < torch.tensor(lens)[:, None]).to(DEV)
    sum((o[i] * gos[i].to(DEV) * valid[..., None]).sum() for i in range(3)).backward()
    return [x.detach() for x in o], [x.grad for x in t], param_grads(layers), valid.cpu()


@pytest.mark.parametrize("mode", MODES, ids=["fp32mfma", "bf16x3", "bf16x3-bwd-bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"N{n}xL{l}" for n, l, _ in CASES])
def test_ragged_decoder_equals_per_image_dense(case, mode):
    from counting_detr_amd import ops
    N, L, lens = case
    layers, ins, mr, mc, gos = make(N, L)
    with ops.arithmetic(mode[0], mode[1]):
        ref_o, ref_gi, ref_gp = yardstick(layers, ins, mr, mc, gos, lens)
        for fused in (True, False):
            what = "fused" if fused else "op-by-op"
            o, gi, gp, valid = ragged(layers, ins, mr, mc, gos, lens, fused)
            for i in range(3):
                assert torch.isfinite(o[i]).all(), f"{what} layer {i}: padded rows must stay finite"
                close(o[i].cpu() * valid[..., None], ref_o[i], mode[2], f"{what} out {i}")
            for name, a, b in zip(NAMES, gi, ref_gi):
                close(a, b, mode[3], f"{what} d{name}")        # (padded query rows: zero on both sides)
            for k in ref_gp:
                close(gp[k], ref_gp[k], mode[3], f"{what} d{k}")
