"""fp64 torch restatements of the ragged (per-image valid length) stage-1 operators, shared by the ragged tests.  No GPU needed.

  * masked_self_attention: softmax(q k^T / sqrt(32)) v per head over the first lens[n] rows of image n, with its gradients; rows at and
    beyond lens[n] are absent on the query and the key side (outputs and gradients 0).
  * criterion_closed_form: the BoundingBoxCriterion over the concatenation of every image's first lens[b] pairs, evaluated in float64
    from the fp32 corner coordinates, with the gradients scattered back to [B, N, 2] (zeros in padded rows)."""
import numpy as np
import torch


def masked_self_attention(qk, v, go, lens, nh=8):
    """qk [N,L,2E] (q | k), v [N,L,E], go [N,L,E] (upstream gradient), lens: N ints.  Returns float64 (o, d_qk, d_v) of the full padded
    shapes.  Padded rows of the inputs are never touched (they may hold NaN)."""
    N, L, E2 = qk.shape
    E = E2 // 2
    d = E // nh
    o = torch.zeros(N, L, E, dtype=torch.float64)
    d_qk = torch.zeros(N, L, E2, dtype=torch.float64)
    d_v = torch.zeros(N, L, E, dtype=torch.float64)
    for n, ln in enumerate(int(x) for x in lens):
        if ln == 0:
            continue
        qk64 = qk[n, :ln].detach().double().cpu().requires_grad_(True)
        v64 = v[n, :ln].detach().double().cpu().requires_grad_(True)
        hs = lambda t: t.reshape(ln, nh, d).permute(1, 0, 2)      # noqa: E731
        a = ((hs(qk64[:, :E]) * d ** -0.5) @ hs(qk64[:, E:]).transpose(-1, -2)).softmax(-1)
        on = (a @ hs(v64)).permute(1, 0, 2).reshape(ln, E)
        on.backward(go[n, :ln].detach().double().cpu())
        o[n, :ln], d_qk[n, :ln], d_v[n, :ln] = on.detach(), qk64.grad, v64.grad
    return o, d_qk, d_v


def valid_rows(lens, N):
    """bool [B, N]: row n of image b is a pair."""
    return torch.arange(N)[None, :] < torch.as_tensor([int(x) for x in lens])[:, None]


def criterion_closed_form(coord, pts, tw, lens):
    """(loss_wh, loss_giou, d loss_wh / d wh [B,N,2], d loss_giou / d wh [B,N,2]) in float64 over the valid pairs: M = sum(lens),
    loss_wh the mean over 2M elements, loss_giou = sum(1 - GIoU) / M.  M == 0 gives zeros."""
    from counting_detr_amd import box_ops
    B, N = coord.shape[:2]
    valid = valid_rows(lens, N).reshape(-1)
    g_wh, g_gi = np.zeros((B * N, 2)), np.zeros((B * N, 2))
    M = int(valid.sum())
    if M == 0:
        return 0.0, 0.0, g_wh.reshape(B, N, 2), g_gi.reshape(B, N, 2)
    pw32 = coord[..., 2:].reshape(-1, 2).float().cpu()[valid]
    p32, t32 = pts.reshape(-1, 2).float().cpu()[valid], tw.reshape(-1, 2).float().cpu()[valid]
    src32 = box_ops.box_cxcywh_to_xyxy(torch.cat([p32, pw32], -1))
    tgt32 = box_ops.box_cxcywh_to_xyxy(torch.cat([p32, t32], -1))
    w = pw32.double().requires_grad_(True)
    dw = w - w.detach()                                               # value 0, derivative 1: x1 = cx - w/2 -> d x1 / d w = -1/2
    src = src32.double() + torch.stack([-0.5 * dw[:, 0], -0.5 * dw[:, 1], 0.5 * dw[:, 0], 0.5 * dw[:, 1]], -1)
    giou = box_ops.generalized_box_iou_pairs(src, tgt32.double())
    l_giou = (1 - giou).sum() / M
    g, = torch.autograd.grad(l_giou, w)
    d = pw32.double() - t32.double()
    g_wh[valid.numpy()] = (torch.sign(d) / (2 * M)).numpy()
    g_gi[valid.numpy()] = g.numpy()
    return float(d.abs().mean()), float(l_giou.detach()), g_wh.reshape(B, N, 2), g_gi.reshape(B, N, 2)
