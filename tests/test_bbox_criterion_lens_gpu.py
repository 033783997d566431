"""cdetr_bbox_criterion_lens_fwd / _bwd (ops.BBoxCriterionFn with counts): the fused 1st-stage criterion over a ragged batch, against the
fp64 closed form on the concatenated valid pairs and the fused = False composition with counts, with NaN in every padded row; bit
equality with the dense entry points at counts == N; all-zero counts; graph replays that follow a changed counts buffer.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from ragged_ref import criterion_closed_form, valid_rows
from test_stage1_criterion_gpu import W_GIOU, W_WH, close, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, LENS = 3, 7, [7, 1, 4]


def poisoned(seed=31, lens=LENS):
    coord, pts, tw = make_case(B, N, seed=seed)                       # exact ties in w, h and both among the pairs
    pad = ~valid_rows(lens, N)
    coord[pad], pts[pad], tw[pad] = float("nan"), float("nan"), float("nan")
    return coord, pts, tw


def counts_of(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def fused_grads(coord, pts, tw, counts):
    from counting_detr_amd import ops
    out = []
    for sel in (0, 1, 2):
        c = coord.to(DEV).clone().requires_grad_(True)
        vec = ops.BBoxCriterionFn.apply(c, pts.to(DEV), tw.to(DEV), W_WH, W_GIOU, counts)
        vec[sel].backward()
        out.append(c.grad.detach().cpu().numpy())
    return vec.detach().cpu().numpy(), out


def test_against_fp64_and_composition_with_nan_padding():
    from counting_detr_amd import stage1
    coord, pts, tw = poisoned()
    vec, (g_wh, g_giou, g_tot) = fused_grads(coord, pts, tw, counts_of(LENS))
    l_wh, l_gi, r_wh, r_gi = criterion_closed_form(coord, pts, tw, LENS)
    print("fused", vec, "fp64", l_wh, l_gi)
    assert np.isfinite(vec).all()
    np.testing.assert_allclose(vec[:2], [l_wh, l_gi], rtol=1e-6)
    pad = (~valid_rows(LENS, N)).numpy()
    for gr in (g_wh, g_giou, g_tot):
        assert np.all(gr[..., :2] == 0) and np.all(gr[pad] == 0)      # xy columns and padded rows: exact zeros
    close(g_wh[..., 2:], r_wh)
    close(g_giou[..., 2:], r_gi)
    c = coord.to(DEV).clone().requires_grad_(True)
    crit = stage1.BoundingBoxCriterion()
    ld, total = crit.forward_with_total({"pred_wh": c[..., 2:], "pred_boxes": c},
                                        {"points": pts.to(DEV), "whs": tw.to(DEV), "counts": counts_of(LENS)})
    total.backward()
    np.testing.assert_allclose(vec, [float(ld["loss_wh"].detach()), float(ld["loss_giou"].detach()), float(total.detach())], rtol=1e-6)
    close(g_tot, c.grad.cpu().numpy())
    got = stage1.BoundingBoxCriterion(fused=True)({"pred_wh": c[..., 2:], "pred_boxes": c},
                                                  {"points": pts.to(DEV), "whs": tw.to(DEV), "counts": counts_of(LENS)})
    assert float(got["loss_wh"]) == vec[0] and float(got["loss_giou"]) == vec[1]


@pytest.mark.parametrize("shape", [(3, 7), (4, 225)], ids=["3x7", "4x225"])
def test_full_counts_equal_the_dense_entry_points_bitwise(shape):
    from counting_detr_amd import ops
    b, n = shape
    coord, pts, tw = make_case(b, n, seed=5)
    res = []
    for counts in (None, torch.full((b,), n, dtype=torch.int32, device=DEV)):
        c = coord.to(DEV).clone().requires_grad_(True)
        vec = ops.BBoxCriterionFn.apply(c, pts.to(DEV), tw.to(DEV), W_WH, W_GIOU, counts)
        vec[2].backward()
        res.append((vec.detach(), c.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_all_zero_counts_give_zeros():
    coord, pts, tw = poisoned(lens=[0, 0, 0])
    vec, grads = fused_grads(coord, pts, tw, counts_of([0, 0, 0]))
    assert np.all(vec == 0)
    for gr in grads:
        assert np.all(gr == 0)


def test_graph_replays_follow_the_counts_buffer():
    from counting_detr_amd import ops
    coord, pts, tw = make_case(B, N, seed=21)
    c = coord.to(DEV).clone().requires_grad_(True)
    sp, st, counts = pts.to(DEV), tw.to(DEV), counts_of(LENS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                        # warm-up outside the capture
        ops.BBoxCriterionFn.apply(c, sp, st, W_WH, W_GIOU, counts)[2].backward()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    c.grad = None
    with torch.cuda.graph(graph):
        vec = ops.BBoxCriterionFn.apply(c, sp, st, W_WH, W_GIOU, counts)
        vec[2].backward()
        grad = c.grad
    seen = []
    for lens in ([2, 7, 3], [7, 7, 7], [1, 0, 0]):
        counts.copy_(counts_of(lens))
        graph.replay()
        torch.cuda.synchronize()
        e_vec, (_, _, e_tot) = fused_grads(coord, pts, tw, counts_of(lens))
        assert np.array_equal(vec.detach().cpu().numpy(), e_vec)
        assert np.array_equal(grad.detach().cpu().numpy(), e_tot)
        l_wh, l_gi, _, _ = criterion_closed_form(coord, pts, tw, lens)
        np.testing.assert_allclose(e_vec[:2], [l_wh, l_gi], rtol=1e-6)
        seen.append(float(e_vec[2]))
    assert len(set(seen)) == 3                                        # the three counts really give three different losses
