"""cdetr_rcda_fwd / cdetr_rcda_bwd (through ops.rcda_core and ops.rcda_fwd_raw / rcda_bwd_raw) against fp64 at the cases of
tests/attn_edges_ref.py: key-padding masks on the second image that fill whole 32-key tiles, cross key 64, start at key 0, leave one
key, or are single holes, with k and v multiplied by 1e3 at every masked key; near-one-hot rows (queries x 8) and logits around +100.
Each tensor is held to max(the bar test_rcda_core holds it to, 4 x the CPU emulation's floor); on top of that max-scaled metric the
saved maps, the key gradients and dV must be EXACTLY zero at masked keys and in the padded columns.  Needs an MI355X."""
import contextlib

import pytest
import torch

import attn_edges_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH = R.NH
# (ops.PRECISION, ops.PRECISION_BWD, arithmetic code of the gradients); the output's code is the forward's
MODES = [(0, 1, 0), (1, 1, 1), (1, 3, 3)]
IDS = ["fp32", "bf16x3", "bf16-bwd"]
case_param = pytest.mark.parametrize("case", R.RCDA_CASES, ids=[c.id for c in R.RCDA_CASES])
mode_param = pytest.mark.parametrize("mode", MODES, ids=IDS)


@contextlib.contextmanager
def arithmetic(precision, bwd):
    from counting_detr_amd import ops
    old = (ops.PRECISION, ops.PRECISION_BWD)
    ops.PRECISION, ops.PRECISION_BWD = precision, bwd
    try:
        yield ops
    finally:
        ops.PRECISION, ops.PRECISION_BWD = old


def device_args(case):
    inp = R.rcda_inputs(case)
    return [inp[k].to(DEV) for k in ("qr", "qc", "kr", "kc", "v")], inp["mr"].to(DEV), inp["mc"].to(DEV), inp["go"].to(DEV)


def hold(case, code, got, names, tag):
    """Every tensor finite and within its bar of the fp64 reference; prints floor, bar and measured error first."""
    ref, bars = R.rcda_reference(case), R.rcda_bars(case, code)
    failed = []
    for k in names:
        assert torch.isfinite(got[k]).all(), f"{k} non-finite"
        err = R.rel_err(got[k].detach().cpu(), ref[k])
        floor, bar = bars[k]
        print(f"EDGE rcda {case.id} {tag} {k}: floor {floor:.2e} bar {bar:.2e}{' (4 x floor)' if bar == 4 * floor else ''} measured {err:.2e}")
        if not err <= bar:
            failed.append(f"{k}: {err:.3e} > {bar:.3e}")
    assert not failed, "; ".join(failed)


def check_maps(case, a_row, a_col):
    """The saved softmaxes: exact zeros at masked keys and in the padded columns, rows that sum to 1, exactly 1.0 on a lone valid key."""
    inp = R.rcda_inputs(case)
    for a, m, n in ((a_row, inp["mr"], case.W), (a_col, inp["mc"], case.H)):
        a = a.cpu()
        assert torch.isfinite(a).all()
        assert float(a[..., n:].abs().sum()) == 0.0, "padded columns"
        dead = m.bool()[:, None, None, :].expand(a.shape[:3] + (n,))
        assert float(a[..., :n][dead].abs().sum()) == 0.0, "masked keys"
        assert float((a.double().sum(-1) - 1).abs().max()) <= 1e-5
        if case.pattern == "one":
            key = int(m[1].eq(0).nonzero())
            assert bool((a[1, :, :, key] == 1.0).all())


@mode_param
@case_param
def test_rcda_edges_vs_fp64(case, mode):
    precision, bwd, code = mode
    args, mr, mc, go = device_args(case)
    inp = R.rcda_inputs(case)
    ins = [t.requires_grad_(True) for t in args]
    with arithmetic(precision, bwd) as ops:
        out = ops.rcda_core(*ins, mr, mc, NH)
        out.backward(go)
        out_raw, a_row, a_col = ops.rcda_fwd_raw(*[t.detach() for t in ins], mr, mc, NH)
    torch.cuda.synchronize()
    assert torch.equal(out_raw, out)
    got = dict(zip(R.RCDA_OUT, [out] + [t.grad for t in ins]))
    hold(case, code, got, R.RCDA_OUT, IDS[MODES.index(mode)])
    check_maps(case, a_row, a_col)
    dead_w, dead_h = inp["mr"].bool(), inp["mc"].bool()
    dk_row, dk_col, dv = got["dk_row"].cpu(), got["dk_col"].cpu(), got["dv"].cpu()
    assert float(dk_row[dead_w].abs().max()) == 0.0 and float(dk_col[dead_h].abs().max()) == 0.0
    assert float(dv[dead_h[:, :, None] | dead_w[:, None, :]].abs().max()) == 0.0


@pytest.mark.parametrize("slices", [None, 6], ids=["default-slices", "6-slices"])
def test_sliced_forward_with_fully_masked_slices(slices, monkeypatch):
    """50 x 50 keys, image 1 valid on rows 0..8 only: of the default five key-row slices (10 rows each) four hold nothing but masked rows
    (six slices: rows 0..8 are exactly slice 0).  Saved maps bit for bit those of the unsliced launch, outputs within the 1e-5 bar of
    test_rcda_forward_key_row_slices, arrival counters left zero."""
    from counting_detr_amd import ops
    case = R.RcdaCase(50, 50, 300, "pad")
    args, mr, mc, _ = device_args(case)
    monkeypatch.setattr(ops, "PRECISION", 1)
    monkeypatch.setattr(ops, "RCDA_SLICES", False)
    o1, ar1, ac1 = ops.rcda_fwd_raw(*args, mr, mc, NH)
    monkeypatch.setattr(ops, "RCDA_SLICES", True)
    if slices is None:
        monkeypatch.delenv("CDETR_RCDA_HS", raising=False)
    else:
        monkeypatch.setenv("CDETR_RCDA_HS", str(slices))
    o2, ar2, ac2 = ops.rcda_fwd_raw(*args, mr, mc, NH)
    o3, _, _ = ops.rcda_fwd_raw(*args, mr, mc, NH)
    torch.cuda.synchronize()
    assert torch.equal(ar1, ar2) and torch.equal(ac1, ac2)
    assert torch.equal(o2, o3)
    assert int(ops.splitk_ws()[:4096].abs().sum()) == 0
    assert R.rel_err(o2.cpu(), o1.cpu()) <= 1e-5 + 1e-6
    check_maps(case, ar2, ac2)
    hold(case, 1, dict(out=o1), ("out",), "unsliced")
    hold(case, 1, dict(out=o2), ("out",), f"sliced-{slices}")


@pytest.mark.parametrize("fuse_dq,fuse_dk", [(False, False), (True, False), (True, True)], ids=["unfused", "dq-fused", "dq-dk-fused"])
def test_backward_fusion_levels_vs_fp64_under_masks(fuse_dq, fuse_dk, monkeypatch):
    """The three fusion levels of test_rcda_backward_fusion_levels_agree, each held to fp64 at 50 x 84 keys with image 1 masked from
    (9, 33) on: the unfused paths contract over Wp and Hp, padded columns included, and rely on the saved maps' zeros there."""
    from counting_detr_amd import ops
    case = R.RcdaCase(50, 84, 77, "pad")
    args, mr, mc, go = device_args(case)
    inp = R.rcda_inputs(case)
    with arithmetic(1, 1):
        _, a_row, a_col = ops.rcda_fwd_raw(*args, mr, mc, NH)
        monkeypatch.setattr(ops, "FUSE_RCDA_DQ", fuse_dq)
        monkeypatch.setattr(ops, "FUSE_RCDA_DK", fuse_dk)
        grads = ops.rcda_bwd_raw(go, *args, a_row, a_col, NH)
    torch.cuda.synchronize()
    got = dict(zip(R.RCDA_OUT[1:], grads))
    hold(case, 1, got, R.RCDA_OUT[1:], f"fuse_dq={int(fuse_dq)},fuse_dk={int(fuse_dk)}")
    dead_w, dead_h = inp["mr"].bool(), inp["mc"].bool()
    assert float(got["dk_row"].cpu()[dead_w].abs().max()) == 0.0 and float(got["dk_col"].cpu()[dead_h].abs().max()) == 0.0
    assert float(got["dv"].cpu()[dead_h[:, :, None] | dead_w[:, None, :]].abs().max()) == 0.0
