"""cdetr_attn_fwd / _bwd (ops.attn_core) and cdetr_mha_fwd_lens / _bwd_lens (ops.mha_fwd_raw / mha_bwd_raw) against fp64 at the cases of
tests/attn_edges_ref.py: near-one-hot rows, and logit offsets of +120 that run up or down over the key index or sit on one half of
the keys -- the flash kernels' running maximum then jumps by more than fp32 exp can represent (the rescale factor is exactly 0) and
one half of the key-split kernel's merge is negligible beside the other.  o, lse, dq, dk and dv are held to max(the BARS of
tests/test_attn_kernels_gpu.py, 4 x the CPU emulation's floor); repeated launches are bit-identical.  Needs an MI355X."""
import pytest
import torch

import attn_edges_ref as R
from test_attn_kernels_gpu import MODES

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH, E = R.NH, R.E
IDS = ["fp32", "bf16x3", "bf16-bwd"]
mode_param = pytest.mark.parametrize("mode", MODES, ids=IDS)


def hold(case, code, got, tag):
    ref, bars = R.attn_reference(case), R.attn_bars(case, code)
    failed = []
    for k in R.ATTN_OUT:
        assert torch.isfinite(got[k]).all(), f"{k} non-finite"
        err = R.rel_err(got[k].detach().cpu(), ref[k])
        floor, bar = bars[k]
        print(f"EDGE attn {case.id} {tag} {k}: floor {floor:.2e} bar {bar:.2e}{' (4 x floor)' if bar == 4 * floor else ''} measured {err:.2e}")
        if not err <= bar:
            failed.append(f"{k}: {err:.3e} > {bar:.3e}")
    assert not failed, "; ".join(failed)


def run_dense(case, mode):
    """dict(o, lse, dq, dk, dv) of ops.attn_core: packed (q | k halves of one tensor) or separate operands that are column slices of
    wider tensors (row stride E + 64), as in tests/test_attn_kernels_gpu.py."""
    from counting_detr_amd import ops
    inp = R.attn_inputs(case)
    N, Lq, Lk = case.N, case.Lq, case.Lk
    if case.layout == "packed":
        qk = torch.cat([inp["q"], inp["k"]], -1).to(DEV).requires_grad_(True)
    else:
        qw, kw = torch.randn(N, Lq, E + 64, generator=R.g(21)), torch.randn(N, Lk, E + 64, generator=R.g(22))
        qw[..., 32:32 + E], kw[..., 32:32 + E] = inp["q"], inp["k"]
        qw, kw = qw.to(DEV).requires_grad_(True), kw.to(DEV).requires_grad_(True)
    v = inp["v"].to(DEV).requires_grad_(True)
    old = (ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16)
    ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = mode[0], 3, mode[1] == 3
    try:
        o = ops.attn_core(qk, None, v, NH) if case.layout == "packed" else ops.attn_core(qw[..., 32:32 + E], kw[..., 32:32 + E], v, NH)
        lse = o.grad_fn.saved_tensors[4].clone()
        o.backward(inp["go"].to(DEV))
    finally:
        ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = old
    torch.cuda.synchronize()
    if case.layout == "packed":
        dq, dk = qk.grad[..., :E], qk.grad[..., E:]
    else:
        dq, dk = qw.grad[..., 32:32 + E], kw.grad[..., 32:32 + E]
        assert float(qw.grad[..., :32].abs().max()) == 0.0 and float(kw.grad[..., 32 + E:].abs().max()) == 0.0
    return dict(o=o.detach(), lse=lse, dq=dq, dk=dk, dv=v.grad)


@mode_param
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=[c.id for c in R.ATTN_CASES])
def test_attn_edges_vs_fp64(case, mode):
    got = run_dense(case, mode)
    hold(case, mode[1], got, IDS[MODES.index(mode)])
    again = run_dense(case, mode)
    for k in R.ATTN_OUT:
        assert torch.equal(got[k], again[k]), f"{k}: repeated launches differ"


def run_lens(case, mode):
    from counting_detr_amd import ops
    inp = R.attn_inputs(case)
    qk, v, go = torch.cat([inp["q"], inp["k"]], -1), inp["v"].clone(), inp["go"].clone()
    for n, ln in enumerate(case.lens):                                  # the padded rows are never read
        qk[n, ln:], v[n, ln:], go[n, ln:] = float("nan"), float("nan"), float("nan")
    qk, v, go = qk.to(DEV), v.to(DEV), go.to(DEV)
    lens = torch.tensor(case.lens, dtype=torch.int32, device=DEV)
    old = (ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16)
    ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = mode[0], 3, mode[1] == 3
    try:
        o, lse = ops.mha_fwd_raw(qk, v, NH, lens)
        d_qk, d_v = ops.mha_bwd_raw(qk, v, o, go, lse, NH, lens)
    finally:
        ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = old
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=d_qk[..., :E], dk=d_qk[..., E:], dv=d_v)


@mode_param
@pytest.mark.parametrize("case", R.ATTN_LENS_CASES, ids=[c.id for c in R.ATTN_LENS_CASES])
def test_mha_lens_edges_vs_fp64_with_nan_padding(case, mode):
    got = run_lens(case, mode)
    hold(case, mode[1], got, IDS[MODES.index(mode)])
    for n, ln in enumerate(case.lens):                                  # padding: exact zeros, written (the outputs start as torch.empty)
        assert float(got["o"][n, ln:].abs().sum()) == 0.0 and float(got["lse"][n, :, ln:].abs().sum()) == 0.0
        assert float(got["dq"][n, ln:].abs().sum()) == 0.0 and float(got["dk"][n, ln:].abs().sum()) == 0.0
        assert float(got["dv"][n, ln:].abs().sum()) == 0.0
        assert not torch.signbit(got["o"][n, ln:]).any()
    again = run_lens(case, mode)
    for k in R.ATTN_OUT:
        assert torch.equal(got[k], again[k]), f"{k}: repeated launches differ"
