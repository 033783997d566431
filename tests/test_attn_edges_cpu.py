"""The edge cases of tests/attn_edges_ref.py are sound before any kernel sees them (no GPU): the fp64 references are finite and agree
with autograd through the closed forms the existing tests use; every (image, axis) keeps a valid key; four times the arithmetic floor
stays under a cap, so that no bar derived from it goes vacuous; every RCDA mask case tells the wrong mask handlings from the right
one by more than ten times its output bar; the peaked cases are near-one-hot and the offset cases have logits exp cannot take."""
import math

import pytest
import torch

import attn_edges_ref as R
from ragged_ref import masked_self_attention

CAP = {0: 1e-3, 1: 1e-3, 3: 5e-2}       # on 4 x floor
rcda_param = pytest.mark.parametrize("case", R.RCDA_CASES, ids=[c.id for c in R.RCDA_CASES])
ALL_ATTN = R.ATTN_CASES + R.ATTN_LENS_CASES
attn_param = pytest.mark.parametrize("case", ALL_ATTN, ids=[c.id for c in ALL_ATTN])


def test_case_tables_cover_what_they_claim():
    ids = [c.id for c in R.RCDA_CASES] + [c.id for c in ALL_ATTN]
    assert len(set(ids)) == len(ids)
    for hw in ((50, 84), (84, 50), (128, 96)):
        assert {c.pattern for c in R.RCDA_CASES if (c.H, c.W) == hw} == {"pad", "both", "one", "holes", "bytes"}
    for c in R.RCDA_CASES:
        assert c.N == 2 and c.H <= 128
    masks = R.rcda_masks(R.RcdaCase(128, 96, 40, "bytes"))
    assert set(masks[0].unique().tolist()) == {0, 255} and set(masks[1].unique().tolist()) == {0, 2}


@rcda_param
def test_rcda_reference_health(case):
    inp, ref = R.rcda_inputs(case), R.rcda_reference(case)
    for k in R.RCDA_OUT + ("a_row", "a_col"):
        assert torch.isfinite(ref[k]).all(), k
    assert not bool(inp["mr"].bool().all(1).any()) and not bool(inp["mc"].bool().all(1).any())       # a valid key on every (image, axis)
    assert float(ref["a_row"][inp["mr"].bool()[:, None, None, :].expand_as(ref["a_row"])].abs().sum()) == 0.0
    assert float(ref["a_col"][inp["mc"].bool()[:, None, None, :].expand_as(ref["a_col"])].abs().sum()) == 0.0
    if case.pattern == "one":
        assert int(inp["mr"][1].eq(0).sum()) == 1 and int(inp["mc"][1].eq(0).sum()) == 1
    if case.L <= 300:          # the hand-written backward is autograd's through the closed form test_rcda_core compares with
        ins = [inp[k].double().requires_grad_(True) for k in ("qr", "qc", "kr", "kc", "v")]
        out = R.rcda_core_ref(*ins, inp["mr"], inp["mc"], R.NH)
        out.backward(inp["go"].double())
        assert R.rel_err(ref["out"], out.detach()) < 1e-12
        for name, t in zip(R.RCDA_OUT[1:], ins):
            assert R.rel_err(ref[name], t.grad) < 1e-11, name
    if case.logit == "peaked":
        top = torch.cat([ref["a_row"].amax(-1).flatten(), ref["a_col"].amax(-1).flatten()])
        print(f"\nPEAK {case.id}: median row maximum {float(top.median()):.3f}")
        assert float(top.median()) >= 0.8
    if case.logit == "offset":
        top = max(float(ref["s_row"].max()), float(ref["s_col"].max()))
        print(f"\nOFFSET {case.id}: largest logit {top:.1f}")
        assert top > 88.8


@rcda_param
def test_rcda_floor_cap_and_discrimination(case):
    for code in (0, 1, 3):
        bars = R.rcda_bars(case, code)
        print(f"\nFLOOR rcda {case.id} code {code}: " + " ".join(f"{k} {f:.1e}/{b:.1e}" for k, (f, b) in bars.items()))
        for k, (floor, b) in bars.items():
            assert math.isfinite(floor) and 4 * floor <= CAP[code], (code, k, floor)
            assert b >= R.rcda_existing_bars(code)[k]
    ref = R.rcda_reference(case)["out"]
    out_bar = max(R.rcda_bars(case, c)["out"][1] for c in (0, 1))
    mutants = R.rcda_mutants(case)
    assert mutants, "no mutant applies"
    for name, out in mutants.items():
        d = R.rel_err(out, ref)
        d = math.inf if not math.isfinite(d) else d
        print(f"MUTANT {case.id} {name}: differs by {d:.2e} (10 x bar = {10 * out_bar:.1e})")
        assert d > 10 * out_bar, name


@attn_param
def test_attn_reference_health_and_floor_cap(case):
    inp, ref = R.attn_inputs(case), R.attn_reference(case)
    for k in R.ATTN_OUT:
        assert torch.isfinite(ref[k]).all(), k
    # the hand-written backward against autograd through the formula of test_attn_kernels_gpu.reference / ragged_ref
    if case.lens is None:
        q, k, v = (inp[x].double().requires_grad_(True) for x in ("q", "k", "v"))
        a = ((R.heads(q) * 32 ** -0.5) @ R.heads(k).transpose(-1, -2)).softmax(-1)
        o = R.unheads(a @ R.heads(v))
        o.backward(inp["go"].double())
        want = dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    else:
        o, d_qk, d_v = masked_self_attention(torch.cat([inp["q"], inp["k"]], -1), inp["v"], inp["go"], case.lens, R.NH)
        want = dict(o=o, dq=d_qk[..., :R.E], dk=d_qk[..., R.E:], dv=d_v)
    for name, t in want.items():
        assert R.rel_err(ref[name], t) < 1e-11, name
    valid = torch.ones(case.N, case.Lq, dtype=torch.bool) if case.lens is None else torch.arange(case.Lq)[None] < torch.tensor(case.lens)[:, None]
    rows = ref["p"].amax(-1).permute(0, 2, 1)[valid]
    if case.pattern == "peaked":
        print(f"\nPEAK {case.id}: median row maximum {float(rows.median()):.3f}")
        assert float(rows.median()) >= 0.8
    elif R.attn_offset(case.pattern, case.Lk) == R.ATTN_OFFSET:          # (the two 33-key ramps end lower: attn_edges_ref.ATTN_OFFSET_LOWERED)
        assert float(ref["lse"].max()) > 88.8
    for code in (0, 1, 3):
        bars = R.attn_bars(case, code)
        print(f"\nFLOOR attn {case.id} code {code}: " + " ".join(f"{k} {f:.1e}/{b:.1e}" for k, (f, b) in bars.items()))
        for k, (floor, _) in bars.items():
            assert math.isfinite(floor) and 4 * floor <= CAP[code], (code, k, floor)


def test_offset_patterns_shift_the_logits_as_stated():
    """late-half at 160 keys: keys from 80 on carry +120 and the first half of every row is negligible (its probabilities underflow fp32);
    ramp-up: the offset of the last key is +120."""
    case = R.AttnCase(160, 160, "separate", "late-half")
    inp, ref = R.attn_inputs(case), R.attn_reference(case)
    base = R.logits(R.heads(inp["q"].double()), R.heads(inp["k"].double()), R.F64)
    assert float(base[..., 80:].min() - base[..., :80].max()) > 104          # exp(-104) is below the smallest fp32 subnormal
    assert float(ref["p"][..., :80].max()) < 1e-45
    off = R.key_offsets("ramp-up", 300)
    assert float(off[0]) == 0.0 and float(off[-1]) == R.ATTN_OFFSET and bool((off[1:] > off[:-1]).all())
