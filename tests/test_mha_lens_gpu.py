"""cdetr_mha_fwd_lens / cdetr_mha_bwd_lens (ops.mha_fwd_raw / mha_bwd_raw with lens): the decoder self-attention with a per-image valid
length read from device memory.  Against fp64 per-image attention on the unpadded rows with NaN in every padded row of qk, v and d_o;
exact zeros in the padded rows of every output; bit equality with cdetr_mha_fwd / _bwd at lens == L; run-to-run bit equality.  Sizes:
lengths 0, 1, inside a 64-key tile, on and one past its boundary, a full image beside a nearly empty one.  Needs an MI355X."""
import pytest
import torch

from ragged_ref import masked_self_attention
from test_attn_kernels_gpu import BARS, MODES, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH, E = 8, 256
CASES = [(3, 70, [70, 1, 37]), (3, 130, [64, 65, 130]), (2, 5, [0, 5]), (2, 300, [300, 3])]
IDS = ["fp32", "bf16x3", "bf16-bwd"]


def g(seed):
    return torch.Generator().manual_seed(seed)


def inputs(N, L, lens, seed, poison=True):
    qk = torch.randn(N, L, 2 * E, generator=g(seed))
    v = torch.randn(N, L, E, generator=g(seed + 1))
    go = torch.randn(N, L, E, generator=g(seed + 2))
    if poison:
        for n, ln in enumerate(lens):
            qk[n, ln:], v[n, ln:], go[n, ln:] = float("nan"), float("nan"), float("nan")
    return qk, v, go


def launch(qk, v, go, lens, mode):
    """(o, lse, d_qk, d_v) through the raw wrappers in the arithmetic `mode` = (forward code, backward code); lens None = the dense
    entry points."""
    from counting_detr_amd import ops
    qk, v, go = qk.to(DEV), v.to(DEV), go.to(DEV)
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    old = (ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16)
    ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = mode[0], 3, mode[1] == 3
    try:
        o, lse = ops.mha_fwd_raw(qk, v, NH, ln)
        d_qk, d_v = ops.mha_bwd_raw(qk, v, o, go, lse, NH, ln)
    finally:
        ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = old
    torch.cuda.synchronize()
    return o, lse, d_qk, d_v


@pytest.fixture(scope="module")
def refs():
    """The fp64 results of every case, computed once and shared by the three arithmetic modes."""
    out = {}
    for i, (N, L, lens) in enumerate(CASES):
        out[i] = masked_self_attention(*inputs(N, L, lens, seed=10 * i), lens, NH)
    return out


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"N{n}xL{l}" for n, l, _ in CASES])
def test_against_fp64_with_nan_padding(case, mode, refs):
    N, L, lens = CASES[case]
    o, lse, d_qk, d_v = launch(*inputs(N, L, lens, seed=10 * case), lens, mode)
    r_o, r_dqk, r_dv = refs[case]
    for t in (o, lse, d_qk, d_v):
        assert torch.isfinite(t).all()
    bo, bg = BARS[mode[1]]
    close(o, r_o, bo, "o")
    close(d_qk[..., :E], r_dqk[..., :E], bg, "dq", floor=1.0)       # (a length of 1: dq = dk = 0 exactly)
    close(d_qk[..., E:], r_dqk[..., E:], bg, "dk", floor=1.0)
    close(d_v, r_dv, bg, "dv", floor=1.0)
    for n, ln in enumerate(lens):                                   # padding: exact zeros, written (the outputs start as torch.empty)
        assert float(o[n, ln:].abs().sum()) == 0.0 and float(lse[n, :, ln:].abs().sum()) == 0.0
        assert float(d_qk[n, ln:].abs().sum()) == 0.0 and float(d_v[n, ln:].abs().sum()) == 0.0
        assert not torch.signbit(o[n, ln:]).any()


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("L", [37, 300])
def test_full_lengths_equal_the_dense_entry_points_bitwise(L, mode):
    N = 2
    qk, v, go = inputs(N, L, [L] * N, seed=7, poison=False)
    dense = launch(qk, v, go, None, mode)
    ragged = launch(qk, v, go, [L] * N, mode)
    for a, b in zip(dense, ragged):
        assert torch.equal(a, b)


def test_repeated_launches_are_bit_identical():
    N, L, lens = CASES[1]
    a = launch(*inputs(N, L, lens, seed=3), lens, (1, 3))
    b = launch(*inputs(N, L, lens, seed=3), lens, (1, 3))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_lens_must_be_a_device_int32_tensor():
    from counting_detr_amd import ops
    qk, v, _ = inputs(2, 5, [5, 5], seed=1, poison=False)
    with pytest.raises(ValueError, match="int32"):
        ops.mha_fwd_raw(qk.to(DEV), v.to(DEV), NH, torch.tensor([5, 5], device=DEV))        # int64
    with pytest.raises(ValueError, match="int32"):
        ops.mha_fwd_raw(qk.to(DEV), v.to(DEV), NH, torch.tensor([5, 5], dtype=torch.int32))   # host
