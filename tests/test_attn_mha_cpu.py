"""attention_type "nn.MultiheadAttention" without a GPU: the model builds with exactly the reference variant's state dict
(tests/golden/g13_attn_mha.npz), loads it strictly, stage 1 refuses the variant, and the C ABI of cdetr_attn_* matches its ctypes twin."""
import pytest
import torch

import abi_header


def _variant_args(**kw):
    from counting_detr_amd.args import default_args
    args = default_args(device="cpu", **kw)
    args.attention_type = "nn.MultiheadAttention"
    return args


def test_state_dict_keys_and_shapes_are_the_reference_variants(golden):
    import counting_detr_amd
    z = golden("g13_attn_mha.npz")
    want = dict(zip((str(k) for k in z["state_dict_keys"]), (str(s) for s in z["state_dict_shapes"])))
    model, _, _ = counting_detr_amd.build_model(_variant_args())
    got = {k: ",".join(str(s) for s in v.shape) for k, v in model.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert got["transformer.encoder_layers.0.self_attn.in_proj_weight"] == "768,256"
    assert got["transformer.decoder_layers.5.cross_attn.in_proj_bias"] == "768"


def test_reference_layout_state_dict_loads_strictly():
    import counting_detr_amd
    from oracle.weights import seeded_state_dict
    from tools.gen_golden_attn_mha import attn_mha_schema
    sd = seeded_state_dict(attn_mha_schema(), heads="wide")
    model, _, _ = counting_detr_amd.build_model(_variant_args())
    model.load_state_dict(sd, strict=True)
    k = "transformer.decoder_layers.2.cross_attn.in_proj_weight"
    assert torch.equal(model.state_dict()[k], sd[k])
    # an RCDA-layout checkpoint does not fit the variant (and vice versa): [5E,E] vs [3E,E] input projections
    from oracle.weights import model_schema
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(seeded_state_dict(model_schema()), strict=True)


def test_variant_leaves_adapt_pos1d_out_of_the_loss():
    import counting_detr_amd
    from counting_detr_amd.engine import model_unused_prefixes
    model, _, _ = counting_detr_amd.build_model(_variant_args())
    assert model_unused_prefixes(model) == ("transformer.adapt_pos1d.",)
    from counting_detr_amd.args import default_args
    rcda, _, _ = counting_detr_amd.build_model(default_args(device="cpu"))
    assert model_unused_prefixes(rcda) == ()


def test_stage1_refuses_the_variant():
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    args = get_args_parser_stage1().parse_args(["--attention_type", "nn.MultiheadAttention", "--device", "cpu"])
    with pytest.raises(NotImplementedError, match="RCDA"):
        stage1.build(args)


def test_attn_desc_struct_matches_header():
    from counting_detr_amd import _ffi
    ctypes_of = {"int64_t": "c_long", "int32_t": "c_int", "float": "c_float"}
    fields = [(name, "c_void_p" if ptr else ctypes_of[base]) for name, base, ptr in abi_header.struct_fields("cdetr_attn_desc")]
    twin = [(n, t.__name__) for n, t in _ffi.AttnDesc._fields_]
    assert twin == fields
    assert "cdetr_attn_fwd" in _ffi.EXPORTS and "cdetr_attn_bwd" in _ffi.EXPORTS


def test_attn_entry_points_validate_before_launching():
    import ctypes
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    d = _ffi.AttnDesc()
    for fn in (L.cdetr_attn_fwd, L.cdetr_attn_bwd):
        assert fn(ctypes.byref(d), None) < 0 and b"cdetr_attn" in L.cdetr_last_error()
    d.q, d.k, d.v, d.o, d.lse = 16, 16, 16, 16, 16          # never dereferenced: the row strides are rejected first
    d.N, d.Lq, d.Lk, d.nh, d.precision = 1, 4, 4, 8, 1
    d.ldq, d.ldk, d.ldv = 256, 255, 256
    assert L.cdetr_attn_fwd(ctypes.byref(d), None) < 0 and b"row strides" in L.cdetr_last_error()
    d.ldk, d.precision = 256, 2
    assert L.cdetr_attn_fwd(ctypes.byref(d), None) < 0 and b"precision" in L.cdetr_last_error()


def test_attention_type_is_checked():
    from counting_detr_amd.transformer import Transformer
    with pytest.raises(ValueError, match="attention_type"):
        Transformer(attention_type="linear")
